"""The reference of every `Engine` comparison (test infrastructure): the oracle's `Game` (MctsGame) driven as the reference's
`InteractivePlay` drives it (rust/src/interactive_play.rs), for P games in lock-step.  The oracle is used as it stands.

  search            bg_thread_tick until bg_thread_should_stop (interactive_play.rs:188-220): root visits >= the target, or a terminal
                    root.  Rounds are the device's: one simulation per active game, and a second one in the same round when the leaf
                    just selected is terminal (it needs no evaluator row) -- which changes no tree, only where a search stands after k
                    rounds (T4 looks there).
  make_moves        State::make_move (interactive_play.rs:169-176) -> MctsGame::make_move (mcts.rs:187-206).  What the reference answers
                    with `false` or a panic is a refusal code, and the game is not touched (the oracle's own make_move would set its
                    sticky error): 1 terminal root, 2 column outside 0..6 or full, 3 the root has no children yet (mcts.rs:196 panics;
                    a non-terminal node has children exactly when it has a visit), 4 a sampled column that is not legal.
  make_random_moves State::make_random_move (interactive_play.rs:178-185) -> the oracle's c4o_game_make_random_move, once the column it
                    will sample (c4o_sample_move on the same policy, seed and temperature) is known to be legal.
  snapshot          root position, root_policy, root q values, visit count, moves made, status (1 active / 64 parked).
  result            to_result (mcts.rs:271-313) of every game whose root is terminal.

`run_script` is the move script of the scripted-games test, written against the interface `c4a0_amd.engine.Engine` and `RefEngine`
share, so that the CPU test can hold the script itself to its floors (games finished, refusals of each kind, moves under a pending
leaf) on the oracle alone."""
from __future__ import annotations

import numpy as np

from tests.helpers import START_EVALS, start_job
from tests.search_ref import C_PLY_PENALTY, oracle_evaluator   # noqa: F401  (re-exported)

ACTIVE, PARKED = 1, 64
OK, REFUSED_TERMINAL, REFUSED_COLUMN, REFUSED_UNSEARCHED, REFUSED_SAMPLE = 0, 1, 2, 3, 4
MOVE_NONE = -1
RECORD_DTYPE = np.dtype([("game_id", "<u8"), ("mask", "<u8"), ("value", "<u8"), ("policy", "<f4", (7,)),
                         ("q_penalty", "<f4"), ("q_no_penalty", "<f4"), ("meta", "<u4")])


class RefSnapshot:
    def __init__(self, records, visits, status, terminal):
        self.records, self.visits, self.status, self.terminal = records, visits, status, terminal
        self.n_moves = (records["meta"] & 0xFFFF).astype(np.int64)


class RefEngine:
    def __init__(self, evaluator, max_mcts_iterations, c_exploration, c_ply_penalty=C_PLY_PENALTY, *, positions, game_ids=None):
        from oracle import c4oracle as O

        self.O = O
        self.ev, self.c, self.cp = evaluator, float(c_exploration), float(c_ply_penalty)
        self.max, self.target = int(max_mcts_iterations), int(max_mcts_iterations)
        self.ids = [int(i) for i in (range(len(positions)) if game_ids is None else game_ids)]
        self.games = [O.Game(O.Pos(int(m), int(v)), gid) for (m, v), gid in zip(positions, self.ids)]
        self.n_games = len(self.games)
        self.status = [None] * self.n_games
        self.last_results = np.zeros(self.n_games, dtype=np.int32)
        self.rounds = 0
        self.retained = []          # (visits the new root kept, visits the old root had) of every accepted move
        self.moves_under_pending_leaf = 0
        for i in range(self.n_games):
            self._resume(i)

    # ------------------------------------------------------------------ state
    def _terminal(self, i):
        return self.O.terminal_state(self.games[i].root_pos()) != 0

    def _resume(self, i, moved=False):
        """ensure_bg_thread (interactive_play.rs:110-113): park at the target or at a terminal root, else search on.  The device
        selects the game's leaf here (the oracle has selected it already: the same tree gives the same leaf) -- unless the game is
        searching already and was not moved -- and a terminal leaf's simulation runs at once, as in any round."""
        g = self.games[i]
        if self._terminal(i) or g.root_visit_count() >= self.target:
            self.status[i] = PARKED
        elif self.status[i] != ACTIVE or moved:
            self.status[i] = ACTIVE
            if self.O.terminal_state(g.leaf_pos()) != 0:
                err = g.on_received_policy([0.0] * 7, 0.0, 0.0, self.c, self.cp)
                assert err == 0, (i, err)
                if g.root_visit_count() >= self.target:
                    self.status[i] = PARKED

    def add_iterations(self, k):
        self.target += int(k)
        assert 1 <= self.target <= self.max
        return self.target

    # ------------------------------------------------------------------ search
    def round(self):
        """one lock-step round of the device: every active game consumes the answer to its leaf; a game whose next leaf is terminal
        runs that simulation too (the network's answer is ignored for it, mcts.rs:92-98)"""
        O = self.O
        act = [i for i in range(self.n_games) if self.status[i] == ACTIVE]
        if not act:
            return 0
        lg, qp, qn = self.ev([self.games[i].leaf_pos() for i in act])
        for j, i in enumerate(act):
            g = self.games[i]
            for trip in range(2):
                err = g.on_received_policy(lg[j], float(qp[j]), float(qn[j]), self.c, self.cp)
                assert err == 0, (i, err)
                if g.root_visit_count() >= self.target:
                    self.status[i] = PARKED
                    break
                if O.terminal_state(g.leaf_pos()) == 0:
                    break
        return len(act)

    def search(self, n=None):
        if n is not None:
            assert 1 <= int(n) <= self.max
            self.target = int(n)
        for i in range(self.n_games):
            self._resume(i)
        need = max([self.target - g.root_visit_count() for g, s in zip(self.games, self.status) if s == ACTIVE], default=0)
        rounds = 0
        while self.round():
            rounds += 1
        assert rounds <= need, (rounds, need)     # a root needs at most target - visits rounds
        self.rounds = rounds
        return rounds

    # ------------------------------------------------------------------ moves
    def _apply(self, i, col, sampled_with=None):
        g = self.games[i]
        before, n_moves = g.root_visit_count(), g.n_moves()
        if self.status[i] == ACTIVE:
            self.moves_under_pending_leaf += 1
        expect = self.O.make_move(g.root_pos(), col)
        err = g.make_move(col, self.c) if sampled_with is None else g.make_random_move(self.c, float(sampled_with))
        assert err == 0 and g.n_moves() == n_moves + 1 and g.root_pos().key() == expect.key(), (i, col, err)
        self.retained.append((int(g.root_visit_count()), int(before)))
        self._resume(i, moved=True)

    def make_moves(self, cols):
        O = self.O
        cols = np.asarray(cols).astype(np.int64).reshape(-1)
        res = np.zeros(self.n_games, dtype=np.int32)
        for i, col in enumerate(cols.tolist()):
            g = self.games[i]
            if col == MOVE_NONE:
                if self.status[i] == PARKED:
                    self._resume(i)
            elif self._terminal(i):
                res[i] = REFUSED_TERMINAL
            elif not (0 <= col <= 6) or not ((O.legal_mask(g.root_pos()) >> col) & 1):
                res[i] = REFUSED_COLUMN
            elif g.root_visit_count() == 0:
                res[i] = REFUSED_UNSEARCHED
            else:
                self._apply(i, col)
        self.last_results = res
        return (res == OK) & (cols != MOVE_NONE)

    def make_random_moves(self, temperature, where=None):
        O = self.O
        sel = np.ones(self.n_games, dtype=bool) if where is None else np.asarray(where, dtype=bool).reshape(-1)
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (self.n_games,))
        res = np.zeros(self.n_games, dtype=np.int32)
        for i in range(self.n_games):
            g = self.games[i]
            if not sel[i]:
                if self.status[i] == PARKED:
                    self._resume(i)
            elif self._terminal(i):
                res[i] = REFUSED_TERMINAL
            elif g.root_visit_count() == 0:
                res[i] = REFUSED_UNSEARCHED
            else:
                col = O.sample_move(self.ids[i], g.n_moves(), g.root_policy(), float(temps[i]))
                if not ((O.legal_mask(g.root_pos()) >> col) & 1):
                    res[i] = REFUSED_SAMPLE
                else:
                    self._apply(i, col, sampled_with=temps[i])
        self.last_results = res
        return (res == OK) & sel

    # ------------------------------------------------------------------ reading
    def snapshot(self, player0_perspective=False):
        recs = np.zeros(self.n_games, dtype=RECORD_DTYPE)
        visits = np.zeros(self.n_games, dtype=np.uint32)
        terminal = np.zeros(self.n_games, dtype=bool)
        for i, g in enumerate(self.games):
            p = g.root_pos()
            qp, qn = np.float32(g.root_q_penalty()), np.float32(g.root_q_no_penalty())
            mask, value = int(p.mask), int(p.value)
            if player0_perspective and bin(mask).count("1") % 2 == 1:     # interactive_play.rs:149-153
                value, qp, qn = mask & ~value, -qp, -qn
            recs[i] = (self.ids[i], mask, value, g.root_policy(), qp, qn, g.n_moves() | (3 << 16))
            visits[i] = g.root_visit_count()
            terminal[i] = self._terminal(i)
        return RefSnapshot(recs, visits, np.array(self.status, dtype=np.uint32), terminal)

    def leaves(self):
        """(mask, value) of every game's pending leaf (MctsGame::leaf_pos)"""
        return [self.games[i].leaf_pos().key() for i in range(self.n_games)]

    def result(self):
        """{game index: [(mask, value, policy bytes, q_penalty bytes, q_no_penalty bytes), ...]} of the games whose root is terminal"""
        out = {}
        for i, g in enumerate(self.games):
            if self._terminal(i):
                out[i] = [(s.mask, s.value, np.array(s.policy, dtype=np.float32).tobytes(), np.float32(s.q_penalty).tobytes(),
                           np.float32(s.q_no_penalty).tobytes()) for s in g.to_result(self.cp)]
        return out


# ---------------------------------------------------------------------------------------------------- positions and evaluators
N_ENGINE_GAMES = 40     # five stepping wavefronts; a partial third 16-board workgroup of the fused launch
_POSITIONS = {}


def engine_positions():
    """(positions, game_ids, kinds): 40 start positions -- the empty board and 39 of tests.helpers.start_job's: the won root, both
    drawn roots, two lost random roots, six roots with exactly one legal column (the drawn line cut 1-3 moves short), and random
    ones of every ply band, odd plies among them; the job's five special ids (0, 42, 43, 1 << 40, 2^64 - 1) ride on the first
    five non-terminal random ones.  kinds[i] = "empty" | "won" | "drawn" | "lost" | "one" | "random"."""
    if _POSITIONS:
        return _POSITIONS["v"]
    from oracle import c4oracle as O

    reqs, starts, part = start_job()
    term = [O.terminal_state(O.Pos(*s)) for s in starts]
    ply = [bin(s[0]).count("1") for s in starts]
    pick, kinds = [], []

    def take(idx, kind, k):
        for i in idx[:k]:
            pick.append(i)
            kinds.append(kind)

    take([i for i, p in enumerate(part) if p == "won"], "won", 1)
    take([i for i, p in enumerate(part) if p == "line" and term[i] == 3], "drawn", 2)
    take([i for i, p in enumerate(part) if p == "random" and term[i] == 2], "lost", 2)
    one = [i for i, p in enumerate(part) if p == "line" and term[i] == 0 and bin(O.legal_mask(O.Pos(*starts[i]))).count("1") == 1 and ply[i] >= 39]
    take(one, "one", 6)
    special = [i for i in range(5)]      # the ids 0, 42, 43, 1 << 40, 2^64 - 1 sit on requests 0..4
    rnd = [i for i, p in enumerate(part) if p == "random" and term[i] == 0 and i not in pick]
    rest = [i for i in special if i in rnd]
    for lo, hi in ((1, 8), (8, 20), (20, 30), (30, 36), (36, 42)):
        band = [i for i in rnd if lo <= ply[i] < hi and i not in rest]
        rest += band[:6]
    take(rest, "random", N_ENGINE_GAMES - 1 - len(pick))
    positions = [(0, 0)] + [starts[i] for i in pick]
    ids = [9_000_001] + [int(reqs[i][0]) for i in pick]
    kinds = ["empty"] + kinds
    assert len(positions) == N_ENGINE_GAMES == len(set(ids))
    _POSITIONS["v"] = (positions, ids, kinds)
    return _POSITIONS["v"]


def c_exploration(ev_name):
    return START_EVALS[ev_name][1]


# ---------------------------------------------------------------------------------------------------- the reference's KAT
# interactive_play.rs:272-303 `forcing_position`: uniform evaluator, 10 000 iterations, c_exploration 4.0, c_ply_penalty 0.01
FORCING = ["⚫⚫⚫⚫⚫⚫⚫"] * 4 + ["⚫⚫🔵🔵⚫⚫⚫", "⚫⚫🔴🔴⚫⚫⚫"]


def uniform_evaluator(leaves):
    """self_play.rs:391-403 UniformEvalPos"""
    n = len(leaves)
    return np.full((n, 7), np.float32(1.0) / np.float32(7.0), dtype=np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)


def forcing_position():
    from oracle import c4oracle as O

    return O.from_rows(FORCING).key()


def forcing_stages(e):
    """the three stages of the reference's test on an Engine or a RefEngine made at 10 000 iterations: [(snapshot, retained)]"""
    out = []
    e.search()
    out.append(e.snapshot(player0_perspective=True))
    for col in (1, 0):
        assert bool(e.make_moves([col])[0])
        e.search()
        out.append(e.snapshot(player0_perspective=True))
    return out


def assert_forcing_thresholds(stages):
    s0, s1, s2 = (s.records[0] for s in stages)
    assert s0["policy"][1] + s0["policy"][4] >= 0.98 and s0["q_penalty"] >= 0.91 and s0["q_no_penalty"] >= 0.98
    assert s1["q_penalty"] >= 0.91 and s1["q_no_penalty"] >= 0.98
    assert s2["policy"][4] >= 0.99 and s2["q_penalty"] >= 0.91 and s2["q_no_penalty"] >= 0.98
    assert [int(s.visits[0]) for s in stages] == [10_000] * 3


# ---------------------------------------------------------------------------------------------------- the move script
def legal_columns(mask):
    return [c for c in range(7) if not (int(mask) >> (35 + c)) & 1]


def run_script(e, target=24, check=None, max_turns=60):
    """The scripted games of T2, on an Engine or a RefEngine fresh from its constructor; check(tag) is called after every
    operation.  Returns the log: (tag, result codes) of every move call.

      a  a move asked of every game before any search: no root has children yet (refusals 3; 1 at terminal roots, 2 where the
         column is full);
      b  search(1), then a sampled move at temperature 1: the root's children have no visits, the policy is uniform and the
         sampled column may be full (refusals 4) -- where it is legal the move is made and keeps nothing;
      c  turns of search(target) + forced moves, the column walking over the legal ones, with a bad column (full, 7, -3) asked of
         every fifth game (refusals 2), finished games asked again (refusals 1), and on every third turn a SECOND move straight
         behind the first, while the first one's new leaf is pending: made where the new root kept visits (it has children),
         refused (3) where it kept none."""
    log = []
    check = check or (lambda tag: None)
    n = e.n_games

    def moves(tag, cols):
        e.make_moves(cols)
        log.append((tag, e.last_results.copy()))
        check(tag)

    moves("a", [i % 7 for i in range(n)])
    e.search(1)
    check("b-search")
    e.make_random_moves(1.0)
    log.append(("b", e.last_results.copy()))
    check("b")
    for t in range(max_turns):
        e.search(target)
        check(f"c{t}-search")
        snap = e.snapshot()
        if bool(snap.terminal.all()):
            break
        cols = []
        for i in range(n):
            legal = legal_columns(snap.records["mask"][i])
            if (i + t) % 5 == 0:
                full = [c for c in range(7) if c not in legal]
                cols.append(full[0] if full and t % 2 == 0 else (7 if t % 3 else -3))
            else:
                cols.append(legal[(3 * i + 5 * t) % len(legal)] if legal else t % 7)
        moves(f"c{t}", cols)
        if t % 3 == 1:
            snap = e.snapshot()
            cols = []
            for i in range(n):
                legal = legal_columns(snap.records["mask"][i])
                cols.append(legal[(i + t) % len(legal)] if legal and i % 2 == 0 else MOVE_NONE)
            moves(f"c{t}-second", cols)
    else:
        raise AssertionError(f"games still under way after {max_turns} turns")
    return log
