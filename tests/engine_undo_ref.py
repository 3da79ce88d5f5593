"""The reference of `Engine.undo_moves` / `Engine.reset_games` (test infrastructure): tests/engine_ref.py's RefEngine with
MctsGame::undo_move (mcts.rs:230-245) and reset_game (mcts.rs:225-227) on top.

The oracle's `Game` has no undo and starts every game at n_moves = 0, so the model keeps what the reference's `moves` list keeps
and stands on the oracle for everything else:

  history   per game, (position, untempered root policy) of every accepted move -- the reference's RecordedMove list;
  base      per game, the moves made before the current oracle `Game` object was created.  The TRUE move count is
            base + Game.n_moves(): the snapshot's meta, and the seed of a sampled move (game_id * (42 + moves.len()), mcts.rs:215);
  undo      the reference pops the last RecordedMove and makes the root Node::new(pos, Weak::new(), 1.0): a fresh oracle Game at
            that position with the game's id (0 visits, no children, leaf = root), the history shortened, base = its length; then
            ensure_bg_thread: the game is active, its root the pending leaf.  reset_game = undo_move until it returns false: a
            game with moves goes to history[0]'s position; one without is not touched (it keeps its tree);
  sampled   the column is c4o_sample_move(id, TRUE count, root policy, temperature) and is made with Game.make_move (the oracle's
            own make_random_move would seed with its own count);
  result    to_result (mcts.rs:271-313) restated over the history: sample i gets +q iff (M - i) is even, q = the terminal value
            of the root; then the uniform terminal sample.  tests/test_engine_undo_ref.py holds this restatement to the oracle's
            to_result on every game the move script finishes.

Result codes of an undo: 0 accepted or none asked, 6 no move made, 7 not a request."""
from __future__ import annotations

import numpy as np

from tests.engine_ref import ACTIVE, OK, PARKED, RefEngine, RefSnapshot

UNDO_NONE, UNDO_ONE, UNDO_ALL = 0, 1, 2
REFUSED_NO_MOVES, REFUSED_REQUEST = 6, 7
UNIFORM = np.full(7, np.float32(1.0) / np.float32(7.0), dtype=np.float32)


class RefEngineUndo(RefEngine):
    def __init__(self, *a, **kw):
        self.history = None
        super().__init__(*a, **kw)
        self.history = [[] for _ in range(self.n_games)]
        self.base = [0] * self.n_games
        self.undone = 0            # accepted undo / reset requests
        self.undone_finished = 0   # ... of games whose root was terminal

    def true_count(self, i):
        return self.base[i] + self.games[i].n_moves()

    # ------------------------------------------------------------------ moves
    def _apply(self, i, col, sampled_with=None):
        assert sampled_with is None                       # (sampled columns are made with make_move, see make_random_moves)
        g = self.games[i]
        self.history[i].append((g.root_pos().key(), g.root_policy().copy()))
        super()._apply(i, col)
        assert self.true_count(i) == len(self.history[i])

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
                res[i] = 1
            elif g.root_visit_count() == 0:
                res[i] = 3
            else:
                col = O.sample_move(self.ids[i], self.true_count(i), g.root_policy(), float(temps[i]))
                if not ((O.legal_mask(g.root_pos()) >> col) & 1):
                    res[i] = 4
                else:
                    self._apply(i, col)
        self.last_results = res
        return (res == OK) & sel

    # ------------------------------------------------------------------ undo
    def undo_requests(self, requests):
        """c4_session_hold_undo: one request per game; returns the result codes"""
        O = self.O
        requests = np.asarray(requests).astype(np.int64).reshape(-1)
        res = np.zeros(self.n_games, dtype=np.int32)
        for i, req in enumerate(requests.tolist()):
            if req == UNDO_NONE:
                pass
            elif req not in (UNDO_ONE, UNDO_ALL):
                res[i] = REFUSED_REQUEST
            elif not self.history[i]:
                res[i] = REFUSED_NO_MOVES
            else:
                keep = len(self.history[i]) - 1 if req == UNDO_ONE else 0
                pos = self.history[i][keep][0]
                self.undone_finished += int(self._terminal(i))
                del self.history[i][keep:]
                self.games[i] = O.Game(O.Pos(*pos), self.ids[i])
                self.base[i] = keep
                self.status[i] = None
                self.undone += 1
            if res[i] != OK or req == UNDO_NONE:
                if self.status[i] == PARKED:              # (the resume every slot gets behind the undo)
                    self._resume(i)
            else:
                self._resume(i, moved=True)
                assert self.status[i] == ACTIVE and self.games[i].leaf_pos().key() == pos
        self.last_results = res
        return res

    def _undo(self, request, where):
        sel = np.ones(self.n_games, dtype=bool) if where is None else np.asarray(where, dtype=bool).reshape(-1)
        res = self.undo_requests(np.where(sel, request, UNDO_NONE))
        return (res == OK) & sel

    def undo_moves(self, where=None):
        return self._undo(UNDO_ONE, where)

    def reset_games(self, where=None):
        return self._undo(UNDO_ALL, where)

    # ------------------------------------------------------------------ reading
    def snapshot(self, player0_perspective=False):
        s = super().snapshot(player0_perspective)
        if self.history is None:
            return s
        recs = s.records.copy()
        for i in range(self.n_games):
            recs["meta"][i] = self.true_count(i) | (3 << 16)
        return RefSnapshot(recs, s.visits, s.status, s.terminal)

    def result(self):
        O = self.O
        out = {}
        for i, g in enumerate(self.games):
            if not self._terminal(i):
                continue
            root = g.root_pos()
            _t, q_pen, q_nopen = O.terminal_value(root, self.cp)
            q_pen, q_nopen = np.float32(q_pen), np.float32(q_nopen)
            m_total = len(self.history[i])
            samples = []
            for k, ((mask, value), policy) in enumerate(self.history[i]):
                sign = np.float32(1.0) if (m_total - k) % 2 == 0 else np.float32(-1.0)
                a, b = (q_pen, q_nopen) if sign > 0 else (-q_pen, -q_nopen)
                samples.append((mask, value, np.asarray(policy, dtype=np.float32).tobytes(), np.float32(a).tobytes(), np.float32(b).tobytes()))
            samples.append((int(root.mask), int(root.value), UNIFORM.tobytes(), q_pen.tobytes(), q_nopen.tobytes()))
            out[i] = samples
        return out


# ---------------------------------------------------------------------------------------------------- the move script with undos
def run_undo_script(e, target=24, check=None, max_turns=150):
    """Scripted games with undos on the way, on an Engine or a RefEngineUndo fresh from its constructor; check(tag) is called after
    every operation.  A turn: search(target); a forced move for every game (the column walks over the legal ones; finished games
    are asked too and refuse); then a third of the games -- (i + t) % 3 == 0, finished ones among them -- take their last move
    back.  The script ends after the move that leaves every root terminal.  Returns the log: (tag, result codes) of every call."""
    from tests.engine_ref import legal_columns

    log = []
    check = check or (lambda tag: None)
    n = e.n_games
    for t in range(max_turns):
        e.search(target)
        check(f"u{t}-search")
        snap = e.snapshot()
        cols = []
        for i in range(n):
            legal = legal_columns(snap.records["mask"][i])
            cols.append(legal[(3 * i + 5 * t) % len(legal)] if legal else t % 7)
        e.make_moves(cols)
        log.append((f"u{t}-move", e.last_results.copy()))
        check(f"u{t}-move")
        if bool(e.snapshot().terminal.all()):
            return log
        e.undo_moves((np.arange(n) + t) % 3 == 0)
        log.append((f"u{t}-undo", e.last_results.copy()))
        check(f"u{t}-undo")
    raise AssertionError(f"games still under way after {max_turns} turns")
