"""GPU-resident interactive play: P games whose trees persist across moves that come from outside.

The reference's `InteractivePlay` (rust/src/interactive_play.rs, the engine behind `run_tui`) is ONE `MctsGame` whose tree lives on:
searched up to a visit budget, moved by `make_move` / `make_random_move(temperature)` with the subtree under the move kept
(mcts.rs:187-206), taken back by `undo_move` / `reset_game` (mcts.rs:225-245), its budget raised by `increase_mcts_iters`, read by
`snapshot()`.  `Engine` is that for P games at once on a hold
session (include/c4a0_hip.h C4_FLAG_HOLD): game i lives on slot i, every operation is one launch for all of them, and nothing but
the moves, the move results and the snapshots crosses to the host.  It plays matches against an outside engine or a person, or
suites of games move by move under host control; finished games come out as the `PlayGamesResult` self-play produces.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .results import PlayGamesResult, SearchResult, results_from_records, terminal_state
from .session import DeviceEvaluator, DeviceSession

_U64 = np.uint64


class Snapshot(SearchResult):
    """`Engine.snapshot()`: per game, in the order the games were given, the root position, root policy and the two root q values
    (the columns of `SearchResult`), plus

    visits: uint32[P] the root's visit count (Snapshot.n_mcts_iterations, interactive_play.rs:160);
    n_moves: int64[P] moves the game has made;  terminal: bool[P] the root is a terminal position;
    status: uint32[P] the slot's status (1 active, 64 parked, else the c4_status that ended the game)."""

    __slots__ = ("visits", "status", "n_moves", "terminal")

    def __init__(self, records: np.ndarray, visits: np.ndarray, status: np.ndarray, terminal: np.ndarray):
        super().__init__(records)
        self.visits, self.status, self.terminal = visits, status, terminal
        self.n_moves = (self.records["meta"] & 0xFFFF).astype(np.int64)

    def __repr__(self):
        return f"Snapshot({len(self.records)} games)"


class Engine:
    """P persistent games on one GPU.

    evaluator: ONE device evaluator, as `search_positions` takes it (e.g. c4a0_amd.nn.InferenceNet).
    max_mcts_iterations: the largest target `search` may be asked for (it sizes the tree arena: 43 n + 8 blocks per game unless
    blocks_per_slot says otherwise -- above 1 523 it must), and the target until `search(n)` / `add_iterations` change it.
    positions: the start positions, a sequence of (mask, value) or uint64[P, 2] (any position a game can show, terminal ones
    included), or n_games: that many games from the empty board.  game_ids: uint64[P] (default 0..P-1): the seed of a sampled move
    is game_id * (42 + moves made) (mcts.rs:215).
    steps_per_graph: rounds per HIP-graph replay for a graph-safe evaluator (0 = never replay graphs)."""

    def __init__(self, evaluator: DeviceEvaluator, max_mcts_iterations: int, c_exploration: float, c_ply_penalty: float, *,
                 positions=None, n_games: Optional[int] = None, game_ids=None, device=None, blocks_per_slot: int = 0,
                 steps_per_graph: int = 8):
        from .api import _positions_array

        if evaluator is None or isinstance(evaluator, dict) or not callable(evaluator):
            raise TypeError("Engine needs ONE device evaluator (a callable on device tensors, e.g. c4a0_amd.nn.InferenceNet)")
        if (positions is None) == (n_games is None):
            raise TypeError("Engine takes either positions= or n_games=")
        pos = _positions_array(positions) if positions is not None else np.zeros((int(n_games), 2), dtype=_U64)
        if len(pos) == 0:
            raise ValueError("Engine needs at least one game")
        if not (1 <= int(max_mcts_iterations) <= 65527):
            raise ValueError("max_mcts_iterations must be between 1 and 65 527")
        ids = np.arange(len(pos), dtype=_U64) if game_ids is None else np.ascontiguousarray(game_ids, dtype=_U64).reshape(-1)
        if len(ids) != len(pos):
            raise ValueError("game_ids must match the games")
        self.evaluator = evaluator
        self.n_games = len(pos)
        self.max_mcts_iterations = int(max_mcts_iterations)
        self.target = self.max_mcts_iterations
        self.steps_per_graph = int(steps_per_graph)
        self._reqs = np.zeros((self.n_games, 3), dtype=_U64)
        self._reqs[:, 0] = ids
        planes_dtype = torch.bfloat16 if getattr(evaluator, "dtype", None) == torch.bfloat16 else torch.float32
        self.session = s = DeviceSession(self.n_games, self.max_mcts_iterations, c_exploration, c_ply_penalty, device=device,
                                         planes_dtype=planes_dtype, blocks_per_slot=blocks_per_slot, hold=True)
        try:
            s.set_games(self._reqs, pos)
            with torch.cuda.device(s.device):
                self._cols = torch.zeros(self.n_games, dtype=torch.int32, device=s.device)
                self._temps = torch.ones(self.n_games, dtype=torch.float32, device=s.device)
                self._results = torch.zeros(self.n_games, dtype=torch.int32, device=s.device)
            s.set_timing(False)   # (no per-launch device clock: the fused output + step launch and graph captures want it off)
            s.bind()
            s.start()
        except Exception:
            s.close()
            raise
        self._graph, self._graph_target = None, None
        self.rounds = 0            # lock-step rounds of the last search()
        self.last_results = np.zeros(self.n_games, dtype=np.int32)   # c4_session_hold_resume's / _hold_undo's codes of the last move / undo call

    # ---------------------------------------------------------------- lifetime
    def close(self):
        self._graph = None
        if getattr(self, "session", None) is not None:
            self.session.close()
            self.session = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- search
    def add_iterations(self, k: int) -> int:
        """InteractivePlay::increase_mcts_iters (interactive_play.rs:63-67): raises the target by k; the next search() runs to it."""
        return self._set_target(self.target + int(k))

    def _set_target(self, n: int) -> int:
        if not (1 <= int(n) <= self.max_mcts_iterations):
            raise ValueError(f"the target must be between 1 and max_mcts_iterations = {self.max_mcts_iterations} (it sizes the tree arena)")
        self.target = int(n)
        return self.target

    def _sync(self):
        torch.cuda.synchronize(self.session.device)

    def search(self, n: Optional[int] = None) -> int:
        """Search every game until its root has the target's visits (n: a new, absolute target; None: the current one) or is
        terminal; games already there stay parked.  Returns the lock-step rounds run.

        Rounds run until the non-blocking probe says no slot is active.  The loop is bounded: a root needs at most
        target - visits rounds (a round is one simulation at least), so with a slot still active after
        max(target - visits) + 2 rounds the search raises instead of polling on."""
        s = self.session
        if n is not None:
            self._set_target(n)
        s.set_iterations(self.target)
        s.hold_resume()
        s.hold_poll()   # (asks: the first answer is there when the first rounds are on their way)
        graph = None
        if self.steps_per_graph > 0 and getattr(self.evaluator, "graph_safe", False):
            if self._graph is None or self._graph_target != self.target:   # a captured launch carries the target it was captured with
                self._graph, self._graph_target = None, None
                self._sync()
                self._graph, self._graph_target = s.capture_steps(self.evaluator, self.steps_per_graph), self.target
            graph = self._graph
        bound = self.target + 2          # until the probe has told how far the farthest root is from the target
        rounds = 0
        while True:
            if graph is not None:
                graph.replay()           # (rounds behind the last parking step nothing: every slot is skipped)
                rounds += self.steps_per_graph
            else:
                for _ in range(max(1, min(8, bound - rounds))):
                    s.round(self.evaluator)
                    rounds += 1
            active, need, err = s.hold_poll()
            if err:
                self._sync()
                s.raise_if_device_error()
            if active == 0:
                break
            if need is not None:
                bound = min(bound, need + 2)
            if rounds >= bound:
                self._sync()
                s.hold_poll()            # (takes what has landed, asks again: the answer below is the state after every round above)
                self._sync()
                active, _need, err = s.hold_poll()
                if err:
                    s.raise_if_device_error()
                if active:
                    raise RuntimeError(f"Engine.search: {active} games still active after {rounds} rounds towards a target of {self.target} visits")
                break
        self.rounds = rounds
        return rounds

    # ---------------------------------------------------------------- moves
    def _move(self, cols: np.ndarray, temps: Optional[np.ndarray]) -> np.ndarray:
        s = self.session
        self._cols.copy_(torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)))
        if temps is not None:
            self._temps.copy_(torch.from_numpy(np.array(temps, dtype=np.float32)))
        s.hold_resume(self._cols, self._temps if temps is not None else None, self._results)
        self.last_results = self._results.cpu().numpy().astype(np.int32)   # (synchronises)
        return (self.last_results == _lib.HOLD_OK) & (cols != _lib.HOLD_MOVE_NONE)

    def make_moves(self, cols) -> np.ndarray:
        """InteractivePlay::make_move (interactive_play.rs:70-76, 169-176) for every game: cols int[P], a column 0..6 or -1 for no
        move.  Returns bool[P]: the move was made.  A refused move (terminal root, column outside 0..6 or full, a root not searched
        yet) leaves its game exactly as it was; `last_results` has the reason (c4a0_amd._lib.HOLD_REFUSED_*).  The subtree under the
        move is kept; the game's next leaf is selected, so search() goes on from the visits retained."""
        cols = np.asarray(cols).astype(np.int64).reshape(-1)
        if len(cols) != self.n_games:
            raise ValueError("one column per game")
        # (-2 is the sampling code of the C ABI: make_random_moves asks for that; anything else outside 0..6 is refused per game)
        cols = np.where((cols < _lib.HOLD_MOVE_NONE) | (cols > 6), 7, cols)
        return self._move(cols, None)

    def make_random_moves(self, temperature, where=None) -> np.ndarray:
        """InteractivePlay::make_random_move (interactive_play.rs:78-85, 178-185; mcts.rs:214-222) for the games `where` selects
        (bool[P]; None = all): the column is sampled from apply_temperature(root policy, temperature) -- temperature a float or
        float[P] -- with seed game_id * (42 + moves made).  Returns bool[P] as make_moves."""
        sel = np.ones(self.n_games, dtype=bool) if where is None else np.asarray(where, dtype=bool).reshape(-1)
        if len(sel) != self.n_games:
            raise ValueError("one flag per game")
        temps = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (self.n_games,))
        return self._move(np.where(sel, _lib.HOLD_MOVE_SAMPLE, _lib.HOLD_MOVE_NONE), temps)

    # ---------------------------------------------------------------- taking moves back
    def _undo(self, request: int, where) -> np.ndarray:
        sel = np.ones(self.n_games, dtype=bool) if where is None else np.asarray(where, dtype=bool).reshape(-1)
        if len(sel) != self.n_games:
            raise ValueError("one flag per game")
        self._cols.copy_(torch.from_numpy(np.where(sel, request, _lib.HOLD_UNDO_NONE).astype(np.int32)))
        self.session.hold_undo(self._cols, self._results)
        self.last_results = self._results.cpu().numpy().astype(np.int32)   # (synchronises)
        return (self.last_results == _lib.HOLD_OK) & sel

    def undo_moves(self, where=None) -> np.ndarray:
        """InteractivePlay::undo_move (MctsGame::undo_move, mcts.rs:230-245) for the games `where` selects (bool[P]; None = all):
        the last move is taken back.  Returns bool[P]: a move was undone; a game that has made no move is refused
        (`last_results`: c4a0_amd._lib.HOLD_REFUSED_NO_MOVES) and stays exactly as it was.  As in the reference the root is a
        FRESH node at the earlier position -- the tree is dropped, the game's arena given back, the next sampled move's seed uses
        the shortened move count -- and is the game's pending leaf: search() searches it towards the target again.  A finished
        game can be undone like any other; it leaves result() until a move finishes it again."""
        return self._undo(_lib.HOLD_UNDO_ONE, where)

    def reset_games(self, where=None) -> np.ndarray:
        """InteractivePlay::reset_game (MctsGame::reset_game, mcts.rs:225-227: undo_move until it returns false) for the games
        `where` selects: back to the start position with a fresh root and no moves.  Returns bool[P]: something was undone; a
        game without moves keeps its tree (`last_results`: HOLD_REFUSED_NO_MOVES)."""
        return self._undo(_lib.HOLD_UNDO_ALL, where)

    # ---------------------------------------------------------------- reading
    def snapshot(self, player0_perspective: bool = False) -> Snapshot:
        """InteractivePlay::snapshot for every game, one launch and one copy.  player0_perspective=True applies
        interactive_play.rs:149-153: at odd ply the position is inverted and both q values negated."""
        recs, visits, status = self.session.snapshot()
        mask, value = recs["mask"].copy(), recs["value"].copy()
        terminal = np.array([terminal_state(int(m), int(v)) != 0 for m, v in zip(mask, value)], dtype=bool)
        if player0_perspective:
            odd = np.array([bin(int(m)).count("1") & 1 for m in mask], dtype=bool)
            recs["value"] = np.where(odd, mask & ~value, value)
            recs["q_penalty"] = np.where(odd, -recs["q_penalty"], recs["q_penalty"])
            recs["q_no_penalty"] = np.where(odd, -recs["q_no_penalty"], recs["q_no_penalty"])
        return Snapshot(recs, visits, status, terminal)

    def result(self) -> PlayGamesResult:
        """The finished games -- a move made their root terminal, or they started from a terminal position (one sample) -- as
        `play_games` returns them: MctsGame::to_result (mcts.rs:271-313).  Games still under way are left out."""
        counts = self.session.sample_counts()
        done = counts > 0
        return results_from_records(self._reqs[done], self.session.drain_samples(), counts[done])
