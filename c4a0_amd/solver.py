"""Exact solver on the GPU: what the reference gets from Pascal Pons' `c4solver` binary, its opening book and a rocksdb cache
(rust/src/solver.rs), here a HIP alpha-beta search (include/c4a0_hip.h "exact solver", c4a0_amd/csrc/c4_solver.hip) with no
binary and no database, and with a book only of what it has solved itself.

    solver = c4a0_amd.Solver()
    r = solver.solve(positions)              # SolveResult: scores int16[P, 7] as `c4solver -a` prints them, solved bool[P]
    solver.score_policies(positions, pol)    # float32[P]: Solution::score_policy (solver.rs:201-228), NaN where unsolved
    result.solver_score(solver)              # PlayGamesResult / SearchResult: the reference's PlayGamesResult.score_policies

Positions with few stones may exhaust `max_nodes_per_position` and come back with solved = False and a row of UNSOLVED.  The
table of the `Solver` lives across calls (the role of the reference's CachingSolver): asking again later, or with a larger
budget, continues from what was learned.  Two options reach further down the stone counts:

    solver = c4a0_amd.Solver(book_entries=1 << 22)     # keep every exact score of a position with <= book_max_stones stones
    solver.solve(positions, split_stones=14)           # a task out of budget with < 14 stones is replaced by its children
    solver.save_book(path); solver.load_book(path)     # the book as a .npy of uint64 entries

Splitting gives a hard position the width of the GPU -- thousands of cheaper tasks a stone deeper instead of seven lanes -- and the
book keeps what that cost: the search kernel reads it, tasks are answered from it without a launch, and it can be saved.  There is
still no book of openings computed elsewhere: how far down this reaches is a matter of budget.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from .results import N_COLS

FULL_COLUMN = -1000      # include/c4a0_hip.h C4_SOLVE_FULL_COLUMN
UNSOLVED = -32768        # C4_SOLVE_UNSOLVED
_CELLS = np.uint64((1 << 42) - 1)
_COL0 = 0x810204081
_START03 = np.uint64(_COL0 | (_COL0 << 1) | (_COL0 << 2) | (_COL0 << 3))


class SolverScore(NamedTuple):
    """`solver_score`: the mean of score_policies over the samples scored, and what was left out of it."""
    score: float        # NaN when n_scored == 0 (the reference's 0.0 / 0)
    n_scored: int       # non-terminal samples with at least min_stones stones that were solved
    n_unsolved: int     # ... that were not solved within the budget
    n_skipped: int      # non-terminal samples with fewer than min_stones stones


def _u(x: int) -> np.uint64:
    return np.uint64(x)


def _has_four(x: np.ndarray) -> np.ndarray:
    h = x & (x >> _u(1)) & (x >> _u(2)) & (x >> _u(3)) & _START03
    v = x & (x >> _u(7)) & (x >> _u(14)) & (x >> _u(21))
    d1 = x & (x >> _u(8)) & (x >> _u(16)) & (x >> _u(24)) & _START03
    d2 = (x >> _u(3)) & (x >> _u(9)) & (x >> _u(15)) & (x >> _u(21)) & _START03
    return (h | v | d1 | d2) != 0


def is_terminal(mask: np.ndarray, value: np.ndarray) -> np.ndarray:
    """bool[P]: a four of either side or a full board (c4r.rs:228-238), for uint64 arrays."""
    mask, value = np.asarray(mask, dtype=np.uint64), np.asarray(value, dtype=np.uint64)
    return _has_four(mask & value) | _has_four(mask & ~value) | ((mask & _CELLS) == _CELLS)


def stone_counts(mask: np.ndarray) -> np.ndarray:
    m = np.ascontiguousarray(mask, dtype=np.uint64)
    return np.unpackbits(m.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def _mirror(x: np.ndarray) -> np.ndarray:
    """The 7 columns of every row reversed (c4r.rs:289-299), for uint64 arrays."""
    out = np.zeros_like(x)
    col = np.uint64(_COL0)
    for c in range(7):
        cells = x & (col << _u(c))
        out |= (cells >> _u(c)) << _u(6 - c)
    return out


def score_rows(scores: np.ndarray, policies: np.ndarray) -> np.ndarray:
    """float32[P]: Solution::score_policy (solver.rs:201-228) of each policy against its score row.  The policy's choice is its
    FIRST maximum; 1.0 if that column's score equals the row's maximum, else 0.5 if its score is > 0, else 0.0; NaN for a row
    of UNSOLVED.  Host arithmetic on given rows: no GPU."""
    scores = np.asarray(scores, dtype=np.int16).reshape(-1, N_COLS)
    policies = np.asarray(policies, dtype=np.float32).reshape(-1, N_COLS)
    if len(scores) != len(policies):
        raise ValueError("scores and policies must have one row per position each")
    out = np.zeros(len(scores), dtype=np.float32)
    if len(scores) == 0:
        return out
    sel = np.argmax(policies, axis=1)
    picked = scores[np.arange(len(scores)), sel]
    out[picked > 0] = 0.5
    out[picked == scores.max(axis=1)] = 1.0
    out[(scores == UNSOLVED).all(axis=1)] = np.nan
    return out


class SolveResult:
    """scores int16[P, 7]: per column what `c4solver -a` prints (FULL_COLUMN for a full column; positive = the side to move
    wins, larger = sooner), a row of UNSOLVED where `solved` is False.  stats: nodes, probes, launches, tasks, unsolved_tasks of
    the call, split_tasks, combined_nodes, dropped_tasks, book_hits_host, book_inserts, book_full (include/c4a0_hip.h
    c4_solver_stats_ex), and unique_positions (what was left after removing duplicates and mirror images)."""

    __slots__ = ("scores", "solved", "stats")

    def __init__(self, scores: np.ndarray, solved: np.ndarray, stats: dict):
        self.scores, self.solved, self.stats = scores, solved, stats

    def best_moves_mask(self) -> np.ndarray:
        """bool[P, 7]: the columns whose score is the row's maximum (all False where unsolved)."""
        return (self.scores == self.scores.max(axis=1, keepdims=True)) & self.solved[:, None] if len(self.scores) else np.zeros((0, 7), dtype=bool)

    def winning_moves_mask(self) -> np.ndarray:
        """bool[P, 7]: the columns with a score > 0."""
        return (self.scores > 0) & self.solved[:, None]

    def score_policies(self, policies) -> np.ndarray:
        return score_rows(self.scores, policies)

    def __len__(self) -> int:
        return len(self.scores)

    def __repr__(self):
        return f"SolveResult({len(self.scores)} positions, {int(self.solved.sum())} solved)"


class Solver:
    """An exact Connect Four solver on one GPU.  `tt_entries`: entries of its transposition table (a power of two, 8 bytes
    each; the default 2^24 = 128 MB), kept until `close()`.  `book_entries`: 0, or the entries of a book of exact scores (a power
    of two, 8 bytes each on the device and on the host) that keeps every position of at most `book_max_stones` stones the solver
    obtains an exact score for; it is never more than half full and nothing leaves it."""

    def __init__(self, device=None, tt_entries: int = 1 << 24, book_entries: int = 0, book_max_stones: int = 20):
        import torch

        from ._lib import check, lib

        if int(tt_entries) < 16 or int(tt_entries) > 1 << 32 or int(tt_entries) & (int(tt_entries) - 1):
            raise ValueError("tt_entries must be a power of two between 16 and 2**32")
        if int(book_entries) != 0 and (int(book_entries) < 16 or int(book_entries) > 1 << 28 or int(book_entries) & (int(book_entries) - 1)):
            raise ValueError("book_entries must be 0 or a power of two between 16 and 2**28")
        if not 1 <= int(book_max_stones) <= 41:
            raise ValueError("book_max_stones must be between 1 and 41")
        if not torch.cuda.is_available():
            raise RuntimeError("c4a0_amd.Solver needs a HIP device: the solver is a GPU kernel and there is no CPU path")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise ValueError("Solver runs on a HIP device")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.tt_entries, self.book_entries, self.book_max_stones = int(tt_entries), int(book_entries), int(book_max_stones)
        self._h = C.c_void_p()
        check(lib().c4_solver_create_ex(self.tt_entries, self.book_entries, self.book_max_stones, self.device.index, C.byref(self._h)))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            from ._lib import check, lib

            check(lib().c4_solver_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _book_entries(self) -> np.ndarray:
        from ._lib import check, lib

        if not self._h:
            raise RuntimeError("this Solver is closed")
        n = C.c_uint64(0)
        check(lib().c4_solver_book_export(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        check(lib().c4_solver_book_export(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value]

    @property
    def book_size(self) -> int:
        """Entries in the book."""
        from ._lib import check, lib

        if not self._h:
            raise RuntimeError("this Solver is closed")
        n = C.c_uint64(0)
        check(lib().c4_solver_book_export(self._h, None, 0, C.byref(n)))
        return int(n.value)

    def save_book(self, path) -> int:
        """Write the book's entries to `path` as a .npy of uint64 (the name as given: no suffix is added); returns how many."""
        entries = self._book_entries()
        with open(path, "wb") as f:
            np.save(f, entries)
        return len(entries)

    def load_book(self, path) -> int:
        """Add the entries of a file written by `save_book` to the book; returns how many the file held.  Every entry is checked
        (include/c4a0_hip.h c4_solver_book_import): a ValueError names the first bad one, and then nothing was added."""
        from ._lib import ERR_BAD_ARG, check, lib

        if not self._h:
            raise RuntimeError("this Solver is closed")
        entries = np.load(path, allow_pickle=False)
        if entries.dtype != np.uint64 or entries.ndim != 1:
            raise ValueError("a book file holds a one-dimensional uint64 array")
        entries = np.ascontiguousarray(entries)
        status = lib().c4_solver_book_import(self._h, entries.ctypes.data, len(entries))
        if status == ERR_BAD_ARG:
            raise ValueError(lib().c4_last_error_string().decode())
        check(status)
        return len(entries)

    def solve(self, positions, *, nodes_per_launch: Optional[int] = None, max_nodes_per_position: Optional[int] = None,
              split_stones: Optional[int] = None, split_max_tasks: Optional[int] = None) -> SolveResult:
        """Solve every position of `positions` -- a sequence of (mask, value) or a uint64[P, 2] array, as `search_positions`
        takes them; each must be non-terminal.  Duplicates are solved once and a position and its mirror image as one.
        `nodes_per_launch`: node visits a GPU lane gets per kernel launch; `max_nodes_per_position`: visits after which a
        child's search is given up (None: the library's defaults, include/c4a0_hip.h).  `split_stones`: a task given up with
        fewer stones than this is replaced by its children instead (None or 0: never); `split_max_tasks`: tasks one call may make
        that way (None: 2^18), a bound on device memory at 392 bytes per task."""
        import torch

        from ._lib import SolverOptions, SolverStatsEx, check, lib
        from .api import _positions_array

        if not self._h:
            raise RuntimeError("this Solver is closed")
        pos = _positions_array(positions)
        for name, v in (("nodes_per_launch", nodes_per_launch), ("max_nodes_per_position", max_nodes_per_position)):
            if v is not None and not (1 <= int(v) < 1 << 40):
                raise ValueError(f"{name} must be between 1 and 2**40")
        if split_stones is not None and not (0 <= int(split_stones) <= 42):
            raise ValueError("split_stones must be between 0 and 42")
        if split_max_tasks is not None and not (1 <= int(split_max_tasks) <= 1 << 24):
            raise ValueError("split_max_tasks must be between 1 and 2**24")
        term = is_terminal(pos[:, 0], pos[:, 1])
        if bool(term.any()):
            raise ValueError(f"position {int(np.flatnonzero(term)[0])}: the position is terminal (nothing to solve)")
        n = len(pos)
        if n == 0:
            return SolveResult(np.zeros((0, 7), dtype=np.int16), np.zeros(0, dtype=bool),
                               dict(SolverStatsEx().as_dict(), unique_positions=0))
        # a position and its mirror image are one problem: the smaller (mask, value) of the two is solved, the row reversed on the way back
        mm, mv = _mirror(pos[:, 0]), _mirror(pos[:, 1])
        flipped = (mm < pos[:, 0]) | ((mm == pos[:, 0]) & (mv < pos[:, 1]))
        canon = np.where(flipped[:, None], np.stack([mm, mv], axis=1), pos)
        uniq, inverse = np.unique(canon, axis=0, return_inverse=True)
        uniq = np.ascontiguousarray(uniq, dtype=np.uint64)
        scores = np.empty((len(uniq), 7), dtype=np.int16)
        solved = np.empty(len(uniq), dtype=np.uint8)
        st = SolverStatsEx()
        opt = SolverOptions(C.sizeof(SolverOptions), int(nodes_per_launch or 0), int(max_nodes_per_position or 0), int(split_stones or 0),
                            int(split_max_tasks or 0))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().c4_solver_solve_ex(self._h, uniq.ctypes.data, len(uniq), C.byref(opt), scores.ctypes.data, solved.ctypes.data, C.byref(st),
                                       C.c_void_p(stream)))
        inverse = np.asarray(inverse).reshape(-1)
        rows = scores[inverse]
        rows[flipped] = rows[flipped][:, ::-1]
        stats = st.as_dict()
        stats["unique_positions"] = len(uniq)
        return SolveResult(np.ascontiguousarray(rows), solved[inverse].astype(bool), stats)

    def score_policies(self, positions, policies, **budget) -> np.ndarray:
        """float32[P]: CachingSolver::score_policies (solver.rs:36-48) -- each policy's first maximum judged against the solved
        position: 1.0 a best move, 0.5 a winning move that is not best, 0.0 otherwise; NaN where the position was not solved."""
        return self.solve(positions, **budget).score_policies(policies)


def solver_score_of_records(recs: np.ndarray, solver: Optional[Solver] = None, *, min_stones: int = 0, **budget) -> SolverScore:
    """PlayGamesResult.score_policies (pybridge.rs:129-147) on packed sample records: the mean of score_policies over the
    non-terminal samples.  Extensions that make it a different number than the reference's when they bite: samples with fewer
    than `min_stones` stones are left out (n_skipped) and so are samples not solved within the budget (n_unsolved).
    `solver`: a Solver to use (and whose table to keep filling); None makes one for the call."""
    mask, value = np.ascontiguousarray(recs["mask"]), np.ascontiguousarray(recs["value"])
    live = ~is_terminal(mask, value)
    enough = stone_counts(mask) >= int(min_stones)
    pick = live & enough
    n_skipped = int((live & ~enough).sum())
    if not bool(pick.any()):
        return SolverScore(float("nan"), 0, 0, n_skipped)
    own = solver is None
    if own:
        solver = Solver()
    try:
        s = solver.score_policies(np.stack([mask[pick], value[pick]], axis=1), np.ascontiguousarray(recs["policy"])[pick], **budget)
    finally:
        if own:
            solver.close()
    ok = ~np.isnan(s)
    n_scored = int(ok.sum())
    # the reference sums f32 scores in sample order and divides by the count (pybridge.rs:143-146); halves sum exactly in f32 up to 2^24
    score = float(np.float32(s[ok].sum(dtype=np.float32)) / np.float32(n_scored)) if n_scored else float("nan")
    return SolverScore(score, n_scored, int((~ok).sum()), n_skipped)
