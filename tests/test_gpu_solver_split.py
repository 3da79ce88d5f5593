"""Splitting and the book of the GPU solver (c4a0_amd.Solver(book_entries=...), solve(split_stones=...): c4_solver_solve_ex,
c4a0_amd/csrc/c4_solver_split.hpp, solver_kernel<true>) against the plain C solver (tests/solver_ref.c): 300 positions of 24 stones
under a budget of 64 node visits per task, which alone solves only part of them.  Every table here has at most 2^16 entries.
Splitting and the book at the stone counts they are meant for, 12 to 14, are in tests/test_gpu_solver_low_stones.py, against the
recorded rows of tests/golden/solver_rows.npz."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, N_POSITIONS, STONES, BUDGET = 20261019, 300, 24, 64
# 228 992: the tasks the CPU emulation makes by splitting on this set (tests/test_solver_split_host.py, launch budget 8); table races
# change node counts on the GPU, hence four times that
CAP = 4 * 228_992
TT = 1 << 16
SPLIT = dict(max_nodes_per_position=BUDGET, split_stones=42, split_max_tasks=CAP)


@functools.lru_cache(maxsize=None)
def the_set():
    """(300 positions of 24 stones, the plain C solver's rows): computed once, shared, never written to."""
    pos = R.playout_positions(SEED, N_POSITIONS, STONES, STONES)
    rows = R.solve(pos)[0]
    pos.setflags(write=False)
    rows.setflags(write=False)
    return pos, rows


def _solver(**kw):
    import c4a0_amd

    return c4a0_amd.Solver(tt_entries=TT, **kw)


def test_splitting_solves_the_set_and_the_budget_alone_does_not():
    pos, want = the_set()
    with _solver() as solver:
        plain = solver.solve(pos, max_nodes_per_position=BUDGET)
        assert 0 < plain.solved.sum() < len(pos) and plain.stats["split_tasks"] == 0
        assert np.array_equal(plain.scores[plain.solved], want[plain.solved]) and (plain.scores[~plain.solved] == R.UNSOLVED).all()
        r = solver.solve(pos, **SPLIT)
    print(r.stats)
    assert r.solved.all() and r.stats["unsolved_tasks"] == 0 and np.array_equal(r.scores, want)
    assert r.stats["split_tasks"] > 0 and r.stats["combined_nodes"] > 0 and r.stats["tasks"] > r.stats["split_tasks"]
    assert r.stats["book_inserts"] == r.stats["book_hits_host"] == r.stats["book_full"] == 0      # there is no book


def test_splitting_under_a_small_launch_budget():
    pos, want = the_set()
    with _solver() as solver:
        r = solver.solve(pos, nodes_per_launch=16, **SPLIT)
    assert r.solved.all() and np.array_equal(r.scores, want) and r.stats["split_tasks"] > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_splitting_edge_counts(n):
    pos, want = the_set()
    with _solver() as solver:
        r = solver.solve(pos[:n], **SPLIT)
    assert r.solved.all() and np.array_equal(r.scores, want[:n])


def test_cap_exhaustion_is_all_or_nothing_and_a_second_call_completes():
    pos, want = the_set()
    with _solver() as solver:
        r = solver.solve(pos, max_nodes_per_position=BUDGET, split_stones=42, split_max_tasks=2000)      # returns normally
        assert 2000 <= r.stats["split_tasks"] < 2007
        assert 0 < r.solved.sum() < len(pos) and r.stats["unsolved_tasks"] > 0
        assert np.array_equal(r.scores[r.solved], want[r.solved]) and (r.scores[~r.solved] == R.UNSOLVED).all()      # never a mixture
        again = solver.solve(pos, **SPLIT)
    assert again.solved.all() and np.array_equal(again.scores, want)


def _descendants(pos, depth):
    """The distinct non-terminal positions `depth` stones below `pos`."""
    from c4a0_amd.solver import is_terminal

    level = {tuple(p) for p in pos.tolist()}
    for _ in range(depth):
        nxt = np.array(sorted({R.play(m, v, c) for m, v in level for c in R.legal(m)}), dtype=np.uint64)
        level = {tuple(p) for p in nxt[~is_terminal(nxt[:, 0], nxt[:, 1])].tolist()}
    return np.array(sorted(level), dtype=np.uint64)


def test_the_kernel_reads_the_book():
    pos, want = the_set()
    pos, want = pos[:50], want[:50]
    below = _descendants(pos, 2)
    with _solver(book_entries=1 << 16, book_max_stones=30) as solver, _solver() as bookless:
        filled = solver.solve(below)
        assert filled.solved.all() and filled.stats["book_full"] == 0 and solver.book_size == filled.stats["book_inserts"] >= filled.stats["unique_positions"]
        r = solver.solve(pos)
        # every child of a task is a position of `below` or answered by the rules: a book leaf, so each null window of a task is one visit
        assert r.stats["tasks"] > 0 and r.stats["launches"] > 0 and r.stats["nodes"] <= 8 * r.stats["tasks"]
        plain = bookless.solve(pos)
        print(r.stats, plain.stats)
        assert r.solved.all() and np.array_equal(r.scores, plain.scores) and np.array_equal(r.scores, want)
        mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
        m = solver.solve(mirrored)
        assert m.stats["launches"] == 0 and m.stats["book_hits_host"] > 0 and np.array_equal(m.scores, want[:, ::-1])


def test_book_persistence(tmp_path):
    pos, want = the_set()
    pos, want = pos[:50], want[:50]
    path = str(tmp_path / "book.npy")
    with _solver(book_entries=1 << 16, book_max_stones=41) as a:
        first = a.solve(pos, **SPLIT)
        assert first.solved.all() and first.stats["launches"] > 0 and first.stats["book_full"] == 0
        assert a.save_book(path) == a.book_size > 0
    with _solver(book_entries=1 << 16, book_max_stones=41) as b:
        assert b.book_size == 0
        assert b.load_book(path) == b.book_size
        r = b.solve(pos)
        assert r.stats["launches"] == 0 and np.array_equal(r.scores, want) and np.array_equal(r.scores, first.scores)
    entries = np.load(path)
    assert entries.dtype == np.uint64
    entries[3] |= np.uint64(1 << 50)
    np.save(path, entries)
    with _solver(book_entries=1 << 16, book_max_stones=41) as c:
        with pytest.raises(ValueError, match="entry 3: "):
            c.load_book(path)
        assert c.book_size == 0
    with _solver() as d:                      # a solver without a book has nowhere to put them
        with pytest.raises(ValueError, match="without a book"):
            d.load_book(path)


def _score_by_hand(samples, min_stones):
    """(non-terminal samples, those with min_stones stones or more, their solver_score) recomputed one sample at a time from the plain C
    solver's rows and Sample.policy, as tests/test_gpu_solver.py does."""
    from c4a0_amd.results import terminal_state

    live = [s for s in samples if terminal_state(s.mask, s.value) == 0]
    late = [s for s in live if bin(s.mask).count("1") >= min_stones]
    rows, _ = R.solve([(s.mask, s.value) for s in late])
    scores = [R.score_policy_row(row, s.policy) for row, s in zip(rows, late)]
    return len(live), len(late), float(np.float32(sum(scores)) / np.float32(len(scores)))


def test_solver_score_with_splitting():
    import c4a0_amd
    from helpers import hash_eval_torch

    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(48)]
    games = c4a0_amd.play_games(reqs, 64, 12, 6.6, 0.01, evaluator=hash_eval_torch)
    with _solver() as solver:
        got = games.solver_score(solver, min_stones=24, max_nodes_per_position=64, split_stones=42)
    n_live, n_late, want = _score_by_hand([s for g in games.results for s in g.samples], 24)
    assert n_late > 10
    assert got.n_unsolved == 0 and got.n_scored == n_late and got.n_scored + got.n_skipped == n_live
    assert got.score == want


def test_options_are_checked_and_the_abi_is_unchanged():
    import c4a0_amd
    from c4a0_amd import _lib

    pos, _ = the_set()
    with _solver() as solver:
        with pytest.raises(ValueError, match="split_stones"):
            solver.solve(pos[:1], split_stones=43)
        with pytest.raises(ValueError, match="split_max_tasks"):
            solver.solve(pos[:1], split_max_tasks=0)
        opt = _lib.SolverOptions(8, 0, 0, 0, 0)      # not sizeof(c4_solver_options)
        scores, solved = np.zeros((1, 7), np.int16), np.zeros(1, np.uint8)
        one = np.ascontiguousarray(pos[:1])
        st = _lib.lib().c4_solver_solve_ex(solver._h, one.ctypes.data, 1, opt, scores.ctypes.data, solved.ctypes.data, None, None)
        assert st == _lib.ERR_BAD_ARG and b"struct_size" in _lib.lib().c4_last_error_string()
        st = _lib.lib().c4_solver_solve_ex(solver._h, one.ctypes.data, 1, None, scores.ctypes.data, solved.ctypes.data, None, None)
        assert st == 0 and solved[0] == 1
        assert solver.book_size == 0
    with pytest.raises(ValueError, match="book_entries"):
        c4a0_amd.Solver(tt_entries=TT, book_entries=1000)
    with pytest.raises(ValueError, match="book_max_stones"):
        c4a0_amd.Solver(tt_entries=TT, book_entries=16, book_max_stones=42)
    assert _lib.lib().c4_abi_version() == 14
