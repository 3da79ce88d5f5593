"""The GPU solver below 20 stones (c4a0_amd.Solver: solver_kernel<false> and <true>, the stack store, splitting and the device book,
c4a0_amd/csrc/c4_solver.hip) against the recorded rows of tests/golden/solver_rows.npz: 12 to 19 stones, where scores reach +-15, a
task's stack 28 frames and the book is probed at the stone counts it is meant for.  The file is loaded, never regenerated, and no
reference runs here (tests/test_solver_golden.py checks the file on the CPU; tests/test_solver_core_host.py puts the same rows, and
those of 10 and 11 stones, through the CPU build of the search).  Every Solver has a table of at most 2^20 entries.  No test may leave
a position unsolved; where an input is narrowed, then only by the reference's node count (`ref_nodes`), with a fixed cutoff."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

from tests.helpers import evidence  # noqa: E402

pytestmark = pytest.mark.gpu

TT = 1 << 20


def _solver(tt_entries=TT, **kw):
    import c4a0_amd

    return c4a0_amd.Solver(tt_entries=tt_entries, **kw)


def _line(tag, pos, r):
    keys = ("nodes", "launches", "tasks", "split_tasks", "book_inserts")
    evidence(f"solver below 20 stones, {tag}: {len(pos)} golden rows equal, " + ", ".join(f"{k} {r.stats[k]}" for k in keys))


@pytest.mark.parametrize("stones", [14, 15, 16, 17, 18, 19])
def test_default_budgets_equal_golden_rows(stones):
    """All 32 rows of the count, a fresh Solver each.  Measured on an MI355X: 19 stones 0.17 s, 18: 0.18 s, 17: 0.25 s, 16: 0.43 s,
    15: 2.1 s (4.2 M visits, 128 launches), 14: 2.3 s (3.6 M visits, 178 launches): no count is narrowed."""
    pos, want = R.golden().select(stones, stones)
    assert len(pos) == 32
    with _solver() as solver:
        r = solver.solve(pos)
    print(r.stats)
    assert r.solved.all() and r.stats["unsolved_tasks"] == 0 and r.stats["split_tasks"] == 0
    assert np.array_equal(r.scores, want)
    assert np.array_equal(r.best_moves_mask(), want == want.max(axis=1, keepdims=True))
    assert np.array_equal(r.winning_moves_mask(), want > 0)
    legal = want[want != R.FULL_COLUMN]
    assert np.abs(legal).max() >= (43 - stones) // 2 - 2          # the large scores are in what was compared
    _line(f"{stones} stones, default budgets", pos, r)


def test_relaunches_with_deep_saved_stacks():
    pos, want = R.golden().select(16, 19)
    assert len(pos) == 128
    with _solver() as solver:
        r = solver.solve(pos, nodes_per_launch=64)
    print(r.stats)
    assert r.solved.all() and np.array_equal(r.scores, want)
    assert r.stats["launches"] > 1
    _line("16-19 stones, 64 visits a launch", pos, r)


def test_small_table_every_store_evicts():
    pos, want = R.golden().select(16, 19)
    with _solver(1 << 10) as solver:
        r = solver.solve(pos)
    print(r.stats)
    assert r.solved.all() and np.array_equal(r.scores, want)
    _line("16-19 stones, a table of 2^10", pos, r)


# (d) ref_nodes cutoffs and the budget of a task.  Under the default budget of 2^20 visits a task that splits has spent 8 s or more
# before it does; BUDGET_D is the smaller measured one.  12-stone rows the table solver needed at most 4.5 M nodes for (14 of 24) and
# 13-stone rows of at most 2.7 M (17 of 24): on the CPU build one 13-stone task of theirs needs 941 936 visits and splits into 6 tasks
# of 14 stones, which may not split under split_stones=14; every other task needs at most 234 278.
# Measured on an MI355X: 4.3 s, 4.09 M visits, 276 launches, 91 tasks, 6 of them made by splitting, 122 book entries -- the CPU build's
# figures to within a tenth.  Under 2^18 visits one of the six 14-stone tasks does not finish (3.2 s, one position unsolved), on the
# CPU build as on the GPU: the budget has less than a factor of two to spare, and splitting under a larger one takes longer than 5 s.
CUT_D = {12: 4_500_000, 13: 2_700_000}
BUDGET_D = 1 << 19


def test_splitting_and_the_device_book_at_12_and_13_stones():
    g = R.golden()
    pos = np.concatenate([g.select(s, s, CUT_D[s])[0] for s in (12, 13)])
    want = np.concatenate([g.select(s, s, CUT_D[s])[1] for s in (12, 13)])
    assert len(pos) == 14 + 17
    budget = dict(max_nodes_per_position=BUDGET_D, split_stones=14)
    with _solver(book_entries=1 << 20) as solver:
        r = solver.solve(pos, **budget)
        print(r.stats)
        assert r.solved.all() and r.stats["unsolved_tasks"] == 0 and np.array_equal(r.scores, want)
        assert r.stats["split_tasks"] > 0
        assert r.stats["book_inserts"] > 0 and r.stats["book_full"] == 0 and solver.book_size == r.stats["book_inserts"]
        again = solver.solve(pos, **budget)
        assert again.stats["launches"] == 0 and again.solved.all() and np.array_equal(again.scores, want)
        mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
        m = solver.solve(mirrored, **budget)
        assert m.stats["launches"] == 0 and np.array_equal(m.scores, want[:, ::-1])
    _line("12-13 stones, split_stones=14 and a book", pos, r)


def _descendants(pos, depth):
    """The distinct non-terminal positions `depth` stones below `pos`."""
    from c4a0_amd.solver import is_terminal

    level = {tuple(p) for p in pos.tolist()}
    for _ in range(depth):
        nxt = np.array(sorted({R.play(m, v, c) for m, v in level for c in R.legal(m)}), dtype=np.uint64)
        level = {tuple(p) for p in nxt[~is_terminal(nxt[:, 0], nxt[:, 1])].tolist()}
    return np.array(sorted(level), dtype=np.uint64)


def test_the_kernel_reads_the_book_at_14_stones():
    """The recipe of tests/test_gpu_solver_split.py::test_the_kernel_reads_the_book, ten stones further down: the first 24 golden
    positions of 14 stones, the book filled with every position two stones below them."""
    pos, want = R.golden().select(14, 14)
    pos, want = pos[:24], want[:24]
    below = _descendants(pos, 2)
    assert all(bin(int(m)).count("1") == 16 for m in below[:, 0])
    with _solver(book_entries=1 << 16, book_max_stones=16) as solver, _solver() as bookless:
        filled = solver.solve(below)
        assert filled.solved.all() and filled.stats["book_full"] == 0
        assert solver.book_size == filled.stats["book_inserts"] >= filled.stats["unique_positions"]
        r = solver.solve(pos)
        # every child of a task is a position of `below` or answered by the rules: a book leaf, so each null window of a task is one visit
        assert r.stats["tasks"] > 0 and r.stats["launches"] > 0 and r.stats["nodes"] <= 8 * r.stats["tasks"]
        plain = bookless.solve(pos)
        print(filled.stats, r.stats, plain.stats)
        assert r.solved.all() and plain.solved.all()
        assert np.array_equal(r.scores, want) and np.array_equal(r.scores, plain.scores)
    _line(f"14 stones over a book of {len(below)} positions of 16", pos, r)


# (f) a budget of 2^16 visits a task under 256 a launch: on the CPU build 1 491 tasks are made by splitting while others wait in the
# stack store with up to 256 launches' worth of saved stacks.  Measured on an MI355X: 3.9 s, 47.2 M visits, 1 822 launches, 1 620 tasks
# made by splitting; under 2^15 visits 43 683 tasks and 3.1 s.
BUDGET_F = 1 << 16


def test_the_stack_store_grows_with_saved_stacks_in_it():
    pos, want = R.golden().select(14, 15)
    assert len(pos) == 64
    with _solver() as solver:
        r = solver.solve(pos, nodes_per_launch=256, max_nodes_per_position=BUDGET_F, split_stones=42, split_max_tasks=1 << 20)
    print(r.stats)
    assert r.solved.all() and np.array_equal(r.scores, want)
    assert r.stats["split_tasks"] > 0 and r.stats["launches"] > 2
    _line("14-15 stones, splits under 256 visits a launch", pos, r)
