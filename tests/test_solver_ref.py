"""The plain C solver (tests/solver_ref.c), the checker of the GPU solver, pinned on the CPU: against a pruning-free brute force in
the same file, on hand-checkable positions; its variant with a transposition table (solve_tt, which writes the recorded rows below 14
stones) against both; and Solution::score_policy (reference rust/src/solver.rs:201-228) against the
product's host arithmetic on given score rows (c4a0_amd.solver.score_rows).  No GPU needed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

from c4a0_amd.results import _has_four  # noqa: E402
from c4a0_amd.solver import FULL_COLUMN, UNSOLVED, score_rows  # noqa: E402


def test_alpha_beta_equals_brute_force():
    """(a) a few hundred random reachable positions with at least 32 stones: pruning changes no score."""
    pos = R.playout_positions(7, 400, 32)
    got, _nodes = R.solve(pos)
    want = R.brute(pos)
    assert np.array_equal(got, want)
    k = R.kinds(pos, got)
    assert min(k.values()) > 0, k          # the set has immediate wins, full columns, 41 stones, single legal moves
    assert (got[got != FULL_COLUMN] != 0).any() and (got == 0).any()


def test_table_solver_equals_brute_force():
    """solve_tt, the checker of the stone counts `solve` cannot reach, on the set of (a): its table changes no score."""
    pos = R.playout_positions(7, 400, 32)
    got, nodes = R.solve_tt(pos)
    assert np.array_equal(got, R.brute(pos)) and 0 < nodes <= R.solve(pos)[1]


def test_table_solver_equals_plain_solver_from_20_stones():
    """The 2 000 positions of 20 or more stones the GPU tests use (tests/test_gpu_solver.py): the plain solver takes about 5 s."""
    pos = R.playout_positions(20261019, 2000, 20)
    want, plain_nodes = R.solve(pos)
    got, nodes = R.solve_tt(pos)
    assert np.array_equal(got, want)
    assert nodes < plain_nodes                                        # measured: 7 773 314 against 111 567 507
    # a row and its node count depend on nothing solved before it: one at a time, in another order, the same
    one_by_one = [R.solve_tt(pos[i:i + 1]) for i in (1999, 7, 0)]
    assert np.array_equal(np.concatenate([r for r, _ in one_by_one]), want[[1999, 7, 0]])
    assert sum(n for _, n in one_by_one) == sum(R.solve_tt(pos[[i]])[1] for i in (0, 7, 1999))
    assert R.solve_tt(pos[:50])[1] == sum(R.solve_tt(pos[i:i + 1])[1] for i in range(50))


@pytest.mark.slow
def test_table_solver_equals_plain_solver_at_16_stones():
    """24 positions of 16 stones: about 25 s of plain solver, scores up to +-13."""
    pos = R.playout_positions(77 + 16, 24, 16, 16)
    want, _ = R.solve(pos)
    got, _ = R.solve_tt(pos)
    assert np.array_equal(got, want)
    assert np.abs(want[want != FULL_COLUMN]).max() == 13


def test_table_solver_edges():
    assert np.array_equal(R.solve_tt([R.from_moves([2, 2, 3, 3, 4])])[0], R.solve([R.from_moves([2, 2, 3, 3, 4])])[0])
    pos = R.playout_positions(13, 200, 28)
    rows, _ = R.solve_tt(pos)
    mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
    assert np.array_equal(R.solve_tt(mirrored)[0], rows[:, ::-1]) and np.array_equal(rows, R.solve(pos)[0])
    late = R.playout_positions(11, 40, 41)
    assert np.array_equal(R.solve_tt(late)[0], R.brute(late))
    assert R.solve_tt(np.zeros((0, 2), np.uint64))[0].shape == (0, 7)


def test_immediate_win_scores_43_minus_s_halved():
    late = [(m, v, None) for m, v in R.playout_positions(3, 30, 30).tolist()]
    # the hand-made one: three stones in column 0 against an open three on the bottom row -- column 0 wins now, after any other move the
    # opponent does (every child is answered at its root, so the plain solver has nothing to search at six stones)
    for mask, value, col in [(*R.from_moves([0, 2, 0, 3, 0, 4]), 0)] + late:
        s = bin(mask).count("1")
        row = R.solve([(mask, value)])[0][0]
        wins = [c for c in R.legal(mask) if _has_four((lambda m, v: m & ~v)(*R.play(mask, value, c)))]
        assert col is None or wins == [col]
        for c in R.legal(mask):
            assert (row[c] == (43 - s) // 2) == (c in wins)      # that score, and only for a move that wins with this stone


def test_41_stones_last_move_without_a_win_is_a_draw():
    pos = R.playout_positions(11, 40, 41)
    rows, _ = R.solve(pos)
    seen = 0
    for (mask, value), row in zip(pos.tolist(), rows):
        (col,) = R.legal(mask)
        assert (np.delete(row, col) == FULL_COLUMN).all()          # six full columns
        m2, v2 = R.play(mask, value, col)
        if _has_four(m2 & ~v2):
            assert row[col] == 1                                    # (43 - 41) / 2
        else:
            assert row[col] == 0
            seen += 1
    assert seen > 0


def test_every_move_loses_at_once():
    """Three in a row on the bottom with both ends open: whatever the side to move does, the opponent wins with the next stone."""
    moves = [2, 2, 3, 3, 4]
    mask, value = R.from_moves(moves)
    s = len(moves)
    row = R.solve([(mask, value)])[0][0]
    assert (row == -((42 - s) // 2)).all(), row


def test_mirrored_position_gives_reversed_row():
    pos = R.playout_positions(13, 200, 28)
    rows, _ = R.solve(pos)
    mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
    assert (mirrored != pos).any()
    assert np.array_equal(R.solve(mirrored)[0], rows[:, ::-1])


# (c) Solution::score_policy: (score row, policy, expected) -- the table of solver.rs:221-227
CASES = [
    ([0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], 1.0),                       # the best move
    ([0, 0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], 0.0),                       # a drawing move where a win exists
    ([-2, 5, 3, 3, 5, -1, FULL_COLUMN], [0, 0, 1, 0, 0, 0, 0], 0.5),           # winning, not best
    ([-2, 5, 3, 3, 5, -1, FULL_COLUMN], [0, 0, 0, 0, 1, 0, 0], 1.0),           # one of two best moves
    ([-2, 5, 3, 3, 5, -1, FULL_COLUMN], [1, 0, 0, 0, 0, 0, 0], 0.0),           # a losing move
    ([-2, 5, 3, 3, 5, -1, FULL_COLUMN], [0, 0, 0, 0, 0, 0, 1], 0.0),           # a full column
    ([-2, 5, 3, 3, 5, -1, FULL_COLUMN], [0.2, 0.3, 0.1, 0.1, 0.3, 0, 0], 1.0),  # a tie in the policy: the FIRST maximum, column 1
    ([5, -2, 3, 3, -1, 5, FULL_COLUMN], [0.1, 0.3, 0.1, 0.1, 0.1, 0.3, 0], 0.0),  # ... column 1 again, here a losing move
    ([-2, 3, 3, 5, -1, 5, FULL_COLUMN], [0, 0.4, 0.4, 0.2, 0, 0, 0], 0.5),     # ... column 1: winning, not best
    ([-3, -1, -5, -1, FULL_COLUMN, -7, -2], [0, 1, 0, 0, 0, 0, 0], 1.0),       # the maximum is negative: the least bad move is best
    ([-3, -1, -5, -1, FULL_COLUMN, -7, -2], [0, 0, 0, 1, 0, 0, 0], 1.0),
    ([-3, -1, -5, -1, FULL_COLUMN, -7, -2], [1, 0, 0, 0, 0, 0, 0], 0.0),
    ([0, 0, -1, 0, -2, FULL_COLUMN, 0], [0, 0, 0, 0, 0, 0, 1], 1.0),           # a draw is best
    ([0, 0, -1, 0, -2, FULL_COLUMN, 0], [0, 0, 1, 0, 0, 0, 0], 0.0),
    ([0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], 1.0),                       # an all-zero policy selects column 0
]


def test_score_policy_table():
    rows = np.array([c[0] for c in CASES], dtype=np.int16)
    pol = np.array([c[1] for c in CASES], dtype=np.float32)
    want = np.array([c[2] for c in CASES], dtype=np.float32)
    assert np.array_equal(score_rows(rows, pol), want)
    assert [R.score_policy_row(r, p) for r, p in zip(rows, pol)] == want.tolist()      # the line-for-line restatement agrees with the table


def test_score_policy_on_random_rows_and_unsolved():
    rng = np.random.default_rng(5)
    rows = rng.integers(-6, 7, size=(500, 7)).astype(np.int16)
    rows[rng.random((500, 7)) < 0.15] = FULL_COLUMN
    rows[:, 3][(rows == FULL_COLUMN).all(axis=1)] = 0
    pol = rng.integers(0, 4, size=(500, 7)).astype(np.float32)        # many ties
    want = np.array([R.score_policy_row(r, p) for r, p in zip(rows, pol)], dtype=np.float32)
    assert np.array_equal(score_rows(rows, pol), want)
    assert set(want.tolist()) == {0.0, 0.5, 1.0}
    rows[::7] = UNSOLVED
    got = score_rows(rows, pol)
    assert np.isnan(got[::7]).all() and np.array_equal(np.delete(got, np.s_[::7]), np.delete(want, np.s_[::7]))
    assert score_rows(np.zeros((0, 7), np.int16), np.zeros((0, 7), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        score_rows(rows, pol[:-1])


def test_reference_kats_as_rows():
    """The reference's own expectations (solver.rs:271-306) follow from score rows of that shape: one-hot policies against a row."""
    def one_hots(row):
        return score_rows(np.tile(np.array(row, dtype=np.int16), (7, 1)), np.eye(7, dtype=np.float32)).tolist()
    assert one_hots([-2, -1, 0, 1, 0, -1, -2]) == [0, 0, 0, 1, 0, 0, 0]             # the empty board's known solution
