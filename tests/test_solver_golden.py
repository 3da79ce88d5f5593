"""tests/golden/solver_rows.npz, the recorded score rows of positions with 10 to 19 stones that pin the solver's search below the
stone counts a test can solve with a reference of its own (tests/golden/make_solver_rows.py wrote it, offline): the file is what
its generator says it is, as far as seconds of CPU can tell.  No GPU needed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "golden"))
import make_solver_rows as G  # noqa: E402


def test_positions_regenerate_from_the_seeds():
    g = R.golden()
    pos, stones = G.positions()
    assert np.array_equal(g.pos, pos) and np.array_equal(g.stones, stones)
    assert G.L == R.GOLDEN_L == g.stones.min()
    for s in range(G.L, 20):                                # every stone count is there, with the number of positions the generator names
        assert (g.stones == s).sum() == {**G.TT_ONLY, **G.PLAIN}[s] == (32 if s >= 14 else 24)
        assert np.array_equal(g.pos[g.stones == s], R.playout_positions(G.SEED + s, int((g.stones == s).sum()), s, s))
    assert set(g.stones.tolist()) == set(range(G.L, 20))
    assert len(np.unique(g.pos, axis=0)) == len(g.pos)
    assert [bin(int(m)).count("1") for m in g.pos[:, 0]] == g.stones.tolist()
    assert (g.ref[g.stones >= 14] == "solve").all() and (g.ref[g.stones < 14] == "solve_tt").all()
    assert os.path.getsize(G.OUT) < 100_000


def test_rows_of_18_and_19_stones_equal_a_fresh_plain_solve():
    g = R.golden()
    pos, want = g.select(18, 19)
    assert len(pos) == 64
    got, nodes = R.solve(pos)
    assert np.array_equal(got, want)
    assert nodes == int(g.ref_nodes[g.stones >= 18].sum())


def test_a_fresh_table_solve_reproduces_rows_of_14_and_15_stones():
    """Sixteen rows the plain solver wrote, eight of either count; and every row the table solver wrote that costs it under 2 M nodes,
    with its node count."""
    g = R.golden()
    for s in (14, 15):
        pos, want = g.select(s, s)
        assert np.array_equal(R.solve_tt(pos[:8])[0], want[:8])
    cheap = (g.ref == "solve_tt") & (g.ref_nodes < 2_000_000)
    assert cheap.sum() >= 24
    for p, want, nodes in zip(g.pos[cheap], g.rows[cheap], g.ref_nodes[cheap]):
        got, n = R.solve_tt([p])
        assert np.array_equal(got[0], want) and n == int(nodes)


def test_the_large_scores_are_in_the_set():
    g = R.golden()
    for s in range(G.L, 20):
        rows = g.rows[g.stones == s]
        legal = rows[rows != R.FULL_COLUMN]
        bound = (43 - s) // 2
        assert np.abs(legal).max() <= bound
        assert legal.max() >= bound - 2 and legal.min() <= -(bound - 2), (s, int(legal.min()), int(legal.max()))
    # beyond what a 20-stone position can hold: the values the clamps, the window bytes and the table bytes never saw before
    assert (np.abs(g.rows[(g.stones <= 16)][g.rows[g.stones <= 16] != R.FULL_COLUMN]) > 11).sum() > 100
    # the rules every row obeys, whatever wrote it: a full column where the mask says so, and nothing else out of range
    full = np.array([[(int(m) >> (35 + c)) & 1 for c in range(7)] for m in g.pos[:, 0]], dtype=bool)
    assert np.array_equal(g.rows == R.FULL_COLUMN, full)
