"""The GPU solver (c4a0_amd.Solver: c4_solver_create / c4_solver_solve, c4a0_amd/csrc/c4_solver.hip) against the plain C solver
(tests/solver_ref.c, pinned on the CPU by tests/test_solver_ref.py): exact equality of every score, under the default launch budget,
a launch budget of 64 node visits, a table of 2^10 entries and a budget too small for some positions; the edge shapes; and
`solver_score` of real results recomputed sample by sample.  Every Solver here has a table of at most 2^16 entries.  20 stones is
the floor of this file only, set by what the plain solver can do inside a test: tests/test_gpu_solver_low_stones.py goes on down to 12
stones against recorded rows (tests/golden/solver_rows.npz)."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# S: the lowest stone count at which the plain C solver finishes the 2 000 positions below in under 10 s (and no higher than 24).
# Measured on the CPU with these very positions: S = 20 -> 5.2 s, 111 567 507 nodes; S = 19 -> 19.3 s, 464 117 078 nodes.
S = 20
N_POSITIONS = 2000
TT = 1 << 16


@functools.lru_cache(maxsize=None)
def the_set():
    """(positions uint64[2000, 2], the plain C solver's rows int16[2000, 7]): computed once, shared, never written to."""
    pos = R.playout_positions(20261019, N_POSITIONS, S)
    rows, _nodes = R.solve(pos)
    pos.setflags(write=False)
    rows.setflags(write=False)
    return pos, rows


def _solver(tt_entries=TT):
    import c4a0_amd

    return c4a0_amd.Solver(tt_entries=tt_entries)


def test_parity_with_the_plain_solver():
    """S = 20; the plain solver's node total on the set is 111 567 507 (the GPU search, with its table, threat rules and move order,
    expands about 0.8 M)."""
    pos, want = the_set()
    assert len(np.unique(pos, axis=0)) == N_POSITIONS
    assert (np.array([bin(int(m)).count("1") for m in pos[:, 0]]) >= S).all()
    k = R.kinds(pos, want)
    assert min(k.values()) > 0, k      # immediate wins, full columns, 41-stone positions, a single legal move: each kind is there
    with _solver() as solver:
        r = solver.solve(pos)
    assert r.solved.all() and r.stats["unsolved_tasks"] == 0
    assert r.scores.dtype == np.int16 and r.scores.shape == (N_POSITIONS, 7)
    assert np.array_equal(r.scores, want)
    assert r.stats["tasks"] > 0 and r.stats["probes"] >= r.stats["nodes"] > 0
    assert np.array_equal(r.best_moves_mask(), want == want.max(axis=1, keepdims=True))
    assert np.array_equal(r.winning_moves_mask(), want > 0)


def test_small_launch_budget_many_relaunches():
    pos, want = the_set()
    with _solver() as solver:
        r = solver.solve(pos, nodes_per_launch=64)
    assert r.solved.all() and np.array_equal(r.scores, want)
    # 64 visits finish few searches of 20-stone positions: the unfinished tasks went on launch after launch, on whichever lane took them
    assert r.stats["launches"] > 1


def test_small_table_every_store_evicts():
    pos, want = the_set()
    with _solver(1 << 10) as solver:
        r = solver.solve(pos)
    assert r.solved.all() and np.array_equal(r.scores, want)


def test_budget_exhaustion_is_all_or_nothing_and_a_second_call_finishes():
    pos = R.playout_positions(99, 15, 16, 20)        # three positions of each stone count 16..20
    want, _ = R.solve(pos)
    with _solver() as solver:
        r = solver.solve(pos, nodes_per_launch=100, max_nodes_per_position=300)      # returns normally
        assert 0 < r.solved.sum() < len(pos)                                        # both kinds occur
        assert r.stats["unsolved_tasks"] > 0
        assert np.array_equal(r.scores[r.solved], want[r.solved])
        assert (r.scores[~r.solved] == R.UNSOLVED).all()                            # never a mixture
        assert not r.best_moves_mask()[~r.solved].any() and not r.winning_moves_mask()[~r.solved].any()
        assert np.isnan(r.score_policies(np.ones((len(pos), 7), np.float32))[~r.solved]).all()
        again = solver.solve(pos)                                                   # the same Solver, the full budget
    assert again.solved.all() and np.array_equal(again.scores, want)


def test_edge_shapes():
    import c4a0_amd

    pos, want = the_set()
    a, b = _solver(), _solver(1 << 12)                 # two Solvers in one process
    try:
        for n in (1, 63, 64, 65):
            r = (a if n % 2 else b).solve(pos[:n])
            assert r.solved.all() and np.array_equal(r.scores, want[:n])
        r = a.solve(np.zeros((0, 2), dtype=np.uint64))
        assert r.scores.shape == (0, 7) and r.solved.shape == (0,) and r.stats["launches"] == 0
        assert r.best_moves_mask().shape == (0, 7) and a.score_policies([], np.zeros((0, 7), np.float32)).shape == (0,)
        # duplicates and mirrored pairs: equal and reversed rows, solved once
        base = pos[100:140]
        mirrored = np.array([R.mirror(m, v) for m, v in base.tolist()], dtype=np.uint64)
        r = b.solve(np.concatenate([base, mirrored, base]))
        assert np.array_equal(r.scores[:40], want[100:140]) and np.array_equal(r.scores[80:], want[100:140])
        assert np.array_equal(r.scores[40:80], want[100:140][:, ::-1])
        assert r.stats["unique_positions"] <= 40
        # refused by name
        won = R.from_moves([3, 0, 3, 0, 3, 0, 3])
        with pytest.raises(ValueError, match="position 1: the position is terminal"):
            a.solve([tuple(pos[0].tolist()), won])
        with pytest.raises(ValueError, match="position 0: a stone above an empty cell"):
            a.solve([(1 << 7, 0)])
        with pytest.raises(ValueError, match="value has bits outside mask"):
            a.solve([(1, 2)])
        with pytest.raises(ValueError, match="nodes_per_launch"):
            a.solve(pos[:1], nodes_per_launch=0)
        # ... by the library too, for a caller that comes through the C ABI
        from c4a0_amd import _lib
        bad = np.array([pos[0].tolist(), list(won)], dtype=np.uint64)
        scores, solved = np.zeros((2, 7), np.int16), np.zeros(2, np.uint8)
        st = _lib.lib().c4_solver_solve(a._h, bad.ctypes.data, 2, 0, 0, scores.ctypes.data, solved.ctypes.data, None, None)
        assert st == _lib.ERR_BAD_ARG and b"position 1: the position is terminal" in _lib.lib().c4_last_error_string()
        with pytest.raises(ValueError):
            c4a0_amd.Solver(tt_entries=1000)
    finally:
        a.close()
        a.close()                                      # twice is harmless
        b.close()
    with pytest.raises(RuntimeError, match="closed"):
        a.solve(pos[:1])
    assert _lib.lib().c4_abi_version() == 14


def _score_by_hand(samples, min_stones):
    """(non-terminal samples, those with min_stones stones or more, their solver_score) recomputed one sample at a time from the plain
    C solver's rows and Sample.policy."""
    from c4a0_amd.results import terminal_state

    live = [s for s in samples if terminal_state(s.mask, s.value) == 0]
    late = [s for s in live if bin(s.mask).count("1") >= min_stones]
    rows, _ = R.solve([(s.mask, s.value) for s in late])
    scores = [R.score_policy_row(row, s.policy) for row, s in zip(rows, late)]
    return len(live), len(late), float(np.float32(sum(scores)) / np.float32(len(scores)))


def test_solver_score_of_played_games_and_of_a_search():
    import c4a0_amd
    from helpers import hash_eval_torch

    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(48)]
    games = c4a0_amd.play_games(reqs, 64, 12, 6.6, 0.01, evaluator=hash_eval_torch)
    assert games._lazy is not None
    with _solver() as solver:
        got = games.solver_score(solver, min_stones=S)
        assert games._lazy is not None                         # scored on the records: no Sample was built
        n_live, n_late, want = _score_by_hand([s for g in games.results for s in g.samples], S)
        assert n_late > 20
        assert got.n_unsolved == 0 and got.n_scored == n_late and got.n_scored + got.n_skipped == n_live
        assert got.score == want and 0.0 <= got.score <= 1.0
        assert isinstance(got, c4a0_amd.SolverScore) and got == tuple(got)
        # nothing to score: NaN, as the reference's 0.0 / 0
        none = games.solver_score(solver, min_stones=43)
        assert np.isnan(none.score) and none[1:] == (0, 0, n_live)
        # the same on a SearchResult: root policies of searched positions
        pos, _ = the_set()
        found = c4a0_amd.search_positions(pos[:96], 16, 6.6, 0.01, evaluator=hash_eval_torch)
        got = found.solver_score(solver, min_stones=S + 2)
        n_live, n_late, want = _score_by_hand(found.samples(), S + 2)
        assert got.n_unsolved == 0 and got.n_scored == n_late and got.n_scored + got.n_skipped == n_live == 96
        assert got.score == want
    with pytest.raises(NotImplementedError, match="solver_score"):
        games.score_policies("a", "b", "c")
