"""`search_positions` without a device: the floors of the fixture that tests/test_gpu_search_positions.py compares the kernels on
(tests/search_ref.py: the oracle's MctsGame searched as mcts.rs' run_mcts searches it, over tests.helpers.start_job's 495
positions), `SearchResult` on hand-made records, and the validation that runs before any device call.

The floors are the oracle's own figures (c_ply_penalty 0.01), asserted exactly: a fixture that stopped expanding, stayed shallow or
produced no peaked policy would make the bit-for-bit comparison on the device mean little."""
import numpy as np
import pytest

from tests.helpers import START_EVALS, start_job
from tests.search_ref import C_PLY_PENALTY, oracle_evaluator, search, start_job_search

# (evaluator, n): expansions, max depth, simulations below level 16 (None: not held), one-hot policies, policies with a zero column (None: not held)
FLOORS = {
    ("hash", 24): (6_621, 10, None, 37, 443),
    ("hash", 100): (20_984, 15, None, 30, 432),
    ("k4sat", 24): (5_555, 15, None, 106, None),
    ("k5sat", 100): (17_060, 33, 2_670, 90, None),
}


def test_the_job_is_what_the_issue_says():
    from oracle import c4oracle as O

    _reqs, starts, part = start_job()
    assert len(starts) == 495 and len(set(starts)) == 386
    assert sum(O.terminal_state(O.Pos(*p)) != 0 for p in starts) == 45
    assert part.count("won") == 1 and part.count("line") == 14
    assert {name: START_EVALS[name][1] for name, _n in FLOORS} == {"hash": 6.6, "k4sat": 6.6, "k5sat": 1.4}


@pytest.mark.parametrize("ev_name,n", list(FLOORS), ids=[f"{e}-n{n}" for e, n in FLOORS])
def test_fixture_floors(ev_name, n):
    expansions, max_depth, deep, one_hot, zero_col = FLOORS[(ev_name, n)]
    ref = start_job_search(ev_name, n)
    pol = ref["policy"]
    got = (int(ref["expansions"].sum()), int(ref["max_depth"].max()), int(ref["sims_deep"].sum()), int((pol.max(axis=1) == 1.0).sum()),
           int((pol == 0.0).any(axis=1).sum()))
    print(f"{ev_name} n={n}: expansions {got[0]}, max depth {got[1]}, sims below level 16 {got[2]}, one-hot {got[3]}, zero column {got[4]}")
    assert got[0] == expansions and got[1] == max_depth and got[3] == one_hot
    assert deep is None or got[2] == deep
    assert zero_col is None or got[4] == zero_col
    assert ref["n_expansions"] == expansions and ref["sims"] == 495 * n
    # every policy is a distribution over the legal columns (or uniform: a root without visited children)
    assert np.all(np.abs(pol.sum(axis=1) - 1.0) < 1e-6)


def test_one_simulation_leaves_every_policy_uniform():
    ref = start_job_search("hash", 1)
    uniform = np.full((495, 7), np.float32(1.0) / np.float32(7.0), dtype=np.float32)
    assert ref["policy"].tobytes() == uniform.tobytes()
    assert ref["select"] == 0


def test_the_won_root_is_searched_not_closed():
    """Pos(0b1111, 0b1111) at n = 100: q_sum / (n + 1) of 100 terminal values, not the terminal value 0.96 / 1.0"""
    ref = search([(0b1111, 0b1111)], 100, oracle_evaluator("hash"), 6.6, C_PLY_PENALTY)
    assert ref["q_penalty"][0] == np.float32(0.95049429) and ref["q_no_penalty"][0] == np.float32(0.99009901)
    assert ref["policy"][0].tobytes() == np.full(7, np.float32(1.0) / np.float32(7.0), dtype=np.float32).tobytes()
    assert ref["n_expansions"] == 0 and ref["backup"] == 0 and ref["select"] == 0
    _reqs, starts, part = start_job()
    job = start_job_search("hash", 100)
    i = part.index("won")
    assert starts[i] == (0b1111, 0b1111) and job["q_penalty"][i] == ref["q_penalty"][0] and job["q_no_penalty"][i] == ref["q_no_penalty"][0]


# ------------------------------------------------------------------------------------------------ SearchResult
def _records(n=5):
    from c4a0_amd.results import RECORD_DTYPE, SEARCH_RECORD_META

    recs = np.zeros(n, dtype=RECORD_DTYPE)
    recs["game_id"] = np.arange(n)
    recs["mask"] = [0, 0b1, 0b10000001, 0b1111, (1 << 42) - 1][:n]
    recs["value"] = [0, 0b1, 0b1, 0b1111, 0x15555555555][:n]
    recs["policy"] = np.array([[1 / 7] * 7, [0, 0.5, 0.5, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1], [0.25, 0.125, 0.25, 0.125, 0.25, 0, 0],
                               [0, 0, 0, 0.3, 0.2, 0.3, 0.2]], dtype=np.float32)[:n]
    recs["q_penalty"] = np.array([0.0, -0.0, 0.5, 0.95049429, -1.0], dtype=np.float32)[:n]
    recs["q_no_penalty"] = np.array([0.25, 0.0, -0.5, 0.99009901, 1.0], dtype=np.float32)[:n]
    recs["meta"] = SEARCH_RECORD_META
    return recs


def test_search_result_reads_the_records():
    import c4a0_amd
    from c4a0_amd.results import RECORD_DTYPE, Sample, SearchResult
    from c4a0_amd.session import SAMPLE_DTYPE

    assert RECORD_DTYPE == SAMPLE_DTYPE and SearchResult.DTYPE == SAMPLE_DTYPE
    assert c4a0_amd.SearchResult is SearchResult and callable(c4a0_amd.search_positions)
    recs = _records()
    r = SearchResult(recs)
    assert len(r) == 5 and r.records is not None and r.records.tobytes() == recs.tobytes()
    assert r.mask.dtype == np.uint64 and r.value.dtype == np.uint64 and r.policy.shape == (5, 7) and r.policy.dtype == np.float32
    assert np.array_equal(r.mask, recs["mask"]) and np.array_equal(r.value, recs["value"])
    assert r.q_penalty.tobytes() == recs["q_penalty"].tobytes() and r.q_no_penalty.tobytes() == recs["q_no_penalty"].tobytes()
    # ties go to the first column of the maximum (Solution::score_policy)
    assert r.best_moves().tolist() == [0, 1, 6, 0, 3] and r.best_moves().dtype == np.int64
    # samples() round-trips: one Sample per position, the record's bits
    ss = r.samples()
    assert len(ss) == 5 and all(isinstance(s, Sample) for s in ss)
    for s, rec in zip(ss, recs):
        assert s == Sample(int(rec["mask"]), int(rec["value"]), rec["policy"], rec["q_penalty"], rec["q_no_penalty"])
    back = np.zeros(5, dtype=RECORD_DTYPE)
    for i, s in enumerate(ss):
        back[i] = (i, s.mask, s.value, s.policy, s.q_penalty, s.q_no_penalty, 2 << 16)
    assert back.tobytes() == recs.tobytes()
    # equality is on the bytes: -0.0 is not 0.0
    assert r == SearchResult(recs.copy()) and SearchResult(recs.view(np.uint8).reshape(5, 64)) == r
    other = recs.copy()
    other["q_penalty"][1] = 0.0
    assert r != SearchResult(other) and r != recs
    assert len(SearchResult(recs[:0])) == 0 and SearchResult(recs[:0]).best_moves().shape == (0,) and SearchResult(recs[:0]).samples() == []
    with pytest.raises(TypeError):
        SearchResult(np.zeros((5, 7), dtype=np.float32))


# ------------------------------------------------------------------------------------------------ validation, before any device call
def _no_device(monkeypatch):
    """search_positions must refuse bad arguments before it touches the library or a device"""
    from c4a0_amd import api

    def boom(*_a, **_k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(api, "_play_locked", boom)
    monkeypatch.setattr(api, "lib", boom)
    return api.search_positions


def _ev(planes):
    raise AssertionError("the evaluator was called")


GOOD = [(0, 0), (0b1, 0b1), (0b10000001, 0b1), (0b1111, 0b1111)]


@pytest.mark.parametrize("bad,what", [
    ((1 << 42, 0), "bits outside the 42 cells"),
    ((0b1, 0b1 | 1 << 63), "bits outside the 42 cells"),
    ((0b1, 0b11), "value has bits outside mask"),
    ((1 << 7, 0), "a stone above an empty cell"),
    ((0b1 | 1 << 14, 0b1), "a stone above an empty cell"),
])
@pytest.mark.parametrize("as_array", [False, True], ids=["sequence", "array"])
def test_invalid_positions_are_refused_with_their_index(monkeypatch, bad, what, as_array):
    search_positions = _no_device(monkeypatch)
    positions = GOOD[:3] + [bad] + GOOD[3:]
    if as_array:
        positions = np.array(positions, dtype=np.uint64)
    with pytest.raises(ValueError, match=f"position 3: {what}"):
        search_positions(positions, 24, 6.6, 0.01, evaluator=_ev)


def test_invalid_arguments_are_refused(monkeypatch):
    search_positions = _no_device(monkeypatch)
    for n in (0, -1):
        with pytest.raises(ValueError, match="n_mcts_iterations"):
            search_positions(GOOD, n, 6.6, 0.01, evaluator=_ev)
    with pytest.raises(TypeError, match="ONE device evaluator"):
        search_positions(GOOD, 24, 6.6, 0.01, evaluator={0: _ev})
    with pytest.raises(TypeError, match="ONE device evaluator"):
        search_positions(GOOD, 24, 6.6, 0.01)
    with pytest.raises(TypeError):
        search_positions(np.zeros((4, 3), dtype=np.uint64), 24, 6.6, 0.01, evaluator=_ev)
    with pytest.raises(TypeError):
        search_positions(np.zeros((4, 2), dtype=np.float32), 24, 6.6, 0.01, evaluator=_ev)
    with pytest.raises(ValueError, match="position 1: negative"):
        search_positions(np.array([[0, 0], [-1, 0]], dtype=np.int64), 24, 6.6, 0.01, evaluator=_ev)
    # nothing to search: an empty result, still without a device
    assert len(search_positions([], 24, 6.6, 0.01, evaluator=_ev)) == 0


def test_every_position_of_the_job_is_valid():
    from c4a0_amd.api import _positions_array

    _reqs, starts, _part = start_job()
    pos = _positions_array(starts)
    assert pos.dtype == np.uint64 and pos.shape == (495, 2) and [tuple(map(int, p)) for p in pos] == starts
    assert _positions_array(pos) is pos or np.array_equal(_positions_array(pos), pos)
