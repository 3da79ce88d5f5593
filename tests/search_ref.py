"""The reference of every `search_positions` comparison (test infrastructure): the oracle's MctsGame searched as the reference's
own helper searches it -- mcts.rs:469-485 `run_mcts`: n x [leaf_pos -> evaluator -> on_received_policy] on `MctsGame::new_from_pos`
(mcts.rs:48-56), then root_policy / root_q_with_penalty / root_q_no_penalty (mcts.rs:248-268).  The oracle is used as it stands.

All positions of a job are searched in lock-step, one evaluator batch per round: a game sees the answers to its own leaves only, so
the batching changes nothing it computes, and a network evaluator (batch-invariant) is asked once per round.

Counters, as the device reports them for a search job (include/c4a0_hip.h C4_FLAG_SEARCH):
  sims        n per position;
  expansions  the oracle's;
  backup      the oracle's backup_nodes (which leaves out the simulations of a terminal root);
  select      the oracle's select_levels WITHOUT the select behind each search's last simulation: nobody consumes that leaf, the
              device hands the slot on instead (whole games subtract select_levels_discarded for the same reason)."""
from __future__ import annotations

import numpy as np

from tests.helpers import START_EVALS, start_job

C_PLY_PENALTY = 0.01
_JOBS = {}


def oracle_evaluator(ev_name):
    """leaves (a list of oracle Pos) -> (logits[B, 7], q_penalty[B], q_no_penalty[B]) by the oracle's own evaluator of
    tests.helpers.START_EVALS: the hash evaluator, or a sharp one"""
    from oracle import c4oracle as O

    sharp = START_EVALS[ev_name][2]

    def ev(leaves):
        if sharp is None:
            out = [O.hash_eval_pos(int(p.mask), int(p.value)) for p in leaves]
            return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float32), np.array([o[2] for o in out], np.float32)
        lg, qp, qn, _tally = O.sharp_eval_batch(np.stack([O.planes(p) for p in leaves]), *sharp)
        return lg, qp, qn

    return ev


def search(positions, n, evaluator, c_exploration, c_ply_penalty=C_PLY_PENALTY):
    """n simulations from every (mask, value) of `positions` as root.  Returns a dict of arrays in the order given -- policy
    float32[P, 7], q_penalty / q_no_penalty float32[P], expansions / max_depth / sims_deep int64[P] -- and the job's counter sums
    "sims", "select", "backup", "expansions" as the device reports them."""
    from oracle import c4oracle as O

    games = [O.Game(O.Pos(int(m), int(v))) for m, v in positions]
    select_before_last = [0] * len(games)
    for it in range(n):
        leaves = [g.leaf_pos() for g in games]
        lg, qp, qn = evaluator(leaves)
        if it == n - 1:
            select_before_last = [g.counters()["select_levels"] for g in games]
        for i, g in enumerate(games):
            err = g.on_received_policy(lg[i], float(qp[i]), float(qn[i]), c_exploration, c_ply_penalty)
            assert err == 0, (i, it, err)
    ctr = [g.counters() for g in games]
    assert all(c["sims"] == n and c["moves"] == 0 for c in ctr)
    return {
        "policy": np.stack([g.root_policy() for g in games]).astype(np.float32) if games else np.zeros((0, 7), np.float32),
        "q_penalty": np.array([g.root_q_penalty() for g in games], dtype=np.float32),
        "q_no_penalty": np.array([g.root_q_no_penalty() for g in games], dtype=np.float32),
        "expansions": np.array([c["expansions"] for c in ctr], dtype=np.int64),
        "max_depth": np.array([c["max_depth"] for c in ctr], dtype=np.int64),
        "sims_deep": np.array([c["sims_deep"] for c in ctr], dtype=np.int64),
        "sims": n * len(games),
        "select": int(sum(select_before_last)),
        "backup": int(sum(c["backup_nodes"] for c in ctr)),
        "n_expansions": int(sum(c["expansions"] for c in ctr)),
    }


def start_job_search(ev_name, n):
    """tests.helpers.start_job's 495 positions searched under one of START_EVALS, computed once and shared (read-only)."""
    key = (ev_name, n)
    if key not in _JOBS:
        _reqs, starts, _part = start_job()
        _JOBS[key] = search(starts, n, oracle_evaluator(ev_name), START_EVALS[ev_name][1])
    return _JOBS[key]


def long_search_positions(k=16):
    """the first k non-terminal random starts of the job (T2: long searches)"""
    from oracle import c4oracle as O

    _reqs, starts, part = start_job()
    return [s for s, p in zip(starts, part) if p == "random" and O.terminal_state(O.Pos(*s)) == 0][:k]


def assert_records_equal(recs, ref, positions):
    """the device's records against `search`'s answer, bit for bit: policy bytes, q bits, the position, game_id == index, the
    search record's meta"""
    pos = np.array(positions, dtype=np.uint64).reshape(-1, 2)
    assert len(recs) == len(pos)
    assert np.array_equal(recs["game_id"], np.arange(len(pos), dtype=np.uint64))
    assert np.array_equal(recs["mask"], pos[:, 0]) and np.array_equal(recs["value"], pos[:, 1])
    assert np.all(recs["meta"] == 2 << 16)
    for name in ("policy", "q_penalty", "q_no_penalty"):
        got, want = np.ascontiguousarray(recs[name]).view(np.uint32), np.ascontiguousarray(ref[name]).view(np.uint32)
        bad = np.flatnonzero((got != want).reshape(len(pos), -1).any(axis=1))
        assert bad.size == 0, f"{name} differs at {bad.size} positions, first {int(bad[0])}: {recs[name][bad[0]]} != {ref[name][bad[0]]}"


def assert_counters(c, ref, n_positions, n):
    """the counter identities of a finished search job (include/c4a0_hip.h C4_FLAG_SEARCH)"""
    assert c["error"] == 0
    assert c["sims"] == ref["sims"] == n_positions * n
    assert c["games_done"] == c["samples"] == c["games_started"] == n_positions
    assert c["moves"] == 0 and c["ref_skipped_sims"] == 0
    assert (c["select_levels"], c["backup_nodes"], c["expansions"]) == (ref["select"], ref["backup"], ref["n_expansions"])
