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


POISON_SEARCH_RATE = 40   # 21 errored searches of 495 at n = 8, 52 at n = 24: under half of the 128 slots (an errored slot stays dead)
_POISON = {}


def poison_search(n, rate, device_order=False):
    """tests.helpers.start_job's 495 positions searched under the hash evaluator poisoned at one position in `rate`
    (tests.helpers.poison_eval_np), every search alone, all in lock-step.  Per position ("ok", policy float32[7], q_penalty,
    q_no_penalty as float32) or (code, where): the C4O_ERR code of the reference's panic, where = "live" | "discarded" -- discarded =
    raised by the select behind the search's LAST simulation, which run_mcts (mcts.rs:469-485) makes and nobody consumes.
    device_order: that select is left out, as the device hands the slot on instead (c4o_game_on_received_policy_gated): such a
    search finishes, and its record may carry a NaN root q.  Also returns the number of evaluator rows."""
    key = (n, rate, bool(device_order))
    if key not in _POISON:
        from oracle import c4oracle as O
        from tests.helpers import hash_eval_np, poison_eval_np, pos_to_planes_np

        _reqs, starts, _part = start_job()
        ev = poison_eval_np(hash_eval_np, rate)
        games = [O.Game(O.Pos(int(m), int(v))) for m, v in starts]
        out, live, rows = [None] * len(games), list(range(len(games))), 0
        for it in range(n):
            leaves = [games[i].leaf_pos() for i in live]
            lg, qp, qn = ev(0, pos_to_planes_np(np.array([p.mask for p in leaves], np.uint64), np.array([p.value for p in leaves], np.uint64)))
            rows += len(live)
            nxt = []
            for j, i in enumerate(live):
                err = games[i].on_received_policy(lg[j], float(qp[j]), float(qn[j]), START_EVALS["hash"][1], C_PLY_PENALTY, gate_n=n if device_order else 0)
                if err:
                    out[i] = (err, "discarded" if it == n - 1 and err == O.ERR_NAN_IN_TREE else "live")
                else:
                    nxt.append(i)
            live = nxt
        for i in live:
            g = games[i]
            out[i] = ("ok", g.root_policy().astype(np.float32), np.float32(g.root_q_penalty()), np.float32(g.root_q_no_penalty()))
        _POISON[key] = (out, rows)
    return _POISON[key]


def same_search_outcome(a, b):
    """two outcomes of poison_search agree: the same code, or the same record under the record rule below"""
    if a[0] != "ok" or b[0] != "ok":
        return a[0] == b[0]
    return all(_same_f32(x, y) for x, y in zip(a[1:], b[1:]))


def _same_f32(x, y):
    """THE RECORD RULE of the non-finite tier: a NaN equals a NaN, everything else bit for bit.  IEEE 754 leaves the payload and
    the sign of a NaN that comes out of an addition or a division to the implementation, and x86 and the GPU may differ; no other
    relaxation, and no position is left out."""
    x, y = np.atleast_1d(np.asarray(x, np.float32)), np.atleast_1d(np.asarray(y, np.float32))
    nan = np.isnan(x)
    return bool(np.array_equal(nan, np.isnan(y)) and np.array_equal(x[~nan].view(np.uint32), y[~nan].view(np.uint32)))


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
