"""Non-finite evaluator outputs, on the CPU: the jobs tests/test_gpu_nonfinite_regime.py plays on the device (tests.helpers.POISON_JOBS)
held to what makes them worth playing, on the oracle alone.  A diverging network is non-finite at SOME positions; the evaluator
here is the hash (or a sharp) evaluator poisoned at one position in `rate` by one of eight kinds (tests.helpers.POISON_KINDS),
and every game of a job is played alone (tests.helpers.oracle_outcomes) to its samples or to the reference's panic: the code, and
whether the panic came from a select somebody consumes (`live`) or from the one behind the simulation that completes the root's n
visits, whose leaf the gate throws away (`discarded`).  This file holds

  * the numpy and torch twins of the evaluator against each other, bit for bit, every kind among the positions;
  * per setting the exact census (FLOORS): outcome classes, kinds that fired at a non-terminal leaf, evaluator rows; at least 10
    games in every class and kind a setting claims (CLAIMS), every class and kind claimed somewhere; errored games at most half the
    slots -- an errored slot is dead, the rest must drain the queue;
  * the two orders of a job: the reference's (select, then the gate) and the device's (the gate first; c4o_game_set_device_order).
    Without poison they give the same samples; with it, the games that differ are games of class `discarded` that escape the panic
    -- DESIGN.md section 3, the fourth counted deviation -- and their number is pinned per setting;
  * three mutants of the reference's rules (c4o_game_set_twin), each of which must change at least 10 games of the matrix: the
    jobs can see a kernel that masks after the softmax's maximum, panics on a single NaN candidate, or propagates NaN in f32::max."""
import collections

import numpy as np
import pytest

from oracle import c4oracle as O
from tests.helpers import (N_POISON_SLOTS, POISON_JOBS, POISON_KINDS, evidence, oracle_outcomes, outcome_class, poison_base, poison_eval_np,
                           poison_eval_torch, poison_job_games, poison_plan_np, poison_settings, pos_to_planes_np)

SETTINGS = poison_settings()
# Exact figures, per setting (named by the first job that has it): games by outcome class in the reference's order, games in which
# each kind (POISON_KINDS order) fired at a non-terminal leaf, evaluator rows, the longest game's rows; `escaped` = games whose
# outcome differs in the device's order (all of them nan_discarded -> finished); `twins` = games changed by the mutants no_mask,
# nan_single, nan_max.
FLOORS = {
    "hash-n8-f32-eager": dict(ok=751, nan_live=12, nan_discarded=12, degenerate=25, kinds=[11, 14, 12, 23, 7, 18, 13, 12], sims=69412, rounds=170, escaped=6, twins=(263, 0, 0)),
    "hash-n24-f32-graph4": dict(ok=553, nan_live=19, nan_discarded=2, degenerate=26, kinds=[10, 51, 33, 26, 10, 15, 11, 15], sims=130989, rounds=476, escaped=0, twins=(207, 0, 0)),
    "k4sat-n8-bf16-graph4": dict(ok=757, nan_live=17, nan_discarded=6, degenerate=20, kinds=[18, 14, 11, 6, 14, 7, 17, 3], sims=56349, rounds=136, escaped=0, twins=(386, 0, 0)),
    "hash-n8-f32-dirichlet": dict(ok=743, nan_live=23, nan_discarded=10, degenerate=24, kinds=[18, 8, 18, 24, 10, 19, 10, 14], sims=72607, rounds=187, escaped=6, twins=(293, 0, 0)),
    "starts-hash-n24-f32-eager": dict(ok=438, nan_live=22, nan_discarded=0, degenerate=35, kinds=[18, 33, 12, 8, 10, 12, 15, 20], sims=35089, rounds=350, escaped=0, twins=(226, 0, 0)),
    "columns-hash-n8-f32-eager": dict(ok=130, nan_live=0, nan_discarded=0, degenerate=38, kinds=[18, 14, 15, 18, 11, 18, 8, 12], sims=1451, rounds=14, escaped=0, twins=(25, 14, 17)),
    "column-pairs-hash-n8-gather": dict(ok=124, nan_live=0, nan_discarded=0, degenerate=44, kinds=[22, 12, 14, 20, 16, 20, 10, 14], sims=1406, rounds=14, escaped=0, twins=(28, 16, 18)),
}
# What each setting is there for: the classes and kinds it must hold at least 10 games of.  nan_illegal needs a full column at a
# non-terminal leaf, which games from the empty board at n = 8 reach rarely; `discarded` needs the gate often, i.e. n = 8.
_ALL_BUT = lambda *names: [k for k in POISON_KINDS if k not in names]   # noqa: E731
CLAIMS = {
    "hash-n8-f32-eager": (["ok", "nan_live", "nan_discarded", "degenerate"], _ALL_BUT("nan_illegal")),
    "hash-n24-f32-graph4": (["ok", "nan_live", "degenerate"], list(POISON_KINDS)),
    "k4sat-n8-bf16-graph4": (["ok", "nan_live", "degenerate"], ["nan_qp", "nan_qn", "inf_qp", "nan_illegal", "ninf_all_legal"]),
    "hash-n8-f32-dirichlet": (["ok", "nan_live", "nan_discarded", "degenerate"], _ALL_BUT("nan_qn")),
    "starts-hash-n24-f32-eager": (["ok", "nan_live", "degenerate"], _ALL_BUT("nan_legal")),
    "columns-hash-n8-f32-eager": (["ok", "degenerate"], _ALL_BUT("ninf_all_legal")),
    "column-pairs-hash-n8-gather": (["ok", "degenerate"], list(POISON_KINDS)),
}


def _same(a, b):
    """two outcomes agree: the same samples, or the same code (where it was raised is what the two orders differ in)"""
    return a == b if a[0] == "ok" and b[0] == "ok" else a[0] == b[0]


# --------------------------------------------------------------------------------------------- the evaluator
@pytest.mark.parametrize("base", ["hash", "k4sat"])
def test_numpy_and_torch_twins_agree_bit_for_bit(base):
    torch = pytest.importorskip("torch")
    mask, value = O.random_positions_np(100_000, 5)
    planes = pos_to_planes_np(mask, value)
    assert np.array_equal(planes[:64], np.stack([O.planes(O.Pos(int(m), int(v))) for m, v in zip(mask[:64], value[:64])]))
    for rate in (4, 150, 300):
        want = poison_eval_np(poison_base(base, "numpy"), rate)(0, planes)
        lg, q = poison_eval_torch(poison_base(base, "torch"), rate)(torch.from_numpy(planes))
        got = (lg.numpy(), q[:, 0].numpy(), q[:, 1].numpy())
        for w, g in zip(want, got):
            assert np.array_equal(w.view(np.uint32), np.ascontiguousarray(g).view(np.uint32))
        # only the default quiet NaN
        for w in want:
            assert set(w[np.isnan(w)].view(np.uint32).tolist()) <= {0x7FC00000}
        kind, legal, chosen = poison_plan_np(mask, value, rate)
        fired = np.bincount(kind[kind >= 0], minlength=8)
        assert fired.min() >= 10, fired
        assert np.all(chosen.sum(axis=1) == (legal.sum(axis=1) > 0)) and np.all(legal | ~chosen)
        hit = kind >= 0
        clean = poison_base(base, "numpy")(0, planes)
        for w, c in zip(want, clean):
            assert np.array_equal(w[~hit], c[~hit])
    evidence(f"non-finite, evaluator twins ({base}): 100 000 reachable positions x rates 4, 150, 300 numpy == torch bit for bit, every kind "
             f"at >= 10 positions, NaNs all 0x7fc00000")


def test_each_kind_does_what_the_header_says_at_one_position():
    """one answer of each sort into a fresh game of the oracle: the reference's outcome, kind by kind (include/c4a0_hip.h lists them)"""
    nan, inf = float("nan"), float("inf")
    two = O.from_moves([0, 1])                                                  # seven legal columns
    one = O.Pos(*poison_job_games(("x", "hash", 8, "f32", 4, {"starts": "columns"}))[1][0])      # one legal column
    full = O.from_moves([3] * 6)                                                # column 3 full
    base = [0.5, -1.0, 0.25, 0.0, 1.0, -0.5, 0.75]

    def run(pos, logits, qp=0.25, qn=0.5, sims=6):
        g = O.Game(pos)
        for _ in range(sims):
            e = g.on_received_policy(logits, qp, qn, 6.6, 0.01)
            if e:
                return e
        return 0

    assert run(two, base) == 0
    assert run(two, base, qp=nan) == O.ERR_NAN_IN_TREE                          # nan_qp: the second simulation's leaf is compared
    assert run(one, base, qp=nan) == 0                                          # ... never with one candidate per level
    assert run(two, base, qn=nan) == 0                                          # nan_qn
    assert run(two, base, qp=inf, sims=1) == 0                                  # inf_qp: +-inf compare fine
    assert run(two, base, qp=inf, sims=12) == O.ERR_NAN_IN_TREE                 # ... until +inf meets -inf in a child's q_sum
    assert run(two, [nan] + base[1:]) == O.ERR_NAN_IN_TREE                      # nan_legal: every prior NaN
    legal_one = [c for c in range(7) if (O.legal_mask(one) >> c) & 1][0]
    assert run(one, [nan if c == legal_one else x for c, x in enumerate(base)]) == O.ERR_DEGENERATE_POLICY   # masked maximum -inf
    assert run(full, [nan if c == 3 else x for c, x in enumerate(base)]) == 0   # nan_illegal: masked
    assert run(two, [0.5] + [-inf] * 6) == 0                                    # ninf_but_one: zero priors
    assert run(full, [1.0 if c == 3 else -inf for c in range(7)]) == O.ERR_DEGENERATE_POLICY   # ninf_all_legal
    assert run(two, [inf] + base[1:]) == O.ERR_DEGENERATE_POLICY                # inf_legal


# --------------------------------------------------------------------------------------------- the jobs
def test_the_matrix_is_what_it_says():
    assert {j[0] for j in SETTINGS} == set(FLOORS) == set(CLAIMS)
    assert {j[2] for j in POISON_JOBS} == {8, 24}
    for job in POISON_JOBS:
        reqs, starts = poison_job_games(job)
        assert len(reqs) > N_POISON_SLOTS and len({r[0] for r in reqs}) == len(reqs) and (starts is None or len(starts) == len(reqs))
    # every class and every kind is claimed by some setting
    assert {c for cl, _k in CLAIMS.values() for c in cl} == {"ok", "nan_live", "nan_discarded", "degenerate"}
    assert {k for _c, ks in CLAIMS.values() for k in ks} == set(POISON_KINDS)


@pytest.mark.parametrize("job", SETTINGS, ids=[j[0] for j in SETTINGS])
def test_census_of_outcomes_and_kinds(job):
    """the exact census of the setting, its claims at >= 10 games each, and the condition of the job: errored games <= half the slots"""
    ref = oracle_outcomes(job)
    oc = collections.Counter(outcome_class(o).replace("-", "_") for o in ref["outcomes"])
    kc = collections.Counter(k for ks in ref["kinds"] for k in ks)
    f = FLOORS[job[0]]
    got = dict(ok=oc["ok"], nan_live=oc["nan_live"], nan_discarded=oc["nan_discarded"], degenerate=oc["degenerate"],
               kinds=[kc[k] for k in range(8)], sims=ref["sims"], rounds=ref["rounds"])
    assert got == {k: f[k] for k in got}, got
    assert sum(oc.values()) == len(ref["outcomes"]) and all(o[0] in ("ok", O.ERR_NAN_IN_TREE, O.ERR_DEGENERATE_POLICY) for o in ref["outcomes"])
    errored = len(ref["outcomes"]) - oc["ok"]
    assert errored <= N_POISON_SLOTS // 2, errored
    classes, kinds = CLAIMS[job[0]]
    assert all(got[c] >= 10 for c in classes) and all(got["kinds"][POISON_KINDS.index(k)] >= 10 for k in kinds)
    # a degenerate policy is raised before the backup, so it is never `discarded`
    assert all(o[1] == "live" for o in ref["outcomes"] if o[0] == O.ERR_DEGENERATE_POLICY)
    evidence(f"non-finite, oracle alone, {job[0]}: {len(ref['outcomes'])} games: {oc['ok']} finished, NaN panics {oc['nan_live']} live + "
             f"{oc['nan_discarded']} discarded, {oc['degenerate']} degenerate policies; kinds fired in {got['kinds']} games; {ref['sims']} rows")


# --------------------------------------------------------------------------------------------- the two orders
def test_the_device_order_changes_no_sample_of_a_healthy_job():
    """one poisoned position in 2^58 = none: both orders give c4o_play_from's samples, game by game"""
    from tests.helpers import oracle_samples_by_game

    for job in (("clean", "hash", 8, "f32", 1 << 58, {"games": 96, "first_id": 1000}), ("clean", "hash", 24, "f32", 1 << 58, {"starts": True})):
        reqs, starts = poison_job_games(job)
        want = oracle_samples_by_game(O.play_from(reqs, starts, job[2], 6.6, 0.01, "hash")[0])
        for dev in (False, True):
            got = oracle_outcomes(job, device_order=dev)
            assert all(o[0] == "ok" for o in got["outcomes"])
            assert {r[0]: o[1] for r, o in zip(reqs, got["outcomes"])} == want


@pytest.mark.parametrize("job", SETTINGS, ids=[j[0] for j in SETTINGS])
def test_the_device_order_lets_only_discarded_panics_escape(job):
    """The reference runs select_new_leaf before the gate (mcts.rs:83-108, self_play.rs:283-301); the device runs the gate first and
    selects once, from the new root.  A game differs between the orders only if the reference panics in the select the device
    leaves out -- class `discarded` -- and then it finishes, or panics later with the same code.  Pinned: which games, how many."""
    ref, dev = oracle_outcomes(job), oracle_outcomes(job, device_order=True)
    differ = [i for i, (a, b) in enumerate(zip(ref["outcomes"], dev["outcomes"])) if not _same(a, b)]
    assert all(ref["outcomes"][i] == (O.ERR_NAN_IN_TREE, "discarded") and dev["outcomes"][i][0] == "ok" for i in differ)
    assert len(differ) == FLOORS[job[0]]["escaped"]
    # the other games of the class panic in a later, live select: the NaN sat in the subtree the move kept
    later = [i for i, (a, b) in enumerate(zip(ref["outcomes"], dev["outcomes"])) if a == (O.ERR_NAN_IN_TREE, "discarded") and b[0] != "ok"]
    assert all(dev["outcomes"][i] == (O.ERR_NAN_IN_TREE, "live") for i in later)
    assert len(later) + len(differ) == FLOORS[job[0]]["nan_discarded"]
    assert not any(o == (O.ERR_NAN_IN_TREE, "discarded") for o in dev["outcomes"])
    evidence(f"non-finite, the two orders, {job[0]}: of {FLOORS[job[0]]['nan_discarded']} games the reference panics in behind the gate, the "
             f"device's order finishes {len(differ)} and panics later in {len(later)}; every other game equal")


# --------------------------------------------------------------------------------------------- searches
# n -> (finished, NaN panics live, NaN panics behind the last simulation, degenerate policies, searches that finish in the device's
# order only, finished searches with a NaN root q_penalty / a NaN q_no_penalty / an infinite q_penalty in the device's order)
SEARCH_FLOORS = {8: (474, 8, 2, 11, 2, 1, 4, 7), 24: (443, 20, 0, 32, 0, 2, 10, 13)}


@pytest.mark.parametrize("n", [8, 24])
def test_census_of_poisoned_searches(n):
    """tests.search_ref.poison_search over start_job()'s 495 positions, the job of tests/test_gpu_search_positions.py T5: exact
    census; errored searches at most half the slots; non-finite values reach records (which is why T5 compares by the record rule)"""
    from tests.search_ref import POISON_SEARCH_RATE, poison_search, same_search_outcome

    ref, _rows = poison_search(n, POISON_SEARCH_RATE)
    dev, _rows = poison_search(n, POISON_SEARCH_RATE, device_order=True)
    oc = collections.Counter(outcome_class(o) for o in ref)
    escaped = [i for i, (a, b) in enumerate(zip(ref, dev)) if not same_search_outcome(a, b)]
    assert all(ref[i] == (O.ERR_NAN_IN_TREE, "discarded") and dev[i][0] == "ok" for i in escaped)
    fin = [o for o in dev if o[0] == "ok"]
    got = (oc["ok"], oc["nan-live"], oc["nan-discarded"], oc["degenerate"], len(escaped), sum(bool(np.isnan(o[2])) for o in fin),
           sum(bool(np.isnan(o[3])) for o in fin), sum(bool(np.isinf(o[2])) for o in fin))
    assert got == SEARCH_FLOORS[n], got
    assert len(ref) - oc["ok"] <= N_POISON_SLOTS // 2 and got[5] >= 1 and got[6] >= 1
    evidence(f"non-finite, searches on the oracle alone, n = {n}: 495 positions: {got[0]} finished, NaN panics {got[1]} live + {got[2]} behind the "
             f"last simulation ({got[4]} finish in the device's order), {got[3]} degenerate; finished records with NaN q {got[5]}, NaN "
             f"q_no_penalty {got[6]}, infinite q {got[7]}")


# --------------------------------------------------------------------------------------------- twin mutants
def test_twin_mutants_of_the_rules_change_the_matrix():
    """no masking before the softmax, a NaN panic with a single candidate, f32::max replaced by a NaN-propagating maximum: each
    changes at least 10 games of the matrix (the last two only where every node has one candidate: the column job)"""
    changed = collections.Counter()
    for job in SETTINGS:
        ref = oracle_outcomes(job)
        per = []
        for name, flag in (("no_mask", O.TWIN_NO_MASK), ("nan_single", O.TWIN_NAN_SINGLE), ("nan_max", O.TWIN_NAN_MAX)):
            got = oracle_outcomes(job, twin=flag)
            n = sum(1 for a, b in zip(ref["outcomes"], got["outcomes"]) if not _same(a, b))
            per.append(n)
            changed[name] += n
        assert tuple(per) == FLOORS[job[0]]["twins"], (job[0], per)
    assert all(changed[k] >= 10 for k in ("no_mask", "nan_single", "nan_max")), changed
    evidence("non-finite, twin mutants of the reference's rules (games of the matrix changed): " + ", ".join(f"{k} {v}" for k, v in changed.items()))
