"""Non-finite evaluator outputs in the tree kernels, on the device against the oracle, game by game.  The evaluator is the hash
evaluator poisoned at some positions (tests.helpers.poison_eval_torch: NaN / +inf q, NaN, -inf and +inf logits, eight kinds), which
is what a diverging network does; tests/test_nonfinite_regime.py holds the jobs (tests.helpers.POISON_JOBS) to their census on the
oracle alone.  Every session is stepped by hand -- DeviceSession.run raises at its first poll -- until no slot is active, and then

  per game  the slot that holds an errored game carries the oracle's code in its status byte (C4_OF_C4O below), an errored game
            has no record, and a finished game's records are the oracle's bit for bit -- also where games of the same wavefront
            (eight play in lock-step, with ballots and DPP exchanges across them) errored beside it;
  per job   counters()["error"] is the code of an errored game and error_slot a slot such a game died on; games_done is the
            oracle's number of finished games.

The oracle plays the DEVICE'S ORDER of a job here (c4o_game_set_device_order): expand, back up, the gate, one select from the new
root.  The reference selects before the gate and throws that leaf away; a NaN which that select alone would compare makes the
reference panic where the device moves on (the fourth counted deviation).  tests/test_nonfinite_regime.py
pins on the CPU which games of each job those are (6 of 800 in each n = 8 setting from the empty board, none elsewhere); every other
game is the same in both orders, so it is compared with the reference's order here as well.

Forms (POISON_JOBS): eager with f32 and bf16 planes, HIP graphs of 4 rounds, Dirichlet noise, a tiny and a roomy evaluation cache,
noise and cache together, reclaimed arenas (period 1, the tightest halves), compact(8) every 7 steps, the gather step kernel --
once over pairs of games that show the evaluator the same leaves, so that one poisoned answered row is gathered by two slots and
both games die of it (from the empty board a poisoned position is hardly ever the leaf of two games in the same round).

What compact() does with a dead slot (pinned by the compact job): an errored slot is neither active nor idle.  The plan counts the A
active slots and treats every other slot below A as a hole: a dead slot below A is overwritten by a game moved down from above --
its status byte and ordinal are gone, so they must be read before; a dead slot at or above A keeps both and falls out of the
narrowed session's rows.  No game is lost or stepped twice.

Established on one MI355X: the games of class `discarded` do on the device what the oracle does in the device's order -- the 6 of
each n = 8 setting finish, the others end later with C4_ERR_NAN_IN_TREE.  The 18 cases take 13 s together, the slowest (the
first, which loads the library) 2.3 s.  """
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import (C4_OF_C4O, N_POISON_SLOTS, POISON_JOBS, SLOT_ACTIVE, SLOT_IDLE, GraphSafePoisonEval, evidence, note_dead_slots,   # noqa: E402
                           oracle_outcomes, planes_to_pos_np, poison_base, poison_c_exploration, poison_eval_np, poison_eval_torch,
                           poison_job_games, poison_plan_np, samples_by_game, step_eager_until_no_slot_is_active,
                           step_graph_until_no_slot_is_active)

DEV = "cuda:0"
ACTIVE, IDLE = SLOT_ACTIVE, SLOT_IDLE
_note_dead, _step_eager, _step_graph = note_dead_slots, step_eager_until_no_slot_is_active, step_graph_until_no_slot_is_active


def _step_compacting(s, ev, every, cap, dead, where):
    """compact(8) every `every`-th step; the docstring's statement about dead slots, checked at every compaction that moves games"""
    widths, overwritten, kept = [], 0, 0
    for step in range(1, cap + 1):
        s.evaluate(ev)
        s.step()
        if step % every:
            continue
        n_act, st0, or0 = _note_dead(s, dead, where)
        if n_act == 0:
            return step, widths, overwritten, kept
        act, rows = s.compact(8)
        widths.append(rows)
        _n, st1, or1 = _note_dead(s, {}, {})
        if act == N_POISON_SLOTS and rows == N_POISON_SLOTS and np.array_equal(st0, st1):
            continue   # requests still queued: a no-op
        assert act == n_act and rows == max(8, -(-act // 8) * 8) == s.rows
        assert np.all(st1[:act] == ACTIVE) and not np.any(st1[act:] == ACTIVE)
        assert sorted(or1[st1 == ACTIVE]) == sorted(or0[st0 == ACTIVE])
        was_dead = (st0 != ACTIVE) & (st0 != IDLE)
        overwritten += int(was_dead[:act].sum())
        kept += int(was_dead[act:].sum())
        assert np.array_equal(st1[act:][was_dead[act:]], st0[act:][was_dead[act:]]) and np.array_equal(or1[act:][was_dead[act:]], or0[act:][was_dead[act:]])
    raise AssertionError(f"slots still active after {cap} steps")


def _step_gather(s, np_eval, rate, cap, dead, where):
    """c4_session_unique_leaves + c4_session_step_gather by hand; counts the (round, row) pairs in which a poisoned position that
    reaches the tree was the leaf of several active slots, i.e. one answered row was gathered by several games, and how many of
    those games ended dead"""
    from c4a0_amd._lib import check

    g = s.n_slots
    inverse = torch.zeros(g, dtype=torch.int32, device=s.device)
    h_planes = torch.zeros((g, 2, 6, 7), dtype=torch.float32).pin_memory()
    h_count = torch.zeros(1, dtype=torch.int32).pin_memory()
    h_out = torch.zeros((g, 9), dtype=torch.float32).pin_memory()
    from oracle import c4oracle as O

    shared, sharers = 0, set()
    for step in range(1, cap + 1):
        check(s.L.c4_session_unique_leaves(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(h_planes.data_ptr()), None, C.c_void_p(h_count.data_ptr())))
        s._bound_stream.synchronize()
        n_u = int(h_count[0])
        if n_u == 0:
            _note_dead(s, dead, where)
            return step - 1, shared, len(sharers & set(dead))
        rows = h_planes.numpy()[:n_u]
        lp, qp, qn = np_eval(0, rows)
        rm, rv = planes_to_pos_np(rows)
        kind, legal, _chosen = poison_plan_np(rm, rv, rate)
        # the filter of oracle_outcomes: the poison reaches the tree -- a non-terminal leaf; nan_illegal only where a column is full
        hit = [j for j in np.flatnonzero(kind >= 0) if (kind[j] != 4 or not legal[j].all()) and O.terminal_state(O.Pos(int(rm[j]), int(rv[j]))) == 0]
        if hit:
            lm, lv, status, ordinal = s.leaves(with_ordinals=True)
            for j in hit:
                on = (lm == rm[j]) & (lv == rv[j]) & (status == ACTIVE)
                if int(on.sum()) >= 2:
                    shared += 1
                    sharers.update(int(o) for o in ordinal[on])
        out = h_out.numpy()
        out[:n_u, :7], out[:n_u, 7], out[:n_u, 8] = lp, qp, qn
        check(s.L.c4_session_step_gather(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(h_out.data_ptr()), n_u))
    raise AssertionError(f"slots still active after {cap} steps")


def play_poison_job(job):
    """one job on the device, stepped by hand until no slot is active -> (records, sample counts, counters, dead, where, extra)"""
    from c4a0_amd.session import DeviceSession
    from tests.test_gpu_reclaim import _half_min

    name, base, n, planes, rate, opt = job
    reqs, starts = poison_job_games(job)
    cap = oracle_outcomes(job, device_order=True)["sims"]   # a step with an active slot runs at least one simulation
    kw = {}
    if "reclaim" in opt:
        kw = dict(reclaim=True, reclaim_period=opt["reclaim"], blocks_per_slot=2 * _half_min(n, opt["reclaim"]))
    s = DeviceSession(N_POISON_SLOTS, n, poison_c_exploration(base), 0.01, device=torch.device(DEV),
                      planes_dtype=torch.float32 if planes == "f32" else torch.bfloat16, **kw)
    s.set_games(reqs, starts)
    if "dirichlet" in opt:
        s.set_dirichlet(*opt["dirichlet"])
    if "cache" in opt:
        s.set_eval_cache(*opt["cache"])
    s.bind()
    s.start()
    dead, where, extra = {}, {}, ""
    ev = poison_eval_torch(poison_base(base, "torch"), rate)
    if "graph" in opt:
        steps = _step_graph(s, GraphSafePoisonEval(poison_base(base, "torch"), rate), opt["graph"], cap, dead, where)
    elif "compact" in opt:
        steps, widths, overwritten, kept = _step_compacting(s, ev, opt["compact"], cap, dead, where)
        assert widths[0] == N_POISON_SLOTS and widths[-1] == 8 and sorted(widths, reverse=True) == widths
        assert overwritten >= 1 and kept >= 1, (overwritten, kept)
        extra = f", widths {sorted(set(widths), reverse=True)}, dead slots overwritten {overwritten} / kept {kept} (slot x compaction)"
    elif "gather" in opt:
        steps, shared, shared_dead = _step_gather(s, poison_eval_np(poison_base(base, "numpy"), rate), rate, cap, dead, where)
        if opt.get("starts") == "column-pairs":   # the job built for it: two games per start position, side by side
            assert shared >= 10 and shared_dead >= 10, (shared, shared_dead)
        extra = f", {shared} poisoned rows gathered by several slots, {shared_dead} of the games that shared one dead"
    else:
        steps = _step_eager(s, ev, cap, dead, where)
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    s.close()
    if "cache" in opt:
        assert 0 < c["eval_cache_hits"] <= c["eval_cache_probes"]
        extra += f", {c['eval_cache_hits']} cache hits"
    if "reclaim" in opt:
        assert c["reclaim_passes"] > 0, "the job does not need its arenas reclaimed"
        extra += f", {c['reclaim_passes']} reclaim passes"
    return recs, counts, c, dead, where, f"{steps} steps" + extra


def check_against(job, want, recs, counts, c, dead, where):
    """the per-game and per-job assertions of the module docstring against `want` = an oracle_outcomes() answer"""
    reqs, _starts = poison_job_games(job)
    got = samples_by_game(recs)
    bad = []
    for i, (req, o) in enumerate(zip(reqs, want["outcomes"])):
        if o[0] == "ok":
            if i in dead or got.get(req[0]) != o[1] or counts[i] != len(o[1]):
                bad.append((i, "finished", dead.get(i, "records differ")))
        elif dead.get(i) != C4_OF_C4O[o[0]] or req[0] in got or counts[i] != 0:
            bad.append((i, o, dead.get(i, "finished")))
    assert not bad, f"{len(bad)} games differ from the oracle, first {bad[:5]}"
    n_ok = sum(1 for o in want["outcomes"] if o[0] == "ok")
    assert len(dead) == len(reqs) - n_ok and c["games_done"] == n_ok and c["games_started"] == len(reqs)
    assert c["error"] in set(dead.values()) and c["error_slot"] in {where[o] for o, code in dead.items() if code == c["error"]}
    # an errored game does nothing after its panic: the work counters are the oracle's, dead games included up to theirs.  (The
    # oracle counts a simulation when it starts, the device when it is backed up: a degenerate policy is raised in between.)
    oc = want["counters"]
    n_degenerate = sum(1 for o in want["outcomes"] if o[0] == 2)
    assert c["sims"] + c["ref_skipped_sims"] == oc["sims"] - n_degenerate and c["ref_skipped_sims"] == oc["sims_terminal_root"]
    assert (c["backup_nodes"], c["expansions"], c["moves"]) == (oc["backup_nodes"], oc["expansions"], oc["moves"])
    return n_ok


@pytest.mark.parametrize("job", POISON_JOBS, ids=[j[0] for j in POISON_JOBS])
def test_poisoned_games_end_as_the_oracle_says_game_by_game(job):
    recs, counts, c, dead, where, extra = play_poison_job(job)
    dev_order, ref_order = oracle_outcomes(job, device_order=True), oracle_outcomes(job)
    same = lambda a, b: a == b if a[0] == b[0] == "ok" else a[0] == b[0]   # noqa: E731
    escaped = [i for i, (a, b) in enumerate(zip(ref_order["outcomes"], dev_order["outcomes"])) if not same(a, b)]
    print(f"{job[0]}: device error {c['error']} at slot {c['error_slot']}, games_done {c['games_done']}, dead {sorted(dead.items())[:8]}..., "
          f"escaped in the device's order {escaped}: on the device {[dead.get(i, 'finished') for i in escaped]}")
    n_ok = check_against(job, dev_order, recs, counts, c, dead, where)
    # the reference's own order: every game but the pinned escapes
    reqs, _starts = poison_job_games(job)
    got = samples_by_game(recs)
    for i, (req, o) in enumerate(zip(reqs, ref_order["outcomes"])):
        if i not in escaped:
            assert (got.get(req[0]) == o[1] and i not in dead) if o[0] == "ok" else dead.get(i) == C4_OF_C4O[o[0]], i
    # healthy games beside errored ones: slots of a wavefront are eight consecutive slots
    beside = sum(1 for o, g in where.items() for o2, g2 in where.items() if o != o2 and g // 8 == g2 // 8)
    codes = {k: sum(1 for v in dead.values() if v == k) for k in sorted(set(dead.values()))}
    evidence(f"non-finite T1 {job[0]}: {len(reqs)} games on {N_POISON_SLOTS} slots: {n_ok} finished == oracle bit for bit, {len(dead)} dead slots "
             f"by code {codes} == oracle game by game ({len(escaped)} escape the reference's panic behind the gate), {beside // 2} pairs of "
             f"dead slots share a wavefront, {extra}")


# --------------------------------------------------------------------------------------------- the fused launch
# sharp_model(1, 32) with unit 0 of each head's last hidden layer (weight row and bias) scaled up, so that the unit overflows to
# +inf on a share of the positions: the policy output layer then gives logits of +-inf, i.e. seven NaN log-probabilities (c4a0_hip.h,
# head out) -- in the tree a masked maximum of -inf, a degenerate policy -- or log-probabilities of -inf, zero priors; the value
# head tanh(+-inf) = +-1, or NaN where both signs meet.  The unit's pre-activation is 0.1 to 2 in magnitude, so 2^126 never reaches
# f32's 2^128.  Measured on the f32 module: over 20 000 reachable positions the policy answer is non-finite at 0.02 % with 2^127,
# 7.4 % with 2^128, 34 % with 2^129, q at 0.02 % with 2^130, 9.7 % with 2^131 (where 114 of this job's 128 games die of a NaN q);
# this job played by the oracle under the f32 module with (policy, value) = (2^128, 2^130): 9 % of the visited positions, 8 games
# die; (1.25 x 2^128, 2^130): 19 %, 53 die, 75 finish; (2^129, 2^130): 46 %, 98 die.  The middle one: both classes well filled.
OVERFLOW_SCALE = {"policy": (1.25, 128), "value": (1.0, 130)}   # mantissa (exact in bf16), exponent
FUSED_JOB = ("overflow-1x32-n8-bf16", "hash", 8, "bf16", 1 << 58, {"games": N_POISON_SLOTS, "first_id": 40_000})   # no refill: most games die


def _overflowing_model():
    from tests.helpers import SHARP_MODEL_K, sharp_model

    model = sharp_model(1, 32, SHARP_MODEL_K)
    with torch.no_grad():
        for head, (m, k) in ((model.fc_policy, OVERFLOW_SCALE["policy"]), (model.fc_value, OVERFLOW_SCALE["value"])):
            lin = head[-3][0]                                        # the last hidden layer's Linear (BN and ReLU follow)
            for t in (lin.weight[0], lin.bias[0]):
                t.mul_(2.0 ** 64).mul_(m * 2.0 ** (k - 64))          # (2^128 is no f32)
            assert bool(torch.isfinite(lin.weight).all())
    return model


def _table_evaluator(mask, value, out):
    """the logged answers as a reference-signature callback (what c4o_eval_table does): a non-terminal position the device never
    showed its evaluator fails the replay"""
    from oracle import c4oracle as O

    idx = {(int(m), int(v)): i for i, (m, v) in enumerate(zip(mask, value))}

    def cb(_model_id, planes):
        m, v = planes_to_pos_np(planes)
        rows = np.zeros((len(m), 9), dtype=np.float32)
        for j, key in enumerate(zip(m.tolist(), v.tolist())):
            i = idx.get(key)
            if i is None:
                assert O.terminal_state(O.Pos(*key)) != 0, f"position {key} was never shown to the device's evaluator"
            else:
                rows[j] = out[i]
        return rows[:, :7], rows[:, 7], rows[:, 8]

    return cb


def test_fused_output_step_launch_with_an_overflowing_network(monkeypatch):
    """T3 under non-finite answers, then the fused launch.  The two-launch form (per-launch timing on) is stepped by hand and logs
    what the bf16 network answered for every row of every step; the oracle replays every game from those answers (device's order)
    and the per-game / per-job assertions of this module hold.  Then the same job through c4_session_step_head_out -- the output
    layers inside the step's launch, logits out of LDS -- with 4 and 8 games per stepping wavefront: the same status bytes and the
    same record bytes.  The share of visited positions at which the f32 module on the CPU answers non-finite is held to 2-50 %."""
    from c4a0_amd._lib import check
    from c4a0_amd.nn import InferenceNet
    from c4a0_amd.session import DeviceSession
    from tests.test_gpu_baseline_configs import _keys_to_positions

    model = _overflowing_model()
    dev = torch.device(DEV)
    net = InferenceNet(model, dev, dtype=torch.bfloat16)
    assert net.gemm == "hip" and net.fused_step_ok
    reqs, _starts = poison_job_games(FUSED_JOB)
    n, g = FUSED_JOB[2], N_POISON_SLOTS
    cap = len(reqs) * 43 * n          # a game is at most 42 moves of n simulations and n more on its last root

    def session(timing):
        s = DeviceSession(g, n, 6.6, 0.01, device=dev, planes_dtype=torch.bfloat16)
        s.set_games(reqs)
        s.set_timing(timing)
        s.bind()
        s.start()
        return s

    # ---- the two-launch form, logged
    s = session(True)
    log_k, log_o = [], []

    def log():
        keys = torch.empty(g, dtype=torch.int64, device=dev)
        check(s.L.c4_session_leaf_keys(s._h, C.c_void_p(keys.data_ptr())))
        log_k.append(keys)
        log_o.append(torch.cat([s.logprobs, s.q], dim=1))

    dead, where = {}, {}
    steps = _step_eager(s, net, cap, dead, where, on_step=log)
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    s.close()
    keys, out = torch.stack(log_k).reshape(-1), torch.stack(log_o).reshape(-1, 9)
    keys, out = keys[keys >= 0], out[keys >= 0]
    order = torch.argsort(keys, stable=True)
    keys, out = keys[order], out[order]
    dup = keys[1:] == keys[:-1]
    assert bool((out.view(torch.int32)[1:][dup] == out.view(torch.int32)[:-1][dup]).all()), "one position, two answers"
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = ~dup
    mask, value = _keys_to_positions(keys[first].cpu().numpy())
    table = np.ascontiguousarray(out[first].cpu().numpy())
    # ---- the share of the visited positions that overflow, by the f32 module on the CPU
    from tests.helpers import pos_to_planes_np

    with torch.no_grad():
        lp, qp, qn = model(torch.from_numpy(pos_to_planes_np(mask, value)))
    share = float((~(torch.isfinite(lp).all(dim=1) & torch.isfinite(qp) & torch.isfinite(qn))).float().mean())
    on_device = float((~np.isfinite(table).all(axis=1)).mean())
    print(f"fused: {len(mask)} distinct positions, non-finite on the f32 module {share:.4f}, in the bf16 network's answers {on_device:.4f}")
    assert 0.02 <= share <= 0.50, share
    # ---- the oracle's replay, game by game
    want = oracle_outcomes(FUSED_JOB, device_order=True, evaluator=_table_evaluator(mask, value, table))
    n_ok = check_against(FUSED_JOB, want, recs, counts, c, dead, where)
    codes = {k: sum(1 for v in dead.values() if v == k) for k in sorted(set(dead.values()))}
    print(f"fused: two-launch form {steps} steps, {n_ok} finished, dead by code {codes}")
    assert n_ok >= 10 and len(dead) >= 10, (n_ok, len(dead))
    # ---- the fused launch
    for gpw in (4, 8):
        s = session(False)
        s.set_step_shape(gpw)
        fused = []
        entry = s.L.c4_session_step_head_out
        monkeypatch.setattr(s.L, "c4_session_step_head_out", lambda *a: (fused.append(1), entry(*a))[1])
        dead2, where2 = {}, {}
        for step in range(1, cap + 1):
            s.round(net)
            if step % 16 == 0 and _note_dead(s, dead2, where2)[0] == 0:
                break
        r2, c2, ctr2 = s.drain_samples(), s.sample_counts(), s.counters()
        s.close()
        monkeypatch.undo()
        assert len(fused) == step, "round() did not take the fused launch"
        assert dead2 == dead and r2.tobytes() == recs.tobytes() and np.array_equal(c2, counts), gpw
        assert ctr2["games_done"] == n_ok and ctr2["error"] in set(dead.values())
    evidence(f"non-finite, fused output + step launch, bf16 1x32 network with an overflowing unit per head: {len(mask)} positions visited, "
             f"{share:.1%} non-finite on the f32 module ({on_device:.1%} in the device's answers); {len(reqs)} games: {n_ok} finished == oracle "
             f"replay of the logged answers, {len(dead)} dead by code {codes} == oracle; fused launch with 4 and 8 games per wavefront: the "
             f"same status bytes and record bytes")
