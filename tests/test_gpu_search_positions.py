"""`search_positions` on the device against the oracle, bit for bit: n simulations from a given position as root, then the root
policy and the two root q values (MctsGame::new_from_pos + the run_mcts helper, mcts.rs:48-56, 469-485).  The reference of every
comparison is tests/search_ref.py; tests/test_search_positions.py holds that fixture to its floors on the oracle alone.

  T1  the SEARCH instantiation of the step kernel (C4_FLAG_SEARCH) in DeviceSession's launch forms over tests.helpers.start_job's
      495 positions on 128 slots (three in four arrive through the refill; 45 are terminal and are searched, not closed): records,
      counts and the counter identities;
  T2  2 000 simulations per position with the default arena, n + 8 blocks per slot;
  T3  a bf16 network through every driver -- the library's own loop (c4_search_positions_bf16) and the Python loop, one and two
      sessions, few and many slots, records left on the device -- the same bytes, equal to oracle games driven in lock-step with
      the same network's answers; once with the f32 chain;
  T4  every refusal, and the session / process works afterwards;
  T5  non-finite evaluator outputs (tests.search_ref.poison_search: the hash evaluator poisoned at one position in 40, n = 8 and
      24): per position the reference's panic code in the slot's status byte, or the one record.  Here non-finite values DO reach
      records -- a NaN root q where the reference finishes the search, e.g. down a chain of single legal columns, and a NaN
      q_no_penalty, which is never compared -- so records are compared by the record rule of tests/search_ref.py: a NaN equals a
      NaN, everything else bit for bit.  The oracle plays the device's order: the select behind a search's last simulation is left
      out (the fourth counted deviation; tests/test_nonfinite_regime.py pins which searches that changes).

Without the feature every test here fails at `search=True` or at the import of `search_positions`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import (N_START_SLOTS, SHARP_MODEL_K, START_EVALS, GraphSafeHashEval, GraphSafeSharpEval, evidence, hash_eval_torch,   # noqa: E402
                           sharp_eval_torch, sharp_model, start_job)
from tests.search_ref import (C_PLY_PENALTY, POISON_SEARCH_RATE, assert_counters, assert_records_equal, long_search_positions,   # noqa: E402
                              oracle_evaluator, poison_search, same_search_outcome, search, start_job_search)

DEV = "cuda:0"

# (name, evaluator, n, planes, how it is launched)
T1_JOBS = [
    ("hash-n24-f32-eager", "hash", 24, "f32", {}),
    ("hash-n100-bf16-graph8", "hash", 100, "bf16", {"graph": 8}),
    ("k4sat-n24-bf16-compact", "k4sat", 24, "bf16", {"compact": 5}),
    ("k5sat-n100-f32-graph2", "k5sat", 100, "f32", {"graph": 2}),
    ("hash-n1-f32-eager", "hash", 1, "f32", {}),
]


def _evaluator(ev_name, graph):
    sharp = START_EVALS[ev_name][2]
    if graph:
        return GraphSafeHashEval() if sharp is None else GraphSafeSharpEval(*sharp)
    return hash_eval_torch if sharp is None else sharp_eval_torch(*sharp)


def _search_session(n_slots, n, c_expl, planes="f32", **kw):
    from c4a0_amd.session import DeviceSession

    return DeviceSession(n_slots, n, c_expl, C_PLY_PENALTY, device=torch.device(DEV),
                         planes_dtype=torch.float32 if planes == "f32" else torch.bfloat16, search=True, **kw)


def _requests(n):
    return np.stack([np.arange(n, dtype=np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)], axis=1)


def _run_compacting(s, ev, every, n_positions):
    """eager rounds with compact(8) every `every`-th step: a no-op while requests are queued, then it narrows the tail"""
    s.bind()
    s.start()
    seen = []
    for step in range(1, 100_000):
        s.evaluate(ev)
        s.step()
        if step % every == 0:
            act, rows = s.compact(8)
            seen.append((act, rows))
            assert act <= rows == s.rows and rows % 8 == 0
            if s.counters()["games_done"] >= n_positions:
                break
    widths = [r for _a, r in seen]
    assert widths[0] == N_START_SLOTS and widths[-1] == 8 and sorted(widths, reverse=True) == widths
    assert any(0 < a and r < N_START_SLOTS for a, r in seen), f"no search was moved while it ran: {seen}"
    return widths


# --------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("job", T1_JOBS, ids=[j[0] for j in T1_JOBS])
def test_searches_bit_identical_to_the_oracle(job):
    from c4a0_amd.session import SAMPLE_DTYPE

    name, ev_name, n, planes, opt = job
    _reqs, starts, _part = start_job()
    ref = start_job_search(ev_name, n)
    s = _search_session(N_START_SLOTS, n, START_EVALS[ev_name][1], planes)
    assert s.arena()["blocks_per_slot"] == n + 8 and s.arena()["reclaim_half_blocks"] == 0
    s.set_games(_requests(len(starts)), starts)
    extra = ""
    if "graph" in opt:
        s.run(_evaluator(ev_name, True), steps_per_graph=opt["graph"])
    elif "compact" in opt:
        widths = _run_compacting(s, _evaluator(ev_name, False), opt["compact"], len(starts))
        extra = f", widths {sorted(set(widths), reverse=True)}"
    else:
        s.run(_evaluator(ev_name, False))
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    packed = s.pack_samples_device().cpu().numpy().reshape(-1).view(SAMPLE_DTYPE)
    s.close()
    assert np.array_equal(counts, np.ones(len(starts), dtype=np.uint32))
    assert_records_equal(recs, ref, starts)
    assert packed.tobytes() == recs.tobytes()
    assert_counters(c, ref, len(starts), n)
    evidence(f"search T1 {name}: {len(starts)} positions, root policy / q / position / id / meta == oracle bit for bit, packed == drained, "
             f"{c['sims']} sims, S {c['select_levels']} K {c['backup_nodes']} E {c['expansions']} == oracle{extra}")


def test_the_won_root_keeps_its_search_value():
    """Pos(0b1111, 0b1111), n = 100: q_sum / (n + 1), as the oracle has it -- not the terminal value a closed game would record"""
    ref = search([(0b1111, 0b1111)], 100, oracle_evaluator("hash"), 6.6)
    s = _search_session(8, 100, 6.6)
    s.set_games(_requests(1), [(0b1111, 0b1111)])
    steps = s.run(hash_eval_torch, poll_every=1)
    recs, c = s.drain_samples(), s.counters()
    s.close()
    assert_records_equal(recs, ref, [(0b1111, 0b1111)])
    assert recs["q_penalty"][0] == np.float32(0.95049429) and recs["q_no_penalty"][0] == np.float32(0.99009901)
    assert_counters(c, ref, 1, 100)
    assert 50 <= steps < 60, steps     # the second-trip rule: two simulations of a terminal root per launch (+ the probe's lag)


# --------------------------------------------------------------------------------------------- T2
def test_long_searches_fit_the_default_arena():
    positions = long_search_positions(16)
    n = 2000
    ref = search(positions, n, oracle_evaluator("hash"), 6.6)
    assert int(ref["expansions"].max()) <= 1757
    s = _search_session(16, n, 6.6)
    assert s.arena()["blocks_per_slot"] == 2008 and s.arena()["reclaim_half_blocks"] == 0
    s.set_games(_requests(16), positions)
    s.run(GraphSafeHashEval(), steps_per_graph=16)
    recs, c = s.drain_samples(), s.counters()
    s.close()
    assert c["error"] == 0     # (5 would be C4_ERR_ARENA_OVERFLOW)
    assert_records_equal(recs, ref, positions)
    assert_counters(c, ref, 16, n)
    evidence(f"search T2: 16 positions x {n} simulations in 2 008 blocks per slot == oracle, at most {int(ref['expansions'].max())} expansions per position")


# --------------------------------------------------------------------------------------------- T3
def _net(kind, **kw):
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    kw.setdefault("dtype", torch.bfloat16)
    if kind == "sharp":
        return InferenceNet(sharp_model(4, 32, SHARP_MODEL_K), torch.device(DEV), **kw)
    torch.manual_seed(1337)
    return InferenceNet(ConnectFourNet(ModelConfig(4, 32, 4, 2)), torch.device(DEV), **kw)


def _network_reference(net, positions, n):
    """oracle games in lock-step, every round's leaves answered by ONE forward of the network (a row's outputs depend on that row
    alone: the batch the oracle asks in and the batches the sessions ask in give a position the same answer)"""
    from oracle import c4oracle as O

    rows = [0]

    def ev(leaves):
        lp, qp, qn = net.forward_numpy(np.stack([O.planes(p) for p in leaves]))
        rows[0] += len(leaves)
        return lp, qp, qn

    return search(positions, n, ev, 6.6), rows[0]


T3_DRIVERS = [   # (host_loop, resident_games, concurrent_sessions, on_device)
    ("native", 64, 1, False), ("native", 512, 2, False), ("native", 64, 2, True),
    ("python", 64, 2, False), ("python", 512, 1, False), ("python", 64, 1, True),
]


@pytest.mark.parametrize("kind", ["default", "sharp"])
def test_network_searches_same_bytes_through_every_driver(kind):
    import c4a0_amd
    from c4a0_amd.results import SearchResult

    net = _net(kind)
    assert net.path == "hip" and net.batch_invariant and net.fused_step_ok
    _reqs, starts, _part = start_job()
    positions, n = starts[:200], 32
    ref, n_rows = _network_reference(net, positions, n)
    first = None
    for host_loop, resident, sessions, on_device in T3_DRIVERS:
        stats = {}
        r = c4a0_amd.search_positions(np.array(positions, dtype=np.uint64) if on_device else positions, n, 6.6, C_PLY_PENALTY, evaluator=net,
                                      host_loop=host_loop, resident_games=resident, concurrent_sessions=sessions, on_device=on_device, stats=stats)
        if on_device:
            assert isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.uint8 and tuple(r.shape) == (200, 64)
            r = SearchResult(r.cpu().numpy())
        assert isinstance(r, SearchResult) and len(r) == 200
        assert stats["host_loop"] == host_loop and stats["concurrent_sessions"] == sessions, stats
        assert_records_equal(r.records, ref, positions)
        assert_counters(stats, ref, 200, n)
        first = first or r
        assert r == first, (host_loop, resident, sessions, on_device)
    assert first.best_moves().tolist() == np.argmax(ref["policy"], axis=1).tolist()
    evidence(f"search T3 {kind} bf16 4x32: 200 positions x {n} == oracle games answered by {n_rows} rows of the same network; "
             f"{len(T3_DRIVERS)} drivers (native / python loop, 64 / 512 slots, 1 / 2 sessions, on_device) byte-identical")


def test_f32_network_searches_through_the_python_loop():
    import c4a0_amd

    net = _net("sharp", dtype=torch.float32, hip_tower=True)
    _reqs, starts, _part = start_job()
    positions, n = starts[:200], 32
    ref, n_rows = _network_reference(net, positions, n)
    stats = {}
    r = c4a0_amd.search_positions(positions, n, 6.6, C_PLY_PENALTY, evaluator=net, host_loop="python", resident_games=64, stats=stats)
    assert stats["host_loop"] == "python"
    assert_records_equal(r.records, ref, positions)
    assert_counters(stats, ref, 200, n)
    with pytest.raises(TypeError, match="host_loop='native'"):
        c4a0_amd.search_positions(positions, n, 6.6, C_PLY_PENALTY, evaluator=net, host_loop="native")
    evidence(f"search T3 f32 chain: 200 positions x {n} == oracle games answered by {n_rows} rows of the same network (Python loop)")


# --------------------------------------------------------------------------------------------- T4
def test_session_refusals_leave_the_session_usable():
    from c4a0_amd._lib import C4Error, check
    from c4a0_amd.session import DeviceSession

    dev = torch.device(DEV)
    for kw in (dict(no_moves=True), dict(reclaim=True)):
        with pytest.raises(C4Error, match="C4_ERR_BAD_ARG.*C4_FLAG_SEARCH"):
            DeviceSession(8, 24, 6.6, 0.01, device=dev, search=True, **kw)
    with pytest.raises(C4Error, match="C4_ERR_BAD_ARG.*n_mcts_iterations"):
        DeviceSession(8, 0, 6.6, 0.01, device=dev, search=True)
    positions = long_search_positions(12)
    s = _search_session(8, 24, 6.6)
    s.set_games(_requests(12), np.array(positions, dtype=np.uint64))
    s.bind()
    for call in (lambda: s.set_dirichlet(0.3, 0.25), lambda: s.set_eval_cache(1024), s.bind_leaf_models):
        with pytest.raises(C4Error, match="C4_ERR_BAD_ARG.*search session"):
            call()
    s.set_dirichlet(0.3, 0.0)      # switching the extensions OFF is no request for them
    s.set_eval_cache(0)
    inverse = torch.zeros(8, dtype=torch.int32, device=dev)
    rows = torch.zeros((8, 2, 6, 7), dtype=torch.float32).pin_memory()
    answers = torch.zeros((8, 9), dtype=torch.float32).pin_memory()
    count = torch.zeros(1, dtype=torch.int32).pin_memory()
    with pytest.raises(C4Error, match="C4_ERR_BAD_ARG.*c4_session_unique_leaves"):
        check(s.L.c4_session_unique_leaves(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(rows.data_ptr()), None, C.c_void_p(count.data_ptr())))
    with pytest.raises(C4Error, match="C4_ERR_BAD_ARG.*c4_session_step_gather"):
        check(s.L.c4_session_step_gather(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(answers.data_ptr()), 0))
    assert not s._extensions
    s.run(hash_eval_torch)
    recs, c = s.drain_samples(), s.counters()
    s.close()
    ref = search(positions, 24, oracle_evaluator("hash"), 6.6)
    assert_records_equal(recs, ref, positions)
    assert_counters(c, ref, 12, 24)


def test_native_and_api_refusals_leave_the_process_usable():
    import c4a0_amd
    from c4a0_amd import _lib
    from c4a0_amd.native import network_struct
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig
    from c4a0_amd.session import SAMPLE_DTYPE

    torch.manual_seed(1337)
    net = InferenceNet(ConnectFourNet(ModelConfig(1, 32, 4, 2)), torch.device(DEV), dtype=torch.bfloat16)
    ns = network_struct(net)
    positions = long_search_positions(12)
    pos = np.array(positions, dtype=np.uint64)
    masks, values = np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])
    recs = np.zeros(12, dtype=SAMPLE_DTYPE)
    L = _lib.lib()

    def call(opt, cap=12, n=8):
        return L.c4_search_positions_bf16(masks.ctypes.data, values.ctypes.data, 12, n, 6.6, 0.01, C.byref(ns), C.byref(opt), recs.ctypes.data, cap, None, None)

    assert call(_lib.PlayOptions(), cap=11) == _lib.ERR_BAD_ARG and b"room for 11" in L.c4_last_error_string()
    assert call(_lib.PlayOptions(), n=0) == _lib.ERR_BAD_ARG
    for field, value in (("dirichlet_epsilon", 0.25), ("eval_cache_entries", 1024), ("flags", _lib.FLAG_RECLAIM), ("flags", _lib.FLAG_NO_RECLAIM)):
        opt = _lib.PlayOptions()
        opt.dirichlet_alpha = 0.3
        setattr(opt, field, value)
        assert call(opt) == _lib.ERR_BAD_ARG, field
    assert not recs.tobytes().strip(b"\0"), "a refused call wrote records"
    games = _lib.PlayOptions()
    games.flags = _lib.FLAG_SEARCH    # the flag belongs to the search entry point
    counts, n_recs, ids = np.zeros(12, np.uint32), C.c_uint64(), _requests(12)
    big = np.zeros(12 * 43, dtype=SAMPLE_DTYPE)
    assert L.c4_play_games_bf16(ids.ctypes.data, 12, 8, 6.6, 0.01, C.byref(ns), C.byref(games), counts.ctypes.data, big.ctypes.data, len(big),
                                C.byref(n_recs), None, None) == _lib.ERR_BAD_ARG
    with pytest.raises(TypeError, match="host_loop='native'"):
        c4a0_amd.search_positions(positions, 8, 6.6, 0.01, evaluator=hash_eval_torch, host_loop="native")
    with pytest.raises(TypeError, match="graph-safe"):
        c4a0_amd.search_positions(positions, 8, 6.6, 0.01, evaluator=hash_eval_torch, concurrent_sessions=2)
    # ... and the same process searches: the library's loop, the C call itself, and an arbitrary device callable through the Python loop
    assert call(_lib.PlayOptions()) == _lib.OK
    r = c4a0_amd.search_positions(positions, 8, 6.6, 0.01, evaluator=net)
    assert r.records.tobytes() == recs.tobytes() and np.all(recs["meta"] == 2 << 16)
    h = c4a0_amd.search_positions(pos, 24, 6.6, 0.01, evaluator=hash_eval_torch)
    assert_records_equal(h.records, search(positions, 24, oracle_evaluator("hash"), 6.6), positions)
    games_after = c4a0_amd.play_games([c4a0_amd.GameMetadata(i, 0, 0) for i in range(8)], 64, 8, 6.6, 0.01, evaluator=net)
    assert len(games_after) == 8


# --------------------------------------------------------------------------------------------- T5
T5_JOBS = [("poison-n8-f32-eager", 8, "f32", {}), ("poison-n24-bf16-graph4", 24, "bf16", {"graph": 4}), ("poison-n8-bf16-graph4", 8, "bf16", {"graph": 4})]


@pytest.mark.parametrize("job", T5_JOBS, ids=[j[0] for j in T5_JOBS])
def test_poisoned_searches_end_as_the_oracle_says(job):
    """stepped by hand until no slot is active (run() raises at its first poll); per position the status byte or the record"""
    from tests.helpers import (C4_OF_C4O, GraphSafePoisonEval, poison_eval_torch, step_eager_until_no_slot_is_active as _step_eager,
                               step_graph_until_no_slot_is_active as _step_graph)

    name, n, planes, opt = job
    _reqs, starts, _part = start_job()
    want, rows = poison_search(n, POISON_SEARCH_RATE, device_order=True)
    ref, _rows = poison_search(n, POISON_SEARCH_RATE)
    s = _search_session(N_START_SLOTS, n, START_EVALS["hash"][1], planes)
    s.set_games(_requests(len(starts)), starts)
    s.bind()
    s.start()
    dead, where = {}, {}
    if "graph" in opt:
        steps = _step_graph(s, GraphSafePoisonEval(hash_eval_torch, POISON_SEARCH_RATE), opt["graph"], rows, dead, where)
    else:
        steps = _step_eager(s, poison_eval_torch(hash_eval_torch, POISON_SEARCH_RATE), rows, dead, where)
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    s.close()
    by_id = {int(r["game_id"]): r for r in recs}
    assert len(by_id) == len(recs)
    bad, nan_q, nan_qn = [], 0, 0
    for i, (o, pos) in enumerate(zip(want, starts)):
        if o[0] == "ok":
            r = by_id.get(i)
            if r is None or i in dead or counts[i] != 1 or (int(r["mask"]), int(r["value"])) != pos or r["meta"] != 2 << 16 or \
                    not same_search_outcome(("ok", r["policy"], r["q_penalty"], r["q_no_penalty"]), o):
                bad.append((i, "finished", dead.get(i, "record differs")))
            nan_q += bool(np.isnan(o[2]))
            nan_qn += bool(np.isnan(o[3]))
        elif dead.get(i) != C4_OF_C4O[o[0]] or i in by_id or counts[i] != 0:
            bad.append((i, o, dead.get(i, "finished")))
    escaped = [i for i, (a, b) in enumerate(zip(ref, want)) if not same_search_outcome(a, b)]
    print(f"{name}: device error {c['error']} at slot {c['error_slot']}, {len(dead)} dead, escaped in the device's order {escaped}: on the device "
          f"{[dead.get(i, 'finished') for i in escaped]}")
    assert not bad, f"{len(bad)} searches differ from the oracle, first {bad[:5]}"
    n_ok = sum(1 for o in want if o[0] == "ok")
    assert len(dead) == len(starts) - n_ok and c["games_done"] == n_ok == len(recs)
    assert c["error"] in set(dead.values()) and c["error_slot"] in {where[o] for o, code in dead.items() if code == c["error"]}
    assert nan_q >= 1 and nan_qn >= 1
    evidence(f"search T5 {name}: {len(starts)} positions: {n_ok} records == oracle (a NaN equals a NaN, else bit for bit; {nan_q} with a NaN "
             f"root q, {nan_qn} with a NaN q_no_penalty), {len(dead)} dead slots == the oracle's panic codes, {len(escaped)} searches escape "
             f"the reference's panic behind the last simulation, {steps} steps")
