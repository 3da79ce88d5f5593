"""The tree kernels against the oracle in the regime a trained network puts them in: peaked priors (legal priors of exactly 0 and
subnormal ones after the tree's own masked softmax), saturated values (q = +-1), searches 13 levels deep on average with 40 % of
the simulations below level 16 -- the slot's second line, Slot::path_deep, written by select_leaf, read back by the backup and by
k_arena_reclaim -- and moves that follow a move with no search between.  The hash evaluator and a default-initialised network
leave all of that nearly untouched at n <= 100 (0.02 % of the simulations below level 16); tests/test_sharp_regime.py holds the
oracle alone, on the same jobs, to the floors that prove these jobs are in the regime.  Everything here is bit for bit.

  T1  DeviceSession / play_games against O.self_play under the sharp evaluators (tests.helpers.SHARP_JOBS): plain, gather and
      cached step kernels, Dirichlet noise, reclaimed arenas, eager launches and HIP-graph replay;
  KAT one line from the empty board to the full board (42 levels) under a constant evaluator;
  T3  the fused output + step launch (c4_out_step_kernel, 4 and 8 games per wavefront) under a sharpened bf16 network: an eager
      run logs every evaluator row, the oracle replays the job from those answers, and every layout of play_games must return
      the records the oracle confirmed; the same for a subset of the 8 x 64, n = 800 shape and for the f32 chain.

What the file is sensitive to (value-only changes to select_leaf / the backup, library rebuilt per change): a backup that does not
negate the value at path levels >= 16 fails 12 of the T1 / KAT cases, `1e-8f` dropped from the prior term fails 7 T1 cases (none of
the hash-evaluator parity tests at n <= 100), equal keys going to the first column fail all 17.  Removing `score + 0.0f` fails
nothing and cannot: q sums are never -0 (x + -x and +0 + -0 are +0), so -q is at most -0 and -0 + (c_exploration * ex >= +0) is +0."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import (N_SHARP_SLOTS, SHARP_EVALS, SHARP_JOBS, SHARP_MODEL_K, GraphSafeSharpEval, evidence,   # noqa: E402
                           oracle_samples_by_game, samples_by_game, sharp_eval_np, sharp_eval_torch, sharp_job_reqs, sharp_model)

DEV = "cuda:0"
THREADS = max(2, min(16, os.cpu_count() or 2))


def _share(st):
    return f"{100.0 * st['sims_deep'] / max(1, st['sims']):.1f} % of {st['sims']} simulations at depth >= 16 (max {st['max_depth']})"


def _assert_counters(c, ost):
    """the device counters are the oracle's (tests/test_gpu_mcts_parity.py: the device skips terminal-root simulations and the
    select whose leaf a move discards)"""
    assert c["error"] == 0
    assert c["sims"] + c["ref_skipped_sims"] == ost["sims"]
    assert c["ref_skipped_sims"] == ost["sims_terminal_root"]
    assert c["select_levels"] == ost["select_levels"] - ost["select_levels_discarded"]
    assert c["backup_nodes"] == ost["backup_nodes"]
    assert c["expansions"] == ost["expansions"]
    assert c["moves"] == ost["moves"]


# --------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("job", SHARP_JOBS, ids=[j[0] for j in SHARP_JOBS])
def test_self_play_sharp_evaluator_bit_identical(job):
    """T1: every sample of every game and the work counters equal the oracle's; 512 games on 256 slots, so every slot is refilled
    and the launch has 32 stepping wavefronts."""
    import c4a0_amd
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.test_gpu_reclaim import _half_min

    name, ev_name, n, planes, first_id, opt = job
    ev, c_expl = SHARP_EVALS[ev_name]
    reqs = sharp_job_reqs(first_id)
    noise = opt.get("dirichlet")
    ores, ost = O.self_play(reqs, 4096, n, c_expl, 0.01, ("sharp",) + ev, n_threads=THREADS, topology="async", dirichlet=noise or (0.0, 0.0))
    want = oracle_samples_by_game(ores)
    dev = torch.device(DEV)
    if opt.get("callback"):   # the numpy callback: unique leaves out, answers back through the gather step kernel
        st = {}
        res = c4a0_amd.play_games([c4a0_amd.GameMetadata(*r) for r in reqs], 200, n, c_expl, 0.01, sharp_eval_np(*ev), device=dev,
                                  resident_games=N_SHARP_SLOTS, stats=st)
        recs, counts = res.to_records()
        c = st
        assert st["nn_positions"] > 0
    else:
        kw = {}
        if "reclaim" in opt:      # the tightest halves the library accepts, looked at every `period`-th launch
            kw = dict(reclaim=True, reclaim_period=opt["reclaim"], blocks_per_slot=2 * _half_min(n, opt["reclaim"]))
        s = DeviceSession(N_SHARP_SLOTS, n, c_expl, 0.01, device=dev, planes_dtype=torch.float32 if planes == "f32" else torch.bfloat16, **kw)
        s.set_games(reqs)
        if noise:
            s.set_dirichlet(*noise)
        if "cache" in opt:
            s.set_eval_cache(*opt["cache"])
        if "graph" in opt:
            s.run(GraphSafeSharpEval(*ev), steps_per_graph=opt["graph"])
        else:
            s.run(sharp_eval_torch(*ev))
        recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
        s.close()
        if "cache" in opt:
            assert 0 < c["eval_cache_hits"] <= c["eval_cache_probes"]
        if "reclaim" in opt:
            # a game allocates at most one half between two copies of its live subtree, so it is copied at least expansions / half - 1 times
            half = _half_min(n, opt["reclaim"])
            floor = ost["expansions"] // half - len(reqs)
            assert floor >= len(reqs) // 2, "the job does not need its arenas reclaimed"
            assert c["reclaim_passes"] >= floor, c
    got = samples_by_game(recs)
    assert set(got) == set(want)
    for gid in want:
        assert got[gid] == want[gid], f"game {gid} differs"
    assert c["games_done"] == len(reqs) and c["samples"] == ost["n_samples"] == len(recs)
    assert np.array_equal(counts, [len(ores[g]) for g, _, _ in reqs])
    _assert_counters(c, ost)
    # sampled from root policies that hold real zeros: legal columns the search never visited
    legal_zero = sum(1 for ss in want.values() for m, _v, pol, _a, _b in ss[:-1]
                     if ((np.frombuffer(pol, dtype=np.float32) == 0.0) & (((m >> (35 + np.arange(7))) & 1) == 0)).any())
    assert legal_zero > 0
    evidence(f"sharp regime T1 {name}: {len(reqs)} games, {len(recs)} samples == oracle bit for bit, counters equal; {_share(ost)}, "
             f"{ost['moves_without_search']} of {ost['moves']} moves straight after a move, {legal_zero} root policies with a legal zero")


# --------------------------------------------------------------------------------------------- line KAT
@pytest.mark.parametrize("n_iter", [200, 500, 1500])
def test_line_kat_to_the_full_board_matches_oracle(n_iter):
    """tests/test_sharp_regime.py's line: constant logits and q = +1, no moves -- the search goes down one line to the full board,
    42 levels, every entry of the deep path.  Root policy, both q and the counters equal the oracle's."""
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.test_sharp_regime import LINE_KAT

    dev = torch.device(DEV)
    lp = torch.tensor([LINE_KAT["logits"]], dtype=torch.float32, device=dev)
    q = torch.tensor([list(LINE_KAT["q"])], dtype=torch.float32, device=dev)
    s = DeviceSession(1, 1 << 30, LINE_KAT["c_exploration"], LINE_KAT["c_ply_penalty"], device=dev, blocks_per_slot=n_iter + 8, no_moves=True)
    s.set_games([(0, 0, 0)], [(0, 0)])
    s.bind()
    s.start()
    s.evaluate(lambda planes: (lp, q))   # constant: evaluate once, the bound tensors never change
    for _ in range(n_iter):
        s.step()
    pol, qp, qn, n, root = s.root_stats(0)
    c = s.counters()
    s.close()
    opol, oqp, oqn, g = O.run_mcts(O.Pos(0, 0), n_iter, LINE_KAT["c_exploration"], LINE_KAT["c_ply_penalty"], LINE_KAT["logits"], LINE_KAT["q"])
    oc = g.counters()
    assert c["error"] == 0 and n == n_iter and root == (0, 0)
    bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(pol), bits(opol)) and np.array_equal(bits([qp, qn]), bits([oqp, oqn]))
    assert (c["sims"], c["select_levels"], c["backup_nodes"], c["expansions"]) == (oc["sims"], oc["select_levels"], oc["backup_nodes"], oc["expansions"])
    assert oc["max_depth"] >= (40 if n_iter >= 500 else 16)
    evidence(f"sharp regime line KAT, {n_iter} iterations: root policy, q and counters == oracle; max depth {oc['max_depth']}, "
             f"{oc['sims_deep']} simulations at depth >= 16, {oc['sims_deep_terminal']} of them on a terminal leaf")


# --------------------------------------------------------------------------------------------- T3: the fused launch
def _sharp_net(blocks, channels, **kw):
    from c4a0_amd.nn import InferenceNet

    kw.setdefault("dtype", torch.bfloat16)
    return InferenceNet(sharp_model(blocks, channels, SHARP_MODEL_K), torch.device(DEV), **kw)


def _t3(net, ids, n_slots, n_iter, planes_dtype=torch.bfloat16):
    """Eager run logging every evaluator row -> the oracle replays the job from those answers.  Returns (records bytes, counts
    bytes, the oracle's statistics) after asserting that every sample equals the oracle's."""
    from oracle import c4oracle as O
    from tests.test_gpu_baseline_configs import _run_logging_every_row

    recs, counts, ctr, table, (n_rows, n_dup) = _run_logging_every_row(net, ids, n_slots, n_iter, planes_dtype=planes_dtype)
    assert ctr["games_done"] == len(ids) and ctr["error"] == 0
    ores, ost = O.self_play([(g, 0, 0) for g in ids], 4096, n_iter, 6.6, 0.01, ("table",) + table, n_threads=THREADS, topology="async")
    assert samples_by_game(recs) == oracle_samples_by_game(ores)
    _assert_counters(ctr, ost)
    # the replay's own counters: the reference, fed the device's answers, searched deep (floor from the issue; bf16 answers differ
    # from the f32 model's, whose floor on the CPU is 10 %)
    assert ost["sims_deep"] >= 0.03 * ost["sims"], _share(ost)
    return recs, counts, ost, n_rows


def _play(net, ids, n_iter, **kw):
    import c4a0_amd

    cb = kw.pop("cb", None)
    res = c4a0_amd.play_games([c4a0_amd.GameMetadata(g, 0, 0) for g in ids], kw.pop("max_batch", 4096), n_iter, 6.6, 0.01, cb, **kw)
    recs, counts = res.to_records()
    return recs.tobytes(), counts.tobytes()


def test_fused_launch_under_a_sharpened_network_t3_and_every_layout(monkeypatch):
    """The headline kernel walks deep paths: sharp_model(4, 32) as a bf16 InferenceNet, 1 536 games at n = 100.  The eager run
    (separate output and step launches) is replayed by the oracle from the evaluator's own answers; then every layout of
    play_games -- each of them the fused output + step launch in a HIP graph, but for the callback -- must return those bytes:
    resident 300 / 1 024 / 4 096, one and two sessions, 4 and 8 games per stepping wavefront, the Python and the native host loop,
    the evaluation cache, the numpy callback (laid out as tests/test_gpu_invariance.py)."""
    from c4a0_amd import session as S

    net = _sharp_net(4, 32)
    assert net.gemm == "hip" and net.fused_step_ok
    n_iter, ids = 100, [9000 + 3 * i for i in range(1536)]
    recs, counts, ost, n_rows = _t3(net, ids, 512, n_iter)
    ref = (recs.tobytes(), counts.tobytes())
    variants = {
        "native loop, resident 4096, two sessions": dict(evaluator=net, resident_games=4096, concurrent_sessions=2),
        "native loop, resident 1024, one session": dict(evaluator=net, resident_games=1024, concurrent_sessions=1),
        "native loop, resident 1024, two sessions": dict(evaluator=net, resident_games=1024, concurrent_sessions=2),
        "native loop, resident 300 (odd batch shape)": dict(evaluator=net, resident_games=300),
        "native loop, evaluation cache on": dict(evaluator=net, resident_games=4096, eval_cache_entries=1 << 20),
        "Python loop, resident 4096, one session": dict(evaluator=net, resident_games=4096, concurrent_sessions=1, host_loop="python"),
        "Python loop, resident 1024, one session, cache": dict(evaluator=net, resident_games=1024, concurrent_sessions=1, eval_cache_entries=1 << 20, host_loop="python"),
    }
    for name, kw in variants.items():
        assert _play(net, ids, n_iter, **kw) == ref, name
    for gpw in (4, 8):   # the knob lives in the Python loop's paired graph; a session alone keeps 8
        monkeypatch.setattr(S, "PAIRED_STEP_GAMES_PER_WAVEFRONT", gpw)
        assert _play(net, ids, n_iter, evaluator=net, resident_games=700, concurrent_sessions=2, host_loop="python") == ref, gpw

    def cb(_model_id, x):   # the shape of ConnectFourNet.forward_numpy (nn.py:119-130)
        with torch.no_grad():
            lp, q = net(torch.from_numpy(x).to(DEV))
            lp, q = lp.float().cpu().numpy(), q.float().cpu().numpy()
        return np.ascontiguousarray(lp), np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])

    assert _play(net, ids, n_iter, cb=cb, max_batch=333, resident_games=512) == ref, "numpy callback"
    evidence(f"sharp regime T3, bf16 4x32 network sharpened 2^{SHARP_MODEL_K}: {len(ids)} games, {len(recs)} samples == oracle replay of {n_rows} logged "
             f"evaluator rows; {len(variants) + 3} layouts of play_games (fused output + step launch) byte-identical to it; {_share(ost)}")


def test_fused_launch_config4_shape_subset_t3():
    """A subset of BASELINE config 4's shape (8 x 64 network, n = 800), sharpened: T3 replay of every game, and the fused launch
    (one session and two) returns the confirmed bytes."""
    net = _sharp_net(8, 64)
    n_iter, ids = 800, list(range(400, 496))
    recs, counts, ost, n_rows = _t3(net, ids, len(ids), n_iter)
    ref = (recs.tobytes(), counts.tobytes())
    assert _play(net, ids, n_iter, evaluator=net, resident_games=len(ids), concurrent_sessions=1) == ref
    assert _play(net, ids, n_iter, evaluator=net, resident_games=64, concurrent_sessions=2, host_loop="python") == ref
    evidence(f"sharp regime T3, bf16 8x64 network sharpened 2^{SHARP_MODEL_K}, n = 800: {len(ids)} games, {len(recs)} samples == oracle replay "
             f"of {n_rows} logged rows, fused launch byte-identical; {_share(ost)}")


def test_f32_chain_under_the_same_sharpening_t3():
    """256 games with the f32 chain (exact-f32 MFMA kernels) and the same sharpening: T3."""
    net = _sharp_net(4, 32, dtype=torch.float32, hip_tower=True, strict=True)
    ids = list(range(256))
    recs, _counts, ost, n_rows = _t3(net, ids, 256, 100, planes_dtype=torch.float32)
    evidence(f"sharp regime T3, f32 4x32 network sharpened 2^{SHARP_MODEL_K}: {len(ids)} games, {len(recs)} samples == oracle replay of {n_rows} "
             f"logged rows; {_share(ost)}")
