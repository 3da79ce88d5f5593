"""InferenceNet(head_dtype=torch.float8_e4m3fn): the opt-in fp8 hidden layers through every layer above the kernels.

The chain it runs equals the chain composed by hand from the C entry points with the net's own `fp8_scales`, bit for bit; its
construction is deterministic; `play_games` gives the same bytes whatever the schedule (the evaluator is a function of the position)
on the Python host loop from HIP graphs with the fused output + step launch; the native loop and the grouped tournament chain refuse
it by name; `search_positions` and `Engine` equal the oracle replayed from the network's own answers (no tolerance: the answers carry
whatever the fp8 chain computed); and a default InferenceNet built in the same process still equals tests/bf16_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import bf16_ref as B
from tests import fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
C_PLY_PENALTY = 0.01


def _model(blocks=4, channels=32, policy=4, value=2, seed=1337):
    from c4a0_amd.nn import ConnectFourNet, ModelConfig

    torch.manual_seed(seed)
    return ConnectFourNet(ModelConfig(blocks, channels, policy, value)).eval()


@functools.lru_cache(maxsize=None)
def _net(policy=4, value=2):
    from c4a0_amd.nn import InferenceNet

    return InferenceNet(_model(policy=policy, value=value), torch.device(DEV), head_dtype=FP8)


def _planes(n=300):
    from tests.helpers import pos_to_planes_np, random_positions

    pos = np.array(random_positions(n), dtype=np.uint64)
    return torch.from_numpy(pos_to_planes_np(pos[:, 0], pos[:, 1])).to(DEV, torch.bfloat16)


def _by_hand(net, planes):
    """The chain from the C entry points alone, with the net's fp8_scales and host-side requantised weights: tower -> quantise ->
    first layer(s) -> further layers, the last hidden layer of each head in bf16."""
    from c4a0_amd._lib import check, lib
    from c4a0_amd.nn import fold_network, quantize_head_weights

    L, st = lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    sc, c = net.fp8_scales, net.channels
    f = 42 * c
    _, _, pol_w, pol_b, val_w, val_b = fold_network(_model(policy=len(net.pol_w), value=len(net.val_w)))
    perm = lambda wt: wt.reshape(wt.shape[0], c, 42).permute(0, 2, 1).reshape(wt.shape[0], f)
    feat = net.tower(planes)
    m = feat.shape[0]
    x8 = torch.empty((m, f), dtype=torch.uint8, device=DEV)
    check(L.c4_quantize_bf16_fp8(p(feat), p(x8), m, f, feat.stride(0), f, 2.0 ** sc["first"], st))
    keep = []

    def layer(x, w, b, e_in, e_out):
        wq, e_w = quantize_head_weights(w)
        dq = R.pow2(-e_in - e_w.to(torch.int64)).float().to(DEV)
        wq, b = wq.to(DEV), b.float().to(DEV).contiguous()
        y = torch.empty((m, w.shape[0]), dtype=torch.uint8 if e_out is not None else torch.bfloat16, device=DEV)
        check(L.c4_linear_fp8(p(x), p(wq), p(dq), p(b), p(y), m, w.shape[0], w.shape[1], x.stride(0), y.stride(0), 1, 1 if e_out is not None else 0,
                              2.0 ** e_out if e_out is not None else 1.0, 0, st))
        keep.extend([wq, dq, b])
        return y

    more_p, more_v = len(pol_w) > 2, len(val_w) > 2
    if more_p == more_v:
        h = layer(x8, torch.cat([perm(pol_w[0]), perm(val_w[0])]), torch.cat([pol_b[0], val_b[0]]), sc["first"], sc["policy.1"] if more_p else None)
        hp, hv = h[:, :f], h[:, f:]
    else:
        hp = layer(x8, perm(pol_w[0]), pol_b[0], sc["first"], sc.get("policy.1"))
        hv = layer(x8, perm(val_w[0]), val_b[0], sc["first"], sc.get("value.1"))
    for i in range(1, len(pol_w) - 1):
        hp = layer(hp, pol_w[i], pol_b[i], sc[f"policy.{i}"], sc.get(f"policy.{i + 1}"))
    for i in range(1, len(val_w) - 1):
        hv = layer(hv, val_w[i], val_b[i], sc[f"value.{i}"], sc.get(f"value.{i + 1}"))
    torch.cuda.synchronize()
    return hp, hv


@pytest.mark.parametrize("policy,value", [(4, 2), (3, 3), (2, 2), (2, 4)])
def test_forward_is_the_chain_composed_by_hand(policy, value):
    from c4a0_amd._lib import check, lib

    net = _net(policy, value)
    assert net.path == "hip" and net.batch_invariant and net.graph_safe and net.fused_step_ok
    assert net.dtype == torch.bfloat16 and net.head_dtype == FP8
    assert set(net.fp8_scales) == {"first"} | {f"policy.{i}" for i in range(1, policy - 1)} | {f"value.{i}" for i in range(1, value - 1)}
    planes = _planes(300)
    hp, hv = net.forward_hidden(planes)
    wp, wv = _by_hand(net, planes)
    assert hp.dtype == hv.dtype == torch.bfloat16 and tuple(hp.shape) == tuple(hv.shape) == (300, 42 * 32)
    assert torch.equal(hp.view(torch.int16), wp.view(torch.int16)) and torch.equal(hv.contiguous().view(torch.int16), wv.contiguous().view(torch.int16))
    assert bool(hp.float().isfinite().all()) and float(hp.float().abs().max()) > 0 and float(hv.float().abs().max()) > 0
    lp, q = net.forward(planes)
    lp2 = torch.empty((300, 7), dtype=torch.float32, device=DEV)
    q2 = torch.empty((300, 2), dtype=torch.float32, device=DEV)
    ow, ovw, ob, ovb = net.head_out_operands()
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib().c4_head_out_bf16(p(wp), p(wv), p(ow), p(ovw), p(ob), p(ovb), 300, wp.shape[1], wp.stride(0), wv.stride(0), p(lp2), p(q2),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(q.view(torch.int32), q2.view(torch.int32))
    # and the numpy entry point (its own stream and graph) gives the same rows
    from tests.helpers import planes_to_pos_np  # noqa: F401  (the planes are 0 / 1: exact in f32)
    nlp, nq0, nq1 = net.forward_numpy(planes.float().cpu().numpy())
    assert np.array_equal(nlp.view(np.uint32), lp.cpu().numpy().view(np.uint32)) and np.array_equal(nq0.view(np.uint32), q[:, 0].cpu().numpy().view(np.uint32))


def test_construction_is_deterministic_and_calibration_counts():
    from c4a0_amd.nn import InferenceNet, calibration_positions, positions_to_planes

    a = _net()
    b = InferenceNet(_model(), torch.device(DEV), head_dtype=FP8)
    assert a.fp8_scales == b.fp8_scales
    la, lb = [ly for ly, _ in a.chain.first] + list(a.chain.layers.values()), [ly for ly, _ in b.chain.first] + list(b.chain.layers.values())
    assert len(la) == len(lb) == 4                               # first.policy, first.value, policy.1, policy.2
    for x, y in zip(la, lb):
        assert x["name"] == y["name"] and torch.equal(x["Wq"], y["Wq"]) and torch.equal(x["dq"], y["dq"]) and torch.equal(x["bias"], y["bias"])
    # the default calibration IS calibration_positions(4096, 0); other rows may give other scales, the same rows the same
    cal = torch.from_numpy(positions_to_planes(calibration_positions(4096, 0)))
    assert InferenceNet(_model(), torch.device(DEV), head_dtype=FP8, calibration=cal).fp8_scales == a.fp8_scales
    few = InferenceNet(_model(), torch.device(DEV), head_dtype=FP8, calibration=cal[:1])
    assert set(few.fp8_scales) == set(a.fp8_scales) and few.fp8_scales["first"] >= a.fp8_scales["first"]     # (one row of the same set)
    for bad in (dict(dtype=torch.float32), dict(hip_tower=False), dict(gemm="hipblaslt"), dict(gemm_config=11)):
        with pytest.raises(ValueError, match="fp8 hidden layers"):
            InferenceNet(_model(), torch.device(DEV), head_dtype=FP8, **bad)
    with pytest.raises(ValueError, match="hidden layer"):
        InferenceNet(_model(policy=1), torch.device(DEV), head_dtype=FP8)


def _reqs(n, first=5000, players=None):
    from c4a0_amd import GameMetadata

    return [GameMetadata(first + i, *(players(i) if players else (0, 0))) for i in range(n)]


def test_play_games_same_bytes_whatever_the_schedule():
    import c4a0_amd

    net = _net()
    fused = [0]
    orig = net.head_out_operands
    net.head_out_operands = lambda: (fused.__setitem__(0, fused[0] + 1), orig())[1]    # only the fused output + step launch asks for them
    try:
        out = {}
        for name, kw in (("32 slots", dict(resident_games=32, concurrent_sessions=1)), ("96 slots", dict(resident_games=96, concurrent_sessions=1)),
                         ("two sessions", dict(resident_games=96, concurrent_sessions=2)),
                         ("cache", dict(resident_games=96, concurrent_sessions=1, eval_cache_entries=1 << 16))):
            stats = {}
            before = fused[0]
            res = c4a0_amd.play_games(_reqs(96), 1, 20, 4.0, C_PLY_PENALTY, None, evaluator=net, stats=stats, **kw)
            recs, counts = res.to_records()
            out[name] = (recs.tobytes(), counts.tobytes())
            assert stats["host_loop"] == "python" and stats["phases"]["graph_captures"] > 0 and stats["error"] == 0, (name, stats)
            assert stats["concurrent_sessions"] == kw["concurrent_sessions"] and stats["games_done"] == 96
            if name != "cache":                                  # (noise and the cache keep evaluate() -> step())
                assert fused[0] > before, name
            else:
                assert stats["eval_cache_hits"] > 0
    finally:
        del net.head_out_operands
    for name, got in out.items():
        assert got == out["32 slots"], name
    assert len(out["32 slots"][0]) // 64 > 96 * 7


def test_native_loop_refuses_by_name():
    import c4a0_amd
    from c4a0_amd.native import network_struct

    net = _net()
    with pytest.raises(TypeError, match="fp8"):
        c4a0_amd.play_games(_reqs(8), 1, 8, 4.0, C_PLY_PENALTY, None, evaluator=net, host_loop="native")
    with pytest.raises(TypeError, match="fp8"):
        network_struct(net)


def test_a_tournament_with_an_fp8_net_takes_the_eager_path():
    import c4a0_amd
    from c4a0_amd.nn import InferenceNet

    bf = InferenceNet(_model(seed=7), torch.device(DEV))
    reqs = _reqs(24, players=lambda i: (1, 2) if i < 12 else (2, 1))
    stats = {}
    res = c4a0_amd.play_games(reqs, 1, 12, 4.0, C_PLY_PENALTY, None, evaluator={1: _net(), 2: bf}, stats=stats)
    assert stats["multi_model"] == "eager" and "fp8 hidden layers run through the Python host loop" in stats["multi_model_reason"]
    recs, counts = res.to_records()
    assert stats["games_done"] == 24 and stats["error"] == 0 and bool((counts > 0).all())
    stats = {}
    c4a0_amd.play_games(reqs, 1, 12, 4.0, C_PLY_PENALTY, None, evaluator={1: bf, 2: InferenceNet(_model(seed=8), torch.device(DEV))}, stats=stats)
    assert stats["multi_model"] == "grouped"                     # (two bf16 nets still group)


def test_search_positions_equals_the_oracle_on_the_networks_answers():
    import c4a0_amd
    from oracle import c4oracle as O
    from tests.helpers import start_job
    from tests.search_ref import assert_counters, assert_records_equal, search

    net = _net()
    _reqs_, starts, _part = start_job()
    positions, n = starts[:32], 30
    rows = [0]

    def ev(leaves):
        rows[0] += len(leaves)
        return net.forward_numpy(np.stack([O.planes(p) for p in leaves]))

    ref = search(positions, n, ev, 6.6)
    stats = {}
    r = c4a0_amd.search_positions(positions, n, 6.6, C_PLY_PENALTY, evaluator=net, resident_games=32, stats=stats)
    assert stats["host_loop"] == "python"
    assert_records_equal(r.records, ref, positions)
    assert_counters(stats, ref, 32, n)
    assert rows[0] > 32 * 10
    with pytest.raises(TypeError, match="fp8"):
        c4a0_amd.search_positions(positions, n, 6.6, C_PLY_PENALTY, evaluator=net, host_loop="native")


def test_engine_equals_the_oracle_on_the_networks_answers():
    from c4a0_amd import Engine
    from oracle import c4oracle as O
    from tests.engine_ref import RefEngine, engine_positions
    from tests.test_gpu_engine import assert_same_results, assert_same_state

    net = _net()
    positions, ids, _kinds = engine_positions()
    positions, ids = positions[:8], ids[:8]
    ev = lambda leaves: net.forward_numpy(np.stack([O.planes(p) for p in leaves]))
    e = Engine(net, 30, 6.6, C_PLY_PENALTY, positions=positions, game_ids=ids, device=torch.device(DEV), steps_per_graph=8)
    r = RefEngine(ev, 30, 6.6, positions=positions, game_ids=ids)
    e.search(30)
    r.search(30)
    assert_same_state(e, r, "search(30)", leaves=False)
    moved, want = e.make_random_moves(1.0), r.make_random_moves(1.0)
    assert np.array_equal(np.asarray(moved), np.asarray(want)) and np.array_equal(e.last_results, r.last_results)
    e.search(30)
    r.search(30)
    assert_same_state(e, r, "after the sampled move", leaves=False)
    assert_same_results(e, r)
    assert e.session.counters()["error"] == 0
    e.close()


def test_the_default_net_is_left_alone():
    """A default InferenceNet built AFTER an fp8 one in the same process: still the bf16 chain, bit for bit tests/bf16_ref.py's on an
    exact-grid network."""
    from c4a0_amd.nn import InferenceNet, _Bf16Chain, _Fp8HeadChain

    _net()
    model = B.eval_model(4, 32)
    net = InferenceNet(model, torch.device(DEV))
    assert net.head_dtype is None and net.fp8_scales is None and type(net.chain) is _Bf16Chain and not isinstance(net.chain, _Fp8HeadChain)
    planes = B.grid_planes(130, seed=3).to(DEV)
    hp, hv = net.forward_hidden(planes)
    rp, rv = B.hidden(planes, B.operands_from_net(net))
    assert torch.equal(hp.double(), rp) and torch.equal(hv.double(), rv)
