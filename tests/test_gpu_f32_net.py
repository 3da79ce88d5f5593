"""The f32 evaluator on the GPU (InferenceNet(dtype=torch.float32, hip_tower=True): c4_conv_tower_f32 + c4_linear_f32 +
c4_head_out_f32 on exact-f32 MFMA) against the plain-C restatement of its documented summation order
(tests/f32_net_ref.c) bit for bit, against the reference's own outputs, batch invariance, and self-play with it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f32_ref as R  # noqa: E402
from test_f32_net_ref import MATRIX, TOL, _fixture_models, random_model, random_planes  # noqa: E402

DEV = "cuda:0"


def _net(model, **kw):
    from c4a0_amd.nn import InferenceNet

    return InferenceNet(model, torch.device(DEV), dtype=torch.float32, hip_tower=True, strict=True, **kw)


def _gpu_layers(net, x):
    """Every intermediate of the GPU chain: features, each head's hidden activations, pre-activations [G, 9], logprobs, q."""
    planes = torch.from_numpy(x).to(DEV)
    feat = net.tower(planes)
    hp = net.hp
    pol, val = [], []
    if net.merged_w1 is not None:
        h = net._linear_relu(feat, net.merged_w1, net.merged_b1)
        p, v = h[:, :hp], h[:, hp:]
        pol.append(p), val.append(v)
        rest_p, rest_v = zip(net.pol_w[1:-1], net.pol_b[1:-1]), zip(net.val_w[1:-1], net.val_b[1:-1])
    else:
        p = v = feat
        rest_p, rest_v = zip(net.pol_w[:-1], net.pol_b[:-1]), zip(net.val_w[:-1], net.val_b[:-1])
    for w, b in rest_p:
        p = net._linear_relu(p, w, b)
        pol.append(p)
    for w, b in rest_v:
        v = net._linear_relu(v, w, b)
        val.append(v)
    pre = torch.empty((x.shape[0], 9), dtype=torch.float32, device=DEV)
    lp, q = net._head_out_f32(p, v, out_preact=pre)
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()
    return {"features": n(feat), "policy_hidden": [n(t) for t in pol], "value_hidden": [n(t) for t in val], "preact": n(pre),
            "logprobs": n(lp), "q": n(q)}


def _ulp_distance(a, b):
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    return np.abs(ia - ib)


def test_f32_mfma_is_one_fmaf_chain_in_the_documented_order():
    """The probe of the guide's claim: c4_linear_f32 on operands whose sums depend on the order (magnitudes over 2^60,
    heavy cancellation, subnormals) equals the C chain bit for bit -- and differs from other orders."""
    rng = np.random.default_rng(7)
    m, n, k = 37, 64, 256
    x = (rng.standard_normal((m, k)) * np.exp2(rng.integers(-30, 30, (m, k)))).astype(np.float32)
    w = (rng.standard_normal((n, k)) * np.exp2(rng.integers(-30, 30, (n, k)))).astype(np.float32)
    x[0, :8] = np.float32(1e-41)                     # subnormal inputs come through unflushed
    w[0, :8] = np.float32(0.5)
    b = rng.standard_normal(n).astype(np.float32)
    want = R.linear(x, w, b, 0)
    from c4a0_amd._lib import check, lib

    xd, wd, bd = (torch.from_numpy(a).to(DEV) for a in (x, w, b))
    y = torch.empty((m, n), dtype=torch.float32, device=DEV)
    check(lib().c4_linear_f32(C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(bd.data_ptr()), C.c_void_p(y.data_ptr()),
                              m, n, k, k, n, 0, None))
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the order matters on these operands: a chain in natural k order gives other bits somewhere
    nat = np.zeros((m, n), np.float32)
    for kk in range(k):
        nat = (nat.astype(np.float64) + x[:, kk][:, None].astype(np.float64) * w[:, kk][None, :].astype(np.float64)).astype(np.float32)
    assert not np.array_equal(nat + b, got)


@pytest.mark.parametrize("cfg", MATRIX, ids=lambda c: "x".join(map(str, c)))
def test_every_layer_equals_the_c_reference_bit_for_bit(cfg):
    from oracle import c4oracle as O

    def host(fn):
        def f(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            out = np.empty_like(a)
            fn(a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), a.size)
            return out
        return f

    expf, logf = host(O.lib().c4o_host_expf), host(O.lib().c4o_host_logf)
    model = random_model(cfg, 21)
    net = _net(model)
    assert net.path == "hip" and net.batch_invariant and not net.fused_step_ok
    pk = R.pack_on_cpu(model)
    for rows in (1, 5, 128, 300):
        x = random_planes(rows, rows)
        want, got = R.forward(pk, x), _gpu_layers(net, x)
        assert np.array_equal(got["features"], want["features"]), (cfg, rows)
        for name in ("policy_hidden", "value_hidden"):
            assert len(got[name]) == len(want[name])
            for g, w in zip(got[name], want[name]):
                assert np.array_equal(g, w), (cfg, rows, name)
        assert np.array_equal(got["preact"], want["preact"]), (cfg, rows)
        assert np.array_equal(got["logprobs"], R.log_softmax_documented(want["preact"][:, :7], expf, logf)), (cfg, rows)
        assert _ulp_distance(got["q"], np.tanh(want["preact"][:, 7:].astype(np.float64))).max() <= 2


def test_reference_fixtures():
    for name, z, model in _fixture_models():
        net = _net(model)
        lp, q = net(torch.from_numpy(z["x"]).to(DEV))
        lp, q = lp.cpu().numpy(), q.cpu().numpy()
        assert np.abs(lp - z["policy_logprobs"]).max() <= TOL, name
        assert np.abs(q[:, 0] - z["q_penalty"]).max() <= TOL and np.abs(q[:, 1] - z["q_no_penalty"]).max() <= TOL, name


def test_batch_invariance_permutation_and_forward_numpy():
    model = random_model((4, 32, 4, 2), 5)
    net = _net(model)
    x = random_planes(4097, 9)
    xd = torch.from_numpy(x).to(DEV)
    lp, q = net(xd)
    full = torch.cat([lp, q], 1).cpu().numpy()
    for n in (1, 2, 3, 17, 64, 65, 300, 1023, 1024, 2048, 2049, 4096):
        for start in (0, 4097 - n):
            a, b = net(xd[start:start + n])
            assert np.array_equal(torch.cat([a, b], 1).cpu().numpy(), full[start:start + n]), (n, start)
    perm = np.random.default_rng(3).permutation(4097)
    a, b = net(xd[torch.from_numpy(perm).to(DEV)])
    assert np.array_equal(torch.cat([a, b], 1).cpu().numpy(), full[perm])
    for n in (1, 129, 4097):
        l2, qp, qn = net.forward_numpy(x[:n])
        assert np.array_equal(l2, full[:n, :7]) and np.array_equal(qp, full[:n, 7]) and np.array_equal(qn, full[:n, 8])
    pinned = torch.from_numpy(x[:333]).pin_memory()
    l2, qp, qn = net.forward_numpy(pinned.numpy())
    assert np.array_equal(l2, full[:333, :7]) and np.array_equal(qn, full[:333, 8])


def test_refusals_and_defaults():
    from c4a0_amd.nn import ConnectFourNet, EvaluatorFallbackWarning, InferenceNet, ModelConfig

    dev = torch.device(DEV)
    m = ConnectFourNet(ModelConfig(1, 32, 2, 2))
    for kw in ({"gemm": "hipblaslt"}, {"gemm_config": 3}, {"tower_config": 2}):
        with pytest.raises(ValueError):
            InferenceNet(m, dev, dtype=torch.float32, hip_tower=True, **kw)
    with pytest.raises(ValueError):
        InferenceNet(ConnectFourNet(ModelConfig(1, 65, 2, 2)), dev, dtype=torch.float32, hip_tower=True)
    with pytest.warns(EvaluatorFallbackWarning, match="hip_tower=True"):
        net = InferenceNet(m, dev, dtype=torch.float32)
    assert net.path == "torch"
    net = InferenceNet(ConnectFourNet(ModelConfig(2, 3, 1, 3)), dev, dtype=torch.float32, hip_tower=True, strict=True)
    lp, q = net(torch.from_numpy(random_planes(70, 1)).to(DEV))
    assert lp.shape == (70, 7) and torch.isfinite(lp).all() and q.shape == (70, 2)


def _records(net, reqs, **kw):
    from c4a0_amd import play_games

    r = play_games(reqs, 4096, 16, 6.6, 0.01, evaluator=net if "py_eval_pos_cb" not in kw else None, **kw)
    return r.to_records()[0].tobytes()


def test_play_games_with_the_f32_net_same_bytes_everywhere():
    import c4a0_amd

    torch.manual_seed(3)
    from c4a0_amd.nn import ConnectFourNet, ModelConfig

    net = _net(ConnectFourNet(ModelConfig(1, 32, 4, 2)).eval())
    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(1200)]
    base = _records(net, reqs, resident_games=300)
    assert _records(net, reqs, resident_games=1024) == base
    assert _records(net, reqs, resident_games=4096) == base
    assert _records(net, reqs, resident_games=1024, concurrent_sessions=2) == base
    assert _records(net, reqs, resident_games=1024, eval_cache_entries=1 << 16) == base
    cb = lambda _mid, x: net.forward_numpy(x)
    assert _records(net, reqs[:300], py_eval_pos_cb=cb, resident_games=300) == _records(net, reqs[:300], resident_games=300)
    with pytest.raises(TypeError):
        c4a0_amd.play_games(reqs[:8], 64, 4, 6.6, 0.01, evaluator=net, host_loop="native")


def test_oracle_replays_a_config2_shape_job_from_the_f32_nets_answers():
    """256 games of a config-2-shape job (4 x 32 network, n = 100) with the f32 net: every evaluator row logged, the distinct
    positions become the oracle's evaluator, every game's samples equal the oracle's bit for bit (tools/full_t3.py's method)."""
    from c4a0_amd._lib import check
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.helpers import oracle_samples_by_game, samples_by_game
    from tests.test_gpu_baseline_configs import _keys_to_positions

    torch.manual_seed(1337)
    net = _net(ConnectFourNet(ModelConfig(4, 32, 4, 2)).eval())
    n, n_iter = 256, 100
    ids = list(range(n))
    dev = torch.device(DEV)
    s = DeviceSession(n, n_iter, 6.6, 0.01, device=dev, planes_dtype=torch.float32)
    s.set_games([(g, 0, 0) for g in ids])
    log_k, log_o = [], []

    def log(_step):
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        check(s.L.c4_session_leaf_keys(s._h, C.c_void_p(keys.data_ptr())))
        log_k.append(keys)
        log_o.append(torch.cat([s.logprobs, s.q], dim=1))

    s.run(net, on_step=log, poll_every=64)
    recs, ctr = s.drain_samples(), s.counters()
    s.close()
    assert ctr["games_done"] == n and ctr["error"] == 0
    keys, out = torch.stack(log_k).reshape(-1), torch.stack(log_o).reshape(-1, 9)
    live = keys >= 0
    keys, out = keys[live], out[live]
    order = torch.argsort(keys, stable=True)
    keys, out = keys[order], out[order]
    dup = keys[1:] == keys[:-1]
    assert bool((out.view(torch.int32)[1:][dup] == out.view(torch.int32)[:-1][dup]).all())
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = ~dup
    mask, value = _keys_to_positions(keys[first].cpu().numpy())
    o = np.lexsort((value, mask))
    table = (mask[o], value[o], np.ascontiguousarray(out[first].cpu().numpy()[o]))
    want, _ = O.self_play([(g, 0, 0) for g in ids], 4096, n_iter, 6.6, 0.01, ("table",) + table, n_threads=8, topology="async")
    assert samples_by_game(recs) == oracle_samples_by_game(want)
