"""The bf16 evaluator's kernels (c4_linear_bf16, c4_conv_tower_bf16, c4_head_out_bf16, and InferenceNet's chain of them)
against tests/bf16_ref.py, the float64 restatement with the documented rounding points (include/c4a0_hip.h).

On exact-grid data (every partial sum an exact f32 in any order, proved per layer by bf16_ref.check_exact) the kernels must
equal the reference BIT FOR BIT: only where and how they round is under test (tests/test_bf16_ref.py shows the data tells a
truncating or ties-away conversion, a misplaced ReLU, a lost bias, a wrong or wrapped tap, a lost residual, a dropped k-tile,
an offset row and a skipped column permutation from the true chain).  On realistic data the GEMM must lie inside the
rigorous interval bf16_ref.interval gives for any f32 summation order.  Output tensors carry sentinels past their last row and
column (and between n and the row stride), which must come back untouched.  bf16 results are compared as values (+0 == -0)."""
import ctypes as C

import pytest
import torch

from tests import bf16_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A            # a bf16 bit pattern no kernel computes here (about 1.5e16)

GEMM_CONFIGS = list(range(1, 60))
# both sides of every cut of the automatic tables (32 channels: 384 / 640 / 896 / 1 024, K >= 2 048: 384 / 640 / 1 024), of
# nn.py's latency_mode choices (1 152, 1 728), tile multiples +- 1, and the bench's sizes
GEMM_M_AUTO = [1, 63, 65, 95, 97, 127, 129, 191, 193, 255, 257, 383, 384, 385, 639, 640, 641, 895, 896, 897, 1023, 1024, 1025,
               1151, 1152, 1153, 1727, 1728, 1729, 2048, 4095, 4096]
GEMM_M_EXPLICIT = [1, 193, 1025, 4095]
PAD = 64                     # extra columns of the strided x (NaN: a read past k shows) and of the strided y (sentinels)


def _lib():
    from c4a0_amd import _lib as L

    return L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.float(), b.float())


def _untouched(t: torch.Tensor) -> bool:
    return bool((t.view(torch.int16) == SENTINEL).all())


def _sentinel_buf(rows: int, cols: int, dtype=torch.bfloat16) -> torch.Tensor:
    t = torch.empty((rows, cols), dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(SENTINEL if dtype == torch.bfloat16 else 0x5A5A5A5A)
    return t


# ------------------------------------------------------------------------------------------------------------------ GEMM
@pytest.fixture(scope="module", params=R.GEMM_SHAPES, ids=lambda s: f"K{s[0]}-N{s[1]}")
def gemm(request):
    k, n = request.param
    x, w, b = R.gemm_case(k, n)
    xs = torch.full((R.GEMM_M, k + PAD), float("nan"), dtype=torch.bfloat16, device=DEV)
    xs[:, :k] = x.to(DEV)
    w, b = w.to(DEV).contiguous(), b.to(DEV).contiguous()
    st = {}
    ref = {relu: R.linear(xs[:, :k], w, b, relu, stats=st if relu == 0 else None) for relu in (0, 1)}   # check_exact at full size
    return {"k": k, "n": n, "x": xs[:, :k], "w": w, "b": b, "ref": ref, "ties": st["ties"][0]}


def _run_linear(x, w, b, m, relu, config):
    from c4a0_amd._lib import check

    n, k = w.shape
    y = _sentinel_buf(m + 3, n + PAD)
    check(_lib().c4_linear_bf16(C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(y.data_ptr()),
                                m, n, k, x.stride(0), y.stride(0), relu, config, _stream()))
    return y


@pytest.mark.parametrize("config", [0] + GEMM_CONFIGS)
def test_linear_exact_grid_bit_for_bit(gemm, config):
    k, n = gemm["k"], gemm["n"]
    down, up = gemm["ties"]
    assert down >= 100 and up >= 100, gemm["ties"]
    for relu in (0, 1):
        for m in (GEMM_M_AUTO if config == 0 else GEMM_M_EXPLICIT):
            y = _run_linear(gemm["x"], gemm["w"], gemm["b"], m, relu, config)
            assert _same(y[:m, :n], gemm["ref"][relu][:m]), f"K {k} N {n} config {config} relu {relu} m {m}: differs from the reference"
            assert _untouched(y[:m, n:]) and _untouched(y[m:]), f"K {k} N {n} config {config} relu {relu} m {m}: wrote past its output"


@pytest.mark.parametrize("k,n", R.GEMM_SHAPES)
def test_linear_realistic_data_inside_the_interval(k, n):
    x, w, b = R.realistic_linear(R.GEMM_M, k, n, seed=k * n)
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
    lo, hi = {}, {}
    for relu in (0, 1):
        lo[relu], hi[relu] = R.interval(x, w, b, relu)
    for config in (0, 1, 7, 11, 17, 19, 31, 32, 35, 46, 59):
        for m in (1, 1025, 4096) if config else (1, 385, 1025, 4096):
            for relu in (0, 1):
                y = _run_linear(x, w, b, m, relu, config)
                yy = y[:m, :n].double()
                ok = (lo[relu][:m] <= yy) & (yy <= hi[relu][:m])
                assert bool(ok.all()), f"K {k} N {n} config {config} relu {relu} m {m}: {int((~ok).sum())} outputs outside the bound"
                assert _untouched(y[:m, n:]) and _untouched(y[m:])


# ------------------------------------------------------------------------------------------------------------------ tower
TOWER_N_AUTO = [1, 2, 3, 255, 511, 512, 513, 1023, 1024, 1025, 1279, 1280, 1281, 2047, 2049]
TOWER_N_EXPLICIT = [1, 3, 513, 2049]


def _run_tower(planes, ops, n, config, n_blocks=None):
    from c4a0_amd._lib import check

    c = ops["channels"]
    out = _sentinel_buf(n + 2, 42 * c)
    check(_lib().c4_conv_tower_bf16(C.c_void_p(planes.data_ptr()), C.c_void_p(ops["tw0"].data_ptr()), C.c_void_p(ops["tw"].data_ptr()),
                                    C.c_void_p(ops["tbias"].data_ptr()), n, c, ops["n_blocks"] if n_blocks is None else n_blocks,
                                    C.c_void_p(out.data_ptr()), config, _stream()))
    return out


def _tower_on_device(channels, blocks, n=R.TOWER_N):
    planes, ops = R.tower_case(channels, blocks, n)
    ops = {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}
    planes = planes.to(DEV).contiguous()
    return planes, ops, R.tower(planes, ops)    # check_exact, layer by layer, at full size


@pytest.mark.parametrize("channels", [32, 64])
@pytest.mark.parametrize("blocks", R.TOWER_BLOCKS)
def test_tower_exact_grid_bit_for_bit(channels, blocks):
    planes, ops, ref = _tower_on_device(channels, blocks)
    for config in range(0, 6 if channels == 32 else 7):
        for n in (TOWER_N_AUTO if config == 0 else TOWER_N_EXPLICIT):
            out = _run_tower(planes, ops, n, config)
            assert _same(out[:n], ref[:n]), f"{channels} channels, {blocks} blocks, config {config}, {n} boards: differs from the reference"
            assert _untouched(out[n:]), f"{channels} channels, {blocks} blocks, config {config}, {n} boards: wrote past the last board"


def test_tower_64_config_4_runs_23_blocks_and_refuses_24():
    from c4a0_amd._lib import C4Error

    planes, ops, ref = _tower_on_device(64, 23, n=515)
    for config in (4, 0):
        out = _run_tower(planes, ops, 515, config)
        assert _same(out[:515], ref) and _untouched(out[515:]), config
    _, ops24 = R.tower_case(64, 24, n=2)
    ops24 = {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in ops24.items()}
    with pytest.raises(C4Error, match="23 residual blocks"):
        _run_tower(planes, ops24, 8, 4)


# ------------------------------------------------------------------------------------------------------------------ head out
def _f32_ulp(t: torch.Tensor) -> torch.Tensor:
    """ulp of an f32 of magnitude |t| (float64 in and out; normal range)."""
    _, e = torch.frexp(t.abs().clamp(min=2.0 ** -126))
    return R.pow2(e - 24)


def _check_head(lp, q, pre):
    """log_softmax / tanh of the exact pre-activations in float64.  Bound: the kernel's v - mx is exact or within half an ulp, expf /
    logf / tanhf are within 2 ulps (device libm), the 7-term sum and the two subtractions add an ulp each of the largest magnitude
    involved: 4 f32 ulps of max(|v|, |mx|, |lse|, |logp|) per row for the log-probabilities, 4 ulps of |q| for q."""
    pre = pre.double()
    want = torch.log_softmax(pre[:, :7], dim=1)
    lse = torch.logsumexp(pre[:, :7], dim=1, keepdim=True)
    scale = torch.cat([pre[:, :7].abs(), lse.abs(), want.abs()], dim=1).amax(1, keepdim=True)
    err = (lp.double() - want).abs()
    assert bool((err <= 4 * _f32_ulp(scale)).all()), float((err / _f32_ulp(scale)).max())
    qw = torch.tanh(pre[:, 7:])
    qe = (q.double() - qw).abs()
    assert bool((qe <= 4 * _f32_ulp(qw)).all()), float((qe / _f32_ulp(qw)).max())


def _head_case(features: int, n: int, seed: int):
    """Exact-grid output layers: hidden integers in [-64, 64] (a third zero) as ONE [n, 2F] tensor (the merged layer's two
    halves), sparse 0 / +-1 weights whose columns 0..8 are an identity (policy o <- feature o, value i <- feature 7 + i), biases
    multiples of 64.  Rows 0..5 are edge rows, zero but for features 0..8 chosen so that the pre-activations are: logits
    hundreds apart (expf underflows for all but the max), all equal, a three-way tie for the max, value pre-activations far
    past +-20 (tanhf saturates)."""
    g = torch.Generator().manual_seed(seed)
    both = torch.randint(-64, 65, (n, 2 * features), generator=g).double()
    both[torch.rand(n, 2 * features, generator=g) < 0.33] = 0
    wp = R._sparse_signs(7, features, 16, g, cover=False)
    wv = R._sparse_signs(2, features, 16, g, cover=False)
    wp[:, :9] = 0
    wv[:, :9] = 0
    wp[torch.arange(7), torch.arange(7)] = 1
    wv[torch.arange(2), 7 + torch.arange(2)] = 1
    bp = torch.randint(-2, 3, (7,), generator=g).double() * 64
    bv = torch.randint(-2, 3, (2,), generator=g).double() * 64
    edge = torch.tensor([[896, 0, 192, 320, 448, 576, 768, 1024, -1024],
                         [64, 64, 64, 64, 64, 64, 64, 128, -128],
                         [128, 512, 512, 64, 512, -192, 0, 64, -64],
                         [-896, 0, -128, -256, -512, -768, -1024, 0, 0],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0],
                         [512, -512, 512, -512, 512, -512, 512, 192, -192]], dtype=torch.float64)
    e = min(6, n)
    b9 = torch.cat([bp, bv])
    for half in (0, 1):
        both[:e, half * features:(half + 1) * features] = 0
        both[:e, half * features:half * features + 9] = edge[:e] - b9     # multiples of 64 below 2 048: exact in bf16
    return both.bfloat16(), wp.bfloat16(), wv.bfloat16(), bp.float(), bv.float()


def _run_head(hp, hv, wp, wv, bp, bv, n, features):
    from c4a0_amd._lib import check

    lp = _sentinel_buf(n + 5, 7, torch.float32)
    q = _sentinel_buf(n + 5, 2, torch.float32)
    check(_lib().c4_head_out_bf16(C.c_void_p(hp.data_ptr()), C.c_void_p(hv.data_ptr()), C.c_void_p(wp.data_ptr()), C.c_void_p(wv.data_ptr()),
                                  C.c_void_p(bp.data_ptr()), C.c_void_p(bv.data_ptr()), n, features, hp.stride(0), hv.stride(0),
                                  C.c_void_p(lp.data_ptr()), C.c_void_p(q.data_ptr()), _stream()))
    return lp, q


@pytest.mark.parametrize("features", [1344, 2688, 320, 1352])   # MFMA form (one / two iterations), dot-product form
@pytest.mark.parametrize("n", [1, 6, 13, 1001, 4099])
def test_head_out_exact_preactivations(features, n):
    both, wp, wv, bp, bv = (t.to(DEV).contiguous() for t in _head_case(features, n, seed=features + n))
    hp, hv = both[:, :features], both[:, features:]
    ops = {"pol_out_w": wp, "pol_out_b": bp, "val_out_w": wv, "val_out_b": bv}
    pre = R.head_preact(hp, hv, ops)
    lp, q = _run_head(hp, hv, wp, wv, bp, bv, n, features)
    _check_head(lp[:n], q[:n], pre)
    sentinel = lambda t: bool((t.view(torch.int32) == 0x5A5A5A5A).all())
    assert sentinel(lp[n:]) and sentinel(q[n:]), "wrote past the last board"
    if n >= 6:   # the edge rows are what they were built to be
        assert float(lp[0, 0]) == 0.0 and float(lp[0, 1]) == -896.0      # every expf but the max's underflows: lse == mx
        assert float(lp[2, 1]) == float(lp[2, 2]) == float(lp[2, 4])
        assert q[0].tolist() == [1.0, -1.0]


# ------------------------------------------------------------------------------------------------------------------ evaluator
EVAL_M = [1, 383, 385, 639, 641, 895, 897, 1023, 1025, 1152, 1153, 1280, 1281, 1728, 1729, 2049]


@pytest.mark.parametrize("blocks,channels", R.EVAL_SHAPES)
def test_evaluator_exact_grid(blocks, channels):
    """InferenceNet on grid weights set through the model: its operands equal bf16_ref.operands_from_model's restatement,
    forward_hidden equals the reference bit for bit at batch sizes across every automatic cut, latency_mode off and on, and
    forward is within the output kernel's bound."""
    from c4a0_amd.nn import InferenceNet

    model = R.eval_model(blocks, channels)
    net = InferenceNet(model, DEV, dtype=torch.bfloat16, strict=True)
    assert net.path == "hip" and net.merged_w1 is not None
    mine, theirs = R.operands_from_model(model), R.operands_from_net(net)
    for key in ("tw0", "tw", "tbias", "pol_out_w", "pol_out_b", "val_out_w", "val_out_b"):
        assert torch.equal(theirs[key].cpu(), mine[key]), key
    for key in ("pol_w", "pol_b", "val_w", "val_b"):
        assert len(theirs[key]) == len(mine[key]) and all(torch.equal(a.cpu(), b.to(a.dtype)) for a, b in zip(theirs[key], mine[key])), key
    f = 42 * channels
    assert torch.equal(net.merged_w1[:f].cpu(), mine["pol_w"][0]) and torch.equal(net.merged_w1[f:].cpu(), mine["val_w"][0])
    assert torch.equal(net._bias32[net.merged_b1.data_ptr()].cpu(), torch.cat([mine["pol_b"][0], mine["val_b"][0]]))

    planes = R.grid_planes(EVAL_M[-1], seed=blocks + channels).to(DEV)
    ops = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else (v.to(DEV) if isinstance(v, torch.Tensor) else v)) for k, v in mine.items()}
    p_ref, v_ref = R.hidden(planes, ops)
    pre = R.head_preact(p_ref, v_ref, ops)
    for latency in (False, True):
        for m in EVAL_M:
            p, v = net.forward_hidden(planes[:m].contiguous(), latency)
            assert _same(p, p_ref[:m]) and _same(v, v_ref[:m]), f"{blocks} x {channels}, latency {latency}, batch {m}"
            lp, q = net.forward(planes[:m].contiguous(), latency=latency)
            _check_head(lp, q, pre[:m])


def test_evaluator_64_channels_random_weights_inside_the_interval():
    """8 x 64 with PyTorch's default init: every GEMM layer, fed the GPU's own input activations, inside the interval bound."""
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    torch.manual_seed(64)
    net = InferenceNet(ConnectFourNet(ModelConfig(8, 64, 4, 2)), DEV, dtype=torch.bfloat16, strict=True)
    planes = (torch.rand(1500, 2, 6, 7, device=DEV) < 0.3).to(torch.bfloat16)
    feat = net.tower(planes)
    assert bool(torch.isfinite(feat.float()).all())
    layers = [(feat, net.merged_w1, net.merged_b1)]
    h = net._linear_relu(feat, net.merged_w1, net.merged_b1)
    f = 42 * 64
    outs = [h]
    p, v = h[:, :f], h[:, f:]
    for w, b in zip(net.pol_w[1:-1], net.pol_b[1:-1]):
        layers.append((p, w, b))
        p = net._linear_relu(p, w, b)
        outs.append(p)
    for w, b in zip(net.val_w[1:-1], net.val_b[1:-1]):
        layers.append((v, w, b))
        v = net._linear_relu(v, w, b)
        outs.append(v)
    assert len(layers) == 3     # the merged first layer, the policy head's two further hidden layers
    for i, ((x, w, b), y) in enumerate(zip(layers, outs)):
        lo, hi = R.interval(x, w, net._bias32[b.data_ptr()], relu=True)
        yy = y.double()
        ok = (lo <= yy) & (yy <= hi)
        assert bool(ok.all()), f"layer {i}: {int((~ok).sum())} outputs outside the bound"
        assert float((y > 0).double().mean()) > 0.05    # the layer is not trivially all zero
