"""The fp8 hidden layers' kernels (c4_quantize_bf16_fp8, c4_linear_fp8) against tests/fp8_ref.py, the float64 restatement of the
numerics contract in include/c4a0_hip.h ("fp8 hidden layers").

On exact-grid data (every partial sum an exact f32 in any order; tests/test_fp8_ref.py shows the data holds its shares of ties,
saturated values and subnormals and tells every fp8_ref.MUTATIONS entry from the true layer) the kernels must equal the reference
BIT FOR BIT, for every m, output mode and `config`.  x8 is a column view whose next 64 columns hold NaN and 448 codes: nothing
behind column k may matter, also where the last k-step is half a step (k = 64, 192, 1344).  Outputs carry sentinels past their last
row and between n and the row stride.  On realistic data every output must lie inside the interval any f32 summation order
satisfies, pushed through the monotone output rounding: no tolerance is chosen by hand."""
import ctypes as C
import functools

import pytest
import torch

from tests import fp8_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIGS = [0, 1, 2, 3, 4]    # every config c4_linear_fp8 accepts
YPAD = 16                    # ldy = n + 16, sentinels behind n
S8, S16 = 0x5A, 0x5A5A       # sentinel byte / bf16 pattern


def _lib():
    from c4a0_amd import _lib as L

    return L.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sentinel_buf(rows: int, cols: int, fp8: bool) -> torch.Tensor:
    if fp8:
        return torch.full((rows, cols), S8, dtype=torch.uint8, device=DEV)
    t = torch.empty((rows, cols), dtype=torch.bfloat16, device=DEV)
    t.view(torch.int16).fill_(S16)
    return t


def _untouched(t: torch.Tensor) -> bool:
    return bool((t == S8).all()) if t.dtype == torch.uint8 else bool((t.view(torch.int16) == S16).all())


def _run_linear(x8, wq, dq, bias, m, k, relu, out_fp8, out_scale, config):
    """x8: a device tensor [>= m, ldx] read as a column view of k columns."""
    from c4a0_amd._lib import check

    n = wq.shape[0]
    y = _sentinel_buf(m + 3, n + YPAD, out_fp8)
    check(_lib().c4_linear_fp8(C.c_void_p(x8.data_ptr()), C.c_void_p(wq.data_ptr()), C.c_void_p(dq.data_ptr()), C.c_void_p(bias.data_ptr()),
                               C.c_void_p(y.data_ptr()), m, n, k, x8.stride(0), y.stride(0), relu, 1 if out_fp8 else 0, float(out_scale), config, _stream()))
    return y


def _same(y, ref, out_fp8) -> bool:
    """fp8: the same codes.  bf16: the same values (+0 == -0), NaN where the reference has NaN."""
    if out_fp8:
        return torch.equal(y.cpu(), ref)
    y = y.cpu().double()
    return bool(((y == ref) | (y.isnan() & ref.isnan())).all())


# ------------------------------------------------------------------------------------------------------------------ quantise
def _all_bf16_patterns(m, k, ldx):
    """bf16 [m][ldx]: the bit patterns 0, 1, 2, ... (every one of the 65 536 where m k reaches that many), +-inf and NaNs included;
    the columns behind k hold other patterns, which must not show."""
    x = ((torch.arange(m * ldx, dtype=torch.int64) * 7 + 0x1234) & 0xFFFF).reshape(m, ldx)
    # (fewer than 65 536 elements: a window around 2^-3 .. 2^9 and its neighbours, where the e4m3 steps lie)
    x[:, :k] = ((torch.arange(m * k, dtype=torch.int64) * (1 if m * k >= 65536 else 37) + (0 if m * k >= 65536 else 0x3B00)) & 0xFFFF).reshape(m, k)
    return torch.where(x >= 0x8000, x - 0x10000, x).to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("m", [1, 3, 130])
@pytest.mark.parametrize("k", [64, 1344])
def test_quantize_bit_for_bit(m, k):
    from c4a0_amd._lib import check

    ldx, ldy = k + 8, k + 16
    x = _all_bf16_patterns(m, k, ldx)
    if m * k >= 65536:
        assert len(torch.unique(x[:, :k].contiguous().view(torch.int16))) == 65536      # every bf16 bit pattern, NaN and +-inf included
    xd = x.to(DEV)
    for scale in (2.0 ** -3, 1.0, 2.0 ** 5):
        y = _sentinel_buf(m + 2, ldy, True)
        check(_lib().c4_quantize_bf16_fp8(C.c_void_p(xd.data_ptr()), C.c_void_p(y.data_ptr()), m, k, ldx, ldy, scale, _stream()))
        ref = R.quantize(x[:, :k], scale)
        got = y[:m, :k].cpu()
        bad = (got != ref).nonzero()
        assert len(bad) == 0, f"m {m} k {k} scale {scale}: {len(bad)} differ, first x bits {int(x[:, :k].contiguous().view(torch.int16)[tuple(bad[0])]) & 0xFFFF:#06x} " \
                              f"got {int(got[tuple(bad[0])]):#04x} want {int(ref[tuple(bad[0])]):#04x}"
        assert _untouched(y[:m, k:]) and _untouched(y[m:]), f"m {m} k {k}: wrote past its output"


def test_quantize_refuses_bad_arguments():
    from c4a0_amd import _lib as L

    x = torch.zeros(4, 72, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(4, 80, dtype=torch.uint8, device=DEV)
    for args in ((4, 60, 72, 80, 1.0), (4, 64, 60, 80, 1.0), (4, 64, 72, 60, 1.0), (4, 64, 72, 80, 0.0), (4, 64, 72, 80, float("nan"))):
        assert _lib().c4_quantize_bf16_fp8(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), *args, _stream()) == L.ERR_BAD_ARG
        assert b"c4_quantize_bf16_fp8" in _lib().c4_last_error_string()


# ------------------------------------------------------------------------------------------------------------------ GEMM, exact grid
@functools.lru_cache(maxsize=None)
def _case(k, n):
    x8, wq, dq, bias, s = R.gemm_case(k, n)
    ref = {(relu, fp8): R.linear(x8, wq, dq, bias, k, bool(relu), bool(fp8), s) for relu in (0, 1) for fp8 in (0, 1)}
    return {"k": k, "n": n, "x8": x8.to(DEV), "wq": wq.to(DEV), "dq": dq.to(DEV), "bias": bias.to(DEV), "s": s, "ref": ref, "cpu": (x8, wq, dq, bias)}


def _check_grid(k, n, ms, config):
    c = _case(k, n)
    assert c["x8"].stride(0) == k + R.PAD and bool((c["x8"][:, k:] >= 0x7E).all())      # NaN and 448 right behind column k
    for relu in (0, 1):
        for fp8 in (0, 1):
            for m in ms:
                y = _run_linear(c["x8"], c["wq"], c["dq"], c["bias"], m, k, relu, fp8, c["s"], config)
                what = f"K {k} N {n} config {config} relu {relu} out {'fp8' if fp8 else 'bf16'} m {m}"
                assert _same(y[:m, :n], c["ref"][(relu, fp8)][:m], fp8), what + ": differs from the reference"
                assert _untouched(y[:m, n:]) and _untouched(y[m:]), what + ": wrote past its output"


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("k,n", R.SMALL_SHAPES)
def test_linear_exact_grid_small_shapes(k, n, config):
    _check_grid(k, n, R.SMALL_M, config)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("k,n", R.LARGE_SHAPES)
def test_linear_exact_grid_net_shapes(k, n, config):
    _check_grid(k, n, [R.GEMM_M], config)


def test_linear_refuses_bad_arguments():
    from c4a0_amd import _lib as L

    c = _case(64, 192)
    y = _sentinel_buf(8, 192 + YPAD, True)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(m=4, n=192, k=64, ldx=128, ldy=208, relu=1, out_fp8=1, out_scale=1.0, config=0)
    for bad in (dict(n=100), dict(k=32), dict(ldx=48), dict(ldx=72), dict(ldy=100), dict(ldy=206), dict(out_scale=0.0), dict(config=5)):
        a = {**good, **bad}
        st = _lib().c4_linear_fp8(p(c["x8"]), p(c["wq"]), p(c["dq"]), p(c["bias"]), p(y), a["m"], a["n"], a["k"], a["ldx"], a["ldy"], a["relu"], a["out_fp8"],
                                  a["out_scale"], a["config"], _stream())
        assert st == L.ERR_BAD_ARG and b"c4_linear_fp8" in _lib().c4_last_error_string(), bad
    assert _lib().c4_linear_fp8(None, p(c["wq"]), p(c["dq"]), p(c["bias"]), p(y), 4, 192, 64, 128, 208, 1, 1, 1.0, 0, _stream()) == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert _untouched(y)


# ------------------------------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("k,n", [(192, 384), (1344, 1344)])
def test_one_nan_code_makes_its_row_nan_and_no_other(k, n):
    c = _case(k, n)
    m, row = 130, 77
    x8 = c["x8"][:m].clone()
    x8[row, k - 3] = 0xFF                                        # the other NaN code, in the half k-step
    for relu in (0, 1):
        for fp8 in (0, 1):
            y = _run_linear(x8, c["wq"], c["dq"], c["bias"], m, k, relu, fp8, c["s"], 0)[:m, :n].cpu()
            ref = c["ref"][(relu, fp8)][:m]
            others = torch.arange(m) != row
            assert _same(y[others], ref[others], fp8), f"K {k} relu {relu} fp8 {fp8}: a NaN leaked into another row"
            if fp8:
                assert bool((y[row] == 0x7F).all()), f"K {k} relu {relu}: the NaN row is not all 0x7F (a NaN was laundered)"
            else:
                assert bool(y[row].isnan().all()), f"K {k} relu {relu}: the NaN row is not all NaN (a NaN was laundered)"


# ------------------------------------------------------------------------------------------------------------------ batch invariance
def test_rows_do_not_depend_on_the_batch():
    """Realistic (inexact) data, so that a different summation order WOULD show: the rows of an m = 300 call equal the same rows
    computed alone, in a call of 129 rows and in a call of all 300 in another order, bit for bit, in both output modes."""
    k, n, m = 1344, 1344, 300
    x8, wq, dq, bias, s = R.realistic_case(m, k, n, seed=9)
    x8, wq, dq, bias = x8.to(DEV), wq.to(DEV), dq.to(DEV), bias.to(DEV)
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(3)).to(DEV)
    for fp8 in (0, 1):
        full = _run_linear(x8, wq, dq, bias, m, k, 1, fp8, s, 0)[:m, :n]
        for config in CONFIGS:
            for row in (0, 77, 299):
                one = _run_linear(x8[row:row + 1].contiguous(), wq, dq, bias, 1, k, 1, fp8, s, config)[:1, :n]
                assert torch.equal(one.view(torch.uint8), full[row:row + 1].contiguous().view(torch.uint8)), (fp8, config, row)
            part = _run_linear(x8[171:].contiguous(), wq, dq, bias, 129, k, 1, fp8, s, config)[:129, :n]
            assert torch.equal(part.contiguous().view(torch.uint8), full[171:].contiguous().view(torch.uint8)), (fp8, config)
            shuffled = _run_linear(x8[perm].contiguous(), wq, dq, bias, m, k, 1, fp8, s, config)[:m, :n]
            assert torch.equal(shuffled.contiguous().view(torch.uint8), full[perm].contiguous().view(torch.uint8)), (fp8, config)


# ------------------------------------------------------------------------------------------------------------------ realistic data
@pytest.mark.parametrize("blocks,channels", [(4, 32), (8, 64)])
def test_net_layers_inside_the_interval(blocks, channels):
    """Weights of a default-initialised ConnectFourNet, activations from the tower on random positions: every layer's GPU result
    lies inside the reference's interval computed on the exactly known quantised operands (the GPU's own output feeds the next
    layer), through both output modes."""
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig, activation_exponent, fold_network, quantize_head_weights
    from tests.helpers import pos_to_planes_np, random_positions
    import numpy as np

    torch.manual_seed(blocks * channels)
    model = ConnectFourNet(ModelConfig(blocks, channels, 4, 2)).eval()
    net = InferenceNet(model, DEV)
    pos = np.array(random_positions(300), dtype=np.uint64)
    feat = net.tower(torch.from_numpy(pos_to_planes_np(pos[:, 0], pos[:, 1])).to(DEV, torch.bfloat16)).cpu()
    _, _, pol_w, pol_b, _, _ = fold_network(model)
    f = 42 * channels
    perm = lambda wt: wt.reshape(wt.shape[0], channels, 42).permute(0, 2, 1).reshape(wt.shape[0], f)
    e_x = activation_exponent(float(feat.float().abs().max()))
    x8 = R.quantize(feat, 2.0 ** e_x)
    checked = 0
    for i, (w, b) in enumerate(zip([perm(pol_w[0])] + pol_w[1:-1], pol_b[:-1])):
        wq, e_w = quantize_head_weights(w)
        dq = R.pow2(-e_x - e_w.to(torch.int64)).float()
        args = (x8.to(DEV), wq.to(DEV), dq.to(DEV), b.float().to(DEV).contiguous())
        yb = _run_linear(*args, 300, f, 1, 0, 1.0, 0)[:300, :f].cpu().double()
        bounds = R.bounds(x8, wq, dq, b.float(), f, True)
        lo, hi = R.interval_bf16(x8, wq, dq, b.float(), f, True, bounds)
        ok = (lo <= yb) & (yb <= hi)
        assert bool(ok.all()), f"layer {i} bf16: {int((~ok).sum())} outputs outside the bound"
        e_next = activation_exponent(float(yb.abs().max()))
        y8 = _run_linear(*args, 300, f, 1, 1, 2.0 ** e_next, 0)[:300, :f].cpu()
        lo, hi = R.interval_codes(x8, wq, dq, b.float(), f, True, 2.0 ** e_next, bounds)
        yv = R.decode(y8)
        ok = (lo <= yv) & (yv <= hi)
        assert bool(ok.all()), f"layer {i} fp8: {int((~ok).sum())} outputs outside the bound"
        checked += 2 * ok.numel()
        x8, e_x = y8, e_next
    assert checked == 3 * 2 * 300 * f
