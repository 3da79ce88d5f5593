"""The f32 evaluator's kernels through the C ABI (c4_linear_f32, c4_conv_tower_f32, c4_head_out_f32) at their edges, against
tests/f32_net_ref.c bit for bit: both sides of every tile and launch cut, row strides above the width with NaN beside every
input, sentinels round every output (between n and the row stride, past the last row or board), both launch forms of the
GEMM, heads of different widths, edge rows of the log-softmax and tanh, the documented outcomes for Inf and NaN
(include/c4a0_hip.h, "non-finite values": NaN where the reference has NaN, equal bits elsewhere), and what the ABI refuses.
The operands come from tests/f32_ref.py; tests/test_f32_edges_ref.py shows on the CPU that they tell a wrong chain (another
order, a dropped block, a misplaced bias or ReLU, a wrong row, a wrapped tap, a lost residual, swapped planes or weight rows)
from the right one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f32_ref as R  # noqa: E402
from tests.helpers import evidence  # noqa: E402
from tests.test_gpu_bf16_exact import DEV, _lib, _sentinel_buf, _stream, _untouched  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 8                      # extra columns of a strided x (NaN, four on each side of the data) and of a strided y (sentinels)
BAD_ARG = 1                  # C4_ERR_BAD_ARG
NAN = float("nan")


def _ptr(t, offset_bytes=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset_bytes)


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _framed(a: np.ndarray) -> torch.Tensor:
    """a [rows, k] as the middle columns of a NaN-filled device tensor [rows, k + PAD]: a 16-byte aligned row view of stride k + PAD."""
    t = torch.full((a.shape[0], a.shape[1] + PAD), NAN, dtype=torch.float32, device=DEV)
    t[:, PAD // 2:PAD // 2 + a.shape[1]] = _dev(a)
    return t[:, PAD // 2:PAD // 2 + a.shape[1]]


def _ulp_distance(a, b):
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------------------------------ linear
def _linear_on_device(recipe, k, n):
    x, w, b = R.linear_case(recipe, k, n)
    ref = {relu: _bits(_dev(R.linear_ref(recipe, k, n, relu))) for relu in (0, 1)}
    return {"recipe": recipe, "k": k, "n": n, "x": {False: _dev(x), True: _framed(x)}, "w": _dev(w), "b": _dev(b), "ref": ref}


@pytest.fixture(scope="module", params=[(r, k, n) for r in R.RECIPES for k, n in R.LINEAR_SHAPES], ids=lambda p: f"{p[0]}-K{p[1]}-N{p[2]}")
def lin(request):
    """One operand set and its reference on the device, built once for the tests that use it and released after them."""
    return _linear_on_device(*request.param)


def _run_linear(x, w, b, m, relu, strided):
    n, k = w.shape
    y = _sentinel_buf(m + 3, n + (PAD if strided else 0), torch.float32)
    rc = _lib().c4_linear_f32(_ptr(x), _ptr(w), _ptr(b), _ptr(y), m, n, k, x.stride(0), y.stride(0), relu, _stream())
    assert rc == 0, rc
    return y


def _check_linear(ops, ms):
    recipe, k, n = ops["recipe"], ops["k"], ops["n"]
    compared = 0
    for relu in (0, 1):
        for strided in (False, True):
            x = ops["x"][strided]
            assert x.stride(0) == k + (PAD if strided else 0)
            for m in ms:
                y = _run_linear(x, ops["w"], ops["b"], m, relu, strided)
                what = f"{recipe} k {k} n {n} relu {relu} strided {strided} m {m}"
                assert torch.equal(_bits(y[:m, :n]), ops["ref"][relu][:m]), what + ": differs from the reference"
                assert _untouched(y[:m, n:]) and _untouched(y[m:]), what + ": wrote outside its output"
                compared += m * n
    evidence(f"c4_linear_f32 {recipe} k {k} n {n}: {compared} outputs over m = {ms[0]}..{ms[-1]} equal f32ref_linear bit for bit, sentinels untouched")


def test_linear_bit_for_bit_across_the_tile_cuts(lin):
    """Both sides of the 32-row tile (and of 16, 64), 1, 2 and 3 idle wavefronts in the last workgroup, one and several column
    tiles, k = 16 (the prefetch wraps to block 0 in the first iteration) to 2 688; relu off and on; contiguous and strided."""
    _check_linear(lin, R.LINEAR_M)


def test_linear_bit_for_bit_across_the_switch_to_64_row_tiles(lin):
    """m = 2 047, 2 048 (the 32-row form's last) and, on the first four shapes, 2 049, 2 111 and 4 097: the 64-row form
    <kLinear, 2, 4> against the reference itself, with 1, 2 and 3 idle wavefronts."""
    k, n = lin["k"], lin["n"]
    ms = [m for m in R.LINEAR_M_LARGE if m <= R.linear_rows(k, n)]
    assert ms == (R.LINEAR_M_LARGE if (k, n) in R.LINEAR_SHAPES[:4] else R.LINEAR_M_LARGE[:2])
    _check_linear(lin, ms)


def test_linear_rows_permuted_and_repeated():
    k, n = 256, 96
    ops = _linear_on_device("realistic", k, n)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(2111)).to(DEV)
    for strided in (False, True):
        x = ops["x"][strided]
        xp = _framed(x[perm].cpu().numpy()) if strided else x[perm].contiguous()
        y = _run_linear(xp, ops["w"], ops["b"], 2111, 1, strided)
        assert torch.equal(_bits(y[:2111, :n]), ops["ref"][1][perm])
        xr = x[77:78].expand(333, k)
        xr = _framed(xr.cpu().numpy()) if strided else xr.contiguous()
        assert xr.stride(0) == k + (PAD if strided else 0)
        y = _run_linear(xr, ops["w"], ops["b"], 333, 0, strided)
        assert torch.equal(_bits(y[:333, :n]), ops["ref"][0][77:78].expand(333, n))
        assert _untouched(y[:333, n:]) and _untouched(y[333:])


def test_linear_nonfinite_values():
    """NaN and Inf x 0 come through without ReLU and are +0.0 with it; +Inf stays, -Inf becomes +0.0 (relu(s) = s > 0 ? s : 0)."""
    c = R.NONFINITE_LINEAR
    x, w, b = R.linear_nonfinite_case()
    want = {relu: R.linear(x, w, b, relu) for relu in (0, 1)}
    for strided in (False, True):
        xd = _framed(x) if strided else _dev(x)
        for relu in (0, 1):
            y = _run_linear(xd, _dev(w), _dev(b), c["m"], relu, strided)
            got = y[:c["m"], :c["n"]].cpu().numpy()
            assert R.same_bits_or_both_nan(got, want[relu]), (strided, relu)
            assert _untouched(y[:c["m"], c["n"]:]) and _untouched(y[c["m"]:])
            if relu:
                assert not np.isnan(got).any() and not got[c["row_mixed"]].view(np.uint32).any()
                assert got[c["row_inf"], c["col_zero_weight"]].view(np.uint32) == 0
            else:
                assert np.isnan(got[c["row_mixed"]]).all() and np.isnan(got[:, c["col_nan_weight"]]).all()
                assert np.isnan(got[c["row_inf"], c["col_zero_weight"]])


# ------------------------------------------------------------------------------------------------------------------ tower
def _run_tower(planes, w0, w, bias, n, cp, n_blocks, null_work=False):
    """n boards of `planes` (followed by two boards of NaN) through c4_conv_tower_f32 -> (out, work), each with two boards of sentinels."""
    p = torch.full((n + 2, 2, 6, 7), NAN, dtype=torch.float32, device=DEV)
    p[:n] = planes[:n]
    out = _sentinel_buf(n + 2, 42 * cp, torch.float32)
    work = None if null_work else _sentinel_buf(n + 2, 42 * cp, torch.float32)
    rc = _lib().c4_conv_tower_f32(_ptr(p), _ptr(w0), None if null_work else _ptr(w), _ptr(bias), n, cp, n_blocks, _ptr(out), _ptr(work), _stream())
    assert rc == 0, rc
    return out, work


def _check_tower(cp, binary):
    planes, w0, w, bias = (_dev(a) for a in R.tower_case(cp, binary))
    ref = [_bits(_dev(s)) for s in R.tower_ref(cp, binary)]
    compared = 0
    for n_blocks in R.TOWER_BLOCKS:
        for n in [g for g in R.TOWER_BOARDS if g <= R.tower_boards(cp, n_blocks)]:
            out, work = _run_tower(planes, w0, w, bias, n, cp, n_blocks)
            what = f"Cp {cp}, {n_blocks} blocks, {n} boards"
            assert torch.equal(_bits(out[:n]), ref[n_blocks][:n]), what + ": differs from the reference"
            assert _untouched(out[n:]) and _untouched(work[n:] if n_blocks else work), what + ": wrote past the last board"
            compared += n * 42 * cp
    most = ", ".join(f"{b} block(s) up to {R.tower_boards(cp, b)} boards" for b in R.TOWER_BLOCKS)
    evidence(f"c4_conv_tower_f32 Cp {cp} {'0/1' if binary else 'random f32'} planes: {compared} features ({most}) equal "
             "f32ref_conv0 / f32ref_conv bit for bit, sentinels untouched")


@pytest.mark.parametrize("cp", R.TOWER_CP)
def test_tower_bit_for_bit_across_the_tile_cuts(cp):
    """A wavefront's tile is 64 cells, a board 42: 32 boards are exactly 21 tiles (three idle wavefronts in the sixth workgroup),
    31 and 33 sit on each side, 61 / 64 / 65 move the board / tile phase.  Random f32 planes."""
    _check_tower(cp, False)


def test_tower_bit_for_bit_on_positions():
    _check_tower(32, True)


def test_tower_without_blocks_takes_null_work_and_weights():
    planes, w0, w, bias = (_dev(a) for a in R.tower_case(48))
    out, _ = _run_tower(planes, w0, w, bias, 33, 48, 0, null_work=True)
    assert torch.equal(_bits(out[:33]), _bits(_dev(R.tower_ref(48)[0][:33]))) and _untouched(out[33:])


def test_tower_nonfinite_values():
    """One Inf plane value: NaN exactly where the reference has NaN, equal bits everywhere else -- on the reference only cells
    within three rows and columns of the Inf, on its board, are not finite (tests/test_f32_edges_ref.py)."""
    c = R.NONFINITE_TOWER
    planes, w0, w, bias = R.tower_nonfinite_case()
    want = R.tower_stages(planes, w0, w, bias, c["n_blocks"])[-1]
    out, work = _run_tower(_dev(planes), _dev(w0), _dev(w), _dev(bias), c["boards"], c["cp"], c["n_blocks"])
    got = out[:c["boards"]].cpu().numpy()
    assert R.same_bits_or_both_nan(got, want)
    assert _untouched(out[c["boards"]:]) and _untouched(work[c["boards"]:])
    other = [g for g in range(c["boards"]) if g != c["board"]]
    assert np.isfinite(got[other]).all() and not np.isfinite(got[c["board"]]).all()
    assert np.array_equal(got[other].view(np.uint32), R.tower_ref(c["cp"])[c["n_blocks"]][other].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ head out
@pytest.fixture(scope="module", params=R.HEAD_SHAPES, ids=lambda p: f"kp{p[0]}-kv{p[1]}")
def head(request):
    kp, kv = request.param
    hp, hv, wp, wv, bp, bv = R.head_case(kp, kv)
    return {"kp": kp, "kv": kv, "hp": _framed(hp), "hv": _framed(hv), "wp": _dev(wp), "wv": _dev(wv), "bp": bp, "bv": bv}


def _run_head(ops, b9, n, with_preact):
    kp, kv = ops["wp"].shape[1], ops["wv"].shape[1]
    lp, q = _sentinel_buf(n + 5, 7, torch.float32), _sentinel_buf(n + 5, 2, torch.float32)
    pre = _sentinel_buf(n + 5, 9, torch.float32) if with_preact else None
    bp, bv = _dev(b9[:7]), _dev(b9[7:])
    assert ops["hp"].stride(0) == kp + PAD and ops["hv"].stride(0) == kv + PAD
    rc = _lib().c4_head_out_f32(_ptr(ops["hp"]), _ptr(ops["hv"]), _ptr(ops["wp"]), _ptr(ops["wv"]), _ptr(bp), _ptr(bv), n, kp, kv,
                                ops["hp"].stride(0), ops["hv"].stride(0), _ptr(lp), _ptr(q), _ptr(pre), _stream())
    assert rc == 0, rc
    return lp, q, pre


def _check_head(ops, pre_want, b9, n, what):
    """preact bit for bit (NaN for NaN), logprobs = the documented log-softmax of it with the glibc ports bit for bit, q within
    2 ulp of float64 tanh (the device libm's bound; +-Inf give +-1.0 exactly, NaN gives NaN), sentinels untouched, and the same
    bits without the preact output."""
    expf, logf = R.host_libm()
    lp, q, pre = _run_head(ops, b9, n, True)
    lp2, q2, _ = _run_head(ops, b9, n, False)
    for t in (lp, q, pre, lp2, q2):
        assert _untouched(t[n:]), what + ": wrote past the last row"
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(q), _bits(q2)), what + ": preact changes the outputs"
    lp, q, pre = (t[:n].cpu().numpy() for t in (lp, q, pre))
    assert R.same_bits_or_both_nan(pre, pre_want), what + ": pre-activations"
    assert R.same_bits_or_both_nan(lp, R.log_softmax_documented(pre_want[:, :7], expf, logf)), what + ": log-probabilities"
    with np.errstate(invalid="ignore"):
        qw = np.tanh(pre_want[:, 7:].astype(np.float64))
    nan = np.isnan(qw)
    assert np.array_equal(np.isnan(q), nan), what + ": q NaN"
    assert _ulp_distance(q[~nan], qw[~nan]).max(initial=0) <= 2, what + ": q"
    inf = np.isinf(pre_want[:, 7:])
    assert np.array_equal(q[inf], np.sign(pre_want[:, 7:][inf])), what + ": q of an infinite pre-activation"
    return lp, q, pre


def test_head_out_heads_of_different_widths(head):
    """One block, exactly one kDepth group (128), a group and a tail (144), several groups; the narrower head's loads clamp to its
    last block and its MFMAs are gated off while the wider one goes on.  n on both sides of the 16-row workgroup."""
    ops, kp, kv = head, head["kp"], head["kv"]
    b9 = R.head_biases(ops["bp"], ops["bv"])
    nonfinite = 0
    for n in R.HEAD_N:
        nonfinite += int(np.isnan(R.head_ref(kp, kv)[:n]).sum())
        lp, q, pre = _check_head(ops, R.head_ref(kp, kv)[:n], b9, n, f"kp {kp} kv {kv} n {n}")
        assert lp[0, 0] == 0.0 and lp[0, 1] == -896.0                                        # every expf but the maximum's underflows: lse == mx
        if n >= R.HEAD_FIRST_RANDOM:
            assert np.array_equal(pre[:len(R.HEAD_EDGE)], R.HEAD_EDGE)
            assert (lp[1] == lp[1, 0]).all() and lp[1, 0] < -1.9                             # seven equal logits: -log 7
            assert lp[2, 1] == lp[2, 2] == lp[2, 4] and lp[2, 1] > lp[2, 0]                  # the three-way tie for the maximum
            assert q[3, 0] > 0.999999 and q[3, 1] < -0.999999 and not q[4].any()             # tanhf past +-20: +-1 inside the 2 ulp checked above
            assert np.isnan(lp[[R.HEAD_ROW_NAN, R.HEAD_ROW_INF]]).all() and np.isnan(q[R.HEAD_ROW_NAN]).all()
            assert q[R.HEAD_ROW_INF, 0] == 1.0 and np.isnan(q[R.HEAD_ROW_INF, 1])
    evidence(f"c4_head_out_f32 kp {kp} kv {kv}: {sum(R.HEAD_N) * 9} pre-activations and {sum(R.HEAD_N) * 7} log-probabilities over n = "
             f"{R.HEAD_N} compared with the reference: equal bits, but NaN for NaN at {nonfinite} pre-activations (the two non-finite "
             "hidden rows) and their rows' log-probabilities; q within 2 ulp; with and without preact")


def test_head_out_nonfinite_logits_and_values(head):
    """Single non-finite pre-activations (through the biases: a non-finite hidden element reaches every output of its row)."""
    ops, kp, kv, n = head, head["kp"], head["kv"], 33
    rows = slice(R.HEAD_FIRST_RANDOM, n)
    lp, q, _ = _check_head(ops, R.head_ref(kp, kv, "nan_logit")[:n], R.head_biases(ops["bp"], ops["bv"], "nan_logit"), n, "a NaN logit")
    assert np.isnan(lp[rows]).all() and (q[rows] == [1.0, -1.0]).all()
    lp, q, _ = _check_head(ops, R.head_ref(kp, kv, "inf_logit")[:n], R.head_biases(ops["bp"], ops["bv"], "inf_logit"), n, "a +Inf logit")
    assert np.isnan(lp[rows]).all() and np.isnan(q[rows, 0]).all() and np.isfinite(q[rows, 1]).all()
    lp, q, _ = _check_head(ops, R.head_ref(kp, kv, "minus_inf_logits")[:n], R.head_biases(ops["bp"], ops["bv"], "minus_inf_logits"), n, "-Inf logits")
    assert np.isneginf(lp[rows][:, [1, 4]]).all() and np.isfinite(lp[rows][:, [0, 2, 3, 5, 6]]).all() and (q[rows] == [-1.0, 1.0]).all()
    lp, q, _ = _check_head(ops, R.head_ref(kp, kv, "all_minus_inf")[:n], R.head_biases(ops["bp"], ops["bv"], "all_minus_inf"), n, "seven -Inf logits")
    assert np.isnan(lp).all() and np.isfinite(q[rows]).all()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_linear_refusals():
    L = _lib()
    x, w, b = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((40, 64), (64, 64), (64,)))
    y = _sentinel_buf(40, 64, torch.float32)

    def call(xp=None, wp=None, bp=None, yp=None, m=32, n=32, k=32, ldx=64, ldy=64):
        args = [_ptr(x) if xp is None else xp, _ptr(w) if wp is None else wp, _ptr(b) if bp is None else bp, _ptr(y) if yp is None else yp]
        return L.c4_linear_f32(*args, m, n, k, ldx, ldy, 0, _stream())

    null = C.c_void_p(None)
    bad = [call(n=48), call(k=24), call(k=32, ldx=34), call(k=32, ldx=16), call(n=64, ldy=32),
           call(xp=_ptr(x, 4)), call(wp=_ptr(w, 4)), call(bp=_ptr(b, 4)), call(yp=_ptr(y, 4)),
           call(xp=null), call(wp=null), call(bp=null), call(yp=null)]
    assert bad == [BAD_ARG] * len(bad), bad
    assert call(m=0) == 0
    torch.cuda.synchronize()
    assert _untouched(y)


def test_tower_refusals():
    L = _lib()
    planes, w0, w, bias = (_dev(a) for a in R.tower_case(16))
    out, work = _sentinel_buf(4, 42 * 80, torch.float32), _sentinel_buf(4, 42 * 80, torch.float32)

    def call(channels=16, n_blocks=1, n=2, work_p=_ptr(work)):
        return L.c4_conv_tower_f32(_ptr(planes), _ptr(w0), _ptr(w), _ptr(bias), n, channels, n_blocks, _ptr(out), work_p, _stream())

    bad = [call(channels=0), call(channels=24), call(channels=80), call(work_p=None)]
    assert bad == [BAD_ARG] * len(bad), bad
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(work)


def test_head_out_refusals():
    L = _lib()
    h = torch.zeros((20, 64), dtype=torch.float32, device=DEV)
    wp, wv, bp, bv = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((7, 64), (2, 64), (7,), (2,)))
    lp, q, pre = (_sentinel_buf(20, c, torch.float32) for c in (7, 2, 9))

    def call(n=16, kp=32, kv=32, ldp=64, ldv=64):
        return L.c4_head_out_f32(_ptr(h), _ptr(h), _ptr(wp), _ptr(wv), _ptr(bp), _ptr(bv), n, kp, kv, ldp, ldv, _ptr(lp), _ptr(q), _ptr(pre), _stream())

    bad = [call(kp=24), call(kv=24), call(kp=32, ldp=16), call(kv=32, ldv=16), call(kp=32, ldp=34), call(kv=32, ldv=34)]
    assert bad == [BAD_ARG] * len(bad), bad
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert _untouched(lp) and _untouched(q) and _untouched(pre)
