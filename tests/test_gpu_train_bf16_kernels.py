"""The kernels of bf16 mixed-precision training through the C ABI (c4a0_amd/csrc/c4_train_bf16.hip): c4_train_cast_bf16,
c4_train_bn_relu_fwd_bf16, c4_train_bn_relu_bwd_bf16, and the three products of a step on c4_linear_bf16, against the float64
restatement of the contract in tests/train_bf16_ref.py.

* The cast and its transpose are held bit for bit to bf16_round, pads and guard frames included.
* The three products run on small-integer data whose every partial sum is exact in f32 and whose result is exact in bf16: z, dx and
  dw equal the reference bit for bit, which pins the transposed-operand wiring and the zero padding of the batch dimension.
  c4_linear_bf16 needs an output width that is a multiple of 192, so at (n, k) = (192, 64) only the forward product exists: dgrad
  and wgrad would be 64 wide and are refused by the GEMM with C4_ERR_BAD_ARG, which the test asserts; (192, 192) stands beside it so
  that all three products are pinned at a small size too.
* The batch-norm kernels are held to the 4 x rule of tests/test_gpu_train_kernels.py: the f32 outputs against PyTorch's own f32
  F.batch_norm + ReLU and autograd on the widened inputs, floor 4 * 2^-24 * max |ref|; the bf16 outputs elementwise,
  |out - ref| <= 2^-8 |ref| + max(4 e_torch, 4 * 2^-24 max |ref|), the first term one bf16 rounding.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_bf16_ref as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG = 1
SENT = {torch.bfloat16: 0x5A5A, torch.float32: 0x5A5A5A5A}     # bit patterns no kernel computes here
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
U = 2.0 ** -24
EPS = 1e-5


def _lib():
    from c4a0_amd import _lib as L

    return L.lib()


def _err():
    return (_lib().c4_last_error_string() or b"").decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _dev(a, dtype=None):
    t = torch.tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)       # f32 values that are bf16 values convert exactly


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _padded(m: int) -> int:
    return 64 * ((m + 63) // 64)


class Framed:
    """An output [rows, cols] (row stride cols + pad) inside a buffer of sentinels: one row above and below, pad / 2 columns left and
    right (pad = 0: a dense matrix or a vector with sentinel rows only)."""

    def __init__(self, rows: int, cols: int, pad: int = 0, dtype=torch.bfloat16):
        self.buf = torch.empty((rows + 2, cols + pad), dtype=dtype, device=DEV)
        self.buf.view(INT[dtype]).fill_(SENT[dtype])
        self.view = self.buf[1:1 + rows, pad // 2:pad // 2 + cols]
        self.ld, self.dtype = cols + pad, dtype
        assert self.view.data_ptr() % 16 == 0

    def intact(self) -> bool:
        b = self.buf.view(INT[self.dtype]).clone()
        r, c = self.view.shape
        off = (self.ld - c) // 2
        b[1:1 + r, off:off + c] = SENT[self.dtype]
        return bool((b == SENT[self.dtype]).all())

    def written(self) -> bool:
        return bool((self.view.contiguous().view(INT[self.dtype]) != SENT[self.dtype]).any())

    def np(self):
        return self.view.float().cpu().numpy()


def _same_bytes(a: Framed, b: Framed) -> bool:
    return torch.equal(a.buf.view(INT[a.dtype]), b.buf.view(INT[b.dtype]))


# ------------------------------------------------------------------------------------------------------------------ cast and transpose
def _cast(src, m, c, dst: bool, dst_t: bool, ldt=None, pad=0):
    out = Framed(m, c, pad) if dst else None
    ldt = _padded(m) if ldt is None else ldt
    out_t = Framed(c, ldt) if dst_t else None
    rc = _lib().c4_train_cast_bf16(_p(src), int(src.dtype == torch.bfloat16), m, c, src.stride(0), _p(out.view) if dst else None, out.ld if dst else 0,
                                   _p(out_t.view) if dst_t else None, ldt, _stream())
    assert rc == 0, _err()
    return out, out_t


def _cast_source(m: int, c: int, as_bf16: bool, seed: int) -> np.ndarray:
    """f32 values over the whole exponent range with ties, values beside ties, zeros of both signs, infinities and subnormals among
    them; as_bf16: rounded, so that they are a bf16 tensor's values"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, (m, c), dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7FFFFFFF) > 0x7F800000] &= 0x807FFFFF                        # no NaN: its payload is nobody's contract
    flat = bits.reshape(-1)
    special = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00008000, 0x80018000, 1],
                       dtype=np.uint32)
    n = min(special.size, flat.size)
    flat[rng.choice(flat.size, n, replace=False)] = special[:n]
    a = bits.view(np.float32)
    return R.bf16_round(a) if as_bf16 else a


@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [64, 1344])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_cast_and_transpose_are_bf16_round_bit_for_bit(m, c, as_bf16):
    a = _cast_source(m, c, as_bf16, 1000 * m + c + as_bf16)
    want = R.bf16_bits(a)
    dtype = torch.bfloat16 if as_bf16 else None
    dense = _dev(a, dtype)
    # the same source as a 16-byte aligned row view of stride c + 8 in a NaN-filled tensor: a read outside the data would show
    wide = torch.full((m + 2, c + 8), float("nan"), dtype=dense.dtype, device=DEV)
    strided = wide[1:1 + m, 8:8 + c]
    strided.copy_(dense)
    mp = _padded(m)
    for what, src, dst, dst_t, ldt, pad in (("dst", dense, True, False, None, 16), ("dst_t", dense, False, True, mp, 0),
                                            ("both, strided, wide ldt", strided, True, True, mp + 264, 0)):
        out, out_t = _cast(src, m, c, dst, dst_t, ldt, pad)
        if dst:
            assert out.intact() and np.array_equal(_bits(out.view), want), what
        if dst_t:
            got = _bits(out_t.view)
            assert out_t.intact() and got.shape == (c, ldt), what               # nothing past ldt, nothing past row c
            assert np.array_equal(got[:, :m], want.T), what
            assert not got[:, m:].any(), what                                    # columns m .. ldt - 1: zeros, bit for bit


# ------------------------------------------------------------------------------------------------------------------ the three products
def _linear(x, w, bias, m, n, k):
    y = Framed(m, n)
    rc = _lib().c4_linear_bf16(_p(x), _p(w), _p(bias), _p(y.view), m, n, k, x.stride(0), y.ld, 0, 0, _stream())
    return rc, y


def _exact(got: Framed, want: np.ndarray, what: str):
    assert np.array_equal(R.r64(want), want), what + ": the reference is not exact in bf16 (the test's precondition)"
    assert got.intact(), what
    # + 0.0 leaves every value but the sign of a zero as it is
    assert np.array_equal(R.bf16_bits(got.np() + np.float32(0)), R.bf16_bits(want.astype(np.float32) + np.float32(0))), what


def _sparse_rows(rng, rows: int, cols: int, per_row: int = 8) -> np.ndarray:
    """integers in {-4 .. 4}, at most per_row of a row nonzero: a product with a dense {-4 .. 4} matrix stays within +-128"""
    a = np.zeros((rows, cols), dtype=np.float32)
    for r in range(rows):
        a[r, rng.choice(cols, per_row, replace=False)] = rng.integers(-4, 5, per_row)
    return a


@pytest.mark.parametrize("n, k", [(192, 64), (192, 192), (1344, 1344)], ids=lambda v: str(v))
@pytest.mark.parametrize("m", [2, 65, 130])
def test_the_three_products_are_exact_on_small_integers(m, n, k):
    """forward x W^T + b, dgrad dz W and wgrad dz^T x through c4_train_cast_bf16 (which makes W^T, x^T and dz^T, the batch padded to
    mp = 64 ceil(m / 64) with zeros) and c4_linear_bf16: integers whose sums stay below 2^8 in magnitude, so every partial sum is exact
    in f32, the result exact in bf16, and any correct wiring gives the reference's bits.  The pad columns of the transposes are
    poisoned first: a stale NaN there, or a pad not written, would show in dw."""
    rng = np.random.default_rng(100 * m + n + k)
    w = rng.integers(-4, 5, (n, k)).astype(np.float32)
    b = rng.integers(-64, 65, n).astype(np.float32)
    x_fwd, dz_dgrad = _sparse_rows(rng, m, k), _sparse_rows(rng, m, n)
    x_wgrad, dz_wgrad = (rng.integers(-1, 2, s).astype(np.float32) for s in ((m, k), (m, n)))      # |dw| <= m <= 130
    mp = _padded(m)
    wb, wb_t = _cast(_dev(w), n, k, True, True)
    zeros = torch.zeros(max(n, k), device=DEV)
    # forward
    xb, _ = _cast(_dev(x_fwd), m, k, True, False)
    rc, z = _linear(xb.view, wb.view, _dev(b), m, n, k)
    assert rc == 0, _err()
    _exact(z, x_fwd.astype(np.float64) @ w.astype(np.float64).T + b, "z")
    if k % 192:
        # dx [m][k] and dw [n][k] would be k = 64 wide: c4_linear_bf16 takes output widths that are multiples of 192 only
        dzb, _ = _cast(_dev(dz_dgrad), m, n, True, False)
        rc, dx = _linear(dzb.view, wb_t.view, zeros, m, k, n)
        torch.cuda.synchronize()
        assert rc == BAD_ARG and "multiple of 192" in _err() and not dx.written()
        return
    # dgrad: x = dz [m][n], w = W^T [k][n]
    dzb, _ = _cast(_dev(dz_dgrad), m, n, True, False)
    rc, dx = _linear(dzb.view, wb_t.view, zeros, m, k, n)
    assert rc == 0, _err()
    _exact(dx, dz_dgrad.astype(np.float64) @ w.astype(np.float64), "dx")
    # wgrad: x = dz^T [n][mp], w = x^T [k][mp], the batch as k
    _, dz_t = _cast(_dev(dz_wgrad), m, n, False, True)
    _, x_t = _cast(_dev(x_wgrad), m, k, False, True)
    assert dz_t.view.shape == (n, mp) and x_t.view.shape == (k, mp)
    rc, dw = _linear(dz_t.view, x_t.view, zeros, n, k, mp)
    assert rc == 0, _err()
    _exact(dw, dz_wgrad.astype(np.float64).T @ x_wgrad.astype(np.float64), "dw")


# ------------------------------------------------------------------------------------------------------------------ batch norm
def _bn_case(m: int, n: int, seed: int):
    """bf16-valued z and dy, f32 gamma and beta, with the edge columns: 0 a constant column (1.25: var = 0, the mean exact),
    1 gamma = 0 and beta = 0 (every pre-activation +0 or -0), 2 every pre-activation <= 0 (beta = -100), 3 gamma = 1e-30, beta = 0
    (tiny pre-activations of either sign).  dy is 0 where the float64 pre-activation lies within 1e-4 of 0 (columns 1 and 3 apart):
    there the sign of a rounding error would decide ReLU' for the kernel, for PyTorch and for nobody in float64."""
    rng = np.random.default_rng(seed)
    z = R.bf16_round((rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-1, 1, n) + rng.standard_normal(n) * 3).astype(np.float32))
    gamma = rng.uniform(0.5, 1.5, n).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    beta = (rng.standard_normal(n) * 0.5).astype(np.float32)
    z[:, 0] = 1.25
    gamma[1] = beta[1] = 0.0
    beta[2] = -100.0
    gamma[3], beta[3] = 1e-30, 0.0
    dy = R.bf16_round(rng.standard_normal((m, n)).astype(np.float32))
    near = np.abs(R.bn_forward(z, gamma, beta, EPS)["pre"]) < 1e-4
    near[:, [1, 3]] = False
    dy[near] = 0.0
    return z, gamma, beta, dy


def _bn_fwd(z, gamma, beta, m, n, with_t=True, pad=0):
    y, mean, var = Framed(m, n, pad), Framed(1, n, 0, torch.float32), Framed(1, n, 0, torch.float32)
    ldt = _padded(m) + 8
    y_t = Framed(n, ldt) if with_t else None
    rc = _lib().c4_train_bn_relu_fwd_bf16(_p(z), _p(gamma), _p(beta), C.c_float(EPS), m, n, z.stride(0), y.ld, _p(y.view), _p(mean.view), _p(var.view),
                                          _p(y_t.view) if with_t else None, ldt, _stream())
    assert rc == 0, _err()
    return y, mean, var, y_t


def _bn_bwd(dy, z, mean, var, gamma, beta, m, n, pad=0):
    dz, ldt = Framed(m, n, pad), _padded(m) + 8
    dz_t = Framed(n, ldt)
    dgamma, dbeta, db = (Framed(1, n, 0, torch.float32) for _ in range(3))
    rc = _lib().c4_train_bn_relu_bwd_bf16(_p(dy), _p(z), _p(mean), _p(var), _p(gamma), _p(beta), C.c_float(EPS), m, n, dy.stride(0), z.stride(0), dz.ld,
                                          _p(dz.view), _p(dz_t.view), ldt, _p(dgamma.view), _p(dbeta.view), _p(db.view), _stream())
    assert rc == 0, _err()
    return dz, dz_t, dgamma, dbeta, db


def _judge(what, got, torch_got, ref):
    """the 4 x rule for an f32 output: max |got - ref| <= max(4 max |torch - ref|, 4 * 2^-24 * max |ref|)"""
    e_k = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    e_t = float(np.abs(np.asarray(torch_got, dtype=np.float64) - ref).max())
    floor = 4 * U * float(np.abs(ref).max())
    evidence(f"{what}: kernel err {e_k:.3e}, PyTorch f32 err {e_t:.3e}, ratio {e_k / e_t if e_t else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


def _judge_bf16(what, got, torch_got, ref):
    """a bf16 output, elementwise: |got - ref| <= 2^-8 |ref| + max(4 e_torch, 4 * 2^-24 max |ref|), ref before the rounding"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    e_t = float(np.abs(np.asarray(torch_got, dtype=np.float64) - ref).max())
    slack = max(4 * e_t, 4 * U * float(np.abs(ref).max()))
    bound = 2.0 ** -8 * np.abs(ref) + slack
    worst = float((err / np.maximum(bound, 1e-300)).max())
    evidence(f"{what}: max err / bound {worst:.3f} (PyTorch f32 err {e_t:.3e}, slack {slack:.3e})")
    assert (err <= bound).all(), (what, worst)


def _transposed_ok(t: Framed, of: Framed, m: int) -> bool:
    got = _bits(t.view)
    return t.intact() and np.array_equal(got[:, :m], _bits(of.view).T) and not got[:, m:].any()


@pytest.mark.parametrize("n", [192, 1344])
@pytest.mark.parametrize("m", [2, 17, 64, 65, 257])
def test_bn_relu_forward_and_backward_against_the_reference(m, n):
    z, gamma, beta, dy = _bn_case(m, n, 7 * m + n)
    ref = R.bn_backward(dy, z, gamma, beta, EPS)
    zd, gd, bd, dyd = _dev(z, torch.bfloat16), _dev(gamma), _dev(beta), _dev(dy, torch.bfloat16)
    # PyTorch's f32 on the same device and the widened inputs
    zt, gt, bt = zd.float().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    rm, rv = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    yt = torch.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 1.0, EPS))     # momentum 1: the running statistics are the batch's
    yt.backward(dyd.float())
    y, mean, var, y_t = _bn_fwd(zd, gd, bd, m, n)
    y2, mean2, var2, y_t2 = _bn_fwd(zd, gd, bd, m, n)
    assert y.intact() and mean.intact() and var.intact()
    assert _same_bytes(y, y2) and _same_bytes(mean, mean2) and _same_bytes(var, var2) and _same_bytes(y_t, y_t2)
    assert _transposed_ok(y_t, y, m)
    y_alone = _bn_fwd(zd, gd, bd, m, n, with_t=False)[0]
    assert _same_bytes(y, y_alone)
    tag = f"train bn bf16 m={m} n={n}"
    _judge_bf16(tag + " y", y.np(), yt.detach().cpu().numpy(), ref["y32"])
    _judge(tag + " mean", mean.np()[0], rm.cpu().numpy(), ref["mean"])
    _judge(tag + " var", var.np()[0], (rv * ((m - 1) / m)).cpu().numpy(), ref["var"])
    assert np.array_equal(var.np()[0, :1], [0.0]) and np.array_equal(mean.np()[0, :1], [1.25])       # the constant column
    dz, dz_t, dgamma, dbeta, db = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    again = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    for a, b in zip((dz, dz_t, dgamma, dbeta, db), again):
        assert a.intact() and _same_bytes(a, b)
    assert _transposed_ok(dz_t, dz, m)
    _judge_bf16(tag + " dz", dz.np(), zt.grad.cpu().numpy(), ref["dz32"])
    _judge(tag + " dgamma", dgamma.np()[0], gt.grad.cpu().numpy(), ref["dgamma"])
    _judge(tag + " dbeta", dbeta.np()[0], bt.grad.cpu().numpy(), ref["dbeta"])
    _judge(tag + " db", db.np()[0], zt.grad.sum(0).cpu().numpy(), ref["db"])
    got, yk = dz.np(), y.np()
    # column 1, pre-activations +0 and -0: y = 0 and ReLU'(0) = 0, nothing of dy arrives anywhere
    assert (yk[:, 1] == 0).all() and (got[:, 1] == 0).all() and dbeta.np()[0, 1] == 0 and dgamma.np()[0, 1] == 0
    assert (got[:, 2] == 0).all() and dgamma.np()[0, 2] == 0 and dbeta.np()[0, 2] == 0   # no pre-activation above 0: exactly 0
    # column 3, tiny pre-activations of either sign: the backward's mask is the forward's -- dbeta sums dy exactly where y > 0
    live = yk[:, 3] > 0
    assert live.any() and not live.all() if m > 2 else True
    want = dy[live, 3].astype(np.float64).sum()
    assert abs(float(dbeta.np()[0, 3]) - want) <= (m + 2) * U * np.abs(dy[:, 3]).astype(np.float64).sum(), (dbeta.np()[0, 3], want)


def test_bn_relu_reads_and_writes_strided_rows_in_place():
    m, n = 17, 192
    z, gamma, beta, dy = _bn_case(m, n, 99)
    zd, gd, bd, dyd = _dev(z, torch.bfloat16), _dev(gamma), _dev(beta), _dev(dy, torch.bfloat16)

    def strided(t):
        wide = torch.full((m + 2, n + 16), float("nan"), dtype=torch.bfloat16, device=DEV)
        v = wide[1:1 + m, 8:8 + n]
        v.copy_(t)
        return v

    y, mean, var, y_t = _bn_fwd(zd, gd, bd, m, n)
    ys, means, vars_, y_ts = _bn_fwd(strided(zd), gd, bd, m, n, pad=16)
    assert ys.intact() and torch.equal(ys.view.contiguous(), y.view.contiguous()) and _same_bytes(mean, means) and _same_bytes(var, vars_)
    assert _same_bytes(y_t, y_ts)
    dense = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    views = _bn_bwd(strided(dyd), strided(zd), mean.view[0], var.view[0], gd, bd, m, n, pad=16)
    assert views[0].intact() and torch.equal(views[0].view.contiguous().view(torch.int16), dense[0].view.contiguous().view(torch.int16))
    for a, b in zip(dense[1:], views[1:]):
        assert _same_bytes(a, b)


# ------------------------------------------------------------------------------------------------------------------ non-finite input
def test_a_non_finite_column_is_poisoned_and_no_other_column_changes():
    """column 5 of z holds one NaN, column 7 one +inf, column 9 values whose f32 sum overflows: y, dz, dgamma and db of exactly these
    columns are NaN, their dbeta is the column sum of dy, and every other column has the bytes of the clean run"""
    m, n = 17, 192
    z, gamma, beta, dy = _bn_case(m, n, 5)
    bad = z.copy()
    bad[3, 5] = np.nan
    bad[11, 7] = np.inf
    bad[:, 9] = R.bf16_round(np.float32(3e38))
    cols = [5, 7, 9]
    gd, bd, dyd = _dev(gamma), _dev(beta), _dev(dy, torch.bfloat16)
    runs = []
    for a in (z, bad):
        zd = _dev(a, torch.bfloat16)
        y, mean, var, y_t = _bn_fwd(zd, gd, bd, m, n)
        runs.append((y, mean, var, y_t) + _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n))
    clean, dirty = runs
    assert all(f.intact() for f in dirty)
    y, mean, var, y_t, dz, dz_t, dgamma, dbeta, db = (f.np() for f in dirty)
    assert np.isnan(y[:, cols]).all() and np.isnan(dz[:, cols]).all() and np.isnan(dgamma[0, cols]).all() and np.isnan(db[0, cols]).all()
    assert np.isnan(y_t[cols, :m]).all() and not y_t[cols, m:].any() and np.isnan(dz_t[cols, :m]).all() and not dz_t[cols, m:].any()
    want = dy[:, cols].astype(np.float64).sum(0)
    assert (np.abs(dbeta[0, cols] - want) <= (m + 2) * U * np.abs(dy[:, cols]).astype(np.float64).sum(0)).all()
    keep = np.ones(n, dtype=bool)
    keep[cols] = False
    keep_d = torch.from_numpy(keep).to(DEV)
    for name, a, b in zip(("y", "mean", "var", "y_t", "dz", "dz_t", "dgamma", "dbeta", "db"), clean, dirty):
        va, vb = a.view.contiguous().view(INT[a.dtype]), b.view.contiguous().view(INT[b.dtype])
        if name in ("y_t", "dz_t"):
            assert torch.equal(va[keep_d], vb[keep_d]), name
        else:
            assert torch.equal(va[:, keep_d], vb[:, keep_d]), name


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_refused_and_nothing_is_written():
    L, s = _lib(), _stream()
    m, n = 4, 192
    a = torch.zeros((8, 256), dtype=torch.bfloat16, device=DEV)
    a32 = torch.zeros((8, 256), dtype=torch.float32, device=DEV)
    v = torch.zeros(256, dtype=torch.float32, device=DEV)
    out, out_t = Framed(8, 256), Framed(256, 64)
    o = [Framed(1, 256, 0, torch.float32) for _ in range(3)]

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == BAD_ARG and word in _err(), (rc, _err())
        assert not out.written() and not out_t.written() and not any(f.written() for f in o)

    f = C.c_float(EPS)
    ov, tv, o0, o1, o2 = _p(out.view), _p(out_t.view), _p(o[0].view), _p(o[1].view), _p(o[2].view)
    # the cast
    refused(L.c4_train_cast_bf16(_p(a32, 4), 0, m, 64, 256, ov, 256, tv, 64, s), "aligned")
    refused(L.c4_train_cast_bf16(_p(a32), 0, m, 64, 256, None, 256, None, 64, s), "null")
    refused(L.c4_train_cast_bf16(_p(a32), 0, m, 40, 256, ov, 256, tv, 64, s), "c % 16")
    refused(L.c4_train_cast_bf16(_p(a32), 0, m, 64, 252, ov, 256, tv, 64, s), "multiple of 8")
    refused(L.c4_train_cast_bf16(_p(a32), 0, m, 64, 256, ov, 32, tv, 64, s), "ldd >= c")
    refused(L.c4_train_cast_bf16(_p(a32), 0, 65, 64, 256, None, 0, tv, 64, s), "ldt >= 64 ceil(m / 64)")
    refused(L.c4_train_cast_bf16(_p(a32), 0, 0, 64, 256, ov, 256, tv, 64, s), "m >= 1")
    # the batch-norm kernels
    refused(L.c4_train_bn_relu_fwd_bf16(_p(a, 4), _p(v), _p(v), f, m, n, 256, 256, ov, o0, o1, tv, 64, s), "aligned")
    refused(L.c4_train_bn_relu_fwd_bf16(_p(a), _p(v), _p(v), f, m, 96, 256, 256, ov, o0, o1, tv, 64, s), "n % 192")
    refused(L.c4_train_bn_relu_fwd_bf16(_p(a), _p(v), _p(v), f, 1, n, 256, 256, ov, o0, o1, tv, 64, s), "m >= 2")
    refused(L.c4_train_bn_relu_fwd_bf16(_p(a), _p(v), _p(v), f, m, n, 256, 252, ov, o0, o1, tv, 64, s), "multiples of 8")
    refused(L.c4_train_bn_relu_fwd_bf16(_p(a), _p(v), _p(v), f, m, n, 256, 256, ov, o0, o1, tv, 60, s), "ldt >= 64 ceil(m / 64)")
    refused(L.c4_train_bn_relu_fwd_bf16(None, _p(v), _p(v), f, m, n, 256, 256, ov, o0, o1, tv, 64, s), "null")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v, 4), _p(v), f, m, n, 256, 256, 256, ov, tv, 64, o0, o1, o2, s), "aligned")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, m, 96, 256, 256, 256, ov, tv, 64, o0, o1, o2, s), "n % 192")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, 1, n, 256, 256, 256, ov, tv, 64, o0, o1, o2, s), "m >= 2")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, m, n, 256, 128, 256, ov, tv, 64, o0, o1, o2, s), "multiples of 8")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, m, n, 256, 256, 256, ov, None, 64, o0, o1, o2, s), "null")
    refused(L.c4_train_bn_relu_bwd_bf16(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, 65, n, 256, 256, 256, ov, tv, 64, o0, o1, o2, s), "ldt >= 64 ceil(m / 64)")
