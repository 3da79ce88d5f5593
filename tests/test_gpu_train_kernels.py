"""The training kernels of the heads' hidden blocks through the C ABI (c4a0_amd/csrc/c4_train.hip): c4_train_linear_dgrad_f32,
c4_train_linear_wgrad_f32, c4_train_bn_relu_fwd_f32 and c4_train_bn_relu_bwd_f32 against float64 numpy computed from the same f32
inputs.

* The products are held, element by element, to the forward-error bound of an L-term dot product, |err| <= gamma S with
  S = sum |a_i| |b_i| (float64), gamma = (L + 2) u / (1 - (L + 2) u), u = 2^-24: it holds for every summation order, fused or not,
  so it is derived, not measured.  With inputs in {-2 .. 2} every partial sum is an integer below 2^24 and the result must be exact.
* The batch-norm kernels are held to PyTorch's own f32 F.batch_norm(training=True) + ReLU and their autograd on the same device
  and inputs: both errors are taken against float64, and the kernel's largest may be at most 4 x PyTorch's (two correct f32
  reductions of one length differ by small constant factors; a wrong divisor or a missing term is off by orders of magnitude), with a
  floor of 4 * 2^-24 * max |ref|.
* Every output lies inside a frame of sentinels that must be intact afterwards; every kernel runs twice and must give the same bytes;
  what the ABI refuses is refused with C4_ERR_BAD_ARG, a message and nothing written.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG = 1
SENT = 0x5A5A5A5A            # an f32 bit pattern (about 1.5e16) no kernel computes here
U = 2.0 ** -24
EPS = 1e-5
# k = 16 and 48, odd multiples of 16, take the 16-wide kernels train_dgrad<1, 2> and train_wgrad<2, 1>: (64, 48) at m = 64 is 2 x 3 dgrad
# tiles in two workgroups, the second with idle wavefronts, (32, 16) at m = 1 a single live wavefront
NK = [(32, 32), (32, 672), (672, 32), (672, 672), (32, 16), (64, 48), (672, 48)]
M_GEMM = [1, 2, 3, 17, 64, 130, 257]      # 16-row tile tails and batch-reduction tails that are no multiple of 4
M_BN = M_GEMM[1:]


def _lib():
    from c4a0_amd import _lib as L

    return L.lib()


def _err():
    return (_lib().c4_last_error_string() or b"").decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _strided(a: np.ndarray) -> torch.Tensor:
    """a [rows, w] as a 16-byte aligned row view of stride w + 8 inside a NaN-filled tensor: a read outside the data shows."""
    t = torch.full((a.shape[0] + 2, a.shape[1] + 8), float("nan"), dtype=torch.float32, device=DEV)
    v = t[1:1 + a.shape[0], 4:4 + a.shape[1]]
    v.copy_(_dev(a))
    return v


class Framed:
    """An output [rows, cols] (row stride cols + pad) inside a buffer of sentinels: one row above and below, pad / 2 columns left and
    right (pad = 0: a dense matrix or a vector with sentinel rows only)."""

    def __init__(self, rows: int, cols: int, pad: int = 8):
        self.buf = torch.empty((rows + 2, cols + pad), dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(SENT)
        self.view = self.buf[1:1 + rows, pad // 2:pad // 2 + cols]
        self.ld = cols + pad
        assert self.view.data_ptr() % 16 == 0

    def intact(self) -> bool:
        b = self.buf.view(torch.int32).clone()
        r, c = self.view.shape
        off = (self.ld - c) // 2
        b[1:1 + r, off:off + c] = SENT
        return bool((b == SENT).all())

    def written(self) -> bool:
        return bool((self.view.contiguous().view(torch.int32) != SENT).any())

    def np(self):
        return self.view.cpu().numpy()


def _gamma(length: int) -> float:
    return (length + 2) * U / (1.0 - (length + 2) * U)


def _same_bytes(a: Framed, b: Framed) -> bool:
    return torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ products
def _dgrad(dz, w, m, n, k, strided=False):
    dx = Framed(m, k, 8 if strided else 0)
    rc = _lib().c4_train_linear_dgrad_f32(_p(dz), _p(w), _p(dx.view), m, n, k, dz.stride(0), dx.ld, _stream())
    assert rc == 0, _err()
    return dx


def _wgrad(dz, x, m, n, k):
    dw, db = Framed(n, k, 0), Framed(1, n, 0)
    rc = _lib().c4_train_linear_wgrad_f32(_p(dz), _p(x), _p(dw.view), _p(db.view), m, n, k, dz.stride(0), x.stride(0), _stream())
    assert rc == 0, _err()
    return dw, db


@pytest.fixture(scope="module", params=NK, ids=lambda s: f"N{s[0]}-K{s[1]}")
def operands(request):
    """dz [257, n], x [257, k], w [n, k]: f32 on the host, on the device (dense and as strided views) and in float64; shared and never
    changed.  Magnitudes spread over four decades so that S is not a constant times the result."""
    n, k = request.param
    rng = np.random.default_rng(1000 * n + k)
    mx = max(M_GEMM)

    def draw(*shape):
        return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(np.float32)

    host = {"dz": draw(mx, n), "x": draw(mx, k), "w": draw(n, k)}
    dev = {name: _dev(a) for name, a in host.items()}
    strided = {name: _strided(a) for name, a in host.items() if name != "w"}
    ints = {name: rng.integers(-2, 3, a.shape).astype(np.float32) for name, a in host.items()}
    return {"n": n, "k": k, "host": host, "dev": dev, "strided": strided, "ints": ints, "ints_dev": {name: _dev(a) for name, a in ints.items()}}


@pytest.mark.parametrize("m", M_GEMM)
def test_dgrad_is_within_the_dot_product_bound_and_repeats(operands, m):
    n, k, h, d = operands["n"], operands["k"], operands["host"], operands["dev"]
    dz64, w64 = h["dz"][:m].astype(np.float64), h["w"].astype(np.float64)
    ref, s = dz64 @ w64, np.abs(dz64) @ np.abs(w64)
    a, b = _dgrad(d["dz"], d["w"], m, n, k), _dgrad(d["dz"], d["w"], m, n, k)
    err = np.abs(a.np().astype(np.float64) - ref)
    assert (err <= _gamma(n) * s).all(), float((err / s).max() / _gamma(n))
    assert a.intact() and _same_bytes(a, b)
    evidence(f"train dgrad m={m} n={n} k={k}: max err / (gamma S) = {float((err / np.maximum(s, 1e-300)).max() / _gamma(n)):.3f}")


@pytest.mark.parametrize("m", M_GEMM)
def test_wgrad_and_db_are_within_the_dot_product_bound_and_repeat(operands, m):
    n, k, h, d = operands["n"], operands["k"], operands["host"], operands["dev"]
    dz64, x64 = h["dz"][:m].astype(np.float64), h["x"][:m].astype(np.float64)
    (dw, db), (dw2, db2) = _wgrad(d["dz"], d["x"], m, n, k), _wgrad(d["dz"], d["x"], m, n, k)
    err = np.abs(dw.np().astype(np.float64) - dz64.T @ x64)
    s = np.abs(dz64).T @ np.abs(x64)
    assert (err <= _gamma(m) * s).all(), float((err / s).max() / _gamma(m))
    err_b = np.abs(db.np()[0].astype(np.float64) - dz64.sum(0))
    assert (err_b <= _gamma(m) * np.abs(dz64).sum(0)).all()
    assert dw.intact() and db.intact() and _same_bytes(dw, dw2) and _same_bytes(db, db2)
    evidence(f"train wgrad m={m} n={n} k={k}: max err / (gamma S) = {float((err / np.maximum(s, 1e-300)).max() / _gamma(m)):.3f}")


@pytest.mark.parametrize("m", [1, 3, 130, 257])
def test_products_of_small_integers_are_exact(operands, m):
    """inputs in {-2 .. 2}: every product and partial sum is an integer below 2^24, so any correct order gives the exact result"""
    n, k, h, d = operands["n"], operands["k"], operands["ints"], operands["ints_dev"]
    dz64, x64, w64 = h["dz"][:m].astype(np.float64), h["x"][:m].astype(np.float64), h["w"].astype(np.float64)
    dx = _dgrad(d["dz"], d["w"], m, n, k)
    dw, db = _wgrad(d["dz"], d["x"], m, n, k)
    for got, want in ((dx.np(), dz64 @ w64), (dw.np(), dz64.T @ x64), (db.np()[0], dz64.sum(0))):
        # + 0.0 leaves every value but the sign of a zero as it is
        assert np.array_equal((got + np.float32(0)).view(np.int32), (want.astype(np.float32) + np.float32(0)).view(np.int32))


@pytest.mark.parametrize("m", [3, 130])
def test_products_read_and_write_strided_rows_in_place(operands, m):
    """dz, x and dx as row views of stride width + 8 with NaN beside every input and sentinels beside every output: the same bytes as
    from dense operands"""
    n, k, d, s = operands["n"], operands["k"], operands["dev"], operands["strided"]
    dense = _dgrad(d["dz"], d["w"], m, n, k)
    view = _dgrad(s["dz"], d["w"], m, n, k, strided=True)
    assert view.intact() and torch.equal(view.view.contiguous().view(torch.int32), dense.view.contiguous().view(torch.int32))
    (dw, db), (dw2, db2) = _wgrad(d["dz"], d["x"], m, n, k), _wgrad(s["dz"], s["x"], m, n, k)
    assert dw2.intact() and db2.intact() and _same_bytes(dw, dw2) and _same_bytes(db, db2)


# ------------------------------------------------------------------------------------------------------------------ batch norm
def _bn_case(m: int, n: int, seed: int):
    """z [m, n], gamma, beta, dy with the edge columns: 0 a constant column (1.25: var = 0, the mean exact), 1 gamma = 0,
    2 every pre-activation <= 0 (beta = -100), 3 every pre-activation exactly 0 (gamma = beta = 0).  dy is 0 where the float64
    pre-activation lies within 1e-4 of 0 (column 3 apart): there the sign of a rounding error would decide ReLU' for the kernel,
    for PyTorch and for nobody in float64."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-1, 1, n) + rng.standard_normal(n) * 3).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, n).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    beta = (rng.standard_normal(n) * 0.5).astype(np.float32)
    z[:, 0] = 1.25
    gamma[1] = 0.0
    beta[2] = -100.0
    gamma[3] = beta[3] = 0.0
    dy = rng.standard_normal((m, n)).astype(np.float32)
    pre = _bn_ref(z, gamma, beta)["pre"]
    near = np.abs(pre) < 1e-4
    near[:, 3] = False
    dy[near] = 0.0
    return z, gamma, beta, dy


def _bn_ref(z, gamma, beta, dy=None):
    z, gamma, beta = z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    m = z.shape[0]
    mean, var = z.mean(0), z.var(0)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(EPS)))
    xh = (z - mean) * rstd
    pre = xh * gamma + beta
    out = {"mean": mean, "var": var, "pre": pre, "y": np.maximum(pre, 0.0)}
    if dy is not None:
        g = np.where(pre > 0, dy.astype(np.float64), 0.0)
        out["dbeta"], out["dgamma"] = g.sum(0), (g * xh).sum(0)
        out["dz"] = gamma * rstd * (g - out["dbeta"] / m - xh * out["dgamma"] / m)
    return out


def _bn_fwd(z, gamma, beta, m, n, pad=0):
    y, mean, var = Framed(m, n, pad), Framed(1, n, 0), Framed(1, n, 0)
    rc = _lib().c4_train_bn_relu_fwd_f32(_p(z), _p(gamma), _p(beta), C.c_float(EPS), m, n, z.stride(0), y.ld, _p(y.view), _p(mean.view), _p(var.view),
                                         _stream())
    assert rc == 0, _err()
    return y, mean, var


def _bn_bwd(dy, z, mean, var, gamma, beta, m, n, pad=0):
    dz, dgamma, dbeta = Framed(m, n, pad), Framed(1, n, 0), Framed(1, n, 0)
    rc = _lib().c4_train_bn_relu_bwd_f32(_p(dy), _p(z), _p(mean), _p(var), _p(gamma), _p(beta), C.c_float(EPS), m, n, dy.stride(0), z.stride(0), dz.ld,
                                         _p(dz.view), _p(dgamma.view), _p(dbeta.view), _stream())
    assert rc == 0, _err()
    return dz, dgamma, dbeta


def _judge(what, got, torch_got, ref):
    """the 4 x rule: max |got - ref| <= max(4 max |torch - ref|, 4 * 2^-24 * max |ref|)"""
    e_k = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    e_t = float(np.abs(np.asarray(torch_got, dtype=np.float64) - ref).max())
    floor = 4 * U * float(np.abs(ref).max())
    evidence(f"{what}: kernel err {e_k:.3e}, PyTorch f32 err {e_t:.3e}, ratio {e_k / e_t if e_t else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


@pytest.mark.parametrize("n", [32, 672])
@pytest.mark.parametrize("m", M_BN)
def test_bn_relu_forward_and_backward_against_pytorch_f32(m, n):
    z, gamma, beta, dy = _bn_case(m, n, 7 * m + n)
    ref = _bn_ref(z, gamma, beta, dy)
    zd, gd, bd, dyd = _dev(z), _dev(gamma), _dev(beta), _dev(dy)
    # PyTorch's f32 on the same device and inputs
    zt, gt, bt = zd.clone().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    rm, rv = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    yt = torch.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 1.0, EPS))     # momentum 1: the running statistics are the batch's
    yt.backward(dyd)
    y, mean, var = _bn_fwd(zd, gd, bd, m, n)
    y2, mean2, var2 = _bn_fwd(zd, gd, bd, m, n)
    assert y.intact() and mean.intact() and var.intact() and _same_bytes(y, y2) and _same_bytes(mean, mean2) and _same_bytes(var, var2)
    tag = f"train bn m={m} n={n}"
    _judge(tag + " y", y.np(), yt.detach().cpu().numpy(), ref["y"])
    _judge(tag + " mean", mean.np()[0], rm.cpu().numpy(), ref["mean"])
    _judge(tag + " var", var.np()[0], (rv * ((m - 1) / m)).cpu().numpy(), ref["var"])
    assert np.array_equal(var.np()[0, :1], [0.0]) and np.array_equal(mean.np()[0, :1], [1.25])       # the constant column
    dz, dgamma, dbeta = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    dz2, dgamma2, dbeta2 = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    assert dz.intact() and dgamma.intact() and dbeta.intact()
    assert _same_bytes(dz, dz2) and _same_bytes(dgamma, dgamma2) and _same_bytes(dbeta, dbeta2)
    _judge(tag + " dz", dz.np(), zt.grad.cpu().numpy(), ref["dz"])
    _judge(tag + " dgamma", dgamma.np()[0], gt.grad.cpu().numpy(), ref["dgamma"])
    _judge(tag + " dbeta", dbeta.np()[0], bt.grad.cpu().numpy(), ref["dbeta"])
    got = dz.np()
    assert (got[:, 1] == 0).all()                                       # gamma = 0: nothing reaches z
    assert (got[:, 2] == 0).all() and dgamma.np()[0, 2] == 0 and dbeta.np()[0, 2] == 0   # no pre-activation above 0: exactly 0
    assert (y.np()[:, 3] == 0).all() and (got[:, 3] == 0).all() and dbeta.np()[0, 3] == 0  # pre-activations of exactly 0: ReLU'(0) = 0


def test_bn_relu_reads_and_writes_strided_rows_in_place():
    m, n = 17, 672
    z, gamma, beta, dy = _bn_case(m, n, 99)
    zd, gd, bd, dyd = _dev(z), _dev(gamma), _dev(beta), _dev(dy)
    y, mean, var = _bn_fwd(zd, gd, bd, m, n)
    ys, means, vars_ = _bn_fwd(_strided(z), gd, bd, m, n, pad=8)
    assert ys.intact() and torch.equal(ys.view.contiguous(), y.view.contiguous()) and _same_bytes(mean, means) and _same_bytes(var, vars_)
    dz, dgamma, dbeta = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
    dzs, dgammas, dbetas = _bn_bwd(_strided(dy), _strided(z), mean.view[0], var.view[0], gd, bd, m, n, pad=8)
    assert dzs.intact() and torch.equal(dzs.view.contiguous(), dz.view.contiguous()) and _same_bytes(dgamma, dgammas) and _same_bytes(dbeta, dbetas)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_refused_and_nothing_is_written():
    L, s = _lib(), _stream()
    m, n, k = 4, 32, 32
    a = torch.zeros((8, 64), dtype=torch.float32, device=DEV)
    v = torch.zeros(64, dtype=torch.float32, device=DEV)
    out, o1, o2 = Framed(8, 64, 0), Framed(1, 64, 0), Framed(1, 64, 0)

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == BAD_ARG and word in _err(), (rc, _err())
        assert not out.written() and not o1.written() and not o2.written()

    f = C.c_float(EPS)
    # a misaligned pointer (4 bytes past a 16-byte boundary), in every call
    refused(L.c4_train_linear_dgrad_f32(_p(a, 4), _p(a), _p(out.view), m, n, k, 64, 64, s), "aligned")
    refused(L.c4_train_linear_wgrad_f32(_p(a), _p(a, 4), _p(out.view), _p(o1.view), m, n, k, 64, 64, s), "aligned")
    refused(L.c4_train_bn_relu_fwd_f32(_p(a, 4), _p(v), _p(v), f, m, n, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "aligned")
    refused(L.c4_train_bn_relu_bwd_f32(_p(a), _p(a), _p(v), _p(v), _p(v, 4), _p(v), f, m, n, 64, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "aligned")
    # n % 32 != 0, k % 16 != 0, a leading dimension that is no multiple of 4 or below the width
    refused(L.c4_train_linear_dgrad_f32(_p(a), _p(a), _p(out.view), m, 48, k, 64, 64, s), "n % 32")
    refused(L.c4_train_linear_wgrad_f32(_p(a), _p(a), _p(out.view), _p(o1.view), m, 48, k, 64, 64, s), "n % 32")
    refused(L.c4_train_linear_dgrad_f32(_p(a), _p(a), _p(out.view), m, n, 24, 64, 64, s), "k % 16")
    refused(L.c4_train_linear_wgrad_f32(_p(a), _p(a), _p(out.view), _p(o1.view), m, n, k, 62, 64, s), "multiples of 4")
    refused(L.c4_train_linear_dgrad_f32(_p(a), _p(a), _p(out.view), m, n, k, 64, 16, s), "ldx >= k")
    refused(L.c4_train_bn_relu_fwd_f32(_p(a), _p(v), _p(v), f, m, 48, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "n % 32")
    refused(L.c4_train_bn_relu_bwd_f32(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, m, 48, 64, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "n % 32")
    # batch statistics of one row
    refused(L.c4_train_bn_relu_fwd_f32(_p(a), _p(v), _p(v), f, 1, n, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "m >= 2")
    refused(L.c4_train_bn_relu_bwd_f32(_p(a), _p(a), _p(v), _p(v), _p(v), _p(v), f, 1, n, 64, 64, 64, _p(out.view), _p(o1.view), _p(o2.view), s), "m >= 2")
    refused(L.c4_train_linear_wgrad_f32(_p(a), _p(a), _p(out.view), _p(o1.view), 0, n, k, 64, 64, s), "m >= 1")
    refused(L.c4_train_linear_dgrad_f32(None, _p(a), _p(out.view), m, n, k, 64, 64, s), "null")
