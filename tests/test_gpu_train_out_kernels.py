"""The training kernels of the heads' output layers and the loss through the C ABI (c4a0_amd/csrc/c4_train_out.hip):
c4_train_out_loss_fwd and c4_train_out_loss_bwd against float64 numpy (tests/train_out_ref.py) computed from the same inputs.

* The backward's products are held, element by element, to the forward-error bound of an L-term dot product, |err| <= gamma S with
  S = |scale| sum |a_i| |b_i| (float64), gamma = (L + 3) u / (1 - (L + 3) u), u = 2^-24, L = 7 or 2 (dx) or m (dW, db): the existing
  file's bound for L + 1 terms, the multiplication by scale being the one more.  It holds for every summation order, so it is derived,
  not measured.  A bf16 dx gets half a bf16 ulp
  more.  With inputs in {-2 .. 2} and scale = 1 every result must be exact.
* The forward is held to PyTorch's own f32 ops (F.linear, log_softmax, tanh, train_common.loss and their autograd) on the same device
  and inputs: both errors are taken against float64, and the kernel's largest may be at most 4 x PyTorch's, with a floor of
  4 * 2^-24 * max |ref|.
* Every output lies inside a frame of sentinels that must be intact afterwards; every call runs twice and must give the same bytes;
  what the ABI refuses is refused with C4_ERR_BAD_ARG, a message that starts with the function's name and nothing written.

k: 8 is less than one wavefront's vector loads, 40 a tail, 672 is F at C = 16.  m, for the 64-row chunk: 1, 2, one below, at and one above
a chunk, a ragged tail, and 577 = nine chunks + one row, where the second stage has more than one term in a group.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c4a0_amd.train_common import loss
from tests import train_out_ref as ref
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG = 1
SENT = {4: 0x5A5A5A5A, 2: 0x5A5A}     # bit patterns (an f32 of about 1.5e16, a bf16 of about 1.5e16) no kernel computes here
INT = {4: torch.int32, 2: torch.int16}
U = 2.0 ** -24
KS = [8, 40, 672]
MS = [1, 2, 63, 64, 65, 130, 577]
M_MAX = max(MS)


def _lib():
    from c4a0_amd import _lib as L

    return L.lib()


def _err():
    return (_lib().c4_last_error_string() or b"").decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), device=DEV).to(dtype)


def _strided(a: torch.Tensor) -> torch.Tensor:
    """a [rows, w] as a 16-byte aligned row view of stride w + 16 inside a NaN-filled tensor: a read outside the data shows."""
    t = torch.full((a.shape[0] + 2, a.shape[1] + 16), float("nan"), dtype=a.dtype, device=DEV)
    v = t[1:1 + a.shape[0], 8:8 + a.shape[1]]
    v.copy_(a)
    assert v.data_ptr() % 16 == 0
    return v


class Framed:
    """An output [rows, cols] inside a buffer of sentinels.  Dense: 64 bytes of sentinels before and after.  strided: a row view with
    16 bytes of sentinels left and right of every row and a row of them above and below."""

    def __init__(self, rows: int, cols: int, dtype=torch.float32, strided: bool = False):
        size = torch.empty((), dtype=dtype).element_size()
        self.int, self.sent = INT[size], SENT[size]
        if strided:
            e16 = 16 // size
            self.buf = torch.empty((rows + 2, cols + 2 * e16), dtype=dtype, device=DEV)
            self.view = self.buf[1:1 + rows, e16:e16 + cols]
            self.ld = cols + 2 * e16
        else:
            g = 64 // size
            self.buf = torch.empty(2 * g + rows * cols, dtype=dtype, device=DEV)
            self.view = self.buf[g:g + rows * cols].view(rows, cols)
            self.ld = cols
        self.buf.view(self.int).fill_(self.sent)
        assert self.view.data_ptr() % 16 == 0

    def intact(self) -> bool:
        b = self.buf.view(self.int).clone()
        if b.dim() == 2:
            (r, c), off = self.view.shape, (b.shape[1] - self.view.shape[1]) // 2
            b[1:1 + r, off:off + c] = self.sent
        else:
            g = (b.numel() - self.view.numel()) // 2
            b[g:g + self.view.numel()] = self.sent
        return bool((b == self.sent).all())

    def written(self) -> bool:
        return bool((self.view.contiguous().view(self.int) != self.sent).any())

    def bits(self) -> torch.Tensor:
        return self.view.contiguous().view(self.int)

    def np(self):
        return self.view.float().cpu().numpy() if self.view.dtype == torch.bfloat16 else self.view.cpu().numpy()


def _same(a: Framed, b: Framed) -> bool:
    return torch.equal(a.buf.view(a.int), b.buf.view(b.int))


def _gamma(length: int) -> float:
    return (length + 2) * U / (1.0 - (length + 2) * U)


def _work(m, k):
    n = C.c_uint64(0)
    assert _lib().c4_train_out_work_bytes(m, k, C.byref(n)) == 0, _err()
    assert n.value == ref.work_bytes(m, k)
    return torch.full((n.value // 4,), float("nan"), dtype=torch.float32, device=DEV)   # the contents are meaningless between calls


def _fwd(xp, xv, wp, bp, wv, bv, t, tp, tn, m, k):
    out, dz, losses = Framed(m, 9), Framed(m, 9), Framed(1, 4)
    rc = _lib().c4_train_out_loss_fwd(_p(xp), _p(xv), int(xp.dtype == torch.bfloat16), xp.stride(0), xv.stride(0), _p(wp), _p(bp), _p(wv), _p(bv),
                                      _p(t), _p(tp), _p(tn), m, k, _p(out.view), _p(dz.view), _p(losses.view), _p(_work(m, k)), _stream())
    assert rc == 0, _err()
    return out, dz, losses


def _bwd(dz, scale, xp, xv, wp, wv, m, k, strided=False, dxp=True, dxv=True):
    """-> Framed dxp, dxv (None where skipped), dwp, dbp, dwv, dbv"""
    o_xp = Framed(m, k, xp.dtype, strided) if dxp else None
    o_xv = Framed(m, k, xv.dtype, strided) if dxv else None
    dwp, dbp, dwv, dbv = Framed(7, k), Framed(1, 7), Framed(2, k), Framed(1, 2)
    rc = _lib().c4_train_out_loss_bwd(_p(dz), _p(scale), _p(xp), _p(xv), int(xp.dtype == torch.bfloat16), xp.stride(0), xv.stride(0), _p(wp), _p(wv),
                                      m, k, _p(o_xp.view) if dxp else None, _p(o_xv.view) if dxv else None, o_xp.ld if dxp else 0,
                                      o_xv.ld if dxv else 0, _p(dwp.view), _p(dbp.view), _p(dwv.view), _p(dbv.view), _p(_work(m, k)), _stream())
    assert rc == 0, _err()
    return o_xp, o_xv, dwp, dbp, dwv, dbv


def _bf16_half_ulp(x: np.ndarray) -> np.ndarray:
    """half a bf16 ulp (8 significant bits) at |x|"""
    return np.ldexp(1.0, np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))).astype(np.int64) - 8)


# ------------------------------------------------------------------------------------------------------------------ operands
@pytest.fixture(scope="module", params=KS, ids=lambda k: f"K{k}")
def operands(request):
    """For one k: activations, weights, targets and a given dz for M_MAX rows -- f32 on the host and on the device, the activations
    also rounded to bf16 (host values widened back) -- shared and never changed.  dz's and x's magnitudes are spread over four decades so
    that S is not a constant times the result."""
    k = request.param
    rng = np.random.default_rng(4000 + k)

    def spread(*shape):
        return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(np.float32)

    bound = 1.0 / np.sqrt(k)                                   # nn.Linear's initialisation
    h = {"xp": rng.standard_normal((M_MAX, k)).astype(np.float32), "xv": rng.standard_normal((M_MAX, k)).astype(np.float32),
         "wp": rng.uniform(-bound, bound, (7, k)).astype(np.float32), "bp": rng.uniform(-bound, bound, 7).astype(np.float32),
         "wv": rng.uniform(-bound, bound, (2, k)).astype(np.float32), "bv": rng.uniform(-bound, bound, 2).astype(np.float32),
         "tp": rng.uniform(-1, 1, M_MAX).astype(np.float32), "tn": np.sign(rng.uniform(-1, 1, M_MAX)).astype(np.float32),
         "dz": spread(M_MAX, 9), "sxp": spread(M_MAX, k), "sxv": spread(M_MAX, k), "swp": spread(7, k), "swv": spread(2, k)}
    # targets: visit-count-like rows, one-hot rows (every third) and a peaked teacher (softmax of logits x 8, every third)
    t = rng.random((M_MAX, 7))
    t[rng.random((M_MAX, 7)) < 0.3] = 0.0
    t[:, 3] += 0.05
    t /= t.sum(axis=1, keepdims=True)
    onehot = np.eye(7)[rng.integers(0, 7, M_MAX)]
    logits = 8.0 * rng.standard_normal((M_MAX, 7))
    teacher = np.exp(logits - logits.max(axis=1, keepdims=True))
    teacher /= teacher.sum(axis=1, keepdims=True)
    rows = np.arange(M_MAX)
    t[rows % 3 == 0] = onehot[rows % 3 == 0]
    t[rows % 3 == 1] = teacher[rows % 3 == 1]
    h["t"] = t.astype(np.float32)
    d = {name: _dev(a) for name, a in h.items()}
    for name in ("xp", "xv", "sxp", "sxv"):
        d[name + "_bf16"] = d[name].to(torch.bfloat16)
        h[name + "_bf16"] = d[name + "_bf16"].float().cpu().numpy()
    ints = {name: rng.integers(-2, 3, h[name].shape).astype(np.float32) for name in ("dz", "xp", "xv", "wp", "wv")}
    return {"k": k, "host": h, "dev": d, "ints": ints, "ints_dev": {name: _dev(a) for name, a in ints.items()},
            "one": torch.ones(4, device=DEV), "scale": torch.tensor([0.8125, 0.0, 0.0, 0.0], device=DEV)}


# ------------------------------------------------------------------------------------------------------------------ backward alone
def _check_bwd(tag, got, want, dz, scale, xp, xv, wp, wv, m, bf16):
    """every element within gamma S of the float64 result (dx in bf16: plus half a bf16 ulp)"""
    dz, xp, xv, wp, wv = (np.asarray(a, dtype=np.float64) for a in (dz, xp, xv, wp, wv))
    gp, gv, s = np.abs(dz[:, :7]), np.abs(dz[:, 7:]), abs(scale)
    bounds = (_gamma(7 + 1) * s * (gp @ np.abs(wp)), _gamma(2 + 1) * s * (gv @ np.abs(wv)), _gamma(m + 1) * s * (gp.T @ np.abs(xp)),
              _gamma(m + 1) * s * gp.sum(0), _gamma(m + 1) * s * (gv.T @ np.abs(xv)), _gamma(m + 1) * s * gv.sum(0))
    worst = 0.0
    for i, (name, g, w, b) in enumerate(zip(("dxp", "dxv", "dwp", "dbp", "dwv", "dbv"), got, want, bounds)):
        if g is None:
            continue
        w = np.asarray(w, dtype=np.float64).reshape(g.view.shape)
        b = np.asarray(b).reshape(g.view.shape)
        if bf16 and i < 2:
            b = b + _bf16_half_ulp(np.abs(w) + b)
        err = np.abs(g.np().astype(np.float64) - w)
        assert (err <= b).all(), (tag, name, float((err / np.maximum(b, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    evidence(f"{tag}: max err / bound = {worst:.3f}")


@pytest.mark.parametrize("m", MS)
def test_backward_is_within_the_dot_product_bound_and_repeats(operands, m):
    k, h, d = operands["k"], operands["host"], operands["dev"]
    scale = float(operands["scale"][0])
    # f32 x, dense
    a = _bwd(d["dz"], operands["scale"], d["sxp"], d["sxv"], d["swp"], d["swv"], m, k)
    b = _bwd(d["dz"], operands["scale"], d["sxp"], d["sxv"], d["swp"], d["swv"], m, k)
    assert all(x.intact() for x in a) and all(_same(x, y) for x, y in zip(a, b))
    want = ref.backward(h["dz"][:m], scale, h["sxp"][:m], h["sxv"][:m], h["swp"], h["swv"])
    _check_bwd(f"train out bwd f32 m={m} k={k}", a, want, h["dz"][:m], scale, h["sxp"][:m], h["sxv"][:m], h["swp"], h["swv"], m, False)
    # bf16 x in strided rows with NaN beside them, dx into strided rows with sentinels beside them
    xp, xv = _strided(d["sxp_bf16"][:m]), _strided(d["sxv_bf16"][:m])
    c = _bwd(d["dz"], operands["scale"], xp, xv, d["swp"], d["swv"], m, k, strided=True)
    c2 = _bwd(d["dz"], operands["scale"], xp, xv, d["swp"], d["swv"], m, k, strided=True)
    assert all(x.intact() for x in c) and all(_same(x, y) for x, y in zip(c, c2))
    want = ref.backward(h["dz"][:m], scale, h["sxp_bf16"][:m], h["sxv_bf16"][:m], h["swp"], h["swv"])
    _check_bwd(f"train out bwd bf16 m={m} k={k}", c, want, h["dz"][:m], scale, h["sxp_bf16"][:m], h["sxv_bf16"][:m], h["swp"], h["swv"], m, True)
    # the same sums in the same order whatever the type of x: on the widened bf16 values the f32 call gives the bf16 call's dW and db
    # bit for bit, and its dx rounded once is the bf16 call's dx
    e = _bwd(d["dz"], operands["scale"], d["sxp_bf16"][:m].float(), d["sxv_bf16"][:m].float(), d["swp"], d["swv"], m, k)
    assert all(torch.equal(x.bits(), y.bits()) for x, y in zip(c[2:], e[2:]))
    assert all(torch.equal(x.view.contiguous(), y.view.to(torch.bfloat16)) for x, y in zip(c[:2], e[:2]))


@pytest.mark.parametrize("m", [1, 65, 577])
def test_backward_of_small_integers_is_exact(operands, m):
    """dz, x and W in {-2 .. 2}, scale = 1: every product and partial sum is an integer below 2^24 (below 2^8 in a bf16 dx), so any
    correct order gives the exact result"""
    k, h, d = operands["k"], operands["ints"], operands["ints_dev"]
    want = ref.backward(h["dz"][:m], 1.0, h["xp"][:m], h["xv"][:m], h["wp"], h["wv"])
    for dtype in (torch.float32, torch.bfloat16):
        got = _bwd(d["dz"], operands["one"], d["xp"].to(dtype), d["xv"].to(dtype), d["wp"], d["wv"], m, k)
        for g, w in zip(got, want):
            w = w.reshape(g.view.shape).astype(np.float32)
            # + 0.0 leaves every value but the sign of a zero as it is
            assert np.array_equal((g.np() + np.float32(0)).view(np.int32), (w + np.float32(0)).view(np.int32))


@pytest.mark.parametrize("m", [2, 130])
def test_backward_scale_and_null_dx(operands, m):
    k, d = operands["k"], operands["dev"]
    half = torch.tensor([0.5, 7.0, 7.0, 7.0], device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        xp, xv = d["xp"].to(dtype), d["xv"].to(dtype)
        full = _bwd(d["dz"], operands["one"], xp, xv, d["wp"], d["wv"], m, k)
        halved = _bwd(d["dz"], half, xp, xv, d["wp"], d["wv"], m, k)
        for a, b in zip(full, halved):       # the values here are far from the subnormals: a half is exact
            assert torch.equal((a.view.float() * 0.5), b.view.float())
        # a NULL dxp / dxv: that head's dx is not written, everything else is the same bytes
        no_p = _bwd(d["dz"], operands["one"], xp, xv, d["wp"], d["wv"], m, k, dxp=False)
        no_v = _bwd(d["dz"], operands["one"], xp, xv, d["wp"], d["wv"], m, k, dxv=False)
        neither = _bwd(d["dz"], operands["one"], xp, xv, d["wp"], d["wv"], m, k, dxp=False, dxv=False)
        for other, skipped in ((no_p, (0,)), (no_v, (1,)), (neither, (0, 1))):
            for i, (a, b) in enumerate(zip(full, other)):
                assert (b is None) if i in skipped else (b.intact() and _same(a, b))
    # both heads reading one buffer (a network without hidden layers)
    one = _bwd(d["dz"], operands["one"], d["xp"], d["xp"], d["wp"], d["wv"], m, k)
    two = _bwd(d["dz"], operands["one"], d["xp"], d["xp"].clone(), d["wp"], d["wv"], m, k)
    assert all(_same(a, b) for a, b in zip(one, two))


# ------------------------------------------------------------------------------------------------------------------ forward
def _torch_f32(xp, xv, wp, bp, wv, bv, t, tp, tn, upstream=None):
    """stock f32 PyTorch on the same device and values: out [m, 9], dz at the pre-activations by autograd, losses [4] and the six
    gradients (dxp, dxv, dwp, dbp, dwv, dbv)"""
    xp, xv, wp, bp, wv, bv = (a.detach().clone().requires_grad_() for a in (xp, xv, wp, bp, wv, bv))
    zp, zv = F.linear(xp, wp, bp), F.linear(xv, wv, bv)
    zp.retain_grad()
    zv.retain_grad()
    logp, q = F.log_softmax(zp, dim=1), torch.tanh(zv)
    losses = loss((logp, q[:, 0], q[:, 1]), (None, t, tp, tn))
    losses[0].backward()
    out = torch.cat([logp, q], dim=1).detach().cpu().numpy()
    dz = torch.cat([zp.grad, zv.grad], dim=1).cpu().numpy()
    grads = tuple(a.grad.cpu().numpy() for a in (xp, xv, wp, bp, wv, bv))
    return out, dz, np.array([float(v.detach()) for v in losses], dtype=np.float32), grads


def _judge(what, got, torch_got, want, where=None):
    """the 4 x rule: max |got - ref| <= max(4 max |torch - ref|, 4 * 2^-24 * max |ref|), over the elements `where` (all)"""
    got, torch_got, want = (np.asarray(a, dtype=np.float64) for a in (got, torch_got, want))
    if where is not None:
        got, torch_got, want = got[where], torch_got[where], want[where]
    if got.size == 0:
        return
    e_k, e_t = float(np.abs(got - want).max()), float(np.abs(torch_got - want).max())
    floor = 4 * U * float(np.abs(want).max())
    evidence(f"{what}: kernel err {e_k:.3e}, PyTorch f32 err {e_t:.3e}, ratio {e_k / e_t if e_t else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


@pytest.mark.parametrize("m", MS)
def test_forward_against_float64_beside_pytorch_f32(operands, m):
    k, h, d = operands["k"], operands["host"], operands["dev"]
    names = ("xp", "xv", "wp", "bp", "wv", "bv", "t", "tp", "tn")
    args = [d[n][:m] if n in ("xp", "xv", "t", "tp", "tn") else d[n] for n in names]
    a, b = _fwd(*args, m, k), _fwd(*args, m, k)
    assert all(x.intact() for x in a) and all(_same(x, y) for x, y in zip(a, b))
    want = ref.forward(*[h[n][:m] if n in ("xp", "xv", "t", "tp", "tn") else h[n] for n in names])
    t_out, t_dz, t_losses, _ = _torch_f32(*args)
    tag = f"train out fwd m={m} k={k}"
    _judge(tag + " out", a[0].np(), t_out, want[0])
    _judge(tag + " dz", a[1].np(), t_dz, want[1])
    for i, name in enumerate(("total", "kl", "mse_pen", "mse_nopen")):
        _judge(f"{tag} {name}", a[2].np()[0, i], t_losses[i], want[2][i])
    # bf16 activations in strided rows: the bytes of the f32 call on the widened values
    xp, xv = d["xp_bf16"][:m], d["xv_bf16"][:m]
    c = _fwd(_strided(xp), _strided(xv), *args[2:], m, k)
    e = _fwd(xp.float(), xv.float(), *args[2:], m, k)
    assert all(x.intact() for x in c) and all(_same(x, y) for x, y in zip(c, e))


@pytest.mark.parametrize("k", [40, 672])
def test_a_rows_outputs_do_not_depend_on_m_or_on_where_the_row_lies(k):
    rng = np.random.default_rng(k)
    m = 130
    bound = 1.0 / np.sqrt(k)
    xp, xv = _dev(rng.standard_normal((m, k)).astype(np.float32)), _dev(rng.standard_normal((m, k)).astype(np.float32))
    wp, bp = _dev(rng.uniform(-bound, bound, (7, k)).astype(np.float32)), _dev(rng.uniform(-bound, bound, 7).astype(np.float32))
    wv, bv = _dev(rng.uniform(-bound, bound, (2, k)).astype(np.float32)), _dev(rng.uniform(-bound, bound, 2).astype(np.float32))
    t = rng.random((m, 7))
    t = _dev((t / t.sum(axis=1, keepdims=True)).astype(np.float32))
    tp, tn = _dev(rng.uniform(-1, 1, m).astype(np.float32)), _dev(rng.uniform(-1, 1, m).astype(np.float32))
    whole = _fwd(xp, xv, wp, bp, wv, bv, t, tp, tn, m, k)[0].bits()
    for at in ([0, 1, 2], [63, 64, 129], [7, 100, 128]):
        idx = torch.tensor(at, device=DEV)
        three = _fwd(xp[idx], xv[idx], wp, bp, wv, bv, t[idx], tp[idx], tn[idx], 3, k)[0].bits()
        assert torch.equal(three, whole[idx]), at


# ------------------------------------------------------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("where", ["xp", "xv", "t"])
def test_a_nan_goes_where_pytorch_sends_it_and_nowhere_else(where):
    m, k = 65, 40
    rng = np.random.default_rng(65)
    bound = 1.0 / np.sqrt(k)
    h = {"xp": rng.standard_normal((m, k)), "xv": rng.standard_normal((m, k)), "wp": rng.uniform(-bound, bound, (7, k)),
         "bp": rng.uniform(-bound, bound, 7), "wv": rng.uniform(-bound, bound, (2, k)), "bv": rng.uniform(-bound, bound, 2)}
    t = rng.random((m, 7))
    h["t"] = t / t.sum(axis=1, keepdims=True)
    h["tp"], h["tn"] = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    h = {n: a.astype(np.float32) for n, a in h.items()}
    h[where][17, 5] = np.nan
    names = ("xp", "xv", "wp", "bp", "wv", "bv", "t", "tp", "tn")
    args = [_dev(h[n]) for n in names]
    out, dz, losses = _fwd(*args, m, k)
    grads = _bwd(dz.view, torch.ones(4, device=DEV), args[0], args[1], args[2], args[4], m, k)
    assert out.intact() and dz.intact() and losses.intact() and all(g.intact() for g in grads)
    t_out, t_dz, t_losses, t_grads = _torch_f32(*args)
    with np.errstate(invalid="ignore"):
        want = ref.forward(*[h[n] for n in names])
        want_grads = ref.backward(want[1], 1.0, h["xp"], h["xv"], h["wp"], h["wv"])
    got = [out.np(), dz.np(), losses.np()[0]] + [g.np() for g in grads]
    theirs = [t_out, t_dz, t_losses] + list(t_grads)
    wants = list(want) + list(want_grads)
    n_bad = 0
    for name, g, th, w in zip(("out", "dz", "losses", "dxp", "dxv", "dwp", "dbp", "dwv", "dbv"), got, theirs, wants):
        th, w = np.asarray(th).reshape(g.shape), np.asarray(w).reshape(g.shape)
        fin = np.isfinite(th)
        assert np.array_equal(np.isfinite(g), fin), (where, name, int((~np.isfinite(g)).sum()), int((~fin).sum()))
        assert np.array_equal(np.isfinite(w), fin), (where, name)       # float64 agrees on where the NaN goes
        n_bad += int((~fin).sum())
        _judge(f"train out nan in {where}: {name}", g, th, w, fin)
    assert n_bad > 0 and np.isfinite(got[0]).sum() > 0
    evidence(f"train out nan in {where}: {n_bad} non-finite elements, the same as PyTorch's")


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_refused_by_name_and_nothing_is_written():
    L, s = _lib(), _stream()
    m, k = 4, 16
    a = torch.zeros((8, 64), dtype=torch.float32, device=DEV)
    v = torch.zeros(64, dtype=torch.float32, device=DEV)
    outs = [Framed(8, 64) for _ in range(7)]
    o = [_p(f.view) for f in outs]
    assert L.c4_train_out_chunk_rows() == ref.CHUNK == 64

    def refused(rc, me, word):
        torch.cuda.synchronize()
        assert rc == BAD_ARG and _err().startswith(me) and word in _err(), (rc, _err())
        assert not any(f.written() for f in outs)

    def fwd(xp=_p(a), ldxp=64, m=m, k=k, bf16=0, work=_p(a)):
        return L.c4_train_out_loss_fwd(xp, _p(a), bf16, ldxp, 64, _p(a), _p(v), _p(a), _p(v), _p(a), _p(v), _p(v), m, k, o[0], o[1], o[2], work, s)

    def bwd(dz=_p(a), ldxp=64, lddxp=64, m=m, k=k, bf16=0, scale=_p(v)):
        return L.c4_train_out_loss_bwd(dz, scale, _p(a), _p(a), bf16, ldxp, 64, _p(a), _p(a), m, k, o[0], o[1], lddxp, 64, o[2], o[3], o[4], o[5],
                                       o[6], s)

    f, b = "c4_train_out_loss_fwd", "c4_train_out_loss_bwd"
    refused(fwd(m=0), f, "m >= 1")
    refused(bwd(m=0), b, "m >= 1")
    refused(fwd(k=12), f, "multiple of 8")
    refused(bwd(k=12), b, "multiple of 8")
    refused(fwd(k=0), f, "multiple of 8")
    refused(fwd(xp=_p(a, 4)), f, "aligned")                      # 4 bytes past a 16-byte boundary
    refused(bwd(dz=_p(a, 4)), b, "aligned")
    refused(bwd(scale=_p(v, 2)), b, "scale")
    refused(fwd(ldxp=62), f, "ldxp")                             # no multiple of 4
    refused(fwd(ldxp=8), f, "ldxp")                              # below k
    refused(fwd(ldxp=20, bf16=1), f, "ldxp")                     # bf16 rows: a multiple of 8
    refused(bwd(ldxp=62), b, "ldxp")
    refused(bwd(lddxp=62), b, "lddxp")
    refused(bwd(lddxp=8), b, "lddxp")
    refused(fwd(work=None), f, "null")
    refused(bwd(dz=None), b, "null")
    n = C.c_uint64(77)
    for bad in ((0, 8), (4, 12), (4, 0)):
        assert L.c4_train_out_work_bytes(bad[0], bad[1], C.byref(n)) == BAD_ARG and _err().startswith("c4_train_out_work_bytes") and n.value == 77
    for mm, kk in ((1, 8), (65, 40), (577, 672), (2000, 1344), (2000, 8)):
        assert L.c4_train_out_work_bytes(mm, kk, C.byref(n)) == 0 and n.value == ref.work_bytes(mm, kk)
