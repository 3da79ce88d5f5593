"""The training kernels of the convolution tower through the C ABI (c4a0_amd/csrc/c4_train_tower.hip): c4_train_conv0_f32,
c4_train_conv3x3_f32 (forward, and dgrad with the tap-flipped weights), c4_train_conv0_wgrad_f32, c4_train_conv3x3_wgrad_f32,
c4_train_bn2d_relu_res_fwd_f32 and c4_train_bn2d_relu_res_bwd_f32 against tests/train_tower_ref.py, the float64 numpy restatement
that tests/test_train_tower_ref.py pins to float64 PyTorch, computed from the same f32 inputs.

* The products are held, element by element, to the forward-error bound of an L-term dot product, |err| <= gamma S with
  S = sum |a_i| |b_i| (float64), gamma = (L + 2) u / (1 - (L + 2) u), u = 2^-24: L = 18 for the first convolution (its 14 zero columns
  add exact zeros), 9 C for the 3x3 ones and dgrad, 42 B for wgrad and db.  L + 2 covers the roundings any term goes through: the chain
  and the bias add of a convolution; for wgrad a chunk's chain of at most 672 rows and then at most ceil(n_chunks / 8) + 7 adds of the
  second stage, fewer than the rows of the other chunks
  (one chunk: the chain alone).  It holds for every summation order, so it is derived, not measured.  With inputs in {-2 .. 2} every partial sum is an
  integer below 2^24 and the result must be exact; a single 1.0 at a corner or centre cell must land on exactly the restatement's taps.
* The batch-norm kernels are held to PyTorch's own f32 F.batch_norm(training=True) + ReLU + add and their autograd on the same device
  and inputs: both errors are taken against float64, the kernel's largest may be at most 4 x PyTorch's, with a floor of
  4 * 2^-24 * max |ref| (tests/test_gpu_train_kernels.py says why).
* Every output and the work space lie inside frames of sentinels that must be intact afterwards; every call runs twice and must give
  the same bytes; what the ABI refuses is refused with C4_ERR_BAD_ARG, a message and nothing written.

Shapes: C in {16, 32, 64}; B in {1, 2, 3, 7, 25} (42 B is never a multiple of 64: the forward's row tiles have tails) and B = 16, 17, 32:
exactly one chunk of C4_TRAIN_TOWER_CHUNK_BOARDS = 16 boards, one chunk plus one board, exactly two chunks.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c4a0_amd.train_tower import work_bytes
from tests import train_tower_ref as ref
from tests.helpers import evidence
from tests.test_gpu_train_kernels import BAD_ARG, DEV, EPS, Framed, _dev, _err, _gamma, _judge, _lib, _p, _same_bytes, _stream

pytestmark = pytest.mark.gpu
CHANNELS = [16, 32, 64]
CHUNK = 16
BOARDS = [1, 2, 3, 7, 25, CHUNK, CHUNK + 1, 2 * CHUNK]
B_MAX = max(BOARDS)
CASES = [(c, b) for c in CHANNELS for b in BOARDS]
IDS = [f"C{c}-B{b}" for c, b in CASES]


def test_the_chunk_is_the_documented_one():
    from c4a0_amd import _lib as L

    assert L.TOWER_CHUNK_BOARDS == CHUNK
    for c in CHANNELS + [48]:
        for b in (1, 16, 17, 2000):
            assert work_bytes(b, c) == -(-b // CHUNK) * (9 * c * c + c) * 4
    n = C.c_uint64(77)
    for b, c, word in ((5, 24, "channels must be"), (0, 32, "n_boards >= 1")):
        assert _lib().c4_train_tower_work_bytes(b, c, C.byref(n)) == BAD_ARG and word in _err() and n.value == 77
    assert _lib().c4_train_tower_work_bytes(5, 32, None) == BAD_ARG and "null" in _err()


def _work(b, c):
    """the work space, exactly c4_train_tower_work_bytes long, between sentinel rows"""
    return Framed(1, work_bytes(b, c) // 4, 0)


# ------------------------------------------------------------------------------------------------------------------ calls
def _conv0(planes, w0, bias, b, c):
    z = Framed(42 * b, c, 0)
    rc = _lib().c4_train_conv0_f32(_p(planes), _p(w0), _p(bias), _p(z.view), b, c, _stream())
    assert rc == 0, _err()
    return z


def _conv(x, w, bias, b, c):
    z = Framed(42 * b, c, 0)
    rc = _lib().c4_train_conv3x3_f32(_p(x), _p(w), _p(bias), _p(z.view), b, c, _stream())
    assert rc == 0, _err()
    return z


def _wgrad(dz, x, b, c, first=False):
    dw, db, work = Framed(c, 32 if first else 9 * c, 0), Framed(1, c, 0), _work(b, c)
    f = _lib().c4_train_conv0_wgrad_f32 if first else _lib().c4_train_conv3x3_wgrad_f32
    rc = f(_p(dz), _p(x), _p(dw.view), _p(db.view), b, c, _p(work.view), _stream())
    assert rc == 0, _err()
    assert work.intact()
    return dw, db


def _bn_fwd(z, a, gamma, beta, b, c):
    y, mean, var, work = Framed(42 * b, c, 0), Framed(1, c, 0), Framed(1, c, 0), _work(b, c)
    rc = _lib().c4_train_bn2d_relu_res_fwd_f32(_p(z), _p(a), _p(gamma), _p(beta), C.c_float(EPS), b, c, _p(y.view), _p(mean.view), _p(var.view),
                                               _p(work.view), _stream())
    assert rc == 0, _err()
    assert work.intact()
    return y, mean, var


def _bn_bwd(dy, z, mean, var, gamma, beta, b, c):
    dz, dgamma, dbeta, work = Framed(42 * b, c, 0), Framed(1, c, 0), Framed(1, c, 0), _work(b, c)
    rc = _lib().c4_train_bn2d_relu_res_bwd_f32(_p(dy), _p(z), _p(mean), _p(var), _p(gamma), _p(beta), C.c_float(EPS), b, c, _p(dz.view),
                                               _p(dgamma.view), _p(dbeta.view), _p(work.view), _stream())
    assert rc == 0, _err()
    assert work.intact()
    return dz, dgamma, dbeta


def _exact(got, want):
    # + 0.0 leaves every value but the sign of a zero as it is
    return np.array_equal((got + np.float32(0)).view(np.int32), (want.astype(np.float32) + np.float32(0)).view(np.int32))


def _within(got, want, s, length):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= _gamma(length) * s).all(), float((err / np.maximum(s, 1e-300)).max() / _gamma(length))
    return float((err / np.maximum(s, 1e-300)).max() / _gamma(length))


# ------------------------------------------------------------------------------------------------------------------ products
@pytest.fixture(scope="module", params=CHANNELS, ids=lambda c: f"C{c}")
def operands(request):
    """planes [32, 2, 6, 7], x and dz [32 * 42, C], w0 [C, 32] (zero from 18 on), w [C, 9 C] and biases: f32 on the host and on the device,
    and small integers; shared and never changed.  A case of B boards takes the first B.  Magnitudes spread over four decades so that S
    is not a constant times the result."""
    c = request.param
    rng = np.random.default_rng(4200 + c)

    def draw(*shape):
        return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(np.float32)

    w0 = draw(c, 32)
    w0[:, 18:] = 0
    host = {"planes": draw(B_MAX, 2, 6, 7), "x": draw(42 * B_MAX, c), "dz": draw(42 * B_MAX, c), "w0": w0, "w": draw(c, 9 * c), "bias": draw(c)}
    ints = {name: rng.integers(-2, 3, a.shape).astype(np.float32) for name, a in host.items()}
    ints["w0"][:, 18:] = 0
    out = {"c": c}
    for tag, arrays in (("host", host), ("ints", ints)):
        arrays["wd"] = ref.flip_for_dgrad(arrays["w"])
        arrays["zero"] = np.zeros(c, dtype=np.float32)
        out[tag] = arrays
        out[tag + "_dev"] = {name: _dev(a) for name, a in arrays.items()}
    return out


def _f64(arrays, b):
    h = {k: v.astype(np.float64) for k, v in arrays.items()}
    h["planes"], h["x"], h["dz"] = h["planes"][:b], h["x"][:42 * b], h["dz"][:42 * b]
    return h


@pytest.mark.parametrize("b", BOARDS)
def test_forward_and_dgrad_are_within_the_dot_product_bound_and_repeat(operands, b):
    c, d, h = operands["c"], operands["host_dev"], _f64(operands["host"], b)
    cols0, cols, cols_dz = ref.im2col0(h["planes"]), ref.im2col3x3(h["x"]), ref.im2col3x3(h["dz"])
    runs = {
        "conv0": (lambda: _conv0(d["planes"], d["w0"], d["bias"], b, c), cols0 @ h["w0"].T + h["bias"], np.abs(cols0) @ np.abs(h["w0"]).T + np.abs(h["bias"]), 18),
        "conv3x3": (lambda: _conv(d["x"], d["w"], d["bias"], b, c), cols @ h["w"].T + h["bias"], np.abs(cols) @ np.abs(h["w"]).T + np.abs(h["bias"]), 9 * c),
        "dgrad": (lambda: _conv(d["dz"], d["wd"], d["zero"], b, c), ref.dgrad(h["dz"], h["w"]), np.abs(cols_dz) @ np.abs(h["wd"]).T, 9 * c),
    }
    for name, (call, want, s, length) in runs.items():
        one, two = call(), call()
        ratio = _within(one.np(), want, s, length)
        assert one.intact() and _same_bytes(one, two), name
        evidence(f"train tower {name} B={b} C={c}: max err / (gamma S) = {ratio:.3f}")


@pytest.mark.parametrize("b", BOARDS)
def test_wgrad_and_db_are_within_the_dot_product_bound_and_repeat(operands, b):
    c, d, h = operands["c"], operands["host_dev"], _f64(operands["host"], b)
    for name, first, x_dev, cols in (("conv3x3", False, d["x"], ref.im2col3x3(h["x"])), ("conv0", True, d["planes"], ref.im2col0(h["planes"]))):
        (dw, db), (dw2, db2) = _wgrad(d["dz"], x_dev, b, c, first), _wgrad(d["dz"], x_dev, b, c, first)
        want_w, want_b = ref.wgrad(h["dz"], cols)
        ratio = _within(dw.np(), want_w, np.abs(h["dz"]).T @ np.abs(cols), 42 * b)
        _within(db.np()[0], want_b, np.abs(h["dz"]).sum(0), 42 * b)
        assert dw.intact() and db.intact() and _same_bytes(dw, dw2) and _same_bytes(db, db2), name
        if first:
            assert np.array_equal(dw.np()[:, 18:].view(np.int32), np.zeros((c, 14), dtype=np.int32))     # +0, selected
        evidence(f"train tower {name} wgrad B={b} C={c}: max err / (gamma S) = {ratio:.3f}")


@pytest.mark.parametrize("b", [3, CHUNK + 1])
def test_products_of_small_integers_are_exact(operands, b):
    """inputs in {-2 .. 2}: every product and partial sum is an integer below 2^24, so any correct order gives the exact result"""
    c, d, h = operands["c"], operands["ints_dev"], _f64(operands["ints"], b)
    assert _exact(_conv0(d["planes"], d["w0"], d["bias"], b, c).np(), ref.conv0(h["planes"], h["w0"], h["bias"]))
    assert _exact(_conv(d["x"], d["w"], d["bias"], b, c).np(), ref.conv3x3(h["x"], h["w"], h["bias"]))
    assert _exact(_conv(d["dz"], d["wd"], d["zero"], b, c).np(), ref.dgrad(h["dz"], h["w"]))
    for first, x_dev, cols in ((False, d["x"], ref.im2col3x3(h["x"])), (True, d["planes"], ref.im2col0(h["planes"]))):
        dw, db = _wgrad(d["dz"], x_dev, b, c, first)
        want_w, want_b = ref.wgrad(h["dz"], cols)
        assert _exact(dw.np(), want_w) and _exact(db.np()[0], want_b), first


@pytest.mark.parametrize("cell", [0, 6, 35, 41, 17], ids=["corner00", "corner06", "corner50", "corner56", "centre23"])
def test_a_single_one_lands_on_exactly_the_restatements_taps(operands, cell):
    """A single 1.0 on the middle board of three, everything else of that operand zero, the other operand distinct integers: a wrong
    halo, an off-by-one row or column, a leak into the neighbouring board or an unflipped dgrad moves or adds an entry."""
    c, b = operands["c"], 3
    row = 42 + cell
    w = (np.arange(c * 9 * c) % 251 + 1).astype(np.float32).reshape(c, 9 * c)                # w[co][tap C + ci]: distinct within a row
    w0 = np.zeros((c, 32), dtype=np.float32)
    w0[:, :18] = (np.arange(c * 18) % 251 + 1).reshape(c, 18)
    pattern = (np.arange(42 * b * c) % 509 + 1).astype(np.float32).reshape(42 * b, c)
    planes_pattern = (np.arange(b * 84) % 83 + 1).astype(np.float32).reshape(b, 2, 6, 7)
    one = np.zeros((42 * b, c), dtype=np.float32)
    one[row, 1] = 1.0
    planes_one = np.zeros((b, 2, 6, 7), dtype=np.float32)
    planes_one[1, 1, cell // 7, cell % 7] = 1.0
    zero = np.zeros(c, dtype=np.float32)
    f = lambda a: a.astype(np.float64)
    got = _conv(_dev(one), _dev(w), _dev(zero), b, c).np()
    assert _exact(got, ref.conv3x3(f(one), f(w), f(zero))) and np.count_nonzero(got) == np.count_nonzero(ref.im2col3x3(f(one))) * c
    got = _conv(_dev(one), _dev(ref.flip_for_dgrad(w)), _dev(zero), b, c).np()
    assert _exact(got, ref.dgrad(f(one), f(w)))
    # the taps by hand: da[cell + offset(tap)][ci] = W[co = 1][tap][ci] where that cell is on the board
    want = np.zeros((b, 6, 7, c))
    for tap in range(9):
        r, q = cell // 7 + tap // 3 - 1, cell % 7 + tap % 3 - 1
        if 0 <= r < 6 and 0 <= q < 7:
            want[1, r, q] = w[1, tap * c:(tap + 1) * c]
    assert _exact(got, want.reshape(42 * b, c))
    got = _conv0(_dev(planes_one), _dev(w0), _dev(zero), b, c).np()
    assert _exact(got, ref.conv0(f(planes_one), f(w0), f(zero))) and np.count_nonzero(got) > 0
    for first, x, cols in ((False, pattern, ref.im2col3x3(f(pattern))), (True, planes_pattern, ref.im2col0(f(planes_pattern)))):
        dw, db = _wgrad(_dev(one), _dev(x), b, c, first)
        want_w, want_b = ref.wgrad(f(one), cols)
        assert _exact(dw.np(), want_w) and _exact(db.np()[0], want_b), first
        assert np.array_equal(dw.np()[1], cols[row].astype(np.float32)) and not np.delete(dw.np(), 1, axis=0).any()


@pytest.mark.parametrize("c,b", CASES, ids=IDS)
def test_conv0_is_the_f32_evaluators_first_convolution_bit_for_bit(c, b):
    rng = np.random.default_rng(c + b)
    planes = _dev(rng.integers(0, 2, (b, 2, 6, 7)).astype(np.float32) * rng.standard_normal((b, 2, 6, 7)).astype(np.float32))
    w0 = rng.standard_normal((c, 32)).astype(np.float32)
    w0[:, 18:] = 0
    w0, bias = _dev(w0), _dev(rng.standard_normal(c).astype(np.float32))
    mine = _conv0(planes, w0, bias, b, c)
    theirs = Framed(42 * b, c, 0)
    rc = _lib().c4_conv_tower_f32(_p(planes), _p(w0), None, _p(bias), b, c, 0, _p(theirs.view), None, _stream())
    assert rc == 0, _err()
    assert mine.intact() and _same_bytes(mine, theirs)


# ------------------------------------------------------------------------------------------------------------------ batch norm
def _bn_case(m, n, seed):
    """z [m, n], a, gamma, beta, dy with the edge columns of tests/test_gpu_train_kernels.py: 0 a constant column (1.25: var = 0, the mean
    exact), 1 gamma = 0, 2 every pre-activation <= 0 (beta = -100), 3 every pre-activation exactly 0 (gamma = beta = 0).  dy is 0 where the
    float64 pre-activation lies within 1e-4 of 0 (column 3 apart): there a rounding error's sign would decide ReLU'."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-1, 1, n) + rng.standard_normal(n) * 3).astype(np.float32)
    a = rng.standard_normal((m, n)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, n).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    beta = (rng.standard_normal(n) * 0.5).astype(np.float32)
    z[:, 0] = 1.25
    gamma[1] = 0.0
    beta[2] = -100.0
    gamma[3] = beta[3] = 0.0
    dy = rng.standard_normal((m, n)).astype(np.float32)
    pre = _bn_ref(z, a, gamma, beta)["pre"]
    near = np.abs(pre) < 1e-4
    near[:, 3] = False
    dy[near] = 0.0
    return z, a, gamma, beta, dy


def _bn_ref(z, a, gamma, beta, dy=None):
    f = lambda t: t.astype(np.float64)
    return ref.bn2d_relu_res(f(z), f(a), f(gamma), f(beta), np.float64(np.float32(EPS)), None if dy is None else f(dy))


@pytest.mark.parametrize("c,b", CASES, ids=IDS)
def test_bn2d_relu_res_forward_and_backward_against_pytorch_f32(c, b):
    m = 42 * b
    z, a, gamma, beta, dy = _bn_case(m, c, 7 * m + c)
    want = _bn_ref(z, a, gamma, beta, dy)
    zd, ad, gd, bd, dyd = _dev(z), _dev(a), _dev(gamma), _dev(beta), _dev(dy)
    # PyTorch's f32 on the same device and inputs
    zt, at, gt, bt = zd.clone().requires_grad_(), ad.clone().requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    rm, rv = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    yt = at + torch.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 1.0, EPS))     # momentum 1: the running statistics are the batch's
    yt.backward(dyd)
    y, mean, var = _bn_fwd(zd, ad, gd, bd, b, c)
    y2, mean2, var2 = _bn_fwd(zd, ad, gd, bd, b, c)
    assert y.intact() and mean.intact() and var.intact() and _same_bytes(y, y2) and _same_bytes(mean, mean2) and _same_bytes(var, var2)
    tag = f"train tower bn B={b} C={c}"
    _judge(tag + " y", y.np(), yt.detach().cpu().numpy(), want["y"])
    _judge(tag + " mean", mean.np()[0], rm.cpu().numpy(), want["mean"])
    _judge(tag + " var", var.np()[0], (rv * ((m - 1) / m)).cpu().numpy(), want["var"])
    assert np.array_equal(var.np()[0, :1], [0.0]) and np.array_equal(mean.np()[0, :1], [1.25])       # the constant column
    dz, dgamma, dbeta = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, b, c)
    dz2, dgamma2, dbeta2 = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, b, c)
    assert dz.intact() and dgamma.intact() and dbeta.intact()
    assert _same_bytes(dz, dz2) and _same_bytes(dgamma, dgamma2) and _same_bytes(dbeta, dbeta2)
    _judge(tag + " dz", dz.np(), zt.grad.cpu().numpy(), want["dz"])
    _judge(tag + " dgamma", dgamma.np()[0], gt.grad.cpu().numpy(), want["dgamma"])
    _judge(tag + " dbeta", dbeta.np()[0], bt.grad.cpu().numpy(), want["dbeta"])
    got = dz.np()
    assert (got[:, 1] == 0).all()                                       # gamma = 0: nothing reaches z
    assert (got[:, 2] == 0).all() and dgamma.np()[0, 2] == 0 and dbeta.np()[0, 2] == 0   # no pre-activation above 0: exactly 0
    assert np.array_equal(y.np()[:, 3], a[:, 3]) and (got[:, 3] == 0).all() and dbeta.np()[0, 3] == 0  # pre-activations of exactly 0: ReLU'(0) = 0


@pytest.mark.parametrize("where", ["first-row", "second-chunk", "last-row"])
def test_a_nan_in_one_column_of_z_stays_in_its_column(where):
    """what tests/test_gpu_train_edges.py asserts for the head kernels: that column's y, dz and dgamma are NaN (a NaN pre-activation
    passes ReLU's predicate !(pre <= 0)), dbeta is the column sum of dy, and no other column changes a byte"""
    c, b, col = 32, CHUNK + 1, 5
    m = 42 * b
    z, a, gamma, beta, dy = _bn_case(m, c, 31)
    poisoned = z.copy()
    poisoned[{"first-row": 0, "second-chunk": 42 * CHUNK + 3, "last-row": m - 1}[where], col] = np.nan
    ad, gd, bd, dyd = _dev(a), _dev(gamma), _dev(beta), _dev(dy)
    out = []
    for zz in (z, poisoned):
        zd = _dev(zz)
        y, mean, var = _bn_fwd(zd, ad, gd, bd, b, c)
        dz, dgamma, dbeta = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, b, c)
        assert all(t.intact() for t in (y, mean, var, dz, dgamma, dbeta))
        out.append([t.np() for t in (y, mean, var, dz, dgamma, dbeta)])
    others = np.arange(c) != col
    for clean, nan in zip(*out):
        assert np.array_equal(clean[:, others].view(np.int32), nan[:, others].view(np.int32))
    y, mean, var, dz, dgamma, dbeta = out[1]
    assert np.isnan(y[:, col]).all() and np.isnan(dz[:, col]).all() and np.isnan(dgamma[0, col]) and np.isnan(mean[0, col]) and np.isnan(var[0, col])
    dy64 = dy[:, col].astype(np.float64)
    assert abs(float(dbeta[0, col]) - dy64.sum()) <= _gamma(m) * np.abs(dy64).sum()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_refused_and_nothing_is_written():
    L, s = _lib(), _stream()
    b, c = 2, 32
    a = torch.zeros((42 * b, 9 * c), dtype=torch.float32, device=DEV)
    v = torch.zeros(64, dtype=torch.float32, device=DEV)
    out, o1, o2, work = Framed(42 * b, 9 * c, 0), Framed(1, 64, 0), Framed(1, 64, 0), _work(b, c)

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == BAD_ARG and word in _err(), (rc, _err())
        assert not out.written() and not o1.written() and not o2.written() and not work.written()

    f = C.c_float(EPS)
    calls = {
        "conv0": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_conv0_f32(x, _p(a), _p(v), z, bb, cc, s),
        "conv3x3": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_conv3x3_f32(x, _p(a), _p(v), z, bb, cc, s),
        "wgrad0": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_conv0_wgrad_f32(_p(a), x, z, _p(o1.view), bb, cc, _p(work.view), s),
        "wgrad": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_conv3x3_wgrad_f32(_p(a), x, z, _p(o1.view), bb, cc, _p(work.view), s),
        "bn_fwd": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_bn2d_relu_res_fwd_f32(x, _p(a), _p(v), _p(v), f, bb, cc, z, _p(o1.view), _p(o2.view),
                                                                                          _p(work.view), s),
        "bn_bwd": lambda x=_p(a), z=_p(out.view), bb=b, cc=c: L.c4_train_bn2d_relu_res_bwd_f32(_p(a), x, _p(v), _p(v), _p(v), _p(v), f, bb, cc, z, _p(o1.view),
                                                                                          _p(o2.view), _p(work.view), s),
    }
    for name, call in calls.items():
        refused(call(cc=24), "channels must be 16, 32, 48 or 64")
        refused(call(cc=80), "channels must be 16, 32, 48 or 64")
        refused(call(bb=0), "n_boards >= 1")
        refused(call(bb=1 << 22), "too large")          # 42 B C = 2^22 * 42 * 32 >= 2^31
        refused(call(x=None), "null")
        if name != "conv0":                       # the planes of the first convolution are read by single floats
            refused(call(x=_p(a, 4)), "aligned")
        refused(call(z=_p(out.view, 4)), "aligned")
    refused(L.c4_train_conv3x3_f32(_p(out.view), _p(a), _p(v), _p(out.view), b, c, s), "z must not be x")
