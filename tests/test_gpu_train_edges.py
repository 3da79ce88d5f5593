"""The training kernels (c4a0_amd/csrc/c4_train.hip) where tests/test_gpu_train_kernels.py does not look, with its helpers and rules:

* the 16-wide product kernels (k an odd multiple of 16) give the bits of the 32-wide ones on the same columns;
* non-finite values in the rows the products read a second time -- row m - 1, which stands in for the rows past the batch, and the
  first block, which the last trip prefetches again -- reach exactly the elements they reach in float64, and a row past m is never read
  into a result;
* a column of z that holds a NaN, an infinity or a sum that overflows leaves the batch-norm kernels as PyTorch's f32
  relu(F.batch_norm(training=True)) leaves it on the same device -- NaN in y, dz and dgamma, ReLU's predicate being !(pre <= 0) -- and
  reaches no other column.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import evidence
from tests.test_gpu_train_kernels import DEV, EPS, _bn_bwd, _bn_case, _bn_fwd, _dev, _dgrad, _gamma, _judge, _same_bytes, _wgrad

pytestmark = pytest.mark.gpu


def _draw(rng, *shape):
    """the magnitudes of test_gpu_train_kernels.operands: four decades, so that S is not a constant times the result"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2, 2, shape)).astype(np.float32)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ 16-wide == 32-wide
@pytest.fixture(scope="module")
def wide64():
    """dz [130, 64], x [130, 64], w [64, 64] on the device; shared and never changed"""
    rng = np.random.default_rng(6464)
    return {"dz": _dev(_draw(rng, 130, 64)), "x": _dev(_draw(rng, 130, 64)), "w": _dev(_draw(rng, 64, 64))}


@pytest.mark.parametrize("k", [48, 16])
@pytest.mark.parametrize("m", [3, 130])
def test_the_16_wide_kernels_give_the_bits_of_the_32_wide_ones(wide64, m, k):
    """k = 64 runs train_dgrad<2, 2> and train_wgrad<2, 2>, k = 48 and 16 run <1, 2> and <2, 1>: an element's chain is the same, so
    the first k columns are the same bytes.  wgrad reads x[:, :k] as a row view of the 64-wide x (ldx = 64)."""
    n, d = 64, wide64
    full = _dgrad(d["dz"], d["w"], m, n, 64)
    part = _dgrad(d["dz"], d["w"][:, :k].contiguous(), m, n, k)
    assert full.intact() and part.intact() and bool(torch.isfinite(part.view).all())
    assert torch.equal(_bits(part.view), _bits(full.view[:, :k]))
    (dw, db), (dwk, dbk) = _wgrad(d["dz"], d["x"], m, n, 64), _wgrad(d["dz"], d["x"][:, :k], m, n, k)
    assert d["x"][:, :k].stride(0) == 64 and dw.intact() and db.intact() and dwk.intact() and dbk.intact()
    assert torch.equal(_bits(dwk.view), _bits(dw.view[:, :k])) and _same_bytes(db, dbk)


# ------------------------------------------------------------------------------------------------------------------ poison in re-read rows
NAN, INF = float("nan"), float("inf")
# name -> cells of dz and of x as (row, column), row -1 = m - 1 and column None = the whole row, and the value
POISON = {
    "nan-last-row": ([(-1, None)], [(-1, None)], NAN),      # the row that stands in for the rows past the batch
    "nan-first-row": ([(0, None)], [(0, None)], NAN),       # the block the last trip prefetches again
    "nan-x-cell-last-row": ([], [(-1, 5)], NAN),            # spoils column 5 of dw and nothing else
    "nan-x-cell-first-row": ([], [(0, 5)], NAN),
    "inf-dz-cell-last-row": ([(-1, 3)], [], INF),           # an infinity times a zero made by multiplying would be NaN
    "inf-x-cell-last-row": ([], [(-1, 5)], INF),
}


def _poisoned(a: np.ndarray, m: int, cells, value) -> np.ndarray:
    a = a[:m].copy()
    for row, col in cells:
        a[row % m, slice(None) if col is None else col] = value
    return a


def _within(what, got, a64, b64, length):
    """got against a64 @ b64 in float64: NaN exactly where that is NaN, the same infinity where it is one, and elsewhere within
    gamma(length) S, S from the finite terms alone (no other term enters such an element)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ref = a64 @ b64
    s = np.abs(np.where(np.isfinite(a64), a64, 0.0)) @ np.abs(np.where(np.isfinite(b64), b64, 0.0))
    nan, inf = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), nan), (what, int(np.isnan(got).sum()), int(nan.sum()))
    assert np.array_equal(got[inf].astype(np.float64), ref[inf]), what
    fin = ~nan & ~inf
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    assert (err <= _gamma(length) * s[fin]).all(), (what, float((err / s[fin]).max() / _gamma(length)))
    return int(nan.sum()), int(inf.sum()), float((err / np.maximum(s[fin], 1e-300)).max() / _gamma(length)) if fin.any() else 0.0


@pytest.fixture(scope="module", params=[(32, 32), (64, 48)], ids=lambda s: f"N{s[0]}-K{s[1]}")
def clean(request):
    n, k = request.param
    rng = np.random.default_rng(77 * n + k)
    return {"n": n, "k": k, "dz": _draw(rng, 131, n), "x": _draw(rng, 131, k), "w": _draw(rng, n, k)}      # 130 rows and one to spare


@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("m", [17, 130])
def test_poison_in_the_rows_read_twice_goes_where_float64_takes_it(clean, m, poison):
    n, k = clean["n"], clean["k"]
    dz_cells, x_cells, value = POISON[poison]
    dz, x, w = _poisoned(clean["dz"], m, dz_cells, value), _poisoned(clean["x"], m, x_cells, value), clean["w"]
    dz64, x64, w64 = dz.astype(np.float64), x.astype(np.float64), w.astype(np.float64)
    dzd, xd, wd = _dev(dz), _dev(x), _dev(w)
    dx = _dgrad(dzd, wd, m, n, k)
    dw, db = _wgrad(dzd, xd, m, n, k)
    assert dx.intact() and dw.intact() and db.intact()
    tag = f"train products m={m} n={n} k={k} {poison}"
    counts = [_within(tag + " dx", dx.np(), dz64, w64, n), _within(tag + " dw", dw.np(), dz64.T, x64, m),
              _within(tag + " db", db.np(), np.ones((1, m)), dz64, m)]
    # what the variant is there for: only the poisoned rows of dx, only the poisoned column of dw
    rows = sorted({r % m for r, _c in dz_cells})
    assert np.array_equal(np.flatnonzero(~np.isfinite(dx.np()).all(1)), rows)
    if not dz_cells:
        assert np.array_equal(np.flatnonzero(~np.isfinite(dw.np()).all(0)), [5]) and np.isfinite(db.np()).all()
    evidence(f"{tag}: (NaN, inf, max err / (gamma S)) dx {counts[0][0]}, {counts[0][1]}, {counts[0][2]:.3f}; "
             f"dw {counts[1][0]}, {counts[1][1]}, {counts[1][2]:.3f}; db {counts[2][0]}, {counts[2][1]}, {counts[2][2]:.3f}")


@pytest.mark.parametrize("m", [17, 130])
def test_the_row_after_the_batch_is_never_read_into_a_result(clean, m):
    """m + 1 rows allocated, m passed: the bytes with NaN in the extra row are the bytes with zeros in it"""
    n, k = clean["n"], clean["k"]
    wd, outs = _dev(clean["w"]), []
    for extra in (0.0, NAN):
        dz, x = clean["dz"][:m + 1].copy(), clean["x"][:m + 1].copy()
        dz[m], x[m] = extra, extra
        dzd, xd = _dev(dz), _dev(x)
        outs.append((_dgrad(dzd, wd, m, n, k), *_wgrad(dzd, xd, m, n, k)))
    for zeros, nans in zip(*outs):
        assert nans.intact() and _same_bytes(zeros, nans) and bool(torch.isfinite(nans.view).all())


# ------------------------------------------------------------------------------------------------------------------ non-finite columns
def _classes(a) -> np.ndarray:
    """0 NaN, 1 +inf, 2 -inf, 3 finite"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 0, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 3)))


@pytest.mark.parametrize("m, n", [(17, 32), (130, 672)])
def test_bn_relu_keeps_a_non_finite_column_non_finite_and_to_itself(m, n):
    """Four columns of a _bn_case are poisoned in single cells: a NaN in row 0, +inf in row m - 1, -inf in row m - 1, and 3e38 in rows
    0 and m - 1 (their sum overflows).  By IEEE arithmetic on the definition (mean = sum / m, var = mean of squared deviations) their
    (mean, var) are (NaN, NaN), (+inf, NaN), (-inf, NaN), (+inf, +inf), so every pre-activation is NaN, and NaN passes ReLU, whose
    predicate is !(pre <= 0): y, dz and dgamma are NaN, and dbeta, where dy passes the mask, is the plain column sum of dy.  That is
    what PyTorch's f32 relu(F.batch_norm(training=True)) and its autograd give on the same device, to which the kernels are held.
    The cells: PyTorch's device kernel updates a running mean row by row (Welford), where an infinite mean turns
    NaN at the next row a thread visits ((-inf) - (-inf)); with the infinities in the last row, and the two 3e38 in the first and the
    last, its statistics have the classes of the definition (observed on an MI355X; elsewhere its mean of the -inf column is NaN and
    its variance of the 3e38 column is NaN for most pairs of rows).
    Every other column is the same bytes as without the poison: nothing crosses the shared LDS reduction."""
    z, gamma, beta, dy = _bn_case(m, n, 11 * m + n)
    cols = [5, n - 23, 14, n - 12]                                   # one workgroup's at n = 32, two at n = 672; none of the edge columns 0..3
    bad = z.copy()
    bad[0, cols[0]] = NAN
    bad[m - 1, cols[1]] = INF
    bad[m - 1, cols[2]] = -INF
    bad[0, cols[3]] = bad[m - 1, cols[3]] = 3e38
    others = np.setdiff1d(np.arange(n), cols)
    gd, bd, dyd = _dev(gamma), _dev(beta), _dev(dy)
    runs = {}
    for name, zz in (("clean", z), ("bad", bad)):
        zd = _dev(zz)
        y, mean, var = _bn_fwd(zd, gd, bd, m, n)
        dz, dgamma, dbeta = _bn_bwd(dyd, zd, mean.view[0], var.view[0], gd, bd, m, n)
        assert all(f.intact() for f in (y, mean, var, dz, dgamma, dbeta))
        runs[name] = {"y": y.np(), "mean": mean.np()[0], "var": var.np()[0], "dz": dz.np(), "dgamma": dgamma.np()[0], "dbeta": dbeta.np()[0]}
    # PyTorch's f32 on the same device and inputs
    zt, gt, bt = _dev(bad).requires_grad_(), gd.clone().requires_grad_(), bd.clone().requires_grad_()
    rm, rv = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    yt = torch.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 1.0, EPS))     # momentum 1: the running statistics are the batch's
    yt.backward(dyd)
    got, tag = runs["bad"], f"train bn m={m} n={n} poisoned"
    t_mean, t_var, t_dbeta = rm.cpu().numpy()[cols], rv.cpu().numpy()[cols], bt.grad.cpu().numpy()[cols]
    evidence(f"{tag} columns {cols}: mean {got['mean'][cols]} (PyTorch {t_mean}), var {got['var'][cols]} (PyTorch {t_var}), "
             f"NaN of {m} in y {np.isnan(got['y'][:, cols]).sum(0)}, in dz {np.isnan(got['dz'][:, cols]).sum(0)}, dgamma {got['dgamma'][cols]}, "
             f"dbeta {got['dbeta'][cols]} (PyTorch {t_dbeta})")
    assert bool(yt[:, cols].isnan().all()) and bool(zt.grad[:, cols].isnan().all()) and bool(gt.grad[cols].isnan().all())     # the reference
    assert np.isnan(got["y"][:, cols]).all()
    assert np.isnan(got["dz"][:, cols]).all()
    assert np.isnan(got["dgamma"][cols]).all()
    assert not np.isfinite(got["mean"][cols]).any() and not np.isfinite(got["var"][cols]).any()
    assert np.array_equal(_classes(got["mean"][cols]), _classes(t_mean)) and np.array_equal(_classes(got["var"][cols]), _classes(t_var))
    assert _classes(got["mean"][cols]).tolist() == [0, 1, 2, 1] and _classes(got["var"][cols]).tolist() == [0, 0, 0, 1]   # the definition's
    nan = np.isnan(t_dbeta)
    assert np.isnan(got["dbeta"][cols][nan]).all()
    if (~nan).any():
        _judge(tag + " dbeta", got["dbeta"][cols][~nan], t_dbeta[~nan], dy.astype(np.float64).sum(0)[cols][~nan])
    for name, a in got.items():
        assert np.array_equal(a[..., others].view(np.int32), runs["clean"][name][..., others].view(np.int32)), name
        assert np.isfinite(a[..., others]).all(), name
