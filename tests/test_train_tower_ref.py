"""tests/train_tower_ref.py -- the float64 restatement the GPU tests hold the training tower's kernels to -- pinned to float64
F.conv2d / F.batch_norm(training=True) and their autograd on the CPU at 1e-12; `resolve_tower` on a CPU model; and
fit(..., tower="torch") against fit(...) byte for byte.  No GPU."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from c4a0_amd import train_tower as TT
from c4a0_amd import training as T
from c4a0_amd.train_heads import forward_train
from tests import train_recipe as R
from tests import train_tower_ref as ref

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))


def t64(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("b,c", [(1, 16), (3, 32), (5, 48)])
def test_convolutions_and_their_gradients_equal_float64_conv2d(b, c):
    rng = np.random.default_rng(100 * b + c)
    planes = rng.standard_normal((b, 2, 6, 7))
    w0, b0 = rng.standard_normal((c, 2, 3, 3)), rng.standard_normal(c)
    w1, b1 = rng.standard_normal((c, c, 3, 3)), rng.standard_normal(c)
    # forward
    pt, w0t, b0t, w1t, b1t = t64(planes), t64(w0, True), t64(b0, True), t64(w1, True), t64(b1, True)
    z0t = F.conv2d(pt, w0t, b0t, padding=1)
    z0t.retain_grad()
    z1t = F.conv2d(z0t, w1t, b1t, padding=1)
    z0 = ref.conv0(planes, ref.pack_conv0(w0), b0)
    z1 = ref.conv3x3(z0, ref.pack_conv3x3(w1), b1)
    assert close(ref.to_nchw(z0), z0t.detach().numpy()) and close(ref.to_nchw(z1), z1t.detach().numpy())
    # backward from a random dz1
    dz1 = rng.standard_normal(z1.shape)
    z1t.backward(t64(ref.to_nchw(dz1)))
    dz0 = ref.dgrad(dz1, ref.pack_conv3x3(w1))
    assert close(ref.to_nchw(dz0), z0t.grad.numpy())
    dw1, db1 = ref.wgrad(dz1, ref.im2col3x3(z0))
    assert close(ref.unpack_conv3x3(dw1), w1t.grad.numpy()) and close(db1, b1t.grad.numpy())
    dw0, db0 = ref.wgrad(dz0, ref.im2col0(planes))
    assert close(ref.unpack_conv0(dw0), w0t.grad.numpy()) and close(db0, b0t.grad.numpy())
    assert not dw0[:, 18:].any()
    # the packing round trip, and the package's own packing functions say the same
    assert np.array_equal(ref.unpack_conv3x3(ref.pack_conv3x3(w1)), w1) and np.array_equal(ref.unpack_conv0(ref.pack_conv0(w0)), w0)
    assert np.array_equal(TT.pack_conv0(t64(w0)).numpy(), ref.pack_conv0(w0))
    assert np.array_equal(TT.pack_conv3x3(t64(w1)).numpy(), ref.pack_conv3x3(w1))
    assert np.array_equal(TT.pack_conv3x3_dgrad(t64(w1)).numpy(), ref.flip_for_dgrad(ref.pack_conv3x3(w1)))
    assert np.array_equal(TT.unpack_conv3x3(t64(dw1)).numpy(), ref.unpack_conv3x3(dw1)) and np.array_equal(TT.unpack_conv0(t64(dw0)).numpy(), ref.unpack_conv0(dw0))


def test_a_single_one_lands_on_the_taps_the_layout_says():
    """x = 1 at one cell, channel 0, and W[co][tap][0] = 10 co + tap + 1: z[cell - offset(tap)][co] is that weight, nothing else is set"""
    c = 16
    w = np.zeros((c, c, 3, 3))
    w[:, 0] = (10 * np.arange(c)[:, None] + np.arange(9)[None, :] + 1).reshape(c, 3, 3)
    for row, col in ((0, 0), (0, 6), (5, 0), (5, 6), (2, 3)):
        x = np.zeros((42, c))
        x[7 * row + col, 0] = 1.0
        z = ref.conv3x3(x, ref.pack_conv3x3(w), np.zeros(c)).reshape(6, 7, c)
        want = np.zeros((6, 7, c))
        for tap in range(9):
            r, q = row - (tap // 3 - 1), col - (tap % 3 - 1)
            if 0 <= r < 6 and 0 <= q < 7:
                want[r, q] = 10 * np.arange(c) + tap + 1
        assert np.array_equal(z, want), (row, col)


@pytest.mark.parametrize("b,c", [(1, 16), (4, 32)])
def test_batch_norm_relu_residual_equals_float64_batch_norm(b, c):
    rng = np.random.default_rng(7 * b + c)
    m = 42 * b
    z, a, dy = rng.standard_normal((m, c)) * 3 + 1, rng.standard_normal((m, c)), rng.standard_normal((m, c))
    gamma, beta = rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c), rng.standard_normal(c) * 0.5
    eps = 1e-5
    zt, at, gt, bt = t64(ref.to_nchw(z), True), t64(ref.to_nchw(a), True), t64(gamma, True), t64(beta, True)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    yt = at + torch.relu(F.batch_norm(zt, rm, rv, gt, bt, True, 1.0, eps))
    yt.backward(t64(ref.to_nchw(dy)))
    out = ref.bn2d_relu_res(z, a, gamma, beta, eps, dy)
    assert close(ref.to_nchw(out["y"]), yt.detach().numpy())
    assert close(out["mean"], rm.numpy()) and close(out["var"] * (m / (m - 1.0)), rv.numpy())
    assert close(ref.to_nchw(out["dz"]), zt.grad.numpy()) and close(out["dgamma"], gt.grad.numpy()) and close(out["dbeta"], bt.grad.numpy())
    assert close(ref.to_nchw(dy), at.grad.numpy())


def test_resolve_tower_on_a_cpu_model():
    model = R.problem()[0].train()
    planes = torch.zeros(4, 2, 6, 7)
    assert TT.TOWERS == ("auto", "hip", "torch")
    assert TT.resolve_tower(model, "auto", planes) == "torch" and TT.resolve_tower(model, "torch", planes) == "torch"
    assert TT.resolve_tower(model) == "torch"
    assert "not on a HIP device" in TT.tower_refusal(model, planes)
    with pytest.raises(ValueError, match='tower="hip": the model is on cpu, not on a HIP device'):
        TT.resolve_tower(model, "hip", planes)
    with pytest.raises(ValueError, match='tower="hip"'):
        forward_train(model, planes, heads="torch", tower="hip")
    with pytest.raises(ValueError, match="tower must be one of"):
        TT.resolve_tower(model, "cuda", planes)
    # the default and "torch" are the module's own forward
    torch.manual_seed(0)
    planes = R.planes(8, np.random.default_rng(0))
    a = forward_train(copy.deepcopy(model), planes)
    b = forward_train(copy.deepcopy(model), planes, heads="auto", tower="torch")
    c = copy.deepcopy(model)(planes)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_fit_with_the_stock_tower_is_fit():
    runs = []
    for kwargs in ({}, {"tower": "torch"}, {"tower": "auto"}):
        student, train, val = R.problem()
        train, val = tuple(t[:200] for t in train), tuple(t[:64] for t in val)
        _best, best_val, history = T.fit(student, train, val, 64, 1, R.TRAIN_CONFIG, seed=5, max_epochs=2, **kwargs)
        runs.append((student.state_dict(), best_val, history))
    for state, best_val, history in runs[1:]:
        assert best_val == runs[0][1] and history == runs[0][2]
        assert all(torch.equal(v, runs[0][0][k]) for k, v in state.items())
