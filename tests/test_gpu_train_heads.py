"""c4a0_amd.train_heads on the GPU: the autograd Function of one hidden block against the nn.Sequential(Linear, BatchNorm1d, ReLU)
it replaces, and forward_train(heads="hip") against heads="torch" on a whole network.

The judge is the 4 x rule of tests/test_gpu_train_kernels.py: both paths' errors are taken against the same computation in float64
on the CPU, and the HIP path's largest may be at most 4 x PyTorch's f32 one (floor 4 * 2^-24 * max |ref|)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_heads import forward_train, hidden_block
from tests import train_recipe as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
F_SIZE = 672


def _judge(what, hip, stock, ref):
    ref = ref.detach().cpu().double().numpy()
    e_k = float(np.abs(hip.detach().cpu().double().numpy() - ref).max())
    e_t = float(np.abs(stock.detach().cpu().double().numpy() - ref).max())
    floor = 4 * U * float(np.abs(ref).max())
    evidence(f"{what}: hip err {e_k:.3e}, PyTorch f32 err {e_t:.3e}, ratio {e_k / e_t if e_t else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


def _block(seed: int):
    torch.manual_seed(seed)
    block = nn.Sequential(nn.Linear(F_SIZE, F_SIZE), nn.BatchNorm1d(F_SIZE), nn.ReLU())
    with torch.no_grad():      # statistics and affine parameters away from their initial 0 / 1
        block[1].weight.uniform_(0.5, 1.5)
        block[1].bias.normal_(0, 0.3)
        block[1].running_mean.normal_(0, 0.2)
        block[1].running_var.uniform_(0.5, 2.0)
        block[1].num_batches_tracked.fill_(5)
    return block


@pytest.mark.parametrize("m", [2, 17, 130])
def test_the_function_equals_the_triple_it_replaces(m):
    truth = _block(m).double().train()
    stock, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    torch.manual_seed(100 + m)
    x64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    dy64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    xs = []
    for block, dtype, dev in ((truth, torch.float64, "cpu"), (stock, torch.float32, DEV), (hip, torch.float32, DEV)):
        x = x64.clone().to(device=dev, dtype=dtype).requires_grad_()
        y = hidden_block(block, x) if block is hip else block(x)
        y.backward(dy64.to(device=dev, dtype=dtype))
        xs.append((x, y))
    tag = f"hidden block m={m}"
    _judge(tag + " y", xs[2][1], xs[1][1], xs[0][1])
    _judge(tag + " dx", xs[2][0].grad, xs[1][0].grad, xs[0][0].grad)
    for name in ("0.weight", "0.bias", "1.weight", "1.bias"):
        p = {k: dict(b.named_parameters())[name].grad for k, b in (("truth", truth), ("stock", stock), ("hip", hip))}
        _judge(f"{tag} d({name})", p["hip"], p["stock"], p["truth"])
    for name in ("running_mean", "running_var"):
        _judge(f"{tag} {name}", getattr(hip[1], name), getattr(stock[1], name), getattr(truth[1], name))
    assert int(hip[1].num_batches_tracked) == int(stock[1].num_batches_tracked) == 6


def _three_blocks(seed: int):
    truth = _block(seed).double().train()
    return truth, copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)


def _judge_blocks(tag, truth, stock, hip):
    for name in ("0.weight", "0.bias", "1.weight", "1.bias"):
        p = {k: dict(b.named_parameters())[name].grad for k, b in (("truth", truth), ("stock", stock), ("hip", hip))}
        _judge(f"{tag} d({name})", p["hip"], p["stock"], p["truth"])
    for name in ("running_mean", "running_var"):
        _judge(f"{tag} {name}", getattr(hip[1], name), getattr(stock[1], name), getattr(truth[1], name))
    assert int(hip[1].num_batches_tracked) == int(stock[1].num_batches_tracked) == 6


@pytest.mark.parametrize("first, copied", [(F_SIZE, False), (1, True)], ids=["row-view", "misaligned-copy"])
def test_the_function_reads_a_column_range_of_a_wider_leaf(first, copied):
    """x = wide[:, first : first + 672] of a [17, 2016] leaf.  At first = 672 it is a 16-byte aligned row view of stride 2016: the
    Function saves the view itself and wgrad reads it with that stride.  At first = 1 it is 4 bytes past a boundary and a dense copy
    is made.  Either way the triple's y, parameter gradients and statistics, and the gradient lands in that column range of wide.grad."""
    m = 17
    truth, stock, hip = _three_blocks(m)
    torch.manual_seed(200 + first)
    wide64 = torch.randn(m, 3 * F_SIZE, dtype=torch.float64)
    dy64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    runs = []
    for block, dtype, dev in ((truth, torch.float64, "cpu"), (stock, torch.float32, DEV), (hip, torch.float32, DEV)):
        wide = wide64.clone().to(device=dev, dtype=dtype).requires_grad_()
        x = wide[:, first:first + F_SIZE]
        y = hidden_block(block, x) if block is hip else block(x)
        if block is hip:
            saved = y.grad_fn.saved_tensors[0]
            assert type(y.grad_fn).__name__ == "HiddenBlockFunctionBackward" and saved.shape == x.shape
            if copied:
                assert x.data_ptr() % 16 == 4 and saved.data_ptr() != x.data_ptr() and saved.stride() == (F_SIZE, 1)
            else:
                assert x.data_ptr() % 16 == 0 and saved.data_ptr() == x.data_ptr() and saved.stride() == x.stride() == (3 * F_SIZE, 1)
        y.backward(dy64.to(device=dev, dtype=dtype))
        runs.append((wide, y))
    tag = f"hidden block m={m} x=wide[:, {first}:{first + F_SIZE}]"
    _judge(tag + " y", runs[2][1], runs[1][1], runs[0][1])
    grads = [w.grad[:, first:first + F_SIZE] for w, _ in runs]
    _judge(tag + " dx", grads[2], grads[1], grads[0])
    outside = runs[2][0].grad.clone()
    outside[:, first:first + F_SIZE] = 0
    assert not outside.any()
    _judge_blocks(tag, truth, stock, hip)


def test_the_function_takes_a_broadcast_dy():
    """y.sum().backward(): dy is one element seen through strides (0, 0)"""
    m = 17
    truth, stock, hip = _three_blocks(m)
    torch.manual_seed(300)
    x64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    runs = []
    for block, dtype, dev in ((truth, torch.float64, "cpu"), (stock, torch.float32, DEV), (hip, torch.float32, DEV)):
        x = x64.clone().to(device=dev, dtype=dtype).requires_grad_()
        y = hidden_block(block, x) if block is hip else block(x)
        y.sum().backward()
        runs.append((x, y))
    tag = f"hidden block m={m} dy broadcast"
    _judge(tag + " y", runs[2][1], runs[1][1], runs[0][1])
    _judge(tag + " dx", runs[2][0].grad, runs[1][0].grad, runs[0][0].grad)
    _judge_blocks(tag, truth, stock, hip)


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


def test_an_input_that_needs_no_gradient_skips_dgrad(monkeypatch):
    """x without requires_grad: c4_train_linear_dgrad_f32 is not called, and the four parameter gradients are the bytes of the run
    whose x requires grad"""
    from c4a0_amd import train_heads

    m = 17
    with_dx, without = copy.deepcopy(_block(m)).to(DEV).train(), copy.deepcopy(_block(m)).to(DEV).train()
    torch.manual_seed(400)
    x, dy = torch.randn(m, F_SIZE, device=DEV), torch.randn(m, F_SIZE, device=DEV)
    counting = _CountingLib(train_heads.lib())
    monkeypatch.setattr(train_heads, "lib", lambda: counting)
    xg = x.clone().requires_grad_()
    hidden_block(with_dx, xg).backward(dy)
    assert counting.calls.count("c4_train_linear_dgrad_f32") == 1 and counting.calls.count("c4_train_linear_wgrad_f32") == 1
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())
    del counting.calls[:]
    y = hidden_block(without, x.clone())
    y.backward(dy)
    assert counting.calls == ["c4_linear_f32", "c4_train_bn_relu_fwd_f32", "c4_train_bn_relu_bwd_f32", "c4_train_linear_wgrad_f32"]
    for (name, p), q in zip(with_dx.named_parameters(), without.parameters()):
        assert q.grad is not None and torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)), name


def test_a_second_backward_doubles_every_gradient():
    """backward(retain_graph=True) twice: the kernels give the same bytes again, so every accumulated gradient is exactly 2 x the first"""
    m = 17
    block = _block(m).to(DEV).train()
    torch.manual_seed(500)
    x, dy = torch.randn(m, F_SIZE, device=DEV).requires_grad_(), torch.randn(m, F_SIZE, device=DEV)
    y = hidden_block(block, x)
    y.backward(dy, retain_graph=True)
    first = [t.grad.clone() for t in (x, *block.parameters())]
    y.backward(dy)
    for one, t in zip(first, (x, *block.parameters())):
        assert bool(one.any()) and torch.equal(t.grad.view(torch.int32), (2 * one).view(torch.int32))
    assert int(block[1].num_batches_tracked) == 6       # the statistics moved once, in the forward


def test_a_nan_in_the_batch_shows_in_the_loss_on_both_paths():
    """One NaN cell in the planes of a batch of 8: the tower's batch norm spreads it over the batch, and heads="hip" must show it
    exactly as heads="torch" does -- a NaN loss, non-finite gradients of the hidden Linear weights -- and not train on zeros."""
    torch.manual_seed(6)
    stock = ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).train()
    hip = copy.deepcopy(stock)
    rng = np.random.default_rng(6)
    planes = R.planes(8, rng)
    planes[3, 1, 2, 4] = float("nan")
    target = torch.from_numpy(rng.dirichlet(np.ones(7), 8).astype(np.float32))
    q = torch.from_numpy(rng.uniform(-1, 1, (2, 8)).astype(np.float32))
    batch = tuple(t.to(DEV) for t in (planes, target, q[0], q[1]))
    losses = {}
    for name, model in (("torch", stock), ("hip", hip)):
        losses[name] = T.loss(forward_train(model, batch[0], name), batch)[0]
        losses[name].backward()
    evidence(f"forward_train, one NaN plane cell: loss {float(losses['hip'].detach())} with heads=hip, {float(losses['torch'].detach())} with heads=torch")
    assert bool(torch.isnan(losses["hip"])) == bool(torch.isnan(losses["torch"]))
    for model in (stock, hip):
        hidden = [layer[0] for head in (model.fc_policy, model.fc_value) for layer in head if isinstance(layer, nn.Sequential)]
        assert len(hidden) == 2
        for lin in hidden:
            assert lin.weight.grad is not None and not bool(torch.isfinite(lin.weight.grad).all())


def test_the_eval_mode_path_is_the_modules():
    block = _block(1).to(DEV).eval()
    x = torch.randn(5, F_SIZE, device=DEV)
    before = {k: v.clone() for k, v in block.state_dict().items()}
    assert torch.equal(hidden_block(block, x), block(x))
    assert all(torch.equal(v, before[k]) for k, v in block.state_dict().items())
    # ... and a whole network in eval mode takes the module forward under heads="auto"
    model = ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).eval()
    planes = R.planes(3, np.random.default_rng(0)).to(DEV)
    for a, b in zip(forward_train(model, planes, "auto"), model(planes)):
        assert torch.equal(a, b)


def test_one_row_is_refused_like_batchnorm_refuses_it():
    block = _block(1).to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hidden_block(block, torch.randn(1, F_SIZE, device=DEV))


def test_forward_train_hip_equals_torch_on_a_whole_network():
    torch.manual_seed(4)
    truth = ConnectFourNet(ModelConfig(1, 16, 3, 2)).double().train()
    stock, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    rng = np.random.default_rng(4)
    planes = R.planes(64, rng)
    target = torch.from_numpy(rng.dirichlet(np.ones(7), 64).astype(np.float32))
    q = torch.from_numpy(rng.uniform(-1, 1, (2, 64)).astype(np.float32))
    losses = {}
    for name, model, dtype, dev, heads in (("truth", truth, torch.float64, "cpu", "torch"), ("stock", stock, torch.float32, DEV, "torch"),
                                           ("hip", hip, torch.float32, DEV, "hip")):
        batch = tuple(t.to(device=dev, dtype=dtype) for t in (planes, target, q[0], q[1]))
        losses[name] = T.loss(forward_train(model, batch[0], heads), batch)[0]
        losses[name].backward()
    _judge("forward_train loss", losses["hip"], losses["stock"], losses["truth"])
    grads = {name: dict(model.named_parameters()) for name, model in (("truth", truth), ("stock", stock), ("hip", hip))}
    for name, p in grads["truth"].items():      # the conv gradients carry the summed dx of the two heads through the tower
        assert grads["hip"][name].grad is not None, name
        _judge(f"forward_train d({name})", grads["hip"][name].grad, grads["stock"][name].grad, p.grad)
    for name, buf in truth.named_buffers():
        if buf.dtype.is_floating_point:
            _judge(f"forward_train {name}", dict(hip.named_buffers())[name], dict(stock.named_buffers())[name], buf)


def test_heads_hip_refuses_by_name():
    planes = R.planes(4, np.random.default_rng(0))
    with pytest.raises(ValueError, match="not a multiple of 16"):
        forward_train(ConnectFourNet(ModelConfig(1, 8, 2, 2)).to(DEV).train(), planes.to(DEV), "hip")
    with pytest.raises(ValueError, match="the kernels are f32"):
        forward_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).double().to(DEV).train(), planes.double().to(DEV), "hip")
    with pytest.raises(ValueError, match="not on a HIP device"):
        forward_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).train(), planes, "hip")
    with pytest.raises(ValueError, match="eval mode"):
        forward_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).eval(), planes.to(DEV), "hip")
    # "auto" takes the module forward in each of these cases
    model = ConnectFourNet(ModelConfig(1, 8, 2, 2)).to(DEV).train()
    assert forward_train(model, planes.to(DEV), "auto")[0].shape == (4, 7)
