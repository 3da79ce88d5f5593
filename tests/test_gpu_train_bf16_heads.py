"""heads="bf16" on the GPU: HiddenBlockBf16Function and forward_train(heads="bf16") against float64, judged beside a stock-PyTorch
emulation with the same rounding points; how the blocks chain and what is launched; the refusals; and the learning recipe.

Truth is float64 on the CPU with no rounding at all.  The comparator is the block in stock PyTorch on the GPU, rounded where the
contract rounds: x.bfloat16(), F.linear on bf16 tensors, F.batch_norm(z.float(), training=True), relu, .bfloat16(), backward through
autograd.  For every output the bf16 path's largest error against truth may be at most 4 x the emulation's, with a floor of
2^-8 * max |truth| (two roundings of the largest element)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_heads import forward_train, hidden_block, resolve_heads
from c4a0_amd.training import TrainConfig, evaluate_loss, fit
from tests import train_recipe as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F_SIZE = 1344
BF16_LAUNCHES_FIRST = ["c4_train_cast_bf16", "c4_train_cast_bf16", "c4_linear_bf16", "c4_train_bn_relu_fwd_bf16"]      # x, W, z, y


def _judge(what, got, emu, truth):
    truth = truth.detach().cpu().double().numpy()
    e_k = float(np.abs(got.detach().cpu().double().numpy() - truth).max())
    e_e = float(np.abs(emu.detach().cpu().double().numpy() - truth).max())
    floor = 2.0 ** -8 * float(np.abs(truth).max())
    evidence(f"{what}: bf16 path err {e_k:.3e}, emulation err {e_e:.3e}, ratio {e_k / e_e if e_e else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_e, floor), (what, e_k, e_e, floor)


def emulated_block(block: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """the hidden triple in stock PyTorch with the contract's rounding points; moves the running statistics as the module does"""
    lin, bn = block[0], block[1]
    z = F.linear(x.bfloat16(), lin.weight.bfloat16(), lin.bias.bfloat16())
    bn.num_batches_tracked += 1
    return torch.relu(F.batch_norm(z.float(), bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)).bfloat16()


def emulated_forward(model: nn.Module, planes: torch.Tensor):
    def head(seq, x):
        for layer in seq:
            x = emulated_block(layer, x) if isinstance(layer, nn.Sequential) else layer(x.float())
        return x

    x = model.conv(planes)
    x = x.reshape(x.shape[0], -1)
    q = head(model.fc_value, x)
    return head(model.fc_policy, x), q[:, 0], q[:, 1]


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
def test_the_function_against_float64_beside_the_emulation(m):
    truth = _block(m).double().train()
    emu, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    torch.manual_seed(100 + m)
    x64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    dy64 = torch.randn(m, F_SIZE, dtype=torch.float64)
    runs = {}
    for name, block, dtype, dev in (("truth", truth, torch.float64, "cpu"), ("emu", emu, torch.float32, DEV), ("hip", hip, torch.float32, DEV)):
        x = x64.clone().to(device=dev, dtype=dtype).requires_grad_()
        y = block(x) if name == "truth" else emulated_block(block, x) if name == "emu" else hidden_block(block, x, "bf16")
        y.backward(dy64.to(device=dev, dtype=y.dtype))
        runs[name] = (x, y)
    assert runs["hip"][1].dtype == torch.bfloat16 and runs["hip"][0].grad.dtype == torch.float32
    tag = f"bf16 hidden block m={m}"
    _judge(tag + " y", runs["hip"][1], runs["emu"][1], runs["truth"][1])
    _judge(tag + " dx", runs["hip"][0].grad, runs["emu"][0].grad, runs["truth"][0].grad)
    for name in ("0.weight", "0.bias", "1.weight", "1.bias"):
        p = {k: dict(b.named_parameters())[name].grad for k, b in (("truth", truth), ("emu", emu), ("hip", hip))}
        assert p["hip"].dtype == torch.float32
        _judge(f"{tag} d({name})", p["hip"], p["emu"], p["truth"])
    for name in ("running_mean", "running_var"):
        _judge(f"{tag} {name}", getattr(hip[1], name), getattr(emu[1], name), getattr(truth[1], name))
    assert int(hip[1].num_batches_tracked) == int(truth[1].num_batches_tracked) == 6


def _batch(n: int, seed: int):
    rng = np.random.default_rng(seed)
    planes = R.planes(n, rng)
    target = torch.from_numpy(rng.dirichlet(np.ones(7), n).astype(np.float32))
    q = torch.from_numpy(rng.uniform(-1, 1, (2, n)).astype(np.float32))
    return planes, target, q[0], q[1]


def test_forward_train_bf16_on_a_whole_network():
    torch.manual_seed(4)
    truth = ConnectFourNet(ModelConfig(1, 32, 3, 2)).double().train()
    emu, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    host = _batch(64, 4)
    losses = {}
    for name, model, dtype, dev in (("truth", truth, torch.float64, "cpu"), ("emu", emu, torch.float32, DEV), ("hip", hip, torch.float32, DEV)):
        batch = tuple(t.to(device=dev, dtype=dtype) for t in host)
        out = model(batch[0]) if name == "truth" else emulated_forward(model, batch[0]) if name == "emu" else forward_train(model, batch[0], "bf16")
        assert all(t.dtype == dtype for t in out)
        losses[name] = T.loss(out, batch)[0]
        losses[name].backward()
    _judge("forward_train bf16 loss", losses["hip"], losses["emu"], losses["truth"])
    grads = {name: dict(model.named_parameters()) for name, model in (("truth", truth), ("emu", emu), ("hip", hip))}
    for name, p in grads["truth"].items():      # the conv gradients carry the summed dx of the two heads through the tower
        assert grads["hip"][name].grad is not None and grads["hip"][name].grad.dtype == torch.float32, name
        _judge(f"forward_train bf16 d({name})", grads["hip"][name].grad, grads["emu"][name].grad, p.grad)
    for name, buf in truth.named_buffers():
        if buf.dtype.is_floating_point:
            _judge(f"forward_train bf16 {name}", dict(hip.named_buffers())[name], dict(emu.named_buffers())[name], buf)
        else:
            assert torch.equal(dict(hip.named_buffers())[name].cpu(), buf), name


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


def test_the_first_block_takes_f32_and_the_second_chains_in_bf16(monkeypatch):
    """fc_policy of ModelConfig(1, 32, 3, 2) has two hidden blocks: the first casts the tower's f32 output and writes y^T beside y,
    the second takes both as they are -- no cast of its input -- and the f32 output layer gets y.float()"""
    from c4a0_amd import train_heads

    torch.manual_seed(7)
    model = ConnectFourNet(ModelConfig(1, 32, 3, 2)).to(DEV).train()
    first, second = model.fc_policy[0], model.fc_policy[1]
    x = torch.randn(17, F_SIZE, device=DEV, requires_grad=True)
    counting = _CountingLib(train_heads.lib())
    monkeypatch.setattr(train_heads, "lib", lambda: counting)
    y1 = hidden_block(first, x, "bf16", emit_t=True)
    assert counting.calls == BF16_LAUNCHES_FIRST
    assert y1.dtype == torch.bfloat16 and y1.c4_transposed.dtype == torch.bfloat16 and tuple(y1.c4_transposed.shape) == (F_SIZE, 64)
    assert torch.equal(y1.c4_transposed[:, :17], y1.detach().t()) and not bool(y1.c4_transposed[:, 17:].any())
    del counting.calls[:]
    y2 = hidden_block(second, y1, "bf16")
    assert counting.calls == ["c4_train_cast_bf16", "c4_linear_bf16", "c4_train_bn_relu_fwd_bf16"]       # W alone is cast
    assert y2.dtype == torch.bfloat16 and not hasattr(y2, "c4_transposed")
    saved = y2.grad_fn.saved_tensors
    assert type(y2.grad_fn).__name__ == "HiddenBlockBf16FunctionBackward" and saved[0].data_ptr() == y1.data_ptr()
    assert saved[1].data_ptr() == y1.c4_transposed.data_ptr() and [t.dtype for t in saved[:4]] == [torch.bfloat16] * 4
    del counting.calls[:]
    out = model.fc_policy[2](y2.float())
    out.sum().backward()
    block_bwd = ["c4_train_bn_relu_bwd_bf16", "c4_train_cast_bf16", "c4_linear_bf16", "c4_linear_bf16"]   # dz, W^T, dgrad, wgrad
    assert counting.calls == block_bwd + block_bwd
    assert x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
    # a chained block without the handed-over transpose makes its own: one more cast, the same bytes
    del counting.calls[:]
    plain = y1.detach().clone()
    y2b = hidden_block(copy.deepcopy(second), plain, "bf16")
    assert counting.calls == ["c4_train_cast_bf16", "c4_train_cast_bf16", "c4_linear_bf16", "c4_train_bn_relu_fwd_bf16"]
    assert torch.equal(y2b.view(torch.int16), y2.detach().view(torch.int16))
    # ... and the whole network walks the same way
    del counting.calls[:]
    forward_train(model, R.planes(8, np.random.default_rng(0)).to(DEV), "bf16")
    assert counting.calls == BF16_LAUNCHES_FIRST + BF16_LAUNCHES_FIRST + ["c4_train_cast_bf16", "c4_linear_bf16", "c4_train_bn_relu_fwd_bf16"]


def test_an_input_that_needs_no_gradient_skips_dgrad(monkeypatch):
    from c4a0_amd import train_heads

    m = 17
    with_dx, without = copy.deepcopy(_block(m)).to(DEV).train(), copy.deepcopy(_block(m)).to(DEV).train()
    torch.manual_seed(400)
    x, dy = torch.randn(m, F_SIZE, device=DEV), torch.randn(m, F_SIZE, device=DEV).bfloat16()
    counting = _CountingLib(train_heads.lib())
    monkeypatch.setattr(train_heads, "lib", lambda: counting)
    xg = x.clone().requires_grad_()
    hidden_block(with_dx, xg, "bf16").backward(dy)
    assert counting.calls.count("c4_linear_bf16") == 3 and xg.grad is not None and bool(xg.grad.any())
    del counting.calls[:]
    hidden_block(without, x.clone(), "bf16").backward(dy)
    assert counting.calls == BF16_LAUNCHES_FIRST + ["c4_train_bn_relu_bwd_bf16", "c4_linear_bf16"]      # no W^T, no dgrad
    for (name, p), q in zip(with_dx.named_parameters(), without.parameters()):
        assert q.grad is not None and torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)), name


def test_a_second_backward_doubles_every_gradient():
    m = 17
    block = _block(m).to(DEV).train()
    torch.manual_seed(500)
    x, dy = torch.randn(m, F_SIZE, device=DEV).requires_grad_(), torch.randn(m, F_SIZE, device=DEV).bfloat16()
    y = hidden_block(block, x, "bf16")
    y.backward(dy, retain_graph=True)
    first = [t.grad.clone() for t in (x, *block.parameters())]
    y.backward(dy)
    for one, t in zip(first, (x, *block.parameters())):
        assert bool(one.any()) and torch.equal(t.grad.view(torch.int32), (2 * one).view(torch.int32))
    assert int(block[1].num_batches_tracked) == 6       # the statistics moved once, in the forward


def test_one_row_is_refused_like_batchnorm_refuses_it():
    block = _block(1).to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hidden_block(block, torch.randn(1, F_SIZE, device=DEV), "bf16")


def test_heads_bf16_refuses_by_name():
    planes = R.planes(4, np.random.default_rng(0))
    with pytest.raises(ValueError, match='heads="bf16": conv_filter_size 16 is not a multiple of 32'):
        forward_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).train(), planes.to(DEV), "bf16")
    with pytest.raises(ValueError, match="the master parameters must be f32"):
        forward_train(ConnectFourNet(ModelConfig(1, 32, 2, 2)).double().to(DEV).train(), planes.double().to(DEV), "bf16")
    with pytest.raises(ValueError, match="not on a HIP device"):
        forward_train(ConnectFourNet(ModelConfig(1, 32, 2, 2)).train(), planes, "bf16")
    with pytest.raises(ValueError, match="eval mode"):
        forward_train(ConnectFourNet(ModelConfig(1, 32, 2, 2)).to(DEV).eval(), planes.to(DEV), "bf16")
    model = ConnectFourNet(ModelConfig(1, 32, 2, 2)).to(DEV).train()
    with pytest.raises(ValueError, match="the batch is torch.float64"):
        forward_train(model, planes.double().to(DEV), "bf16")
    with pytest.raises(ValueError, match="the batch is torch.float32 on cpu"):
        resolve_heads(model, "bf16", planes)
    assert resolve_heads(model, "bf16", planes.to(DEV)) == "bf16" and resolve_heads(model, "auto", planes.to(DEV)) == "torch"


def test_a_nan_in_the_batch_shows_in_the_loss_as_on_the_torch_path():
    torch.manual_seed(6)
    stock = ConnectFourNet(ModelConfig(1, 32, 2, 2)).to(DEV).train()
    bf16 = copy.deepcopy(stock)
    host = list(_batch(8, 6))
    host[0][3, 1, 2, 4] = float("nan")
    batch = tuple(t.to(DEV) for t in host)
    losses = {}
    for name, model in (("torch", stock), ("bf16", bf16)):
        losses[name] = T.loss(forward_train(model, batch[0], name), batch)[0]
        losses[name].backward()
    evidence(f"forward_train, one NaN plane cell: loss {float(losses['bf16'].detach())} with heads=bf16, {float(losses['torch'].detach())} with heads=torch")
    assert bool(torch.isnan(losses["torch"])) and bool(torch.isnan(losses["bf16"]))
    for model in (stock, bf16):
        for lin in [layer[0] for head in (model.fc_policy, model.fc_value) for layer in head if isinstance(layer, nn.Sequential)]:
            assert lin.weight.grad is not None and not bool(torch.isfinite(lin.weight.grad).all())


# ------------------------------------------------------------------------------------------------------------------ learning
CONFIG = ModelConfig(1, 32, 2, 2)       # tests/train_recipe.py's problem at C = 32: its C = 16 cannot take the bf16 path
TRAIN_CONFIG = TrainConfig({0: 2e-3}, 4e-4)
N_TRAIN, N_VAL, BATCH, EPOCHS = 1024, 256, 128, 4


@pytest.fixture(scope="module")
def problem():
    """(student, train, val) on the CPU: a student learns the answers of a teacher of the same architecture whose output layers are
    scaled by 8, on two random disjoint binary planes per input (the recipe of tests/train_recipe.py)"""
    torch.manual_seed(1337)
    student, teacher = ConnectFourNet(CONFIG), ConnectFourNet(CONFIG).eval()
    with torch.no_grad():
        for layer in (teacher.fc_policy[-2], teacher.fc_value[-2]):
            layer.weight.mul_(8.0)
            layer.bias.mul_(8.0)
    rng = np.random.default_rng(1337)
    sets = []
    for n in (N_TRAIN, N_VAL):
        pos = R.planes(n, rng)
        with torch.no_grad():
            logp, q_pen, q_nopen = teacher(pos)
        sets.append(tuple(t.to(DEV) for t in (pos, logp.exp().contiguous(), q_pen.contiguous(), q_nopen.contiguous())))
    return student, sets[0], sets[1]


def _run(problem, heads: str):
    student, train, val = problem
    student = copy.deepcopy(student).to(DEV)
    untrained = evaluate_loss(copy.deepcopy(student), val, BATCH)
    _best, best_val, history = fit(student, train, val, BATCH, 1, TRAIN_CONFIG, seed=1337, heads=heads, max_epochs=EPOCHS)
    return untrained, best_val, history, student


@pytest.fixture
def deterministic_stock_ops():
    """The tower's convolutions and the output layers stay stock PyTorch; their backward kernels are asked to be deterministic ones,
    so that a difference between two runs can only come from the bf16 path.  (Adam turns the rounding noise of a gradient that is 0
    in real numbers -- a bias in front of a batch norm -- into steps of the size of the learning rate: an atomic sum in a stock
    kernel would show in the fourth digit of the first epoch's loss.)"""
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


def test_the_loop_learns_with_bf16_heads_and_repeats_byte_for_byte(problem, deterministic_stock_ops):
    untrained, best_val, history, model = _run(problem, "bf16")
    _u, _b, stock, stock_model = _run(problem, "torch")
    _u, _b, _h, stock_again = _run(problem, "torch")
    evidence("bf16 train recipe: two heads=\"torch\" runs from one seed give " +
             ("the same bytes" if all(torch.equal(p, q) for p, q in zip(stock_model.state_dict().values(), stock_again.state_dict().values()))
              else "DIFFERENT bytes (the stock ops are not deterministic here)"))
    val = {name: [h["val_loss"] for h in hist] for name, hist in (("bf16", history), ("torch", stock))}
    evidence(f"bf16 train recipe (C = 32): val_loss per epoch bf16 {val['bf16']}, torch {val['torch']}; train_loss bf16 "
             f"{[h['train_loss'] for h in history]}, torch {[h['train_loss'] for h in stock]}; untrained {untrained}")
    assert len(history) == EPOCHS and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in history)
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[-1]["val_loss"] < untrained
    assert best_val == min(val["bf16"])
    _u2, _b2, history2, again = _run(problem, "bf16")
    assert [h["train_loss"] for h in history2] == [h["train_loss"] for h in history]
    for (name, p), q in zip(model.state_dict().items(), again.state_dict().values()):
        assert torch.equal(p, q), name
