"""c4a0_amd.train_tower on the GPU, through autograd: forward_train(tower="hip") against the same model in float64 on the CPU, judged
beside the stock f32 module on the same device (the 4 x rule of tests/test_gpu_train_kernels.py: the HIP path's largest error against
float64 may be at most 4 x PyTorch's f32 one, floor 4 * 2^-24 * max |ref|), eval mode, and what the feature is for: a step and a
whole `fit` that repeat themselves byte for byte with no vendor switch set, eagerly and from the graph."""
import copy

import numpy as np
import pytest
import torch

from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_heads import forward_train
from c4a0_amd.train_tower import resolve_tower, tower_forward
from tests import train_recipe as R
from tests.helpers import evidence
from tests.test_gpu_train_heads import _judge

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _batch(n: int, seed: int):
    rng = np.random.default_rng(seed)
    planes = R.planes(n, rng)
    target = torch.from_numpy(rng.dirichlet(np.ones(7), n).astype(np.float32))
    q = torch.from_numpy(rng.uniform(-1, 1, (2, n)).astype(np.float32))
    return planes, target, q[0], q[1]


def _model(config: ModelConfig, seed: int) -> ConnectFourNet:
    """a network whose BatchNorm2d layers are away from their initial statistics and affine parameters"""
    torch.manual_seed(seed)
    model = ConnectFourNet(config).double().train()
    with torch.no_grad():
        for blk in list(model.conv)[1:]:
            bn = blk.block[2]
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
            bn.running_mean.normal_(0, 0.2)
            bn.running_var.uniform_(0.5, 2.0)
            bn.num_batches_tracked.fill_(5)
    return model


def equal_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


@pytest.mark.parametrize("config,n", [(ModelConfig(2, 16, 2, 2), 5), (ModelConfig(1, 32, 2, 2), 33)], ids=["2x16-B5", "1x32-B33"])
def test_forward_train_with_the_hip_tower_against_the_float64_model(config, n):
    truth = _model(config, 10 + n)
    stock, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    data = _batch(n, n)
    outs, losses = {}, {}
    for name, model, dtype, dev, tower in (("truth", truth, torch.float64, "cpu", "torch"), ("stock", stock, torch.float32, DEV, "torch"),
                                           ("hip", hip, torch.float32, DEV, "hip")):
        batch = tuple(t.to(device=dev, dtype=dtype) for t in data)
        outs[name] = forward_train(model, batch[0], heads="torch", tower=tower)
        losses[name] = T.loss(outs[name], batch)[0]
        losses[name].backward()
    tag = f"forward_train tower=hip {config.n_residual_blocks}x{config.conv_filter_size} B={n}"
    for i, what in enumerate(("policy log-probabilities", "q_penalty", "q_no_penalty")):
        assert outs["hip"][i].shape == outs["truth"][i].shape
        _judge(f"{tag} {what}", outs["hip"][i], outs["stock"][i], outs["truth"][i])
    grads = {name: dict(model.named_parameters()) for name, model in (("truth", truth), ("stock", stock), ("hip", hip))}
    for name, p in grads["truth"].items():
        assert grads["hip"][name].grad is not None and grads["hip"][name].grad.shape == p.grad.shape, name
        _judge(f"{tag} d({name})", grads["hip"][name].grad, grads["stock"][name].grad, p.grad)
    compared = 0
    for name, buf in truth.named_buffers():
        mine, theirs = dict(hip.named_buffers())[name], dict(stock.named_buffers())[name]
        if buf.dtype.is_floating_point:
            _judge(f"{tag} {name}", mine, theirs, buf)
        else:
            assert int(mine) == int(theirs) == int(buf), name
            if name.startswith("conv."):
                assert int(mine) == 6, name
        compared += name.startswith("conv.")
    assert compared == 3 * config.n_residual_blocks      # running_mean, running_var, num_batches_tracked of every BatchNorm2d


def test_the_eval_mode_path_is_the_modules():
    model = _model(ModelConfig(1, 16, 2, 2), 3).float().to(DEV).eval()
    planes = R.planes(3, np.random.default_rng(0)).to(DEV)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        assert torch.equal(tower_forward(model.conv, planes), model.conv(planes).reshape(3, -1))
        for a, b in zip(forward_train(model, planes, heads="auto", tower="auto"), model(planes)):
            assert torch.equal(a, b)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    with pytest.raises(ValueError, match='tower="hip": the model is in eval mode'):
        forward_train(model, planes, heads="torch", tower="hip")


def test_tower_hip_refuses_by_name():
    planes = R.planes(4, np.random.default_rng(0))
    with pytest.raises(ValueError, match="not a multiple of 16 up to 64"):
        resolve_tower(ConnectFourNet(ModelConfig(1, 8, 2, 2)).to(DEV).train(), "hip", planes.to(DEV))
    with pytest.raises(ValueError, match="not a multiple of 16 up to 64"):
        resolve_tower(ConnectFourNet(ModelConfig(1, 80, 1, 1)).to(DEV).train(), "hip", planes.to(DEV))
    with pytest.raises(ValueError, match="the kernels are f32"):
        resolve_tower(ConnectFourNet(ModelConfig(1, 16, 2, 2)).double().to(DEV).train(), "hip", planes.double().to(DEV))
    model = ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).train()
    assert resolve_tower(model, "hip", planes.to(DEV)) == "hip" and resolve_tower(model, "auto", planes.to(DEV)) == "torch"
    with pytest.raises(ValueError, match="the batch is"):
        resolve_tower(model, "hip", planes)


def test_a_step_repeats_itself_byte_for_byte(monkeypatch):
    """two forward + backward calls on equal inputs, the vendor library left to its own choice of algorithms"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    first = _model(ModelConfig(2, 32, 2, 2), 8).float().to(DEV)
    second = copy.deepcopy(first)
    batch = tuple(t.to(DEV) for t in _batch(40, 8))      # 40 boards: three chunks, the last a half
    for model in (first, second):
        T.loss(forward_train(model, batch[0], heads="hip", tower="hip"), batch)[0].backward()
    names = [n for n, _ in first.named_parameters() if n.startswith("conv.")]
    assert len(names) == 2 + 2 * 6
    for (name, p), q in zip(first.named_parameters(), second.parameters()):
        if name.startswith("conv."):
            assert bool(p.grad.any()) and equal_bits(p.grad, q.grad), name
    for (name, a), b in zip(first.named_buffers(), second.buffers()):
        assert equal_bits(a, b), name


def _fit(**kwargs):
    """the recipe's student on 300 samples at batch 64 (a partial last batch of 44), 2 epochs"""
    student, train, val = R.problem()
    student = student.to(DEV)
    train, val = tuple(t[:300].to(DEV) for t in train), tuple(t[:64].to(DEV) for t in val)
    _best, best_val, history = T.fit(student, train, val, 64, 1, R.TRAIN_CONFIG, seed=1337, heads="hip", tower="hip", max_epochs=2, **kwargs)
    return student.state_dict(), best_val, history


def _small(rows: int):
    """the recipe's student on its first `rows` training samples (at batch 64: 130 is 64 + 64 + 2, the smallest batch a kernel takes;
    129 leaves a tail of one, which is skipped) and 64 validation samples"""
    student, train, val = R.problem()
    return student.to(DEV), tuple(t[:rows].to(DEV) for t in train), tuple(t[:64].to(DEV) for t in val)


def _small_fit(rows: int, **kwargs):
    student, train, val = _small(rows)
    _best, _best_val, history = T.fit(student, train, val, 64, 1, R.TRAIN_CONFIG, seed=1337, heads="hip", tower="hip", max_epochs=2, **kwargs)
    return student.state_dict(), history


def _small_by_hand(rows: int, make_optimiser):
    """`fit`'s loop restated: 2 epochs of steps through the public forward_train, the sums in float64 in step order"""
    student, train, val = _small(rows)
    opt = make_optimiser(student.parameters(), lr=2e-3, weight_decay=4e-4)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(1337)
    history = []
    try:
        for epoch in range(2):
            student.train()
            perm = torch.randperm(rows, generator=gen).to(DEV)
            total, seen, steps = 0.0, 0, 0
            for i in range(0, rows, 64):
                idx = perm[i:i + 64]
                if len(idx) < 2:
                    continue
                b = tuple(t[idx] for t in train)
                opt.zero_grad()
                step_loss = T.loss(forward_train(student, b[0], "hip", "hip"), b)[0]
                step_loss.backward()
                opt.step()
                total += float(step_loss.detach()) * len(idx)
                seen += len(idx)
                steps += 1
            student.eval()
            with torch.no_grad():
                val_loss = float(T.loss(student(val[0]), val)[0])      # one batch of 64: its loss is the sample mean (x 64 / 64 is exact)
            history.append({"epoch": epoch, "train_loss": total / seen, "val_loss": val_loss, "lr": 2e-3, "steps": steps})
    finally:
        if hasattr(opt, "release"):      # HipAdam: the student does not keep gradients a dead table points at, as `fit` guarantees
            opt.release()
    return student.state_dict(), history


def _assert_same_run(name: str, got, want):
    different = [k for k, v in want[0].items() if not equal_bits(v, got[0][k])]
    assert list(got[0]) == list(want[0]) and not different, (name, different)
    assert got[1] == want[1], (name, got[1], want[1])


def test_fit_with_torch_adam_is_byte_for_byte_a_hand_written_loop():
    want = _small_by_hand(130, torch.optim.Adam)
    assert [h["steps"] for h in want[1]] == [3, 3]
    assert not torch.equal(R.problem()[0].state_dict()["conv.0.weight"], want[0]["conv.0.weight"].cpu())        # trained at all
    _assert_same_run("optimizer=torch", _small_fit(130, optimizer="torch"), want)


@pytest.mark.parametrize("rows,steps", [(130, 3), (129, 2)])
def test_fit_with_hip_adam_eagerly_and_from_the_graph_is_byte_for_byte_a_hand_written_loop(rows, steps):
    from c4a0_amd import train_graph

    want = _small_by_hand(rows, train_graph.HipAdam)
    assert [h["steps"] for h in want[1]] == [steps, steps]
    assert not torch.equal(R.problem()[0].state_dict()["conv.0.weight"], want[0]["conv.0.weight"].cpu())
    _assert_same_run("optimizer=hip", _small_fit(rows, optimizer="hip"), want)
    _assert_same_run("graph=True", _small_fit(rows, graph=True), want)


def test_a_whole_fit_repeats_itself_byte_for_byte_eagerly_and_from_the_graph(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    runs = {"A": _fit(optimizer="hip"), "A'": _fit(optimizer="hip"), "G": _fit(graph=True)}
    assert [h["steps"] for h in runs["A"][2]] == [5, 5]
    fresh = R.problem()[0].state_dict()
    assert not torch.equal(fresh["conv.0.weight"], runs["A"][0]["conv.0.weight"].cpu())        # the tower was trained at all
    for other in ("A'", "G"):
        different = [k for k, v in runs["A"][0].items() if not equal_bits(v, runs[other][0][k])]
        evidence(f"fit(tower=hip, heads=hip, optimizer=hip) 300 samples, batch 64, 2 epochs: A against {other}: "
                 f"{len(runs['A'][0]) - len(different)} of {len(runs['A'][0])} tensors byte-equal")
        assert not different, (other, different)
        assert runs[other][2] == runs["A"][2] and runs[other][1] == runs["A"][1], other
