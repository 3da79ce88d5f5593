"""outputs="hip" on the GPU through Python: `loss_train` against a float64 copy of the model beside outputs="torch", what is launched,
reproducibility of a whole fit, the learning recipe, that outputs="torch" is the step it was, the refusals, and a generation end to end."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import c4a0_amd
from c4a0_amd import train_graph, train_out
from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_heads import loss_train
from tests import train_recipe as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _batch(n: int, seed: int):
    rng = np.random.default_rng(seed)
    planes = R.planes(n, rng)
    target = rng.dirichlet(np.ones(7), n)
    target[::3] = np.eye(7)[rng.integers(0, 7, len(target[::3]))]          # one-hot rows
    q = torch.from_numpy(rng.uniform(-1, 1, (2, n)).astype(np.float32))
    return planes, torch.from_numpy(target.astype(np.float32)), q[0], q[1]


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().double().numpy()


def _judge(what, got, other, truth, floor_u=U):
    """the 4 x rule: max |got - truth| <= max(4 max |other - truth|, 4 floor_u max |truth|)"""
    truth = _np(truth)
    e_k, e_t = float(np.abs(_np(got) - truth).max()), float(np.abs(_np(other) - truth).max())
    floor = 4 * floor_u * float(np.abs(truth).max())
    evidence(f"{what}: outputs=hip err {e_k:.3e}, outputs=torch err {e_t:.3e}, ratio {e_k / e_t if e_t else float('inf'):.2f}, floor {floor:.3e}")
    assert e_k <= max(4 * e_t, floor), (what, e_k, e_t, floor)


def equal_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ loss_train
@pytest.mark.parametrize("n", [2, 130])
@pytest.mark.parametrize("config", [ModelConfig(1, 16, 2, 2), ModelConfig(1, 16, 1, 1)], ids=["hidden", "no-hidden"])
def test_loss_train_with_hip_outputs_against_the_float64_model(config, n):
    """no-hidden: both heads read the tower's output, and its gradient is the sum of the two dx"""
    torch.manual_seed(20 + n)
    truth = ConnectFourNet(config).double().train()
    stock, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    data = _batch(n, n)
    losses = {}
    for name, model, dtype, dev, outputs in (("truth", truth, torch.float64, "cpu", "torch"), ("stock", stock, torch.float32, DEV, "torch"),
                                             ("hip", hip, torch.float32, DEV, "hip")):
        batch = tuple(t.to(device=dev, dtype=dtype) for t in data)
        losses[name] = loss_train(model, batch, heads="torch", tower="torch", outputs=outputs)
        losses[name][0].backward()
    tag = f"loss_train outputs=hip {config.n_policy_layers}/{config.n_value_layers} layers B={n}"
    for i, what in enumerate(("total", "policy_kl", "q_penalty_mse", "q_no_penalty_mse")):
        assert losses["hip"][i].shape == () and losses["hip"][i].dtype == torch.float32
        _judge(f"{tag} {what}", losses["hip"][i], losses["stock"][i], losses["truth"][i])
    assert losses["hip"][0].requires_grad and not any(v.requires_grad for v in losses["hip"][1:])
    grads = {name: dict(model.named_parameters()) for name, model in (("truth", truth), ("stock", stock), ("hip", hip))}
    for name, p in grads["truth"].items():
        assert grads["hip"][name].grad is not None and grads["hip"][name].grad.shape == p.grad.shape, name
        _judge(f"{tag} d({name})", grads["hip"][name].grad, grads["stock"][name].grad, p.grad)


def test_loss_train_hands_bf16_activations_to_the_kernels(monkeypatch):
    """heads="bf16" at ModelConfig(1, 32, 2, 2): the Function receives the blocks' bf16 output as it is and returns a bf16 dx; judged
    against float64 beside heads="bf16", outputs="torch" by test_gpu_train_bf16_heads.py's rule (floor 2^-8 max |truth|)"""
    torch.manual_seed(9)
    truth = ConnectFourNet(ModelConfig(1, 32, 2, 2)).double().train()
    stock, hip = copy.deepcopy(truth).float().to(DEV), copy.deepcopy(truth).float().to(DEV)
    data = _batch(64, 9)
    seen = []
    apply = train_out.OutLossFunction.apply

    def spy(*args):
        seen.append((args[0].dtype, args[1].dtype))
        return apply(*args)

    monkeypatch.setattr(train_out.OutLossFunction, "apply", spy)
    losses = {}
    for name, model, dtype, dev, heads, outputs in (("truth", truth, torch.float64, "cpu", "torch", "torch"),
                                                    ("stock", stock, torch.float32, DEV, "bf16", "torch"), ("hip", hip, torch.float32, DEV, "bf16", "hip")):
        batch = tuple(t.to(device=dev, dtype=dtype) for t in data)
        losses[name] = loss_train(model, batch, heads=heads, tower="torch", outputs=outputs)
        losses[name][0].backward()
    assert seen == [(torch.bfloat16, torch.bfloat16)]
    for i, what in enumerate(("total", "policy_kl", "q_penalty_mse", "q_no_penalty_mse")):
        _judge(f"loss_train heads=bf16 outputs=hip {what}", losses["hip"][i], losses["stock"][i], losses["truth"][i], floor_u=2.0 ** -10)
    grads = {name: dict(model.named_parameters()) for name, model in (("truth", truth), ("stock", stock), ("hip", hip))}
    for name, p in grads["truth"].items():
        assert grads["hip"][name].grad is not None and grads["hip"][name].grad.dtype == torch.float32, name
        _judge(f"loss_train heads=bf16 outputs=hip d({name})", grads["hip"][name].grad, grads["stock"][name].grad, p.grad, floor_u=2.0 ** -10)


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


def test_one_library_call_forward_and_one_backward(monkeypatch):
    torch.manual_seed(3)
    model = ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).train()
    batch = tuple(t.to(DEV) for t in _batch(17, 3))
    counting = _CountingLib(train_out.lib())
    monkeypatch.setattr(train_out, "lib", lambda: counting)
    total = loss_train(model, batch, heads="torch", tower="torch", outputs="hip")[0]
    assert counting.calls == ["c4_train_out_loss_fwd"]
    del counting.calls[:]
    total.backward()
    assert counting.calls == ["c4_train_out_loss_bwd"]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in model.parameters())


# ------------------------------------------------------------------------------------------------------------------ whole fits
def _fit(**kwargs):
    """the recipe's student on 300 samples at batch 64 (a partial last batch of 44), 2 epochs, every part of a step on the kernels"""
    student, train, val = R.problem()
    student = student.to(DEV)
    train, val = tuple(t[:300].to(DEV) for t in train), tuple(t[:64].to(DEV) for t in val)
    _best, best_val, history = T.fit(student, train, val, 64, 1, R.TRAIN_CONFIG, seed=1337, heads="hip", tower="hip", outputs="hip", max_epochs=2,
                                     **kwargs)
    return student.state_dict(), best_val, history


def test_a_whole_fit_repeats_itself_byte_for_byte_eagerly_and_from_the_graph(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
    runs = {"A": _fit(optimizer="hip"), "A'": _fit(optimizer="hip"), "G": _fit(graph=True)}
    assert [h["steps"] for h in runs["A"][2]] == [5, 5]
    fresh = R.problem()[0].state_dict()
    assert not torch.equal(fresh["fc_policy.1.weight"], runs["A"][0]["fc_policy.1.weight"].cpu())        # the output layer was trained at all
    for other in ("A'", "G"):
        different = [k for k, v in runs["A"][0].items() if not equal_bits(v, runs[other][0][k])]
        evidence(f"fit(outputs=hip, tower=hip, heads=hip, optimizer=hip) 300 samples, batch 64, 2 epochs: A against {other}: "
                 f"{len(runs['A'][0]) - len(different)} of {len(runs['A'][0])} tensors byte-equal")
        assert not different, (other, different)
        assert runs[other][2] == runs["A"][2] and runs[other][1] == runs["A"][1], other


def _recipe(device, outputs: str, dtype=torch.float32):
    student, train, val = R.problem()
    student = student.to(device=device, dtype=dtype)
    train = tuple(t.to(device=device, dtype=dtype) for t in train)
    val = tuple(t.to(device=device, dtype=dtype) for t in val)
    untrained = T.evaluate_loss(copy.deepcopy(student), val, R.BATCH)
    _best, best_val, history = T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, seed=1337, heads="torch", outputs=outputs, max_epochs=R.EPOCHS)
    return untrained, best_val, history


def test_the_recipe_learns_with_hip_outputs_and_tracks_the_torch_path():
    untrained, best_val, history = _recipe(DEV, "hip")
    _u, _b, stock = _recipe(DEV, "torch")
    _u64, _b64, truth = _recipe("cpu", "torch", torch.float64)
    val = {name: [h["val_loss"] for h in hist] for name, hist in (("hip", history), ("torch", stock), ("float64", truth))}
    evidence(f"train recipe outputs=hip val_loss per epoch: hip {val['hip']}, torch {val['torch']}, float64 {val['float64']}; train_loss "
             f"{[h['train_loss'] for h in history]}; untrained {untrained}")
    assert len(history) == R.EPOCHS and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in history)
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[-1]["val_loss"] < untrained
    assert best_val == min(val["hip"])
    for e in range(R.EPOCHS):
        e_hip, e_torch = abs(val["hip"][e] - val["float64"][e]), abs(val["torch"][e] - val["float64"][e])
        assert e_hip <= max(4 * e_torch, 4 * U * abs(val["float64"][e])), (e, e_hip, e_torch)


def test_outputs_torch_is_the_step_it_was():
    """train_step's default argument and outputs_path="torch" from one state: the same bytes; fit() and fit(outputs="torch"): the same
    history and the same bytes.  Heads and tower run on the deterministic kernels (the stock tower's backward adds with atomics), so the
    stock ops of a step are the output layers and the loss, which repeat themselves at this size, as tests/test_gpu_train_tower.py relies
    on."""
    student, train, _val = R.problem()
    batch = tuple(t[:64].to(DEV) for t in train)
    models = [copy.deepcopy(student).to(DEV).train() for _ in range(2)]
    opts = [torch.optim.Adam(m.parameters(), lr=2e-3, weight_decay=4e-4) for m in models]
    a = train_graph.train_step(models[0], opts[0], batch, "hip", "hip")
    b = train_graph.train_step(models[1], opts[1], batch, "hip", "hip", "torch")
    assert equal_bits(a, b) and all(equal_bits(p, q) for p, q in zip(models[0].state_dict().values(), models[1].state_dict().values()))
    assert not torch.equal(models[0].state_dict()["fc_policy.1.weight"].cpu(), student.state_dict()["fc_policy.1.weight"])
    runs = []
    for kwargs in ({}, {"outputs": "torch"}):
        model, train, val = R.problem()
        model = model.to(DEV)
        train, val = tuple(t[:130].to(DEV) for t in train), tuple(t[:64].to(DEV) for t in val)
        _best, best_val, history = T.fit(model, train, val, 64, 1, R.TRAIN_CONFIG, seed=1337, heads="hip", tower="hip", max_epochs=2, **kwargs)
        runs.append((model.state_dict(), best_val, history))
    assert runs[0][2] == runs[1][2] and runs[0][1] == runs[1][1]
    assert all(equal_bits(v, runs[1][0][k]) for k, v in runs[0][0].items())


def test_outputs_hip_refuses_by_name():
    planes = R.planes(4, np.random.default_rng(0))
    batch = (planes, torch.full((4, 7), 1 / 7), torch.zeros(4), torch.zeros(4))
    on_dev = tuple(t.to(DEV) for t in batch)
    with pytest.raises(ValueError, match='outputs="hip": the model is on cpu, not on a HIP device'):
        loss_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).train(), batch, outputs="hip")
    with pytest.raises(ValueError, match='outputs="hip": the model is torch.bfloat16, the kernels are f32'):
        loss_train(ConnectFourNet(ModelConfig(1, 16, 2, 2)).bfloat16().to(DEV).train(), tuple(t.bfloat16() for t in on_dev), outputs="hip")
    with pytest.raises(ValueError, match='outputs="hip": conv_filter_size 6 is not a multiple of 4'):
        loss_train(ConnectFourNet(ModelConfig(1, 6, 2, 2)).to(DEV).train(), on_dev, outputs="hip")
    model = ConnectFourNet(ModelConfig(1, 16, 2, 2)).to(DEV).train()
    with pytest.raises(ValueError, match="outputs must be one of"):
        loss_train(model, on_dev, outputs="cuda")
    with pytest.raises(ValueError, match="outputs must be one of"):
        T.fit(model, on_dev, on_dev, 4, 0, T.TrainConfig(), outputs="cuda", max_epochs=1)
    with pytest.raises(ValueError, match="the batch is torch.float32 on cpu"):
        train_out.resolve_outputs(model, "hip", planes)
    assert train_out.resolve_outputs(model, "auto", on_dev[0]) == "torch" and train_out.resolve_outputs(model, "hip", on_dev[0]) == "hip"
    # conv_filter_size 4: F = 168, the smallest network the kernels take
    small = ConnectFourNet(ModelConfig(1, 4, 2, 1)).to(DEV).train()
    assert bool(torch.isfinite(loss_train(small, on_dev, outputs="hip")[0]))
    # the work space a step allocates is the library's figure
    for m, k in ((1, 8), (2000, 1344), (2000, 8), (577, 672)):
        assert train_out._work(m, k, DEV).numel() * 4 == train_out.work_bytes(m, k)


def test_train_single_gen_end_to_end_with_hip_outputs(tmp_path):
    base = str(tmp_path)
    torch.manual_seed(11)
    parent = T.TrainingGen.load_latest_with_default(base, 30, 6.6, 0.01, 64, 256, ModelConfig(1, 32, 2, 2), T.TrainConfig({0: 2e-3}, 4e-4))
    gen = c4a0_amd.train_single_gen(base, DEV, parent, n_self_play_games=64, n_mcts_iterations=30, c_exploration=6.6, c_ply_penalty=0.01,
                                    self_play_batch_size=64, training_batch_size=256, outputs="hip", heads="hip", graph=True, max_epochs=2,
                                    resident_games=64)
    assert sorted(os.listdir(gen.gen_folder(base))) == ["games.pkl", "metadata.json", "model.json", "model.pt"]
    assert gen.gen_n == 1 and gen.val_loss is not None and math.isfinite(gen.val_loss)
