"""Training from a captured HIP graph on the GPU: `fit(graph=True)` -- every step a replay of `train_graph.GraphedTrainStep` with
`train_graph.HipAdam` -- against the same loop run eagerly (`optimizer="hip"`), the learning recipe of tests/train_recipe.py under
the graph for every head path, and `train_single_gen(graph=True)` end to end."""
import copy
import functools
import math
import os

import pytest
import torch

import c4a0_amd
from c4a0_amd import train_graph
from c4a0_amd import training as T
from c4a0_amd.nn import InferenceNet, ModelConfig
from tests import train_recipe as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


@pytest.fixture
def optimisers(monkeypatch):
    """every HipAdam a `fit` of the test makes, in order"""
    made = []

    class Recorded(train_graph.HipAdam):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(train_graph, "HipAdam", Recorded)
    return made


def run(heads: str, batch: int, epochs: int, n_train: int = R.N_TRAIN, **fit_kwargs):
    """the recipe's problem on the GPU with `fit`'s new arguments: (untrained val_loss, best_val, history, the trained model)"""
    student, train, val = R.problem()
    student = student.to(DEV)
    train = tuple(t[:n_train].to(DEV) for t in train)
    val = tuple(t.to(DEV) for t in val)
    untrained = T.evaluate_loss(copy.deepcopy(student), val, R.BATCH)
    _best, best_val, history = T.fit(student, train, val, batch, 1, R.TRAIN_CONFIG, seed=1337, heads=heads, max_epochs=epochs, **fit_kwargs)
    return untrained, best_val, history, student


def is_hidden(key: str) -> bool:
    """a parameter or buffer of a head's hidden block: fc_policy.<block>.<layer>.<name>"""
    return key.startswith(("fc_policy.", "fc_value.")) and key.count(".") == 3


def equal_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def test_one_step_is_bit_for_bit_the_eager_step(optimisers):
    # 128 samples at batch 128: one epoch is exactly one step
    _u, _b, hist_e, eager = run("hip", 128, 1, n_train=128, optimizer="hip")
    _u, _b, hist_g, graphed = run("hip", 128, 1, n_train=128, graph=True)
    assert hist_e[0]["steps"] == hist_g[0]["steps"] == 1
    opt_e, opt_g = optimisers
    assert opt_e.steps == opt_g.steps == 1
    se, sg = eager.state_dict(), graphed.state_dict()
    hidden = [k for k in se if is_hidden(k)]
    assert len(hidden) == 2 * 7      # one hidden block a head: Linear weight, bias; BatchNorm1d weight, bias, running_mean, running_var, count
    for k in hidden:
        assert equal_bits(se[k], sg[k]), k
    names = [n for n, p in eager.named_parameters() if p.requires_grad]
    assert len(names) == len(opt_e.m) == len(opt_g.m)
    compared = 0
    for i, n in enumerate(names):
        if is_hidden(n):
            assert equal_bits(opt_e.m[i], opt_g.m[i]) and equal_bits(opt_e.v[i], opt_g.v[i]), n
            assert float(opt_g.v[i].abs().max()) > 0, n          # the step ran: autograd's backward landed in the capture
            compared += 1
    assert compared == 2 * 4
    # the step moved the parameters at all
    fresh = R.problem()[0].state_dict()
    assert not torch.equal(fresh["fc_policy.0.0.weight"], sg["fc_policy.0.0.weight"].cpu())
    assert hist_e[0]["train_loss"] == hist_g[0]["train_loss"]


def test_warm_up_leaves_no_trace(optimisers):
    _u, _b, history, model = run("hip", 120, 1, graph=True)       # 8 full batches and a tail of 64: two captures, each after warm-up steps
    steps = history[0]["steps"]
    assert steps == 9
    counts = {k: int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(counts) == 1 + 2 and set(counts.values()) == {steps}, counts        # the tower's BatchNorm2d, the heads' two BatchNorm1d
    assert optimisers[0].steps == steps
    assert all(p.grad is None for p in model.parameters())          # the finished optimiser released its persistent gradients


def test_the_snapshot_is_taken_before_the_warm_up_starts_behind_a_backlog():
    """A capture made while the current stream still has work queued, as a fit's lazily captured tail graph is behind the epoch's
    replays: the snapshot's clones and the side stream's warm-up steps both wait for that work and then start together, so the
    warm-up must also wait for the clones.  Every value the warm-up writes is compared, not only the counts."""
    student, train, _val = R.problem()
    model = student.to(DEV).train()
    train = tuple(t[:128].to(DEV) for t in train)
    opt = train_graph.HipAdam(model.parameters(), lr=2e-3, weight_decay=4e-4)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a, out = torch.randn(4096, 4096, device=DEV), torch.empty(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    for _ in range(40):            # tens of milliseconds of queued work: the host is far ahead when the capture begins
        torch.mm(a, a, out=out)
    step = train_graph.GraphedTrainStep(model, opt, "hip", 128, train)
    torch.cuda.synchronize()
    after = model.state_dict()
    for k in before:
        assert equal_bits(before[k], after[k]), k
    assert all(not t.any() for t in opt.m + opt.v) and opt.steps == 0 and float(step.total) == 0.0
    step.run(torch.arange(128, device=DEV))
    assert opt.steps == 1 and int(after["conv.1.block.2.num_batches_tracked"]) == 1 and float(step.total) > 0.0
    opt.release()


def test_a_failing_fit_releases_the_persistent_gradients():
    student, train, val = R.problem()
    model = student.to(DEV)
    train, val = tuple(t[:256].to(DEV) for t in train), tuple(t.to(DEV) for t in val)

    def broken(_model, _val, _batch):
        raise RuntimeError("no validation today")

    for kwargs in (dict(optimizer="hip"), dict(graph=True)):
        with pytest.raises(RuntimeError, match="no validation today"):
            T.fit(model, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, heads="hip", val_loss_fn=broken, **kwargs)
        assert all(p.grad is None for p in model.parameters()), kwargs


def test_several_steps_against_the_eager_paths_own_noise(optimisers, monkeypatch):
    """A, A' (eager HipAdam, twice) and G (the graph) from one seed.  The vendor's kernels are asked for their deterministic
    algorithms: left to themselves the tower's convolution backward adds with atomics (a one-step gradient differs from itself by
    3e-8 to 8e-8) and, from the second step on, the stock path and this one were each seen to land on either of two gradients of the
    tower that differ by 3e-4 -- run to run, torch.optim.Adam's loop included -- so that A = A' says nothing about the next run.
    Asked, the eager path repeats itself bit for bit (measured: noise 0 in every tensor), which makes the strict branch the one that
    runs.  Measured without the flag, three repetitions of A, A', G: max |A - A'| over the tensors 4.3e-4, 9.9e-5, 5.2e-5; G within
    4 x noise per tensor in two of them, in the third fc_policy.0.0.weight 4.3e-4 from A where A' was 3.4e-7 from it -- the first
    repetition's own |A - A'|: one pair is no measure of the eager path's spread there."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    runs = {name: run("hip", 120, 2, **kw) for name, kw in (("A", dict(optimizer="hip")), ("A'", dict(optimizer="hip")), ("G", dict(graph=True)))}
    states = {name: r[3].state_dict() for name, r in runs.items()}
    hist = {name: r[2] for name, r in runs.items()}
    assert [h["steps"] for h in hist["G"]] == [h["steps"] for h in hist["A"]] == [9, 9]
    noise = {k: float((states["A"][k].double() - states["A'"][k].double()).abs().max()) for k in states["A"]}
    if max(noise.values()) == 0.0 and hist["A"] == hist["A'"]:
        case = "the eager path repeats itself bit for bit: the graph must equal it byte for byte"
        for k in states["A"]:
            assert equal_bits(states["A"][k], states["G"][k]), k
        assert hist["G"] == hist["A"]
        assert runs["G"][1] == runs["A"][1]
    else:
        case = f"the eager path differs from itself (max {max(noise.values()):.3e}): the graph within 4 x that, per tensor"
        for k in states["A"]:
            d = float((states["A"][k].double() - states["G"][k].double()).abs().max())
            assert d <= 4 * noise[k], (k, d, noise[k])
    print("graph against eager:", case)
    evidence(f"fit(graph=True) against eager HipAdam, 2 epochs at batch 120 (64-row tail graph): {case}")
    # a tail of one sample is skipped, as in the eager loop
    _u, _b, h_e, _m = run("hip", 120, 1, n_train=961, optimizer="hip")
    _u, _b, h_g, _m = run("hip", 120, 1, n_train=961, graph=True)
    assert h_g[0]["steps"] == h_e[0]["steps"] == 8
    assert optimisers[-1].steps == 8


@functools.lru_cache(maxsize=None)
def baselines():
    """val_loss per epoch of the recipe on the stock path: f32 on the GPU, float64 on the CPU"""
    stock = [h["val_loss"] for h in R.run(DEV, "torch")[2]]
    truth = [h["val_loss"] for h in R.run("cpu", "torch", dtype=torch.float64)[2]]
    return stock, truth


@pytest.mark.parametrize("heads", ["torch", "hip", "bf16"])
def test_the_recipe_learns_under_the_graph(heads, monkeypatch):
    if heads == "bf16":
        monkeypatch.setattr(R, "CONFIG", ModelConfig(1, 32, 2, 2))     # c4_linear_bf16 needs F = 42 C to be a multiple of 192
    untrained, best_val, history, _model = run(heads, R.BATCH, R.EPOCHS, graph=True)
    val = [h["val_loss"] for h in history]
    print(f"graph, heads={heads}: val_loss per epoch {val}, train_loss {[h['train_loss'] for h in history]}, untrained {untrained}")
    evidence(f"train recipe under graph=True, heads={heads}: val_loss per epoch {val}")
    assert len(history) == R.EPOCHS and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in history)
    assert [h["steps"] for h in history] == [R.N_TRAIN // R.BATCH] * R.EPOCHS
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[-1]["val_loss"] < untrained
    assert best_val == min(val)
    if heads != "bf16":
        stock, truth = baselines()
        for e in range(R.EPOCHS):
            e_graph, e_torch = abs(val[e] - truth[e]), abs(stock[e] - truth[e])
            print(f"epoch {e}: |graph - float64| = {e_graph:.3e}, |torch - float64| = {e_torch:.3e}")
            assert e_graph <= max(4 * e_torch, 4 * U * abs(truth[e])), (e, e_graph, e_torch)


def test_graph_refusals_by_name():
    student, train, val = R.problem()
    student = student.to(DEV)
    train, val = tuple(t.to(DEV) for t in train), tuple(t.to(DEV) for t in val)
    with pytest.raises(ValueError, match='graph=True needs optimizer="hip"'):
        T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, graph=True, optimizer="torch")
    with pytest.raises(ValueError, match="graph=True: the model is not f32"):
        T.fit(student.double(), tuple(t.double() for t in train), tuple(t.double() for t in val), R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, graph=True)


def test_hip_adam_keeps_its_gradients_and_counts_on_the_device():
    torch.manual_seed(3)
    layer = torch.nn.Linear(5, 3).to(DEV)
    opt = train_graph.HipAdam(layer.parameters(), lr=1e-2, weight_decay=4e-4)
    grads = [p.grad for p in layer.parameters()]
    assert all(g is not None and not g.any() for g in grads) and opt.steps == 0
    x = torch.randn(8, 5, device=DEV)
    for step in range(1, 4):
        opt.zero_grad()
        layer(x).square().sum().backward()
        assert all(p.grad is g and p.grad.data_ptr() == g.data_ptr() for p, g in zip(layer.parameters(), grads))   # accumulated in place
        opt.step()
        assert opt.steps == step
    layer.weight.grad = None                       # dropped from outside: zero_grad puts the persistent one back
    opt.zero_grad()
    assert layer.weight.grad is grads[0] and not grads[0].any() and not grads[1].any()


def test_train_single_gen_under_the_graph_end_to_end(tmp_path):
    base = str(tmp_path)
    torch.manual_seed(11)
    parent = T.TrainingGen.load_latest_with_default(base, 30, 6.6, 0.01, 64, 256, ModelConfig(1, 32, 2, 2), T.TrainConfig({0: 2e-3}, 4e-4))
    timings = {}
    gen = c4a0_amd.train_single_gen(base, DEV, parent, n_self_play_games=64, n_mcts_iterations=30, c_exploration=6.6, c_ply_penalty=0.01,
                                    self_play_batch_size=64, training_batch_size=256, heads="hip", max_epochs=3, timings=timings, graph=True,
                                    resident_games=64)
    folder = gen.gen_folder(base)
    assert sorted(os.listdir(folder)) == ["games.pkl", "metadata.json", "model.json", "model.pt"]
    assert gen.gen_n == 1 and gen.parent == parent.created_at and timings["epochs"] == 3
    games = gen.get_games(base)
    child = gen.get_model(base)
    _train, val = T.generation_tensors(games, DEV)
    again = T.evaluate_loss(child.to(DEV), val, 256)
    assert math.isfinite(gen.val_loss) and gen.val_loss == pytest.approx(again, rel=1e-6)
    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(32)]
    by_child = c4a0_amd.play_games(reqs, 32, 30, 6.6, 0.01, evaluator=InferenceNet(child, DEV), resident_games=32)
    by_parent = c4a0_amd.play_games(reqs, 32, 30, 6.6, 0.01, evaluator=InferenceNet(parent.get_model(base), DEV), resident_games=32)
    assert len(by_child) == 32
    assert by_child.to_records()[0].tobytes() != by_parent.to_records()[0].tobytes()
