"""c4a0_amd.training on the CPU (heads="torch"): the loss, the learning-rate schedule, early stopping and the best model, the
generation folder, the training tensors, determinism, and that the loop learns."""
import copy
import json
from datetime import datetime

import numpy as np
import pytest
import torch

from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from tests import train_recipe as R


def test_loss_equals_a_float64_restatement():
    rng = np.random.default_rng(5)
    for b in (1, 7, 64):
        logits = rng.standard_normal((b, 7))
        logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
        target = rng.random((b, 7))
        target[rng.random((b, 7)) < 0.3] = 0.0          # zero targets: log(0 + EPS)
        target = (target / np.maximum(target.sum(1, keepdims=True), 1e-9)).astype(np.float32)
        q = rng.uniform(-1, 1, (4, b)).astype(np.float32)
        got = T.loss(tuple(torch.from_numpy(a) for a in (logp, q[0], q[1])), (None,) + tuple(torch.from_numpy(a) for a in (target, q[2], q[3])))
        # in f32 as the code forms it: t + EPS; the rest in float64
        t = (target + np.float32(1e-8)).astype(np.float64)
        kl = (t * (np.log(t) - logp.astype(np.float64))).sum(1).mean()
        mse_p = ((q[0].astype(np.float64) - q[2]) ** 2).mean()
        mse_n = ((q[1].astype(np.float64) - q[3]) ** 2).mean()
        want = (kl + mse_p + mse_n, kl, mse_p, mse_n)
        for g, w in zip(got, want):
            assert abs(float(g) - w) <= 1e-5 * max(1.0, abs(w)), (float(g), w)
    # an exact prediction of a positive target costs nothing
    p = torch.tensor([[0.1, 0.2, 0.3, 0.1, 0.1, 0.1, 0.1]])
    z = torch.zeros(1)
    assert abs(float(T.loss((torch.log(p + 1e-8), z, z), (None, p, z, z))[0])) < 1e-6


def test_lr_schedule_picks_like_the_reference():
    s = {0: 2e-3, 10: 8e-4}
    assert [T.lr_for_gen(s, g) for g in (0, 9, 10, 11)] == [2e-3, 2e-3, 8e-4, 8e-4]
    assert T.lr_for_gen({10: 8e-4, 0: 2e-3, 20: 1e-4}, 25) == 1e-4
    assert T.lr_for_gen({5: 1e-3}, 0) == 1e-3                     # the first entry holds from the start whatever its threshold
    assert T.parse_lr_schedule([0, 2e-3, 10, 8e-4]) == s
    with pytest.raises(AssertionError):
        T.parse_lr_schedule([0, 2e-3, 10])
    with pytest.raises(AssertionError):
        T.parse_lr_schedule([0.5, 2e-3])


def _tiny():
    torch.manual_seed(3)
    model = ConnectFourNet(ModelConfig(0, 1, 2, 1))
    rng = np.random.default_rng(3)
    pos = R.planes(12, rng)
    data = (pos, torch.full((12, 7), 1 / 7), torch.zeros(12), torch.zeros(12))
    return model, data


def _scripted(losses):
    """a val_loss hook that answers from a script and records the model's first conv bias at each call"""
    calls = []

    def hook(model, val, batch_size):
        calls.append(model.conv[0].bias.detach().clone())
        return losses[len(calls) - 1]

    return hook, calls


def test_early_stopping_and_best_model_follow_a_scripted_validation_loss():
    # epoch 2 is the strict minimum; epoch 5 ties it (no improvement); ten epochs without improvement after epoch 2: stop after epoch 12
    script = [0.9, 0.8, 0.5, 0.6, 0.7, 0.5, 0.55] + [0.6] * 20
    model, data = _tiny()
    hook, calls = _scripted(script)
    best, best_val, history = T.fit(model, data, data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook)
    assert len(history) == len(calls) == 13 and [h["val_loss"] for h in history] == script[:13]
    assert best_val == 0.5
    assert torch.equal(best.conv[0].bias, calls[2]) and not torch.equal(calls[2], calls[5]) and not torch.equal(calls[2], calls[12])
    assert all(h["steps"] == 3 for h in history)
    # an improvement resets the count: 0.4 at epoch 9 gives ten more epochs
    script = [0.5] + [0.6] * 8 + [0.4] + [0.7] * 30
    model, data = _tiny()
    hook, calls = _scripted(script)
    best, best_val, history = T.fit(model, data, data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook)
    assert len(history) == 20 and best_val == 0.4 and torch.equal(best.conv[0].bias, calls[9])
    # max_epochs and patience are arguments
    model, data = _tiny()
    hook, calls = _scripted([1.0] * 50)
    assert len(T.fit(model, data, data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook, patience=3)[2]) == 4
    model, data = _tiny()
    hook, calls = _scripted([1.0 - 0.01 * i for i in range(50)])
    best, best_val, history = T.fit(model, data, data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook, max_epochs=6)
    assert len(history) == 6 and best_val == pytest.approx(0.95) and torch.equal(best.conv[0].bias, calls[5])


def test_a_trailing_batch_of_one_sample_is_skipped():
    model, data = _tiny()
    data = tuple(t[:9] for t in data)
    hook, _ = _scripted([1.0] * 3)
    history = T.fit(model, data, data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook, max_epochs=1)[2]
    assert history[0]["steps"] == 2                              # 4 + 4, the ninth sample alone is left out
    history = T.fit(model, tuple(t[:7] for t in data), data, 4, 0, T.TrainConfig({0: 1e-2}, 0.0), heads="torch", val_loss_fn=hook, max_epochs=1)[2]
    assert history[0]["steps"] == 2                              # 4 + 3: the partial batch is kept


def test_fit_is_byte_for_byte_a_hand_written_loop():
    """9 samples at batch 4 (two steps and a skipped tail of one), 2 epochs: `fit` against the loop restated here"""
    cfg, epochs, seed = T.TrainConfig({0: 1e-2}, 4e-4), 2, 5
    model, data = _tiny()
    data = tuple(t[:9] for t in data)
    mine = copy.deepcopy(model)
    _best, _best_val, history = T.fit(model, data, data, 4, 0, cfg, seed=seed, heads="torch", optimizer="torch", max_epochs=epochs)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    opt = torch.optim.Adam(mine.parameters(), lr=1e-2, weight_decay=4e-4)
    means = []
    for _epoch in range(epochs):
        mine.train()
        perm = torch.randperm(9, generator=gen)
        total, seen = np.float64(0.0), 0
        for i in range(0, 9, 4):
            idx = perm[i:i + 4]
            if len(idx) < 2:
                continue
            b = tuple(t[idx] for t in data)
            opt.zero_grad()
            step_loss = T.loss(mine(b[0]), b)[0]
            step_loss.backward()
            opt.step()
            total += np.float64(step_loss.detach().item()) * len(idx)
            seen += len(idx)
        means.append(float(total) / seen)
    assert len(history) == epochs and [h["steps"] for h in history] == [2, 2]
    assert [h["train_loss"] for h in history] == means
    a, b = model.state_dict(), mine.state_dict()
    assert list(a) == list(b) and all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)
    assert not torch.equal(a["conv.0.weight"], _tiny()[0].state_dict()["conv.0.weight"])     # the steps moved the model at all


def test_heads_hip_is_refused_by_name_on_the_cpu():
    model, data = _tiny()
    with pytest.raises(ValueError, match="not on a HIP device"):
        T.fit(model, data, data, 4, 0, T.TrainConfig(), heads="hip", max_epochs=1)
    with pytest.raises(ValueError, match="heads must be one of"):
        T.fit(model, data, data, 4, 0, T.TrainConfig(), heads="cuda", max_epochs=1)


def test_metadata_round_trips_with_the_reference_keys(tmp_path):
    base = str(tmp_path)
    gen = T.TrainingGen(created_at=datetime(2024, 5, 6, 7, 8, 9, 123456), gen_n=3, n_mcts_iterations=1400, c_exploration=6.6, c_ply_penalty=0.01,
                        self_play_batch_size=2000, training_batch_size=2000, parent=datetime(2024, 5, 6, 7, 0, 0), val_loss=0.25,
                        solver_score=0.75, solver_n_scored=10, solver_n_unsolved=1, solver_n_skipped=2)
    gen.save_metadata(base)
    with open(tmp_path / "2024-05-06T07:08:09.123456" / "metadata.json") as f:
        d = json.load(f)
    assert tuple(d) == T.REFERENCE_KEYS + T.EXTRA_KEYS
    assert T.REFERENCE_KEYS == ("created_at", "gen_n", "n_mcts_iterations", "c_exploration", "c_ply_penalty", "self_play_batch_size",
                                "training_batch_size", "parent", "val_loss", "solver_score")      # training.py:30-39
    assert d["created_at"] == "2024-05-06T07:08:09.123456" and d["parent"] == "2024-05-06T07:00:00" and d["val_loss"] == 0.25
    assert T.TrainingGen.load(base, gen.created_at) == gen == T.TrainingGen.load_latest(base) and T.TrainingGen.load_all(base) == [gen]
    # the reference's own file (no extras, null optionals) loads
    ref = {k: d[k] for k in T.REFERENCE_KEYS}
    ref.update(parent=None, val_loss=None, solver_score=None)
    got = T.TrainingGen.from_json(json.dumps(ref))
    assert got.parent is None and got.solver_n_scored is None and got.gen_n == 3


def test_load_latest_with_default_creates_generation_zero(tmp_path):
    base = str(tmp_path / "runs")
    with pytest.raises(FileNotFoundError):
        T.TrainingGen.load_latest(base)
    cfg, tc = ModelConfig(1, 16, 2, 2), T.TrainConfig({0: 2e-3, 10: 8e-4}, 4e-4)
    gen = T.TrainingGen.load_latest_with_default(base, 50, 6.6, 0.01, 64, 128, cfg, tc)
    assert gen.gen_n == 0 and gen.parent is None and gen.val_loss is None
    assert gen.get_games(base) is None and gen.get_train_config(base) == tc
    model = gen.get_model(base)
    assert model.config == cfg and not model.training
    assert list(model.state_dict()) == list(ConnectFourNet(cfg).state_dict())
    again = T.TrainingGen.load_latest_with_default(base, 1, 1.0, 1.0, 1, 1, ModelConfig(0, 1, 1, 1))
    assert again == gen                                          # the existing generation, not a new one
    # a later generation is the latest, and its model round-trips bit for bit
    torch.manual_seed(9)
    child_model = ConnectFourNet(cfg)
    child = T.TrainingGen(created_at=datetime.now(), gen_n=1, n_mcts_iterations=50, c_exploration=6.6, c_ply_penalty=0.01, self_play_batch_size=64,
                          training_batch_size=128, parent=gen.created_at, val_loss=1.5)
    child.save_all(base, None, child_model, tc)
    assert T.TrainingGen.load_latest(base) == child and [g.gen_n for g in T.TrainingGen.load_all(base)] == [1, 0]
    loaded = child.get_model(base).state_dict()
    assert all(torch.equal(v, loaded[k]) for k, v in child_model.state_dict().items())


def test_generation_tensors_are_the_reference_split_plus_mirrors():
    from c4a0_amd.results import results_from_records
    from c4a0_amd.session import SAMPLE_DTYPE

    rng = np.random.default_rng(21)
    counts = rng.integers(1, 8, 40).astype(np.uint32)
    n = int(counts.sum())
    recs = np.zeros(n, dtype=SAMPLE_DTYPE)
    recs["mask"] = rng.integers(0, 1 << 42, n, dtype=np.uint64)
    recs["value"] = recs["mask"] & rng.integers(0, 1 << 42, n, dtype=np.uint64)
    recs["policy"] = rng.random((n, 7), dtype=np.float32)
    recs["q_penalty"] = rng.random(n, dtype=np.float32) * 2 - 1
    recs["q_no_penalty"] = np.sign(recs["q_penalty"])
    games = results_from_records(np.stack([np.arange(40, dtype=np.uint64)] * 3, 1), recs, counts)
    train, test = games.split_train_test(0.8, 1337)                       # training.py:207
    got = T.generation_tensors(games, "cpu")
    assert len(train) > 0 and len(test) > 0
    for samples, tensors in ((train, got[0]), (test, got[1])):
        samples = samples + [s.flip_h() for s in samples]                # SampleDataModule.__init__
        want = [np.stack(x) for x in zip(*[s.to_numpy() for s in samples])]
        assert len(tensors) == 4
        for t, w in zip(tensors, want):
            assert t.dtype == torch.float32 and np.array_equal(t.numpy(), w)


@pytest.fixture(scope="module")
def cpu_run():
    return R.run("cpu", "torch")


def test_the_same_seed_gives_the_same_history_and_state_dict_bytes(cpu_run):
    _u, best_val, history, model = cpu_run
    _u2, best_val2, history2, model2 = R.run("cpu", "torch")
    assert history == history2 and best_val == best_val2
    a, b = model.state_dict(), model2.state_dict()
    assert all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)
    assert R.run("cpu", "torch", seed=7)[2] != history


def test_the_loop_learns_on_the_cpu(cpu_run):
    untrained, best_val, history, _model = cpu_run
    print("train_loss", [round(h["train_loss"], 4) for h in history], "val_loss", [round(h["val_loss"], 4) for h in history], "untrained", untrained)
    assert len(history) == R.EPOCHS and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in history)
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[-1]["val_loss"] < untrained
    assert best_val == min(h["val_loss"] for h in history)


def test_lazy_exports():
    import c4a0_amd

    assert c4a0_amd.train_single_gen is T.train_single_gen and c4a0_amd.training_loop is T.training_loop
    assert c4a0_amd.TrainingGen is T.TrainingGen and c4a0_amd.TrainConfig is T.TrainConfig
