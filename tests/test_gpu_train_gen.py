"""A generation on the GPU: the learning recipe of tests/train_recipe.py with the heads' hidden blocks on the HIP kernels, and
c4a0_amd.train_single_gen end to end."""
import math
import os

import numpy as np
import pytest
import torch

import c4a0_amd
from c4a0_amd import training as T
from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig
from tests import train_recipe as R
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def test_the_loop_learns_with_hip_heads_and_tracks_the_torch_path():
    untrained, best_val, history, _model = R.run(DEV, "hip")
    _u, _b, stock, _m = R.run(DEV, "torch")
    _u64, _b64, truth, _m64 = R.run("cpu", "torch", dtype=torch.float64)
    val = {name: [h["val_loss"] for h in hist] for name, hist in (("hip", history), ("torch", stock), ("float64", truth))}
    print("val_loss per epoch:", val, "train_loss (hip):", [h["train_loss"] for h in history], "untrained:", untrained)
    evidence(f"train recipe val_loss per epoch: hip {val['hip']}, torch {val['torch']}, float64 {val['float64']}")
    assert len(history) == R.EPOCHS and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in history)
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[-1]["val_loss"] < untrained
    assert best_val == min(val["hip"])
    # the two f32 paths against the float64 run of the same recipe and seed: the 4 x rule, epoch by epoch
    for e in range(R.EPOCHS):
        e_hip, e_torch = abs(val["hip"][e] - val["float64"][e]), abs(val["torch"][e] - val["float64"][e])
        assert e_hip <= max(4 * e_torch, 4 * U * abs(val["float64"][e])), (e, e_hip, e_torch)


def test_train_single_gen_end_to_end(tmp_path):
    base = str(tmp_path)
    torch.manual_seed(11)
    parent = T.TrainingGen.load_latest_with_default(base, 30, 6.6, 0.01, 64, 256, ModelConfig(1, 32, 2, 2), T.TrainConfig({0: 2e-3}, 4e-4))
    timings = {}
    gen = c4a0_amd.train_single_gen(base, DEV, parent, n_self_play_games=64, n_mcts_iterations=30, c_exploration=6.6, c_ply_penalty=0.01,
                                    self_play_batch_size=64, training_batch_size=256, heads="hip", max_epochs=3, timings=timings,
                                    resident_games=64)
    folder = gen.gen_folder(base)
    assert sorted(os.listdir(folder)) == ["games.pkl", "metadata.json", "model.json", "model.pt"]
    assert gen.gen_n == 1 and gen.parent == parent.created_at and gen.solver_score is None
    assert T.TrainingGen.load_latest(base) == gen and [g.gen_n for g in T.TrainingGen.load_all(base)] == [1, 0]
    games = gen.get_games(base)
    assert len(games) == 64
    child = gen.get_model(base)
    assert child.config == ModelConfig(1, 32, 2, 2) and gen.get_train_config(base) == T.TrainConfig({0: 2e-3}, 4e-4)
    # val_loss is the loss of the saved model on the validation tensors
    _train, val = T.generation_tensors(games, DEV)
    assert timings["epochs"] == 3 and timings["val_samples"] == val[0].shape[0] > 0
    again = T.evaluate_loss(child.to(DEV), val, 256)
    assert math.isfinite(gen.val_loss) and gen.val_loss == pytest.approx(again, rel=1e-6)
    # the child plays, and not as the parent does
    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(32)]
    by_child = c4a0_amd.play_games(reqs, 32, 30, 6.6, 0.01, evaluator=InferenceNet(child, DEV), resident_games=32)
    by_parent = c4a0_amd.play_games(reqs, 32, 30, 6.6, 0.01, evaluator=InferenceNet(parent.get_model(base), DEV), resident_games=32)
    assert len(by_child) == 32
    assert by_child.to_records()[0].tobytes() != by_parent.to_records()[0].tobytes()
