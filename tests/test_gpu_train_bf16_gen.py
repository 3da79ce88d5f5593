"""c4a0_amd.train_single_gen(heads="bf16") end to end on a tiny job: self-play, one epoch of bf16 mixed-precision training, and a
generation folder that reads back."""
import math
import os

import pytest
import torch

import c4a0_amd
from c4a0_amd import training as T
from c4a0_amd.nn import ModelConfig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_train_single_gen_with_bf16_heads(tmp_path):
    base = str(tmp_path)
    torch.manual_seed(12)
    config = ModelConfig(1, 32, 2, 2)
    parent = T.TrainingGen.load_latest_with_default(base, 10, 6.6, 0.01, 8, 64, config, T.TrainConfig({0: 2e-3}, 4e-4))
    timings = {}
    gen = c4a0_amd.train_single_gen(base, DEV, parent, n_self_play_games=8, n_mcts_iterations=10, c_exploration=6.6, c_ply_penalty=0.01,
                                    self_play_batch_size=8, training_batch_size=64, heads="bf16", max_epochs=1, timings=timings,
                                    resident_games=8)
    folder = gen.gen_folder(base)
    assert sorted(os.listdir(folder)) == ["games.pkl", "metadata.json", "model.json", "model.pt"]
    assert gen.gen_n == 1 and gen.parent == parent.created_at and timings["epochs"] == 1
    assert T.TrainingGen.load(base, gen.created_at) == gen == T.TrainingGen.load_latest(base)
    child = gen.get_model(base)
    assert child.config == config and math.isfinite(gen.val_loss)
    before = dict(parent.get_model(base).named_parameters())
    for name, p in child.named_parameters():
        assert p.dtype == torch.float32 and bool(torch.isfinite(p).all()), name
    assert any(not torch.equal(p, before[name]) for name, p in child.named_parameters())      # it was trained
