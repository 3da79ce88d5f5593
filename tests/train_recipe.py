"""The small learning problem of the training tests (test infrastructure; tests/test_train_loop.py runs it on the CPU,
tests/test_gpu_train_gen.py on the GPU): a student ConnectFourNet(ModelConfig(1, 16, 2, 2)) learns the answers of a teacher of the
same architecture whose output layers are scaled by 8 (peaked policies, q away from 0) on 1 024 training and 256 validation inputs
of two random disjoint binary planes; Adam 2e-3, l2 4e-4, batch 128, 4 epochs.

Measured on the stock-PyTorch path on a CPU (heads="torch", seed 1337): training loss per epoch 0.58 -> 0.43 -> 0.26 -> 0.16,
val_loss 0.30 -> 0.35 -> 0.24 -> 0.21, the untrained student 0.48.  The tests ask for two conditions: the last epoch's mean
training loss below the first's, the final val_loss below the untrained model's."""
import copy

import numpy as np
import torch

from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.training import TrainConfig, evaluate_loss, fit

CONFIG = ModelConfig(1, 16, 2, 2)
TRAIN_CONFIG = TrainConfig({0: 2e-3}, 4e-4)
N_TRAIN, N_VAL, BATCH, EPOCHS = 1024, 256, 128, 4


def planes(n: int, rng) -> torch.Tensor:
    """two random disjoint binary planes per input: every cell empty, mine or the opponent's"""
    cell = rng.integers(0, 3, (n, 6, 7))
    return torch.from_numpy(np.stack([cell == 1, cell == 2], axis=1).astype(np.float32))


def problem(seed: int = 1337):
    """(student, train, val) on the CPU; the same for a seed"""
    torch.manual_seed(seed)
    student, teacher = ConnectFourNet(CONFIG), ConnectFourNet(CONFIG).eval()
    with torch.no_grad():
        for layer in (teacher.fc_policy[-2], teacher.fc_value[-2]):
            layer.weight.mul_(8.0)
            layer.bias.mul_(8.0)
    rng = np.random.default_rng(seed)
    sets = []
    for n in (N_TRAIN, N_VAL):
        pos = planes(n, rng)
        with torch.no_grad():
            logp, q_pen, q_nopen = teacher(pos)
        sets.append((pos, logp.exp().contiguous(), q_pen.contiguous(), q_nopen.contiguous()))
    return student, sets[0], sets[1]


def run(device, heads: str, dtype=torch.float32, seed: int = 1337):
    """The recipe on `device`: (untrained val_loss, best_val_loss, history, trained model)."""
    student, train, val = problem(seed)
    student = student.to(device=device, dtype=dtype)
    train = tuple(t.to(device=device, dtype=dtype) for t in train)
    val = tuple(t.to(device=device, dtype=dtype) for t in val)
    untrained = evaluate_loss(copy.deepcopy(student), val, BATCH)
    _best, best_val, history = fit(student, train, val, BATCH, 1, TRAIN_CONFIG, seed=seed, heads=heads, max_epochs=EPOCHS)
    return untrained, best_val, history, student
