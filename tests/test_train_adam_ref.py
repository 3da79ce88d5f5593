"""What needs no GPU of the fused Adam and the graphed training step: tests/adam_ref.py (the float64 restatement of the kernel's
contract) pinned to torch.optim.Adam in float64, the binding of the new entry points, and `fit`'s new arguments -- refusals by name,
and the stock path's bytes unchanged."""
import os
import re

import numpy as np
import pytest
import torch

from c4a0_amd import _lib
from c4a0_amd import training as T
from tests import adam_ref
from tests import train_recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 3, 4, 5, 7, 1023, 1025)
LR, WD, STEPS = 2e-3, 4e-4, 20


@pytest.mark.parametrize("foreach", [False, True])
def test_adam_ref_is_torch_adam_in_float64(foreach):
    rng = np.random.default_rng(7)
    params = [rng.standard_normal(n) for n in LENGTHS]
    # gradients from 1e-6 to 10 in magnitude, either sign, fresh every step
    grads = [[rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 1.0, n) for n in LENGTHS] for _ in range(STEPS)]
    tensors = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    opt = torch.optim.Adam(tensors, lr=LR, weight_decay=WD, foreach=foreach)
    for step in grads:
        for t, g in zip(tensors, step):
            t.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    worst = 0.0
    for i, (p0, t) in enumerate(zip(params, tensors)):
        p, m, v = adam_ref.adam_steps(p0, [step[i] for step in grads], LR, weight_decay=WD)
        state = opt.state[t]
        assert int(state["step"]) == STEPS
        for mine, theirs in ((p, t.detach().numpy()), (m, state["exp_avg"].numpy()), (v, state["exp_avg_sq"].numpy())):
            rel = np.abs(mine - theirs) / np.abs(theirs)
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-10, (LENGTHS[i], float(rel.max()))
    print("worst relative difference:", worst)


def test_adam_ref_takes_the_step_before_the_call_and_skips_a_zero_weight_decay():
    p, g, m, v = np.array([np.inf, 1.0]), np.array([0.5, 0.0]), np.zeros(2), np.zeros(2)
    p2, m2, v2 = adam_ref.adam_step(p, g, m, v, 0, 1e-3)          # weight_decay == 0: p is not multiplied, an infinite p stays
    assert p2[0] == np.inf and m2[0] == pytest.approx(0.05) and v2[0] == pytest.approx(0.00025)
    assert (p2[1], m2[1], v2[1]) == (1.0, 0.0, 0.0)                # a zero gradient on a zero state moves nothing
    assert adam_ref.pow_u32(0.9, 1000) == pytest.approx(0.9 ** 1000, rel=1e-12)
    # step t = t_before + 1: the first call's step size is lr, whatever the gradient's size
    assert adam_ref.adam_step([0.0], [3.0], [0.0], [0.0], 0, 1e-3)[0][0] == pytest.approx(-1e-3, rel=1e-6)


def test_new_entry_points_are_bound_with_the_headers_argument_counts():
    hdr = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    for name in ("c4_train_adam_f32", "c4_train_adam_block_elems"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", hdr, flags=re.M | re.S)
        assert decl is not None, name
        args = decl.group(1).strip()
        n_args = 0 if args == "void" else args.count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args)
    assert "#define C4_ABI_VERSION 14" in hdr and _lib.ABI_VERSION == 14       # functions were only added
    assert f"#define C4_ADAM_BLOCK_ELEMS {_lib.ADAM_BLOCK_ELEMS}" in hdr
    import ctypes as C

    assert C.sizeof(_lib.AdamSegment) == 48 and _lib.AdamSegment.n.offset == 32 and _lib.AdamSegment.first_block.offset == 40


def test_adam_table_lays_segments_out_as_the_header_says():
    from c4a0_amd.train_graph import adam_table

    table, n_blocks = adam_table([(16, 32, 48, 64, 1), (1600, 3200, 4800, 6400, 4096), (160, 320, 480, 640, 4097)])
    assert n_blocks == 1 + 1 + 2 and table.dtype == np.uint8 and table.size == 3 * 48
    rows = np.frombuffer(table.tobytes(), dtype=np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<u8"),
                                                          ("first_block", "<u4"), ("reserved", "<u4")]))
    assert rows["first_block"].tolist() == [0, 1, 2] and rows["n"].tolist() == [1, 4096, 4097] and rows["v"].tolist() == [64, 6400, 640]
    with pytest.raises(ValueError, match="16-byte aligned"):
        adam_table([(16, 32, 52, 64, 8)])
    with pytest.raises(ValueError, match="n >= 1"):
        adam_table([(16, 32, 48, 64, 0)])


def test_graph_and_hip_optimizer_are_refused_by_name_without_a_gpu():
    student, train, val = R.problem()
    with pytest.raises(ValueError, match="graph=True: the model is on cpu, not on a HIP device"):
        T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, graph=True)
    with pytest.raises(ValueError, match='graph=True needs optimizer="hip"'):
        T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, graph=True, optimizer="torch")
    with pytest.raises(ValueError, match='optimizer="hip": the model is on cpu'):
        T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, optimizer="hip")
    with pytest.raises(ValueError, match="optimizer must be one of"):
        T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, max_epochs=1, optimizer="sgd")
    from c4a0_amd.train_graph import resolve_optimizer

    assert resolve_optimizer("auto", False) == "torch" and resolve_optimizer("auto", True) == "hip" and resolve_optimizer("hip", False) == "hip"


def test_the_stock_path_keeps_its_bytes_under_the_new_arguments():
    _u, best_a, hist_a, model_a = R.run("cpu", "torch")
    student, train, val = R.problem()
    _best, best_b, hist_b = T.fit(student, train, val, R.BATCH, 1, R.TRAIN_CONFIG, seed=1337, heads="torch", max_epochs=R.EPOCHS,
                                  optimizer="torch", graph=False)
    assert hist_a == hist_b and best_a == best_b
    sa, sb = model_a.state_dict(), student.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].numpy().tobytes() == sb[k].numpy().tobytes(), k
