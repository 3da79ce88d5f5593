"""tests/train_out_ref.py, the float64 restatement of the output-layer kernels' contract, against float64 PyTorch autograd of
`ConnectFourNet`'s output layers + `train_common.loss`; the new entry points' declarations; and what needs no GPU of
c4a0_amd/train_out.py."""
import os
import re

import numpy as np
import pytest
import torch

from c4a0_amd import _lib
from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_common import loss
from tests import train_out_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(m: int, k: int, seed: int):
    rng = np.random.default_rng(seed)
    xp, xv = rng.standard_normal((m, k)), rng.standard_normal((m, k))
    t = rng.random((m, 7))
    t[rng.random((m, 7)) < 0.3] = 0.0
    t[:, 3] += 0.05
    t /= t.sum(axis=1, keepdims=True)
    t[0] = 0.0
    t[0, 2] = 1.0                                         # a one-hot target row
    return xp, xv, t, rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)


@pytest.mark.parametrize("k", [8, 40])
@pytest.mark.parametrize("m", [1, 2, 65])
def test_the_reference_equals_float64_autograd_of_the_output_layers_and_the_loss(m, k):
    """the model's own output layers (fc_policy[-2:], fc_value[-2:] of a network without hidden layers whose F is k) in float64"""
    torch.manual_seed(100 * m + k)
    net = ConnectFourNet(ModelConfig(0, 4, 1, 1)).double()
    lin_p, lin_v = torch.nn.Linear(k, 7).double(), torch.nn.Linear(k, 2).double()
    assert isinstance(net.fc_policy[-1], torch.nn.LogSoftmax) and isinstance(net.fc_value[-1], torch.nn.Tanh)
    xp, xv, t, tp, tn = _case(m, k, 7 * m + k)
    txp, txv = torch.tensor(xp, requires_grad=True), torch.tensor(xv, requires_grad=True)
    zp = lin_p(txp)
    zv = lin_v(txv)
    zp.retain_grad()
    zv.retain_grad()
    logp, q = net.fc_policy[-1](zp), net.fc_value[-1](zv)
    # t + EPS is formed in float64 on both sides
    losses = loss((logp, q[:, 0], q[:, 1]), (None, torch.tensor(t), torch.tensor(tp), torch.tensor(tn)))
    upstream = 0.75
    (losses[0] * upstream).backward()
    wp, bp, wv, bv = (p.detach().numpy() for p in (lin_p.weight, lin_p.bias, lin_v.weight, lin_v.bias))
    out, dz, got = ref.forward(xp, xv, wp, bp, wv, bv, t, tp, tn)
    grads = ref.backward(dz, upstream, xp, xv, wp, wv)

    def close(a, b, what):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        assert err <= 1e-12, (what, err)

    close(out, torch.cat([logp, q], dim=1).detach().numpy(), "out")
    close(got, [float(v.detach()) for v in losses], "losses")
    close(dz * upstream, torch.cat([zp.grad, zv.grad], dim=1).numpy(), "dz")
    for g, w, what in zip(grads, (txp.grad, txv.grad, lin_p.weight.grad, lin_p.bias.grad, lin_v.weight.grad, lin_v.bias.grad),
                          ("dxp", "dxv", "dwp", "dbp", "dwv", "dbv")):
        close(g, w.numpy(), what)


def test_the_second_stage_adds_eight_groups_in_order():
    part = np.arange(1.0, 20.0)[:, None]                   # 19 chunks
    groups = [sum(part[c, 0] for c in range(g, 19, 8)) for g in range(8)]
    assert ref.second_stage(part)[0] == sum(groups) and ref.second_stage(part[:1])[0] == 1.0
    assert ref.chunk_sums(np.ones((130, 2))).tolist() == [[64.0, 64.0], [64.0, 64.0], [2.0, 2.0]]
    assert ref.work_bytes(1, 8) == 4 * 84 and ref.work_bytes(2000, 1344) == 4 * 32 * (9 * 1344 + 12) and ref.work_bytes(2000, 8) == 4 * (8000 + 128)


def test_new_entry_points_are_bound_with_the_headers_argument_counts():
    hdr = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    for name in ("c4_train_out_work_bytes", "c4_train_out_chunk_rows", "c4_train_out_loss_fwd", "c4_train_out_loss_bwd"):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)", hdr, flags=re.M | re.S)
        assert decl is not None, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).strip()
        n_args = 0 if args == "void" else args.count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, (name, n_args)
    assert len(_lib.SIGNATURES["c4_train_out_loss_fwd"][1]) == 19 and len(_lib.SIGNATURES["c4_train_out_loss_bwd"][1]) == 21
    assert "#define C4_ABI_VERSION 14" in hdr and _lib.ABI_VERSION == 14       # functions were only added
    assert f"#define C4_TRAIN_OUT_CHUNK_ROWS {_lib.OUT_CHUNK_ROWS}" in hdr and _lib.OUT_CHUNK_ROWS == ref.CHUNK
    assert "training: the output layers and the loss" in hdr


def test_outputs_hip_is_refused_by_name_on_a_cpu_model():
    from c4a0_amd import train_out
    from c4a0_amd import training as T

    model = ConnectFourNet(ModelConfig(0, 4, 1, 1))
    assert train_out.OUTPUTS == ("auto", "torch", "hip") and train_out.AUTO_OUTPUTS == "torch"
    assert "not on a HIP device" in train_out.out_refusal(model)
    with pytest.raises(ValueError, match='outputs="hip".*not on a HIP device'):
        train_out.resolve_outputs(model, "hip")
    with pytest.raises(ValueError, match="outputs must be one of"):
        train_out.resolve_outputs(model, "cuda")
    assert train_out.resolve_outputs(model, "auto") == "torch" and train_out.resolve_outputs(model, "torch") == "torch"
    data = (torch.zeros(4, 2, 6, 7), torch.full((4, 7), 1 / 7), torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="not on a HIP device"):
        T.fit(model, data, data, 4, 0, T.TrainConfig(), outputs="hip", max_epochs=1)
    with pytest.raises(ValueError, match="not on a HIP device"):
        T.loss_train(model, data, outputs="hip")


def test_loss_train_with_the_stock_outputs_is_loss_of_the_model_on_the_cpu():
    from c4a0_amd import training as T

    torch.manual_seed(2)
    model = ConnectFourNet(ModelConfig(1, 4, 2, 2)).train()
    rng = np.random.default_rng(2)
    data = (torch.tensor(rng.integers(0, 2, (6, 2, 6, 7)).astype(np.float32)), torch.full((6, 7), 1 / 7), torch.zeros(6), torch.ones(6))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    got = T.loss_train(model, data)
    model.load_state_dict(state)                           # the running statistics moved
    want = loss(model(data[0]), data)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
