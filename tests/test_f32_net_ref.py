"""The f32 evaluator's documented summation order (include/c4a0_hip.h, "f32 evaluator"), restated in plain C
(tests/f32_net_ref.c), against the reference's own outputs and float64 PyTorch -- and the f32 kernels' code shape
(exact-f32 MFMA, no scratch, no spills).  No GPU needed.

Tolerance: 1e-5 absolute on log-probabilities and q.  PyTorch's CPU f32 forward of the same nets differs from float64 by
at most ~3e-7 (measured below on every net of the matrix and asserted), the C restatement by the same order: 1e-5 leaves
a 30x margin for the fixtures, which the reference computed in f32 in its own order, and is the order the issue asks for
(three orders tighter than the bf16 chain's 0.03)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from c4a0_amd.nn import ConnectFourNet, ModelConfig

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import f32_ref as R  # noqa: E402

TOL = 1e-5
# the last two: heads of unequal depth, so no merged first layer and output layers of different widths -- (2, 3, 1, 3): the policy
# output reads the 672 features, the value output its 128-wide hidden layer; (1, 20, 3, 1): policy 864 (hidden), value 1 344 (features)
MATRIX = [(0, 16, 1, 1), (1, 32, 4, 2), (4, 32, 4, 2), (1, 37, 2, 2), (1, 64, 4, 2), (2, 3, 1, 3), (1, 20, 3, 1)]


def random_model(cfg, seed):
    """Default PyTorch initialisation with non-trivial BatchNorm statistics (so that folding matters)."""
    torch.manual_seed(seed)
    m = ConnectFourNet(ModelConfig(*cfg))
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
    return m.eval()


def random_planes(g, seed):
    rng = np.random.default_rng(seed)
    occ, mine = rng.random((g, 42)) < 0.5, rng.random((g, 42)) < 0.5
    p = np.zeros((g, 2, 42), np.float32)
    p[:, 0], p[:, 1] = occ & mine, occ & ~mine
    return p.reshape(g, 2, 6, 7)


def ref_outputs(model, x):
    """The C restatement's (logprobs, q) with a float64 log-softmax / tanh on its f32 pre-activations."""
    v = R.forward(R.pack_on_cpu(model), x)["preact"].astype(np.float64)
    return torch.log_softmax(torch.from_numpy(v[:, :7]), 1).numpy(), np.tanh(v[:, 7:])


def _fixture_models():
    from closed_form_weights import fill_closed_form

    z = np.load(os.path.join(HERE, "golden", "nn_fixture.npz"))
    m = ConnectFourNet(ModelConfig(*[int(v) for v in z["cfg"]]))
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
    yield "nn_fixture", z, m.eval()
    z = np.load(os.path.join(HERE, "golden", "nn_fixture_1x32.npz"))
    m = ConnectFourNet(ModelConfig(*[int(v) for v in z["cfg"]])).eval()
    with torch.no_grad():
        fill_closed_form(m)
    yield "nn_fixture_1x32", z, m


def test_c_reference_matches_the_references_own_outputs():
    for name, z, model in _fixture_models():
        lp, q = ref_outputs(model, z["x"])
        assert np.abs(lp - z["policy_logprobs"]).max() <= TOL, name
        assert np.abs(q[:, 0] - z["q_penalty"]).max() <= TOL and np.abs(q[:, 1] - z["q_no_penalty"]).max() <= TOL, name


@pytest.mark.parametrize("cfg", MATRIX, ids=lambda c: "x".join(map(str, c)))
def test_c_reference_matches_float64_pytorch(cfg):
    model = random_model(cfg, 11)
    x = random_planes(64, 5)
    # both PyTorch forwards on ATen's own convolution (im2col + BLAS, the path float64 takes anyway): oneDNN's f32 kernels
    # pad C = 37 to blocks of 16 channels, and on some CPUs the padding reached the result (spreads of 5e-3 that changed
    # from run to run), which measured oneDNN, not the f32 arithmetic this spread stands for
    mkldnn = torch.backends.mkldnn.enabled
    torch.backends.mkldnn.enabled = False
    (nnpack,) = torch.backends.nnpack.set_flags(False)
    try:
        with torch.no_grad():
            lp32, qa32, qb32 = model(torch.from_numpy(x))
            lp64, qa64, qb64 = model.double()(torch.from_numpy(x).double())
    finally:
        torch.backends.mkldnn.enabled = mkldnn
        torch.backends.nnpack.set_flags(nnpack)
    lp, q = ref_outputs(model.float(), x)
    torch_spread = max(np.abs(lp32.numpy() - lp64.numpy()).max(), np.abs(qa32.numpy() - qa64.numpy()).max())
    assert torch_spread < 1e-6                                   # the f32 spread the tolerance is judged by
    assert np.abs(lp - lp64.numpy()).max() <= TOL
    assert np.abs(q[:, 0] - qa64.numpy()).max() <= TOL and np.abs(q[:, 1] - qb64.numpy()).max() <= TOL


def test_padding_is_exact_zero():
    """Padded channels of the tower and padded hidden features are +0 exactly (zero weights, zero bias, zero inputs)."""
    pk = R.pack_on_cpu(random_model((1, 37, 2, 2), 3))
    r = R.forward(pk, random_planes(9, 1))
    assert pk["cp"] == 48 and pk["hp"] == 1568
    assert not r["features"].reshape(9, 42, 48)[:, :, 37:].any()
    assert not r["policy_hidden"][0][:, 42 * 37:].any()


def test_f32_kernels_use_exact_f32_mfma_without_scratch(tmp_path):
    """Every kernel of c4_f32_net.hip: v_mfma_f32_*_f32 in its code, ScratchSize 0, no VGPR / SGPR spills (hipcc for gfx950)."""
    root = os.path.dirname(HERE)
    src = os.path.join(root, "c4a0_amd", "csrc", "c4_f32_net.hip")
    asm = tmp_path / "f32.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                        "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    remarks = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        remarks[m.group(1)] = m.group(2)
    kernels = [k for k in remarks if "f32_gemm" in k or "f32_head_out" in k]
    assert any("f32_gemm" in k for k in kernels) and any("f32_head_out" in k for k in kernels)
    text = asm.read_text()
    for k in kernels:
        body = remarks[k]
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", body), k
        assert re.search(r"VGPRs Spill: 0\b", body) and re.search(r"SGPRs Spill: 0\b", body), k
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", body).group(1))
        assert occ >= 2, k
        code = text[re.search(r"^" + re.escape(k) + r":", text, re.M).start():]
        code = code[:code.index(".Lfunc_end")]
        assert re.search(r"v_mfma_f32_(16x16x4|32x32x2)_f32", code), k
