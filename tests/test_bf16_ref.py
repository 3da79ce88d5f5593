"""CPU checks of tests/bf16_ref.py, the float64 restatement of the bf16 evaluator chain, and of the exact-grid data the GPU
tests (tests/test_gpu_bf16_exact.py) feed the kernels: the reference agrees with PyTorch's own float64 conv2d / linear on the
model's layout, the data meets the exactness precondition and covers what it must, and every plausible kernel bug of
bf16_ref.MUTATIONS changes the reference's answer on exactly those inputs (so the bit-for-bit GPU comparison would catch it).
The GPU tests' inputs are used as row / board prefixes here: rows are independent, and the GPU test re-checks the precondition
at full size."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import bf16_ref as R

M_CPU = 256      # GEMM rows checked here (a prefix of the GPU test's 4 096)
N_CPU = 64       # boards checked here (a prefix of the GPU test's 2 049)


def _model_side(model, planes):
    """The bf16 chain restated on the MODEL's layout: NCHW float64 conv2d, "c h w" flattening, F.linear with the model's own
    (BN-folded) weights -- rounded at the same points.  Independent of the packing and of the column permutation."""
    from c4a0_amd.nn import _fold_bn

    r = lambda t: R.bf16(t)
    d = lambda t: t.detach().double()
    x = r(F.conv2d(planes.double(), d(model.conv[0].weight), d(model.conv[0].bias), padding=1))
    for blk in list(model.conv)[1:]:
        c1, c2, bn = blk.block[0], blk.block[1], blk.block[2]
        t = r(F.conv2d(x, d(c1.weight).bfloat16().double(), d(c1.bias), padding=1))
        w2, b2 = _fold_bn(c2.weight, c2.bias, bn)
        x = r(x + torch.relu(F.conv2d(t, w2.double().bfloat16().double(), b2.double(), padding=1)))
    feat = x.reshape(x.shape[0], -1)
    outs = []
    for seq in (model.fc_policy, model.fc_value):
        h = feat
        for m in list(seq)[:-2]:
            w, b = _fold_bn(m[0].weight, m[0].bias, m[1])
            h = r(torch.relu(F.linear(h, w.bfloat16().double(), b.bfloat16().double())))
        out = list(seq)[-2]
        outs.append((h, F.linear(h, d(out.weight).bfloat16().double(), d(out.bias).float().double())))
    return outs


@pytest.mark.parametrize("blocks,channels", R.EVAL_SHAPES + [(2, 32), (1, 64)])
def test_reference_matches_float64_torch_on_the_models_layout(blocks, channels):
    model = R.eval_model(blocks, channels)
    planes = R.grid_planes(N_CPU, seed=3)
    ops = R.operands_from_model(model)          # packed tower, permuted + bf16 hidden weights: what the kernels see
    p, v = R.hidden(planes, ops)
    (hp, lp), (hv, lv) = _model_side(model, planes.double())
    assert torch.equal(p, hp) and torch.equal(v, hv)
    assert torch.equal(R.head_preact(p, v, ops), torch.cat([lp, lv], dim=1))


def test_unpack_inverts_the_packing():
    for c in (32, 64):
        planes, ops = R.tower_case(c, 2, n=4)
        w0, ws = R.unpack_tower(ops["tw0"], ops["tw"], c)     # asserts the round trip itself
        cw, _ = R.grid_tower_weights(c, 2, seed=100 * c + 2, per_row=R.tower_per_row(2))
        assert torch.equal(w0, cw[0].double()) and all(torch.equal(a, b.double()) for a, b in zip(ws, cw[1:]))


def test_directed_rounding_and_interval():
    t = torch.tensor([1.0, 1.0 + 2 ** -9, -(1.0 + 2 ** -9), 3.0 * 2 ** -140, 0.0, 255.5], dtype=torch.float64)
    lo, hi = R.bf16_directed(t, False), R.bf16_directed(t, True)
    assert lo.tolist() == [1.0, 1.0, -(1.0 + 2 ** -7), 0.0, 0.0, 255.0]
    assert hi.tolist() == [1.0, 1.0 + 2 ** -7, -1.0, 2.0 ** -133, 0.0, 256.0]     # 2^-133: bf16's smallest subnormal
    # the bound contains the f32 chain of any order: a sequential f32 sum and a pairwise one of the same products
    x, w, b = R.realistic_linear(8, 1344, 192, seed=1)
    lo, hi = R.interval(x, w, b, relu=False)
    prod = x.float()[:, None, :] * w.float()[None, :, :]             # exact products in f32
    seq = torch.zeros(8, 192)
    for k in range(0, 1344, 64):
        seq = seq + prod[..., k:k + 64].sum(-1)
    for y in (seq + b, prod.sum(-1) + b):
        yb = y.bfloat16().double()
        assert bool(((lo <= yb) & (yb <= hi)).all())


@pytest.mark.parametrize("k,n", R.GEMM_SHAPES)
def test_gemm_data_is_exact_and_covers(k, n):
    x, w, b = R.gemm_case(k, n)
    # the precondition at the GPU test's full size, from the generator's bounds (no 4 096-row float64 GEMM on the CPU) ...
    unit = R.lowest_bit(x.double()) * R.lowest_bit(w.double())
    unit = min(unit, R.lowest_bit(b.double()))
    worst = (w.double().abs().sum(1) * x.double().abs().max() + b.double().abs()).max()   # any row with |x| <= max |x|
    assert worst < 2.0 ** 24 * unit
    # ... and measured on the prefix, with the data's coverage
    st = {}
    y = R.linear(x[:M_CPU], w, b, relu=False, stats=st)
    down, up = st["ties"][0]
    assert down >= 100 and up >= 100, (down, up)
    assert bool((w != 0).any(0).all()), "a k index without any nonzero weight"
    assert bool((x[:M_CPU] != 0).any(0).all())
    assert (y < 0).any() and (y > 0).any()


@pytest.mark.parametrize("channels", [32, 64])
@pytest.mark.parametrize("blocks", R.TOWER_BLOCKS)
def test_tower_data_is_exact_and_covers(channels, blocks):
    planes, ops = R.tower_case(channels, blocks, n=N_CPU)
    st = {}
    R.tower(planes, ops, stats=st)          # check=True: the precondition, layer by layer
    down = sum(t[0] for t in st["ties"])
    up = sum(t[1] for t in st["ties"])
    assert down >= 100 and up >= 100, (down, up)
    # edge cells see nonzero neighbours along every tap: each of the 9 taps of each border cell hits a set plane somewhere
    occ = F.pad((planes.double() != 0).any(1).double(), (1, 1, 1, 1))
    for dr in range(3):
        for dc in range(3):
            nb = occ[:, dr:dr + 6, dc:dc + 7].any(0)
            on_board = torch.zeros(6, 7, dtype=torch.bool)
            on_board[max(0, 1 - dr):6 - max(0, dr - 1), max(0, 1 - dc):7 - max(0, dc - 1)] = True
            assert bool(nb[on_board].all()), (dr, dc)
    w0, ws = R.unpack_tower(ops["tw0"], ops["tw"], channels)
    assert bool((w0.reshape(channels, -1) != 0).any(0).all())
    if R.tower_per_row(blocks) == 0:   # every (ci, tap) column of every layer has a nonzero weight
        for w in ws:
            assert bool((w.reshape(channels, -1) != 0).any(0).all())
    for i, s1 in enumerate(st.get("conv1", [])):
        assert float((s1 < 0).double().mean()) > 0.2, f"block {i}: conv1 outputs must include negative values"
    for i, f in enumerate(st.get("changed", [])):
        assert f > 0.03, f"block {i} changes only {f:.3f} of the stream"


def _differs(a, b):
    return not torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _tower_good(channels, blocks):
    planes, ops = R.tower_case(channels, blocks, n=N_CPU)
    return planes, ops, R.tower(planes, ops, check=False)


@functools.lru_cache(maxsize=None)
def _gemm_good(k, n, relu):
    x, w, b = R.gemm_case(k, n, m=M_CPU)
    return x, w, b, R.linear(x, w, b, relu, check=False)


TOWER_MUTATIONS = ["trunc", "away", "relu1", "bias_last", "edge_tap", "wrap", "no_residual"]
GEMM_MUTATIONS = ["trunc", "away", "bias_last", "drop_ktile", "row_offset"]


@pytest.mark.parametrize("mut", TOWER_MUTATIONS)
@pytest.mark.parametrize("channels,blocks", [(32, 2), (64, 8), (32, 1)])
def test_tower_mutations_are_detected(mut, channels, blocks):
    planes, ops, good = _tower_good(channels, blocks)
    assert _differs(R.tower(planes, ops, {mut}, check=False), good), R.MUTATIONS[mut]


@pytest.mark.parametrize("mut", GEMM_MUTATIONS)
@pytest.mark.parametrize("k,n", R.GEMM_SHAPES)
def test_gemm_mutations_are_detected(mut, k, n):
    for relu in (False, True):
        x, w, b, good = _gemm_good(k, n, relu)
        assert _differs(R.linear(x, w, b, relu, {mut}, check=False), good), (R.MUTATIONS[mut], relu)


@pytest.mark.parametrize("blocks,channels", R.EVAL_SHAPES)
def test_permutation_mutation_is_detected(blocks, channels):
    ops = R.operands_from_model(R.eval_model(blocks, channels))
    planes = R.grid_planes(32, seed=3)
    p, v = R.hidden(planes, ops, check=False)
    pm, vm = R.hidden(planes, ops, {"no_perm"}, check=False)
    assert _differs(p, pm) and _differs(v, vm)


def test_generators_refuse_to_be_inexact():
    """The precondition check fails loudly when data leaves the exact range."""
    x = torch.full((2, 64), 2.0 ** 20, dtype=torch.float64)
    w = torch.full((192, 64), 1.0, dtype=torch.float64)
    with pytest.raises(AssertionError, match="precondition"):
        R.linear(x, w, torch.full((192,), 2.0 ** -30, dtype=torch.float64), relu=False)
