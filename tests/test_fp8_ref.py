"""CPU checks of the fp8 hidden layers' pure parts: c4a0_amd.nn.to_fp8_e4m3 / quantize_head_weights / calibration_positions
against tests/fp8_ref.py (the float64 restatement of include/c4a0_hip.h's "fp8 hidden layers", with a q8 in integer arithmetic of
its own), and of the exact-grid data tests/test_gpu_fp8_exact.py feeds the kernels: it meets the exactness precondition, holds the
shares of ties, saturated values and e4m3 subnormals it must, and every plausible kernel bug of fp8_ref.MUTATIONS changes the
reference's answer on exactly those inputs (so the bit-for-bit GPU comparison would catch it)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import fp8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_CPU = 300


def test_to_fp8_equals_the_reference_on_every_code():
    from c4a0_amd.nn import to_fp8_e4m3

    codes = torch.arange(256, dtype=torch.uint8)
    vals = R.decode(codes)
    back_ref, back = R.q8(vals), to_fp8_e4m3(vals.float())
    want = codes.clone()
    want[0xFF] = 0x7F                                            # both NaN codes come back as 0x7F
    assert torch.equal(back_ref, want) and torch.equal(back, want)


def test_to_fp8_rounds_every_midpoint_to_even():
    from c4a0_amd.nn import to_fp8_e4m3

    pos = R.decode(torch.arange(0x7F, dtype=torch.uint8))        # 0 .. 448 ascending
    mid = (pos[:-1] + pos[1:]) / 2                               # exact in f32: one more significand bit
    even = torch.where(torch.arange(0x7E) % 2 == 0, torch.arange(0x7E), torch.arange(1, 0x7F)).to(torch.uint8)
    for sign, bit in ((1.0, 0), (-1.0, 0x80)):
        assert torch.equal(R.q8(sign * mid), even | bit)
        assert torch.equal(to_fp8_e4m3((sign * mid).float()), even | bit)
    # and a hair to either side of a midpoint goes to the nearer code
    lo, hi = mid.float().double() * (1 - 2.0 ** -20), mid.float().double() * (1 + 2.0 ** -20)
    for t, want in ((lo.float(), torch.arange(0x7E)), (hi.float(), torch.arange(1, 0x7F))):
        assert torch.equal(R.q8(t.double()), want.to(torch.uint8)) and torch.equal(to_fp8_e4m3(t), want.to(torch.uint8))


def test_to_fp8_edges():
    from c4a0_amd.nn import to_fp8_e4m3

    t = torch.tensor([448.0, -448.0, 449.0, -449.0, 1e9, -1e9, 2.0 ** -10, -(2.0 ** -10), 0.0, -0.0, float("nan"), float("inf"), -float("inf"),
                      2.0 ** -9, 1.5 * 2.0 ** -10, 2.0 ** -140])
    want = torch.tensor([0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0xFE, 0x00, 0x80, 0x00, 0x80, 0x7F, 0x7E, 0xFE, 0x01, 0x01, 0x00], dtype=torch.uint8)
    assert torch.equal(R.q8(t.double()), want)
    assert torch.equal(to_fp8_e4m3(t), want)


def test_to_fp8_equals_the_reference_on_random_f32():
    from c4a0_amd.nn import to_fp8_e4m3

    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-2 ** 31, 2 ** 31, (200_000,), generator=g, dtype=torch.int64).to(torch.int32)
    t = bits.view(torch.float32)
    t = torch.cat([t, torch.randn(100_000, generator=g) * torch.exp2(torch.randint(-12, 10, (100_000,), generator=g).float())])
    assert torch.equal(R.q8(t.double()), to_fp8_e4m3(t))


def test_quantize_head_weights_follows_the_row_rule():
    from c4a0_amd.nn import quantize_head_weights, to_fp8_e4m3

    g = torch.Generator().manual_seed(11)
    w = torch.randn(12, 128, generator=g) * torch.exp2(torch.randint(-20, 8, (12, 1), generator=g).float())
    w[3] = 0                                                     # an all-zero row
    w[5] = w[5].clamp(-0.4, 0.4)
    w[5, 17] = 448.0 * 2.0 ** -9                                 # a row whose max is exactly 448 2^-e
    w[6] = w[6].clamp(-0.4, 0.4)
    w[6, 3] = -(448.0 * 2.0 ** -9) * (1 + 2.0 ** -23)            # ... and one ulp above it
    wq, e = quantize_head_weights(w)
    assert wq.dtype == torch.uint8 and wq.shape == w.shape and e.shape == (12,)
    assert int(e[3]) == 0 and not bool(wq[3].any())
    assert int(e[5]) == 9 and int(wq[5, 17]) == 0x7E
    assert int(e[6]) == 8
    for n in range(12):
        amax = float(w[n].double().abs().max())
        if amax == 0:
            continue
        en = int(e[n])
        assert -64 <= en <= 64
        assert amax * 2.0 ** en <= 448.0 and (en == 64 or amax * 2.0 ** (en + 1) > 448.0)
        assert torch.equal(wq[n], R.q8((w[n].double() * 2.0 ** en)))
        assert torch.equal(wq[n], to_fp8_e4m3((w[n].double() * 2.0 ** en).float()))
    # range is adapted, never precision: the largest element of a row lands in the top binade
    top = R.decode(wq).abs().amax(dim=1)
    assert bool(((top >= 224) | (top == 0)).all())


def test_activation_exponent_rule():
    from c4a0_amd.nn import activation_exponent

    assert activation_exponent(0.0) == 0 and activation_exponent(float("nan")) == 0
    for a in (1.0, 224.0, 224.5, 3.0e-5, 7.25, 1234.0):
        e = activation_exponent(a)
        assert 2 * a * 2.0 ** e <= 448.0 < 2 * a * 2.0 ** (e + 1)


def test_calibration_positions_are_deterministic_and_legal():
    from c4a0_amd.api import _positions_array
    from c4a0_amd.nn import calibration_positions, positions_to_planes
    from tests.helpers import planes_to_pos_np

    a, b = calibration_positions(4096, 0), calibration_positions(4096, 0)
    assert a.dtype == np.uint64 and a.shape == (4096, 2) and np.array_equal(a, b)
    assert not np.array_equal(a, calibration_positions(4096, 1))
    assert np.array_equal(calibration_positions(100, 0), a[:100])
    _positions_array(a)                                          # raises on a position no game can show
    plies = np.array([bin(int(m)).count("1") for m in a[:, 0]])
    assert plies.min() == 0 and plies.max() >= 36                # all plies: from the empty board to nearly full ones
    planes = positions_to_planes(a)
    assert planes.shape == (4096, 2, 6, 7) and planes.dtype == np.float32
    mask, value = planes_to_pos_np(planes)
    assert np.array_equal(np.asarray(mask, dtype=np.uint64), a[:, 0]) and np.array_equal(np.asarray(value, dtype=np.uint64), a[:, 1])


def test_fp8_heads_refuse_a_cpu_device():
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    model = ConnectFourNet(ModelConfig(1, 32, 4, 2))
    with pytest.raises(ValueError, match="HIP device"):
        InferenceNet(model, torch.device("cpu"), head_dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="head_dtype"):
        InferenceNet(model, torch.device("cpu"), head_dtype=torch.float16)


def test_grouped_nets_and_native_loop_refuse_fp8_heads():
    from c4a0_amd.api import _native_loop_refusal
    from c4a0_amd.nn import GroupedNets, InferenceNet

    net = InferenceNet.__new__(InferenceNet)                     # no device: only the attribute the refusals read first
    net.head_dtype = torch.float8_e4m3fn
    assert "fp8 hidden layers run through the Python host loop" in _native_loop_refusal(net, None, None, None)
    assert "fp8 hidden layers run through the Python host loop" in GroupedNets.refusal({1: net})


def test_entry_points_are_declared_and_the_abi_number_stays():
    from c4a0_amd import _lib

    header = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    for name in ("c4_linear_fp8", "c4_quantize_bf16_fp8"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+C4_ABI_VERSION\s+14\b", header) and _lib.ABI_VERSION == 14
    assert len(_lib.SIGNATURES["c4_linear_fp8"][1]) == 15 and len(_lib.SIGNATURES["c4_quantize_bf16_fp8"][1]) == 8


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' data
@functools.lru_cache(maxsize=None)
def _case(k, n):
    return R.gemm_case(k, n, M_CPU)


@functools.lru_cache(maxsize=None)
def _true(k, n, relu, out_fp8):
    x8, wq, dq, bias, s = _case(k, n)
    stats = {}
    return R.linear(x8, wq, dq, bias, k, relu, out_fp8, s, stats=stats), stats


@pytest.mark.parametrize("k,n", R.SMALL_SHAPES + R.LARGE_SHAPES)
def test_grid_outputs_hold_the_shares(k, n):
    """Conditions on the INPUTS: at least 1 % ties, 1 % saturated values and 1 % e4m3 subnormals before the output rounding (the
    reference asserts along the way that every sum and every v is an exact f32)."""
    for relu in (False, True):
        _, stats = _true(k, n, relu, True)
        tie, sat, sub = R.shares(stats["pre_round"])
        assert tie >= 0.01 and sat >= 0.01 and sub >= 0.01, (k, n, relu, tie, sat, sub)


def test_grid_partial_sums_are_exact_in_any_order():
    from tests.bf16_ref import check_exact

    for k, n in R.SMALL_SHAPES + R.LARGE_SHAPES:
        x8, wq, dq, bias, _ = _case(k, n)
        x, w = R.decode(x8[:, :k]), R.decode(wq)
        assert bool((x == x.round()).all()) and bool((w == w.round()).all()) and float(x.abs().max()) <= 8 and float(w.abs().max()) <= 8
        b_int = bias.double() / dq.double()
        assert bool((b_int == b_int.round()).all())
        check_exact(x, w, torch.zeros(n, dtype=torch.float64), x.abs() @ w.abs().t() + b_int.abs(), f"fp8 grid {k} x {n}")
        assert bool((x8[:, k:] >= 0x7E).all()) and x8.shape[1] == k + R.PAD     # the sentinel columns: NaN and 448


@pytest.mark.parametrize("name", sorted(R.MUTATIONS))
def test_every_mutation_changes_an_output(name):
    """... of the GPU tests' inputs, in at least one (shape, relu, output mode) the GPU test runs."""
    mut = frozenset([name])
    changed = []
    for k, n in R.SMALL_SHAPES + [(1344, 1344)]:
        x8, wq, dq, bias, s = _case(k, n)
        for relu in (False, True):
            for out_fp8 in (True, False):
                want, _ = _true(k, n, relu, out_fp8)
                got = R.linear(x8, wq, dq, bias, k, relu, out_fp8, s, mut=mut)
                same = torch.equal(got, want) if out_fp8 else bool(((got == want) | (got.isnan() & want.isnan())).all())
                if not same:
                    changed.append((k, n, relu, out_fp8))
    assert changed, f"mutation {name!r} ({R.MUTATIONS[name]}) changes nothing on the GPU tests' inputs"


def test_realistic_intervals_hold_the_float64_answer():
    x8, wq, dq, bias, s = R.realistic_case(64, 192, 192, seed=2)
    acc, _ = R._acc(x8, wq, 192)
    r = torch.relu(acc * dq.double() + bias.double())
    lo, hi = R.interval_codes(x8, wq, dq, bias, 192, True, s)
    y = R.decode(R.q8((r * s).float().double()))
    assert bool(((lo <= y) & (y <= hi)).all()) and float((hi - lo).max()) <= 32.0
    lo, hi = R.interval_bf16(x8, wq, dq, bias, 192, True)
    y = r.float().bfloat16().double()
    assert bool(((lo <= y) & (y <= hi)).all())
