"""tests/train_bf16_ref.py::bf16_round, the integer-arithmetic rounding the bf16 training reference rests on, against
torch.Tensor.to(torch.bfloat16); and what heads="bf16" is on a machine without a GPU: an accepted value that is refused by name."""
import numpy as np
import pytest
import torch

from c4a0_amd.nn import ConnectFourNet, ModelConfig
from c4a0_amd.train_heads import AUTO_HEADS, HEADS, resolve_heads
from tests import train_bf16_ref as R


def _torch_bits(bits: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(bits.astype(np.uint32).view(np.int32).copy()).view(torch.float32)
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _check(bits: np.ndarray, what: str):
    bits = np.asarray(bits, dtype=np.uint32)
    bits = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]       # a NaN's payload is nobody's contract
    assert bits.size, what
    got, want = R.bf16_bits(bits.view(np.float32)), _torch_bits(bits)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, hex(int(bits[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


def test_bf16_round_is_torchs_rounding_on_random_bit_patterns():
    rng = np.random.default_rng(16)
    _check(rng.integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(np.uint32), "random")


def test_bf16_round_takes_every_tie_to_even():
    high = np.arange(2 ** 16, dtype=np.uint32) << 16
    _check(high | 0x8000, "ties")                          # every kept half, odd and even, with the dropped half exactly one half
    _check(high | 0x7FFF, "just below a tie")
    _check(high | 0x8001, "just above a tie")
    _check(high, "bf16 values themselves")


def test_bf16_round_around_zero_subnormals_and_the_largest_values():
    sign = np.array([0, 0x80000000], dtype=np.uint32)[:, None]
    around_zero = np.arange(0, 0x30000, dtype=np.uint32)[None, :] | sign          # +-0 and the smallest subnormals, past two bf16 steps
    _check(around_zero.reshape(-1), "around zero")
    rng = np.random.default_rng(17)
    sub = rng.integers(0, 0x00800000, 2 ** 14, dtype=np.uint64).astype(np.uint32)[None, :] | sign
    _check(sub.reshape(-1), "subnormals")
    _check((np.arange(0x007E0000, 0x00820000, dtype=np.uint32)[None, :] | sign).reshape(-1), "the subnormal / normal border")
    _check((np.arange(0x7F7E0000, 0x7F800001, dtype=np.uint32)[None, :] | sign).reshape(-1), "the largest finite values and the infinities")
    # the largest finite f32 rounds to an infinity, the largest bf16 stays
    assert np.isinf(R.bf16_round(np.float32(3.4028235e38))) and R.bf16_bits(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32))[0] == 0x7F7F
    assert np.isnan(R.bf16_round(np.float32("nan")))


def test_heads_bf16_is_a_value_and_names_the_device_it_lacks():
    assert HEADS == ("auto", "hip", "torch", "bf16") and AUTO_HEADS == "torch"
    model = ConnectFourNet(ModelConfig(1, 32, 2, 2)).train()
    with pytest.raises(ValueError, match=r'heads="bf16": the model is on cpu, not on a HIP device'):
        resolve_heads(model, "bf16")
    assert resolve_heads(model, "auto") == "torch"          # opt-in: "auto" never becomes "bf16"
    with pytest.raises(ValueError, match="heads must be one of"):
        resolve_heads(model, "fp16")
