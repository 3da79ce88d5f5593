"""CPU-side checks of the tournament fast path (ABI 14): the boundary declares and exports the router and the grouped bf16 chain,
the row bound of a routed batch holds for every way the slots can fall to the models, and `GroupedNets.refusal` names the reason a
set of evaluators cannot be stacked.  No GPU needed."""
import itertools
import os
import re

import pytest

torch = pytest.importorskip("torch")

from c4a0_amd import _lib
from c4a0_amd.nn import ConnectFourNet, GroupedNets, InferenceNet, ModelConfig
from c4a0_amd.session import route_rows_cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("c4_session_route_leaves", "c4_conv_tower_bf16_grouped", "c4_linear_bf16_grouped", "c4_head_out_bf16_grouped", "c4_grouped_row_align")


def test_header_declares_and_library_exports_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char\*)\s+(c4_\w+)\s*\(", hdr, flags=re.M))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SIGNATURES)
    assert int(re.search(r"#define C4_ABI_VERSION (\d+)", hdr).group(1)) == 14 == _lib.ABI_VERSION
    assert int(re.search(r"#define C4_ROUTE_MAX_MODELS (\d+)", hdr).group(1)) == _lib.ROUTE_MAX_MODELS >= 16
    assert int(re.search(r"#define C4_GROUPED_ROW_ALIGN (\d+)", hdr).group(1)) == _lib.GROUPED_ROW_ALIGN
    L = _lib.lib()
    assert L.c4_abi_version() == 14
    for name in NEW:
        assert getattr(L, name) is not None
    # a multiple of every grouped kernel's rows per workgroup (tower 16 / 8 boards, GEMM 128 rows, output kernel 16), and an
    # `align` c4_session_route_leaves accepts
    align = L.c4_grouped_row_align()
    assert align == _lib.GROUPED_ROW_ALIGN and align % 128 == 0 and 16 <= align <= 256 and align & (align - 1) == 0


def test_rows_cap_bounds_every_count_vector():
    """rows_cap = round_up(n_slots + n_models (align - 1), align) is never below the rows a routed batch needs -- the sum of the
    models' counts, each rounded up to align -- whatever the counts, and at most one `align` above the worst case."""
    align = 16
    up = lambda c: -(-c // align) * align
    for n_models in range(1, 5):
        best = [0] * 41          # best[n]: max over the count vectors of k models that sum to n, built model by model (exact)
        for _ in range(n_models):
            best = [max(best[n - c] + up(c) for c in range(n + 1)) for n in range(41)]
        for n_slots in range(1, 41):
            need = max(best[: n_slots + 1])                      # idle slots: any sum up to n_slots
            cap = route_rows_cap(n_slots, n_models, align)
            assert cap % align == 0 and need <= cap, (n_slots, n_models, need, cap)
            if n_slots >= n_models:   # (every model can have a row: then the bound is the worst case or one `align` above it)
                assert cap <= need + align, (n_slots, n_models, need, cap)
    # ... and the model-by-model maximum above IS the maximum over all vectors: checked by plain enumeration where that is small
    for n_models, n_slots in ((2, 40), (3, 21), (4, 13)):
        brute = max(sum(up(c) for c in v) for v in itertools.product(range(n_slots + 1), repeat=n_models) if sum(v) <= n_slots)
        assert brute <= route_rows_cap(n_slots, n_models, align) <= brute + align
    assert route_rows_cap(4096, 2, 128) == 4352 and route_rows_cap(40, 5, 16) == 128


def _net(blocks=1, channels=32, pol=2, val=2, seed=0):
    torch.manual_seed(seed)
    return InferenceNet(ConnectFourNet(ModelConfig(blocks, channels, pol, val)), torch.device("cpu"), dtype=torch.bfloat16)


def test_refusal_names_the_reason():
    a, b = _net(seed=1), _net(seed=2)
    why = GroupedNets.refusal({1: a, 2: _net(channels=64)})
    assert why is not None and "channels" in why and "32" in why and "64" in why
    why = GroupedNets.refusal({1: a, 2: _net(blocks=2)})
    assert why is not None and "residual blocks" in why
    why = GroupedNets.refusal({1: a, 2: _net(pol=3)})
    assert why is not None and "head depths" in why
    why = GroupedNets.refusal({1: a, 2: _net(val=1)})
    assert why is not None and "without a hidden layer" in why
    why = GroupedNets.refusal({1: a, 2: lambda planes: None})
    assert why is not None and "not a c4a0_amd.nn.InferenceNet" in why

    class Counting(InferenceNet):
        def forward(self, *args, **kw):
            return super().forward(*args, **kw)
        __call__ = forward

    torch.manual_seed(3)
    why = GroupedNets.refusal({1: a, 2: Counting(ConnectFourNet(ModelConfig(1, 32, 2, 2)), torch.device("cpu"), dtype=torch.bfloat16)})
    assert why is not None and "overrides" in why
    why = GroupedNets.refusal({i: a for i in range(_lib.ROUTE_MAX_MODELS + 1)})
    assert why is not None and "more than" in why
    # equal architectures on the CPU: what is left is that they do not run the hand-written kernels
    why = GroupedNets.refusal({1: a, 2: b})
    assert why is not None and "hand-written" in why
    with pytest.raises(ValueError, match="hand-written"):
        GroupedNets({1: a, 2: b})
