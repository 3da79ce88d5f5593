"""The built-in players' kernels against their definition restated in numpy (tests/builtin_players_ref.py), through the C ABI:
c4_builtin_eval on ragged batches of f32 and bf16 planes with sentinel rows behind the batch, c4_builtin_eval_grouped on
hand-written segment bounds (an empty segment, rows behind the last segment, bounds moved past leading segments), what both
refuse, and `GroupedPlayers.forward` for a dict of built-in players alone.  Bit for bit: every output is an exact dyadic rational."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import builtin_players_ref as R

ROWS = (1, 63, 300)          # none a multiple of the 64 rows of a workgroup; 300: more than one workgroup, a ragged last one
PAD = 64                     # sentinel rows behind the batch
SENTINEL = -77.25
BIG = (1 << 63) + 7
_POS = {}


def _planes_np(n=512):
    if n not in _POS:
        from tests.helpers import pos_to_planes_np, random_positions

        pos = np.array(random_positions(n, seed=4242), dtype=np.uint64)
        _POS[n] = pos_to_planes_np(pos[:, 0], pos[:, 1])
    return _POS[n]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernel_equals_the_twin_and_writes_nothing_behind_the_batch(kind, dtype):
    from c4a0_amd import _lib
    from c4a0_amd.builtin import KINDS

    L = _lib.lib()
    planes_np = _planes_np()
    planes = torch.from_numpy(planes_np).to("cuda:0", dtype)
    for rows, mid, seed in itertools.product(ROWS, R.IDS, R.SEEDS):
        lg = torch.full((rows + PAD, 7), SENTINEL, dtype=torch.float32, device="cuda:0")
        q = torch.full((rows + PAD, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        _lib.check(L.c4_builtin_eval(C.c_void_p(planes.data_ptr()), 1 if dtype == torch.bfloat16 else 0, rows, KINDS[kind], seed, mid,
                                     C.c_void_p(lg.data_ptr()), C.c_void_p(q.data_ptr()), _stream()))
        lg, q = lg.cpu().numpy(), q.cpu().numpy()
        w_lg, w_qp, w_qn = R.forward_numpy(kind, seed, mid, planes_np[:rows])
        assert lg[:rows].tobytes() == w_lg.tobytes(), (rows, mid, seed)
        assert q[:rows, 0].tobytes() == w_qp.tobytes() and q[:rows, 1].tobytes() == w_qn.tobytes(), (rows, mid, seed)
        assert np.all(lg[rows:] == SENTINEL) and np.all(q[rows:] == SENTINEL), "rows behind the batch were written"


def test_evaluator_object_and_what_the_entry_point_refuses():
    from c4a0_amd import _lib
    from c4a0_amd.builtin import BuiltinEvaluator

    L = _lib.lib()
    planes_np = _planes_np()[:63]
    ev = BuiltinEvaluator("random", BIG, seed=9, device="cuda:0")
    assert (ev.graph_safe, ev.batch_invariant, ev.dtype) == (True, True, None)
    want = R.forward_numpy("random", 9, BIG, planes_np)
    for dtype in (torch.float32, torch.bfloat16):
        planes = torch.from_numpy(planes_np).to("cuda:0", dtype)
        lg, q = ev(planes)
        assert lg.cpu().numpy().tobytes() == want[0].tobytes() and q[:, 0].cpu().numpy().tobytes() == want[1].tobytes()
        out_lg, out_q = torch.zeros((63, 7), device="cuda:0"), torch.zeros((63, 2), device="cuda:0")
        got = ev(planes, out_logprobs=out_lg, out_q=out_q)
        assert got[0] is out_lg and got[1] is out_q and torch.equal(out_lg, lg) and torch.equal(out_q, q)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(ev.forward_numpy(planes_np), want))
    # a negative zero is an empty cell, any other value a stone (bf16 and f32 alike)
    odd = torch.from_numpy(planes_np * np.float32(-2.5)).to("cuda:0")
    odd[odd == 0] = -0.0
    assert torch.equal(ev(odd)[0], lg) and torch.equal(ev(odd.to(torch.bfloat16))[0], lg)
    with pytest.raises(TypeError):
        ev(planes.to(torch.float16))
    planes = torch.from_numpy(planes_np).to("cuda:0")
    out_lg, out_q = torch.full((63, 7), SENTINEL, device="cuda:0"), torch.full((63, 2), SENTINEL, device="cuda:0")
    args = lambda **kw: [kw.get("planes", C.c_void_p(planes.data_ptr())), kw.get("dtype", 0), kw.get("rows", 63), kw.get("kind", 1), 0, 0,
                         C.c_void_p(out_lg.data_ptr()), C.c_void_p(out_q.data_ptr()), _stream()]
    assert L.c4_builtin_eval(*args(rows=0)) == _lib.OK
    assert L.c4_builtin_eval(*args(rows=0, planes=None)) == _lib.OK
    for bad, word in ((dict(kind=2), "kind"), (dict(dtype=2), "planes_dtype"), (dict(planes=C.c_void_p(planes.data_ptr() + 4)), "aligned"),
                      (dict(planes=None), "null")):
        assert L.c4_builtin_eval(*args(**bad)) == _lib.ERR_BAD_ARG, bad
        assert word in L.c4_last_error_string().decode(), bad
    torch.cuda.synchronize()
    assert bool((out_lg == SENTINEL).all()) and bool((out_q == SENTINEL).all()), "a refused or empty call wrote outputs"


def _grouped(L, planes, seg, n_segments, kinds, seeds, ids, answers, seg_offset=0):
    return L.c4_builtin_eval_grouped(C.c_void_p(planes.data_ptr()), C.c_void_p(seg.data_ptr() + 4 * seg_offset), n_segments, (C.c_uint32 * len(kinds))(*kinds),
                                     (C.c_uint64 * len(seeds))(*seeds), (C.c_uint64 * len(ids))(*ids), planes.shape[0], C.c_void_p(answers.data_ptr()), _stream())


def test_grouped_kernel_on_hand_written_segments():
    from c4a0_amd import _lib

    L = _lib.lib()
    planes_np = _planes_np()
    planes = torch.from_numpy(planes_np).to("cuda:0", torch.bfloat16)
    seg = torch.tensor([0, 128, 128, 384], dtype=torch.int32, device="cuda:0")   # uniform, an empty random segment, random with another seed
    players = [("uniform", 0, 5), ("random", 1, 3), ("random", (1 << 64) - 1, BIG)]
    kinds, seeds, ids = [0, 1, 1], [p[1] for p in players], [p[2] for p in players]
    answers = torch.full((512, 9), SENTINEL, dtype=torch.float32, device="cuda:0")
    _lib.check(_grouped(L, planes, seg, 3, kinds, seeds, ids, answers))
    got = answers.cpu().numpy()
    assert got[:128].tobytes() == R.answers9("uniform", 0, 5, planes_np[:128]).tobytes()
    assert got[128:384].tobytes() == R.answers9("random", (1 << 64) - 1, BIG, planes_np[128:384]).tobytes()
    assert np.all(got[384:] == SENTINEL), "rows behind the last segment were written"
    assert got[128:384].tobytes() != R.answers9("random", 1, 3, planes_np[128:384]).tobytes()      # (the empty segment's player answered nothing)
    # the bounds moved past the first segment, as a tournament moves them past its networks' segments: rows 0..127 are not this call's
    answers.fill_(SENTINEL)
    _lib.check(_grouped(L, planes, seg, 2, kinds[1:], seeds[1:], ids[1:], answers, seg_offset=1))
    again = answers.cpu().numpy()
    assert np.all(again[:128] == SENTINEL) and again[128:384].tobytes() == got[128:384].tobytes() and np.all(again[384:] == SENTINEL)
    # nothing to do, and what is refused
    answers.fill_(SENTINEL)
    assert _grouped(L, planes, seg, 0, [0], [0], [0], answers) == _lib.OK
    assert _grouped(L, planes[:0], seg, 3, kinds, seeds, ids, answers) == _lib.OK
    for call, word in ((lambda: _grouped(L, planes, seg, 3, [0, 7, 1], seeds, ids, answers), "kinds[1]"),
                       (lambda: _grouped(L, planes[:448], seg, 3, kinds, seeds, ids, answers), "C4_GROUPED_ROW_ALIGN"),
                       (lambda: _grouped(L, planes, seg, _lib.ROUTE_MAX_MODELS + 1, kinds * 11, seeds * 11, ids * 11, answers), "C4_ROUTE_MAX_MODELS")):
        assert call() == _lib.ERR_BAD_ARG and word in L.c4_last_error_string().decode(), word
    torch.cuda.synchronize()
    assert bool((answers == SENTINEL).all())


def test_grouped_players_of_built_ins_alone():
    from c4a0_amd.builtin import BuiltinEvaluator, GroupedPlayers
    from c4a0_amd.nn import GroupedNets

    evs = {5: BuiltinEvaluator("uniform", 5, device="cuda:0"), 3: BuiltinEvaluator("random", 3, seed=1, device="cuda:0"),
           BIG: BuiltinEvaluator("random", BIG, seed=9, device="cuda:0")}
    assert GroupedNets.refusal(evs) is None
    g = GroupedPlayers(evs)
    assert (g.n_models, g.n_nets, g.row_align, g.ids) == (3, 0, 128, [5, 3, BIG]) and g.device == torch.device("cuda:0")
    assert g.model_ids.cpu().numpy().view(np.uint64).tolist() == [5, 3, BIG]
    buf = g.buffers(512)
    assert set(buf) == {"rows_cap", "planes", "answers"}, "no network: planes and answers only"
    planes_np = _planes_np()
    buf["planes"].copy_(torch.from_numpy(planes_np).to("cuda:0", torch.bfloat16))
    buf["answers"].fill_(SENTINEL)
    seg = torch.tensor([0, 128, 256, 384], dtype=torch.int32, device="cuda:0")
    got = g.forward(buf, seg).cpu().numpy()
    want = np.concatenate([R.answers9("uniform", 0, 5, planes_np[:128]), R.answers9("random", 1, 3, planes_np[128:256]),
                           R.answers9("random", 9, BIG, planes_np[256:384])])
    assert got[:384].tobytes() == want.tobytes() and np.all(got[384:] == SENTINEL)
