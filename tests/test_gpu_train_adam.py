"""c4_train_adam_f32 on the GPU, through the C ABI: the fused multi-tensor Adam against tests/adam_ref.py (float64) judged beside f32
torch.optim.Adam on the same inputs on the same device, its reproducibility, its device-side step count, non-finite gradients, the
call captured alone into a graph, and its refusals."""
import numpy as np
import pytest
import torch

from c4a0_amd import _lib
from c4a0_amd.train_graph import adam_table
from tests import adam_ref
from tests.helpers import evidence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
LR, BETAS, EPS = 2e-3, (0.9, 0.999), 1e-8
LENGTHS = (1, 3, 4, 5, 7, 1023, 1024, 1025, 4099)
TABLES = {"all": LENGTHS, "alone": (4099,), "small37": tuple(1 + (5 * i) % 7 for i in range(37))}
SENTINEL = 12345.0


class Segments:
    """Segments of the given lengths in one flat device buffer per quantity, every segment 16-byte aligned, the pad elements between
    them holding SENTINEL (the kernel must leave them alone), and their c4_adam_segment table."""

    def __init__(self, lengths):
        self.lengths = tuple(lengths)
        self.offsets = np.concatenate([[0], np.cumsum([4 * ((n + 3) // 4) + 4 for n in self.lengths])]).astype(np.int64)   # + 4: a whole pad group
        total = int(self.offsets[-1])
        self.buf = {k: torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV) for k in "pgmv"}
        self.step = torch.zeros(4, dtype=torch.int32, device=DEV)
        table, self.n_blocks = adam_table([tuple(self.buf[k].data_ptr() + 4 * int(o) for k in "pgmv") + (n,)
                                           for o, n in zip(self.offsets, self.lengths)])
        self.table = torch.from_numpy(table).to(DEV)

    def load(self, state, t_before: int):
        for k in "pgmv":
            flat = np.full(int(self.offsets[-1]), SENTINEL, dtype=np.float32)
            for o, a in zip(self.offsets, state[k]):
                flat[o:o + a.size] = a
            self.buf[k].copy_(torch.from_numpy(flat))
        self.step.zero_()
        self.step[0] = t_before

    def call(self, wd: float) -> int:
        return _lib.lib().c4_train_adam_f32(self.table.data_ptr(), len(self.lengths), self.n_blocks, self.step.data_ptr(), LR, BETAS[0], BETAS[1], EPS,
                                            wd, torch.cuda.current_stream().cuda_stream)

    def read(self):
        flat = {k: self.buf[k].cpu().numpy() for k in "pgmv"}
        return {k: [flat[k][o:o + n].copy() for o, n in zip(self.offsets, self.lengths)] for k in "pgmv"}, flat

    @property
    def steps(self) -> int:
        return int(self.step[0].item())


def make_state(lengths, seed: int, grads: str):
    """p, g, m, v per segment (f32 numpy).  grads: "random" (magnitudes 1e-6 .. 10, either sign), "zero", or "tiny" (g, m and
    sqrt(v) around 1e-12 and below: the denominator is eps)."""
    rng = np.random.default_rng(seed)
    st = {k: [] for k in "pgmv"}
    for n in lengths:
        st["p"].append(rng.standard_normal(n).astype(np.float32))
        if grads == "tiny":
            st["g"].append((rng.choice([-1.0, 1.0], n) * 1e-12 * rng.uniform(0.5, 2.0, n)).astype(np.float32))
            st["m"].append((rng.standard_normal(n) * 1e-12).astype(np.float32))
            st["v"].append((rng.uniform(0.1, 4.0, n) * 1e-26).astype(np.float32))
        else:
            g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 1.0, n)
            st["g"].append((g if grads == "random" else np.zeros(n)).astype(np.float32))
            st["m"].append((rng.standard_normal(n) * 0.1).astype(np.float32))
            st["v"].append(((rng.standard_normal(n) * 0.1) ** 2).astype(np.float32))
    return st


def torch_adam(state, t_before: int, wd: float):
    """One step of f32 torch.optim.Adam on the device from the same state: (p, m, v) per segment"""
    params = [torch.from_numpy(a.copy()).to(DEV).requires_grad_() for a in state["p"]]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    for prm, g, m, v in zip(params, state["g"], state["m"], state["v"]):
        prm.grad = torch.from_numpy(g.copy()).to(DEV)
        opt.state[prm] = {"step": torch.tensor(float(t_before)), "exp_avg": torch.from_numpy(m.copy()).to(DEV),
                          "exp_avg_sq": torch.from_numpy(v.copy()).to(DEV)}
    opt.step()
    assert all(int(opt.state[prm]["step"]) == t_before + 1 for prm in params)
    return {"p": [prm.detach().cpu().numpy() for prm in params], "m": [opt.state[prm]["exp_avg"].cpu().numpy() for prm in params],
            "v": [opt.state[prm]["exp_avg_sq"].cpu().numpy() for prm in params]}


@pytest.mark.parametrize("shape", list(TABLES))
def test_kernel_against_float64_beside_torch_adam(shape):
    lengths = TABLES[shape]
    seg = Segments(lengths)
    worst, compared = 0.0, 0
    for t in (1, 2, 1000):
        for wd in (0.0, 4e-4):
            for grads in ("random", "zero", "tiny"):
                state = make_state(lengths, 1000 * t + len(grads), grads)
                seg.load(state, t - 1)
                _lib.check(seg.call(wd))
                got, flat = seg.read()
                assert seg.steps == t
                stock = torch_adam(state, t - 1, wd)
                for i, n in enumerate(lengths):
                    ref = dict(zip("pmv", adam_ref.adam_step(state["p"][i], state["g"][i], state["m"][i], state["v"][i], t - 1, LR, *BETAS, EPS, wd)))
                    for k in "pmv":
                        e_hip = float(np.abs(got[k][i].astype(np.float64) - ref[k]).max())
                        e_torch = float(np.abs(stock[k][i].astype(np.float64) - ref[k]).max())
                        allowed = max(4 * e_torch, 4 * U * float(np.abs(ref[k]).max()))
                        if allowed > 0:
                            worst = max(worst, e_hip / allowed)
                        compared += 1
                        assert e_hip <= allowed, (shape, t, wd, grads, n, k, e_hip, e_torch, allowed)
                    assert got["g"][i].tobytes() == state["g"][i].tobytes()
                # the pad elements between the segments are untouched
                for k in "pgmv":
                    mask = np.ones(flat[k].size, dtype=bool)
                    for o, n in zip(seg.offsets, lengths):
                        mask[o:o + n] = False
                    assert (flat[k][mask] == SENTINEL).all(), (shape, k)
    print(f"adam {shape}: {compared} tensors, worst error / allowed = {worst:.3f}")
    evidence(f"c4_train_adam_f32 table {shape!r}: {compared} tensors against float64 beside torch.optim.Adam, worst error / allowed = {worst:.3f}")


def test_two_calls_give_the_same_bytes_and_the_counter_advances_by_one():
    state = make_state(LENGTHS, 5, "random")
    a, b = Segments(LENGTHS), Segments(LENGTHS)
    for seg in (a, b):
        seg.load(state, 6)
        _lib.check(seg.call(4e-4))
    assert a.steps == b.steps == 7
    flat_a, flat_b = a.read()[1], b.read()[1]
    for k in "pgmv":
        assert flat_a[k].tobytes() == flat_b[k].tobytes(), k
    _lib.check(a.call(4e-4))
    _lib.check(a.call(4e-4))
    assert a.steps == 9
    assert a.read()[1]["p"].tobytes() != flat_a["p"].tobytes()


def test_a_non_finite_gradient_stays_in_its_element():
    lengths = (5, 1025)
    clean = make_state(lengths, 9, "random")
    dirty = {k: [a.copy() for a in v] for k, v in clean.items()}
    spots = [(0, 4, -np.inf), (1, 3, np.inf), (1, 700, np.nan), (1, 1024, np.nan)]   # (0, 4) and (1, 1024): the element-wise tails
    for s, i, value in spots:
        dirty["g"][s][i] = value
    a, b = Segments(lengths), Segments(lengths)
    a.load(clean, 2)
    b.load(dirty, 2)
    _lib.check(a.call(4e-4))
    _lib.check(b.call(4e-4))
    (got_a, flat_a), (got_b, flat_b) = a.read(), b.read()
    for k in "pmv":
        for s, i, _value in spots:
            assert not np.isfinite(got_b[k][s][i]), (k, s, i)
            flat_b[k][a.offsets[s] + i] = flat_a[k][a.offsets[s] + i]
        assert flat_a[k].tobytes() == flat_b[k].tobytes(), k


def test_the_call_captured_alone_replays_as_eager_calls():
    from c4a0_amd.session import capture

    state = make_state(LENGTHS, 3, "random")
    eager, graphed = Segments(LENGTHS), Segments(LENGTHS)
    eager.load(state, 0)
    for _ in range(3):
        _lib.check(eager.call(4e-4))
    graphed.load(state, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture(graph):
        _lib.check(graphed.call(4e-4))
    torch.cuda.synchronize()
    assert graphed.steps == 0                      # a capture executes nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert graphed.steps == eager.steps == 3       # the replayed graph advances the device's count
    flat_e, flat_g = eager.read()[1], graphed.read()[1]
    for k in "pgmv":
        assert flat_e[k].tobytes() == flat_g[k].tobytes(), k


def test_bad_arguments_are_refused_and_launch_nothing():
    L = _lib.lib()
    seg = Segments((7, 1025))
    seg.load(make_state(seg.lengths, 1, "random"), 4)
    before = seg.read()[1]
    s = torch.cuda.current_stream().cuda_stream
    n = len(seg.lengths)
    calls = {
        "null table": (None, n, seg.n_blocks, seg.step.data_ptr()),
        "null step": (seg.table.data_ptr(), n, seg.n_blocks, None),
        "n_segs == 0": (seg.table.data_ptr(), 0, seg.n_blocks, seg.step.data_ptr()),
        "n_blocks == 0": (seg.table.data_ptr(), n, 0, seg.step.data_ptr()),
        "n_blocks < n_segs": (seg.table.data_ptr(), n, 1, seg.step.data_ptr()),
        "misaligned table": (seg.table.data_ptr() + 8, 1, 1, seg.step.data_ptr()),
    }
    for what, (table, n_segs, n_blocks, step) in calls.items():
        assert L.c4_train_adam_f32(table, n_segs, n_blocks, step, LR, BETAS[0], BETAS[1], EPS, 4e-4, s) == _lib.ERR_BAD_ARG, what
        assert L.c4_last_error_string().decode().startswith("c4_train_adam_f32: "), what
    torch.cuda.synchronize()
    after = seg.read()[1]
    assert seg.steps == 4
    for k in "pgmv":
        assert before[k].tobytes() == after[k].tobytes(), k
    assert L.c4_train_adam_block_elems() == _lib.ADAM_BLOCK_ELEMS
