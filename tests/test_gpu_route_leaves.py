"""c4_session_route_leaves on the device against numpy: the resident games' leaves as one batch grouped by the model that must
answer them -- segment bounds, every slot's row (ranks in slot order), the routed rows' planes, zeroed pad rows, the count of
slots whose model the table does not hold -- over the steps of a running multi-model session, and the refusals by name."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BIG = (1 << 63) + 7
IDS = (3, 5, 9, BIG)
UNUSED = 77                      # a table entry no game uses: an empty segment
N_SLOTS, N_STEPS = 40, 24
SENTINEL = 0x7F7F                # a bf16 pattern no plane holds
NO_ROW = 0xFFFFFFFF


def _session():
    """40 slots, 60 requests over four model ids: ten games from the empty board and fifty that start one to three moves before a
    drawn board is full (one legal column each), so that the request list runs dry and slots fall idle within the 24 steps."""
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.helpers import DRAWN_LINE

    pairs = [(a, b) for a in IDS for b in IDS]
    reqs, starts = [], []
    for i in range(60):
        p0, p1 = pairs[(5 * i + 1) % len(pairs)]
        reqs.append((1000 + i, p0, p1))
        starts.append((0, 0) if i % 6 == 0 else O.from_moves(DRAWN_LINE[: 42 - (1 + i % 3)]).key())
    s = DeviceSession(N_SLOTS, 2, 6.6, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16)   # (two simulations per move: the move has a visit)
    s.set_games(reqs, starts)
    return s


def _table(ids):
    return torch.tensor(np.array(ids, dtype=np.uint64).view(np.int64), dtype=torch.int64, device="cuda:0")


def _route(s, ids, align):
    from c4a0_amd.session import route_rows_cap

    rows_cap = route_rows_cap(s.n_slots, len(ids), align)
    out = torch.full((rows_cap, 2, 6, 7), SENTINEL, dtype=torch.int16, device=s.device).view(torch.bfloat16)
    inverse = torch.full((s.n_slots,), 12345, dtype=torch.int32, device=s.device)
    seg = torch.full((len(ids) + 1,), -5, dtype=torch.int32, device=s.device)
    lost = torch.full((1,), -5, dtype=torch.int32, device=s.device)
    s.route_leaves(_table(ids), align, out, inverse, seg, lost)
    torch.cuda.synchronize()
    return (out.view(torch.int16).cpu().numpy().reshape(rows_cap, 84).view(np.uint16), inverse.cpu().numpy().view(np.uint32),
            seg.cpu().numpy().view(np.uint32), int(lost.item()))


def _expect(s, ids, align, rows_cap):
    """numpy, from the slots as the host reads them: leaf_models, leaves() and the planes tensor"""
    models = s.leaf_models.cpu().numpy().view(np.uint64)
    _m, _v, status = s.leaves()
    planes = s.planes.view(torch.int16).cpu().numpy().reshape(s.n_slots, 84).view(np.uint16)
    active = status == 1
    seg, inverse = [0], np.full(s.n_slots, NO_ROW, dtype=np.uint32)
    rows = np.full((rows_cap, 84), SENTINEL, dtype=np.uint16)
    for mid in ids:
        slots = np.flatnonzero(active & (models == np.uint64(mid)))        # ascending slot order
        lo = seg[-1]
        hi = lo + -(-len(slots) // align) * align
        inverse[slots] = lo + np.arange(len(slots), dtype=np.uint32)
        rows[lo: lo + len(slots)] = planes[slots]
        rows[lo + len(slots): hi] = 0                                       # pad rows: empty boards
        seg.append(hi)
    lost = int((active & ~np.isin(models, np.array(ids, dtype=np.uint64))).sum())
    return rows, inverse, np.array(seg, dtype=np.uint32), lost, active, models


def test_route_leaves_matches_numpy_over_a_running_session():
    from tests.helpers import hash_eval_torch

    s = _session()
    try:
        s.bind()
        s.bind_leaf_models()
        s.start()
        full = IDS[:2] + (UNUSED,) + IDS[2:]
        seen_idle = seen_models = 0
        uneven = False
        for step in range(N_STEPS + 1):
            if step:
                s.evaluate(hash_eval_torch)
                s.step()
            torch.cuda.synchronize()
            for align in (16, 128):
                got = _route(s, full, align)
                want = _expect(s, full, align, got[0].shape[0])
                assert np.array_equal(got[2], want[2]), (step, align, got[2], want[2])          # seg_start
                assert np.array_equal(got[1], want[1]), (step, align)                           # inverse, idle slots 0xFFFFFFFF
                assert np.array_equal(got[0], want[0]), (step, align)                           # routed rows, zero pads, the rest untouched
                assert got[3] == want[3] == 0
                assert got[2][3] == got[2][2]                                                   # the unused model: an empty segment
            active, models = want[4], want[5]
            seen_idle = max(seen_idle, int((~active).sum()))
            seen_models = max(seen_models, len(set(models[active].tolist())))
            uneven = uneven or any(int((active & (models == np.uint64(m))).sum()) % 16 for m in IDS)
            # one id taken out of the table: its slots are not routed and are counted
            for gone in (IDS[0], BIG):
                part = tuple(m for m in full if m != gone)
                got = _route(s, part, 16)
                want = _expect(s, part, 16, got[0].shape[0])
                assert got[3] == want[3] == int((active & (models == np.uint64(gone))).sum())
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0])
        assert seen_idle > 0 and int((~active).sum()) > 0, "the last step must see idle slots"
        assert seen_models == 4 and uneven
        s.raise_if_device_error()
    finally:
        s.close()


def test_route_leaves_refusals_name_the_bound():
    from c4a0_amd._lib import C4Error, ROUTE_MAX_MODELS
    from c4a0_amd.session import DeviceSession, route_rows_cap

    s = _session()
    try:
        s.bind()
        dev = s.device
        inverse = torch.zeros(N_SLOTS, dtype=torch.int32, device=dev)
        seg = torch.zeros(ROUTE_MAX_MODELS + 2, dtype=torch.int32, device=dev)
        lost = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.zeros((route_rows_cap(N_SLOTS, len(IDS), 16), 2, 6, 7), dtype=torch.bfloat16, device=dev)
        with pytest.raises(C4Error, match="no leaf models bound"):
            s.route_leaves(_table(IDS), 16, out, inverse, seg, lost)
        s.bind_leaf_models()
        s.start()
        s.route_leaves(_table(IDS), 16, out, inverse, seg, lost)                 # the bound itself is accepted
        with pytest.raises(C4Error, match="rows_cap 96 is below .* = 112"):
            s.route_leaves(_table(IDS), 16, out[:-16], inverse, seg, lost)
        for align in (8, 24, 512):
            with pytest.raises(C4Error, match="align must be a power of two in 16..256"):
                s.route_leaves(_table(IDS), align, out, inverse, seg, lost)
        big = torch.zeros((route_rows_cap(N_SLOTS, ROUTE_MAX_MODELS + 1, 16), 2, 6, 7), dtype=torch.bfloat16, device=dev)
        with pytest.raises(C4Error, match="n_models must be between 1 and"):
            s.route_leaves(_table(range(ROUTE_MAX_MODELS + 1)), 16, big, inverse, seg, lost)
        torch.cuda.synchronize()
    finally:
        s.close()
    f32 = DeviceSession(8, 2, 6.6, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.float32)
    try:
        f32.set_games([(i, 3, 5) for i in range(8)])
        f32.bind()
        f32.bind_leaf_models()
        with pytest.raises(C4Error, match="planes must be bf16"):
            f32.route_leaves(_table(IDS), 16, out, torch.zeros(8, dtype=torch.int32, device="cuda:0"), seg, lost)
    finally:
        f32.close()
    srch = DeviceSession(8, 4, 6.6, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16, search=True)
    try:
        srch.set_games([(i, 0, 0) for i in range(8)], [(0, 0)] * 8)
        srch.bind()
        with pytest.raises(C4Error, match="search session"):
            srch.route_leaves(_table(IDS), 16, out, torch.zeros(8, dtype=torch.int32, device="cuda:0"), seg, lost)
    finally:
        srch.close()
