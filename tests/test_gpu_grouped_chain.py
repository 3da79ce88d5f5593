"""The grouped bf16 chain (c4_conv_tower_bf16_grouped, c4_linear_bf16_grouped, c4_head_out_bf16_grouped) against the ungrouped
entry points: every stage, run once on a batch whose rows are cut into one segment per model, equals the ungrouped kernel run per
model on that model's rows BIT FOR BIT; rows past the last segment are not written; an empty segment writes nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL16, SENTINEL32 = 0x7F7F, 0x7F7F7F7F   # bf16 / f32 patterns (large finite values) that no stage produces
_NETS, _PLANES = {}, {}


def _nets(channels, blocks, pol_hidden, val_hidden):
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    key = (channels, blocks, pol_hidden, val_hidden)
    if key not in _NETS:
        nets = {}
        for i, mid in enumerate((3, (1 << 63) + 7, 9)):
            torch.manual_seed(100 * channels + 10 * blocks + i)
            model = ConnectFourNet(ModelConfig(blocks, channels, pol_hidden + 1, val_hidden + 1))
            with torch.no_grad():   # BatchNorm statistics that are not the identity, so that the folded biases differ per model
                for m in model.modules():
                    if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                        m.running_mean.normal_(0.0, 0.1)
                        m.running_var.uniform_(0.5, 1.5)
            nets[mid] = InferenceNet(model, torch.device("cuda:0"), dtype=torch.bfloat16, strict=True)
        _NETS[key] = nets
    return _NETS[key]


def _planes(n):
    """n random legal positions as bf16 planes (computed once, shared, never written)"""
    if n not in _PLANES:
        from tests.helpers import pos_to_planes_np, random_positions

        pos = random_positions(n, seed=4242)
        mask, value = np.array([p[0] for p in pos], dtype=np.uint64), np.array([p[1] for p in pos], dtype=np.uint64)
        _PLANES[n] = torch.from_numpy(pos_to_planes_np(mask, value)).to("cuda:0", torch.bfloat16)
    return _PLANES[n]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _filled(shape, dtype):
    if dtype == torch.bfloat16:
        return torch.full(shape, SENTINEL16, dtype=torch.int16, device="cuda:0").view(torch.bfloat16)
    return torch.full(shape, SENTINEL32, dtype=torch.int32, device="cuda:0").view(torch.float32)


@pytest.mark.parametrize("channels,blocks", [(32, 1), (64, 1), (32, 0)])
@pytest.mark.parametrize("heads", [(2, 1), (1, 1)])
@pytest.mark.parametrize("shape", ["a+3,0,1", "1,2a,5"])
def test_grouped_stages_equal_the_ungrouped_kernels_bit_for_bit(channels, blocks, heads, shape):
    from c4a0_amd.nn import GroupedNets

    nets = _nets(channels, blocks, *heads)
    g = GroupedNets(nets)
    a = g.row_align
    counts = (a + 3, 0, 1) if shape == "a+3,0,1" else (1, 2 * a, 5)
    seg = np.concatenate([[0], np.cumsum([-(-c // a) * a for c in counts])]).astype(np.int32)
    rows_cap = max(5 * 128, int(seg[-1]) + a)          # >= five GEMM row tiles: the XCD-rectangle map is not the identity
    assert rows_cap % a == 0 and seg[-1] < rows_cap
    seg_dev = torch.from_numpy(seg).to("cuda:0")
    # real rows: random legal positions; pad rows: empty boards (as the router leaves them); beyond the last segment: positions
    # again (they must not be computed)
    planes = _planes(1024)[:rows_cap].clone()
    for m, c in enumerate(counts):
        planes[int(seg[m]) + c: int(seg[m + 1])] = 0
    f = 42 * channels
    end = int(seg[-1])

    def check(out, per_model, what):
        torch.cuda.synchronize()
        for m, net in enumerate(nets.values()):
            lo, hi = int(seg[m]), int(seg[m + 1])
            if lo == hi:
                continue
            want = per_model(net, lo, hi)
            assert torch.equal(_bits(out[lo:hi]), _bits(want)), (what, m)
        tail = _bits(out[end:])
        assert bool((tail == (SENTINEL16 if out.dtype == torch.bfloat16 else SENTINEL32)).all()), (what, "rows past the last segment were written")

    # tower
    feat = g.tower(planes, seg_dev, _filled((rows_cap, f), torch.bfloat16))
    check(feat, lambda net, lo, hi: net.chain.tower(planes[lo:hi]), "tower")
    # merged first layer of both heads
    h1 = g.linear_relu(feat, g.w1, g.b1, seg_dev, _filled((rows_cap, 2 * f), torch.bfloat16))
    check(h1, lambda net, lo, hi: net.chain.linear_relu(feat[lo:hi], net.merged_w1, net.merged_b1), "merged layer")
    p, v = h1[:, :f], h1[:, f:]
    # a further layer, its input a column range of the merged tensor
    for i in range(len(g.pol_w)):
        nxt = g.linear_relu(p, g.pol_w[i], g.pol_b[i], seg_dev, _filled((rows_cap, f), torch.bfloat16))
        check(nxt, lambda net, lo, hi, p=p, i=i: net.chain.linear_relu(p[lo:hi], net.pol_w[1 + i], net.pol_b[1 + i]), f"policy layer {i}")
        p = nxt
    assert len(g.pol_w) == heads[0] - 1 and len(g.val_w) == heads[1] - 1
    # head out: [rows][9] = 7 log-probabilities, q_penalty, q_no_penalty
    ans = g.head_out(p, v, seg_dev, _filled((rows_cap, 9), torch.float32))

    def head(net, lo, hi):
        lp, q = net.chain.head_out(p[lo:hi], v[lo:hi])
        return torch.cat([lp, q], dim=1)
    check(ans, head, "head out")
    # the whole chain at once is the stages in a row, and a real row is what the model's InferenceNet gives that position
    buf = g.buffers(rows_cap)
    buf["planes"].copy_(planes)
    buf["answers"].copy_(_filled((rows_cap, 9), torch.float32))
    whole = g.forward(buf, seg_dev)
    torch.cuda.synchronize()
    assert torch.equal(_bits(whole), _bits(ans))
    for m, (net, c) in enumerate(zip(nets.values(), counts)):
        if c:
            lo = int(seg[m])
            lp, q = net(planes[lo: lo + c])
            assert torch.equal(_bits(whole[lo: lo + c]), _bits(torch.cat([lp, q], dim=1)))


def test_grouped_entry_points_refuse_bad_shapes():
    from c4a0_amd._lib import C4Error
    from c4a0_amd.nn import GroupedNets

    g = GroupedNets(_nets(32, 1, 1, 1))
    a = g.row_align
    seg = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    planes = torch.zeros((a + 16, 2, 6, 7), dtype=torch.bfloat16, device="cuda:0")
    out = torch.zeros((a + 16, 42 * 32), dtype=torch.bfloat16, device="cuda:0")
    with pytest.raises(C4Error, match="rows_cap must be a multiple of C4_GROUPED_ROW_ALIGN"):
        g.tower(planes, seg, out)
    with pytest.raises(C4Error, match="rows_cap must be a multiple of C4_GROUPED_ROW_ALIGN"):
        g.linear_relu(out, g.w1, g.b1, seg, torch.zeros((a + 16, 2 * 42 * 32), dtype=torch.bfloat16, device="cuda:0"))
    with pytest.raises(C4Error, match="rows_cap must be a multiple of C4_GROUPED_ROW_ALIGN"):
        g.head_out(out, out, seg, torch.zeros((a + 16, 9), dtype=torch.float32, device="cuda:0"))
