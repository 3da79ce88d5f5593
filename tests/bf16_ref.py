"""A float64 restatement of the bf16 evaluator chain (c4_conv_tower_bf16 -> c4_linear_bf16 -> c4_head_out_bf16), on the
operands as the GPU sees them, with the roundings at the points include/c4a0_hip.h documents.

Every product and sum is computed in float64; a value is rounded to bf16 only where the kernels round, and only after it is
asserted to be exactly an f32 (then torch's round-to-nearest-even `.float().bfloat16()` is the kernels' conversion).  On
operands from the exact-grid generators below every partial sum of every output, in ANY order, is an exact f32
(`check_exact` proves it per layer), so the kernels' results do not depend on their MFMA accumulation order and must equal
this reference bit for bit: what is under test is only where and how the chain rounds.  For arbitrary data `interval`
gives the rigorous bound any f32-or-wider summation order satisfies.

`mut` (a set of names, MUTATIONS) switches on plausible kernel bugs, so that tests/test_bf16_ref.py can show the GPU tests'
inputs tell each of them from the true chain."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from c4a0_amd.nn import _fold_bn, pack_tower_weights

D = torch.float64
U = 2.0 ** -24   # unit roundoff of f32

MUTATIONS = {
    "trunc": "f32 -> bf16 by truncation instead of round-to-nearest-even",
    "away": "f32 -> bf16 rounding ties away from zero",
    "relu1": "a ReLU after the first conv of the last block",
    "bias_last": "output channel 0's bias dropped in the last tower layer and in the GEMM",
    "edge_tap": "tap (0, +1) dropped for the cells of column 0 in the last tower layer",
    "wrap": "column 6's (., +1) taps read the next row's column 0 instead of zero in the last tower layer",
    "no_residual": "the last block's residual omitted (y = relu(s) instead of x + relu(s))",
    "drop_ktile": "the GEMM's last 64-deep k-tile dropped",
    "row_offset": "GEMM rows 64..127 written with the result of rows 128..191",
    "no_perm": "the first hidden layers' input columns not permuted from 'c h w' to the tower's cell-major order",
}


# ------------------------------------------------------------------------------------------------------------------ rounding
def assert_f32(t: torch.Tensor, what: str = "value") -> None:
    bad = t.float().double() != t
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {t.reshape(-1)[i].item()!r} is not exactly an f32 (the exact-grid precondition is broken)")


def bf16(t: torch.Tensor, mut=frozenset(), what: str = "value") -> torch.Tensor:
    """float64 t (asserted to be exactly f32) -> the bf16 value it rounds to, as float64."""
    assert_f32(t, what)
    if "trunc" in mut or "away" in mut:
        u = t.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        low = u & 0xFFFF
        if "trunc" in mut:
            u = u - low
        else:
            u = u - low + torch.where(low >= 0x8000, 0x10000, 0)
        u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
        return u.view(torch.float32).double()
    return t.float().bfloat16().double()


def pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64 for integer e in [-1022, 1023], built from the exponent bits (torch.ldexp / pow are not exact on every
    device)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def bf16_directed(t: torch.Tensor, up: bool) -> torch.Tensor:
    """Round float64 t to bf16 toward -inf (up=False) or +inf (up=True); f32-range values, subnormals included."""
    m, e = torch.frexp(t)                                     # t = m 2^e, 0.5 <= |m| < 1
    ulp = pow2(torch.clamp(e - 8, min=-133))
    q = t / ulp                                               # exact: a power-of-two scale
    q = torch.ceil(q) if up else torch.floor(q)
    return torch.where(t == 0, t, q * ulp)


def ties(t: torch.Tensor):
    """(ties RNE rounds toward zero, ties it rounds away from zero) among the exact f32 values t about to be rounded."""
    u = t.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    tie = (u & 0xFFFF) == 0x8000
    odd = ((u >> 16) & 1) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum())


# ------------------------------------------------------------------------------------------------------------------ exactness
def lowest_bit(t: torch.Tensor) -> float:
    """The largest power of two that divides every element of float64 t (1.0 for an all-zero t)."""
    nz = t[t != 0].abs()
    if nz.numel() == 0:
        return 1.0
    m, e = torch.frexp(nz)
    # m has at most 53 bits: m 2^53 is an integer; its trailing zeros give the lowest set bit of each element
    mi = (m * 2.0 ** 53).to(torch.int64)
    tz = ((mi & -mi).double().log2()).round().to(torch.int64)
    return float(2.0 ** int((e.to(torch.int64) - 53 + tz).min()))


def check_exact(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, abs_sum: torch.Tensor, what: str) -> None:
    """Every partial sum of every output is a multiple of unit = min(lowbit(x) lowbit(w), lowbit(b)) and bounded by
    abs_sum = sum |x_k w_k| + |b| < 2^24 unit: then all of them, in any order, are exact f32 values."""
    unit = lowest_bit(x) * lowest_bit(w)
    if bool((b != 0).any()):
        unit = min(unit, lowest_bit(b))
    worst = float(abs_sum.max()) if abs_sum.numel() else 0.0
    if not worst < 2.0 ** 24 * unit:
        raise AssertionError(f"{what}: exact-grid precondition broken: sum |x w| + |b| reaches {worst} >= 2^24 x {unit}")


# ------------------------------------------------------------------------------------------------------------------ operands
def unpack_tower(w0p: torch.Tensor, wp: torch.Tensor, channels: int):
    """Inverse of pack_tower_weights' fragment order: (conv0 [C, 2, 3, 3], [conv [C, C, 3, 3]] per layer), float64.  Asserts
    the round trip (unpack, pack again) reproduces the packed bits and that the padding of w0 is zero."""
    c = channels
    mt, kc = c // 16, c // 32
    p0 = w0p.double().reshape(3, mt, 4, 16, 8)                            # [s, m, g, co_l, j]
    w0 = torch.zeros(c, 2, 9, dtype=D)
    for s in range(3):
        for g in range(4):
            if 4 * s + g < 9:
                w0[:, :, 4 * s + g] = p0[s, :, g, :, 0:2].reshape(c, 2)
    layers = []
    for lw in wp.double().reshape(-1, 9, mt, kc, 4, 16, 8):               # [tap, m, kc, g, co_l, j]
        layers.append(lw.permute(1, 4, 2, 3, 5, 0).reshape(c, c, 3, 3))   # [co, ci, tap] -> [co, ci, kh, kw]
    w0 = w0.reshape(c, 2, 3, 3)
    r0, rw, _ = pack_tower_weights([w0.float()] + [w.float() for w in layers], [torch.zeros(c)] * (1 + len(layers)), c)
    assert torch.equal(r0.to(w0p.dtype), w0p.cpu()) and torch.equal(rw.to(wp.dtype).reshape(wp.shape), wp.cpu()), "unpack_tower does not invert pack_tower_weights"
    return w0, layers


def permute_chw(w: torch.Tensor, channels: int) -> torch.Tensor:
    """A first hidden layer's weights over "c h w" features -> over the tower's cell-major [cell][channel] features."""
    n = w.shape[0]
    return w.reshape(n, channels, 42).permute(0, 2, 1).reshape(n, 42 * channels)


def operands_from_model(model) -> dict:
    """The bf16 evaluator's operands as InferenceNet prepares them for the HIP kernels, restated: BN folded (eval statistics),
    tower weights bf16 and packed, tower and output biases f32, hidden weights bf16 with the first layers' columns permuted to
    cell-major and merged (policy rows first), hidden biases rounded to bf16 (then widened to f32 for the GEMM's epilogue)."""
    c = model.config.conv_filter_size
    conv_w, conv_b = [model.conv[0].weight.detach().float()], [model.conv[0].bias.detach().float()]
    for blk in list(model.conv)[1:]:
        c1, c2, bn = blk.block[0], blk.block[1], blk.block[2]
        conv_w.append(c1.weight.detach().float())
        conv_b.append(c1.bias.detach().float())
        w, b = _fold_bn(c2.weight, c2.bias, bn)
        conv_w.append(w)
        conv_b.append(b)
    w0, w, bias = pack_tower_weights(conv_w, conv_b, c)

    def head(seq):
        mods = list(seq)
        ws, bs = [], []
        for m in mods[:-2]:
            wf, bf = _fold_bn(m[0].weight, m[0].bias, m[1])
            ws.append(wf.bfloat16())
            bs.append(bf.bfloat16().float())
        return ws, bs, mods[-2].weight.detach().bfloat16(), mods[-2].bias.detach().float()

    pw, pb, pow_, pob = head(model.fc_policy)
    vw, vb, vow, vob = head(model.fc_value)
    for ws in (pw, vw):
        if ws:
            ws[0] = permute_chw(ws[0], c)
    if not pw:
        pow_ = permute_chw(pow_, c)
    if not vw:
        vow = permute_chw(vow, c)
    return {"channels": c, "n_blocks": len(model.conv) - 1, "tw0": w0.bfloat16(), "tw": w.bfloat16(), "tbias": bias,
            "pol_w": pw, "pol_b": pb, "val_w": vw, "val_b": vb, "pol_out_w": pow_, "pol_out_b": pob, "val_out_w": vow, "val_out_b": vob}


def operands_from_net(net) -> dict:
    """The same dict from a bf16 HIP InferenceNet's own device tensors (what its kernels are handed)."""
    c = net.channels
    b32 = lambda b: net._bias32[b.data_ptr()]
    return {"channels": c, "n_blocks": net.n_blocks, "tw0": net.tw0, "tw": net.tw, "tbias": net.tbias,
            "pol_w": list(net.pol_w[:-1]), "pol_b": [b32(b) for b in net.pol_b[:-1]],
            "val_w": list(net.val_w[:-1]), "val_b": [b32(b) for b in net.val_b[:-1]],
            "pol_out_w": net.pol_w[-1], "pol_out_b": net.pol_b32, "val_out_w": net.val_w[-1], "val_out_b": net.val_b32}


# ------------------------------------------------------------------------------------------------------------------ the chain
def _conv(x, w, b, mut=frozenset(), last=False):
    """3x3 'same' convolution of cell-major x [G, 6, 7, Ci] with w [Co, Ci, 3, 3] + b: (s, sum |x w| + |b|), float64."""
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                                      # [G, 8, 9, Ci]
    ap = xp.abs()
    s = b.expand(*x.shape[:3], -1).clone()
    a = b.abs().expand(*x.shape[:3], -1).clone()
    for dr in range(3):
        for dc in range(3):
            wt = w[:, :, dr, dc].t()
            part = xp[:, dr:dr + 6, dc:dc + 7, :] @ wt
            if last and "edge_tap" in mut and (dr, dc) == (1, 2):
                part[:, :, 0, :] = 0
            if last and "wrap" in mut and dc == 2:
                # flattened cells: (r, 7) is (r + 1, 0), r = h + dr - 1; past the last row it is zero
                nxt = F.pad(x, (0, 0, 0, 0, 0, 2))[:, dr:dr + 6, 0, :]
                part[:, :, 6, :] = nxt @ wt
            s = s + part
            a = a + ap[:, dr:dr + 6, dc:dc + 7, :] @ wt.abs()
    return s, a


def tower(planes: torch.Tensor, ops: dict, mut=frozenset(), check: bool = True, stats: dict = None) -> torch.Tensor:
    """bf16 planes [G, 2, 6, 7] -> the tower's features [G, 42 C] (cell-major), float64 holding bf16 values.

    Rounding points (include/c4a0_hip.h): conv0 -> bf16; first conv of a block -> bf16, no ReLU; second conv (BN folded)
    y = bf16(x + relu(s)), the add in f32 from the bf16 residual x.  Biases f32.  stats (optional) collects what the tests of
    the data's coverage need."""
    c, nb = ops["channels"], ops["n_blocks"]
    dev = planes.device
    w0, ws = unpack_tower(ops["tw0"].cpu(), ops["tw"].cpu(), c)
    w0, ws = w0.to(dev), [w.to(dev) for w in ws]
    bias = ops["tbias"].double().to(dev)
    x = planes.double().permute(0, 2, 3, 1)                                # [G, 6, 7, 2]
    s, a = _conv(x, w0, bias[0], mut, last=nb == 0)
    if check:
        check_exact(x, w0, bias[0], a, "conv0")
    if nb == 0 and "bias_last" in mut:
        s[..., 0] -= bias[0][0]
    x = bf16(s, mut, "conv0")
    if stats is not None:
        stats.setdefault("ties", []).append(ties(s))
        stats["conv0"] = x
    for i in range(nb):
        last = i == nb - 1
        w1, w2, b1, b2 = ws[2 * i], ws[2 * i + 1], bias[1 + 2 * i], bias[2 + 2 * i]
        s1, a1 = _conv(x, w1, b1)
        if check:
            check_exact(x, w1, b1, a1, f"block {i} conv 1")
        t = bf16(s1, mut, f"block {i} conv 1")
        if last and "relu1" in mut:
            t = torch.relu(t)
        s2, a2 = _conv(t, w2, b2, mut, last)
        if check:
            check_exact(t, w2, b2, a2, f"block {i} conv 2")
        if last and "bias_last" in mut:
            s2[..., 0] -= b2[0]
        r = torch.relu(s2)
        y = r if (last and "no_residual" in mut) else x + r
        if check:   # the residual add is one more f32 operation: exact when both terms sit on a common grid below 2^24 units
            unit = min(lowest_bit(x), lowest_bit(r))
            assert float((x.abs() + r.abs()).max()) < 2.0 ** 24 * unit, f"block {i}: the residual add x + relu(s) is not exact in f32"
        if stats is not None:
            stats["ties"] += [ties(s1), ties(y)]
            stats.setdefault("conv1", []).append(s1)
            stats.setdefault("changed", []).append(float((r != 0).double().mean()))
        x = bf16(y, mut, f"block {i} conv 2")
    return x.reshape(x.shape[0], 42 * c)


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, relu: bool, mut=frozenset(), check: bool = True,
           stats: dict = None) -> torch.Tensor:
    """c4_linear_bf16: bf16(act(sum_k x w + b)), x [m, k] bf16 values, w [n, k] bf16, b f32 [n]; float64 result."""
    x, w, b = x.double(), w.double(), b.double()
    if "drop_ktile" in mut:
        x, w = x[:, :-64], w[:, :-64]
    s = x @ w.t() + b
    if check:
        check_exact(x, w, b, x.abs() @ w.abs().t() + b.abs(), f"linear {tuple(x.shape)} x {tuple(w.shape)}")
    if "bias_last" in mut:
        s[:, 0] -= b[0]
    if relu:
        s = torch.relu(s)
    if stats is not None:
        stats.setdefault("ties", []).append(ties(s))
    y = bf16(s, mut, "linear")
    if "row_offset" in mut and y.shape[0] >= 192:
        y[64:128] = y[128:192]
    return y


def interval(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, relu: bool):
    """Rigorous bounds (lo, hi) on c4_linear_bf16's output for ANY f32-or-wider summation order of the K products and the
    bias: |chain - s| <= gamma_{K+1} (sum |x w| + |b|), gamma_n = n u / (1 - n u), u = 2^-24 (every product of two bf16 is
    exact in f32); the float64 s itself is within K 2^-53 of the same sum.  Then the output lies in
    [act(RD_bf16(s - e)), act(RU_bf16(s + e))] for round-to-nearest of the f32 result."""
    x, w, b = x.double(), w.double(), b.double()
    k = x.shape[1]
    s = x @ w.t() + b
    a = x.abs() @ w.abs().t() + b.abs()
    n = k + 1
    e = (n * U / (1 - n * U) + k * 2.0 ** -53) * a
    lo, hi = bf16_directed(s - e, up=False), bf16_directed(s + e, up=True)
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    return lo, hi


def head_preact(hp: torch.Tensor, hv: torch.Tensor, ops: dict, check: bool = True) -> torch.Tensor:
    """The output layers' pre-activations [G, 9] (7 policy logits, 2 value) in float64 (exact f32 values on grid operands)."""
    out = []
    for h, w, b in ((hp, ops["pol_out_w"], ops["pol_out_b"]), (hv, ops["val_out_w"], ops["val_out_b"])):
        h, w, b = h.double(), w.double().to(h.device), b.double().to(h.device)
        s = h @ w.t() + b
        if check:
            check_exact(h, w, b, h.abs() @ w.abs().t() + b.abs(), "head out")
            assert_f32(s, "head out")
        out.append(s)
    return torch.cat(out, dim=1)


def hidden(planes: torch.Tensor, ops: dict, mut=frozenset(), check: bool = True, stats: dict = None):
    """InferenceNet.forward_hidden: planes -> (policy head's last hidden activations, value head's), float64 bf16 values."""
    c = ops["channels"]
    dev = planes.device
    x = tower(planes, ops, mut, check, stats)
    mv = lambda t: t.to(dev)

    first = mv
    if "no_perm" in mut:   # the first layers' columns as the model stores them ("c h w"), read as if cell-major
        first = lambda w: mv(w).reshape(w.shape[0], 42, c).permute(0, 2, 1).reshape(w.shape[0], 42 * c)
    p = v = x
    for j, (w, b) in enumerate(zip(ops["pol_w"], ops["pol_b"])):
        p = linear(p, first(w) if j == 0 else mv(w), mv(b), True, mut, check, stats)
    for j, (w, b) in enumerate(zip(ops["val_w"], ops["val_b"])):
        v = linear(v, first(w) if j == 0 else mv(w), mv(b), True, mut, check, stats)
    return p, v


# ------------------------------------------------------------------------------------------------------------------ generators
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def grid_planes(n: int, seed: int) -> torch.Tensor:
    """bf16 [n, 2, 6, 7] of 0 / 1 with both planes set in places (the kernels do not care that a real board cannot)."""
    g = _gen(seed)
    return (torch.rand(n, 2, 6, 7, generator=g) < 0.45).bfloat16()


def _sparse_signs(rows: int, cols: int, per_row: int, g, cover: bool = True) -> torch.Tensor:
    """rows x cols of 0 / +-1 with about per_row (at least one) nonzeros per row; cover: every column holds at least one
    (columns dealt round-robin to shuffled rows, which alone gives cols / rows per row)."""
    w = torch.zeros(rows, cols, dtype=D)
    w[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 1.0
    base = 1.0
    if cover:
        owner = torch.randperm(cols, generator=g) % rows
        w[owner, torch.arange(cols)] = 1.0
        base = max(1.0, cols / rows)
    extra = torch.rand(rows, cols, generator=g) < max(0.0, per_row - base) / cols
    w[extra] = 1.0
    sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0).double()
    return w * sign


def grid_tower_weights(channels: int, n_blocks: int, seed: int, per_row: float = 0):
    """Exact-grid conv weights and biases (float32 tensors: conv_w [C, Ci, 3, 3], conv_b [C]) for 1 + 2 n_blocks layers.
    Weights are sparse 0 / +-1 -- by default every (ci, tap) column of every layer used, 9 per output channel; per_row > 0:
    about per_row per output channel without that guarantee (deep towers, whose stream would outgrow the exact range) --,
    biases integers: activations stay integers through every bf16 rounding.  conv0 spreads the features over about
    [-300, 500] so that they carry 9+ significant bits (rounding, ties); each block's second bias is negative enough that
    the ReLU drops a good part of the update."""
    c = channels
    g = _gen(seed)
    conv_w = [torch.randint(-3, 4, (c, 2, 3, 3), generator=g).double()]
    conv_b = [torch.randint(-300, 501, (c,), generator=g).double()]

    def layer():
        w = _sparse_signs(c, 9 * c, per_row or 9, g, cover=not per_row)
        return w.reshape(c, 9, c).permute(0, 2, 1).reshape(c, c, 3, 3).contiguous()   # column = tap C + ci
    for _ in range(n_blocks):
        conv_w.append(layer())
        conv_b.append(torch.randint(-64, 65, (c,), generator=g).double())
        conv_w.append(layer())
        conv_b.append(torch.randint(-1500, 101, (c,), generator=g).double())
    return [w.float() for w in conv_w], [b.float() for b in conv_b]


def grid_linear(m: int, k: int, n: int, seed: int):
    """Exact-grid GEMM operands: x [m, k] bf16 on the 2^-6 grid (|i| <= 256, a third zeros, like post-ReLU rows), w [n, k]
    bf16 on the 2^-6 grid (|j| <= 16, half zeros, every k column used), bias f32 on the 2^-12 grid.  The last 192 output
    columns are tie columns: ONE nonzero weight each, so that y = x_k w + b often has exactly 9 significant bits."""
    g = _gen(seed)
    x = torch.randint(-256, 257, (m, k), generator=g).double()
    x[torch.rand(m, k, generator=g) < 0.33] = 0
    w = torch.randint(-16, 17, (n, k), generator=g).double()
    w[torch.rand(n, k, generator=g) < 0.5] = 0
    w[torch.randint(0, n, (k,), generator=g), torch.arange(k)] = torch.where(torch.rand(k, generator=g) < 0.5, -3.0, 5.0).double()
    b = torch.randint(-2 ** 14, 2 ** 14 + 1, (n,), generator=g).double()
    t = 192
    w[n - t:] = 0
    w[n - t + torch.arange(t), torch.randint(0, k, (t,), generator=g)] = torch.randint(-16, 17, (t,), generator=g).double().clamp(min=1) * 2 + 1
    b[n - t:] = torch.randint(-2 ** 10, 2 ** 10 + 1, (t,), generator=g).double() * 8
    return (x / 64).bfloat16(), (w / 64).bfloat16(), (b / 4096).float()


def realistic_linear(m: int, k: int, n: int, seed: int):
    """Data of the kind the net produces: post-ReLU activations with many zeros, rows scaled over 2^-20 .. 2^20, weights
    ~ N(0, 1 / k), biases ~ N(0, 1) scaled by 2^-20 .. 2^20 per column (f32, any bits)."""
    g = _gen(seed)
    x = torch.relu(torch.randn(m, k, generator=g))
    x = x * torch.exp2(torch.randint(-20, 21, (m, 1), generator=g).double()).float()
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).double()).float()
    return x.bfloat16(), w.bfloat16(), b.float()


def set_grid_model(model, seed: int, per_row: float = 0):
    """Grid-valued weights set THROUGH the model (ConnectFourNet): tower as grid_tower_weights, BN with eps = 0, var = 1 and
    mean / gamma / beta on the grid (gamma 1 or 2), so that InferenceNet's fold is exact; hidden Linear weights sparse
    (about 3 per row, every input column used), biases on the 2^-3 grid with bits below bf16's (rounded by the net);
    output layers sparse 0 / +-1 as well.  Returns the model."""
    c, nb = model.config.conv_filter_size, model.config.n_residual_blocks
    g = _gen(seed + 1)
    cw, cb = grid_tower_weights(c, nb, seed, per_row)
    with torch.no_grad():
        model.conv[0].weight.copy_(cw[0])
        model.conv[0].bias.copy_(cb[0])
        for i, blk in enumerate(list(model.conv)[1:]):
            c1, c2, bn = blk.block[0], blk.block[1], blk.block[2]
            c1.weight.copy_(cw[1 + 2 * i])
            c1.bias.copy_(cb[1 + 2 * i])
            gamma = torch.where(torch.rand(c, generator=g) < 0.25, 2.0, 1.0)
            mean = torch.randint(-8, 9, (c,), generator=g).float() / 8
            beta = torch.randint(-8, 9, (c,), generator=g).float() / 8
            # fold: w' = gamma w2, b' = (b2 - mean) gamma + beta: w2, b2 chosen so that w', b' are grid_tower_weights' (exact)
            c2.weight.copy_(cw[2 + 2 * i] / gamma.reshape(-1, 1, 1, 1))
            c2.bias.copy_((cb[2 + 2 * i] - beta) / gamma + mean)
            bn.eps = 0.0
            bn.running_var.fill_(1.0)
            bn.running_mean.copy_(mean)
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        f = 42 * c
        for seq in (model.fc_policy, model.fc_value):
            mods = list(seq)
            for m in mods[:-2]:
                lin, bn = m[0], m[1]
                lin.weight.copy_(_sparse_signs(f, f, 3, g).float())
                lin.bias.copy_(torch.randint(-4096, 4097, (f,), generator=g).float() / 8)
                bn.eps = 0.0
                bn.running_var.fill_(1.0)
                bn.running_mean.copy_(torch.randint(-8, 9, (f,), generator=g).float() / 8)
                bn.weight.fill_(1.0)
                bn.bias.copy_(torch.randint(-8, 9, (f,), generator=g).float() / 8)
            out = mods[-2]
            out.weight.copy_(_sparse_signs(out.weight.shape[0], f, 3, g, cover=False).float())
            out.bias.copy_(torch.randint(-64, 65, (out.weight.shape[0],), generator=g).float() / 8)
    return model


# ------------------------------------------------------------------------------------------------------------------ GPU cases
# The inputs tests/test_gpu_bf16_exact.py feeds the kernels: tests/test_bf16_ref.py checks on the CPU that they meet the
# exactness precondition, cover what they must and tell every MUTATIONS entry from the true chain.
GEMM_SHAPES = [(1344, 1344), (1344, 2688), (2688, 2688), (2688, 5376)]   # (K, N): the 32- and 64-channel nets' layers
GEMM_M = 4096


def gemm_case(k: int, n: int, m: int = GEMM_M):
    """(x, w, b) of the exact-grid GEMM test; m < GEMM_M: the first m rows of the same data."""
    x, w, b = grid_linear(GEMM_M, k, n, seed=k + n)
    return x[:m], w, b


TOWER_BLOCKS = [0, 1, 2, 8]
TOWER_N = 2049   # boards: above every automatic cut (512, 1 024, 1 280) with a ragged last workgroup


def tower_per_row(n_blocks: int) -> float:
    """Nonzero weights per output channel: up to two blocks every (ci, tap) column is used (9 per channel); deeper towers
    get sparser weights so that their residual stream stays inside the exact range."""
    return 0 if n_blocks <= 2 else (2 if n_blocks <= 8 else 0.5)


def tower_case(channels: int, n_blocks: int, n: int = TOWER_N):
    """(planes [n, 2, 6, 7] bf16, ops) of the exact-grid tower test."""
    cw, cb = grid_tower_weights(channels, n_blocks, seed=100 * channels + n_blocks, per_row=tower_per_row(n_blocks))
    w0, w, b = pack_tower_weights(cw, cb, channels)
    ops = {"channels": channels, "n_blocks": n_blocks, "tw0": w0.bfloat16(), "tw": w.bfloat16(), "tbias": b}
    return grid_planes(TOWER_N, seed=channels + n_blocks)[:n], ops


EVAL_SHAPES = [(4, 32), (8, 64)]   # BASELINE's nets, heads 4 / 2


def eval_model(blocks: int, channels: int):
    from c4a0_amd.nn import ConnectFourNet, ModelConfig

    return set_grid_model(ConnectFourNet(ModelConfig(blocks, channels, 4, 2)).eval(), seed=blocks * channels,
                          per_row=tower_per_row(blocks))
