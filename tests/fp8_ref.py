"""A float64 restatement of the fp8 hidden layers (c4_quantize_bf16_fp8, c4_linear_fp8): include/c4a0_hip.h, "fp8 hidden layers".

Codes are OCP e4m3fn bytes (uint8 tensors).  `q8` is written here with integer arithmetic on the f32 bit pattern -- no float8 cast
of torch's -- and `decode` is a 256-entry table built from the format's definition.  Sums and products are float64; a value is
rounded only where the kernels round, and only after it is asserted to be exactly an f32.  On operands from `grid_case` every
partial sum of every output, in ANY order, is an exact f32 (integer-valued codes, power-of-two dq, bias on dq's grid), so the
kernel's result does not depend on the MFMA's accumulation order and must equal this reference bit for bit.  For arbitrary data
`interval_codes` / `interval_bf16` give the bounds any f32-or-wider summation order satisfies, pushed through the monotone output
rounding.

`mut` (a set of names, MUTATIONS) switches on plausible kernel bugs, so that tests/test_fp8_ref.py can show the GPU tests' inputs
tell each of them from the true layer."""
from __future__ import annotations

import torch

from tests.bf16_ref import D, U, assert_f32, bf16, bf16_directed, pow2

MUTATIONS = {
    "trunc": "output rounding by truncation instead of round-to-nearest-even",
    "away": "output rounding with ties away from zero",
    "noclamp": "no clamp in front of the convert: an overflow becomes NaN",
    "flush": "e4m3 subnormal results flushed to zero",
    "fnuz": "the fnuz format's exponent bias (8) in the output conversion",
    "drop_half": "the last half k-step (64 columns of a k that is 64 mod 128) dropped",
    "read_far": "the last half k-step reads 64 columns too far (the activations' row goes on, the weights' next row begins)",
    "dq_after_bias": "dq applied after the bias: (acc + bias) dq",
    "relu_after_round": "the relu after the output rounding, keeping the -0 a small negative value rounds to",
}

NAN_CODE = 0x7F
MAX_BITS = 0x43E00000   # f32 bits of 448.0


# ------------------------------------------------------------------------------------------------------------------ the format
def _decode_table() -> torch.Tensor:
    t = torch.zeros(256, dtype=D)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (8 + m) * 2.0 ** (e - 10)       # (1 + m / 8) 2^(e - 7)
        t[c] = -v if c & 0x80 else v
    return t


DECODE = _decode_table()


def decode(codes: torch.Tensor) -> torch.Tensor:
    """e4m3fn codes (uint8) -> float64 values (NaN for 0x7F / 0xFF; 0x80 is -0)."""
    return DECODE.to(codes.device)[codes.to(torch.int64)]


def q8(t: torch.Tensor, mut=frozenset(), what: str = "value") -> torch.Tensor:
    """float64 t (asserted to be exactly f32, or NaN / inf) -> e4m3fn codes: NaN -> 0x7F; clamp to [-448, 448]; round to nearest,
    ties to even; subnormals and the sign of zero kept.  Integer arithmetic on the f32 bits."""
    fin = torch.isfinite(t)
    assert_f32(torch.where(fin, t, torch.zeros_like(t)), what)
    u = t.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    sign = (u >> 31) & 1
    a = u & 0x7FFFFFFF
    nan = a > 0x7F800000
    if "fnuz" in mut:                                           # bias 8: a value is encoded as the OCP code of twice the value
        a = torch.where((a >= 0x00800000) & (a < 0x7F000000), a + 0x00800000, a)
    over = a > MAX_BITS
    if "noclamp" not in mut:
        a = torch.where(over, torch.full_like(a, MAX_BITS), a)
    e = (a >> 23) - 127                                         # a = 1.man x 2^e (f32 subnormals: below every e4m3 step, see shift)
    sig = (a & 0x7FFFFF) | 0x800000
    normal = e >= -6
    shift = torch.where(normal, torch.full_like(e, 20), torch.clamp(14 - e, max=40))
    fl = sig >> shift
    rem = sig & ((torch.ones_like(sig) << shift) - 1)
    half = torch.ones_like(sig) << (shift - 1)
    if "trunc" in mut:
        up = torch.zeros_like(fl)
    elif "away" in mut:
        up = (rem >= half).to(torch.int64)
    else:
        up = ((rem > half) | ((rem == half) & ((fl & 1) == 1))).to(torch.int64)
    n = fl + up
    code = torch.where(normal, ((e + 6) << 3) + n, n)           # a carry out of the significand lands in the exponent field
    code = torch.where((a >> 23) == 0, torch.zeros_like(code), code)
    if "flush" in mut:
        code = torch.where(code < 8, torch.zeros_like(code), code)
    overflow = (code > 0x7E) | (e > 8)
    code = torch.where(overflow, torch.full_like(code, NAN_CODE), code)
    code = torch.where(overflow, code, code | (sign << 7))
    code = torch.where(nan, torch.full_like(code, NAN_CODE), code)
    return code.to(torch.uint8)


def q8_directed(t: torch.Tensor, up: bool) -> torch.Tensor:
    """The e4m3 VALUE (float64) next below (up=False) or above (up=True) the clamped float64 t: the monotone envelope of q8."""
    c = torch.clamp(t, -448.0, 448.0)
    m, e = torch.frexp(c)
    ulp = pow2(torch.clamp(e - 4, min=-9))
    q = c / ulp
    q = torch.ceil(q) if up else torch.floor(q)
    return torch.where(c == 0, c, q * ulp)


# ------------------------------------------------------------------------------------------------------------------ the kernels
def quantize(x_bf16: torch.Tensor, scale: float, mut=frozenset()) -> torch.Tensor:
    """c4_quantize_bf16_fp8: q8(x scale), x bf16, scale a power of two (an exact f32 multiply unless it leaves f32's range)."""
    v = (x_bf16.double() * scale).float().double()             # the kernel's f32 multiply: exact, or f32's own overflow / underflow
    return q8(v, mut, "quantize")


def _acc(x8: torch.Tensor, wq: torch.Tensor, k: int, mut=frozenset()):
    """(acc, sum |x w|) of x8[:, :k] . wq^T in float64; x8 may be wider than k (a column view: what lies behind must not matter)."""
    w = decode(wq)
    kk = k
    if "drop_half" in mut and k % 128 == 64:
        kk = k - 64
    x = decode(x8[:, :kk])
    acc = x @ w[:, :kk].t()
    a = x.abs() @ w[:, :kk].abs().t()
    if "read_far" in mut and k % 128 == 64:
        xf = torch.zeros(x8.shape[0], 64, dtype=D)
        have = min(64, x8.shape[1] - k)
        xf[:, :have] = decode(x8[:, k:k + have])
        wf = torch.zeros(w.shape[0], 64, dtype=D)               # row n goes on with the first 64 weights of row n + 1
        wf[:-1] = w[1:, :64]
        acc = acc + xf @ wf.t()
    return acc, a


def _finish(acc, dq, bias, relu: bool, mut=frozenset(), exact: bool = True):
    """acc -> r: v = acc dq + bias (an exact multiply, one f32 rounding in the add), r = relu ? (v <= 0 ? +0 : v) : v."""
    dq, bias = dq.double(), bias.double()
    if "dq_after_bias" in mut:
        v = (acc + bias) * dq
    else:
        p = acc * dq
        if exact:
            assert_f32(torch.where(torch.isfinite(p), p, torch.zeros_like(p)), "acc dq")
        v = p + bias
    if exact:
        assert_f32(torch.where(torch.isfinite(v), v, torch.zeros_like(v)), "acc dq + bias")
    if relu and "relu_after_round" not in mut:
        v = torch.where(v <= 0, torch.zeros_like(v), v)
    return v


def linear(x8, wq, dq, bias, k: int, relu: bool, out_fp8: bool, out_scale: float = 1.0, mut=frozenset(), stats: dict = None) -> torch.Tensor:
    """c4_linear_fp8 on exact-grid operands: uint8 codes [m, n] (out_fp8) or bf16 values as float64."""
    acc, _ = _acc(x8, wq, k, mut)
    assert_f32(torch.where(torch.isfinite(acc), acc, torch.zeros_like(acc)), "acc")
    r = _finish(acc, dq, bias, relu, mut)
    if not out_fp8:
        if relu and "relu_after_round" in mut:
            r = torch.where(r < 0, torch.zeros_like(r), r)
        fin = torch.isfinite(r)
        y = bf16(torch.where(fin, r, torch.zeros_like(r)), mut, "linear_fp8 -> bf16")
        return torch.where(fin, y, r)
    s = r * out_scale
    if stats is not None:
        stats["pre_round"] = s
    codes = q8(s, mut, "r out_scale")
    if relu and "relu_after_round" in mut:                      # relu on the rounded value, by comparison: -0 passes
        codes = torch.where((decode(codes) < 0), torch.zeros_like(codes), codes)
    return codes


def bounds(x8, wq, dq, bias, k: int, relu: bool):
    """(lo, hi) float64 around r for ANY f32-or-wider order of the k products: |acc_f32 - acc| <= gamma_k sum |x w| (a product of
    two e4m3 values is exact in f32), acc dq exact, then one f32 rounding of the add (relative 2^-24, and an absolute 2^-149 where it
    lands among f32 subnormals)."""
    acc, a = _acc(x8, wq, k)
    dq, bias = dq.double(), bias.double()
    e = (k * U / (1 - k * U) + k * 2.0 ** -53) * a * dq
    s = acc * dq + bias
    e = e + (s.abs() + e) * (U + 2.0 ** -52) + 2.0 ** -149
    lo, hi = s - e, s + e
    if relu:
        lo, hi = torch.where(lo <= 0, torch.zeros_like(lo), lo), torch.where(hi <= 0, torch.zeros_like(hi), hi)
    return lo, hi


def interval_codes(x8, wq, dq, bias, k: int, relu: bool, out_scale: float, pre=None):
    """Bounds (lo, hi), as e4m3 VALUES, on the value of c4_linear_fp8's fp8 output for finite operands (pre: bounds() for
    the same operands, computed once for both output modes)."""
    lo, hi = pre if pre is not None else bounds(x8, wq, dq, bias, k, relu)
    return q8_directed(lo * out_scale, up=False), q8_directed(hi * out_scale, up=True)


def interval_bf16(x8, wq, dq, bias, k: int, relu: bool, pre=None):
    """Bounds (lo, hi) on c4_linear_fp8's bf16 output for finite operands."""
    lo, hi = pre if pre is not None else bounds(x8, wq, dq, bias, k, relu)
    return bf16_directed(lo, up=False), bf16_directed(hi, up=True)


# ------------------------------------------------------------------------------------------------------------------ generators
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def int_codes(v: torch.Tensor) -> torch.Tensor:
    """Integer values in [-16, 16] -> their (exact) e4m3 codes."""
    assert bool((v.abs() <= 16).all()) and bool((v == v.round()).all())
    c = q8(v.double())
    assert torch.equal(decode(c), v.double())
    return c


def grid_case(m: int, k: int, n: int, seed: int):
    """Exact-grid operands of one c4_linear_fp8 call: x8 [m, k] and Wq [n, k] integer-valued codes in [-8, 8], dq[c] = 2^d_c,
    bias[c] = (an integer) 2^d_c, out_scale = 2^4: v = (acc + b) 2^d_c exactly, every partial sum an integer below 2^24 units.
    The columns are dealt four kinds by c % 8, so that the outputs spread over the whole e4m3 range:
      0, 1  small sums (8 nonzero weights, |b| <= 24) with d_c = -14: r out_scale = i 2^-10 -- e4m3 subnormals, every odd i a tie;
      2     small sums with d_c from -11 .. -6: the low binades, many ties;
      3     dense weights with d_c = +2: saturated (far beyond 448);
      4..7  dense weights, d_c from -12 .. -3: the whole normal range, some saturated.
    Nonzero weights of the small columns sit in the first AND the last 64 columns of k (the half k-step must count)."""
    g = _gen(seed)
    x = torch.randint(-8, 9, (m, k), generator=g).double()
    x[torch.rand(m, k, generator=g) < 0.3] = 0
    w = torch.randint(-8, 9, (n, k), generator=g).double()
    w[torch.rand(n, k, generator=g) < 0.4] = 0
    w[torch.randint(0, n, (k,), generator=g), torch.arange(k)] = 5.0      # every k column used
    kind = torch.arange(n) % 8
    small = kind <= 2
    ws = torch.zeros(n, k, dtype=D)
    for j in range(4):                                                     # 4 nonzeros in the first 64 columns, 4 in the last 64
        for base in (0, k - 64):
            ws[torch.arange(n), base + torch.randint(0, 64, (n,), generator=g)] = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    w = torch.where(small[:, None], ws, w)
    d = torch.randint(-12, -2, (n,), generator=g)
    d = torch.where(kind <= 1, torch.full_like(d, -14), d)
    d = torch.where(kind == 2, torch.randint(-11, -5, (n,), generator=g), d)
    d = torch.where(kind == 3, torch.full_like(d, 2), d)
    b = torch.randint(-1000, 1001, (n,), generator=g).double()
    b = torch.where(small, torch.randint(-24, 25, (n,), generator=g).double(), b)
    dq = pow2(d)
    return int_codes(x), int_codes(w), dq.float(), (b * dq).float(), 16.0


def realistic_case(m: int, k: int, n: int, seed: int):
    """Finite e4m3 operands of the kind the net produces: post-ReLU activations with many zeros quantised at a calibrated scale,
    weights ~ N(0, 1 / k) quantised by the row rule, f32 biases ~ N(0, 0.1): (x8, wq, dq, bias, out_scale)."""
    from c4a0_amd.nn import activation_exponent, quantize_head_weights

    g = _gen(seed)
    x = torch.relu(torch.randn(m, k, generator=g)).bfloat16()
    e_x = activation_exponent(float(x.float().abs().max()))
    w = torch.randn(n, k, generator=g) / k ** 0.5
    wq, e_w = quantize_head_weights(w)
    dq = pow2(-e_x - e_w.to(torch.int64)).float()
    return quantize(x, 2.0 ** e_x), wq, dq, (torch.randn(n, generator=g) * 0.1).float(), 2.0 ** activation_exponent(4.0)


# ------------------------------------------------------------------------------------------------------------------ GPU cases
# The inputs tests/test_gpu_fp8_exact.py feeds the kernels; tests/test_fp8_ref.py checks on the CPU that they meet the exactness
# precondition, hold the ties / saturated / subnormal shares and tell every MUTATIONS entry from the true layer.
SMALL_SHAPES = [(64, 192), (128, 192), (192, 384)]               # (k, n)
LARGE_SHAPES = [(1344, 1344), (1344, 2688), (2688, 2688)]
SMALL_M = [1, 15, 17, 127, 129, 300]
GEMM_M = 300
PAD = 64                                                          # columns behind x8's k: 0x7F (NaN) and 0x7E (448) alternating


def gemm_case(k: int, n: int, m: int = GEMM_M):
    """(x8 [m, k + PAD] with the sentinel columns behind k, wq, dq, bias, out_scale); m < GEMM_M: the first m rows of the same data."""
    x8, wq, dq, bias, s = grid_case(GEMM_M, k, n, seed=k + n)
    pad = torch.where(torch.arange(PAD) % 2 == 0, NAN_CODE, 0x7E).to(torch.uint8).expand(GEMM_M, PAD)
    return torch.cat([x8, pad], dim=1)[:m].contiguous(), wq, dq, bias, s


def shares(s: torch.Tensor):
    """(ties, saturated, subnormal) shares among the exact values s about to be rounded to e4m3."""
    a = s.abs()
    u = a.float().view(torch.int32).to(torch.int64)
    e = (u >> 23) - 127
    sig = (u & 0x7FFFFF) | 0x800000
    shift = torch.where(e >= -6, torch.full_like(e, 20), torch.clamp(14 - e, max=40))
    rem = sig & ((torch.ones_like(sig) << shift) - 1)
    tie = (rem == (torch.ones_like(sig) << (shift - 1))) & (a > 0) & (a <= 448)
    sat = a > 448
    sub = (a > 0) & (a < 2.0 ** -6)
    n = s.numel()
    return float(tie.sum()) / n, float(sat.sum()) / n, float(sub.sum()) / n
