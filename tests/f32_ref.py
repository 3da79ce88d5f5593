"""The plain-C reference of the f32 evaluator (tests/f32_net_ref.c, built here with gcc -ffp-contract=off) and a forward
pass composed from it: every intermediate the GPU chain exposes, in the same padded layouts.  Further down: its wrong twins
(tests/f32_net_mutants.c) and the operand sets of the kernels' edge tests."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import torch

from c4a0_amd.nn import InferenceNet, pack_f32_weights

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_mut_lib = None


def _build(source: str) -> C.CDLL:
    out = os.path.join(tempfile.mkdtemp(prefix="f32ref"), "lib" + source[:-2] + ".so")
    cmd = ["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-shared", "-fPIC",
           os.path.join(HERE, source), "-o", out, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(out)


def ref_lib():
    global _lib
    if _lib is None:
        L = _build("f32_net_ref.c")
        fp, i = C.c_void_p, C.c_int
        L.f32ref_linear.argtypes = [fp, i, fp, fp, fp, i, i, i, i, i]
        L.f32ref_conv0.argtypes = [fp, i, i, fp, fp, fp]
        L.f32ref_conv.argtypes = [fp, i, i, fp, fp, fp, fp]
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pack_on_cpu(model) -> dict:
    """pack_f32_weights of the BN-folded model (folded by InferenceNet on the CPU, the PyTorch path), as numpy arrays."""
    net = InferenceNet(model, torch.device("cpu"), dtype=torch.float32)
    pk = pack_f32_weights([w.contiguous() for w in net.conv_w], net.conv_b, net.pol_w, net.pol_b, net.val_w, net.val_b, net.channels)
    out = {k: (v.numpy() if isinstance(v, torch.Tensor) else ([t.numpy() for t in v] if isinstance(v, list) else v)) for k, v in pk.items()}
    out["n_blocks"] = net.n_blocks
    return out


def linear(x, w, b, act):
    x, w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, b))
    y = np.empty((x.shape[0], w.shape[0]), np.float32)
    ref_lib().f32ref_linear(_p(x), x.shape[1], _p(w), _p(b), _p(y), y.shape[1], x.shape[0], w.shape[0], w.shape[1], int(act))
    return y


def forward(pk: dict, planes: np.ndarray) -> dict:
    """planes f32 [G, 2, 6, 7] -> {"features" [G, 42 Cp], "policy_hidden" / "value_hidden" [list of [G, Hp]], "preact" [G, 9]}."""
    L = ref_lib()
    planes = np.ascontiguousarray(planes, dtype=np.float32)
    g, cp = planes.shape[0], pk["cp"]
    x = np.empty((g, 42 * cp), np.float32)
    L.f32ref_conv0(_p(planes), g, cp, _p(pk["w0"]), _p(pk["bias"][0]), _p(x))
    t = np.empty_like(x)
    for i in range(pk["n_blocks"]):
        L.f32ref_conv(_p(x), g, cp, _p(np.ascontiguousarray(pk["w"][2 * i])), _p(np.ascontiguousarray(pk["bias"][1 + 2 * i])), _p(t), None)
        L.f32ref_conv(_p(t), g, cp, _p(np.ascontiguousarray(pk["w"][2 * i + 1])), _p(np.ascontiguousarray(pk["bias"][2 + 2 * i])), _p(x), _p(x))
    res = {"features": x}
    for name, key in (("policy", "pol"), ("value", "val")):
        h, hidden = x, []
        for w, b in zip(pk[key + "_w"][:-1], pk[key + "_b"][:-1]):
            h = linear(h, w, b, 1)
            hidden.append(h)
        res[name + "_hidden"] = hidden
        res[name + "_out"] = linear(h, pk[key + "_w"][-1], pk[key + "_b"][-1], 0)
    res["preact"] = np.concatenate([res["policy_out"], res["value_out"]], axis=1)
    return res


def log_softmax_documented(v: np.ndarray, expf, logf) -> np.ndarray:
    """The documented log-softmax on f32 pre-activations [G, 7] with the given expf / logf (arrays in, arrays out)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):    # Inf - Inf in the non-finite rows is meant
        return _log_softmax_documented(v, expf, logf)


def _log_softmax_documented(v, expf, logf):
    v = v.astype(np.float32)
    mx = v[:, 0].copy()
    for o in range(1, 7):
        mx = np.fmax(mx, v[:, o])                    # fmaxf: a NaN logit is skipped
    e = expf(np.ascontiguousarray(v - mx[:, None]).reshape(-1)).reshape(v.shape)
    sm = np.zeros(v.shape[0], np.float32)
    for o in range(7):
        sm = (sm + e[:, o]).astype(np.float32)
    lse = (mx + logf(sm)).astype(np.float32)
    return (v - lse[:, None]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# The wrong twins (tests/f32_net_mutants.c) and the operand sets of the edge tests: tests/test_gpu_f32_exact.py feeds them to
# the kernels, tests/test_f32_edges_ref.py shows on the CPU that they tell every twin from the true chain.  Everything is
# generated once per process at the largest batch a shape is run with; a test with fewer rows uses a prefix (a row's outputs
# depend on that row alone).
MUTANTS = {"natural_order": 1, "drop_last_block": 2, "bias_starts_chain": 3, "relu_before_bias": 4, "next_row": 5, "no_board_edge": 6,
           "no_residual": 7, "planes_swapped": 8, "value_row_0": 9}


def mutant_lib():
    global _mut_lib
    if _mut_lib is None:
        L = _build("f32_net_mutants.c")
        fp, i = C.c_void_p, C.c_int
        L.f32mut_linear.argtypes = [fp, i, fp, fp, fp, i, i, i, i, i, i]
        L.f32mut_conv0.argtypes = [fp, i, i, fp, fp, fp, i]
        L.f32mut_conv.argtypes = [fp, i, i, fp, fp, fp, fp, i]
        _mut_lib = L
    return _mut_lib


def linear_mutant(x, w, b, act, mut: int):
    x, w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, b))
    y = np.empty((x.shape[0], w.shape[0]), np.float32)
    mutant_lib().f32mut_linear(_p(x), x.shape[1], _p(w), _p(b), _p(y), y.shape[1], x.shape[0], w.shape[0], w.shape[1], int(act), mut)
    return y


def tower_stages(planes, w0, w, bias, n_blocks: int, mut: int = None) -> list:
    """The features [G, 42 Cp] after conv0 and after each of n_blocks residual blocks (n_blocks + 1 arrays): the true chain
    (mut None: tests/f32_net_ref.c) or a wrong twin."""
    planes, w0, w, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in (planes, w0, w, bias))
    g, cp = planes.shape[0], w0.shape[0]
    L, tail = (ref_lib(), ()) if mut is None else (mutant_lib(), (mut,))
    conv0, conv = (L.f32ref_conv0, L.f32ref_conv) if mut is None else (L.f32mut_conv0, L.f32mut_conv)
    x = np.empty((g, 42 * cp), np.float32)
    conv0(_p(planes), g, cp, _p(w0), _p(bias[0]), _p(x), *tail)
    stages = [x.copy()]
    t = np.empty_like(x)
    for i in range(n_blocks):
        conv(_p(x), g, cp, _p(w[2 * i]), _p(bias[1 + 2 * i]), _p(t), None, *tail)
        conv(_p(t), g, cp, _p(w[2 * i + 1]), _p(bias[2 + 2 * i]), _p(x), _p(x), *tail)
        stages.append(x.copy())
    return stages


def same_bits_or_both_nan(got: np.ndarray, want: np.ndarray) -> bool:
    """NaN where the reference has NaN (payloads are not compared: x86 and the GPU propagate different ones), equal bits elsewhere."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and \
        bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


# ---- c4_linear_f32
LINEAR_SHAPES = [(16, 32), (32, 64), (48, 96), (256, 96), (672, 32), (2688, 64)]          # (k, n)
LINEAR_M = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 129]
LINEAR_M_LARGE = [2047, 2048, 2049, 2111, 4097]      # both sides of the m > 2048 switch to 64-row tiles; 1, 2, 3 idle wavefronts
LINEAR_M_LARGEST = [2049, 2111, 4097]                # ... of which these run on the first four shapes only (the oracle's cost)
RECIPES = ("wide", "realistic")


def linear_rows(k: int, n: int) -> int:
    return 4097 if (k, n) in LINEAR_SHAPES[:4] else 2048


WIDE_JITTER = 8


def wide_operands(m, k, n, seed):
    """Magnitudes over 2^+-30 on both sides and eight subnormal inputs, as in test_gpu_f32_net.py's probe of the order, but with
    the exponents arranged so that every launch shows every twin: input column k carries 2^e[k], weight column k 2^-e[k] (e over
    -22..22), each element a further 2^-8..2^8.  The products then spread over 2^+-16 instead of 2^+-60: hundreds of terms of a
    sum matter to its low bits (heavy cancellation), not the two or three largest, so a change of order shows on twice as many
    outputs and still does where a ReLU zeroes half of them.  The bias of a column is N(0, 1) times the median |sum| of that
    column (from the operands in float64): on the scale of the sums, so that where it joins the chain shows too."""
    rng = np.random.default_rng(seed)
    j = WIDE_JITTER
    e = rng.integers(-30 + j, 30 - j + 1, k)
    x = (rng.standard_normal((m, k)) * np.exp2(e + rng.integers(-j, j + 1, (m, k)))).astype(np.float32)
    w = (rng.standard_normal((n, k)) * np.exp2(-e + rng.integers(-j, j + 1, (n, k)))).astype(np.float32)
    x[0, :8] = np.float32(1e-41)                     # subnormal inputs come through unflushed
    w[0, :8] = np.float32(0.5)
    sums = x[:min(m, 256)].astype(np.float64) @ w.astype(np.float64).T
    return x, w, (rng.standard_normal(n) * np.median(np.abs(sums), axis=0)).astype(np.float32)


def realistic_operands(m, k, n, seed):
    """x ~ N(0, 1), w ~ N(0, 1 / sqrt(k)), b ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    return x, w, rng.standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def linear_case(recipe: str, k: int, n: int):
    gen = {"wide": wide_operands, "realistic": realistic_operands}[recipe]
    return gen(linear_rows(k, n), k, n, seed=1000 * RECIPES.index(recipe) + k + n)


@functools.lru_cache(maxsize=None)
def linear_ref(recipe: str, k: int, n: int, relu: int) -> np.ndarray:
    x, w, b = linear_case(recipe, k, n)
    y = linear(x, w, b, relu)
    y.setflags(write=False)
    return y


NONFINITE_LINEAR = {"k": 48, "n": 96, "m": 40, "row_mixed": 3, "row_inf": 7, "k_inf": 2, "col_zero_weight": 5, "col_nan_weight": 11}


@functools.lru_cache(maxsize=None)
def linear_nonfinite_case():
    """Realistic operands with: input row 3 holding +Inf, -Inf and NaN; input row 7 holding one +Inf at k = 2, where weight row 5
    is zero (Inf x 0 in the chain); weight row 11 holding a NaN."""
    c = NONFINITE_LINEAR
    x, w, b = realistic_operands(c["m"], c["k"], c["n"], seed=5)
    x[c["row_mixed"], [1, 5, 9]] = [np.inf, -np.inf, np.nan]
    x[c["row_inf"], c["k_inf"]] = np.inf
    w[c["col_zero_weight"], c["k_inf"]] = 0.0
    w[c["col_nan_weight"], 4] = np.nan
    return x, w, b


# ---- c4_conv_tower_f32
TOWER_CP = [16, 32, 48, 64]
TOWER_BLOCKS = [0, 1, 2]
TOWER_BOARDS = [1, 2, 3, 31, 32, 33, 61, 64, 65, 97]   # 32 boards = 21 tiles of 64 cells exactly; 61 / 64 / 65 move the board / tile phase


def tower_boards(cp: int, n_blocks: int) -> int:
    """The most boards a shape is run with (two blocks at 64 channels: 65, the oracle's cost)."""
    return 65 if (cp == 64 and n_blocks == 2) else 97


@functools.lru_cache(maxsize=None)
def tower_case(cp: int, binary: bool = False):
    """Planes [97, 2, 6, 7] (random f32, or 0 / 1 positions), w0 [Cp][32] (zero from k = 18 on), w [4][Cp][9 Cp], bias [5][Cp]: the
    scale of a default initialisation, U(-1, 1) / sqrt(K) (K = 18, 9 Cp) and biases U(-0.1, 0.1)."""
    rng = np.random.default_rng(100 + cp + int(binary))
    g = max(TOWER_BOARDS)
    if binary:
        occ, mine = rng.random((g, 42)) < 0.5, rng.random((g, 42)) < 0.5
        planes = np.stack([occ & mine, occ & ~mine], axis=1).astype(np.float32).reshape(g, 2, 6, 7)
    else:
        planes = rng.standard_normal((g, 2, 6, 7)).astype(np.float32)
    w0 = np.zeros((cp, 32), np.float32)
    w0[:, :18] = rng.uniform(-1, 1, (cp, 18)) / np.sqrt(18)
    w = (rng.uniform(-1, 1, (4, cp, 9 * cp)) / np.sqrt(9 * cp)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, (5, cp)).astype(np.float32)
    return planes, w0, w, bias


@functools.lru_cache(maxsize=None)
def tower_ref(cp: int, binary: bool = False) -> list:
    """tower_case's features after 0, 1 and 2 blocks, each at tower_boards(cp, n_blocks) boards."""
    planes, w0, w, bias = tower_case(cp, binary)
    stages = tower_stages(planes, w0, w, bias, 1)
    stages.append(_third_stage(stages[1][:tower_boards(cp, 2)], w, bias))
    for s in stages:
        s.setflags(write=False)
    return stages


def _third_stage(x, w, bias):
    x, t, cp = np.ascontiguousarray(x).copy(), np.empty_like(x), w.shape[1]
    L = ref_lib()
    L.f32ref_conv(_p(x), x.shape[0], cp, _p(np.ascontiguousarray(w[2])), _p(np.ascontiguousarray(bias[3])), _p(t), None)
    L.f32ref_conv(_p(t), x.shape[0], cp, _p(np.ascontiguousarray(w[3])), _p(np.ascontiguousarray(bias[4])), _p(x), _p(x))
    return x


NONFINITE_TOWER = {"cp": 32, "n_blocks": 1, "boards": 5, "board": 2, "plane": 1, "row": 0, "col": 0, "radius": 3}


@functools.lru_cache(maxsize=None)
def tower_nonfinite_case():
    """Five boards of tower_case(32), one block; board 2 has +Inf at plane 1, cell (0, 0).  Three convolutions: the cells up to
    three rows and columns away can be reached, no other."""
    c = NONFINITE_TOWER
    planes, w0, w, bias = tower_case(c["cp"])
    planes = planes[:c["boards"]].copy()
    planes[c["board"], c["plane"], c["row"], c["col"]] = np.inf
    return planes, w0, w, bias


# ---- c4_head_out_f32
HEAD_SHAPES = [(16, 16), (16, 144), (144, 16), (128, 128), (672, 128), (128, 672), (1344, 1344), (2688, 1344)]      # (kp, kv)
HEAD_N = [1, 15, 16, 17, 33, 1001]
# pre-activations (7 logits, 2 values) of the edge rows: logits hundreds apart (every expf but the maximum's underflows: lse == mx,
# the maximum's log-probability is 0.0), seven equal logits, a three-way tie for the maximum, value pre-activations past +-20
# (tanhf saturates), all zero
HEAD_EDGE = np.array([[896, 0, 192, 320, 448, 576, 768, 1024, -1024],
                      [64, 64, 64, 64, 64, 64, 64, 128, -128],
                      [128, 512, 512, 64, 512, -192, 0, 64, -64],
                      [-896, 0, -128, -256, -512, -768, -1024, 21, -25],
                      [0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
HEAD_ROW_NAN, HEAD_ROW_INF = 5, 6       # hidden rows with a NaN / a +Inf element (present from n = 15 on)
HEAD_FIRST_RANDOM = 7
# biases through which single logits / value pre-activations become non-finite (a non-finite hidden element reaches every output of
# its row: NaN x 0 and Inf x 0 are NaN): index -> value for the 7 policy + 2 value biases
HEAD_BIAS_VARIANTS = {"nan_logit": {2: np.nan, 7: np.inf, 8: -np.inf},
                      "inf_logit": {2: np.inf, 7: np.nan},
                      "minus_inf_logits": {1: -np.inf, 4: -np.inf, 7: -np.inf, 8: np.inf},
                      "all_minus_inf": {o: -np.inf for o in range(7)}}


@functools.lru_cache(maxsize=None)
def head_case(kp: int, kv: int):
    """1 001 hidden rows per head (N(0, 1)), output weights N(0, 1 / sqrt(k)) whose first columns are an identity block (policy
    output o <- feature o, value output i <- feature i), integer biases in [-3, 3].  Rows 0..4 are the edge rows: zero but for
    the identity block's features, which hold HEAD_EDGE - bias (small integers: every sum is exact, the pre-activations ARE
    HEAD_EDGE).  Row 5 has a NaN in each head's hidden row, row 6 a +Inf at the value head's feature 0 (weight 1 for q[0], weight
    0 for q[1]) and at the policy head's feature 9 (random weights)."""
    rng = np.random.default_rng(kp * 3 + kv)
    n = max(HEAD_N)
    hp, hv = rng.standard_normal((n, kp)).astype(np.float32), rng.standard_normal((n, kv)).astype(np.float32)
    wp, wv = (rng.standard_normal((7, kp)) / np.sqrt(kp)).astype(np.float32), (rng.standard_normal((2, kv)) / np.sqrt(kv)).astype(np.float32)
    wp[:, :7], wv[:, :2] = np.eye(7, dtype=np.float32), np.eye(2, dtype=np.float32)
    bp, bv = rng.integers(-3, 4, 7).astype(np.float32), rng.integers(-3, 4, 2).astype(np.float32)
    e = len(HEAD_EDGE)
    hp[:e], hv[:e] = 0, 0
    hp[:e, :7], hv[:e, :2] = HEAD_EDGE[:, :7] - bp, HEAD_EDGE[:, 7:] - bv
    hp[HEAD_ROW_NAN, 3], hv[HEAD_ROW_NAN, 1] = np.nan, np.nan
    hp[HEAD_ROW_INF, 9], hv[HEAD_ROW_INF, 0] = np.inf, np.inf
    return hp, hv, wp, wv, bp, bv


def head_preact(hp, hv, wp, wv, bp, bv) -> np.ndarray:
    """The pre-activations [n, 9] of the output layers: f32ref_linear with 7 and with 2 columns."""
    return np.concatenate([linear(hp, wp, bp, 0), linear(hv, wv, bv, 0)], axis=1)


@functools.lru_cache(maxsize=None)
def head_ref(kp: int, kv: int, variant: str = None) -> np.ndarray:
    hp, hv, wp, wv, bp, bv = head_case(kp, kv)
    b9 = head_biases(bp, bv, variant)
    pre = head_preact(hp, hv, wp, wv, b9[:7], b9[7:])
    pre.setflags(write=False)
    return pre


def head_biases(bp, bv, variant: str = None) -> np.ndarray:
    b9 = np.concatenate([bp, bv]).astype(np.float32)
    for i, v in (HEAD_BIAS_VARIANTS[variant] if variant else {}).items():
        b9[i] = v
    return b9


def host_libm():
    """(expf, logf) of the oracle's glibc ports, arrays in and out: what the kernels' c4_expf / c4_logf compute."""
    from oracle import c4oracle as O

    def host(fn):
        def f(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            out = np.empty_like(a)
            fn(a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), a.size)
            return out
        return f

    return host(O.lib().c4o_host_expf), host(O.lib().c4o_host_logf)
