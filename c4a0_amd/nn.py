"""ConnectFourNet inference for the self-play evaluator (reference src/c4a0/nn.py).

Only the forward pass is in scope: the reference evaluates leaves through
`ConnectFourNet.forward_numpy` (nn.py:119-130), a host round trip per batch.  Here the same
network runs as PyTorch-ROCm on the device that holds the trees, on the tensors the HIP step
kernel reads and writes.

* `ConnectFourNet` has the reference's module tree, so `state_dict()` keys are identical
  (`conv.0.*`, `conv.{i}.block.{0,1,2}.*`, `fc_policy.*`, `fc_value.*`; nn.py:64-100,184-195)
  and a reference checkpoint loads unchanged.
* `InferenceNet` is the evaluator: BatchNorm folded into the preceding conv/linear (eval-mode
  statistics), weights in bf16 (or f32), log-softmax/tanh in f32, outputs written into
  caller-provided tensors; optionally captured in a HIP graph.
"""
from __future__ import annotations

import ctypes
import threading
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import check, lib

N_COLS, N_ROWS = 7, 6


@dataclass
class ModelConfig:  # nn.py:16-38 (training-only fields omitted)
    n_residual_blocks: int = 1
    conv_filter_size: int = 32
    n_policy_layers: int = 4
    n_value_layers: int = 2


class ResidualBlock(nn.Module):  # nn.py:184-195: x + ReLU(BN(Conv(Conv(x))))
    def __init__(self, n_channels: int):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(n_channels, n_channels, kernel_size=3, padding=1),
            nn.Conv2d(n_channels, n_channels, kernel_size=3, padding=1),
            nn.BatchNorm2d(n_channels),
            nn.ReLU(),
        )

    def forward(self, x):
        return x + self.block(x)


class ConnectFourNet(nn.Module):
    def __init__(self, config: ModelConfig):
        super().__init__()
        self.config = config
        c = config.conv_filter_size
        self.conv = nn.Sequential(  # nn.py:64-70: first conv has no BN / ReLU
            nn.Conv2d(2, c, kernel_size=3, padding=1),
            *[ResidualBlock(c) for _ in range(config.n_residual_blocks)],
        )
        fc = c * N_ROWS * N_COLS  # nn.py:72,132-138
        self.fc_policy = nn.Sequential(  # nn.py:75-86
            *[nn.Sequential(nn.Linear(fc, fc), nn.BatchNorm1d(fc), nn.ReLU()) for _ in range(config.n_policy_layers - 1)],
            nn.Linear(fc, N_COLS),
            nn.LogSoftmax(dim=1),
        )
        self.fc_value = nn.Sequential(  # nn.py:89-100
            *[nn.Sequential(nn.Linear(fc, fc), nn.BatchNorm1d(fc), nn.ReLU()) for _ in range(config.n_value_layers - 1)],
            nn.Linear(fc, 2),
            nn.Tanh(),
        )

    def forward(self, x) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:  # nn.py:109-117
        x = self.conv(x)
        x = x.reshape(x.shape[0], -1)  # "b c h w -> b (c h w)"
        policy_logprobs = self.fc_policy(x)
        q = self.fc_value(x)
        return policy_logprobs, q[:, 0], q[:, 1]


def _fold_bn(weight: torch.Tensor, bias: torch.Tensor, bn: nn.modules.batchnorm._BatchNorm):
    """Eval-mode BN(y) = (y - mean) / sqrt(var + eps) * gamma + beta folded into y = W x + b."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shape = [-1] + [1] * (weight.dim() - 1)
    w = weight.detach().double() * scale.reshape(shape)
    b = (bias.detach().double() - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
    return w.float(), b.float()


def pack_tower_weights(conv_w, conv_b, channels: int):
    """Re-order the (BN-folded) conv weights into the MFMA A-fragment order the HIP tower kernel
    reads (c4a0_amd/csrc/c4_conv_tower.hip): for v_mfma_f32_16x16x32_bf16 lane l holds
    A[row = l & 15][k = 8 (l >> 4) + j], j = 0..7.

      conv_w[0]  [C, 2, 3, 3]  -> w0 [3 steps][C/16][64 lanes][8]: k-step s, k-group g <-> tap 4 s + g,
                                  element j <-> input channel j (only j < 2 non-zero)
      conv_w[1:] [C, C, 3, 3]  -> w  [layer][9 taps][C/16][C/32][64 lanes][8]:
                                  W[co = 16 m + (l & 15)][ci = 32 kc + 8 (l >> 4) + j][tap]
      conv_b     [C] each      -> bias [1 + 2 n_blocks][C] float32
    """
    c = channels
    mt, kc = c // 16, c // 32
    w0 = conv_w[0].float().reshape(c, 2, 9)                       # [co, ci, tap]
    p0 = torch.zeros(3, mt, 4, 16, 8)                             # [s, m, g, co_l, j]
    for s in range(3):
        for g in range(4):
            tap = 4 * s + g
            if tap < 9:
                p0[s, :, g, :, 0:2] = w0[:, :, tap].reshape(mt, 16, 2)
    p0 = p0.reshape(3, mt, 64, 8)
    layers = []
    for w in conv_w[1:]:
        wt = w.float().reshape(c, c, 9).permute(2, 0, 1)          # [tap, co, ci]
        wt = wt.reshape(9, mt, 16, kc, 4, 8).permute(0, 1, 3, 4, 2, 5)  # [tap, m, kc, g, co_l, j]
        layers.append(wt.reshape(9, mt, kc, 64, 8))
    pw = torch.stack(layers) if layers else torch.zeros(0, 9, mt, kc, 64, 8)
    bias = torch.stack([b.float() for b in conv_b])
    return p0.contiguous(), pw.contiguous(), bias.contiguous()


def pack_f32_weights(conv_w, conv_b, pol_w, pol_b, val_w, val_b, channels: int) -> dict:
    """The (BN-folded) f32 network in the layouts of the f32 kernels (c4a0_amd/csrc/c4_f32_net.hip; the order of every sum is
    include/c4a0_hip.h's "f32 evaluator").  C channels are padded to Cp = 16 ceil(C / 16), the heads' hidden width F = 42 C to
    Hp = 32 ceil(F / 32); padded weights and biases are zero, so padded channels and features stay zero.

      conv_w[0] [C, 2, 3, 3]  -> w0   [Cp][32]:    w0[co][2 tap + ci], tap = 3 kh + kw (zero from 18 on)
      conv_w[1:] [C, C, 3, 3] -> w    [2 n_blocks][Cp][9 Cp]: w[co][tap Cp + ci]
      conv_b                  -> bias [1 + 2 n_blocks][Cp]
      heads: the first layer's input "c h w" (nn.py:111) becomes the tower's cell-major [42][Cp]; hidden layers [Hp][K],
             output layers [7 | 2][K], K = 42 Cp for the first layer and Hp after it."""
    c = channels
    cp, f = -(-c // 16) * 16, 42 * c
    hp = -(-f // 32) * 32
    w0 = torch.zeros(cp, 32)
    w0[:c, :18] = conv_w[0].float().reshape(c, 2, 9).permute(0, 2, 1).reshape(c, 18)
    layers = [F.pad(w.float().reshape(c, c, 9).permute(0, 2, 1), (0, cp - c, 0, 0, 0, cp - c)).reshape(cp, 9 * cp) for w in conv_w[1:]]
    w = torch.stack(layers) if layers else torch.zeros(0, cp, 9 * cp)
    bias = torch.stack([F.pad(b.float(), (0, cp - c)) for b in conv_b])

    def head(ws, bs):
        out_w, out_b = [], []
        for i, (wt, b) in enumerate(zip(ws, bs)):
            n = wt.shape[0] if i == len(ws) - 1 else hp
            if i == 0:
                wt = F.pad(wt.float().reshape(-1, c, 42).permute(0, 2, 1), (0, cp - c)).reshape(-1, 42 * cp)
            else:
                wt = F.pad(wt.float(), (0, hp - f))
            out_w.append(F.pad(wt, (0, 0, 0, n - wt.shape[0])).contiguous())
            out_b.append(F.pad(b.float(), (0, n - b.shape[0])).contiguous())
        return out_w, out_b

    pw, pb = head(pol_w, pol_b)
    vw, vb = head(val_w, val_b)
    return {"cp": cp, "hp": hp, "w0": w0.contiguous(), "w": w.contiguous(), "bias": bias.contiguous(),
            "pol_w": pw, "pol_b": pb, "val_w": vw, "val_b": vb}


def fold_network(model: ConnectFourNet):
    """The network as BN-folded f32 host weights (eval-mode statistics), reference layout (the heads' first layers read
    "c h w", nn.py:111): (conv_w, conv_b, pol_w, pol_b, val_w, val_b), each a list -- the first conv and every block's two;
    one entry per Linear of a head, the output layer last."""
    conv0 = model.conv[0]
    conv_w, conv_b = [conv0.weight.detach().float()], [conv0.bias.detach().float()]
    for blk in list(model.conv)[1:]:
        c1, c2, bn = blk.block[0], blk.block[1], blk.block[2]
        w, b = _fold_bn(c2.weight, c2.bias, bn)
        conv_w += [c1.weight.detach().float(), w]
        conv_b += [c1.bias.detach().float(), b]

    def head(seq):
        mods = list(seq)
        folded = [_fold_bn(m[0].weight, m[0].bias, m[1]) for m in mods[:-2]]
        folded.append((mods[-2].weight.detach().float(), mods[-2].bias.detach().float()))
        return [w for w, _ in folded], [b for _, b in folded]

    return (conv_w, conv_b, *head(model.fc_policy), *head(model.fc_value))


def _stream(device: torch.device) -> int:
    """The current stream of `device`, as the handle the library's entry points take."""
    return torch.cuda.current_stream(device).cuda_stream


class _TorchChain:
    """A kernel chain: InferenceNet constructs exactly one, from fold_network()'s weights, and calls it for everything that
    touches a kernel -- tower(), linear_relu() (one hidden layer), head_out() (both output layers) and, on the HIP chains,
    np_planes() (the head of forward_numpy's graph: it leaves the planes to evaluate).  It owns its operands on the device:
    conv_w ... val_b, pol_b32 / val_b32, _bias32, and tw0 / tw / tbias / cp / hp where it has them.

    This one is PyTorch's kernels in `dtype` (F.conv2d, the library GEMM, F.linear + log_softmax / tanh; reference layout; a
    position's low bits depend on the batch) and the base of the two HIP chains, which replace all three operations."""
    np_planes = None        # no graph: forward_numpy is a plain forward and a copy back
    np_converts = False     # np_planes() is c4_planes_from_f32: from the f32 batch the pinned slot (c4_f32_batch) points at, on the
                            # device or in pinned host memory, to the state's bf16 planes

    def __init__(self, folded, device: torch.device, dtype: torch.dtype):
        conv_w, conv_b, pol_w, pol_b, val_w, val_b = folded
        self.device, self.dtype = device, dtype
        mv = lambda ts: [t.to(device, dtype).contiguous() for t in ts]
        self.conv_w = [w.to(device, dtype).contiguous(memory_format=torch.channels_last) for w in conv_w]
        self.conv_b, self.pol_w, self.pol_b, self.val_w, self.val_b = mv(conv_b), mv(pol_w), mv(pol_b), mv(val_w), mv(val_b)
        self.pol_b32 = pol_b[-1].to(device, torch.float32).contiguous()
        self.val_b32 = val_b[-1].to(device, torch.float32).contiguous()
        self.fused_epilogue = device.type == "cuda" and hasattr(torch, "_addmm_activation")   # bias and ReLU in the GEMM's epilogue
        self._bias32 = {}   # f32 copies of the hidden layers' biases for c4_linear_bf16's epilogue, by bias tensor

    def hidden_bias_added(self, b: torch.Tensor):
        """linear_relu() will be handed `b` (the merged first layer's bias) like the biases this chain made itself."""

    def tower(self, planes, config=0):
        x = planes.to(self.dtype)
        x = F.conv2d(x, self.conv_w[0], self.conv_b[0], padding=1)
        for i in range(1, len(self.conv_w), 2):
            y = F.conv2d(x, self.conv_w[i], self.conv_b[i], padding=1)
            y = F.conv2d(y, self.conv_w[i + 1], self.conv_b[i + 1], padding=1)
            x = x + F.relu(y)
        return x.reshape(x.shape[0], -1)

    def linear_relu(self, x, w, b, out=None, config=0):
        if self.fused_epilogue:
            return torch._addmm_activation(b, x, w.t(), use_gelu=False)
        return F.relu(F.linear(x, w, b))

    def head_out(self, p, v, out_logprobs=None, out_q=None):
        p = F.linear(p, self.pol_w[-1], self.pol_b[-1]).float()
        v = F.linear(v, self.val_w[-1], self.val_b[-1]).float()
        return torch.log_softmax(p, dim=1, out=out_logprobs), torch.tanh(v, out=out_q)


class _Bf16Chain(_TorchChain):
    """The product: c4_conv_tower_bf16, c4_linear_bf16, c4_head_out_bf16 (32 or 64 channels).  The base's bf16 operands with the
    heads' first layers permuted to the tower's cell-major features; hip_gemm=False (gemm="hipblaslt", the A/B switch) keeps
    the base's library GEMM for the hidden layers."""
    np_converts = True

    def __init__(self, folded, device: torch.device, hip_gemm: bool):
        conv_w, conv_b, pol_w, pol_b, val_w, val_b = folded
        c = self.channels = conv_w[0].shape[0]
        # the tower emits [cell][channel]; the reference flattens "c h w" (nn.py:111): permute
        # the input dimension of each head's first Linear once instead of the activations
        perm = lambda wt: wt.reshape(wt.shape[0], c, 42).permute(0, 2, 1).reshape(wt.shape[0], 42 * c)
        super().__init__((conv_w, conv_b, [perm(pol_w[0])] + pol_w[1:], pol_b, [perm(val_w[0])] + val_w[1:], val_b), device, torch.bfloat16)
        self.L: ctypes.CDLL = lib()
        self.n_blocks, self.hip_gemm = len(conv_w) // 2, hip_gemm
        w0, w, bias = pack_tower_weights(conv_w, conv_b, c)
        self.tw0, self.tw = w0.to(device, torch.bfloat16).contiguous(), w.to(device, torch.bfloat16).contiguous()
        self.tbias = bias.to(device, torch.float32).contiguous()
        for b in self.pol_b[:-1] + self.val_b[:-1]:
            self.hidden_bias_added(b)

    def hidden_bias_added(self, b):
        if self.hip_gemm:
            self._bias32[b.data_ptr()] = b.float().contiguous()

    def np_planes(self, st: dict, bucket: int):
        check(self.L.c4_planes_from_f32(st["slot"].data_ptr(), None, 0, st["planes"].data_ptr(), bucket, _stream(self.device)))
        return st["planes"][:bucket]

    def tower(self, planes, config=0):
        x = planes.to(torch.bfloat16).contiguous()
        g = x.shape[0]
        out = torch.empty((g, 42 * self.channels), dtype=torch.bfloat16, device=self.device)
        check(self.L.c4_conv_tower_bf16(x.data_ptr(), self.tw0.data_ptr(), self.tw.data_ptr(), self.tbias.data_ptr(),
                                        g, self.channels, self.n_blocks, out.data_ptr(), config, _stream(self.device)))
        return out

    def linear_relu(self, x, w, b, out=None, config=0):
        if not self.hip_gemm:
            return super().linear_relu(x, w, b)
        assert x.stride(1) == 1 and w.is_contiguous()
        m, (n, k) = x.shape[0], w.shape
        y = out if out is not None else torch.empty((m, n), dtype=torch.bfloat16, device=self.device)
        check(self.L.c4_linear_bf16(x.data_ptr(), w.data_ptr(), self._bias32[b.data_ptr()].data_ptr(), y.data_ptr(),
                                    m, n, k, x.stride(0), y.stride(0), 1, config, _stream(self.device)))
        return y

    def head_out(self, p, v, out_logprobs=None, out_q=None):
        # both output layers + log-softmax + tanh in one HIP launch, written in place
        g = p.shape[0]
        lp = out_logprobs if out_logprobs is not None else torch.empty((g, 7), dtype=torch.float32, device=self.device)
        q = out_q if out_q is not None else torch.empty((g, 2), dtype=torch.float32, device=self.device)
        assert p.stride(1) == 1 and v.stride(1) == 1
        check(self.L.c4_head_out_bf16(p.data_ptr(), v.data_ptr(), self.pol_w[-1].data_ptr(), self.val_w[-1].data_ptr(),
                                      self.pol_b32.data_ptr(), self.val_b32.data_ptr(), g, p.shape[1], p.stride(0), v.stride(0),
                                      lp.data_ptr(), q.data_ptr(), _stream(self.device)))
        return lp, q


# ---------------------------------------------------------------------------------------------- fp8 hidden layers (opt-in)
# include/c4a0_hip.h, "fp8 hidden layers": the numerics contract.  The helpers below need no GPU.
FP8_MAX = 448.0


def to_fp8_e4m3(t_f32: torch.Tensor) -> torch.Tensor:
    """The contract's q8: f32 -> OCP e4m3fn codes (uint8).  NaN -> 0x7F; otherwise clamp to [-448, 448], then round to nearest, ties
    to even; subnormals and the sign of zero are kept."""
    t = t_f32.to(torch.float32)
    nan = torch.isnan(t)
    c = torch.clamp(torch.where(nan, torch.zeros_like(t), t), -FP8_MAX, FP8_MAX)
    q = c.to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(nan, torch.full_like(q, 0x7F), q)


def _pow2_exponent_below(a: torch.Tensor, limit_m: float, limit_e: int) -> torch.Tensor:
    """Per element of the positive finite float64 a: the largest integer e with a 2^e <= limit_m 2^limit_e (0.5 <= limit_m < 1)."""
    m, ex = torch.frexp(a)                                        # a = m 2^ex, 0.5 <= m < 1
    return torch.where(m <= limit_m, limit_e - ex, limit_e - 1 - ex).to(torch.int64)


def quantize_head_weights(w_f32: torch.Tensor):
    """(Wq uint8 [N, K], e_w int32 [N]) of the BN-folded f32 weights W [N, K]: per output row n, e_w[n] is the largest integer in
    [-64, 64] with max_k |W[n][k]| 2^e_w[n] <= 448 (an all-zero row: 0) and Wq[n][k] = q8(W[n][k] 2^e_w[n]).  Powers of two: the
    scaling is exact, only range is adapted."""
    w = w_f32.detach().to("cpu", torch.float64)
    amax = w.abs().amax(dim=1)
    ok = (amax > 0) & torch.isfinite(amax)
    e = _pow2_exponent_below(torch.where(ok, amax, torch.ones_like(amax)), 0.875, 9)       # 448 = 0.875 x 2^9
    e = torch.where(ok, torch.clamp(e, -64, 64), torch.zeros_like(e))
    wq = to_fp8_e4m3(torch.ldexp(w, e[:, None]).float())
    return wq.contiguous(), e.to(torch.int32)


def activation_exponent(a: float) -> int:
    """The e_x of a GEMM input tensor whose calibration rows reach max |x| = a: the largest integer (kept in [-64, 64]) with
    2 a 2^e_x <= 448, a factor 2 of headroom; 0 for a = 0 (or a non-finite a)."""
    a = float(a)
    if not (a > 0.0) or a == float("inf"):
        return 0
    e = int(_pow2_exponent_below(torch.tensor([2.0 * a], dtype=torch.float64), 0.875, 9)[0])
    return max(-64, min(64, e))


def _c4_won(stones) -> bool:
    """Four in a row among the cells `stones` ([6][7] booleans)."""
    for r in range(N_ROWS):
        for c in range(N_COLS):
            if not stones[r][c]:
                continue
            for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                if all(0 <= r + i * dr < N_ROWS and 0 <= c + i * dc < N_COLS and stones[r + i * dr][c + i * dc] for i in range(1, 4)):
                    return True
    return False


def calibration_positions(n: int = 4096, seed: int = 0) -> np.ndarray:
    """uint64[n, 2] (mask, value) positions for choosing the fp8 activation scales: every position of seeded random legal playouts
    from the empty board to the end of the game (the empty board included), so all plies are covered.  Pure numpy, deterministic:
    the scales are a function of (weights, calibration rows) only.  Bit 7 r + c is cell (row r from the bottom, column c); `value`
    holds the stones of the player to move (c4r.rs:13-17)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n, 2), dtype=np.uint64)
    k = 0
    while k < n:
        mine = [[False] * N_COLS for _ in range(N_ROWS)]          # the stones of the player to move
        theirs = [[False] * N_COLS for _ in range(N_ROWS)]
        heights = [0] * N_COLS
        while k < n:
            mask = sum(1 << (7 * r + c) for r in range(N_ROWS) for c in range(N_COLS) if mine[r][c] or theirs[r][c])
            value = sum(1 << (7 * r + c) for r in range(N_ROWS) for c in range(N_COLS) if mine[r][c])
            out[k] = (mask, value)
            k += 1
            legal = [c for c in range(N_COLS) if heights[c] < N_ROWS]
            if not legal or _c4_won(theirs):                      # (only the player who just moved can have won)
                break
            c = legal[int(rng.integers(len(legal)))]
            mine[heights[c]][c] = True
            heights[c] += 1
            mine, theirs = theirs, mine
    return out


def positions_to_planes(pos: np.ndarray) -> np.ndarray:
    """uint64[P, 2] (mask, value) -> float32 [P, 2, 6, 7] planes (c4r.rs:378-392: the mover's stones, the opponent's)."""
    pos = np.asarray(pos, dtype=np.uint64).reshape(-1, 2)
    bit = np.arange(42, dtype=np.uint64)[None, :]
    mine = ((pos[:, 1:2] >> bit) & np.uint64(1)).astype(np.float32)
    opp = (((pos[:, 0:1] ^ pos[:, 1:2]) >> bit) & np.uint64(1)).astype(np.float32)
    return np.stack([mine, opp], axis=1).reshape(len(pos), 2, N_ROWS, N_COLS)


class _Fp8HeadChain(_Bf16Chain):
    """_Bf16Chain with the heads' hidden layers in OCP e4m3 (c4_quantize_bf16_fp8, c4_linear_fp8; the contract is
    include/c4a0_hip.h's "fp8 hidden layers").  The tower, the output layers (the bf16 pol_w[-1] / val_w[-1]) and everything the
    session does with them are the base's.  Per hidden layer it keeps Wq, dq, the f32 bias as folded and the exponents, found by the
    bf16 weight tensor InferenceNet hands to linear_relu(); the first layer of both heads is one merged launch when both heads go on
    in fp8 (or both end there), else one launch per head, because a head's LAST hidden layer writes bf16."""

    def __init__(self, folded, device: torch.device):
        super().__init__(folded, device, hip_gemm=True)
        conv_w, _, pol_w, pol_b, val_w, val_b = folded
        c = self.channels
        perm = lambda wt: wt.reshape(wt.shape[0], c, 42).permute(0, 2, 1).reshape(wt.shape[0], 42 * c)
        # the BN-folded f32 hidden layers, first layers cell-major like the base's: what is quantised (never the bf16 copies)
        self._f32_hidden = {"policy": ([perm(pol_w[0].float())] + [w.float() for w in pol_w[1:-1]], [b.float() for b in pol_b[:-1]]),
                            "value": ([perm(val_w[0].float())] + [w.float() for w in val_w[1:-1]], [b.float() for b in val_b[:-1]])}
        self.layers = {}        # data_ptr of the bf16 weight tensor linear_relu() is handed -> the layer's fp8 operands
        self.first = None       # the first layer's launches: [(layer, column range of the merged output or None)]
        self.fp8_scales = {}    # name of a GEMM input tensor -> its exponent e_x

    def _layer(self, name, w, b, e_in, out_fp8):
        wq, e_w = quantize_head_weights(w)
        dq = torch.ldexp(torch.ones(len(e_w), dtype=torch.float64), (-e_in - e_w.to(torch.int64))).float()
        return {"name": name, "Wq": wq.to(self.device), "e_w": e_w, "dq": dq.to(self.device).contiguous(), "bias": b.float().to(self.device).contiguous(),
                "e_in": int(e_in), "out_fp8": bool(out_fp8), "e_out": None, "n": int(w.shape[0]), "k": int(w.shape[1])}

    def quantize(self, x, e_x: int):
        """bf16 [m][k] row view -> e4m3 codes (uint8 [m][k]) of x 2^e_x."""
        assert x.dtype == torch.bfloat16 and x.stride(1) == 1
        m, k = x.shape
        y = torch.empty((m, k), dtype=torch.uint8, device=self.device)
        check(self.L.c4_quantize_bf16_fp8(x.data_ptr(), y.data_ptr(), m, k, x.stride(0), y.stride(0), float(2.0 ** e_x), _stream(self.device)))
        return y

    def run_layer(self, ly, x8, out_fp8=None, e_out=None):
        """One c4_linear_fp8 launch of layer `ly` on the e4m3 rows x8 (out_fp8 / e_out: the calibration's overrides)."""
        assert x8.dtype == torch.uint8 and x8.stride(1) == 1 and x8.shape[1] == ly["k"]
        out_fp8 = ly["out_fp8"] if out_fp8 is None else out_fp8
        e_out = ly["e_out"] if e_out is None else e_out
        m = x8.shape[0]
        y = torch.empty((m, ly["n"]), dtype=torch.uint8 if out_fp8 else torch.bfloat16, device=self.device)
        check(self.L.c4_linear_fp8(x8.data_ptr(), ly["Wq"].data_ptr(), ly["dq"].data_ptr(), ly["bias"].data_ptr(), y.data_ptr(), m, ly["n"], ly["k"],
                                   x8.stride(0), y.stride(0), 1, 1 if out_fp8 else 0, float(2.0 ** e_out) if out_fp8 else 1.0, 0, _stream(self.device)))
        return y

    @torch.no_grad()
    def calibrate(self, net, planes):
        """Choose every exponent from the calibration rows and build the layers: the input of layer i comes from the fp8 layers in
        front of it; layer i runs once with bf16 output to observe a_i = max |r|, which sets the e_x of the tensor it writes."""
        (pw, pb), (vw, vb) = self._f32_hidden["policy"], self._f32_hidden["value"]
        amax = lambda t: float(t.float().abs().max()) if t.numel() else 0.0
        feat = net.tower(planes.to(self.device, torch.bfloat16), latency=False)
        e0 = self.fp8_scales["first"] = activation_exponent(amax(feat))
        x8 = self.quantize(feat, e0)
        more_p, more_v = len(pw) > 1, len(vw) > 1
        f = pw[0].shape[0]
        if more_p == more_v:    # one merged launch: both halves fp8 (one output tensor, one exponent) or both bf16
            ly = self._layer("first", torch.cat([pw[0], vw[0]]), torch.cat([pb[0], vb[0]]), e0, more_p)
            self.first = [(ly, None)]
            if more_p:
                ly["e_out"] = self.fp8_scales["policy.1"] = self.fp8_scales["value.1"] = activation_exponent(amax(self.run_layer(ly, x8, out_fp8=False)))
                h = self.run_layer(ly, x8)
                p8, v8 = h[:, :f], h[:, f:]
        else:                   # a head that ends with its first layer takes bf16 from it: one launch per head
            lp, lv = self._layer("first.policy", pw[0], pb[0], e0, more_p), self._layer("first.value", vw[0], vb[0], e0, more_v)
            self.first = [(lp, (0, f)), (lv, (f, 2 * f))]
            for ly, more, key in ((lp, more_p, "policy.1"), (lv, more_v, "value.1")):
                if more:
                    ly["e_out"] = self.fp8_scales[key] = activation_exponent(amax(self.run_layer(ly, x8, out_fp8=False)))
            p8 = self.run_layer(lp, x8) if more_p else None
            v8 = self.run_layer(lv, x8) if more_v else None
        for head, ws, bs, bf16_ws, x8 in (("policy", pw, pb, self.pol_w, p8 if more_p else None), ("value", vw, vb, self.val_w, v8 if more_v else None)):
            for i in range(1, len(ws)):
                last = i == len(ws) - 1
                ly = self._layer(f"{head}.{i}", ws[i], bs[i], self.fp8_scales[f"{head}.{i}"], not last)
                self.layers[bf16_ws[i].data_ptr()] = ly
                if not last:
                    ly["e_out"] = self.fp8_scales[f"{head}.{i + 1}"] = activation_exponent(amax(self.run_layer(ly, x8, out_fp8=False)))
                    x8 = self.run_layer(ly, x8)
        torch.cuda.synchronize(self.device)

    def first_layer(self, feat):
        """The tower's bf16 features -> (policy head's, value head's) first hidden activations: e4m3 where the head goes on, bf16
        where this was its last hidden layer."""
        x8 = self.quantize(feat, self.fp8_scales["first"])
        if len(self.first) == 1:
            h = self.run_layer(self.first[0][0], x8)
            f = h.shape[1] // 2
            return h[:, :f], h[:, f:]
        return self.run_layer(self.first[0][0], x8), self.run_layer(self.first[1][0], x8)

    def linear_relu(self, x, w, b, out=None, config=0):
        """A further hidden layer (w: the bf16 weight tensor of the base, which names the layer; its tile configuration is not ours)."""
        return self.run_layer(self.layers[w.data_ptr()], x)


class _F32Chain(_TorchChain):
    """c4_conv_tower_f32, c4_linear_f32, c4_head_out_f32 (1 to 64 channels): every product an exact-f32 MFMA fmaf chain in the
    documented order (include/c4a0_hip.h), so a row's outputs depend on that row alone and equal tests/f32_net_ref.c bit for
    bit.  Operands in pack_f32_weights' padded layouts (cp channels, hp hidden features); no unpacked conv weights are kept."""

    def __init__(self, folded, device: torch.device):
        pk = pack_f32_weights(*folded, folded[0][0].shape[0])
        super().__init__(([], [], pk["pol_w"], pk["pol_b"], pk["val_w"], pk["val_b"]), device, torch.float32)
        self.L: ctypes.CDLL = lib()
        self.cp, self.hp, self.n_blocks = pk["cp"], pk["hp"], len(folded[0]) // 2
        self.tw0, self.tw, self.tbias = (pk[k].to(device, torch.float32).contiguous() for k in ("w0", "w", "bias"))

    def np_planes(self, st: dict, bucket: int):
        return st["in"][:bucket]   # the f32 positions as they are (rows from the batch's end to `bucket`: earlier batches, unread)

    def tower(self, planes, config=0):
        x = planes.float().contiguous()
        g = x.shape[0]
        out = torch.empty((g, 42 * self.cp), dtype=torch.float32, device=self.device)
        work = torch.empty_like(out) if self.n_blocks else None
        check(self.L.c4_conv_tower_f32(x.data_ptr(), self.tw0.data_ptr(), self.tw.data_ptr(), self.tbias.data_ptr(), g, self.cp, self.n_blocks,
                                       out.data_ptr(), work.data_ptr() if work is not None else None, _stream(self.device)))
        return out

    def linear_relu(self, x, w, b, out=None, config=0):
        assert x.stride(1) == 1 and w.is_contiguous()
        m, (n, k) = x.shape[0], w.shape
        y = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=self.device)
        check(self.L.c4_linear_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), m, n, k, x.stride(0), y.stride(0), 1, _stream(self.device)))
        return y

    def head_out(self, p, v, out_logprobs=None, out_q=None, out_preact=None):
        """Both output layers, log-softmax and tanh written in place (out_preact [G, 9]: the pre-activations too)."""
        g = p.shape[0]
        lp = out_logprobs if out_logprobs is not None else torch.empty((g, 7), dtype=torch.float32, device=self.device)
        q = out_q if out_q is not None else torch.empty((g, 2), dtype=torch.float32, device=self.device)
        assert p.stride(1) == 1 and v.stride(1) == 1
        check(self.L.c4_head_out_f32(p.data_ptr(), v.data_ptr(), self.pol_w[-1].data_ptr(), self.val_w[-1].data_ptr(),
                                     self.pol_b32.data_ptr(), self.val_b32.data_ptr(), g, self.pol_w[-1].shape[1], self.val_w[-1].shape[1], p.stride(0),
                                     v.stride(0), lp.data_ptr(), q.data_ptr(), out_preact.data_ptr() if out_preact is not None else None, _stream(self.device)))
        return lp, q


class EvaluatorFallbackWarning(UserWarning):
    """An InferenceNet on a HIP device that runs neither hand-written chain: not bf16 with 32 or 64 channels (the bf16 chain),
    and not f32 with hip_tower=True (the f32 chain, 1 to 64 channels), so PyTorch's kernels evaluate it."""


class InferenceNet:
    """Device-resident evaluator: planes[G,2,6,7] -> (policy_logprobs[G,7] f32, q[G,2] f32).

    BatchNorm is folded into the preceding conv / linear (fold_network) and ONE kernel chain is constructed, whose operands are
    readable here under its names (_CHAIN_OPERANDS).  `hip_tower=True` (default on a HIP device in bf16 with 32 or 64 channels) is
    _Bf16Chain; with dtype=torch.float32 it is _F32Chain instead (exact-f32 MFMA, any width 1..64, batch-invariant like the first);
    otherwise _TorchChain: PyTorch-ROCm convs + the library GEMM -- a path whose low bits depend on the batch (`batch_invariant`
    False), slower, and never the one the parity suite certifies.  Leaving the hand-written kernels is therefore LOUD:
    `strict=True` refuses (ValueError), the default warns once per construction (EvaluatorFallbackWarning) and `path` says
    which one runs ("hip" | "torch"; the bench line carries it).  `head_dtype=torch.float8_e4m3fn` (opt-in) is _Fp8HeadChain: the bf16
    chain with the heads' hidden layers in OCP FP8 at static, calibrated scales -- `dtype` stays bfloat16 (the planes are), `head_dtype`
    tells the two apart, and every flag of the bf16 chain (`path`, `batch_invariant`, `graph_safe`, `fused_step_ok`) stays true."""

    latency_mode = False  # True while ONE session plays alone on the device (api._play sets it): the narrow layers of a
                          # > 1 024-row batch then use the 128 x 96 tile (12.7 vs 16.8 us alone at 1 700 rows; beside a
                          # second session's kernels the fat 128 x 192 tile wins, c4_head_gemm.hip) and the 32-channel
                          # tower 8 boards per workgroup up to 2 048 boards (27.3 -> 19.1 us alone at 2 048)
    graph_safe = True  # forward() is pure device work on caller-owned outputs: may be captured in a HIP graph
    stage_hook = None  # optional callable(stage): 0 = before the tower is launched, 2 = after it, 1 = after the first hidden layer's
                       # GEMM is launched, 3 + i = after the policy head's i-th further layer (session.capture_pair records /
                       # waits cross-stream events there)
    _CHAIN_OPERANDS = frozenset(("tw0", "tw", "tbias", "conv_w", "conv_b", "pol_w", "pol_b", "val_w", "val_b", "pol_b32", "val_b32",
                                 "_bias32", "cp", "hp"))

    def __init__(self, model: ConnectFourNet, device: torch.device, dtype: torch.dtype = torch.bfloat16,
                 hip_tower: Optional[bool] = None, gemm: Optional[str] = None, gemm_config=None, tower_config: int = 0,
                 strict: bool = False, head_dtype: Optional[torch.dtype] = None, calibration: Optional[torch.Tensor] = None):
        """gemm: "hip" (the hand-written MFMA GEMM, default with the HIP tower) or "hipblaslt" (PyTorch's library GEMM, an
        A/B switch: its low bits depend on the batch shape).  gemm_config: c4_linear_bf16's tile configuration, one number or
        "wide,narrow" (the merged 2F-wide first layer, the F-wide layers); tower_config: c4_conv_tower_bf16's workgroup
        shape; 0 / None = automatic.  Measurement switches are constructor arguments: nothing is read from the environment.
        head_dtype: None (default: today's chain exactly) or torch.float8_e4m3fn -- the heads' hidden layers in OCP FP8 with f32
        accumulation (_Fp8HeadChain; include/c4a0_hip.h "fp8 hidden layers"), opt-in; its static activation scales are chosen here
        from `calibration`, a planes tensor [B, 2, 6, 7] (None: calibration_positions(4096, 0)), and readable as `fp8_scales`."""
        self.device, self.dtype = torch.device(device), dtype
        model = model.eval()
        self.channels = model.config.conv_filter_size
        self.n_blocks = len(model.conv) - 1
        self.head_dtype = head_dtype
        if head_dtype is not None:
            if head_dtype != torch.float8_e4m3fn:
                raise ValueError("head_dtype must be None or torch.float8_e4m3fn")
            why = ("a HIP device" if self.device.type != "cuda" else "dtype=torch.bfloat16" if dtype != torch.bfloat16 else
                   "the HIP tower (hip_tower=False was given)" if hip_tower is False else "gemm='hip'" if gemm not in (None, "hip") else
                   "32 or 64 channels" if self.channels not in (32, 64) else
                   "both heads with at least one hidden layer" if min(model.config.n_policy_layers, model.config.n_value_layers) < 2 else
                   "no bf16 tile configuration (gemm_config: c4_linear_fp8 chooses its own)" if gemm_config is not None else None)
            if why is not None:
                raise ValueError(f"fp8 hidden layers (head_dtype=torch.float8_e4m3fn) run on the bf16 HIP chain only: they need {why}")
        # f32 networks on the hand-written path only when asked for (hip_tower=True): the f32 chain has no bf16 switches
        f32 = dtype == torch.float32 and bool(hip_tower)
        if f32:
            if self.device.type != "cuda" or not 1 <= self.channels <= 64:
                raise ValueError("the f32 HIP evaluator needs a HIP device and 1 to 64 channels")
            if gemm not in (None, "hip") or gemm_config is not None or tower_config:
                raise ValueError("gemm / gemm_config / tower_config are bf16 switches: the f32 HIP evaluator has none")
        can_tower = self.device.type == "cuda" and ((dtype == torch.bfloat16 and self.channels in (32, 64)) or f32)
        if hip_tower and not can_tower:
            raise ValueError("hip_tower needs a HIP device, bf16 and 32 or 64 channels")
        self.hip_tower = can_tower if hip_tower is None else bool(hip_tower)
        if not self.hip_tower and hip_tower is None and self.device.type == "cuda":
            # nobody asked for PyTorch's kernels (hip_tower=False does: the A/B switch of the tests): say so
            why = (f"{self.channels} channels (the HIP tower and GEMM are written for 32 and 64)" if dtype == torch.bfloat16
                   else f"dtype {dtype} (the default HIP kernels compute in bf16; f32 networks: hip_tower=True)")
            msg = (f"InferenceNet: {why}: this evaluator runs on PyTorch's convolutions and the library GEMM, not on the "
                   "hand-written HIP kernels -- slower, and a position's low bits depend on the batch it is evaluated in")
            if strict:
                raise ValueError(msg + " (strict=True)")
            warnings.warn(msg, EvaluatorFallbackWarning, stacklevel=2)
        folded = fold_network(model)
        # Hidden layers of the heads: "hip" = the hand-written MFMA GEMM (c4_linear_bf16; c4_linear_f32 on the f32 chain), whose
        # result for a position does not depend on the batch or the row it sits in -- the default wherever the HIP
        # tower runs; "hipblaslt" = PyTorch's library GEMM (kept for A/B timing: its low bits depend on
        # the batch shape).
        gemm = gemm or ("hip" if self.hip_tower else "hipblaslt")
        if gemm not in ("hip", "hipblaslt"):
            raise ValueError("gemm must be 'hip' or 'hipblaslt'")
        if gemm == "hip" and not (self.hip_tower and (f32 or (42 * self.channels) % 192 == 0)):
            raise ValueError("gemm='hip' needs the HIP tower (bf16, 32 or 64 channels on a HIP device)")
        self.gemm = gemm
        if strict and gemm != "hip":
            raise ValueError("InferenceNet(strict=True): gemm='hipblaslt' leaves the hand-written GEMM (its low bits depend on the batch)")
        # every kernel of the evaluator computes a row from that row alone in one fixed order: a position's outputs do
        # not depend on the batch (session.narrow_if_worthwhile may then narrow whenever it likes)
        self.batch_invariant = self.hip_tower and gemm == "hip"
        # tile configuration: one number, or "wide,narrow" (the merged 2F-wide first layer, the F-wide layers); 0 = automatic
        cfg = str(gemm_config if gemm_config is not None else "0").split(",")
        self.gemm_config = (int(cfg[0]), int(cfg[-1]))
        self.tower_config = int(tower_config)   # c4_conv_tower_bf16's config, 0 = automatic
        self._np_lock = threading.Lock()   # forward_numpy keeps ONE pinned slot, stream and graph set per net
        ch = self.chain = (_F32Chain(folded, self.device) if f32 else _Fp8HeadChain(folded, self.device) if head_dtype is not None
                           else _Bf16Chain(folded, self.device, hip_gemm=gemm == "hip") if self.hip_tower else _TorchChain(folded, self.device, dtype))
        self.merged_w1 = self.merged_b1 = None   # the first hidden layer of BOTH heads as one 2F-wide layer (forward_hidden)
        if len(ch.pol_w) > 1 and len(ch.val_w) > 1:
            self.merged_w1 = torch.cat([ch.pol_w[0], ch.val_w[0]], dim=0).contiguous()
            self.merged_b1 = torch.cat([ch.pol_b[0], ch.val_b[0]], dim=0).contiguous()
            ch.hidden_bias_added(self.merged_b1)
        if head_dtype is not None:
            if calibration is None:
                calibration = torch.from_numpy(positions_to_planes(calibration_positions(4096, 0)))
            if calibration.dim() != 4 or tuple(calibration.shape[1:]) != (2, N_ROWS, N_COLS) or calibration.shape[0] == 0:
                raise ValueError("calibration must be a planes tensor [B, 2, 6, 7] with at least one row")
            ch.calibrate(self, calibration)

    @property
    def fp8_scales(self) -> Optional[dict]:
        """fp8 heads: the exponent e_x of every GEMM input tensor by name ("first", "policy.1", "value.1", ...: x8 = q8(x 2^e_x)),
        a function of (weights, calibration rows) only; None on every other chain."""
        return dict(self.chain.fp8_scales) if self.head_dtype is not None else None

    def __getattr__(self, name):
        if name in InferenceNet._CHAIN_OPERANDS and "chain" in self.__dict__:
            return getattr(self.chain, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    @property
    def path(self) -> str:
        """Which kernels run: "hip" = the hand-written tower, GEMM and output kernels; "torch" = any PyTorch / library kernel in the chain."""
        return "hip" if (self.hip_tower and self.gemm == "hip") else "torch"

    @torch.no_grad()
    def tower(self, planes: torch.Tensor, latency: Optional[bool] = None) -> torch.Tensor:
        """Conv tower -> flattened features [G, 42*C] (cell-major when hip_tower, else "c h w").  latency: this call's
        answer to `latency_mode` (None = the attribute)."""
        latency = self.latency_mode if latency is None else latency
        # c4_conv_tower_bf16's workgroup shape.  Alone on the device (latency_mode): 8 boards per workgroup from 1 025 to 2 048 boards
        # (up to 1 024 boards the automatic choice is already the narrow-launch shape: 2 or 4 boards per workgroup)
        config = self.tower_config or (2 if (latency and self.channels == 32 and 1024 < planes.shape[0] <= 2048) else 0)
        return self.chain.tower(planes, config)

    @torch.no_grad()
    def forward_hidden(self, planes: torch.Tensor, latency: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Everything but the heads' output layers: planes -> (policy head's last hidden activations, value head's), bf16
        [G, F] row views (column stride 1; f32 [G, Hp] on the f32 chain, Hp = F padded to a multiple of 32).  The output layers follow in `forward`, or inside the session's fused output +
        step launch (DeviceSession.round, c4_session_step_head_out)."""
        hook, ch = self.stage_hook, self.chain
        if hook is not None:
            hook(0)
        x = self.tower(planes, latency)
        if hook is not None:
            hook(2)                # after the tower is launched (capture_pair's offset_stage measurements)
        if self.merged_w1 is not None:
            # first hidden layer of BOTH heads as one GEMM (same input, N = 2F): better tile occupancy.  (Round 4 tried the two
            # halves as two launches, the value head's on a side stream beside the policy head's second layer, so that a
            # session's chain holds an F-wide layer instead of the 2F-wide one: same bits, but every cross-stream edge
            # costs more than the 3.5 us it saves -- the bench halved, 28.0 -> 13.7 k games/s -- and ROCm 7.2's
            # hipStreamEndCapture crashes on a fork from a non-origin stream, tools/capture_nested_fork_repro.py.)
            if self.head_dtype is not None:   # fp8 heads: quantise, then the first layer in e4m3 (bf16 where a head ends with it)
                p, v = ch.first_layer(x)
            else:
                h = self._linear_relu(x, self.merged_w1, self.merged_b1, latency=latency)
                f = self.merged_w1.shape[0] // 2
                p, v = h[:, :f], h[:, f:]
            rest = slice(1, -1)
        else:   # no merged first layer (a head without hidden layers): the heavy half ends with the tower
            p, v, rest = x, x, slice(0, -1)
        if hook is not None:
            hook(1)
        for i, (w, b) in enumerate(zip(ch.pol_w[rest], ch.pol_b[rest])):
            p = self._linear_relu(p, w, b, latency=latency)
            if hook is not None:
                hook(3 + i)      # after each narrow policy layer (capture_pair's offset_stage)
        for w, b in zip(ch.val_w[rest], ch.val_b[rest]):
            v = self._linear_relu(v, w, b, latency=latency)
        return p, v

    @property
    def fused_step_ok(self) -> bool:
        """The session may run this evaluator's output layers inside its step launch (c4_session_step_head_out), i.e. call
        forward_hidden() + head_out_operands() INSTEAD of forward().  Only while forward() is InferenceNet's own: a subclass
        that overrides `forward` / `__call__` (counting calls, post-processing logits, observers) must see every evaluation,
        so for it the session keeps evaluate() -> step() (the same answer as setting
        DeviceSession.fuse_output_step = False)."""
        own = type(self).forward is InferenceNet.forward and type(self).__call__ is InferenceNet.__call__
        return own and bool(self.hip_tower) and self.dtype == torch.bfloat16 and (42 * self.channels) % 1344 == 0

    def head_out_operands(self):
        """(w_policy, w_value, b_policy f32, b_value f32) of the output layers, as the HIP output kernels take them."""
        ch = self.chain
        return ch.pol_w[-1], ch.val_w[-1], ch.pol_b32, ch.val_b32

    @torch.no_grad()
    def forward(self, planes: torch.Tensor, out_logprobs: Optional[torch.Tensor] = None,
                out_q: Optional[torch.Tensor] = None, latency: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        p, v = self.forward_hidden(planes, latency)
        return self.chain.head_out(p, v, out_logprobs, out_q)

    def _head_out_f32(self, p, v, out_logprobs=None, out_q=None, out_preact=None):
        """The f32 chain's c4_head_out_f32 with its extra output (out_preact [G, 9]: the pre-activations too)."""
        return self.chain.head_out(p, v, out_logprobs, out_q, out_preact)

    # ---------------------------------------------------------------- the reference's numpy entry point
    _NP_BUCKET = 128

    @torch.no_grad()
    def forward_numpy(self, x):
        """`ConnectFourNet.forward_numpy` (reference src/c4a0/nn.py:119-130): float32 numpy positions [B, 2, 6, 7] ->
        (policy_logprobs float32 [B, 7], q_penalty float32 [B], q_no_penalty float32 [B]), fresh C-contiguous arrays --
        what the reference's callers hand to `play_games` as `lambda model_id, x: model.forward_numpy(x)`
        (training.py:179-189), so a caller that swaps its model for this class keeps its callback.

        The reference's version is a host round trip around ~35 eager launches.  Here, on the HIP chains, ONE HIP-graph replay and one stream
        synchronisation: the graph (captured once per batch size rounded up to a multiple of 128 rows: the kernels compute a
        row from that row alone, so padding rows change nothing) is c4_planes_from_f32 + tower + GEMMs + output kernel, and
        the output kernel writes into pinned host memory itself.  The f32 network (hip_tower=True) reads f32 positions as they
        are: the batch is copied into the graph's device input (no conversion kernel), then the same one replay.  On the bf16 chain a batch that already lives in pinned host memory -- what
        `play_games` hands its callback -- is read by the first kernel over PCIe where it is (its address travels in a
        pinned word, c4_f32_batch); any other array takes one copy into a device buffer first."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        b = int(x.shape[0])
        if b == 0:
            return np.zeros((0, 7), np.float32), np.zeros((0,), np.float32), np.zeros((0,), np.float32)
        if self.chain.np_planes is None:
            lp, q = self.forward(torch.from_numpy(x).to(self.device))
            lp, q = lp.float().cpu().numpy(), q.float().cpu().numpy()
            return np.ascontiguousarray(lp), np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
        if x.shape[1:] != (2, 6, 7):
            raise ValueError(f"forward_numpy: positions must be [B, 2, 6, 7], got {x.shape}")
        bucket = -(-b // self._NP_BUCKET) * self._NP_BUCKET
        # ONE pinned slot, stream and graph set per net: two threads calling forward_numpy on the same net (a tournament's
        # callbacks, the cpu_baseline's evaluator thread beside the main thread) take turns -- the reference's
        # forward_numpy is re-entrant, this one is serialised
        with self._np_lock:
            return self._forward_numpy_locked(x, b, bucket)

    def _forward_numpy_locked(self, x, b: int, bucket: int):
        ch = self.chain
        st = getattr(self, "_np", None)
        if st is None or st["cap"] < bucket:
            cap = max(2048, 1 << (bucket - 1).bit_length())
            st = self._np = {"cap": cap, "graphs": {}, "stream": torch.cuda.Stream(device=self.device),
                             "in": torch.zeros((cap, 2, 6, 7), dtype=torch.float32, device=self.device),
                             "slot": torch.zeros(2, dtype=torch.int64).pin_memory(),      # c4_f32_batch {data, n_boards}
                             "h_lp": torch.zeros((cap, 7), dtype=torch.float32).pin_memory(),
                             "h_q": torch.zeros((cap, 2), dtype=torch.float32).pin_memory(),
                             "planes": torch.zeros((cap, 2, 6, 7), dtype=torch.bfloat16, device=self.device) if ch.np_converts else None}
            st["slot_np"] = st["slot"].numpy()
        stream = st["stream"]
        with torch.cuda.stream(stream):
            g = st["graphs"].get(bucket)
            if g is None:
                from .session import CAPTURE_ERROR_MODE

                def body():
                    # the output kernel's stores go to pinned host memory: no copy after it.  latency=True: a host round
                    # trip, this forward has the chip to itself (an argument of the call, not a mutation of the shared net)
                    self.forward(ch.np_planes(st, bucket), out_logprobs=st["h_lp"][:bucket], out_q=st["h_q"][:bucket], latency=True)

                st["slot_np"][0], st["slot_np"][1] = st["in"].data_ptr(), 0     # warm-up and capture run on empty boards
                for _ in range(2):      # warm-up outside the capture (lazy module loads, LDS opt-ins)
                    body()
                stream.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream, capture_error_mode=CAPTURE_ERROR_MODE):
                    body()
                st["graphs"][bucket] = g
            if ch.np_converts and x.flags.writeable and x.ctypes.data % 16 == 0 and torch.from_numpy(x).is_pinned():
                st["slot_np"][0] = x.ctypes.data
            else:
                st["in"][:b].copy_(torch.from_numpy(x if x.flags.writeable else x.copy()), non_blocking=True)
                st["slot_np"][0] = st["in"].data_ptr()
            st["slot_np"][1] = b
            g.replay()
        stream.synchronize()
        lp, q = st["h_lp"].numpy()[:b], st["h_q"].numpy()[:b]
        return lp.copy(), np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])

    def _alone_config(self, m: int, n: int, k: int, latency: Optional[bool] = None) -> int:
        """Tile configuration of a hidden layer when ONE session has the device to itself (latency_mode).  Above 1 024 rows the
        automatic choice is the fat tile that wins beside a second session's kernels; alone, up to 1 728 rows the 96 x 96 tile (at
        most 2 x 256 workgroups, two per CU) and beyond that the 128 x 96 tile for the F-wide layers are faster.  Up to 1 024 rows the
        wave-specialised forms of the small tiles (two or four wavefronts that only issue the DMA pieces) are 3-15 % faster ALONE and
        5 % slower beside a second session (profiles/r04_gemm_configs.txt (3), profiles/r05_small_rows_ab.txt), so they too are asked
        for here and nowhere else.  Every configuration computes the same bits.  0 = the library's automatic choice."""
        if not (self.latency_mode if latency is None else latency):
            return 0
        wide = n > k
        if k >= 2048:   # the 64-channel net: the automatic 256 x 192 tile for the 2F-wide layer, 128 x 192 for the F-wide ones
            return 0 if (m <= 1024 or wide) else 11   # (alone at 2 048 rows: 31 us against 49)
        if m <= 1024:
            if not self.use_loader_waves:
                return 0
            # (thresholds = where a tile's grid stops being one wave of workgroups; re-probed in round 5 with every configuration,
            # tools/gemm_sweep.py, profiles/r05_gemm_configs.txt (6))
            if wide:
                return 41 if m <= 384 else (42 if m <= 576 else (44 if m <= 864 else 43))
            return 41 if m <= 512 else 42
        if m <= 1728:
            if wide and self.use_loader_waves and self.wide_tiles_r5:
                # the 2F-wide layer (round 5, profiles/r05_gemm_configs.txt (5)): 128 x 96 while its 9 x 28 tiles are one wave of workgroups
                # (10.7-11.1 us against 14-15), then 192 x 96 with two loading wavefronts (<= 9 x 28 tiles up to 1 728 rows, a quarter
                # fewer operand bytes per CU than 96 x 96: 13.5-15.2 us against 15-17.4)
                return 43 if m <= 1152 else 59
            return 44 if self.use_loader_waves else 23   # 96 x 96, four computing (+ four loading) wavefronts
        # alone, the wave-specialised forms: 128 x 192 on 8 + 4 wavefronts for the 2F-wide layer, 128 x 96 on 4 + 2 for the F-wide ones
        if self.use_loader_waves:
            return 35 if wide else 43
        return 11 if wide else 10

    use_loader_waves = True   # False: no wave-specialised (loader-wavefront) forms anywhere (A/B)
    wide_tiles_r5 = True      # False: round 4's choice for the 2F-wide layer between 1 025 and 1 728 rows (A/B)

    def _linear_relu(self, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
                     latency: Optional[bool] = None) -> torch.Tensor:
        """ReLU(x W^T + b): one hidden layer on this net's chain.  The tile configuration (c4_linear_bf16's; the other GEMMs have
        none) is `gemm_config`'s or, where that says automatic, `_alone_config`'s."""
        n, k = w.shape
        return self.chain.linear_relu(x, w, b, out, self.gemm_config[0 if n > k else 1] or self._alone_config(x.shape[0], n, k, latency))

    __call__ = forward


class GroupedNets:
    """Several bf16 `InferenceNet`s of ONE architecture as the operands of the grouped chain (c4_conv_tower_bf16_grouped,
    c4_linear_bf16_grouped, c4_head_out_bf16_grouped; include/c4a0_hip.h): every weight / bias operand of the chain stacked along a
    new leading dimension in the order of `ids` -- tw0, tw, tbias, the merged first layer (w1, b1), the heads' further hidden layers
    (pol_w / pol_b, val_w / val_b: one stacked tensor per layer) and the output layers with their f32 biases.  `forward` runs the
    chain on a batch whose rows are grouped by model (DeviceSession.route_leaves): a real row's nine outputs are bit-identical to
    what its model's InferenceNet computes for it.  What tournaments replay from a HIP graph (api._GroupedModelEvaluator)."""

    @staticmethod
    def refusal(nets: dict) -> Optional[str]:
        """None, or the reason these evaluators cannot be grouped (then a tournament takes the eager path).  Needs no GPU.
        Accepted: unmodified bf16 InferenceNets of one architecture and / or built-in players (c4a0_amd.builtin.BuiltinEvaluator)."""
        from ._lib import ROUTE_MAX_MODELS
        from .builtin import BuiltinEvaluator

        players = list(nets.values())
        if not players:
            return "no evaluators"
        # built-in players (c4a0_amd.builtin.BuiltinEvaluator) need no weights: c4_builtin_eval_grouped answers their segments of
        # the routed batch beside the networks' chain (builtin.GroupedPlayers); the conditions below are the networks'
        evs = [ev for ev in players if not isinstance(ev, BuiltinEvaluator)]
        for ev in evs:
            if not isinstance(ev, InferenceNet):
                return "an evaluator is not a c4a0_amd.nn.InferenceNet"
            if type(ev).forward is not InferenceNet.forward or type(ev).__call__ is not InferenceNet.__call__:
                return "an evaluator overrides InferenceNet.forward (it must see every evaluation)"
            if getattr(ev, "head_dtype", None) is not None:
                return "fp8 hidden layers run through the Python host loop (the grouped chain is bf16)"
        if len(players) > ROUTE_MAX_MODELS:
            return f"more than {ROUTE_MAX_MODELS} models"
        builtins = [ev for ev in players if isinstance(ev, BuiltinEvaluator)]
        home = (evs or builtins)[0].device
        for ev in builtins:
            if ev.device != home:
                return f"the evaluators are on different devices ({home}, {ev.device})"
        if not evs:   # built-in players alone: no chain, nothing more to ask
            return None
        a = evs[0]
        for ev in evs:
            if len(ev.pol_w) < 2 or len(ev.val_w) < 2 or ev.merged_w1 is None:
                return "a head without a hidden layer (the grouped chain starts with the merged first layer of both heads)"
        for ev in evs[1:]:
            if ev.channels != a.channels:
                return f"the architectures differ: {a.channels} and {ev.channels} channels"
            if ev.n_blocks != a.n_blocks:
                return f"the architectures differ: {a.n_blocks} and {ev.n_blocks} residual blocks"
            if (len(ev.pol_w), len(ev.val_w)) != (len(a.pol_w), len(a.val_w)):
                return f"the architectures differ: head depths (policy, value) {(len(a.pol_w), len(a.val_w))} and {(len(ev.pol_w), len(ev.val_w))}"
        for ev in evs[1:]:
            if ev.device != a.device:
                return f"the evaluators are on different devices ({a.device}, {ev.device})"
        for ev in evs:
            if not ev.fused_step_ok or ev.path != "hip" or ev.dtype != torch.bfloat16 or not ev.batch_invariant:
                return "an evaluator does not run the hand-written bf16 kernels (path 'hip', bfloat16, batch-invariant)"
            if ev.gemm_config != (0, 0) or ev.tower_config or not ev.use_loader_waves or not ev.wide_tiles_r5 or ev.stage_hook is not None:
                return "an evaluator carries a measurement switch (tile configuration, stage hook)"
        return None

    def __init__(self, nets: dict):
        why = GroupedNets.refusal(nets)
        if why is not None:
            raise ValueError(f"GroupedNets: {why}")
        if not all(isinstance(ev, InferenceNet) for ev in nets.values()):
            raise ValueError("GroupedNets stacks networks; built-in players go through c4a0_amd.builtin.GroupedPlayers")
        self.ids = [int(k) & ((1 << 64) - 1) for k in nets]
        evs = list(nets.values())
        a = evs[0]
        self.L: ctypes.CDLL = lib()
        self.device, self.dtype, self.channels, self.n_blocks, self.n_models = a.device, torch.bfloat16, a.channels, a.n_blocks, len(evs)
        self.row_align = int(self.L.c4_grouped_row_align())
        stack = lambda ts: torch.stack([t for t in ts]).contiguous()
        b32 = lambda ev, b: ev.chain._bias32[b.data_ptr()]     # the f32 copy c4_linear_bf16's epilogue is handed
        self.tw0, self.tw, self.tbias = stack(ev.tw0 for ev in evs), stack(ev.tw for ev in evs), stack(ev.tbias for ev in evs)
        self.w1, self.b1 = stack(ev.merged_w1 for ev in evs), stack(b32(ev, ev.merged_b1) for ev in evs)
        self.pol_w = [stack(ev.pol_w[i] for ev in evs) for i in range(1, len(a.pol_w) - 1)]
        self.pol_b = [stack(b32(ev, ev.pol_b[i]) for ev in evs) for i in range(1, len(a.pol_w) - 1)]
        self.val_w = [stack(ev.val_w[i] for ev in evs) for i in range(1, len(a.val_w) - 1)]
        self.val_b = [stack(b32(ev, ev.val_b[i]) for ev in evs) for i in range(1, len(a.val_w) - 1)]
        self.pol_out_w, self.val_out_w = stack(ev.pol_w[-1] for ev in evs), stack(ev.val_w[-1] for ev in evs)
        self.pol_out_b, self.val_out_b = stack(ev.pol_b32 for ev in evs), stack(ev.val_b32 for ev in evs)
        self.model_ids = torch.tensor(np.array(self.ids, dtype=np.uint64).view(np.int64), dtype=torch.int64, device=self.device)

    def buffers(self, rows_cap: int) -> dict:
        """The chain's activations for batches of rows_cap rows: allocated once, so that a captured round owns no allocation."""
        f = 42 * self.channels
        mk = lambda *shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype, device=self.device)
        return {"rows_cap": int(rows_cap), "planes": mk(rows_cap, 2, 6, 7), "feat": mk(rows_cap, f), "h1": mk(rows_cap, 2 * f),
                "p": [mk(rows_cap, f) for _ in range(min(2, len(self.pol_w)))], "v": [mk(rows_cap, f) for _ in range(min(2, len(self.val_w)))],
                "answers": mk(rows_cap, 9, dtype=torch.float32)}

    def tower(self, planes, seg_start, out):
        check(self.L.c4_conv_tower_bf16_grouped(planes.data_ptr(), self.tw0.data_ptr(), self.tw.data_ptr() if self.n_blocks else None, self.tbias.data_ptr(),
                                                seg_start.data_ptr(), self.n_models, planes.shape[0], self.channels, self.n_blocks, out.data_ptr(),
                                                _stream(self.device)))
        return out

    def linear_relu(self, x, w, b, seg_start, out):
        assert x.stride(1) == 1 and out.stride(1) == 1
        check(self.L.c4_linear_bf16_grouped(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), seg_start.data_ptr(), self.n_models, x.shape[0],
                                            w.shape[1], w.shape[2], x.stride(0), out.stride(0), 1, _stream(self.device)))
        return out

    def head_out(self, p, v, seg_start, answers):
        assert p.stride(1) == 1 and v.stride(1) == 1
        check(self.L.c4_head_out_bf16_grouped(p.data_ptr(), v.data_ptr(), self.pol_out_w.data_ptr(), self.val_out_w.data_ptr(), self.pol_out_b.data_ptr(),
                                              self.val_out_b.data_ptr(), seg_start.data_ptr(), self.n_models, p.shape[0], p.shape[1], p.stride(0), v.stride(0),
                                              answers.data_ptr(), _stream(self.device)))
        return answers

    @torch.no_grad()
    def forward(self, buf: dict, seg_start: torch.Tensor) -> torch.Tensor:
        """buf["planes"] (rows grouped by model, segment bounds seg_start int32[n_models + 1] on the device) -> buf["answers"]
        f32 [rows_cap, 9]: InferenceNet.forward's chain, one grouped launch per layer."""
        x = self.tower(buf["planes"], seg_start, buf["feat"])
        h = self.linear_relu(x, self.w1, self.b1, seg_start, buf["h1"])
        f = h.shape[1] // 2
        p, v = h[:, :f], h[:, f:]
        for i, (w, b) in enumerate(zip(self.pol_w, self.pol_b)):
            p = self.linear_relu(p, w, b, seg_start, buf["p"][i & 1])
        for i, (w, b) in enumerate(zip(self.val_w, self.val_b)):
            v = self.linear_relu(v, w, b, seg_start, buf["v"][i & 1])
        return self.head_out(p, v, seg_start, buf["answers"])


class GraphedEvaluator:
    """The evaluator captured once in a HIP graph: one replay per step instead of ~25 eager
    launches.  Reads `planes`, writes `logprobs` and `q` (the session's bound tensors)."""

    def __init__(self, net: InferenceNet, planes: torch.Tensor, logprobs: torch.Tensor, q: torch.Tensor, warmup: int = 3):
        self.net, self.planes, self.logprobs, self.q = net, planes, logprobs, q
        side = torch.cuda.Stream(device=planes.device)
        side.wait_stream(torch.cuda.current_stream(planes.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                net.forward(planes, out_logprobs=logprobs, out_q=q)
        torch.cuda.current_stream(planes.device).wait_stream(side)
        torch.cuda.synchronize(planes.device)
        self.graph = torch.cuda.CUDAGraph()
        from .session import CAPTURE_ERROR_MODE
        with torch.cuda.graph(self.graph, capture_error_mode=CAPTURE_ERROR_MODE):
            net.forward(planes, out_logprobs=logprobs, out_q=q)

    def __call__(self, _planes: torch.Tensor):
        self.graph.replay()
        return self.logprobs, self.q


def flops_per_leaf(cfg: ModelConfig) -> int:
    """2*MAC count of one forward."""
    c, f = cfg.conv_filter_size, cfg.conv_filter_size * 42
    conv = 2 * 42 * 9 * 2 * c + cfg.n_residual_blocks * 2 * (2 * 42 * 9 * c * c)
    pol = (cfg.n_policy_layers - 1) * 2 * f * f + 2 * 7 * f
    val = (cfg.n_value_layers - 1) * 2 * f * f + 2 * 2 * f
    return conv + pol + val

