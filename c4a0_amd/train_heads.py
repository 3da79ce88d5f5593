"""Training forward / backward of ConnectFourNet with the heads' hidden blocks on hand-written HIP kernels.

A hidden block of a head is `nn.Sequential(Linear(F, F), BatchNorm1d(F), ReLU())` (reference src/c4a0/nn.py:75-100); the four of
the default network are over 90 % of a training step's FLOPs.  `HiddenBlockFunction` runs one block in train mode on
`c4_linear_f32` (z = x W^T + b), `c4_train_bn_relu_fwd_f32`, `c4_train_bn_relu_bwd_f32`, `c4_train_linear_dgrad_f32` and
`c4_train_linear_wgrad_f32` (c4a0_amd/csrc/c4_train.hip); `forward_train` walks the unchanged module tree of `c4a0_amd.nn.ConnectFourNet`
and sends its hidden triples through it.  The tower, the two output layers, log-softmax, tanh and the loss stay stock PyTorch
autograd by default; tower="hip" (opt-in) sends the tower through c4a0_amd/train_tower.py's deterministic kernels instead, and
outputs="hip" (opt-in; `step_losses`, `loss_train`) the output layers and the loss through c4a0_amd/train_out.py's.

heads="bf16" (opt-in) runs the same triples in bf16 mixed precision: `HiddenBlockBf16Function` rounds x and the f32 master weights to
bf16, takes all three products of a step -- forward x W^T, dgrad dz W, wgrad dz^T x -- from the bf16 MFMA GEMM `c4_linear_bf16`, and the
batch norm, the casts and the transposes the GEMM's k-major operands need from c4a0_amd/csrc/c4_train_bf16.hip.  Where it rounds is
include/c4a0_hip.h's "bf16 mixed-precision training"; parameters, gradients, Adam and the running statistics stay f32.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._lib import check, lib
from .train_common import cuda_stream, kernel_refusal, loss, update_running_stats
from .train_out import out_losses, resolve_outputs
from .train_tower import resolve_tower, tower_forward

HEADS = ("auto", "hip", "torch", "bf16")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """`t` as the kernels read a matrix: f32, unit column stride, row stride a multiple of 4, 16-byte aligned (else a dense copy)."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


class HiddenBlockFunction(torch.autograd.Function):
    """y = relu(batch_norm(x W^T + b)) with batch statistics (train mode).  Returns (y, mean, var): the batch mean and the BIASED
    batch variance of z, not differentiable, for the running statistics.  Saves x, z, mean and var; the backward recomputes the
    pre-activation from z."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, eps: float):
        m, (n, k) = x.shape[0], weight.shape
        if m < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        L, dev = lib(), x.device
        x, w = _rows(x), weight.contiguous()
        z = torch.empty((m, n), dtype=torch.float32, device=dev)
        y = torch.empty((m, n), dtype=torch.float32, device=dev)
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        var = torch.empty(n, dtype=torch.float32, device=dev)
        s = cuda_stream(dev)
        check(L.c4_linear_f32(x.data_ptr(), w.data_ptr(), bias.data_ptr(), z.data_ptr(), m, n, k, x.stride(0), n, 0, s))
        check(L.c4_train_bn_relu_fwd_f32(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, m, n, n, n, y.data_ptr(), mean.data_ptr(),
                                         var.data_ptr(), s))
        ctx.save_for_backward(x, w, gamma, beta, z, mean, var)
        ctx.eps = eps
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, w, gamma, beta, z, mean, var = ctx.saved_tensors
        m, (n, k) = x.shape[0], w.shape
        L, dev = lib(), x.device
        dy = _rows(dy)
        dz = torch.empty((m, n), dtype=torch.float32, device=dev)
        dgamma = torch.empty(n, dtype=torch.float32, device=dev)
        dbeta = torch.empty(n, dtype=torch.float32, device=dev)
        s = cuda_stream(dev)
        check(L.c4_train_bn_relu_bwd_f32(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ctx.eps,
                                         m, n, dy.stride(0), n, n, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), s))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((m, k), dtype=torch.float32, device=dev)
            check(L.c4_train_linear_dgrad_f32(dz.data_ptr(), w.data_ptr(), dx.data_ptr(), m, n, k, n, k, s))
        dw = torch.empty((n, k), dtype=torch.float32, device=dev)
        db = torch.empty(n, dtype=torch.float32, device=dev)
        check(L.c4_train_linear_wgrad_f32(dz.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), m, n, k, n, x.stride(0), s))
        return dx, dw, db, dgamma, dbeta, None


def _rows8(t: torch.Tensor) -> torch.Tensor:
    """`t` as the bf16 kernels read a matrix: unit column stride, row stride a multiple of 8, 16-byte aligned (else a dense copy)."""
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def _cast_bf16(src: torch.Tensor, dst: bool, dst_t: bool):
    """c4_train_cast_bf16 of an f32 or bf16 matrix [m][c]: (bf16 [m][c] or None, the transpose bf16 [c][64 ceil(m / 64)], its pad
    columns zeros, or None)."""
    m, c = src.shape
    mp = 64 * ((m + 63) // 64)
    out = torch.empty((m, c), dtype=torch.bfloat16, device=src.device) if dst else None
    out_t = torch.empty((c, mp), dtype=torch.bfloat16, device=src.device) if dst_t else None
    check(lib().c4_train_cast_bf16(src.data_ptr(), int(src.dtype == torch.bfloat16), m, c, src.stride(0), out.data_ptr() if dst else None, c,
                                   out_t.data_ptr() if dst_t else None, mp, cuda_stream(src.device)))
    return out, out_t


def _linear_bf16(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, m: int, n: int, k: int) -> torch.Tensor:
    """bf16(x[:m, :k] w[:n, :k]^T + bias) [m][n] by c4_linear_bf16, the tile configuration automatic"""
    y = torch.empty((m, n), dtype=torch.bfloat16, device=x.device)
    check(lib().c4_linear_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), m, n, k, x.stride(0), n, 0, 0, cuda_stream(x.device)))
    return y


class HiddenBlockBf16Function(torch.autograd.Function):
    """y = bf16(relu(batch_norm(bf16(bf16(x) bf16(W)^T + b)))) with batch statistics: the block in bf16 mixed precision, rounded where
    include/c4a0_hip.h's "bf16 mixed-precision training" says and nowhere else.  x is f32 (the first block of a head) or bf16 (a
    chained block, with `x_t`, the previous block's zero-padded y^T, if it made one); the parameters are f32.  Returns (y, y_t, mean,
    var): y bf16, y_t its transpose for the next block (None unless `emit_t`), mean and the BIASED variance of z in f32, not
    differentiable.  Saves xb, xb_t, Wb, z, mean, var, gamma and beta; the backward recomputes the pre-activation from z.  All
    three products are c4_linear_bf16: dgrad reads Wb^T [k][n], wgrad dz^T [n][mp] and xb^T [k][mp] with the batch as its k."""

    @staticmethod
    def forward(ctx, x, x_t, weight, bias, gamma, beta, eps: float, emit_t: bool):
        m, (n, k) = x.shape[0], weight.shape
        if m < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        L, dev = lib(), x.device
        mp = 64 * ((m + 63) // 64)
        ctx.x_dtype = x.dtype
        if x.dtype not in (torch.float32, torch.bfloat16) or x.device.type != "cuda" or any(t.dtype != torch.float32 for t in (weight, bias, gamma, beta)):
            raise ValueError(f"the bf16 block takes an f32 or bf16 input on a HIP device and f32 parameters, not {x.dtype} on {x.device}")
        if x.dtype == torch.bfloat16:
            xb = _rows8(x)
            xb_t = x_t if x_t is not None and tuple(x_t.shape) == (k, mp) else _cast_bf16(xb, False, True)[1]
        else:
            xb, xb_t = _cast_bf16(_rows8(x), True, True)
        wb = _cast_bf16(weight.contiguous(), True, False)[0]
        z = _linear_bf16(xb, wb, bias, m, n, k)
        y = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
        y_t = torch.empty((n, mp), dtype=torch.bfloat16, device=dev) if emit_t else None
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        var = torch.empty(n, dtype=torch.float32, device=dev)
        check(L.c4_train_bn_relu_fwd_bf16(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, m, n, n, n, y.data_ptr(), mean.data_ptr(),
                                          var.data_ptr(), y_t.data_ptr() if emit_t else None, mp, cuda_stream(dev)))
        ctx.save_for_backward(xb, xb_t, wb, z, mean, var, gamma, beta)
        ctx.eps = eps
        if emit_t:
            ctx.mark_non_differentiable(y_t, mean, var)
        else:
            ctx.mark_non_differentiable(mean, var)
        return y, y_t, mean, var

    @staticmethod
    def backward(ctx, dy, _dy_t, _dmean, _dvar):
        xb, xb_t, wb, z, mean, var, gamma, beta = ctx.saved_tensors
        m, (n, k) = xb.shape[0], wb.shape
        L, dev = lib(), xb.device
        mp = xb_t.shape[1]
        dy = _rows8(dy) if dy.dtype == torch.bfloat16 else _cast_bf16(_rows8(dy.float()), True, False)[0]
        dz = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
        dz_t = torch.empty((n, mp), dtype=torch.bfloat16, device=dev)
        dgamma = torch.empty(n, dtype=torch.float32, device=dev)
        dbeta = torch.empty(n, dtype=torch.float32, device=dev)
        db = torch.empty(n, dtype=torch.float32, device=dev)
        check(L.c4_train_bn_relu_bwd_bf16(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ctx.eps,
                                          m, n, dy.stride(0), n, n, dz.data_ptr(), dz_t.data_ptr(), mp, dgamma.data_ptr(), dbeta.data_ptr(),
                                          db.data_ptr(), cuda_stream(dev)))
        zeros = torch.zeros(max(n, k), dtype=torch.float32, device=dev)
        dx = None
        if ctx.needs_input_grad[0]:
            wb_t = _cast_bf16(wb, False, True)[1]                  # [k][n]: n % 64 == 0, no pad
            dx = _linear_bf16(dz, wb_t, zeros, m, k, n).to(ctx.x_dtype)
        dw = _linear_bf16(dz_t, xb_t, zeros, n, k, mp).float()
        return dx, None, dw, db, dgamma, dbeta, None, None


def hidden_block(block: nn.Sequential, x: torch.Tensor, path: str = "hip", emit_t: bool = False) -> torch.Tensor:
    """One `Sequential(Linear, BatchNorm1d, ReLU)` on the HIP kernels.  Train mode: batch statistics, and the running statistics
    move exactly as `nn.BatchNorm1d` moves them (momentum 0.1, the UNBIASED variance var m / (m - 1), num_batches_tracked += 1).
    Eval mode: the module's own forward.  path="hip": f32 in, f32 out (HiddenBlockFunction).  path="bf16": f32 or bf16 in, bf16 out
    (HiddenBlockBf16Function); with emit_t the block also writes y^T and hands it to a following block (as `y.c4_transposed`), which
    then needs no cast launch of its own."""
    lin, bn = block[0], block[1]
    if path not in ("hip", "bf16"):
        raise ValueError(f'path must be "hip" or "bf16", not {path!r}')
    if not bn.training:
        if path == "bf16":
            raise ValueError('heads="bf16": the block is in eval mode (the kernels are the train-mode block)')
        return block(x)
    if path == "bf16":
        y, y_t, mean, var = HiddenBlockBf16Function.apply(x, getattr(x, "c4_transposed", None), lin.weight, lin.bias, bn.weight, bn.bias, bn.eps,
                                                          emit_t)
        if emit_t:
            y.c4_transposed = y_t
    else:
        y, mean, var = HiddenBlockFunction.apply(x, lin.weight, lin.bias, bn.weight, bn.bias, bn.eps)
    update_running_stats(bn, mean, var, x.shape[0])
    return y


def hip_refusal(model: nn.Module, planes: Optional[torch.Tensor] = None, path: str = "hip") -> Optional[str]:
    """Why `model` (and `planes`) cannot take the "hip" path (or, path="bf16", the bf16 one), or None if it can."""
    def shape(c: int) -> Optional[str]:
        if path == "bf16" and c % 32:
            return f"conv_filter_size {c} is not a multiple of 32 (c4_linear_bf16 needs F = 42 C to be a multiple of 192)"
        if c % 16:
            return f"conv_filter_size {c} is not a multiple of 16 (F = 42 C must be a multiple of 32)"
        return None

    not_f32 = "the model is {dtype}, the kernels are f32" if path == "hip" else "the model is {dtype}, the master parameters must be f32"
    return kernel_refusal(model, planes, not_f32, shape, train_mode_of="block")


# What heads="auto" means where "hip" is possible: the path the recorded whole-step measurement shows faster at the default shape
# (tools/train_rate.py, profiles/train_rate.json "step": ModelConfig(1, 32, 4, 2), batch 2 000 on one MI355X -- 3.68 ms a step with
# heads="hip", 2.00 ms with heads="torch").  The hand-written f32 kernels do not reach the vendor GEMM yet.
AUTO_HEADS = "torch"


def resolve_heads(model: nn.Module, heads: str = "auto", planes: Optional[torch.Tensor] = None) -> str:
    """"hip", "bf16" or "torch".  heads="hip" and heads="bf16" raise ValueError naming the reason where the kernels cannot run; "auto"
    takes "torch" there.  "bf16" is opt-in: "auto" never resolves to it."""
    if heads not in HEADS:
        raise ValueError(f"heads must be one of {HEADS}, not {heads!r}")
    if heads == "torch":
        return "torch"
    why = hip_refusal(model, planes, "bf16" if heads == "bf16" else "hip")
    if heads in ("hip", "bf16"):
        if why is not None:
            raise ValueError(f'heads="{heads}": {why}')
        return heads
    return "torch" if why is not None else AUTO_HEADS


def _head(seq: nn.Sequential, x: torch.Tensor, path: str = "hip") -> torch.Tensor:
    layers = list(seq)
    for i, layer in enumerate(layers):
        if isinstance(layer, nn.Sequential):
            x = hidden_block(layer, x, path, emit_t=_emits_t(layers, i, path))
        else:
            x = layer(x.float() if x.dtype == torch.bfloat16 else x)   # the f32 output layer: autograd rounds its dx back to bf16
    return x


def forward_train(model: nn.Module, planes: torch.Tensor, heads: str = "auto", tower: str = "torch") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`model(planes)` -- (policy log-probabilities [B, 7], q_penalty [B], q_no_penalty [B]) -- with autograd, the hidden triples of
    both heads on the HIP kernels where heads resolves to "hip" (an f32 model in train mode on a HIP device whose conv_filter_size is a
    multiple of 16) or to "bf16" (the same, a multiple of 32; bf16 mixed precision), else the plain module forward.  tower: "torch" (the
    module's convolutions), "hip" (train_tower.tower_forward: the tower forward and backward on the deterministic f32 kernels; ValueError
    where they cannot run) or "auto" (train_tower.AUTO_TOWER)."""
    return forward_resolved(model, planes, resolve_heads(model, heads, planes), resolve_tower(model, tower, planes))


def forward_resolved(model: nn.Module, planes: torch.Tensor, path: str, tower_path: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`forward_train` on paths already resolved (`resolve_heads`'s and `resolve_tower`'s answers), with no check of its own: what a
    training step calls, so that a step does not walk the model's parameters on the host."""
    if path == "torch" and tower_path == "torch":
        return model(planes)
    x = _features(model, planes, tower_path)
    if path == "torch":
        q = model.fc_value(x)
        return model.fc_policy(x), q[:, 0], q[:, 1]
    q = _head(model.fc_value, x, path)
    return _head(model.fc_policy, x, path), q[:, 0], q[:, 1]


def _features(model: nn.Module, planes: torch.Tensor, tower_path: str) -> torch.Tensor:
    """the tower's output [B, 42 C] in the reference's flatten order, on the resolved tower path"""
    if tower_path == "hip":
        return tower_forward(model.conv, planes)
    x = model.conv(planes)
    return x.reshape(x.shape[0], -1)


def _emits_t(layers, i: int, path: str) -> bool:
    """a bf16 block that feeds another writes its y^T too: the next block's wgrad operand, without a cast launch"""
    return path == "bf16" and i + 1 < len(layers) and isinstance(layers[i + 1], nn.Sequential)


def _hidden(seq: nn.Sequential, x: torch.Tensor, path: str) -> Tuple[torch.Tensor, nn.Linear]:
    """A head up to its output layer: (the last hidden activations -- `x` itself where the head has no hidden layer --, the output
    `nn.Linear`).  The hidden blocks run as `_head` runs them (path "torch": the modules' own forward)."""
    layers = list(seq)
    for i, layer in enumerate(layers):
        if not isinstance(layer, nn.Sequential):
            return x, layer
        if path == "torch":
            x = layer(x)
        else:
            x = hidden_block(layer, x, path, emit_t=_emits_t(layers, i, path))
    raise ValueError("the head has no output layer")


def step_losses(model: nn.Module, batch, heads_path: str, tower_path: str, outputs_path: str = "torch"):
    """THE loss of a training step on `batch` = (pos, policy, q_penalty, q_no_penalty), on resolved paths: (total, policy_kl,
    q_penalty_mse, q_no_penalty_mse) with autograd.  outputs_path="torch": exactly `loss(forward_resolved(...), batch)`.
    outputs_path="hip": the tower and every hidden block as `forward_resolved` runs them, then the two output layers, log-softmax, tanh
    and the loss as one call of `train_out.OutLossFunction` on the heads' last activations (f32, or bf16 on the bf16 path: no cast to
    f32 and no rounding back of dx by autograd)."""
    if outputs_path == "torch":
        return loss(forward_resolved(model, batch[0], heads_path, tower_path), batch)
    x = _features(model, batch[0], tower_path)
    xv, value_out = _hidden(model.fc_value, x, heads_path)
    xp, policy_out = _hidden(model.fc_policy, x, heads_path)
    return out_losses(policy_out, value_out, xp, xv, batch)


def loss_train(model: nn.Module, batch, heads: str = "auto", tower: str = "auto", outputs: str = "auto"):
    """`loss(model(pos), batch)` -- (total, policy_kl, q_penalty_mse, q_no_penalty_mse) -- with autograd, on the paths `heads`, `tower` and
    `outputs` resolve to: the counterpart of `forward_train` for a whole step's loss.  outputs: "torch" (the stock output layers and
    `loss`), "hip" (train_out's kernels; ValueError where they cannot run) or "auto" (train_out.AUTO_OUTPUTS)."""
    planes = batch[0]
    return step_losses(model, batch, resolve_heads(model, heads, planes), resolve_tower(model, tower, planes), resolve_outputs(model, outputs, planes))
