"""Training forward / backward of ConnectFourNet with the heads' hidden blocks on hand-written HIP kernels.

A hidden block of a head is `nn.Sequential(Linear(F, F), BatchNorm1d(F), ReLU())` (reference src/c4a0/nn.py:75-100); the four of
the default network are over 90 % of a training step's FLOPs.  `HiddenBlockFunction` runs one block in train mode on
`c4_linear_f32` (z = x W^T + b), `c4_train_bn_relu_fwd_f32`, `c4_train_bn_relu_bwd_f32`, `c4_train_linear_dgrad_f32` and
`c4_train_linear_wgrad_f32` (c4a0_amd/csrc/c4_train.hip); `forward_train` walks the unchanged module tree of `c4a0_amd.nn.ConnectFourNet`
and sends its hidden triples through it.  The tower, the two output layers, log-softmax, tanh and the loss stay stock PyTorch
autograd: that is plumbing.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ._lib import check, lib

HEADS = ("auto", "hip", "torch")


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


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
        s = _stream(dev)
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
        s = _stream(dev)
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


def hidden_block(block: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """One `Sequential(Linear, BatchNorm1d, ReLU)` on the HIP kernels.  Train mode: batch statistics, and the running statistics
    move exactly as `nn.BatchNorm1d` moves them (momentum 0.1, the UNBIASED variance var m / (m - 1), num_batches_tracked += 1).
    Eval mode: the module's own forward."""
    lin, bn = block[0], block[1]
    if not bn.training:
        return block(x)
    y, mean, var = HiddenBlockFunction.apply(x, lin.weight, lin.bias, bn.weight, bn.bias, bn.eps)
    if bn.track_running_stats and bn.running_mean is not None:
        m = x.shape[0]
        with torch.no_grad():
            bn.num_batches_tracked += 1
            f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1.0 - f).add_(mean, alpha=f)
            bn.running_var.mul_(1.0 - f).add_(var * (m / (m - 1.0)), alpha=f)
    return y


def hip_refusal(model: nn.Module, planes: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why `model` (and `planes`) cannot take the "hip" path, or None if it can."""
    p = next(model.parameters())
    if p.device.type != "cuda":
        return f"the model is on {p.device}, not on a HIP device"
    if any(q.dtype != torch.float32 for q in model.parameters()):
        return f"the model is {p.dtype}, the kernels are f32"
    c = model.config.conv_filter_size
    if c % 16:
        return f"conv_filter_size {c} is not a multiple of 16 (F = 42 C must be a multiple of 32)"
    if not model.training:
        return "the model is in eval mode (the kernels are the train-mode block)"
    if planes is not None and (planes.device != p.device or planes.dtype != torch.float32):
        return f"the batch is {planes.dtype} on {planes.device}, the model f32 on {p.device}"
    return None


# What heads="auto" means where "hip" is possible: the path the recorded whole-step measurement shows faster at the default shape
# (tools/train_rate.py, profiles/train_rate.json "step": ModelConfig(1, 32, 4, 2), batch 2 000 on one MI355X -- 3.68 ms a step with
# heads="hip", 2.00 ms with heads="torch").  The hand-written f32 kernels do not reach the vendor GEMM yet.
AUTO_HEADS = "torch"


def resolve_heads(model: nn.Module, heads: str = "auto", planes: Optional[torch.Tensor] = None) -> str:
    """"hip" or "torch".  heads="hip" raises ValueError naming the reason where the kernels cannot run; "auto" takes "torch" there."""
    if heads not in HEADS:
        raise ValueError(f"heads must be one of {HEADS}, not {heads!r}")
    if heads == "torch":
        return "torch"
    why = hip_refusal(model, planes)
    if heads == "hip":
        if why is not None:
            raise ValueError(f'heads="hip": {why}')
        return "hip"
    return "torch" if why is not None else AUTO_HEADS


def _head(seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    for layer in seq:
        x = hidden_block(layer, x) if isinstance(layer, nn.Sequential) else layer(x)
    return x


def forward_train(model: nn.Module, planes: torch.Tensor, heads: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`model(planes)` -- (policy log-probabilities [B, 7], q_penalty [B], q_no_penalty [B]) -- with autograd, the hidden triples of
    both heads on the HIP kernels where heads resolves to "hip" (an f32 model in train mode on a HIP device whose conv_filter_size is a
    multiple of 16), else the plain module forward."""
    if resolve_heads(model, heads, planes) == "torch":
        return model(planes)
    x = model.conv(planes)
    x = x.reshape(x.shape[0], -1)
    q = _head(model.fc_value, x)
    return _head(model.fc_policy, x), q[:, 0], q[:, 1]
