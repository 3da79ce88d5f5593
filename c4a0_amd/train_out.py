"""The end of a training step on deterministic HIP kernels (outputs="hip"): the heads' output layers -- `Linear(F, 7)` + `LogSoftmax`,
`Linear(F, 2)` + `Tanh` (reference src/c4a0/nn.py:84-85, 98-99) -- `train_common.loss` and the gradients of all of it.

`OutLossFunction` is the `torch.autograd.Function` over the two C calls `c4_train_out_loss_fwd` and `c4_train_out_loss_bwd`
(c4a0_amd/csrc/c4_train_out.hip; the arithmetic and every summation order are include/c4a0_hip.h's "training: the output layers and
the loss"): one library call forward, one backward, from f32 or bf16 activations, with `dx` returned in the activations' type.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ._lib import OUT_CHUNK_ROWS, check, lib
from .train_common import cuda_stream, kernel_refusal

OUTPUTS = ("auto", "torch", "hip")

# What outputs="auto" means where "hip" is possible.  Measured (tools/train_rate.py --outputs, profiles/train_rate_outputs.json, DESIGN
# 4.15) the kernels win -- a graphed step at batch 2 000 goes from 1.936 to 1.773 ms with heads="torch", from 1.471 to 1.354 ms with
# heads="bf16" -- but the path is opt-in: the default stays the stock ops until whole generations have been trained both ways.
AUTO_OUTPUTS = "torch"


def work_bytes(m: int, k: int) -> int:
    """c4_train_out_work_bytes: the bytes of work space a call of the output kernels needs at (m, k)"""
    n = ctypes.c_uint64(0)
    check(lib().c4_train_out_work_bytes(m, k, ctypes.byref(n)))
    return int(n.value)


def _work(m: int, k: int, device: torch.device) -> torch.Tensor:
    """The work space of a forward call and its backward call: the header's formula (c4_train_out_work_bytes; tests pin the two to each
    other), computed here so that a step makes no library call for it."""
    n_chunks = (m + OUT_CHUNK_ROWS - 1) // OUT_CHUNK_ROWS
    return torch.empty(max(4 * m + 4 * n_chunks, n_chunks * (9 * k + 12)), dtype=torch.float32, device=device)


def _rows(t: torch.Tensor) -> torch.Tensor:
    """`t` as the kernels read a matrix of activations: unit column stride, row stride a multiple of 16 bytes and at least the width,
    16-byte aligned (else a dense copy)."""
    mult = 8 if t.dtype == torch.bfloat16 else 4
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % mult == 0 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def _dense(t: torch.Tensor) -> torch.Tensor:
    """`t` dense, f32 and 16-byte aligned (a parameter or a batch's target is: then `t` itself)"""
    t = t.contiguous()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class OutLossFunction(torch.autograd.Function):
    """(xp, xv, Wp, bp, Wv, bv, policy_t, q_pen_t, q_nopen_t) -> (total, parts, out): `total` the step's loss (0-dim), `parts` [3] =
    (policy_kl, q_penalty_mse, q_no_penalty_mse) and `out` [m, 9] = (policy log-probabilities, q_penalty, q_no_penalty) per row.  Only
    `total` is differentiable; `parts` and `out` are marked non-differentiable (total and parts are one buffer of four floats, `losses`
    of the C call).  xp and xv [m, k] are both f32 or both bf16 and may be the same tensor; their gradients come back in their type.
    The forward also writes dz, the gradient of `total` at the nine pre-activations, which is all the backward needs besides x and W."""

    @staticmethod
    def forward(ctx, xp, xv, wp, bp, wv, bv, policy_t, q_pen_t, q_nopen_t):
        if xp.dtype != xv.dtype or xp.dtype not in (torch.float32, torch.bfloat16) or xp.shape != xv.shape or xp.dim() != 2:
            raise ValueError(f"the output kernels take two [m, k] matrices of activations, both f32 or both bf16, not {xp.dtype} "
                             f"{tuple(xp.shape)} and {xv.dtype} {tuple(xv.shape)}")
        m, k = xp.shape
        dev = xp.device
        xp, xv = _rows(xp), _rows(xv)
        wp, bp, wv, bv = _dense(wp), _dense(bp), _dense(wv), _dense(bv)
        policy_t, q_pen_t, q_nopen_t = _dense(policy_t), _dense(q_pen_t), _dense(q_nopen_t)
        out = torch.empty((m, 9), dtype=torch.float32, device=dev)
        dz = torch.empty((m, 9), dtype=torch.float32, device=dev)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        work = _work(m, k, dev)
        check(lib().c4_train_out_loss_fwd(xp.data_ptr(), xv.data_ptr(), int(xp.dtype == torch.bfloat16), xp.stride(0), xv.stride(0), wp.data_ptr(),
                                          bp.data_ptr(), wv.data_ptr(), bv.data_ptr(), policy_t.data_ptr(), q_pen_t.data_ptr(), q_nopen_t.data_ptr(),
                                          m, k, out.data_ptr(), dz.data_ptr(), losses.data_ptr(), work.data_ptr(), cuda_stream(dev)))
        ctx.save_for_backward(xp, xv, wp, wv, dz)
        ctx.work = work   # the backward's work space too: its contents are meaningless between the calls
        total, parts = losses[0], losses[1:]
        ctx.mark_non_differentiable(parts, out)
        return total, parts, out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_total, _d_parts, _d_out):
        xp, xv, wp, wv, dz = ctx.saved_tensors
        m, k = xp.shape
        dev = xp.device
        scale = d_total.to(torch.float32).contiguous()   # a device scalar: the host never reads it
        dxp = torch.empty((m, k), dtype=xp.dtype, device=dev) if ctx.needs_input_grad[0] else None
        dxv = torch.empty((m, k), dtype=xv.dtype, device=dev) if ctx.needs_input_grad[1] else None
        dwp, dbp = torch.empty_like(wp), torch.empty(7, dtype=torch.float32, device=dev)
        dwv, dbv = torch.empty_like(wv), torch.empty(2, dtype=torch.float32, device=dev)
        work = ctx.work
        check(lib().c4_train_out_loss_bwd(dz.data_ptr(), scale.data_ptr(), xp.data_ptr(), xv.data_ptr(), int(xp.dtype == torch.bfloat16),
                                          xp.stride(0), xv.stride(0), wp.data_ptr(), wv.data_ptr(), m, k,
                                          dxp.data_ptr() if dxp is not None else None, dxv.data_ptr() if dxv is not None else None, k, k,
                                          dwp.data_ptr(), dbp.data_ptr(), dwv.data_ptr(), dbv.data_ptr(), work.data_ptr(), cuda_stream(dev)))
        return dxp, dxv, dwp, dbp, dwv, dbv, None, None, None


def out_losses(policy_out: nn.Linear, value_out: nn.Linear, xp: torch.Tensor, xv: torch.Tensor,
               batch: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`train_common.loss`'s four values -- (total, policy_kl, q_penalty_mse, q_no_penalty_mse) -- of the two output layers on the
    heads' last activations xp and xv and `batch` = (pos, policy target, q_penalty target, q_no_penalty target), by the kernels."""
    total, parts, _out = OutLossFunction.apply(xp, xv, policy_out.weight, policy_out.bias, value_out.weight, value_out.bias, batch[1], batch[2],
                                               batch[3])
    return total, parts[0], parts[1], parts[2]


def out_refusal(model: nn.Module, planes: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why `model` (and `planes`) cannot take outputs="hip", or None if it can."""
    def shape(c: int) -> Optional[str]:
        return f"conv_filter_size {c} is not a multiple of 4 (F = 42 C must be a multiple of 8)" if c % 4 else None

    return kernel_refusal(model, planes, shape=shape)


def resolve_outputs(model: nn.Module, outputs: str = "auto", planes: Optional[torch.Tensor] = None) -> str:
    """"hip" or "torch".  outputs="hip" raises ValueError naming the reason where the kernels cannot run; "auto" is AUTO_OUTPUTS where
    they can and "torch" where they cannot."""
    if outputs not in OUTPUTS:
        raise ValueError(f"outputs must be one of {OUTPUTS}, not {outputs!r}")
    if outputs == "torch":
        return "torch"
    why = out_refusal(model, planes)
    if outputs == "hip":
        if why is not None:
            raise ValueError(f'outputs="hip": {why}')
        return "hip"
    return "torch" if why is not None else AUTO_OUTPUTS
