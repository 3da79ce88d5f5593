"""Training forward / backward of ConnectFourNet's convolution tower on deterministic HIP kernels (tower="hip").

The tower is `Conv2d(2, C)` and, per residual block, `x + ReLU(BatchNorm2d(Conv2d(Conv2d(x))))` (reference src/c4a0/nn.py:64-70, 184-195).
In train mode it is the one part of a step whose stock kernels are not a fixed function of their inputs: the vendor's convolution
backward adds with atomics.  Here every product and every reduction has one order that the shape alone decides
(include/c4a0_hip.h, "training the convolution tower"; c4a0_amd/csrc/c4_train_tower.hip), so a step repeats itself byte for byte.

Activations are cell-major `[B][42][C]`, the layout `c4_conv_tower_f32` writes: a tower activation is a row-major matrix `[42 B][C]`
and `BatchNorm2d` a batch norm over its rows.  `Conv0Function`, `Conv3x3Function` and `Bn2dReluResFunction` are the
`torch.autograd.Function`s over the C calls; the weight packing, the flipped weights of dgrad and the permute to the reference's
"c h w" flatten order at the tower's end are small tensor ops.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
import torch.nn as nn

from ._lib import check, lib
from .train_common import cuda_stream, kernel_refusal, update_running_stats

TOWERS = ("auto", "hip", "torch")

# What tower="auto" means where "hip" is possible.  The kernels' claim is reproducibility: call by call they are level with the vendor's
# convolutions, a whole step under the graph is a tie (1.886 ms against 1.897 ms) and the eager tower loses to its host side
# (tools/train_rate.py --tower, profiles/train_rate_tower.json), so the default stays the stock tower.
AUTO_TOWER = "torch"


def work_bytes(n_boards: int, c: int) -> int:
    """c4_train_tower_work_bytes: the bytes of work space a call of the tower's training kernels needs at (n_boards, C)"""
    n = ctypes.c_uint64(0)
    check(lib().c4_train_tower_work_bytes(n_boards, c, ctypes.byref(n)))
    return int(n.value)


def _work(n_boards: int, c: int, device: torch.device) -> torch.Tensor:
    """The work space of one call, from PyTorch's caching allocator like every other buffer of a step."""
    return torch.empty(work_bytes(n_boards, c) // 4, dtype=torch.float32, device=device)


def pack_conv0(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d(2, C).weight [C, 2, 3, 3] -> w0 [C][32], w0[co][2 tap + ci] (zero from 18 on): pack_f32_weights' order"""
    c = weight.shape[0]
    w0 = weight.new_zeros((c, 32))
    w0[:, :18] = weight.reshape(c, 2, 9).permute(0, 2, 1).reshape(c, 18)
    return w0


def unpack_conv0(dw0: torch.Tensor) -> torch.Tensor:
    c = dw0.shape[0]
    return dw0[:, :18].reshape(c, 9, 2).permute(0, 2, 1).reshape(c, 2, 3, 3)


def pack_conv3x3(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d(C, C).weight [co, ci, 3, 3] -> w [co][tap C + ci]"""
    co, ci = weight.shape[:2]
    return weight.reshape(co, ci, 9).permute(0, 2, 1).reshape(co, 9 * ci).contiguous()


def pack_conv3x3_dgrad(weight: torch.Tensor) -> torch.Tensor:
    """The weights with which the forward convolution of dz is dgrad: W'[ci][(8 - tap) C + co] = W[co][tap C + ci]"""
    co, ci = weight.shape[:2]
    return weight.reshape(co, ci, 9).flip(2).permute(1, 2, 0).reshape(ci, 9 * co).contiguous()


def unpack_conv3x3(dw: torch.Tensor) -> torch.Tensor:
    c = dw.shape[0]
    return dw.reshape(c, 9, c).permute(0, 2, 1).reshape(c, c, 3, 3)


class Conv0Function(torch.autograd.Function):
    """z [42 B, C] = the first convolution of planes [B, 2, 6, 7] (no gradient reaches the planes)."""

    @staticmethod
    def forward(ctx, planes, weight, bias):
        b, c, dev = planes.shape[0], weight.shape[0], planes.device
        planes = planes.contiguous()
        z = torch.empty((42 * b, c), dtype=torch.float32, device=dev)
        check(lib().c4_train_conv0_f32(planes.data_ptr(), pack_conv0(weight).data_ptr(), bias.data_ptr(), z.data_ptr(), b, c, cuda_stream(dev)))
        ctx.save_for_backward(planes)
        ctx.c = c
        return z

    @staticmethod
    def backward(ctx, dz):
        (planes,) = ctx.saved_tensors
        b, c, dev = planes.shape[0], ctx.c, planes.device
        dz = dz.contiguous()
        dw0 = torch.empty((c, 32), dtype=torch.float32, device=dev)
        db = torch.empty(c, dtype=torch.float32, device=dev)
        work = _work(b, c, dev)
        check(lib().c4_train_conv0_wgrad_f32(dz.data_ptr(), planes.data_ptr(), dw0.data_ptr(), db.data_ptr(), b, c, work.data_ptr(), cuda_stream(dev)))
        return None, unpack_conv0(dw0), db


class Conv3x3Function(torch.autograd.Function):
    """z [42 B, C] = a 3x3 convolution (padding 1) of x [42 B, C], both cell-major."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        c, dev = weight.shape[0], x.device
        b = x.shape[0] // 42
        x = x.contiguous()
        z = torch.empty_like(x)
        check(lib().c4_train_conv3x3_f32(x.data_ptr(), pack_conv3x3(weight).data_ptr(), bias.data_ptr(), z.data_ptr(), b, c, cuda_stream(dev)))
        ctx.save_for_backward(x, weight)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, weight = ctx.saved_tensors
        c, dev = weight.shape[0], x.device
        b = x.shape[0] // 42
        L, s = lib(), cuda_stream(dev)
        dz = dz.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            zero = torch.zeros(c, dtype=torch.float32, device=dev)
            check(L.c4_train_conv3x3_f32(dz.data_ptr(), pack_conv3x3_dgrad(weight).data_ptr(), zero.data_ptr(), dx.data_ptr(), b, c, s))
        dw = torch.empty((c, 9 * c), dtype=torch.float32, device=dev)
        db = torch.empty(c, dtype=torch.float32, device=dev)
        work = _work(b, c, dev)
        check(L.c4_train_conv3x3_wgrad_f32(dz.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), b, c, work.data_ptr(), s))
        return dx, unpack_conv3x3(dw), db


class Bn2dReluResFunction(torch.autograd.Function):
    """y = a + relu(batch_norm(z)) with batch statistics over the 42 B rows.  Returns (y, mean, var): the batch mean and the BIASED batch
    variance, not differentiable, for the running statistics.  The gradient with respect to a is dy itself."""

    @staticmethod
    def forward(ctx, z, a, gamma, beta, eps: float):
        c, dev = z.shape[1], z.device
        b = z.shape[0] // 42
        z, a = z.contiguous(), a.contiguous()
        y = torch.empty_like(z)
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        var = torch.empty(c, dtype=torch.float32, device=dev)
        work = _work(b, c, dev)
        check(lib().c4_train_bn2d_relu_res_fwd_f32(z.data_ptr(), a.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, b, c, y.data_ptr(),
                                                   mean.data_ptr(), var.data_ptr(), work.data_ptr(), cuda_stream(dev)))
        ctx.save_for_backward(z, mean, var, gamma, beta)
        ctx.eps = eps
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        z, mean, var, gamma, beta = ctx.saved_tensors
        c, dev = z.shape[1], z.device
        b = z.shape[0] // 42
        dy = dy.contiguous()
        dz = torch.empty_like(z)
        dgamma = torch.empty(c, dtype=torch.float32, device=dev)
        dbeta = torch.empty(c, dtype=torch.float32, device=dev)
        work = _work(b, c, dev)
        check(lib().c4_train_bn2d_relu_res_bwd_f32(dy.data_ptr(), z.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                   ctx.eps, b, c, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), work.data_ptr(), cuda_stream(dev)))
        return dz, dy, dgamma, dbeta, None


def _bn2d_relu_res(bn: nn.BatchNorm2d, z: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """a + relu(bn(z)) in train mode; the running statistics move exactly as `nn.BatchNorm2d` moves them (momentum 0.1, the UNBIASED
    variance var m / (m - 1) with m = 42 B, num_batches_tracked += 1)."""
    y, mean, var = Bn2dReluResFunction.apply(z, a, bn.weight, bn.bias, bn.eps)
    update_running_stats(bn, mean, var, z.shape[0])
    return y


def tower_forward(conv: nn.Sequential, planes: torch.Tensor) -> torch.Tensor:
    """`model.conv` on planes [B, 2, 6, 7] -> features [B, 42 C] in the reference's flatten order "c h w", with autograd, on the HIP
    kernels.  In eval mode the module's own forward runs (the kernels are the train-mode tower)."""
    b = planes.shape[0]
    if not conv.training:
        return conv(planes).reshape(b, -1)
    first = conv[0]
    c = first.weight.shape[0]
    x = Conv0Function.apply(planes, first.weight, first.bias)
    for blk in list(conv)[1:]:
        c1, c2, bn = blk.block[0], blk.block[1], blk.block[2]
        z = Conv3x3Function.apply(Conv3x3Function.apply(x, c1.weight, c1.bias), c2.weight, c2.bias)
        x = _bn2d_relu_res(bn, z, x)
    return x.reshape(b, 42, c).permute(0, 2, 1).reshape(b, 42 * c)


def tower_refusal(model: nn.Module, planes: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why `model` (and `planes`) cannot take tower="hip", or None if it can."""
    def shape(c: int) -> Optional[str]:
        return f"conv_filter_size {c} is not a multiple of 16 up to 64" if c % 16 or not 16 <= c <= 64 else None

    return kernel_refusal(model, planes, shape=shape, train_mode_of="tower")


def resolve_tower(model: nn.Module, tower: str = "auto", planes: Optional[torch.Tensor] = None) -> str:
    """"hip" or "torch".  tower="hip" raises ValueError naming the reason where the kernels cannot run; "auto" is AUTO_TOWER where they
    can and "torch" where they cannot."""
    if tower not in TOWERS:
        raise ValueError(f"tower must be one of {TOWERS}, not {tower!r}")
    if tower == "torch":
        return "torch"
    why = tower_refusal(model, planes)
    if tower == "hip":
        if why is not None:
            raise ValueError(f'tower="hip": {why}')
        return "hip"
    return "torch" if why is not None else AUTO_TOWER
