"""What the training modules share, below all of them (train_tower, train_heads, train_graph and training import it, it imports none
of them): the loss, the stream handle the C calls take, the running statistics of a train-mode batch norm, and the checks every
refusal starts with."""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn

EPS = 1e-8  # nn.py:57: avoids log(0)


def loss(model_outputs, batch):
    """The reference's training loss (nn.py:160-181) of `model_outputs` = (policy log-probabilities [B, 7], q_penalty [B],
    q_no_penalty [B]) on `batch` = (pos, policy target, q_penalty target, q_no_penalty target):

        policy_kl = mean_b sum_j (t + EPS) (log(t + EPS) - logp)      [assumption]
        total     = policy_kl + mean (q_penalty - target)^2 + mean (q_no_penalty - target)^2

    [assumption] policy_kl restates torchmetrics' `KLDivergence(log_prob=True)` called as (log(targets + EPS), prediction) from its
    documented definition -- sum_j p_j (log p_j - log q_j) per row with p = exp of the first argument, mean over rows;
    torchmetrics itself was not available to compare against.

    Returns (total, policy_kl, q_penalty_mse, q_no_penalty_mse)."""
    logp, q_pen, q_nopen = model_outputs
    _pos, policy_t, q_pen_t, q_nopen_t = batch
    t = policy_t + EPS
    policy_kl = (t * (torch.log(t) - logp)).sum(dim=1).mean()
    q_pen_mse = ((q_pen - q_pen_t) ** 2).mean()
    q_nopen_mse = ((q_nopen - q_nopen_t) ** 2).mean()
    return policy_kl + q_pen_mse + q_nopen_mse, policy_kl, q_pen_mse, q_nopen_mse


def cuda_stream(device: torch.device) -> int:
    """the current stream of `device` as the C calls take it"""
    return torch.cuda.current_stream(device).cuda_stream


def update_running_stats(bn: nn.Module, mean: torch.Tensor, var: torch.Tensor, m: int) -> None:
    """Move a train-mode batch norm's running statistics exactly as PyTorch moves them, from the batch `mean` and the BIASED batch
    variance `var` of `m` rows: num_batches_tracked += 1, the factor `momentum` (1 / count where it is None), the UNBIASED variance
    var m / (m - 1)."""
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1.0 - f).add_(mean, alpha=f)
            bn.running_var.mul_(1.0 - f).add_(var * (m / (m - 1.0)), alpha=f)


def kernel_refusal(model: nn.Module, planes: Optional[torch.Tensor] = None, not_f32: str = "the model is {dtype}, the kernels are f32",
                   shape: Optional[Callable[[int], Optional[str]]] = None, train_mode_of: Optional[str] = None) -> Optional[str]:
    """Why `model` (and `planes`) cannot run on f32 training kernels, or None if it can.  In this order: no parameters; not on a HIP
    device; a parameter that is not f32 (`not_f32`, formatted with the first parameter's dtype); `shape(conv_filter_size)`'s own
    reason; eval mode, where `train_mode_of` names what the kernels are the train-mode form of; a batch elsewhere or not f32."""
    params = list(model.parameters())
    if not params:
        return "the model has no parameters"
    p = params[0]
    if p.device.type != "cuda":
        return f"the model is on {p.device}, not on a HIP device"
    if any(q.dtype != torch.float32 for q in params):
        return not_f32.format(dtype=p.dtype)
    why = shape(model.config.conv_filter_size) if shape is not None else None
    if why is not None:
        return why
    if train_mode_of is not None and not model.training:
        return f"the model is in eval mode (the kernels are the train-mode {train_mode_of})"
    if planes is not None and (planes.device != p.device or planes.dtype != torch.float32):
        return f"the batch is {planes.dtype} on {planes.device}, the model f32 on {p.device}"
    return None
