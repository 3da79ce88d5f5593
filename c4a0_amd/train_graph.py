"""The optimiser step of training as device work only: `HipAdam`, Adam over every parameter of a network in one launch
(`c4_train_adam_f32`, c4a0_amd/csrc/c4_train_adam.hip), `train_step`, the one place a step is written down (zero_grad, forward, `loss`,
backward, the optimiser), and the two ways `fit` runs it: `EagerSteps`, and `GraphedSteps` / `GraphedTrainStep`, one whole step -- the
gather of the batch, `train_step` and the epoch's running loss -- captured once as a HIP graph and replayed.

An eager step of the default network is bound by the host (2.91 ms a step around 0.6 ms of hidden-block kernels);
`torch.optim.Adam` alone makes a dozen passes over some 30 tensors and keeps its step count on the host, where a replayed graph cannot
advance it.  `HipAdam` keeps the count in device memory and gives every parameter a persistent `.grad`, so that every pointer a
captured step touches is the one the replay touches.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from ._lib import ADAM_BLOCK_ELEMS, AdamSegment, check, lib
from .session import capture
from .train_common import cuda_stream, kernel_refusal
from .train_heads import resolve_heads, step_losses
from .train_out import resolve_outputs
from .train_tower import resolve_tower

OPTIMIZERS = ("auto", "torch", "hip")
WARMUP_STEPS = 3   # eager steps of a shape before its capture: hipBLASLt's workspaces and MIOpen's choice of algorithm are made lazily


def resolve_optimizer(optimizer: str = "auto", graph: bool = False) -> str:
    """"torch" or "hip".  "auto" is "torch" without a graph (the stock loop) and "hip" with one; graph=True with "torch" raises
    ValueError: `torch.optim.Adam` counts its steps on the host, where a replayed graph cannot advance them."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
    if graph and optimizer == "torch":
        raise ValueError('graph=True needs optimizer="hip": torch.optim.Adam keeps its step count on the host, where a replayed graph '
                         'cannot advance it')
    if optimizer == "auto":
        return "hip" if graph else "torch"
    return optimizer


def graph_refusal(model: nn.Module) -> Optional[str]:
    """Why a step of `model` cannot be captured (or run with HipAdam), or None if it can."""
    return kernel_refusal(model, not_f32="the model is not f32 (HipAdam's kernel is f32)")


def adam_table(segments: Sequence[Tuple[int, int, int, int, int]]) -> Tuple[np.ndarray, int]:
    """(the c4_adam_segment table as a numpy uint8 array, n_blocks) of segments (p, g, m, v, n): device addresses and a length."""
    table = (AdamSegment * len(segments))()
    first = 0
    for s, (p, g, m, v, n) in zip(table, segments):
        if n < 1 or any(a % 16 for a in (p, g, m, v)):
            raise ValueError("an Adam segment has n >= 1 elements and 16-byte aligned p, g, m and v")
        s.p, s.g, s.m, s.v, s.n, s.first_block, s.reserved = p, g, m, v, n, first, 0
        first += (n + ADAM_BLOCK_ELEMS - 1) // ADAM_BLOCK_ELEMS
    return np.frombuffer(bytes(table), dtype=np.uint8).copy(), first


class HipAdam:
    """Adam with coupled L2 -- `torch.optim.Adam(params, lr, betas, eps, weight_decay)` -- whose `step()` is one `c4_train_adam_f32` on
    the current stream.  m, v, the step count (a uint32) and the segment table live in device memory; every parameter gets a
    persistent zero-filled `.grad` into which autograd accumulates in place, and `zero_grad()` zeroes it, never drops it.  The
    arithmetic is include/c4a0_hip.h's "training: the optimiser"."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        self.params: List[torch.Tensor] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("HipAdam: no parameter requires a gradient")
        dev = self.params[0].device
        for p in self.params:
            if p.device != dev or dev.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"HipAdam takes contiguous f32 parameters on one HIP device, not {p.dtype} on {p.device}")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.device = dev
        self.grads = []
        for p in self.params:
            p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self.grads.append(p.grad)
        self.m = [torch.zeros_like(g) for g in self.grads]
        self.v = [torch.zeros_like(g) for g in self.grads]
        self.step_count = torch.zeros(4, dtype=torch.int32, device=dev)   # [0] is the count; 16 bytes
        table, self.n_blocks = adam_table([(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                                           for p, g, m, v in zip(self.params, self.grads, self.m, self.v)])
        self.table = torch.from_numpy(table).to(dev)
        self.n_segs = len(self.params)

    def step(self) -> None:
        check(lib().c4_train_adam_f32(self.table.data_ptr(), self.n_segs, self.n_blocks, self.step_count.data_ptr(), self.lr, self.betas[0],
                                      self.betas[1], self.eps, self.weight_decay, cuda_stream(self.device)))

    def zero_grad(self) -> None:
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:   # dropped or replaced from outside: the table points at g
                p.grad = g
        torch._foreach_zero_(self.grads)

    @property
    def steps(self) -> int:
        """The device's step count (synchronises: for tests and logs)."""
        return int(self.step_count[0].item()) & 0xFFFFFFFF

    def state(self) -> List[torch.Tensor]:
        """Every tensor of the optimiser's state, for a snapshot: m, v and the count."""
        return self.m + self.v + [self.step_count]

    def release(self) -> None:
        """Drop the persistent gradients from the parameters (the optimiser is finished)."""
        for p in self.params:
            p.grad = None


def train_step(model: nn.Module, opt, batch: Sequence[torch.Tensor], heads_path: str, tower_path: str, outputs_path: str = "torch") -> torch.Tensor:
    """THE optimiser step of training on `batch` = (pos, policy, q_penalty, q_no_penalty), on resolved paths: zero_grad, the forward and the
    loss (`train_heads.step_losses`: with outputs_path "torch" `loss(forward_resolved(...))`, with "hip" train_out's kernels), backward,
    `opt.step()`.  Returns the step's loss, detached.  `torch.optim.Adam` drops its gradients; `HipAdam.zero_grad()` zeroes
    its persistent ones in place."""
    if isinstance(opt, torch.optim.Optimizer):
        opt.zero_grad(set_to_none=True)
    else:
        opt.zero_grad()
    step_loss = step_losses(model, batch, heads_path, tower_path, outputs_path)[0]
    step_loss.backward()
    opt.step()
    return step_loss.detach()


class EagerSteps:
    """The steps of one `fit` run eagerly, with either optimiser: `run(idx)` gathers the batch and takes `train_step`; `total` (a float64
    device scalar, a fresh zero after every `reset()`) is the epoch's running sum of loss * rows."""

    def __init__(self, model: nn.Module, opt, heads_path: str, train: Sequence[torch.Tensor], tower_path: str, outputs_path: str = "torch"):
        self.model, self.opt, self.heads_path, self.tower_path, self.train = model, opt, heads_path, tower_path, train
        self.outputs_path = outputs_path
        self.reset()

    def reset(self) -> None:
        self.total = torch.zeros((), dtype=torch.float64, device=self.train[0].device)

    def run(self, idx: torch.Tensor) -> None:
        step_loss = train_step(self.model, self.opt, tuple(t[idx] for t in self.train), self.heads_path, self.tower_path, self.outputs_path)
        self.total += step_loss.double() * idx.shape[0]


class GraphedTrainStep:
    """One optimiser step of `model` on `batch_size` rows of `train` as a HIP graph.  The graph holds the gather of the batch from the
    training tensors by the static index buffer, `train_step` on heads_path, tower_path and outputs_path (checked once, here, as
    `forward_train` and `loss_train` check them) and `total += loss * rows` (`total`: a float64 device scalar, the epoch's running sum; one is made if none is given).
    `run(idx)` copies the indices into the static buffer and replays: nothing else happens on the host.

    Before the capture WARMUP_STEPS eager steps run on the capture's side stream, because the vendor libraries initialise lazily; the
    parameters, the buffers (running statistics, num_batches_tracked), m, v, the step count and `total` are snapshotted before them and
    restored in place after them, and a capture executes nothing: the first replay is the first step."""

    def __init__(self, model: nn.Module, opt: HipAdam, heads_path: str, batch_size: int, train: Sequence[torch.Tensor],
                 total: Optional[torch.Tensor] = None, tower_path: str = "torch", outputs_path: str = "torch"):
        why = graph_refusal(model)
        if why is not None:
            raise ValueError(f"graph=True: {why}")
        if batch_size < 2:
            raise ValueError("a training step needs at least 2 rows (BatchNorm in train mode)")
        dev = opt.device
        self.train = tuple(train)
        heads_path, tower_path = resolve_heads(model, heads_path, self.train[0]), resolve_tower(model, tower_path, self.train[0])
        outputs_path = resolve_outputs(model, outputs_path, self.train[0])
        self.model, self.opt, self.heads_path, self.tower_path, self.batch_size = model, opt, heads_path, tower_path, int(batch_size)
        self.outputs_path = outputs_path
        self.total = total if total is not None else torch.zeros((), dtype=torch.float64, device=dev)
        self.idx = torch.zeros(self.batch_size, dtype=torch.int64, device=dev)
        self.batch = tuple(torch.empty((self.batch_size,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in self.train)
        self.pos, self.policy, self.q_penalty, self.q_no_penalty = self.batch

        def step():
            for src, dst in zip(self.train, self.batch):
                torch.index_select(src, 0, self.idx, out=dst)
            self.total += train_step(model, opt, self.batch, heads_path, tower_path, outputs_path).double() * self.batch_size

        keep = [t for t in list(model.parameters()) + list(model.buffers()) + opt.state() + [self.total]]
        current = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        with torch.no_grad():
            saved = [t.clone() for t in keep]
        side.wait_stream(current)   # AFTER the snapshot is queued: the warm-up, which writes what it reads, waits for the clones too
        with torch.cuda.stream(side):
            for _ in range(WARMUP_STEPS):
                step()
            with torch.no_grad():
                for t, s in zip(keep, saved):
                    t.copy_(s)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with capture(self.graph, side):
            step()
        current.wait_stream(side)

    def run(self, idx: torch.Tensor) -> None:
        self.idx.copy_(idx, non_blocking=True)
        self.graph.replay()


class GraphedSteps:
    """The graphs of one `fit`: one `GraphedTrainStep` per batch shape, captured when the shape first comes (two at most: the full
    batch and the epoch's last partial one), all adding to one `total`."""

    def __init__(self, model: nn.Module, opt: HipAdam, heads_path: str, train: Sequence[torch.Tensor], tower_path: str = "torch",
                 outputs_path: str = "torch"):
        self.model, self.opt, self.heads_path, self.tower_path, self.train = model, opt, heads_path, tower_path, train
        self.outputs_path = outputs_path
        self.total = torch.zeros((), dtype=torch.float64, device=opt.device)
        self.by_rows: Dict[int, GraphedTrainStep] = {}

    def reset(self) -> None:
        self.total.zero_()   # in place: the captured steps add to this tensor

    def run(self, idx: torch.Tensor) -> None:
        rows = int(idx.shape[0])
        step = self.by_rows.get(rows)
        if step is None:
            step = self.by_rows[rows] = GraphedTrainStep(self.model, self.opt, self.heads_path, rows, self.train, self.total, self.tower_path,
                                                          self.outputs_path)
        step.run(idx)
