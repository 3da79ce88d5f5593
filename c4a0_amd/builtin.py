"""The two evaluators that need no weights -- the tournament's anchors `uniform` and `random` (reference src/c4a0/tournament.py:
54-77) -- on the library's kernels (include/c4a0_hip.h "built-in players", csrc/c4_builtin.hpp), and `GroupedPlayers`: what a
tournament of networks AND anchors hands the grouped path (api._GroupedModelEvaluator).

Both players are pure functions of (kind, seed, model id, position).  The reference's RandomPlayer draws from torch's global
generator, so its answer to a position differs at every call and no game can be replayed; here the draw is keyed by the position.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._lib import BUILTIN_RANDOM, BUILTIN_UNIFORM, check, lib

_U64 = (1 << 64) - 1
KINDS = {"uniform": BUILTIN_UNIFORM, "random": BUILTIN_RANDOM}


def _kind(kind) -> int:
    k = KINDS.get(kind, kind)
    if k not in (BUILTIN_UNIFORM, BUILTIN_RANDOM):
        raise ValueError('kind must be "uniform" or "random"')
    return int(k)


def builtin_eval_numpy(x, kind, seed: int = 0, model_id: int = 0):
    """c4_builtin_eval_host: float32 positions [B, 2, 6, 7] -> (logits float32 [B, 7], q_penalty float32 [B], q_no_penalty
    float32 [B]), fresh C-contiguous arrays -- the reference's forward_numpy.  Needs no GPU."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = int(x.shape[0])
    if x.size != b * 84:
        raise ValueError("positions must be [B, 2, 6, 7]")
    lg, qp, qn = np.zeros((b, 7), np.float32), np.zeros(b, np.float32), np.zeros(b, np.float32)
    check(lib().c4_builtin_eval_host(x.ctypes.data, b, _kind(kind), int(seed) & _U64, int(model_id) & _U64, lg.ctypes.data, qp.ctypes.data, qn.ctypes.data))
    return lg, qp, qn


class BuiltinEvaluator:
    """A built-in player as a device evaluator: planes [G, 2, 6, 7] (f32 or bf16) -> (logits [G, 7] f32, q [G, 2] f32), one launch
    of c4_builtin_eval on the current stream, written into the caller's tensors where they are given.  Pure device work and a
    function of the row alone, so it is a valid single evaluator of `play_games`, `search_positions` and `Engine` (HIP graphs,
    concurrent sessions), and `play_games(evaluator={id: ...})` plays it on the grouped path beside the networks."""
    graph_safe = True        # no host synchronisation, no allocation when the outputs are given
    batch_invariant = True   # a row's answer is a function of that row
    dtype = None             # takes the session's planes as they are, f32 or bf16

    def __init__(self, kind, model_id: int = 0, seed: int = 0, device=None):
        self.kind, self.model_id, self.seed = _kind(kind), int(model_id) & _U64, int(seed) & _U64
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.L = lib()

    def __call__(self, planes: torch.Tensor, out_logprobs: Optional[torch.Tensor] = None, out_q: Optional[torch.Tensor] = None):
        if planes.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("a built-in player takes float32 or bfloat16 planes")
        if not planes.is_cuda:
            raise ValueError("a built-in player's device evaluator takes device tensors (forward_numpy answers numpy arrays)")
        rows = int(planes.shape[0])
        if planes.numel() != rows * 84:
            raise ValueError("planes must be [G, 2, 6, 7]")
        if not planes.is_contiguous():
            planes = planes.contiguous()
        if out_logprobs is None:
            out_logprobs = torch.empty((rows, 7), dtype=torch.float32, device=planes.device)
            out_q = torch.empty((rows, 2), dtype=torch.float32, device=planes.device)
        elif not (out_logprobs.is_contiguous() and out_q.is_contiguous() and out_logprobs.dtype == out_q.dtype == torch.float32
                  and out_logprobs.numel() == rows * 7 and out_q.numel() == rows * 2):
            raise ValueError("out_logprobs [G, 7] and out_q [G, 2] must be contiguous float32")
        check(self.L.c4_builtin_eval(C.c_void_p(planes.data_ptr()), 1 if planes.dtype == torch.bfloat16 else 0, rows, self.kind, self.seed, self.model_id,
                                     C.c_void_p(out_logprobs.data_ptr()), C.c_void_p(out_q.data_ptr()), C.c_void_p(torch.cuda.current_stream(planes.device).cuda_stream)))
        return out_logprobs, out_q

    def forward_numpy(self, x):
        return builtin_eval_numpy(x, self.kind, self.seed, self.model_id)


class GroupedPlayers:
    """The players of a tournament as the grouped path takes them (the interface api._GroupedModelEvaluator uses: n_models,
    model_ids, row_align, device, buffers, forward): bf16 `InferenceNet`s of one architecture, stacked (`c4a0_amd.nn.GroupedNets`),
    and / or `BuiltinEvaluator`s.  The networks' ids come first in `model_ids`: the router cuts the batch into one segment per
    player, the grouped network chain is launched for the first n_nets segments of the bounds (its kernels write nothing past
    them, and spend no arithmetic there) and c4_builtin_eval_grouped fills the rest.  With networks only this is GroupedNets'
    forward, launch for launch."""

    def __init__(self, players: dict):
        from .nn import GroupedNets, InferenceNet

        why = GroupedNets.refusal(players)
        if why is not None:
            raise ValueError(f"GroupedPlayers: {why}")
        nets = {k: v for k, v in players.items() if isinstance(v, InferenceNet)}
        self.builtins = [(int(k) & _U64, v) for k, v in players.items() if isinstance(v, BuiltinEvaluator)]
        self.nets = GroupedNets(nets) if nets else None
        self.n_nets = len(nets)
        self.n_models = len(players)
        self.L = lib()
        self.device = self.nets.device if self.nets is not None else self.builtins[0][1].device
        self.row_align = self.nets.row_align if self.nets is not None else int(self.L.c4_grouped_row_align())
        self.ids = (self.nets.ids if self.nets is not None else []) + [k for k, _ in self.builtins]
        self.model_ids = torch.tensor(np.array(self.ids, dtype=np.uint64).view(np.int64), dtype=torch.int64, device=self.device)
        n_b = len(self.builtins)
        # the built-in segments' players, as c4_builtin_eval_grouped reads them (host arrays; the kernel takes them by value)
        self._kinds = (C.c_uint32 * max(1, n_b))(*[ev.kind for _, ev in self.builtins])
        self._seeds = (C.c_uint64 * max(1, n_b))(*[ev.seed for _, ev in self.builtins])
        self._ids = (C.c_uint64 * max(1, n_b))(*[ev.model_id for _, ev in self.builtins])

    def buffers(self, rows_cap: int) -> dict:
        """The routed batch and the answers -- with networks, their chain's activations too: allocated once."""
        if self.nets is not None:
            return self.nets.buffers(rows_cap)
        return {"rows_cap": int(rows_cap), "planes": torch.zeros((rows_cap, 2, 6, 7), dtype=torch.bfloat16, device=self.device),
                "answers": torch.zeros((rows_cap, 9), dtype=torch.float32, device=self.device)}

    @torch.no_grad()
    def forward(self, buf: dict, seg_start: torch.Tensor) -> torch.Tensor:
        """buf["planes"] (rows grouped by player, seg_start int32[n_models + 1] on the device) -> buf["answers"] f32 [rows_cap, 9]."""
        if seg_start.numel() < self.n_models + 1:
            raise ValueError("seg_start must hold n_models + 1 bounds")
        if self.nets is not None:
            self.nets.forward(buf, seg_start)           # n_models = n_nets: rows from seg_start[n_nets] on are not touched
        if self.builtins:
            planes, answers = buf["planes"], buf["answers"]
            check(self.L.c4_builtin_eval_grouped(C.c_void_p(planes.data_ptr()), C.c_void_p(seg_start.data_ptr() + 4 * self.n_nets), len(self.builtins),
                                                 self._kinds, self._seeds, self._ids, int(planes.shape[0]), C.c_void_p(answers.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return buf["answers"]

