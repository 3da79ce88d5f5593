"""Shared helpers of the parity tests (test infrastructure)."""
from __future__ import annotations

import numpy as np

P1, P2, P3, P4, MOD = 1000003, 998244353, 19260817, 1000000007, 2147483647


def planes_to_pos_np(planes: np.ndarray):
    """float[B,2,6,7] -> (mask, value) uint64 arrays (inverse of c4r.rs:378-392)."""
    b = planes.reshape(planes.shape[0], 2, 42) != 0
    w = (np.uint64(1) << np.arange(42, dtype=np.uint64))
    value = (b[:, 0, :].astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
    opp = (b[:, 1, :].astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
    return value | opp, value


def hash_eval_np(_model_id, planes: np.ndarray):
    """numpy twin of oracle c4o_hash_eval_pos (reference callback signature)."""
    mask, value = planes_to_pos_np(planes)
    mask = mask.astype(np.int64)
    value = value.astype(np.int64)
    h = ((value & 0x1FFFFF) * P1 + (value >> 21) * P2 + (mask & 0x1FFFFF) * P3 + (mask >> 21) * P4) % MOD
    c = np.arange(7, dtype=np.int64)[None, :]
    hc = (h[:, None] * (2 * c + 3) + 7919 * c) % 1000003
    logits = ((hc & 63) - 32).astype(np.float32) / np.float32(8.0)
    qp = (((h >> 5) & 255) - 128).astype(np.float32) / np.float32(128.0)
    qn = (((h >> 13) & 255) - 128).astype(np.float32) / np.float32(128.0)
    return logits, qp, qn


def hash_eval_torch(planes):
    """torch twin (device evaluator): planes[G,2,6,7] -> (logits[G,7] f32, q[G,2] f32)."""
    import torch

    g = planes.shape[0]
    b = (planes.reshape(g, 2, 42) != 0).to(torch.int64)
    w = (torch.ones(42, dtype=torch.int64, device=planes.device) << torch.arange(42, dtype=torch.int64, device=planes.device))
    value = (b[:, 0, :] * w).sum(dim=1)
    mask = value | (b[:, 1, :] * w).sum(dim=1)
    h = ((value & 0x1FFFFF) * P1 + (value >> 21) * P2 + (mask & 0x1FFFFF) * P3 + (mask >> 21) * P4) % MOD
    c = torch.arange(7, dtype=torch.int64, device=planes.device)[None, :]
    hc = (h[:, None] * (2 * c + 3) + 7919 * c) % 1000003
    logits = ((hc & 63) - 32).to(torch.float32) / 8.0
    qp = (((h >> 5) & 255) - 128).to(torch.float32) / 128.0
    qn = (((h >> 13) & 255) - 128).to(torch.float32) / 128.0
    return logits, torch.stack([qp, qn], dim=1)


class GraphSafeHashEval:
    """hash_eval_torch as a graph-safe device evaluator (pure device work written into the caller's
    tensors): lets the parity tests drive the HIP-graph / concurrent-session paths of play_games with
    an evaluator whose answers are exact integers of the position (independent of batch shape)."""
    graph_safe = True
    dtype = None

    def __call__(self, planes, out_logprobs=None, out_q=None):
        lp, q = hash_eval_torch(planes)
        if out_logprobs is None:
            return lp, q
        out_logprobs.copy_(lp)
        out_q.copy_(q)
        return out_logprobs, out_q


def _hash_h_np(planes: np.ndarray):
    mask, value = planes_to_pos_np(planes)
    mask = mask.astype(np.int64)
    value = value.astype(np.int64)
    return ((value & 0x1FFFFF) * P1 + (value >> 21) * P2 + (mask & 0x1FFFFF) * P3 + (mask >> 21) * P4) % MOD


def sharp_eval_np(k: int, q_mode: str = "hash", ties: bool = False):
    """numpy twin of the oracle's c4o_eval_sharp as a reference-signature callback: the hash evaluator in the regime of a trained
    network.  Logits = the hash logits x 2^k (exact in f32; raw logits, the tree's own masked softmax does the underflowing to
    subnormal and zero priors), q_mode "sat" answers sign(q) in {-1, 0, +1}, ties gives the positions with h % 8 == 0 seven
    equal logits (0) so that the last-maximum rule decides at depth.  No transcendental anywhere: every twin agrees bit for bit."""
    assert q_mode in ("hash", "sat") and 0 <= int(k) <= 16

    def cb(_model_id, planes: np.ndarray):
        logits, qp, qn = hash_eval_np(_model_id, planes)
        logits = logits * np.float32(2.0 ** int(k))
        if ties:
            logits = np.where((_hash_h_np(planes) % 8 == 0)[:, None], np.float32(0.0), logits)
        if q_mode == "sat":
            qp, qn = np.sign(qp), np.sign(qn)
        return (np.ascontiguousarray(logits, dtype=np.float32), np.ascontiguousarray(qp, dtype=np.float32),
                np.ascontiguousarray(qn, dtype=np.float32))

    return cb


def sharp_eval_torch(k: int, q_mode: str = "hash", ties: bool = False):
    """torch twin of sharp_eval_np (device evaluator): planes[G,2,6,7] -> (logits[G,7] f32, q[G,2] f32)."""
    assert q_mode in ("hash", "sat") and 0 <= int(k) <= 16

    def ev(planes):
        import torch

        logits, q = hash_eval_torch(planes)
        logits = logits * float(2.0 ** int(k))
        if ties:
            g = planes.shape[0]
            b = (planes.reshape(g, 2, 42) != 0).to(torch.int64)
            w = (torch.ones(42, dtype=torch.int64, device=planes.device) << torch.arange(42, dtype=torch.int64, device=planes.device))
            value = (b[:, 0, :] * w).sum(dim=1)
            mask = value | (b[:, 1, :] * w).sum(dim=1)
            h = ((value & 0x1FFFFF) * P1 + (value >> 21) * P2 + (mask & 0x1FFFFF) * P3 + (mask >> 21) * P4) % MOD
            logits = torch.where((h % 8 == 0)[:, None], torch.zeros_like(logits), logits)
        if q_mode == "sat":
            q = torch.sign(q)
        return logits, q

    return ev


class GraphSafeSharpEval(GraphSafeHashEval):
    """sharp_eval_torch as a graph-safe device evaluator (see GraphSafeHashEval)."""

    def __init__(self, k: int, q_mode: str = "hash", ties: bool = False):
        self.ev = sharp_eval_torch(k, q_mode, ties)

    def __call__(self, planes, out_logprobs=None, out_q=None):
        lp, q = self.ev(planes)
        if out_logprobs is None:
            return lp, q
        out_logprobs.copy_(lp)
        out_q.copy_(q)
        return out_logprobs, out_q


def sharp_model(blocks: int, channels: int, k: int, seed: int = 1337):
    """A default-initialised ConnectFourNet (4 policy / 2 value layers) sharpened into the regime of a trained one: the policy
    output layer (weight and bias) x 2^k, the value output layer x 2^(k // 2) and its bias + 0.5 afterwards.  Powers of two keep
    the bf16 weights exact scalings of the unsharpened network's; the priors turn peaked and tanh saturates, so the search goes
    deep (tests/test_sharp_regime.py asserts how deep)."""
    import torch
    from c4a0_amd.nn import ConnectFourNet, ModelConfig

    torch.manual_seed(seed)
    model = ConnectFourNet(ModelConfig(blocks, channels, 4, 2)).eval()
    pol, val = model.fc_policy[-2], model.fc_value[-2]
    with torch.no_grad():
        pol.weight.mul_(2.0 ** k)
        pol.bias.mul_(2.0 ** k)
        val.weight.mul_(2.0 ** (k // 2))
        val.bias.mul_(2.0 ** (k // 2)).add_(0.5)
    return model


# sharp_model's k in the GPU tests.  Measured on the oracle with the f32 PyTorch model as its evaluator (tests/test_sharp_regime.py
# asserts the first): 4 x 32, n = 100, 32 games: 15.7 % of the simulations at depth >= 16 with k = 8, 29 % with 9, 38 % with 10;
# 8 x 64, n = 800, 8 games: 8.2 %, 28 %, 32 %.  8 meets the CPU floor of 10 % but leaves the 8 x 64 shape near the 3 % the GPU
# replay must show with bf16 answers; 9 clears both with room.
SHARP_MODEL_K = 9

# The evaluators of the sharp regime, (k, q_mode, ties), and with which exploration constant they are played.
SHARP_EVALS = {
    "k4": ((4, "hash", False), 6.6),
    "k4sat": ((4, "sat", False), 6.6),
    "k5sat": ((5, "sat", False), 1.4),
    "k4ties": ((4, "sat", True), 6.6),
}

# T1 matrix of the sharp regime: tests/test_gpu_sharp_regime.py plays each job on the device against the oracle, and
# tests/test_sharp_regime.py holds the oracle alone, on exactly these jobs (ids, n, c, evaluator, Dirichlet), to the coverage
# floors.  (name, evaluator, n, planes, first id, options); every job is N_SHARP_GAMES games on N_SHARP_SLOTS slots, so every
# slot is refilled.  The tie evaluator spreads a search over seven equal priors at one position in eight and reaches the floors
# of the deep path at n = 400 only; it runs at 24 and 400.  Dirichlet noise (0.3, 0.25) gives every child of a root a share of its
# visits, so a move straight after a move becomes rare (1-3 % of the moves at n >= 100, under that floor): the noisy jobs run at
# n = 24, where the noise meets the zero and subnormal priors; below the root it changes nothing.  The reclaimed arenas run under the
# k = 5, c = 1.4 evaluator: it expands 250-740 nodes per game, several halves' worth, where k = 4 reuses its tree (95 per game).
N_SHARP_GAMES, N_SHARP_SLOTS = 512, 256
SHARP_JOBS = [
    ("k4-n100-f32-eager", "k4", 100, "f32", 10_000, {}),
    ("k4sat-n100-bf16-graph", "k4sat", 100, "bf16", 20_000, {"graph": 8}),
    ("k5sat-n100-f32-graph", "k5sat", 100, "f32", 30_000, {"graph": 2}),
    ("k4sat-n24-f32-dirichlet", "k4sat", 24, "f32", 35_000, {"dirichlet": (0.3, 0.25)}),
    ("k4ties-n400-bf16-eager", "k4ties", 400, "bf16", 40_000, {}),
    ("k4sat-n400-f32-tiny-cache", "k4sat", 400, "f32", 50_000, {"cache": (1024, 8)}),
    ("k4-n24-bf16-roomy-cache", "k4", 24, "bf16", 60_000, {"cache": (1 << 16, 0)}),
    ("k4sat-n24-bf16-dirichlet-cache", "k4sat", 24, "bf16", 70_000, {"dirichlet": (0.3, 0.25), "cache": (1 << 16, 0)}),
    ("k5sat-n100-f32-reclaim1", "k5sat", 100, "f32", 80_000, {"reclaim": 1}),
    ("k5sat-n400-bf16-reclaim3-graph", "k5sat", 400, "bf16", 90_000, {"reclaim": 3, "graph": 4}),
    ("k4ties-n24-f32-graph", "k4ties", 24, "f32", 100_000, {"graph": 16}),
    ("k5sat-n24-f32-tiny-cache", "k5sat", 24, "f32", 110_000, {"cache": (1024, 8)}),
    ("k4-n400-f32-graph", "k4", 400, "f32", 120_000, {"graph": 8}),
    ("k4sat-n100-callback-gather", "k4sat", 100, "f32", 130_000, {"callback": True}),
]


def sharp_job_reqs(first_id: int, n_games: int = N_SHARP_GAMES):
    """ids include 0 (seed 0 on every move), colliding seeds 43 * 42 == 42 * 43 (mcts.rs:215) and 64-bit patterns"""
    ids = [0, 42, 43, 1 << 40, (1 << 64) - 1] + list(range(first_id, first_id + n_games - 5))
    return [(g, 0, 0) for g in ids]


# ------------------------------------------------------------------------------------------------ games from start positions
# The job of tests/test_start_positions.py (the oracle alone: floors, twin mutants) and tests/test_gpu_start_positions.py (the
# device against the oracle): whole games from given positions, where popcount(root) -- temperature, ply penalty, leaf model --
# and the moves the game has recorded -- move seed, Dirichlet key, record index, sign of every sample's q -- are different numbers.
START_SEED = 11
START_BANDS = ((1, 8), (8, 20), (20, 30), (30, 36), (36, 42))   # plies [lo, hi) of the random part
START_PER_BAND = 96
N_START_SLOTS = 128
# tests/test_oracle_rules.py test_pos_ops_edge_cases' drawn board, move by move
DRAWN_LINE = [0, 1, 2, 3, 4, 5] * 3 + [5, 4, 3, 2, 1, 0] * 3 + [6] * 6
_START_JOB = {}


def start_job(seed: int = START_SEED):
    """(reqs, starts, part): 495 games, shuffled so that terminal, late and early starts interleave; part[i] = "random" | "line"
    | "won", where game i's start comes from.
    Random part: 96 positions from each ply band of START_BANDS, the first of O.random_positions_np(200_000, seed) that fall into
    it (terminal ones, kind 2, included as they come).  Constructed part: DRAWN_LINE cut k = 0..6 moves short, each twice (k = 0:
    a terminal draw; k >= 1: one legal column, drawn after k moves, samples' q alternating 0.0 / -0.0), and Pos(0b1111, 0b1111), a
    terminal start of kind 1.  Ids: 0, 42, 43, 1 << 40, 2^64 - 1 (mcts.rs:215: seed 0 on every move, colliding seeds 43 * 42 ==
    42 * 43, 64-bit patterns) on five of the random games, then distinct ones; the players' ids differ (mcts.rs:70-76)."""
    if seed in _START_JOB:
        return _START_JOB[seed]
    from oracle import c4oracle as O

    mask, value = O.random_positions_np(200_000, seed)
    ply = np.array([bin(int(m)).count("1") for m in mask])
    starts, part = [], []
    for lo, hi in START_BANDS:
        idx = np.flatnonzero((ply >= lo) & (ply < hi))[:START_PER_BAND]
        assert len(idx) == START_PER_BAND, (lo, hi, len(idx))
        starts += [(int(mask[i]), int(value[i])) for i in idx]
        part += ["random"] * START_PER_BAND
    for k in range(7):
        starts += [O.from_moves(DRAWN_LINE[: 42 - k]).key()] * 2
        part += ["line"] * 2
    starts.append((0b1111, 0b1111))
    part.append("won")
    ids = [0, 42, 43, 1 << 40, (1 << 64) - 1]
    ids = ids + [7_000_000 + 3 * i for i in range(len(starts) - len(ids))]
    order = np.random.default_rng(seed).permutation(len(starts))
    starts, part = [starts[i] for i in order], [part[i] for i in order]
    reqs = [(g, 11, (1 << 63) + 5) for g in ids]   # ids stay in list order: the special ones land on shuffled positions
    _START_JOB[seed] = (reqs, starts, part)
    return _START_JOB[seed]


# The evaluators the job is played under: name -> (the oracle's evaluator, c_exploration, (k, q_mode, ties) of the sharp twins or
# None = the hash evaluator).
START_EVALS = {
    "hash": ("hash", 6.6, None),
    "k4sat": (("sharp",) + SHARP_EVALS["k4sat"][0], SHARP_EVALS["k4sat"][1], SHARP_EVALS["k4sat"][0]),
    "k5sat": (("sharp",) + SHARP_EVALS["k5sat"][0], SHARP_EVALS["k5sat"][1], SHARP_EVALS["k5sat"][0]),
}
# (evaluator, n): the settings of the T1 matrix below; tests/test_start_positions.py holds the oracle to the floors under each
START_SETTINGS = [("hash", 24), ("hash", 100), ("k4sat", 24), ("k5sat", 100)]
# T1 matrix of tests/test_gpu_start_positions.py: (name, evaluator, n, planes, options), every job the 495 games on N_START_SLOTS
# slots, so that three starts in four arrive through the refill.
START_JOBS = [
    ("hash-n24-f32-eager", "hash", 24, "f32", {}),
    ("hash-n100-bf16-eager", "hash", 100, "bf16", {}),
    ("k4sat-n24-bf16-graph2", "k4sat", 24, "bf16", {"graph": 2}),
    ("k5sat-n100-f32-graph8", "k5sat", 100, "f32", {"graph": 8}),
    ("hash-n100-f32-tiny-cache", "hash", 100, "f32", {"cache": (1024, 8)}),
    ("k4sat-n24-bf16-roomy-cache", "k4sat", 24, "bf16", {"cache": (1 << 16, 0)}),
    ("hash-n24-f32-dirichlet", "hash", 24, "f32", {"dirichlet": (0.3, 0.25)}),
    ("k4sat-n24-bf16-dirichlet-cache-graph", "k4sat", 24, "bf16", {"dirichlet": (0.3, 0.25), "cache": (1 << 16, 0), "graph": 4}),
    ("k5sat-n100-f32-reclaim1", "k5sat", 100, "f32", {"reclaim": 1}),
    ("hash-n100-bf16-reclaim3-graph", "hash", 100, "bf16", {"reclaim": 3, "graph": 4}),
    ("hash-n24-f32-compact", "hash", 24, "f32", {"compact": 5}),
    ("k5sat-n100-bf16-compact", "k5sat", 100, "bf16", {"compact": 7}),
    ("hash-n24-gather", "hash", 24, "f32", {"gather": True}),
    ("k4sat-n24-gather-dirichlet", "k4sat", 24, "f32", {"gather": True, "dirichlet": (0.3, 0.25)}),
]


def uniform_eval_torch(planes):
    """self_play.rs:391-403 UniformEvalPos on device."""
    import torch

    g = planes.shape[0]
    lp = torch.full((g, 7), float(np.float32(1.0) / np.float32(7.0)), dtype=torch.float32, device=planes.device)
    return lp, torch.zeros((g, 2), dtype=torch.float32, device=planes.device)


def samples_by_game(recs: np.ndarray):
    """structured sample array -> {game_id: [(mask, value, policy bytes, q_pen bits, q_nopen bits), ...]} in index order."""
    out = {}
    order = np.lexsort((recs["meta"] & 0xFFFF, recs["game_id"]))
    for r in recs[order]:
        out.setdefault(int(r["game_id"]), []).append(
            (int(r["mask"]), int(r["value"]), r["policy"].astype(np.float32).tobytes(),
             np.float32(r["q_penalty"]).tobytes(), np.float32(r["q_no_penalty"]).tobytes()))
    return out


def oracle_samples_by_game(res: dict):
    out = {}
    for gid, samples in res.items():
        out[int(gid)] = [(s.mask, s.value, np.array(s.policy, dtype=np.float32).tobytes(),
                          np.float32(s.q_penalty).tobytes(), np.float32(s.q_no_penalty).tobytes()) for s in samples]
    return out


def random_positions(n: int, seed: int = 1337):
    """The reference's `random_pos` strategy (c4r.rs:610-629), vectorised in numpy: play up to
    `k` random columns from the empty board, skipping illegal ones, stopping at terminal."""
    from oracle import c4oracle as O
    import random

    rng = random.Random(seed)
    out = []
    L = O.lib()
    import ctypes as C
    while len(out) < n:
        pos = O.Pos(0, 0)
        for _ in range(rng.randrange(0, 60)):
            if L.c4o_terminal_state(C.byref(pos)) != 0:
                break
            mov = rng.randrange(7)
            if (L.c4o_legal_mask(C.byref(pos)) >> mov) & 1:
                nx = O.Pos()
                L.c4o_make_move(C.byref(pos), mov, C.byref(nx))
                pos = nx
            out.append((int(pos.mask), int(pos.value)))  # every prefix is a reachable position too
            if len(out) >= n:
                break
    return out[:n]


EVIDENCE = []


def evidence(line: str) -> None:
    """A line for the end of the pytest run (tests/conftest.py pytest_terminal_summary): how much a parity test compared, so that
    the count lands in the driver's record of the run and not only in a builder-side log."""
    EVIDENCE.append(line)
