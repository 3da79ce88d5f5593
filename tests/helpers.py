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


# ------------------------------------------------------------------------------------------------ non-finite evaluator outputs
# A diverging network: the base evaluator (hash or sharp), its answer replaced at the positions where mix64(mask, value) % rate == 0
# by one of eight poisons, chosen evenly by further bits of the same hash.  What the reference does with each (oracle/c4_oracle.c):
#   nan_qp          NaN q_penalty: backed up along the path; the next select that compares two scores panics (utils.rs:12)
#   nan_qn          NaN q_no_penalty only: never compared, never recorded by a game (a search's record carries it)
#   inf_qp          +inf q_penalty: scores of +-inf compare fine; a second one of the other sign makes a NaN
#   nan_legal       NaN on one legal logit: f32::max ignores it, every prior of the node becomes NaN; with one legal column the
#                   masked maximum is -inf: a degenerate policy (mcts.rs:421-425)
#   nan_illegal     NaN on the full columns only: masked (c4r.rs:272-286); nothing where no column is full
#   ninf_but_one    -inf on all legal logits but one: zero priors
#   ninf_all_legal  -inf on all legal logits, the full columns finite: degenerate policy
#   inf_legal       +inf on one legal logit: degenerate policy
POISON_KINDS = ("nan_qp", "nan_qn", "inf_qp", "nan_legal", "nan_illegal", "ninf_but_one", "ninf_all_legal", "inf_legal")
_MIX = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0xD6E8FEB86659FD93)


def mix64_np(mask: np.ndarray, value: np.ndarray) -> np.ndarray:
    """63 well-mixed bits of a position (uint64 arithmetic modulo 2^64, then the top 63 bits: non-negative as an int64 too)"""
    m, v = np.asarray(mask, dtype=np.uint64), np.asarray(value, dtype=np.uint64)
    x = m * np.uint64(_MIX[0]) + v * np.uint64(_MIX[1]) + np.uint64(_MIX[2])   # (the empty board is a position like any other)
    x = x ^ (x >> np.uint64(29))
    x = x * np.uint64(_MIX[2])
    x = x ^ (x >> np.uint64(32))
    return x >> np.uint64(1)


def poison_plan_np(mask: np.ndarray, value: np.ndarray, rate: int):
    """(kind int64[B]: index into POISON_KINDS or -1 = the base answer stands, legal bool[B, 7], chosen bool[B, 7]: the one legal
    column the kinds `nan_legal`, `ninf_but_one` and `inf_legal` single out)"""
    h = mix64_np(mask, value).astype(np.int64)
    kind = np.where(h % rate == 0, (h // rate) % 8, -1)
    m = np.asarray(mask, dtype=np.uint64)
    legal = ((m[:, None] >> (np.uint64(35) + np.arange(7, dtype=np.uint64))[None, :]) & np.uint64(1)) == 0
    n_legal = legal.sum(axis=1)
    pick = (h // (8 * rate)) % np.maximum(n_legal, 1)
    chosen = legal & ((np.cumsum(legal, axis=1) - 1) == pick[:, None])
    return kind, legal, chosen


def poison_eval_np(base, rate: int):
    """`base` (a reference-signature callback: hash_eval_np or a sharp_eval_np) poisoned at one position in `rate`."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def cb(model_id, planes: np.ndarray):
        lg, qp, qn = base(model_id, planes)
        lg, qp, qn = np.array(lg, dtype=np.float32), np.array(qp, dtype=np.float32), np.array(qn, dtype=np.float32)
        mask, value = planes_to_pos_np(planes)
        kind, legal, chosen = poison_plan_np(mask, value, rate)
        k = kind[:, None]
        qp = np.where(kind == 0, nan, np.where(kind == 2, inf, qp))
        qn = np.where(kind == 1, nan, qn)
        lg = np.where((k == 3) & chosen, nan, lg)
        lg = np.where((k == 4) & ~legal, nan, lg)
        lg = np.where((k == 5) & legal & ~chosen, -inf, lg)
        lg = np.where((k == 6) & legal, -inf, lg)
        lg = np.where((k == 7) & chosen, inf, lg)
        return np.ascontiguousarray(lg, dtype=np.float32), np.ascontiguousarray(qp, dtype=np.float32), np.ascontiguousarray(qn, dtype=np.float32)

    return cb


def poison_eval_torch(base, rate: int):
    """torch twin of poison_eval_np (device evaluator; `base` = hash_eval_torch or a sharp_eval_torch): pure device work, no
    synchronisation, so it can be captured into a HIP graph.  int64 arithmetic wraps modulo 2^64 as the numpy twin's uint64 does;
    the logical shifts are arithmetic ones with the sign's copies masked away."""
    c = [x - (1 << 64) if x >= 1 << 63 else x for x in _MIX]

    def ev(planes):
        import torch

        lg, q = base(planes)
        dev = planes.device
        g = planes.shape[0]
        b = (planes.reshape(g, 2, 42) != 0).to(torch.int64)
        w = (torch.ones(42, dtype=torch.int64, device=dev) << torch.arange(42, dtype=torch.int64, device=dev))
        value = (b[:, 0, :] * w).sum(dim=1)
        mask = value | (b[:, 1, :] * w).sum(dim=1)
        x = mask * c[0] + value * c[1] + c[2]
        x = x ^ ((x >> 29) & ((1 << 35) - 1))
        x = x * c[2]
        x = x ^ ((x >> 32) & ((1 << 32) - 1))
        h = (x >> 1) & ((1 << 63) - 1)
        kind = torch.where(h % rate == 0, (h // rate) % 8, torch.full_like(h, -1))
        legal = ((mask[:, None] >> (35 + torch.arange(7, dtype=torch.int64, device=dev))[None, :]) & 1) == 0
        n_legal = legal.sum(dim=1)
        pick = (h // (8 * rate)) % torch.clamp(n_legal, min=1)
        chosen = legal & ((torch.cumsum(legal.to(torch.int64), dim=1) - 1) == pick[:, None])
        nan = torch.full_like(lg, float("nan"))
        inf = torch.full_like(lg, float("inf"))
        k = kind[:, None]
        qp, qn = q[:, 0], q[:, 1]
        qp = torch.where(kind == 0, nan[:, 0], torch.where(kind == 2, inf[:, 0], qp))
        qn = torch.where(kind == 1, nan[:, 0], qn)
        lg = torch.where((k == 3) & chosen, nan, lg)
        lg = torch.where((k == 4) & ~legal, nan, lg)
        lg = torch.where((k == 5) & legal & ~chosen, -inf, lg)
        lg = torch.where((k == 6) & legal, -inf, lg)
        lg = torch.where((k == 7) & chosen, inf, lg)
        return lg, torch.stack([qp, qn], dim=1)

    return ev


class GraphSafePoisonEval:
    """poison_eval_torch as a graph-safe device evaluator (pure device work written into the caller's tensors, as GraphSafeHashEval)."""
    graph_safe = True
    dtype = None

    def __init__(self, base, rate: int):
        self.ev = poison_eval_torch(base, rate)

    def __call__(self, planes, out_logprobs=None, out_q=None):
        lp, q = self.ev(planes)
        if out_logprobs is None:
            return lp, q
        out_logprobs.copy_(lp)
        out_q.copy_(q)
        return out_logprobs, out_q


def poison_base(base: str, form: str):
    """the base evaluator of a poison job, "hash" or a key of SHARP_EVALS, as a numpy callback ("numpy") or a torch function"""
    if base == "hash":
        return hash_eval_np if form == "numpy" else hash_eval_torch
    return (sharp_eval_np if form == "numpy" else sharp_eval_torch)(*SHARP_EVALS[base][0])


def poison_c_exploration(base: str) -> float:
    return 6.6 if base == "hash" else SHARP_EVALS[base][1]


def pos_to_planes_np(mask: np.ndarray, value: np.ndarray) -> np.ndarray:
    """(mask, value) uint64[B] -> float32[B, 2, 6, 7] (c4r.rs:378-392), the inverse of planes_to_pos_np"""
    m, v = np.asarray(mask, dtype=np.uint64), np.asarray(value, dtype=np.uint64)
    bit = np.arange(42, dtype=np.uint64)[None, :]
    mine = ((v[:, None] >> bit) & np.uint64(1)).astype(np.float32)
    opp = (((m ^ v)[:, None] >> bit) & np.uint64(1)).astype(np.float32)
    return np.stack([mine, opp], axis=1).reshape(len(m), 2, 6, 7)


# The jobs of the non-finite tier: tests/test_nonfinite_regime.py holds the oracle alone to the floors on exactly these jobs, and
# tests/test_gpu_nonfinite_regime.py plays each on the device against oracle_outcomes().  (name, base, n, planes, rate, options);
# options: "games" and "first_id" (that many games from the empty board, ids first_id onward) or "starts" (True: start_job()'s
# positions and requests, which hold the drawn line's one-legal-column chain; "columns": column_job()'s), then the
# launch form as in START_JOBS.  More games than slots, so that finished slots refill while errored slots stay dead; a job's
# errored games number at most half its slots (test_nonfinite_regime checks it), so the queue always drains.  Small n is the point:
# the gate is reached every n simulations, and the select behind it is the one the device leaves out.  Jobs that share base, n,
# rate, games and noise share one oracle run.
N_POISON_SLOTS = 128
# The id windows and rates were chosen on the oracle alone (tests/test_nonfinite_regime.py FLOORS holds each to its census): at
# n = 8, 800 games at one poisoned position in 300 give 10-16 games of class `discarded` under 64 errored games; at n = 24 the class
# is rare (2 games in 600) and those jobs do not claim it.  The start-position job reaches full columns early and claims nan_illegal.
_A = {"games": 800, "first_id": 17_000}                                  # hash, n = 8
_B = {"games": 800, "first_id": 9_800, "dirichlet": (0.3, 0.25)}         # hash, n = 8, Dirichlet noise
_C = {"games": 600, "first_id": 14_200}                                  # hash, n = 24
_E = {"games": 800, "first_id": 7_400}                                   # k4sat, n = 8
POISON_JOBS = [
    ("hash-n8-f32-eager", "hash", 8, "f32", 300, {**_A}),
    ("hash-n8-bf16-eager", "hash", 8, "bf16", 300, {**_A}),
    ("hash-n24-f32-graph4", "hash", 24, "f32", 400, {**_C, "graph": 4}),
    ("k4sat-n8-bf16-graph4", "k4sat", 8, "bf16", 300, {**_E, "graph": 4}),
    ("hash-n8-f32-dirichlet", "hash", 8, "f32", 300, {**_B}),
    ("hash-n8-f32-tiny-cache", "hash", 8, "f32", 300, {**_A, "cache": (1024, 8)}),
    ("hash-n24-bf16-roomy-cache", "hash", 24, "bf16", 400, {**_C, "cache": (1 << 16, 0)}),
    ("hash-n8-bf16-dirichlet-cache", "hash", 8, "bf16", 300, {**_B, "cache": (1 << 16, 0)}),
    ("hash-n24-f32-reclaim1", "hash", 24, "f32", 400, {**_C, "reclaim": 1}),
    ("hash-n8-f32-compact", "hash", 8, "f32", 300, {**_A, "compact": 7}),
    ("hash-n8-gather", "hash", 8, "f32", 300, {**_A, "gather": True}),
    ("hash-n8-gather-dirichlet", "hash", 8, "f32", 300, {**_B, "gather": True}),
    ("starts-hash-n24-f32-eager", "hash", 24, "f32", 150, {"starts": True}),
    ("starts-hash-n24-bf16-graph4", "hash", 24, "bf16", 150, {"starts": True, "graph": 4}),
    ("columns-hash-n8-f32-eager", "hash", 8, "f32", 4, {"starts": "columns"}),
    ("columns-hash-n8-bf16-graph4", "hash", 8, "bf16", 4, {"starts": "columns", "graph": 4}),
    ("column-pairs-hash-n8-gather", "hash", 8, "f32", 4, {"starts": "column-pairs", "gather": True}),
]
_POISON_OUTCOMES = {}


_COLUMN_JOB = []


def column_job():
    """(reqs, starts): 168 start positions with exactly ONE legal column, none terminal.  The drawn board of DRAWN_LINE has no four in
    a row, so neither has any part of it: the board, and its mirror image, with the top k = 1..6 discs of one column c = 0..6 taken
    off, once with the first player's discs as the side to move's and once with the second player's (a start position is any
    (mask, value), mcts.rs:48-56; nothing asks how it was reached).  Every node of such a game's tree has one candidate, which is
    where the reference never compares a NaN (utils.rs:12 needs two keys) and where a NaN logit leaves the masked maximum at -inf
    (f32::max ignores the NaN, mcts.rs:417-425); random play reaches 27 distinct positions of this sort in 400 000."""
    if not _COLUMN_JOB:
        from oracle import c4oracle as O

        full = O.from_moves(DRAWN_LINE)
        starts = []
        for board in (full, O.flip_h(full)):
            for c in range(7):
                for k in range(1, 7):
                    gone = sum(1 << (7 * row + c) for row in range(6 - k, 6))
                    mask = int(board.mask) & ~gone
                    for mine in (int(board.value), int(board.mask) ^ int(board.value)):
                        starts.append((mask, mine & mask))
        assert len(set(starts)) == len(starts) == 168
        _COLUMN_JOB.append(([(9_000_000 + 7 * i, 0, 0) for i in range(len(starts))], starts))
    return _COLUMN_JOB[0]


def poison_job_games(job):
    """(reqs, starts or None) of a poison job"""
    opt = job[5]
    if opt.get("starts") == "columns":
        return column_job()
    if opt.get("starts") == "column-pairs":   # every second start of column_job() twice, side by side, under two ids: with one legal
        _reqs, cols = column_job()           # column a game does not depend on its id, so the two games show the evaluator the same leaves
        starts = [p for p in cols[::2] for _ in (0, 1)]
        return [(9_500_000 + 7 * i, 0, 0) for i in range(len(starts))], starts
    if opt.get("starts"):
        reqs, starts, _part = start_job()
        return reqs, starts
    return [(g, 0, 0) for g in range(opt["first_id"], opt["first_id"] + opt["games"])], None


def poison_setting(job):
    """what a poison job's games depend on: jobs with equal settings share their oracle runs"""
    _name, base, n, _planes, rate, opt = job
    return (base, n, rate, opt.get("games"), opt.get("first_id"), opt.get("starts"), opt.get("dirichlet"))


def poison_settings():
    """the distinct settings of POISON_JOBS, each named by and given as the first job that has it"""
    seen = {}
    for job in POISON_JOBS:
        seen.setdefault(poison_setting(job), job)
    return list(seen.values())


def outcome_class(o) -> str:
    """an outcome of oracle_outcomes as one of "ok", "nan-live", "nan-discarded", "degenerate" """
    if o[0] == "ok":
        return "ok"
    return {1: "nan-" + o[1], 2: "degenerate"}[o[0]]


def oracle_outcomes(job, device_order: bool = False, twin: int = 0, evaluator=None):
    """Every game of a poison job played ALONE in the oracle (Game.step), all games in lock-step so that one evaluator batch
    answers a round.  Returns a dict (computed once per setting and shared; read-only):
      "outcomes"  per request, in order: ("ok", [sample tuples as oracle_samples_by_game gives them]) or (code, where) -- the C4O_ERR
                  code of the reference's panic and "live" | "discarded": discarded = the failing step left the root with >= n
                  visits and n_moves unchanged, i.e. the panic came from the select whose leaf the gate throws away;
      "kinds"     per request: the set of POISON_KINDS indices that fired at a non-terminal leaf of the game (nan_illegal only
                  where a column is full);
      "sims"      evaluator rows = c4o_game_step calls, all games together; "rounds" = the longest game's;
      "counters"  the games' own counters summed (c4o_counters), errored games included up to their panic.
    evaluator: a reference-signature callback to play the job's games under instead of the poisoned base (not shared; no kinds).
    device_order: the oracle plays the device's order of a job (c4o_game_set_device_order); twin: TWIN_* mutants."""
    name, base, n, _planes, rate, opt = job
    noise = opt.get("dirichlet")
    key = poison_setting(job) + (bool(device_order), int(twin))
    if evaluator is None and key in _POISON_OUTCOMES:
        return _POISON_OUTCOMES[key]
    from oracle import c4oracle as O

    reqs, starts = poison_job_games(job)
    ev = evaluator if evaluator is not None else poison_eval_np(poison_base(base, "numpy"), rate)
    c_expl = poison_c_exploration(base)
    games = []
    for i, r in enumerate(reqs):
        g = O.Game(O.Pos(*starts[i]) if starts is not None else None, *r)
        if noise:
            g.set_dirichlet(*noise)
        g.set_device_order(device_order)
        g.set_twin(twin)
        games.append(g)
    outcomes, kinds = [None] * len(reqs), [set() for _ in reqs]
    live, sims, rounds = list(range(len(reqs))), 0, 0
    while live:
        leaves = [games[i].leaf_pos() for i in live]
        mask = np.array([p.mask for p in leaves], dtype=np.uint64)
        value = np.array([p.value for p in leaves], dtype=np.uint64)
        lg, qp, qn = ev(0, pos_to_planes_np(mask, value))
        kind, legal, _chosen = poison_plan_np(mask, value, rate if evaluator is None else 1 << 58)
        nxt = []
        rounds += 1
        for j, i in enumerate(live):
            g = games[i]
            k = int(kind[j])
            if k >= 0 and O.terminal_state(leaves[j]) == 0 and (k != 4 or not legal[j].all()):
                kinds[i].add(k)
            moves = g.n_moves()
            rc = g.step(lg[j], float(qp[j]), float(qn[j]), n, c_expl, 0.01)
            sims += 1
            if rc == 0:
                nxt.append(i)
            elif rc == 1:
                outcomes[i] = ("ok", [(s.mask, s.value, np.array(s.policy, dtype=np.float32).tobytes(), np.float32(s.q_penalty).tobytes(),
                                       np.float32(s.q_no_penalty).tobytes()) for s in g.to_result(0.01)])
            else:
                discarded = g.root_visit_count() >= n and g.n_moves() == moves
                outcomes[i] = (-rc, "discarded" if discarded else "live")
        live = nxt
    ctr = {}
    for g in games:
        for k, v in g.counters().items():
            ctr[k] = max(ctr.get(k, 0), v) if k == "max_depth" else ctr.get(k, 0) + v
    res = {"outcomes": outcomes, "kinds": kinds, "sims": sims, "rounds": rounds, "counters": ctr}
    if evaluator is None:
        _POISON_OUTCOMES[key] = res
    return res


# ---- the device side of the non-finite tier: sessions stepped by hand (DeviceSession.run raises at its first poll)
# the oracle's panic codes (oracle/c4_oracle.h C4O_ERR_*) -> the library's (include/c4a0_hip.h C4_ERR_*)
C4_OF_C4O = {1: 3, 2: 4, 3: 8}   # NAN_IN_TREE, DEGENERATE_POLICY, ILLEGAL_MOVE
SLOT_ACTIVE, SLOT_IDLE = 1, 0


def note_dead_slots(s, dead, where):
    """read every slot of a DeviceSession; a slot that is neither idle nor active holds an errored game: dead[ordinal] = its status
    byte, where[ordinal] = the slot.  Returns (number of active slots, status, ordinals)."""
    _m, _v, status, ordinal = s.leaves(with_ordinals=True)
    for g in np.flatnonzero((status != SLOT_ACTIVE) & (status != SLOT_IDLE)):
        o = int(ordinal[g])
        assert dead.setdefault(o, int(status[g])) == int(status[g])
        where.setdefault(o, int(g))
    return int((status == SLOT_ACTIVE).sum()), status, ordinal


def step_eager_until_no_slot_is_active(s, ev, cap, dead, where, every=16, on_step=None):
    """evaluate + step until no slot is active, looking every `every` steps; on_step() runs between the two (observers)"""
    for step in range(1, cap + 1):
        s.evaluate(ev)
        if on_step is not None:
            on_step()
        s.step()
        if step % every == 0 and note_dead_slots(s, dead, where)[0] == 0:
            return step
    raise AssertionError(f"slots still active after {cap} steps")


def step_graph_until_no_slot_is_active(s, ev, spg, cap, dead, where):
    """replays of a HIP graph of `spg` rounds until no slot is active, looking every 4 replays"""
    import torch

    graph = s.capture_steps(ev, spg)
    for k in range(1, cap // spg + 2):
        graph.replay()
        if k % 4 == 0:
            torch.cuda.synchronize()
            if note_dead_slots(s, dead, where)[0] == 0:
                return k * spg
    raise AssertionError(f"slots still active after {cap} steps")


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
