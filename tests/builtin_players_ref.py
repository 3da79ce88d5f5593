"""The built-in players (the tournament's anchors `uniform` and `random`) restated in numpy uint64 from their definition in
include/c4a0_hip.h ("built-in players") -- test infrastructure: what c4_builtin_eval_host, c4_builtin_eval and
c4_builtin_eval_grouped are compared against, bit for bit, and the callback the oracle replays tournaments with.

    value = sum [plane0[i] != 0] << i,   mask = value | sum [plane1[i] != 0] << i           (tests.helpers.planes_to_pos_np)
    uniform: seven logits 1.0, q = 0
    random:  G = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
             k = mix(seed + G); k = mix(k ^ model_id); k = mix(k ^ mask); k = mix(k ^ value)
             u[j] = mix(k + (j + 1) G) >> 40 (j = 0..7);  logit[j] = u[j] 2^-24 (j = 0..6);  q = (u[7] - 2^23) 2^-23
"""
from __future__ import annotations

import numpy as np

from tests.helpers import planes_to_pos_np

U64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
IDS = (0, 5, (1 << 63) + 7)
SEEDS = (0, (1 << 64) - 1)
KINDS = ("uniform", "random")


def _u(x: int) -> np.uint64:
    return np.uint64(int(x) & U64)


def mix(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def answers(kind: str, seed: int, model_id: int, mask: np.ndarray, value: np.ndarray):
    """(logits float32[B, 7], q_penalty float32[B], q_no_penalty float32[B]) of positions given as bitboards."""
    mask, value = np.asarray(mask, dtype=np.uint64).reshape(-1), np.asarray(value, dtype=np.uint64).reshape(-1)
    b = len(mask)
    if kind == "uniform":
        return np.ones((b, 7), np.float32), np.zeros(b, np.float32), np.zeros(b, np.float32)
    assert kind == "random"
    with np.errstate(over="ignore"):
        k = mix(np.full(b, _u(seed), dtype=np.uint64) + _u(G))
        k = mix(k ^ _u(model_id))
        k = mix(k ^ mask)
        k = mix(k ^ value)
        u = np.stack([mix(k + _u((j + 1) * G)) >> np.uint64(40) for j in range(8)], axis=1)      # uint64 [B, 8], 24 bits each
    logits = (u[:, :7].astype(np.float64) / 2.0 ** 24).astype(np.float32)                       # exact: 24-bit integers over 2^24
    q = ((u[:, 7].astype(np.int64) - (1 << 23)).astype(np.float64) / 2.0 ** 23).astype(np.float32)
    return np.ascontiguousarray(logits), q, q.copy()


def forward_numpy(kind: str, seed: int, model_id: int, planes: np.ndarray):
    mask, value = planes_to_pos_np(np.asarray(planes))
    return answers(kind, seed, model_id, mask, value)


def answers9(kind: str, seed: int, model_id: int, planes: np.ndarray) -> np.ndarray:
    """float32 [B, 9]: the row format of the grouped answers (7 logits, q_penalty, q_no_penalty)."""
    lg, qp, qn = forward_numpy(kind, seed, model_id, planes)
    return np.concatenate([lg, qp[:, None], qn[:, None]], axis=1)


def twin_callback(players: dict):
    """players = {model_id: (kind, seed)} -> a reference-signature callback cb(model_id, float32[B, 2, 6, 7]) for the oracle."""
    table = {int(k) & U64: v for k, v in players.items()}

    def cb(model_id, planes):
        kind, seed = table[int(model_id) & U64]
        return forward_numpy(kind, seed, int(model_id) & U64, planes)

    return cb


_GAMES = {}


def round_robin(ids, games_per_match: int):
    """the reference's schedule (tournament.py:127-129) as (game_id, player0_id, player1_id) triples"""
    import itertools

    pairings = list(itertools.permutations(ids, 2)) * int(games_per_match / 2)
    return [(i, p0, p1) for i, (p0, p1) in enumerate(pairings)]


def oracle_games(players: dict, games_per_match: int, n: int, c_exploration: float = 1.4):
    """(reqs, {game_id: [oracle samples]}): the round robin of players = {model_id: (kind, seed)} as the oracle plays it with the
    twin as its callback; computed once and shared (read-only)."""
    key = (tuple(players.items()), games_per_match, n, c_exploration)
    if key not in _GAMES:
        from oracle import c4oracle as O

        reqs = round_robin(list(players), games_per_match)
        played, _stats = O.self_play(reqs, 64, n, c_exploration, 0.01, twin_callback(players))
        _GAMES[key] = (reqs, played)
    return _GAMES[key]
