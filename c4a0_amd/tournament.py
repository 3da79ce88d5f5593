"""Round-robin tournaments: which network is the best, and how far above the two fixed anchors (reference
src/c4a0/tournament.py: `play_tournament`, `TournamentResult`, `ModelPlayer` / `RandomPlayer` / `UniformPlayer`).

The reference plays a tournament through its numpy callback, one model per evaluator tick.  Here every player that has a device
evaluator -- networks (`ModelPlayer`) and the two anchors -- is one entry of `play_games(evaluator={model_id: ...})`, which plays
such a job on the grouped path: leaves routed by player on the device, the networks' chain and one launch for all anchors,
rounds replayed from a HIP graph.  A player that only offers `forward_numpy` (a user's subclass of `Player`) sends the whole job
through the numpy callback, as the reference does.

The anchors are pure functions of (seed, model id, position) (include/c4a0_hip.h "built-in players").  The reference's
RandomPlayer draws from torch's global generator: not reproducible, another answer to the same position at every call.  Here
the draw is keyed by the position, so a tournament with `random` in it can be replayed game by game.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from datetime import datetime
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .results import _START03, GameMetadata, PlayGamesResult

_U64 = (1 << 64) - 1


class Player:
    """A participant (tournament.py:26-35): `name`, `model_id`, and how it evaluates positions."""

    def __init__(self, name: str, model_id: int):
        self.name, self.model_id = str(name), int(model_id)

    def forward_numpy(self, x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """float32 positions [B, 2, 6, 7] -> (policy logits float32 [B, 7], q_penalty float32 [B], q_no_penalty float32 [B])."""
        raise NotImplementedError

    def device_evaluator(self, device):
        """The player as a device evaluator of `play_games` on `device`, or None: it only answers numpy batches."""
        return None

    def numpy_callback(self) -> Callable:
        """The player as a `py_eval_pos_cb` of `play_games`."""
        return lambda _model_id, x: self.forward_numpy(x)


class ModelPlayer(Player):
    """Player whose policy and value come from a ConnectFourNet (tournament.py:38-51), wrapped in a `c4a0_amd.nn.InferenceNet` on
    `device` (inference_kwargs are its: dtype, strict, ...).  Named gen{model_id}."""

    def __init__(self, model_id: int, model, device, **inference_kwargs):
        import torch

        from .nn import InferenceNet

        super().__init__(f"gen{model_id}", model_id)
        self.model, self.device = model, torch.device(device)
        self.net = InferenceNet(model, self.device, **inference_kwargs)

    def forward_numpy(self, x):
        return self.net.forward_numpy(x)

    def device_evaluator(self, device):
        return self.net   # (on the device it was made for; play_games refuses a job whose evaluators live on different ones)


class _BuiltinPlayer(Player):
    kind = ""

    def __init__(self, model_id: int, seed: int = 0):
        super().__init__(self.kind, model_id)
        self.seed = int(seed)

    def forward_numpy(self, x):
        from .builtin import builtin_eval_numpy

        return builtin_eval_numpy(x, self.kind, self.seed, self.model_id)

    def device_evaluator(self, device):
        from .builtin import BuiltinEvaluator

        return BuiltinEvaluator(self.kind, self.model_id, self.seed, device)


class RandomPlayer(_BuiltinPlayer):
    """Player that answers random logits in [0, 1) and one random q in [-1, 1) (tournament.py:54-64), named "random".  Unlike
    the reference's, which draws from torch's global generator, the draw is a fixed function of (seed, model_id, position): the
    same position gets the same answer in every batch, every call and every process, on the CPU and on the GPU."""
    kind = "random"


class UniformPlayer(_BuiltinPlayer):
    """Player that answers seven equal logits and q = 0 (tournament.py:67-77), named "uniform"."""
    kind = "uniform"

    def __init__(self, model_id: int):
        super().__init__(model_id, 0)


def _has_four(x: np.ndarray) -> np.ndarray:
    """results._has_four for uint64 arrays."""
    s = np.uint64
    start = s(_START03)
    h = x & (x >> s(1)) & (x >> s(2)) & (x >> s(3)) & start
    v = x & (x >> s(7)) & (x >> s(14)) & (x >> s(21))
    d1 = x & (x >> s(8)) & (x >> s(16)) & (x >> s(24)) & start
    d2 = (x >> s(3)) & (x >> s(9)) & (x >> s(15)) & (x >> s(21)) & start
    return (h | v | d1 | d2) != 0


def player0_scores(games: PlayGamesResult) -> Tuple[np.ndarray, np.ndarray]:
    """(ids uint64[n, 3], score float64[n]): `GameResult.player0_score()` (types.rs:77-99) of every game, from the packed
    records -- no Sample is built.  The first terminal sample decides: the side to move there has won (1), lost (0) or drawn
    (0.5), and it is player 1's view when the number of stones is odd."""
    ids, recs, counts = games._tables()
    n = len(counts)
    if n == 0:
        return ids, np.zeros(0, dtype=np.float64)
    mask, value = np.ascontiguousarray(recs["mask"]), np.ascontiguousarray(recs["value"])
    stones = np.unpackbits(mask.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1, dtype=np.int64)
    win, loss = _has_four(mask & value), _has_four(mask & ~value)
    term = win | loss | (stones == 42)
    game_of = np.repeat(np.arange(n, dtype=np.int64), counts.astype(np.int64))
    at = np.flatnonzero(term)
    decided, where = np.unique(game_of[at], return_index=True)         # (at ascends: the first occurrence is a game's first terminal sample)
    if len(decided) != n:
        raise RuntimeError("player0_score called on an unfinished game")   # reference panics
    first = at[where]
    side = np.where(win[first], 1.0, np.where(loss[first], 0.0, 0.5))
    return ids, np.where(stones[first] % 2 == 1, 1.0 - side, side)


@dataclass
class TournamentResult:
    """The results of a tournament (tournament.py:80-109)."""
    model_ids: List[int]
    date: datetime = field(default_factory=datetime.now)
    games: Optional[PlayGamesResult] = None

    def _scores(self):
        assert self.games is not None, "tournament has not been played"
        return player0_scores(self.games)

    def get_scores(self) -> List[Tuple[int, float]]:
        """[(model_id, score)], best first; equal scores in the order the players first appear in the games (player 0 before
        player 1 of a game): the reference's dict of sums, stably sorted."""
        ids, s0 = self._scores()
        who = ids[:, 1:3].reshape(-1)                                 # player0, player1 of game 0, of game 1, ...
        pts = np.stack([s0, 1.0 - s0], axis=1).reshape(-1)
        uniq, first_seen, inv = np.unique(who, return_index=True, return_inverse=True)
        total = np.zeros(len(uniq), dtype=np.float64)
        np.add.at(total, inv.reshape(-1), pts)                         # (multiples of 0.5: exact in any order)
        ret = [(int(uniq[i]), float(total[i])) for i in np.argsort(first_seen, kind="stable")]
        ret.sort(key=lambda x: x[1], reverse=True)
        return ret

    def score_matrix(self) -> np.ndarray:
        """float64 [P, P]: entry [i, j] = the points model_ids[i] took from its games against model_ids[j] (both colours)."""
        ids, s0 = self._scores()
        index = {int(m) & _U64: i for i, m in enumerate(self.model_ids)}
        out = np.zeros((len(self.model_ids), len(self.model_ids)), dtype=np.float64)
        try:
            a = np.array([index[p] for p in ids[:, 1].tolist()], dtype=np.int64)
            b = np.array([index[p] for p in ids[:, 2].tolist()], dtype=np.int64)
        except KeyError as e:
            raise KeyError(f"a game was played by model id {e.args[0]}, which is not in model_ids") from None
        np.add.at(out, (a, b), s0)
        np.add.at(out, (b, a), 1.0 - s0)
        return out

    def scores_table(self, get_name: Callable[[int], str]) -> str:
        """The table the reference prints with tabulate(..., headers=["Player", "Score"], tablefmt="github"), written out here:
        names left-aligned, scores in %g aligned at the decimal point."""
        rows = [(str(get_name(mid)), format(score, "g")) for mid, score in self.get_scores()]
        frac = [len(s) - s.index(".") if "." in s else 0 for _, s in rows]
        nums = [s + " " * (max(frac) - f) for (_, s), f in zip(rows, frac)] if rows else []
        w0 = max([len("Player") + 2] + [len(name) for name, _ in rows])
        w1 = max([len("Score") + 2] + [len(s) for s in nums])
        lines = [f"| {'Player'.ljust(w0)} | {'Score'.rjust(w1)} |", f"|{'-' * (w0 + 2)}|{'-' * (w1 + 2)}|"]
        lines += [f"| {name.ljust(w0)} | {s.rjust(w1)} |" for (name, _), s in zip(rows, nums)]
        return "\n".join(lines)

    def get_top_models(self) -> List[int]:
        """The model ids in descending order of performance."""
        return [model_id for model_id, _ in self.get_scores()]


def tournament_requests(model_ids: Sequence[int], games_per_match: int) -> List[GameMetadata]:
    """The reference's schedule (tournament.py:127-129): every ordered pair, the list repeated games_per_match / 2 times,
    game_id = the index."""
    if int(games_per_match) % 2 != 0 or int(games_per_match) < 0:
        raise ValueError("games_per_match must be even")
    ids = [int(m) for m in model_ids]
    if len(set(i & _U64 for i in ids)) != len(ids):
        raise ValueError("duplicate model ids")
    pairings = list(itertools.permutations(ids, 2)) * (int(games_per_match) // 2)
    return [GameMetadata(i, p0, p1) for i, (p0, p1) in enumerate(pairings)]


def play_tournament(players: Sequence[Player], games_per_match: int, batch_size: int, mcts_iterations: int, exploration_constant: float,
                    c_ply_penalty: float = 0.01, **play_kwargs) -> TournamentResult:
    """Play a round robin (tournament.py:112-142): every ordered pair of players meets games_per_match / 2 times, so every pair
    plays games_per_match games, half with each colour.  play_kwargs go to `c4a0_amd.play_games` (device, resident_games,
    stats, ...); stats["multi_model"] says which path the job took.

    If every player has a device evaluator (`ModelPlayer`, `RandomPlayer`, `UniformPlayer`) the job is
    `play_games(evaluator={model_id: ...})`: networks of one architecture and the anchors on the grouped path.  If any player
    offers `forward_numpy` only, the whole job goes through the numpy callback, as the reference's does."""
    from .api import play_games

    players = list(players)
    reqs = tournament_requests([p.model_id for p in players], games_per_match)
    by_id = {int(p.model_id): p for p in players}
    tournament = TournamentResult(model_ids=[p.model_id for p in players])
    device = play_kwargs.get("device")
    if device is None:
        device = next((p.device for p in players if getattr(p, "device", None) is not None), None)
    evaluators = {mid: p.device_evaluator(device) for mid, p in by_id.items()}
    if all(ev is not None for ev in evaluators.values()):
        tournament.games = play_games(reqs, batch_size, mcts_iterations, exploration_constant, c_ply_penalty, evaluator=evaluators, **play_kwargs)
    else:
        tournament.games = play_games(reqs, batch_size, mcts_iterations, exploration_constant, c_ply_penalty,
                                      lambda player_id, pos: by_id[int(player_id)].forward_numpy(pos), **play_kwargs)
    return tournament


def gen_players(base_dir: str, device, gens: Optional[Sequence[int]] = None, **inference_kwargs) -> List[ModelPlayer]:
    """`ModelPlayer`s for the generations of a training folder (`TrainingGen.load_all` / `get_model`), model_id = gen_n, oldest
    first; gens: the gen_n values wanted (None: all).  With the anchors, a training run is ranked in two lines:

        players = gen_players(base_dir, "cuda:0") + [RandomPlayer(10**6), UniformPlayer(10**6 + 1)]
        print(play_tournament(players, 20, 2000, 100, 1.4).scores_table(lambda i: {p.model_id: p.name for p in players}[i]))"""
    from .training import TrainingGen

    want = None if gens is None else {int(g) for g in gens}
    found = sorted((g for g in TrainingGen.load_all(base_dir) if want is None or g.gen_n in want), key=lambda g: g.gen_n)
    if want is not None and want - {g.gen_n for g in found}:
        raise FileNotFoundError(f"no generation {sorted(want - {g.gen_n for g in found})} in {base_dir}")
    return [ModelPlayer(g.gen_n, g.get_model(base_dir), device, **inference_kwargs) for g in found]
