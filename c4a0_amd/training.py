"""Generation-based training: self-play on the GPU, then one network trained from the games (reference src/c4a0/training.py and
the training half of src/c4a0/nn.py) -- without Lightning, pydantic or torchmetrics.

`train_single_gen` plays a generation's games with the parent network (`c4a0_amd.play_games`), optionally scores them against the
GPU solver, splits them exactly as the reference does (`dataset.split_train_test_tensors`), trains a copy of the parent (`fit`) and
writes the generation's folder.  A generation's folder holds `metadata.json` (the reference's keys, readable by its
`TrainingGen.model_validate_json`), `games.pkl` (the `PlayGamesResult` pickle) and -- where the reference pickles a Lightning module --
`model.pt` (the `state_dict`, whose keys are the reference's) with `model.json` (`ModelConfig` and `TrainConfig`).
"""
from __future__ import annotations

import copy
import dataclasses
import json
import math
import os
import pickle
from dataclasses import dataclass, field
from datetime import datetime
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import train_graph
from .nn import ConnectFourNet, ModelConfig
from .train_common import EPS, loss  # noqa: F401  (`training.loss` and `training.EPS` are public)
from .train_heads import loss_train, resolve_heads  # noqa: F401  (`training.loss_train` is public)
from .train_out import resolve_outputs
from .train_tower import resolve_tower


@dataclass
class TrainConfig:
    """The training-only fields of the reference's ModelConfig (nn.py:31-38)."""
    lr_schedule: Dict[int, float] = field(default_factory=lambda: {0: 2e-3})   # gen_n from which a learning rate holds -> the rate
    l2_reg: float = 4e-4                                                       # Adam's weight_decay (coupled L2)


def parse_lr_schedule(floats: Sequence[float]) -> Dict[int, float]:
    """A sequence like `0 2e-3 10 8e-4` as {0: 2e-3, 10: 8e-4} (training.py:349-360)."""
    assert len(floats) % 2 == 0, "lr_schedule must have an even number of elements"
    schedule = {}
    for i in range(0, len(floats), 2):
        threshold = int(floats[i])
        assert threshold == floats[i], "lr_schedule must alternate between gen_id (int) and lr (float)"
        schedule[threshold] = floats[i + 1]
    return schedule


def lr_for_gen(lr_schedule: Dict[int, float], gen_n: int) -> float:
    """nn.py:143-148: the first entry's rate, replaced by every later entry whose threshold gen_n has reached."""
    schedule = sorted((int(k), float(v)) for k, v in lr_schedule.items())
    _, lr = schedule.pop(0)
    for gen_threshold, gen_rate in schedule:
        if gen_n < gen_threshold:
            break
        lr = gen_rate
    return lr


def evaluate_loss(model, data, batch_size: int) -> float:
    """The sample mean of `loss` over `data` in eval mode (what Lightning's batch-size-weighted epoch mean of val_loss equals).  The
    sum is kept in float64 on the data's device and read once: one synchronisation a pass, not one a batch.  The model's mode is
    restored."""
    was_training = model.training
    model.eval()
    n = data[0].shape[0]
    total = torch.zeros((), dtype=torch.float64, device=data[0].device)
    with torch.no_grad():
        for i in range(0, n, batch_size):
            b = tuple(t[i:i + batch_size] for t in data)
            total += loss(model(b[0]), b)[0].double() * b[0].shape[0]
    model.train(was_training)
    return float(total) / n


def fit(model, train, val, batch_size: int, gen_n: int, cfg: TrainConfig, seed: int = 1337, heads: str = "auto", max_epochs: int = 100,
        patience: int = 10, val_loss_fn: Optional[Callable] = None, optimizer: str = "auto", graph: bool = False, tower: str = "auto",
        outputs: str = "auto"):
    """Train `model` in place on `train`, watching `val` (both tuples (pos, policy, q_penalty, q_no_penalty) of tensors on the
    model's device), as the reference's `trainer.fit` does (training.py:206-225):

    * Adam(lr = lr_for_gen(cfg.lr_schedule, gen_n), weight_decay = cfg.l2_reg): coupled L2, default betas and eps (nn.py:140-152).
    * Every epoch draws a fresh `torch.randperm` from a generator seeded once by `seed`; the last partial batch is kept.  A trailing
      batch of exactly ONE sample is skipped: BatchNorm in train mode cannot take it (the reference would raise there).
    * Steps run in train mode as `train_graph.train_step` on the paths `heads`, `tower` and `outputs` resolve to, once, before the first epoch;
      after every epoch val_loss is the sample mean of `loss` over the whole of `val` in eval mode (`val_loss_fn(model, val,
      batch_size)` if given, else `evaluate_loss`).
    * A deep copy of the model with the strictly lowest val_loss is kept (utils.py:79-82).  Training stops after `patience`
      consecutive epochs without a strictly lower val_loss (Lightning's EarlyStopping(patience, min_delta=0): a tie is no
      improvement) or after `max_epochs` epochs.  max_epochs = 100 and patience = 10 are the values the reference hard-codes.

    optimizer: "torch" is `torch.optim.Adam`; "hip" is `train_graph.HipAdam`, the same update as one launch with its state and step
    count on the device; "auto" is "torch" without a graph and "hip" with one.  graph=True (opt-in; an f32 model on a HIP device and
    optimizer "hip", else ValueError) captures one whole step per batch shape -- the full batch and the epoch's last partial one -- as a
    HIP graph and replays it (`train_graph.GraphedSteps`); without it the steps run eagerly (`train_graph.EagerSteps`).
    History and return values mean the same on every path.

    tower: `forward_train`'s -- "torch" (the stock convolutions), "hip" (opt-in: the tower forward and backward on the deterministic
    kernels of `train_tower`; with heads="hip" and optimizer="hip" a fit then repeats itself byte for byte, eagerly and from the graph)
    or "auto" (`train_tower.AUTO_TOWER`: "torch").

    outputs: `loss_train`'s -- "torch" (the stock output layers, log-softmax, tanh and `loss`, with their autograd), "hip" (opt-in: all of
    that as one forward and one backward call of `train_out`'s deterministic kernels) or "auto" (`train_out.AUTO_OUTPUTS`: "torch").

    Returns (best_model, best_val_loss, history), history = one dict per epoch: epoch, train_loss (the sample mean of the steps'
    losses), val_loss, lr, steps."""
    optimizer = train_graph.resolve_optimizer(optimizer, graph)
    if optimizer == "hip":
        why = train_graph.graph_refusal(model)
        if why is not None:
            raise ValueError(("graph=True" if graph else 'optimizer="hip"') + f": {why}")
    val_loss_fn = val_loss_fn or evaluate_loss
    lr = lr_for_gen(cfg.lr_schedule, gen_n)
    dev = train[0].device
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    n = train[0].shape[0]
    model.train()
    path = resolve_heads(model, heads, train[0])
    tower_path = resolve_tower(model, tower, train[0])
    outputs_path = resolve_outputs(model, outputs, train[0])
    if optimizer == "hip":   # looked up at call time: the tests put a recording subclass there
        opt = train_graph.HipAdam(model.parameters(), lr=lr, weight_decay=cfg.l2_reg)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=cfg.l2_reg)
    try:
        steps = (train_graph.GraphedSteps if graph else train_graph.EagerSteps)(model, opt, path, train, tower_path, outputs_path)
        best_model, best_val, since_best, history = None, math.inf, 0, []
        for epoch in range(max_epochs):
            model.train()
            perm = torch.randperm(n, generator=gen).to(dev)
            steps.reset()
            seen = n_steps = 0
            for i in range(0, n, batch_size):
                idx = perm[i:i + batch_size]
                if idx.shape[0] < 2:
                    continue
                steps.run(idx)
                seen += idx.shape[0]
                n_steps += 1
            train_loss = float(steps.total) / max(seen, 1)
            val_loss = float(val_loss_fn(model, val, batch_size))
            history.append({"epoch": epoch, "train_loss": train_loss, "val_loss": val_loss, "lr": lr, "steps": n_steps})
            if val_loss < best_val:
                best_model, best_val, since_best = copy.deepcopy(model), val_loss, 0
            else:
                since_best += 1
                if since_best >= patience:
                    break
        if best_model is None:   # no epoch, or no finite val_loss: the model as it is
            best_model = copy.deepcopy(model)
        return best_model, best_val, history
    finally:
        if optimizer == "hip":
            opt.release()   # also when a step, a capture or val_loss_fn raises: the model does not keep gradients a dead table points at


# metadata.json: the reference's fields (training.py:30-39), then what this package adds
REFERENCE_KEYS = ("created_at", "gen_n", "n_mcts_iterations", "c_exploration", "c_ply_penalty", "self_play_batch_size", "training_batch_size",
                  "parent", "val_loss", "solver_score")
EXTRA_KEYS = ("solver_n_scored", "solver_n_unsolved", "solver_n_skipped")


@dataclass
class TrainingGen:
    """A single generation of training (training.py:25-146)."""
    created_at: datetime
    gen_n: int
    n_mcts_iterations: int
    c_exploration: float
    c_ply_penalty: float
    self_play_batch_size: int
    training_batch_size: int
    parent: Optional[datetime] = None
    val_loss: Optional[float] = None
    solver_score: Optional[float] = None
    solver_n_scored: Optional[int] = None
    solver_n_unsolved: Optional[int] = None
    solver_n_skipped: Optional[int] = None

    @staticmethod
    def _gen_folder(created_at: datetime, base_dir: str) -> str:
        return os.path.join(base_dir, created_at.isoformat())

    def gen_folder(self, base_dir: str) -> str:
        return TrainingGen._gen_folder(self.created_at, base_dir)

    def to_json(self) -> str:
        d = dataclasses.asdict(self)
        for k in ("created_at", "parent"):
            d[k] = d[k].isoformat() if d[k] is not None else None
        return json.dumps(d, indent=2)

    @staticmethod
    def from_json(text: str) -> "TrainingGen":
        d = json.loads(text)
        d = {k: d.get(k) for k in REFERENCE_KEYS + EXTRA_KEYS if k in d}
        for k in ("created_at", "parent"):
            if d.get(k) is not None:
                d[k] = datetime.fromisoformat(d[k])
        return TrainingGen(**d)

    def save_metadata(self, base_dir: str):
        gen_dir = self.gen_folder(base_dir)
        os.makedirs(gen_dir, exist_ok=True)
        with open(os.path.join(gen_dir, "metadata.json"), "w") as f:
            f.write(self.to_json())

    def save_all(self, base_dir: str, games, model: ConnectFourNet, train_config: Optional[TrainConfig] = None):
        """metadata.json, games.pkl and the model: model.pt (`state_dict` on the CPU) + model.json (ModelConfig, TrainConfig)."""
        self.save_metadata(base_dir)
        gen_dir = self.gen_folder(base_dir)
        with open(os.path.join(gen_dir, "games.pkl"), "wb") as f:
            pickle.dump(games, f)
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(gen_dir, "model.pt"))
        tc = train_config if train_config is not None else TrainConfig()
        with open(os.path.join(gen_dir, "model.json"), "w") as f:
            json.dump({"model_config": dataclasses.asdict(model.config),
                       "train_config": {"lr_schedule": {str(k): v for k, v in tc.lr_schedule.items()}, "l2_reg": tc.l2_reg}}, f, indent=2)

    @staticmethod
    def load(base_dir: str, created_at: datetime) -> "TrainingGen":
        with open(os.path.join(TrainingGen._gen_folder(created_at, base_dir), "metadata.json"), "r") as f:
            return TrainingGen.from_json(f.read())

    @staticmethod
    def _timestamps(base_dir: str) -> List[datetime]:
        return sorted([datetime.fromisoformat(f) for f in os.listdir(base_dir) if os.path.isdir(os.path.join(base_dir, f))], reverse=True)

    @staticmethod
    def load_all(base_dir: str) -> List["TrainingGen"]:
        return [TrainingGen.load(base_dir, t) for t in TrainingGen._timestamps(base_dir)]

    @staticmethod
    def load_latest(base_dir: str) -> "TrainingGen":
        timestamps = TrainingGen._timestamps(base_dir) if os.path.isdir(base_dir) else []
        if not timestamps:
            raise FileNotFoundError("No existing generations")
        return TrainingGen.load(base_dir, timestamps[0])

    @staticmethod
    def load_latest_with_default(base_dir: str, n_mcts_iterations: int, c_exploration: float, c_ply_penalty: float, self_play_batch_size: int,
                                 training_batch_size: int, model_config: ModelConfig, train_config: Optional[TrainConfig] = None) -> "TrainingGen":
        """The latest generation of base_dir; where there is none, generation 0 is created: a freshly initialised network, no games."""
        try:
            return TrainingGen.load_latest(base_dir)
        except FileNotFoundError:
            gen = TrainingGen(created_at=datetime.now(), gen_n=0, n_mcts_iterations=n_mcts_iterations, c_exploration=c_exploration,
                              c_ply_penalty=c_ply_penalty, self_play_batch_size=self_play_batch_size, training_batch_size=training_batch_size)
            gen.save_all(base_dir, None, ConnectFourNet(model_config), train_config)
            return gen

    def get_games(self, base_dir: str):
        with open(os.path.join(self.gen_folder(base_dir), "games.pkl"), "rb") as f:
            return pickle.load(f)

    def get_train_config(self, base_dir: str) -> TrainConfig:
        with open(os.path.join(self.gen_folder(base_dir), "model.json"), "r") as f:
            tc = json.load(f)["train_config"]
        return TrainConfig({int(k): float(v) for k, v in tc["lr_schedule"].items()}, float(tc["l2_reg"]))

    def get_model(self, base_dir: str) -> ConnectFourNet:
        """This generation's network (on the CPU, in eval mode)."""
        gen_dir = self.gen_folder(base_dir)
        with open(os.path.join(gen_dir, "model.json"), "r") as f:
            model = ConnectFourNet(ModelConfig(**json.load(f)["model_config"]))
        model.load_state_dict(torch.load(os.path.join(gen_dir, "model.pt"), map_location="cpu"))
        return model.eval()


def generation_tensors(games, device=None):
    """The (train, validation) tensors a generation is trained on: `games.split_train_test(0.8, 1337)` (training.py:207), each side
    followed by the mirror images of its samples (`SampleDataModule`, training.py:317-318), as tensors on `device`."""
    from .dataset import split_train_test_tensors

    return split_train_test_tensors(games, 0.8, 1337, device)


def train_single_gen(base_dir: str, device, parent: TrainingGen, n_self_play_games: int, n_mcts_iterations: int, c_exploration: float,
                     c_ply_penalty: float, self_play_batch_size: int, training_batch_size: int, solver=None, heads: str = "auto", seed: int = 1337,
                     max_epochs: int = 100, patience: int = 10, timings: Optional[dict] = None, optimizer: str = "auto", graph: bool = False,
                     tower: str = "auto", outputs: str = "auto", **play_kwargs) -> TrainingGen:
    """Train a new generation from `parent` (training.py:155-239): self-play with the parent's network, optionally the games'
    `solver_score(solver)`, the reference's train / validation split with mirror images, `fit` on a copy of the parent, and the new
    generation's folder.  solver: a `c4a0_amd.Solver` (None: no scoring).  play_kwargs go to `c4a0_amd.play_games`
    (resident_games, dirichlet, ...).  timings (a dict) receives the wall seconds of play / split / train.  optimizer, graph,
    tower and outputs are `fit`'s."""
    import time

    from . import GameMetadata
    from .api import play_games
    from .nn import InferenceNet

    device = torch.device(device)
    t0 = time.perf_counter()
    model = parent.get_model(base_dir).to(device)
    train_config = parent.get_train_config(base_dir)
    reqs = [GameMetadata(i, 0, 0) for i in range(n_self_play_games)]
    games = play_games(reqs, self_play_batch_size, n_mcts_iterations, c_exploration, c_ply_penalty, evaluator=InferenceNet(model, device),
                       **play_kwargs)
    score = games.solver_score(solver) if solver is not None else None
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    train, val = generation_tensors(games, device)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    best_model, best_val, _history = fit(copy.deepcopy(model), train, val, training_batch_size, parent.gen_n + 1, train_config, seed=seed,
                                         heads=heads, max_epochs=max_epochs, patience=patience, optimizer=optimizer, graph=graph, tower=tower,
                                         outputs=outputs)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(play_s=t1 - t0, split_s=t2 - t1, train_s=t3 - t2, epochs=len(_history), train_samples=int(train[0].shape[0]),
                       val_samples=int(val[0].shape[0]))
    gen = TrainingGen(created_at=datetime.now(), gen_n=parent.gen_n + 1, n_mcts_iterations=n_mcts_iterations, c_exploration=c_exploration,
                      c_ply_penalty=c_ply_penalty, self_play_batch_size=self_play_batch_size, training_batch_size=training_batch_size,
                      parent=parent.created_at, val_loss=best_val if math.isfinite(best_val) else None,
                      solver_score=score.score if score is not None else None,
                      solver_n_scored=score.n_scored if score is not None else None,
                      solver_n_unsolved=score.n_unsolved if score is not None else None,
                      solver_n_skipped=score.n_skipped if score is not None else None)
    gen.save_all(base_dir, games, best_model, train_config)
    return gen


def training_loop(base_dir: str, device, n_self_play_games: int, n_mcts_iterations: int, c_exploration: float, c_ply_penalty: float,
                  self_play_batch_size: int, training_batch_size: int, model_config: ModelConfig, max_gens: Optional[int] = None, solver=None,
                  train_config: Optional[TrainConfig] = None, heads: str = "auto", tower: str = "auto", outputs: str = "auto",
                  **kwargs) -> TrainingGen:
    """Generation after generation (training.py:242-294) from the latest one of base_dir (generation 0 is created where there is
    none, with `model_config` and `train_config`), until gen_n reaches max_gens (None: for ever)."""
    gen = TrainingGen.load_latest_with_default(base_dir, n_mcts_iterations, c_exploration, c_ply_penalty, self_play_batch_size,
                                               training_batch_size, model_config, train_config)
    while True:
        gen = train_single_gen(base_dir, device, gen, n_self_play_games, n_mcts_iterations, c_exploration, c_ply_penalty, self_play_batch_size,
                               training_batch_size, solver=solver, heads=heads, tower=tower, outputs=outputs, **kwargs)
        if max_gens is not None and gen.gen_n >= max_gens:
            return gen
