#!/usr/bin/env python3
"""A turn against an outside opponent, done two ways from the same positions, evaluator and n:

  engine   `Engine.make_moves` + `Engine.search`: the tree under the move is kept, the session, its arena and its graph live on;
  fresh    one `search_positions` call on the moved positions: a fresh tree and a fresh job per turn (what the parent of the
           engine could already do: the baseline).

    python tools/engine_turns.py P N [--turns 3] [--blocks 4] [--channels 32] [--plies 8]

P games start from random positions `--plies` plies into a game and are searched to N visits (untimed); then, `--turns` times, every
game makes the best move of its root policy and is searched to N visits again.  One JSON line: per turn the seconds of both ways
(engine = make_moves + search), the lock-step rounds, and the share of the N visits the move kept."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_positions(n, plies, seed=1337):
    """n non-terminal positions `plies` random legal moves from the empty board, as (mask, value) of the side to move"""
    from c4a0_amd.results import terminal_state

    rng, out = random.Random(seed), []
    while len(out) < n:
        mask = value = 0
        for _ in range(plies):
            col = rng.choice([c for c in range(7) if not (mask >> (35 + c)) & 1])
            row = next(r for r in range(6) if not (mask >> (7 * r + col)) & 1)
            value, mask = mask & ~value, mask | (1 << (7 * row + col))     # the mover's stone joins; the view passes to the opponent
            if terminal_state(mask, value):
                break
        else:
            out.append((mask, value))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("p", type=int)
    ap.add_argument("n", type=int)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--plies", type=int, default=8)
    a = ap.parse_args()
    import c4a0_amd
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    dev = torch.device("cuda:0")
    torch.manual_seed(1337)
    net = InferenceNet(ConnectFourNet(ModelConfig(a.blocks, a.channels, 4, 2)), dev, dtype=torch.bfloat16)
    positions = random_positions(a.p, a.plies)
    c4a0_amd.search_positions(positions[:64], 20, 6.6, 0.01, evaluator=net)     # untimed: code objects, LDS opt-ins
    # (the arena: a root takes at most n blocks; the start and every turn have one root each)
    eng = c4a0_amd.Engine(net, a.n, 6.6, 0.01, positions=positions, device=dev, blocks_per_slot=min(65535, a.n * (a.turns + 1) + 8))
    eng.search()
    turns = []
    for _ in range(a.turns):
        snap = eng.snapshot()
        cols = np.where(snap.terminal, -1, np.argmax(snap.records["policy"], axis=1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        made = eng.make_moves(cols)
        t_move = time.perf_counter() - t0
        moved = eng.snapshot()                                               # (untimed: only this tool wants the visits kept)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rounds = eng.search()
        torch.cuda.synchronize()
        t_search = time.perf_counter() - t0
        live = made & ~moved.terminal
        st = {}
        t0 = time.perf_counter()
        fresh = c4a0_amd.search_positions(np.stack([moved.records["mask"], moved.records["value"]], axis=1), a.n, 6.6, 0.01, evaluator=net, stats=st)
        t_fresh = time.perf_counter() - t0
        after = eng.snapshot()
        same = bool(np.array_equal(np.argmax(after.records["policy"][live], axis=1), np.argmax(fresh.policy[live], axis=1)))
        turns.append({"engine_s": round(t_move + t_search, 5), "make_moves_s": round(t_move, 5), "search_s": round(t_search, 5), "engine_rounds": rounds,
                      "fresh_s": round(t_fresh, 5), "fresh_rounds": st["steps"], "moves": int(made.sum()), "games_live": int(live.sum()),
                      "visits_kept_share": round(float(moved.visits[live].mean()) / a.n, 4) if live.any() else None,
                      "same_best_move_both_ways": same})
    eng.close()
    print(json.dumps({"tool": "engine_turns", "P": a.p, "n": a.n, "net": f"{a.blocks}x{a.channels}", "start_plies": a.plies, "turns": turns}), flush=True)


if __name__ == "__main__":
    main()
