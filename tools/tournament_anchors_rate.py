"""How fast is a round robin of networks AND the two anchors?  `play_tournament` of 2 networks + `random` + `uniform` at the size of
tools/tournament_rate.py (8 192 games on 4 096 resident games, n_mcts_iterations = 100, 4-block / 32-channel bf16 networks), twice:

  grouped   the players as they are: the grouped path (device-side router, the networks' grouped chain, one launch of
            c4_builtin_eval_grouped for the anchors' segments, rounds replayed from a HIP graph)
  eager     the same players' evaluators wrapped in plain callables, which `play_games` cannot group: the eager per-model path
            (api._MultiModelEvaluator: a sort, two host reads and one eager chain per player every round) -- unchanged code, the yardstick

Each is played once untimed and then `--runs` times; the median wall time is reported with every run's seconds, and the records of
every run are hashed (sha256 of the CBOR encoding): both paths must give the same bytes.  One JSON document.

    python tools/tournament_anchors_rate.py --out profiles/tournament_anchors.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import c4a0_amd  # noqa: E402
from c4a0_amd.nn import ConnectFourNet, ModelConfig  # noqa: E402
from c4a0_amd.tournament import ModelPlayer, RandomPlayer, UniformPlayer, tournament_requests  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192, help="games per call (rounded down to whole round robins of 12 pairings)")
    ap.add_argument("--resident-games", type=int, default=4096)
    ap.add_argument("--n-mcts", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    players = []
    for i in range(2):
        torch.manual_seed(1337 + i)
        players.append(ModelPlayer(11 + i, ConnectFourNet(ModelConfig(args.blocks, args.channels, 4, 2)), dev, dtype=torch.bfloat16, strict=True))
    players += [RandomPlayer(1000), UniformPlayer(1001)]
    n_pairings = len(players) * (len(players) - 1)
    games_per_match = 2 * (args.games // n_pairings)          # every ordered pair games_per_match / 2 times
    reqs = tournament_requests([p.model_id for p in players], games_per_match)
    evs = {p.model_id: p.device_evaluator(dev) for p in players}
    jobs = {"grouped": evs, "eager": {mid: (lambda planes, ev=ev: ev(planes)) for mid, ev in evs.items()}}
    out = {"config": {"players": [p.name for p in players], "games": len(reqs), "games_per_match": games_per_match, "resident_games": args.resident_games,
                      "n_mcts_iterations": args.n_mcts,
                      "network": f"{args.blocks}-block / {args.channels}-channel ConnectFourNet (4 policy / 2 value layers), bf16", "runs": args.runs,
                      "device": torch.cuda.get_device_name(dev)},
           "variants": {}}
    scores = None
    for name, ev in jobs.items():
        secs, hashes, st = [], [], {}
        for r in range(args.runs + 1):          # the first call is untimed (lazy module loads, LDS opt-ins, the allocator's first blocks)
            st = {}
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = c4a0_amd.play_games(reqs, 2000, args.n_mcts, 1.4, 0.01, evaluator=ev, resident_games=args.resident_games, stats=st)
            dt = time.perf_counter() - t0
            if r:
                secs.append(dt)
            hashes.append(hashlib.sha256(res.to_cbor()).hexdigest())
        assert len(set(hashes)) == 1, f"{name}: the runs' records differ"
        med = statistics.median(secs)
        out["variants"][name] = {"seconds_median": med, "seconds": secs, "games_per_s": len(reqs) / med, "sims_per_s": st["sims"] / med, "rounds": st["steps"],
                                 "path": st.get("multi_model"), "reason": st.get("multi_model_reason"),
                                 "graph_captures": st.get("phases", {}).get("graph_captures"), "records_sha256": hashes[0], "samples": st["samples"]}
        print(name, json.dumps(out["variants"][name]), file=sys.stderr, flush=True)
        t = c4a0_amd.TournamentResult(model_ids=[p.model_id for p in players], games=res)
        scores = [(next(p.name for p in players if p.model_id == mid), s) for mid, s in t.get_scores()]
    v = out["variants"]
    out["grouped_over_eager"] = v["eager"]["seconds_median"] / v["grouped"]["seconds_median"]
    out["records_identical"] = v["grouped"]["records_sha256"] == v["eager"]["records_sha256"]
    out["scores"] = scores        # (untrained networks: says nothing about strength, only that the table adds up)
    doc = json.dumps(out, indent=1)
    print(doc)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
