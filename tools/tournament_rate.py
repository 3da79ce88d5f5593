"""How fast are games between different networks?  Whole `play_games(evaluator={model_id: net})` calls at BASELINE config 2's shape
(4 096 resident games, n_mcts_iterations = 100, 4-block / 32-channel bf16 network), in four variants:

  grouped_2 / grouped_8   2 models (both colours) / 8 models (round robin) on the grouped path: device-side router, grouped bf16
                          chain, rounds replayed from a HIP graph (api._GroupedModelEvaluator)
  eager_2 / eager_8       the same two jobs on the eager per-model path (api._MultiModelEvaluator): the same networks wrapped in plain
                          callables, which is what `play_games` cannot stack
  selfplay                single-model self-play of the same size (the library's own loop), for the ratio

Every variant is played once untimed and then `--runs` times; the median is reported with every run's seconds, and the records of
every run are hashed (sha256 of the CBOR encoding): the grouped and the eager path must give the same bytes.  One JSON document.

    python tools/tournament_rate.py --out profiles/tournament_rate.json
"""
import argparse
import hashlib
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import c4a0_amd  # noqa: E402
from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192, help="games per call (two generations of the resident games)")
    ap.add_argument("--resident-games", type=int, default=4096)
    ap.add_argument("--n-mcts", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--variants", default="grouped_2,grouped_8,eager_2,eager_8,selfplay")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    nets = {}
    for i in range(8):
        torch.manual_seed(1337 + i)
        nets[11 + i] = InferenceNet(ConnectFourNet(ModelConfig(args.blocks, args.channels, 4, 2)), dev, dtype=torch.bfloat16, strict=True)
    ids = list(nets)

    def reqs_for(k):
        pairs = list(itertools.permutations(ids[:k], 2)) if k > 1 else [(ids[0], ids[0])]
        return [c4a0_amd.GameMetadata(i, *pairs[i % len(pairs)]) for i in range(args.games)]

    def job(name):
        if name == "selfplay":
            return reqs_for(1), nets[ids[0]]
        kind, k = name.split("_")
        sub = {m: nets[m] for m in ids[: int(k)]}
        if kind == "eager":
            sub = {m: (lambda planes, net=net: net(planes)) for m, net in sub.items()}
        return reqs_for(int(k)), sub

    out = {"config": {"games": args.games, "resident_games": args.resident_games, "n_mcts_iterations": args.n_mcts,
                      "network": f"{args.blocks}-block / {args.channels}-channel ConnectFourNet (4 policy / 2 value layers), bf16", "runs": args.runs,
                      "device": torch.cuda.get_device_name(dev)},
           "variants": {}}
    for name in args.variants.split(","):
        reqs, ev = job(name)
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
        out["variants"][name] = {"seconds_median": med, "seconds": secs, "games_per_s": args.games / med, "sims_per_s": st["sims"] / med,
                                 "rounds": st["steps"], "path": st.get("multi_model", st.get("host_loop")), "reason": st.get("multi_model_reason"),
                                 "graph_captures": st.get("phases", {}).get("graph_captures"), "records_sha256": hashes[0], "samples": st["samples"]}
        print(name, json.dumps(out["variants"][name]), file=sys.stderr, flush=True)
    v = out["variants"]
    for k in ("2", "8"):
        if f"grouped_{k}" in v and f"eager_{k}" in v:
            out[f"grouped_over_eager_{k}"] = v[f"eager_{k}"]["seconds_median"] / v[f"grouped_{k}"]["seconds_median"]
            out[f"records_identical_{k}"] = v[f"grouped_{k}"]["records_sha256"] == v[f"eager_{k}"]["records_sha256"]
        if f"grouped_{k}" in v and "selfplay" in v:
            out[f"grouped_{k}_rate_over_selfplay"] = v[f"grouped_{k}"]["games_per_s"] / v["selfplay"]["games_per_s"]
    doc = json.dumps(out, indent=1)
    print(doc)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
