"""What the exact solver (c4a0_amd.Solver) does per second, and what it solves -> profiles/solver_rate.json.

    python tools/solver_rate.py [out.json] [--quick]

(a) Rate.  18 000 distinct positions with 12..16 stones from seeded random playouts give about as many tasks as the chip has lanes
    (2 048 workgroups x 64; never more, so one launch reaches them all), most of them far larger than a launch budget.  For nodes_per_launch B in a sweep, and then at the library's
    default, one call with max_nodes_per_position = B: every lane spends its whole budget once, tasks are given up after their
    first launch, so wall time / launches is the time of one full launch of budget B and nodes / wall the chip's rate.  A second
    pass with only 64 tasks (one wavefront) gives the rate of a lane that has the machine to itself.  Wall-clock around the call
    (it ends with the stream synchronised; the host's share -- folding mirrors, building tasks, two copies -- is inside), median of 3.
(b) Reach.  The samples of one small play_games job (hash evaluator, 64 games, 12 simulations per move), grouped by stone count:
    per group the solved fraction and the wall time under the default budgets, one Solver (default table) for the lot, from
    the most stones down so that the table helps as it would in use.  --quick caps (b) at 2^14 visits per child.
Speed is recorded here, never asserted in a test."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import c4a0_amd  # noqa: E402
from c4a0_amd import _lib  # noqa: E402
from c4a0_amd.solver import is_terminal, stone_counts  # noqa: E402
from helpers import hash_eval_torch  # noqa: E402
from solver_ref import playout_positions  # noqa: E402

LANES = 2048 * 64


def header_default(name):
    import re

    text = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    expr = re.search(r"#define %s\s+\(?([^/\n]*?)\)?\s*(?:/\*|$)" % name, text, flags=re.M).group(1)
    return int(eval(expr.replace("ull", "")))


def one_launch_budget(solver, pos, budget, repeats=3):
    walls, last = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = solver.solve(pos, nodes_per_launch=budget, max_nodes_per_position=budget)
        walls.append(time.perf_counter() - t0)
    wall = statistics.median(walls)
    st = last.stats
    lanes = min(st["tasks"], LANES)
    return {"nodes_per_launch": budget, "tasks": st["tasks"], "launches": st["launches"], "nodes": st["nodes"], "probes": st["probes"],
            "wall_s": wall, "wall_s_all": walls, "launch_ms": 1e3 * wall / max(1, st["launches"]),
            "nodes_per_s_chip": st["nodes"] / wall, "probes_per_s_chip": st["probes"] / wall,
            "nodes_per_s_lane": st["nodes"] / wall / lanes, "lanes_busy": lanes}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    quick = "--quick" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "solver_rate.json")
    default_npl = header_default("C4_SOLVER_NODES_PER_LAUNCH")
    default_cap = header_default("C4_SOLVER_MAX_NODES_PER_POSITION")
    res = {"device": torch.cuda.get_device_name(0), "defaults": {"nodes_per_launch": default_npl, "max_nodes_per_position": default_cap,
                                                                  "tt_entries": _lib.SOLVER_TT_ENTRIES}}
    # ---- (a)
    pos = playout_positions(1, 18000, 12, 16)
    rate = {"positions": len(pos), "stones": "12..16", "full_chip": [], "one_wavefront": []}
    with c4a0_amd.Solver() as solver:
        solver.solve(pos[:256], nodes_per_launch=256, max_nodes_per_position=256)          # warm-up: the kernel is loaded
        for b in sorted({1024, 4096, 16384, default_npl}):
            rate["full_chip"].append(one_launch_budget(solver, pos, b))
            print("full chip", rate["full_chip"][-1], flush=True)
        for b in sorted({4096, default_npl}):
            rate["one_wavefront"].append(one_launch_budget(solver, pos[:14], b))
            print("one wavefront", rate["one_wavefront"][-1], flush=True)
    at_default = [r for r in rate["full_chip"] if r["nodes_per_launch"] == default_npl][0]
    rate["launch_ms_at_default_nodes_per_launch"] = at_default["launch_ms"]
    rate["nodes_per_launch_for_50_ms"] = int(default_npl * 50.0 / at_default["launch_ms"])
    res["rate"] = rate
    # ---- (b)
    games = c4a0_amd.play_games([c4a0_amd.GameMetadata(i, 0, 0) for i in range(64)], 64, 12, 6.6, 0.01, evaluator=hash_eval_torch)
    recs, _ = games.to_records()
    live = ~is_terminal(recs["mask"], recs["value"])
    stones = stone_counts(recs["mask"])
    budget = {"max_nodes_per_position": 1 << 14} if quick else {}
    reach = {"job": "play_games, 64 games, hash evaluator, 12 simulations per move", "non_terminal_samples": int(live.sum()),
             "budget": budget or "defaults", "by_stones": []}
    with c4a0_amd.Solver() as solver:
        for s in sorted(set(stones[live].tolist()), reverse=True):
            pick = live & (stones == s)
            p = np.stack([recs["mask"][pick], recs["value"][pick]], axis=1)
            t0 = time.perf_counter()
            r = solver.solve(p, **budget)
            wall = time.perf_counter() - t0
            row = {"stones": int(s), "samples": int(pick.sum()), "unique_positions": r.stats["unique_positions"], "solved": int(r.solved.sum()),
                   "solved_fraction": float(r.solved.mean()), "wall_s": wall, "nodes": r.stats["nodes"], "launches": r.stats["launches"],
                   "tasks": r.stats["tasks"], "unsolved_tasks": r.stats["unsolved_tasks"]}
            reach["by_stones"].append(row)
            print(row, flush=True)
        t0 = time.perf_counter()
        score = games.solver_score(solver, **budget)
        reach["solver_score_after"] = dict(score._asdict(), wall_s=time.perf_counter() - t0)
    res["reach"] = reach
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
