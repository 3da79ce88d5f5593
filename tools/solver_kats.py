"""The reference's three solver known-answer tests (rust/src/solver.rs:271-306) on the GPU solver, under the DEFAULT budgets, with
no opening book -> profiles/solver_kats.json.

    python tools/solver_kats.py [out.json]

Per KAT: the score row and whether one-hot policies score as the reference expects -- or "unsolved within budget", with the nodes and
seconds spent.  A run ends by the budget (max_nodes_per_position), never by a time limit.  Run once; not part of pytest."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import c4a0_amd  # noqa: E402
from c4a0_amd.solver import score_rows  # noqa: E402
from solver_ref import from_moves  # noqa: E402

KATS = [("default_pos", [], [0, 0, 0, 1, 0, 0, 0]),
        ("p0_winning_pos", [2, 2, 3, 3], [0, 1, .5, .5, 1, 0, 0]),
        ("p1_winning_pos", [0], [0, 1, .5, 1, 0, .5, 0])]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "solver_kats.json")
    res = []
    with c4a0_amd.Solver() as solver:
        for name, moves, expected in KATS:
            pos = [from_moves(moves)]
            t0 = time.perf_counter()
            r = solver.solve(pos)
            wall = time.perf_counter() - t0
            row = {"kat": name, "moves": moves, "expected": expected, "seconds": wall, "nodes": r.stats["nodes"], "probes": r.stats["probes"],
                   "launches": r.stats["launches"], "tasks": r.stats["tasks"], "unsolved_tasks": r.stats["unsolved_tasks"]}
            if r.solved[0]:
                got = score_rows(np.tile(r.scores, (7, 1)), np.eye(7, dtype=np.float32)).tolist()
                row.update(outcome="match" if got == expected else "MISMATCH", scores=r.scores[0].tolist(), got=got)
            else:
                row.update(outcome="unsolved within budget")
            res.append(row)
            print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
