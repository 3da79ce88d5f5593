"""How far down the stone counts the exact solver reaches with splitting and a book, and without -> profiles/solver_split_reach.json.

    python tools/solver_split_reach.py [out.json] [--time-limit SECONDS] [--min-stones N]

The samples of the 64-game play_games job of tools/solver_rate.py, grouped by stone count from the most stones down, and then the
three known-answer positions of tools/solver_kats.py.  Per group two solve calls under the default budgets: one with splitting off
on a Solver without a book (what the solver did before), one with split_stones = 14 on a Solver with a book of 2^22 entries.  Every
solve call is a process of its own under its own time limit (a solve call cannot be interrupted from inside); the book travels from
one step to the next as a file (Solver.save_book / load_book), the lossy table does not.  A step that exceeds the limit is recorded
as "exceeded the time limit" and never tried again; because the groups only get harder, and because a process killed in the middle of
its work is no state to go on from, every step that would follow it is recorded as "not run".  Results are written after every step,
so what was measured before is kept.
Reach and speed are recorded here, never promised and never asserted in a test."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPLIT_STONES, BOOK_ENTRIES = 14, 1 << 22


def step(args):
    """One solve call: positions from a .npy, the book in from / out to a .npy, a JSON row on the last line of stdout."""
    import c4a0_amd

    positions, split, book_in, book_out = args
    pos = np.load(positions)
    kw = dict(book_entries=BOOK_ENTRIES) if split == "split" else {}
    with c4a0_amd.Solver(**kw) as solver:
        if split == "split" and os.path.exists(book_in):
            solver.load_book(book_in)
        t0 = time.perf_counter()
        r = solver.solve(pos, **(dict(split_stones=SPLIT_STONES) if split == "split" else {}))
        wall = time.perf_counter() - t0
        if split == "split":
            solver.save_book(book_out)
        row = dict(r.stats, positions=len(pos), solved=int(r.solved.sum()), solved_fraction=float(r.solved.mean()), wall_s=wall,
                   book_size=solver.book_size, scores=r.scores.tolist() if len(pos) == 1 else None)
    print(json.dumps(row))


def run_step(positions, split, book, limit):
    book_out = book + ".next.npy"
    cmd = [sys.executable, os.path.abspath(__file__), "--step", positions, split, book, book_out]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"outcome": "exceeded the time limit", "time_limit_s": limit}
    if r.returncode != 0:
        return {"outcome": "failed", "returncode": r.returncode, "stderr": r.stderr[-2000:]}
    if split == "split":
        os.replace(book_out, book)
    return dict(json.loads(r.stdout.strip().splitlines()[-1]), outcome="ran", process_s=time.perf_counter() - t0)


def main():
    import torch

    import c4a0_amd
    from c4a0_amd.solver import is_terminal, stone_counts
    from helpers import hash_eval_torch
    from solver_kats import KATS
    from solver_ref import from_moves

    argv = sys.argv[1:]
    limit = float(argv[argv.index("--time-limit") + 1]) if "--time-limit" in argv else 120.0
    min_stones = int(argv[argv.index("--min-stones") + 1]) if "--min-stones" in argv else 0
    named = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--time-limit", "--min-stones"))]
    out = named[0] if named else os.path.join(ROOT, "profiles", "solver_split_reach.json")
    games = c4a0_amd.play_games([c4a0_amd.GameMetadata(i, 0, 0) for i in range(64)], 64, 12, 6.6, 0.01, evaluator=hash_eval_torch)
    recs, _ = games.to_records()
    live = ~is_terminal(recs["mask"], recs["value"])
    stones = stone_counts(recs["mask"])
    groups = [("%d stones" % s, int(s), np.stack([recs["mask"][live & (stones == s)], recs["value"][live & (stones == s)]], axis=1))
              for s in sorted(set(stones[live].tolist()), reverse=True) if s >= min_stones]
    groups += [("KAT " + name, len(moves), np.array([from_moves(moves)], dtype=np.uint64)) for name, moves, _ in KATS]
    res = {"device": torch.cuda.get_device_name(0), "job": "play_games, 64 games, hash evaluator, 12 simulations per move; then the three KATs",
           "split_stones": SPLIT_STONES, "book_entries": BOOK_ENTRIES, "budgets": "defaults", "time_limit_s": limit, "min_stones": min_stones,
           "steps": []}
    tmp = tempfile.mkdtemp(prefix="splitreach")
    book = os.path.join(tmp, "book.npy")
    stopped = None
    for name, s, pos in groups:
        path = os.path.join(tmp, "positions.npy")
        np.save(path, pos)
        row = {"group": name, "stones": s, "samples": len(pos)}
        for split in ("unsplit", "split"):
            if stopped:
                row[split] = {"outcome": "not run: " + stopped}
                continue
            row[split] = run_step(path, split, book, limit)
            if row[split]["outcome"] != "ran":
                stopped = "%s, %s: %s" % (name, split, row[split]["outcome"])
        res["steps"].append(row)
        print(row, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(sys.argv[2:6])
    else:
        main()
