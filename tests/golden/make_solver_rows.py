"""Generates tests/golden/solver_rows.npz: score rows of positions with 10 to 19 stones, the stone counts below the ones at which
a test can afford to run a reference itself.  The solver tests (tests/test_solver_golden.py, test_solver_core_host.py,
test_solver_split_host.py on the CPU, test_gpu_solver_low_stones.py on the GPU) load the file; none of them regenerates it.

    python tests/golden/make_solver_rows.py            # writes the file
    python tests/golden/make_solver_rows.py --check    # generates it again and compares it with the committed file, byte for byte

CPUs only, a process pool over positions.  Positions: solver_ref.playout_positions(SEED + s, n, s, s) per stone count s.

  14..19 stones, 32 positions each: rows of the plain `solve` (tests/solver_ref.c: no table, the trust anchor).  `solve_tt` runs on
                 all of them too, and on any difference nothing is written.
  10..13 stones, 24 positions each: rows of `solve_tt`, which is pinned to `solve` by tests/test_solver_ref.py and by the 192 rows above.

Per position: mask, value (row-major, as everywhere in the tests), stones, row (int16[7]), ref (an index into `references`:
0 = solve, 1 = solve_tt) and ref_nodes, the nodes that reference visited for the row.

Measured on 8 CPUs (wall time of each pool.map over 8 processes; the whole run takes about two minutes):
  solve     14..19 stones, 192 positions: 59.3 s, 9 340 619 690 nodes
  solve_tt  14..19 stones, the same 192:   2.0 s,   100 590 200 nodes -- 93 times fewer nodes than the plain solver, at about the
            same nodes per second; on the 2 000 positions of 20 or more stones of tests/test_gpu_solver.py 14 times fewer (7.8 M
            against 111.6 M nodes, 1.0 s against 5.0 s on one CPU)
  solve_tt  13 stones: 1.5 s, 56 M nodes   12 stones: 4.7 s, 187 M   11 stones: 21.5 s, 519 M   10 stones: 35.8 s, 1 141 M nodes
            (the most for one position: 232 M)
L = 10 is the lowest count in the file.  The table solver would reach further in the 20 minutes it was allowed; what stops at 10 is
the other side: the CPU build of the kernel's search needs 1 to 6 minutes per setting for the 24 positions of 10 stones under the
small budgets and tables (tests/test_solver_core_host.py), a factor of 3 to 4 more per stone.  Nothing below 10 was tried.
"""
import io
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import solver_ref as R  # noqa: E402

OUT = os.path.join(HERE, "solver_rows.npz")
SEED = 77
L = 10
PLAIN = {s: 32 for s in range(14, 20)}       # stones -> positions, rows of solve
TT_ONLY = {s: 24 for s in range(L, 14)}      # ... rows of solve_tt
REFERENCES = ("solve", "solve_tt")
PROCESSES = 8


def positions():
    """uint64[N, 2] in ascending stone count, and the stone count of each."""
    counts = {**TT_ONLY, **PLAIN}
    pos = np.concatenate([R.playout_positions(SEED + s, counts[s], s, s) for s in sorted(counts)])
    stones = np.concatenate([np.full(counts[s], s, dtype=np.uint8) for s in sorted(counts)])
    return pos, stones


def _one(job):
    which, mask, value = job
    rows, nodes = (R.solve, R.solve_tt)[which]([(mask, value)])
    return rows[0], nodes


def _run(pool, which, pos):
    """(rows, nodes, wall seconds) of one reference on `pos`, the positions with the fewest stones (the longest searches) first."""
    t = time.time()
    got = pool.map(_one, [(which, int(m), int(v)) for m, v in pos.tolist()], chunksize=1)
    return np.array([g[0] for g in got], dtype=np.int16).reshape(-1, 7), np.array([g[1] for g in got], dtype=np.uint64), time.time() - t


def npz_bytes(arrays) -> bytes:
    """An .npz that np.load reads, the same bytes every time: stored, not deflated, with the epoch of the zip format as every date."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as zf:
        for name, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, member.getvalue())
    return buf.getvalue()


def generate() -> bytes:
    pos, stones = positions()
    assert len(np.unique(pos, axis=0)) == len(pos)
    assert [bin(int(m)).count("1") for m in pos[:, 0]] == stones.tolist()
    R.ref_lib()                                  # built once, before the pool forks
    high = stones >= 14
    with multiprocessing.get_context("fork").Pool(PROCESSES) as pool:
        rows = np.zeros((len(pos), 7), dtype=np.int16)
        nodes = np.zeros(len(pos), dtype=np.uint64)
        rows[high], nodes[high], wall = _run(pool, 0, pos[high])
        print(f"solve     14..19 stones, {int(high.sum())} positions: {wall:.1f} s, {int(nodes[high].sum())} nodes", flush=True)
        tt_rows, tt_nodes, wall = _run(pool, 1, pos[high])
        print(f"solve_tt  14..19 stones, {int(high.sum())} positions: {wall:.1f} s, {int(tt_nodes.sum())} nodes", flush=True)
        if not np.array_equal(tt_rows, rows[high]):
            bad = np.flatnonzero((tt_rows != rows[high]).any(axis=1))
            raise SystemExit(f"solve_tt differs from solve on {len(bad)} positions, the first {pos[high][bad[0]].tolist()}: nothing written")
        for s in sorted(TT_ONLY, reverse=True):
            sel = stones == s
            rows[sel], nodes[sel], wall = _run(pool, 1, pos[sel])
            print(f"solve_tt  {s} stones, {int(sel.sum())} positions: {wall:.1f} s, {int(nodes[sel].sum())} nodes, max {int(nodes[sel].max())}", flush=True)
    for s in sorted(set(stones.tolist())):
        legal = rows[stones == s][rows[stones == s] != R.FULL_COLUMN]
        print(f"{s} stones: scores {int(legal.min())}..{int(legal.max())}")
    return npz_bytes({"mask": pos[:, 0], "value": pos[:, 1], "stones": stones, "row": rows, "ref": (~high).astype(np.uint8),
                      "ref_nodes": nodes, "references": np.array(REFERENCES)})


def main():
    data = generate()
    if "--check" in sys.argv[1:]:
        same = open(OUT, "rb").read() == data
        print("the committed file is reproduced byte for byte" if same else "DIFFERENT from the committed file")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
