"""The plain C solver and its variant with a table (tests/solver_ref.c, built here with gcc) behind numpy, the positions the solver
tests share, the recorded rows of 10 to 19 stones (tests/golden/solver_rows.npz), and
Solution::score_policy (reference rust/src/solver.rs:201-228) restated one row at a time."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from c4a0_amd.results import _has_four, flip_h_bits, terminal_state

HERE = os.path.dirname(os.path.abspath(__file__))
FULL_COLUMN, UNSOLVED = -1000, -32768
_COL0 = 0x810204081


@functools.lru_cache(maxsize=None)
def ref_lib() -> C.CDLL:
    out = os.path.join(tempfile.mkdtemp(prefix="solverref"), "libsolver_ref.so")
    cmd = ["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "solver_ref.c"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    L.solve_scores.restype, L.solve_scores.argtypes = C.c_uint64, [C.c_void_p, C.c_uint64, C.c_void_p]
    L.brute_scores.restype, L.brute_scores.argtypes = None, [C.c_void_p, C.c_uint64, C.c_void_p]
    L.solve_scores_tt.restype, L.solve_scores_tt.argtypes = C.c_uint64, [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def _as_positions(positions) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(positions, dtype=np.uint64).reshape(-1, 2))


def solve(positions):
    """(int16[P, 7] scores, nodes visited) of the plain alpha-beta solver."""
    pos = _as_positions(positions)
    out = np.zeros((len(pos), 7), dtype=np.int16)
    nodes = ref_lib().solve_scores(pos.ctypes.data, len(pos), out.ctypes.data)
    return out, int(nodes)


def solve_tt(positions):
    """(int16[P, 7] scores, nodes visited) of the same negamax with a transposition table: the checker below the stone counts
    `solve` reaches.  Every position starts from an empty table, so a row and its node count do not depend on the batch."""
    pos = _as_positions(positions)
    out = np.zeros((len(pos), 7), dtype=np.int16)
    nodes = ref_lib().solve_scores_tt(pos.ctypes.data, len(pos), out.ctypes.data)
    if nodes == (1 << 64) - 1:
        raise MemoryError("solve_scores_tt: no memory for its table")
    return out, int(nodes)


def brute(positions) -> np.ndarray:
    """int16[P, 7]: the same rows with no pruning at all."""
    pos = _as_positions(positions)
    out = np.zeros((len(pos), 7), dtype=np.int16)
    ref_lib().brute_scores(pos.ctypes.data, len(pos), out.ctypes.data)
    return out


def play(mask: int, value: int, col: int):
    """The position after the side to move drops a stone into `col` (c4r.rs:58-72)."""
    h = bin(mask & (_COL0 << col)).count("1")
    assert h < 6
    bit = 1 << (7 * h + col)
    mask |= bit
    return mask, ~(value | bit) & mask


def from_moves(moves):
    mask = value = 0
    for c in moves:
        mask, value = play(mask, value, c)
    return mask, value


def legal(mask: int):
    return [c for c in range(7) if not (mask >> (35 + c)) & 1]


def mirror(mask: int, value: int):
    return flip_h_bits(mask), flip_h_bits(value)


def playout_positions(seed: int, n: int, min_stones: int, max_stones: int = 41) -> np.ndarray:
    """uint64[n, 2]: distinct non-terminal positions with min_stones..max_stones stones from seeded random playouts, in the order
    met.  Every other playout declines a winning move while another move exists, so that games reach the last cells."""
    rng = np.random.default_rng(seed)
    seen, out, game = set(), [], 0
    while len(out) < n:
        mask = value = 0
        shy = game % 2 == 1
        game += 1
        while terminal_state(mask, value) == 0:
            s = bin(mask).count("1")
            if min_stones <= s <= max_stones and (mask, value) not in seen:
                seen.add((mask, value))
                out.append((mask, value))
                if len(out) == n:
                    break
            cols = legal(mask)
            if shy:
                quiet = [c for c in cols if not _has_four(play(mask, value, c)[0] & ~play(mask, value, c)[1])]
                cols = quiet or cols
            mask, value = play(mask, value, int(cols[rng.integers(len(cols))]))
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


class GoldenRows:
    """tests/golden/solver_rows.npz (written by tests/golden/make_solver_rows.py, never by a test): positions of GOLDEN_L to 19 stones
    and their score rows, the plain solver's from 14 stones up, the table solver's below.  Loaded once; the arrays are read-only."""

    def __init__(self, z):
        self.pos = np.stack([z["mask"], z["value"]], axis=1).astype(np.uint64)
        self.stones, self.rows = z["stones"].astype(np.int64), z["row"].astype(np.int16)
        self.ref = np.array([str(z["references"][i]) for i in z["ref"]])
        self.ref_nodes = z["ref_nodes"].astype(np.uint64)
        for a in (self.pos, self.stones, self.rows, self.ref, self.ref_nodes):
            a.setflags(write=False)

    def select(self, lo, hi, max_ref_nodes=None):
        """(positions, rows) with lo..hi stones, in the file's order; max_ref_nodes: only those whose reference visited no more
        nodes for the row -- the one way a test narrows its input."""
        keep = (self.stones >= lo) & (self.stones <= hi)
        if max_ref_nodes is not None:
            keep &= self.ref_nodes <= np.uint64(max_ref_nodes)
        return self.pos[keep], self.rows[keep]


GOLDEN_L = 10      # the lowest stone count of the golden rows


@functools.lru_cache(maxsize=None)
def golden() -> GoldenRows:
    with np.load(os.path.join(HERE, "golden", "solver_rows.npz"), allow_pickle=False) as z:
        return GoldenRows(z)


def kinds(positions, scores):
    """How many rows of each kind the edge tests want to see: immediate wins, full columns, 41 stones, a single legal move."""
    pos = _as_positions(positions)
    stones = np.array([bin(int(m)).count("1") for m in pos[:, 0]])
    win_now = (scores == ((43 - stones) // 2)[:, None]) & (scores > 0)
    # a score of (43 - s) / 2 is only reachable by winning with this very stone
    full = scores == FULL_COLUMN
    return {"immediate_win": int(win_now.any(axis=1).sum()), "full_column": int(full.any(axis=1).sum()),
            "stones_41": int((stones == 41).sum()), "single_legal_move": int((full.sum(axis=1) == 6).sum())}


def score_policy_row(row, policy) -> float:
    """Solution::score_policy, line for line."""
    row = [int(x) for x in row]
    sol_max = max(row)
    best_moves = [i for i, x in enumerate(row) if x == sol_max]
    winning_moves = [i for i, x in enumerate(row) if x > 0]
    policy = [float(p) for p in policy]
    policy_max = max(policy)
    selected = policy.index(policy_max)
    if selected in best_moves:
        return 1.0
    if selected in winning_moves:
        return 0.5
    return 0.0
