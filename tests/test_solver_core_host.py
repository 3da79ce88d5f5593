"""The GPU solver's search stepped on the CPU (tests/solver_core_host.cpp compiles c4a0_amd/csrc/c4_solver_core.hpp, the code the
kernel runs, with g++) against the plain C solver: full budget, a launch budget of 64 node visits (every unfinished task goes on from its
saved stack, many times), a table of 2^10 entries (every store evicts) and a budget too small for some -- on 1 000 positions of 24
stones, which the plain solver solves inside the test -- and under the same settings against the recorded rows of
tests/golden/solver_rows.npz from 19 stones down to 10, where the scores, the stacks and the root windows are larger than any
position of 24 stones has them.  No GPU needed."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import solver_ref as R  # noqa: E402

S = 24      # the reference solves 1 000 such positions in ~0.1 s


@functools.lru_cache(maxsize=None)
def emu_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="solvercore"), "libsolver_core_host.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "solver_core_host.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    L.emu_solve.restype = C.c_int
    L.emu_solve.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def emu(pos, nodes_per_launch, max_nodes, log2_entries):
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    scores, solved, stats = np.zeros((len(pos), 7), np.int16), np.zeros(len(pos), np.uint8), np.zeros(6, np.uint64)
    assert emu_lib().emu_solve(pos.ctypes.data, len(pos), nodes_per_launch, max_nodes, log2_entries, scores.ctypes.data, solved.ctypes.data,
                               stats.ctypes.data) == 0
    return scores, solved.astype(bool), dict(zip(("nodes", "probes", "launches", "tasks", "unsolved_tasks", "max_task_nodes"), stats.tolist()))


@functools.lru_cache(maxsize=None)
def the_set():
    pos = R.playout_positions(20261019, 1000, S)
    return pos, R.solve(pos)[0]


@pytest.mark.parametrize("nodes_per_launch,log2_entries", [(1 << 30, 16), (64, 16), (1 << 30, 10), (64, 10), (16, 4)])
def test_search_core_equals_plain_solver(nodes_per_launch, log2_entries):
    pos, want = the_set()
    got, solved, stats = emu(pos, nodes_per_launch, 1 << 22, log2_entries)
    assert solved.all() and stats["unsolved_tasks"] == 0
    assert np.array_equal(got, want)
    assert (stats["launches"] > 1) == (nodes_per_launch < 1 << 30)
    assert stats["probes"] >= stats["nodes"] > 0 and stats["tasks"] > len(pos) // 2


# Below 20 stones there is no reference a test can run: the rows are the recorded ones of tests/golden/solver_rows.npz.  Scores reach
# +-16 there (at most +-11 from 20 stones up) and a task's stack 30 frames (19).  A band = (lowest, highest stone count, first position,
# positions): the 12-stone rows go in two halves, so that no case takes much more than 30 s.  Per band and setting: the most node visits
# ONE task needed, measured with an unbounded budget -- a test gives every task twice that -- and the seconds the case took on one
# core.  The search on the CPU is deterministic, so the visits are exact.
LOW = {
    (14, 19, 0, 192): {(1 << 30, 20): (541_642, 3), (64, 16): (1_273_899, 4), (1 << 30, 10): (4_456_921, 4), (16, 4): (13_520_496, 14)},
    (13, 13, 0, 24): {(1 << 30, 20): (361_570, 1), (64, 16): (831_151, 1), (1 << 30, 10): (4_921_183, 2), (16, 4): (19_254_721, 7)},
    (12, 12, 0, 12): {(1 << 30, 20): (1_580_064, 3), (64, 16): (5_055_062, 5), (1 << 30, 10): (15_150_202, 8), (16, 4): (57_967_926, 25)},
    (12, 12, 12, 12): {(1 << 30, 20): (1_446_210, 2), (64, 16): (3_731_066, 3), (1 << 30, 10): (9_738_513, 4), (16, 4): (39_742_114, 17)},
    (11, 11, 0, 24): {(1 << 30, 20): (2_369_151, 6), (64, 16): (10_666_841, 20), (1 << 30, 10): (25_300_734, 25), (16, 4): (94_093_476, 100)},
    (10, 10, 0, 24): {(1 << 30, 20): (4_502_226, 14), (64, 16): (37_264_044, 71), (1 << 30, 10): (108_830_868, 90),
                      (16, 4): (289_429_601, 360)},
}
# the 10- and 11-stone bands are minutes under the small budgets and tables: only their first setting runs with the plain suite
LOW_CASES = [pytest.param(band, setting, marks=[pytest.mark.slow] if band[0] < 12 and setting != (1 << 30, 20) else [],
                          id="-".join(map(str, band + setting))) for band, settings in LOW.items() for setting in settings]


def test_the_low_bands_are_every_golden_row():
    g = R.golden()
    taken = np.concatenate([np.flatnonzero((g.stones >= lo) & (g.stones <= hi))[first:first + n] for lo, hi, first, n in LOW])
    assert np.array_equal(np.sort(taken), np.arange(len(g.pos))) and R.GOLDEN_L == 10


@pytest.mark.parametrize("band,setting", LOW_CASES)
def test_search_core_equals_golden_rows_below_20_stones(band, setting):
    """(64, 16): every unfinished task goes on from a saved stack up to 30 frames deep, many times; (16, 4): a table of 16 entries."""
    lo, hi, first, n = band
    pos, want = R.golden().select(lo, hi)
    pos, want = pos[first:first + n], want[first:first + n]
    assert len(pos) == n
    needed, _seconds = LOW[band][setting]
    got, solved, stats = emu(pos, setting[0], 2 * needed, setting[1])
    print(band, setting, stats)
    assert solved.all() and stats["unsolved_tasks"] == 0
    assert np.array_equal(got, want)
    assert stats["max_task_nodes"] == needed                       # the budget is what it says: twice what the hardest task takes
    assert (stats["launches"] > 1) == (setting[0] < 1 << 30)
    assert stats["probes"] >= stats["nodes"] > 0 and stats["tasks"] > len(pos)


def test_search_core_budget_exhaustion_is_all_or_nothing():
    pos, want = the_set()
    got, solved, stats = emu(pos, 8, 24, 16)
    assert 0 < solved.sum() < len(pos) and stats["unsolved_tasks"] > 0
    assert np.array_equal(got[solved], want[solved])
    assert (got[~solved] == R.UNSOLVED).all()
