"""The GPU solver's search stepped on the CPU (tests/solver_core_host.cpp compiles c4a0_amd/csrc/c4_solver_core.hpp, the code the
kernel runs, with g++) against the plain C solver: full budget, a launch budget of 64 node visits (every unfinished task goes on from its
saved stack, many times), a table of 2^10 entries (every store evicts) and a budget too small for some.  No GPU needed."""
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
    scores, solved, stats = np.zeros((len(pos), 7), np.int16), np.zeros(len(pos), np.uint8), np.zeros(5, np.uint64)
    assert emu_lib().emu_solve(pos.ctypes.data, len(pos), nodes_per_launch, max_nodes, log2_entries, scores.ctypes.data, solved.ctypes.data,
                               stats.ctypes.data) == 0
    return scores, solved.astype(bool), dict(zip(("nodes", "probes", "launches", "tasks", "unsolved_tasks"), stats.tolist()))


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


def test_search_core_budget_exhaustion_is_all_or_nothing():
    pos, want = the_set()
    got, solved, stats = emu(pos, 8, 24, 16)
    assert 0 < solved.sum() < len(pos) and stats["unsolved_tasks"] > 0
    assert np.array_equal(got[solved], want[solved])
    assert (got[~solved] == R.UNSOLVED).all()
