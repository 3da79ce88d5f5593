"""The solver's scheduler and book (c4a0_amd/csrc/c4_solver_split.hpp) on the CPU: tests/solver_split_host.cpp gives it a "launch"
that loops over the Lane::step the kernel runs, and the plain C solver (tests/solver_ref.c) says what every row must be.  Splitting
at a budget of 64 node visits, the cap on split tasks, the book (canonical keys, export and import, a second solve without a launch,
a book that fills up, invalid entries refused by index) on positions of 24 stones, which the plain solver solves inside the test;
splitting and the book once more at 12 and 13 stones, where they are meant to be used, against the recorded rows of
tests/golden/solver_rows.npz; and the same driver as a stand-alone program under AddressSanitizer and UBSan.  No GPU needed."""
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

STATS = ("nodes", "probes", "launches", "tasks", "unsolved_tasks", "split_tasks", "combined_nodes", "dropped_tasks", "book_hits_host",
         "book_inserts", "book_full")
SEED, N_POSITIONS, STONES, BUDGET = 20261019, 300, 24, 64
SPLIT_TASKS = 170_462      # measured: test_splitting_solves_what_the_budget_alone_does_not


def _compile(extra, out):
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror"] + extra + [os.path.join(HERE, "solver_split_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@functools.lru_cache(maxsize=None)
def emu_lib():
    L = C.CDLL(_compile(["-O2", "-shared", "-fPIC"], os.path.join(tempfile.mkdtemp(prefix="solversplit"), "libsolver_split_host.so")))
    vp, u64 = C.c_void_p, C.c_uint64
    L.sp_create.restype, L.sp_create.argtypes = vp, [C.c_uint32, u64, C.c_int]
    L.sp_destroy.restype, L.sp_destroy.argtypes = None, [vp]
    L.sp_solve.restype, L.sp_solve.argtypes = C.c_int, [vp, vp, u64, u64, u64, u64, u64, vp, vp, vp, C.c_char_p, u64]
    L.sp_canonical_key.restype, L.sp_canonical_key.argtypes = u64, [u64, u64]
    L.sp_book_size.restype, L.sp_book_size.argtypes = u64, [vp]
    L.sp_book_export.restype, L.sp_book_export.argtypes = u64, [vp, vp, u64]
    L.sp_book_import.restype, L.sp_book_import.argtypes = C.c_int, [vp, vp, u64, C.c_char_p, u64]
    return L


class Emu:
    def __init__(self, log2_entries=16, book_entries=0, book_max_stones=41):
        self.h = C.c_void_p(emu_lib().sp_create(log2_entries, book_entries, book_max_stones))

    def close(self):
        emu_lib().sp_destroy(self.h)

    def solve(self, pos, nodes_per_launch=8, max_nodes=BUDGET, split_stones=42, split_max_tasks=1 << 20):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        scores, solved, stats = np.zeros((len(pos), 7), np.int16), np.zeros(len(pos), np.uint8), np.zeros(len(STATS), np.uint64)
        err = C.create_string_buffer(256)
        status = emu_lib().sp_solve(self.h, pos.ctypes.data, len(pos), nodes_per_launch, max_nodes, split_stones, split_max_tasks, scores.ctypes.data,
                                    solved.ctypes.data, stats.ctypes.data, err, len(err))
        assert status == 0, (status, err.value)
        return scores, solved.astype(bool), dict(zip(STATS, stats.tolist()))

    def book(self):
        out = np.zeros(emu_lib().sp_book_size(self.h), np.uint64)
        assert emu_lib().sp_book_export(self.h, out.ctypes.data, len(out)) == len(out)
        return out

    def load(self, entries):
        entries = np.ascontiguousarray(entries, dtype=np.uint64)
        err = C.create_string_buffer(256)
        return emu_lib().sp_book_import(self.h, entries.ctypes.data, len(entries), err, len(err)), err.value.decode()


@functools.lru_cache(maxsize=None)
def the_set():
    """(300 positions of 24 stones, the plain C solver's rows): computed once, shared, never written to."""
    pos = R.playout_positions(SEED, N_POSITIONS, STONES, STONES)
    rows = R.solve(pos)[0]
    pos.setflags(write=False)
    rows.setflags(write=False)
    return pos, rows


def test_splitting_solves_what_the_budget_alone_does_not():
    """Measured on the set, with a table of 2^16 entries: 228 992 tasks made by splitting (229 443 tasks, 9 726 199 node visits, 92
    launches) under a launch budget of 8, and 170 462 (170 913 tasks, 7 172 316 visits, 12 launches) under one of 2^30: the launch
    budget changes the order in which the lanes store to the table and so the node counts, never a score.  Without splitting the
    budget of 64 visits solves only part of the set."""
    pos, want = the_set()
    assert all(bin(int(m)).count("1") == STONES for m in pos[:, 0]) and len(np.unique(pos, axis=0)) == N_POSITIONS
    results = []
    for nodes_per_launch in (8, 1 << 30):
        e = Emu()
        got, solved, stats = e.solve(pos, nodes_per_launch=nodes_per_launch)
        print(nodes_per_launch, stats)
        assert solved.all() and stats["unsolved_tasks"] == 0 and np.array_equal(got, want)
        assert stats["split_tasks"] > 0 and stats["combined_nodes"] > 0 and stats["tasks"] > stats["split_tasks"]
        plain, plain_solved, plain_stats = e.solve(pos, nodes_per_launch=nodes_per_launch, split_stones=0)
        assert 0 < plain_solved.sum() < len(pos) and plain_stats["split_tasks"] == 0 and plain_stats["unsolved_tasks"] > 0
        assert np.array_equal(plain[plain_solved], want[plain_solved]) and (plain[~plain_solved] == R.UNSOLVED).all()
        e.close()
        results.append(got)
    assert np.array_equal(results[0], results[1])


def test_split_stones_bounds_which_tasks_split():
    pos, want = the_set()
    e = Emu()
    got, solved, stats = e.solve(pos, split_stones=STONES + 1)      # the tasks have 25 stones: none may split
    assert stats["split_tasks"] == 0 and 0 < solved.sum() < len(pos)
    got, solved, stats = e.solve(pos, split_stones=STONES + 3)      # 25 and 26 stones may
    assert stats["split_tasks"] > 0 and np.array_equal(got[solved], want[solved]) and (got[~solved] == R.UNSOLVED).all()
    e.close()


def test_cap_on_split_tasks_is_all_or_nothing_and_a_larger_cap_finishes():
    pos, want = the_set()
    cap = 2000
    assert cap < SPLIT_TASKS
    e = Emu()
    got, solved, stats = e.solve(pos, split_max_tasks=cap)          # returns normally
    assert cap <= stats["split_tasks"] < cap + 7                    # the split that reaches the cap is the last
    assert 0 < solved.sum() < len(pos) and stats["unsolved_tasks"] > 0
    assert np.array_equal(got[solved], want[solved]) and (got[~solved] == R.UNSOLVED).all()      # never a mixture
    assert stats["dropped_tasks"] > 0                               # what only the failed positions needed left the live list
    got, solved, stats = e.solve(pos, split_max_tasks=1 << 20)
    assert solved.all() and np.array_equal(got, want)
    e.close()


def test_canonical_key_of_a_position_and_its_mirror():
    pos, _ = the_set()
    key = emu_lib().sp_canonical_key
    keys = set()
    for m, v in pos[:100].tolist():
        mm, mv = R.mirror(m, v)
        assert key(m, v) == key(mm, mv) and key(m, v) < 1 << 49
        keys.add(key(m, v))
    assert len(keys) == len({min((m, v), R.mirror(m, v)) for m, v in pos[:100].tolist()})      # and of nothing else
    assert key(0, 0) == 0 and key(1, 1) == key(1 << 6, 1 << 6) == 2 and key(1, 0) == 1


def test_book_round_trip_and_a_second_solve_without_a_launch():
    pos, want = the_set()
    pos, want = pos[:60], want[:60]
    a = Emu(book_entries=1 << 17)
    got, solved, stats = a.solve(pos)
    assert solved.all() and np.array_equal(got, want) and stats["book_inserts"] > 0 and stats["book_full"] == 0
    entries = a.book()
    assert len(entries) == stats["book_inserts"] and (entries != 0).all()
    got, solved, stats = a.solve(pos)
    assert stats["launches"] == 0 and stats["tasks"] == 0 and stats["book_hits_host"] > 0 and np.array_equal(got, want)
    mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
    got, solved, stats = a.solve(mirrored)
    assert stats["launches"] == 0 and np.array_equal(got, want[:, ::-1])
    b = Emu(book_entries=1 << 17)
    assert b.load(entries) == (0, "")
    assert np.array_equal(np.sort(b.book()), np.sort(entries))
    got, solved, stats = b.solve(pos, split_stones=0)
    assert stats["launches"] == 0 and np.array_equal(got, want)
    # the book as the search's leaves: positions one stone up use what is known below them
    up = R.playout_positions(SEED + 1, 40, STONES - 2, STONES - 2)
    got, solved, stats = b.solve(up)
    assert solved.all() and np.array_equal(got, R.solve(up)[0])
    a.close()
    b.close()


def test_splitting_and_the_book_at_12_and_13_stones_against_golden_rows():
    """The stone counts the book and `split_stones=14` are meant for, against the recorded rows (tests/golden/solver_rows.npz): scores to
    +-15 in the book's bytes.  Measured with a table of 2^20 entries: under 3 * 2^19 visits a task, two 13-stone tasks of the 48 positions
    run out and split into 7 tasks of 14 stones, which may not split and all finish (189 tasks, 23.8 M visits, 237 book entries, 5 s);
    under 2^20 visits two 14-stone tasks do not finish, under 2^22 nothing splits."""
    pos, want = R.golden().select(12, 13)
    assert len(pos) == 48
    e = Emu(log2_entries=20, book_entries=1 << 17)
    budget = dict(nodes_per_launch=1 << 30, max_nodes=3 << 19, split_stones=14)
    got, solved, stats = e.solve(pos, **budget)
    print(stats)
    assert solved.all() and stats["unsolved_tasks"] == 0 and np.array_equal(got, want)
    assert stats["split_tasks"] > 0 and stats["combined_nodes"] > 0
    assert stats["book_inserts"] > len(pos) and stats["book_full"] == 0 and len(e.book()) == stats["book_inserts"]
    scores_in_book = (e.book() >> np.uint64(56)).astype(np.int64) - 32
    assert scores_in_book.max() >= 13 and scores_in_book.min() <= -13        # beyond any score of a 20-stone position
    got, solved, stats = e.solve(pos, **budget)
    assert stats["launches"] == 0 and stats["tasks"] == 0 and stats["book_hits_host"] > 0 and solved.all() and np.array_equal(got, want)
    mirrored = np.array([R.mirror(m, v) for m, v in pos.tolist()], dtype=np.uint64)
    got, solved, stats = e.solve(mirrored, **budget)
    assert stats["launches"] == 0 and np.array_equal(got, want[:, ::-1])
    e.close()


def test_a_book_of_16_entries_fills_up_and_the_scores_stay_exact():
    pos, want = the_set()
    e = Emu(book_entries=16)
    got, solved, stats = e.solve(pos[:60])
    assert solved.all() and np.array_equal(got, want[:60])
    assert stats["book_full"] > 0 and stats["book_inserts"] == 8 and len(e.book()) == 8      # half full, and no further
    e.close()


def test_invalid_book_entries_are_refused_by_index():
    pos, _ = the_set()
    a = Emu(book_entries=1 << 17, book_max_stones=30)
    a.solve(pos[:20])
    good = a.book()
    assert len(good) > 10
    a.close()
    n = lambda e: bin(_mask_of_key(int(e) & ((1 << 49) - 1))).count("1")      # noqa: E731
    late = R.playout_positions(SEED, 1, 31, 31)[0].tolist()
    i = 5
    key, score = int(good[i]) & ((1 << 56) - 1), int(good[i]) >> 56
    mirror_key = sum(((key >> (7 * c)) & 0x7F) << (7 * (6 - c)) for c in range(7))
    assert mirror_key != key
    bad = {
        "bits between the key and the score": int(good[i]) | 1 << 52,
        "stones in the sentinel row": (key | 0x7F) | score << 56,
        "do not fit the side to move": 2 | 33 << 56,                       # one stone on the board and it is the mover's
        "a four on the board": _key_of_moves([0, 1, 0, 1, 0, 1, 0, 2]) | 32 << 56,
        "not the canonical key": mirror_key | score << 56,
        "more stones than book_max_stones": emu_lib().sp_canonical_key(*late) | 32 << 56,
        "a score outside the range": key | (32 + (43 - n(good[i])) // 2 + 1) << 56,
        "empty": 0,
    }
    for why, entry in bad.items():
        b = Emu(book_entries=1 << 17, book_max_stones=30)
        entries = good.copy()
        entries[i] = np.uint64(entry)
        status, err = b.load(entries)
        assert status == 1 and err.startswith(f"entry {i}: "), (why, err)
        if why != "empty":
            assert why in err, (why, err)
        assert len(b.book()) == 0                                          # all or none
        assert b.load(good) == (0, "")
        b.close()
    tiny = Emu(book_entries=16)
    status, err = tiny.load(good)
    assert status == 1 and "half full" in err
    assert tiny.load(np.repeat(good[:8], 3)) == (0, "") and len(tiny.book()) == 8      # duplicates count once: eight entries fit
    tiny.close()
    # the same position with another score: refused by the index of the second, in one file or against the book
    other = np.uint64(int(good[i]) ^ (1 << 56))
    b = Emu(book_entries=1 << 17, book_max_stones=30)
    status, err = b.load(np.concatenate([good, [other]]))
    assert status == 1 and err.startswith(f"entry {len(good)}: the position is already known") and len(b.book()) == 0
    assert b.load(good) == (0, "") and b.load(good) == (0, "") and len(b.book()) == len(good)
    status, err = b.load(np.array([good[0], other], dtype=np.uint64))
    assert status == 1 and err.startswith("entry 1: the position is already known")
    b.close()


def _mask_of_key(key):
    mask = 0
    for c in range(7):
        col = ((key >> (7 * c)) & 0x7F) + 1
        mask |= ((1 << (col.bit_length() - 1)) - 1) << (7 * c)
    return mask


def _key_of_moves(moves):
    """The canonical key of the position after `moves`, whatever it is (terminal positions included): computed here, bit by bit."""
    height, stones = [0] * 7, [0, 0]
    for k, c in enumerate(moves):
        stones[k % 2] |= 1 << (7 * c + height[c])
        height[c] += 1
    mask, pos = stones[0] | stones[1], stones[len(moves) % 2]
    key = pos + mask
    mirror = sum(((key >> (7 * c)) & 0x7F) << (7 * (6 - c)) for c in range(7))
    return min(key, mirror)


def test_the_driver_as_a_stand_alone_program_under_sanitizers():
    exe = _compile(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSPLIT_HOST_MAIN"],
                   os.path.join(tempfile.mkdtemp(prefix="solversplit"), "solver_split_host"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "solver_split_host ok" in r.stdout, r.stdout + r.stderr
