"""Whole games from given start positions, on the CPU.  Every other whole-game parity test starts from the empty board, where the
ply of the root, popcount(root mask), and the number of moves the game has recorded, n_moves, are the same number; the reference
uses the first for the temperature (self_play.rs:294-299), the ply penalty and the leaf's model (mcts.rs:70-76), the second for
the move seed game_id * (42 + n_moves) (mcts.rs:215), the record index and the sign of every sample's q (mcts.rs:271-313).  From a
start position (MctsGame::new_from_pos, mcts.rs:48-56) they differ.  This file holds

  * the oracle's driver for such games, c4o_play_from, against c4o_self_play (empty starts) and against a plain Python loop over
    the Game API;
  * the job tests/test_gpu_start_positions.py plays on the device (tests.helpers.start_job) to the floors that make it worth
    playing: odd-ply and late starts, terminal starts, games ending on the full board and drawn (the only records that hold
    -0.0), first moves made where the two temperature rules disagree;
  * twin mutants of the Python loop -- temperature from n_moves, seed from the ply, q sign from the ply, start position by slot
    instead of by ordinal -- each of which must change a game of the job: the inputs discriminate."""
import numpy as np
import pytest

from oracle import c4oracle as O
from tests.helpers import (N_START_SLOTS, START_EVALS, START_SETTINGS, evidence, oracle_samples_by_game, start_job)

PLY = lambda m: bin(int(m)).count("1")   # noqa: E731


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# --------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("noise", [(0.0, 0.0), (0.3, 0.25)], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_play_from_with_empty_starts_equals_self_play(ev_name, noise):
    """the id list of tests/test_gpu_mcts_parity.py test_self_play_hash_evaluator_bit_identical: samples bit for bit, and the tree
    counters (the evaluator rows differ: c4o_self_play asks once per distinct position of a tick)"""
    ev, c_expl, _ = START_EVALS[ev_name]
    n_games, n_iter = 96, 25
    ids = [0, 42, 43, 1 << 40, (1 << 64) - 1] + list(range(1000, 1000 + n_games))
    reqs = [(g, 0, 0) for g in ids[:n_games]]
    want, wst = O.self_play(reqs, 1 << 20, n_iter, c_expl, 0.01, ev, dirichlet=noise)
    for starts in (None, [(0, 0)] * n_games):
        got, gst = O.play_from(reqs, starts, n_iter, c_expl, 0.01, ev, dirichlet=noise)
        assert oracle_samples_by_game(got) == oracle_samples_by_game(want)
        for k in ("n_games", "n_samples", "sims", "sims_terminal_root", "select_levels", "select_levels_discarded", "backup_nodes", "expansions",
                  "nodes_created", "moves", "sims_deep", "sims_deep_terminal", "max_depth", "moves_without_search"):
            assert gst[k] == wst[k], k
        assert gst["nn_calls"] == gst["nn_positions"] == gst["sims"]
    if noise[1] > 0:
        assert oracle_samples_by_game(want) != oracle_samples_by_game(O.self_play(reqs, 1 << 20, n_iter, c_expl, 0.01, ev)[0])


def _temperature(ply):   # self_play.rs:294-299
    return 4.0 if ply < 4 else (2.0 if ply < 8 else 1.0)


def game_loop(req, start, n_iter, c_expl, c_ply, temperature_from="ply", seed_from="n_moves", sign_from="n_moves"):
    """One game through the Game API, c4o_game_step (self_play.rs:268-323) and c4o_game_to_result (mcts.rs:271-313) taken apart so
    that each use of the ply / of n_moves can be swapped for the other.  With the defaults it IS the reference's loop."""
    gid, p0, p1 = req
    g = O.Game(O.Pos(*start), gid, p0, p1)
    while True:
        leaf = g.leaf_pos()
        lp, qp, qn = O.hash_eval_pos(leaf.mask, leaf.value)
        assert g.on_received_policy(lp, qp, qn, c_expl, c_ply) == 0
        if g.root_visit_count() < n_iter:
            continue
        root = g.root_pos()
        if O.terminal_state(root) != 0:
            break
        t = _temperature(PLY(root.mask) if temperature_from == "ply" else g.n_moves())
        col = O.sample_move(gid, g.n_moves() if seed_from == "n_moves" else PLY(root.mask), g.root_policy(), t)
        assert g.make_move(col, c_expl) == 0
    out = g.to_result(c_ply)
    m = g.n_moves() if sign_from == "n_moves" else PLY(out[-1].mask)
    q, qn = out[-1].q_penalty, out[-1].q_no_penalty
    for i, s in enumerate(out[:-1]):   # sample i gets +q iff (M - i) is even
        neg = (m - i) & 1
        s.q_penalty, s.q_no_penalty = (float(-np.float32(q)), float(-np.float32(qn))) if neg else (q, qn)
    return out, g


def _loop_samples(reqs, starts, n_iter, c_expl, **kw):
    return oracle_samples_by_game({r[0]: game_loop(r, s, n_iter, c_expl, 0.01, **kw)[0] for r, s in zip(reqs, starts)})


def test_play_from_equals_a_plain_loop_over_the_game_api():
    """the whole job at n = 24 and every fourth game at n = 100, hash evaluator: samples bit for bit, counters summed"""
    reqs, starts, _part = start_job()
    for n_iter, step in ((24, 1), (100, 4)):
        rq, st = reqs[::step], starts[::step]
        got, gst = O.play_from(rq, st, n_iter, 6.6, 0.01, "hash")
        loop = {}
        ctr = {}
        for r, s in zip(rq, st):
            loop[r[0]], g = game_loop(r, s, n_iter, 6.6, 0.01)
            for k, v in g.counters().items():
                ctr[k] = max(ctr.get(k, 0), v) if k == "max_depth" else ctr.get(k, 0) + v
        assert oracle_samples_by_game(got) == oracle_samples_by_game(loop)
        for k, v in ctr.items():
            if k not in ("select_levels_discarded", "moves_without_search"):   # kept by c4o_game_step itself, which the loop takes apart
                assert gst[k] == v, k
    # and the reference's loop from the empty board is the reference's self_play
    rq = [(g, 0, 0) for g in [0, 42, 43, 1 << 40, (1 << 64) - 1] + list(range(1000, 1011))]
    assert _loop_samples(rq, [(0, 0)] * len(rq), 24, 6.6) == oracle_samples_by_game(O.self_play(rq, 64, 24, 6.6, 0.01, "hash")[0])


# --------------------------------------------------------------------------------------------- the job
def test_the_job_is_what_it_says():
    reqs, starts, part = start_job()
    assert len(reqs) == len(starts) == 495 > 3 * N_START_SLOTS and len({r[0] for r in reqs}) == 495
    assert {0, 42, 43, 1 << 40, (1 << 64) - 1} <= {r[0] for r in reqs} and all(p0 != p1 for _g, p0, p1 in reqs)
    kind = [O.terminal_state(O.Pos(*s)) for s in starts]
    ply = [PLY(m) for m, _v in starts]
    rnd = [i for i, p in enumerate(part) if p == "random"]
    assert len(rnd) == 480 and part.count("line") == 14 and part.count("won") == 1
    # the constructed part: the drawn board cut k moves short has one legal column
    line = sorted(ply[i] for i, p in enumerate(part) if p == "line")
    assert line == sorted(2 * list(range(36, 43)))
    for i, p in enumerate(part):
        if p == "line":
            assert kind[i] == (3 if ply[i] == 42 else 0) and (ply[i] == 42 or bin(O.legal_mask(O.Pos(*starts[i]))).count("1") == 1)
        if p == "won":
            assert kind[i] == 1 and O.terminal_value(O.Pos(*starts[i]), 0.01)[1:] == (pytest.approx(0.96), 1.0)
    # floors on the inputs
    odd = sum(p & 1 for p in ply)
    late = sum(1 for i in rnd if ply[i] >= 30)
    assert odd >= 0.40 * len(starts) and late >= 0.25 * len(rnd) and kind.count(2) >= 32 and kind.count(3) == 2
    # terminal, late and early starts interleave: every run of N_START_SLOTS consecutive games holds each sort
    for lo in range(0, len(starts) - N_START_SLOTS + 1, 16):
        w = range(lo, lo + N_START_SLOTS)
        assert any(kind[i] for i in w) and any(ply[i] < 8 for i in w) and any(ply[i] >= 30 and not kind[i] for i in w)
    evidence(f"start positions, the job: {len(starts)} games on {N_START_SLOTS} slots, {odd} starts at odd ply, {late} of {len(rnd)} random "
             f"starts at ply >= 30, terminal starts by kind {[kind.count(k) for k in (1, 2, 3)]}")


@pytest.mark.parametrize("ev_name,n_iter", START_SETTINGS, ids=[f"{e}-n{n}" for e, n in START_SETTINGS])
def test_the_job_reaches_the_end_of_the_game_under_every_setting(ev_name, n_iter):
    """floors on what the oracle plays from these starts, under each setting the device is compared at"""
    reqs, starts, part = start_job()
    ev, c_expl, _ = START_EVALS[ev_name]
    res, st = O.play_from(reqs, starts, n_iter, c_expl, 0.01, ev)
    full = sum(1 for r, p in zip(reqs, part) if p == "random" and PLY(res[r[0]][-1].mask) == 42)
    drawn = sum(1 for r in reqs if O.terminal_state(O.Pos(res[r[0]][-1].mask, res[r[0]][-1].value)) == 3)
    neg_zero = sum(1 for ss in res.values() for s in ss if _bits(s.q_penalty) == 0x80000000)
    # the first move is made at ply >= 8 (temperature 1) with n_moves = 0 (4, were the temperature taken from it)
    disagree = sum(1 for r, s in zip(reqs, starts) if PLY(s[0]) >= 8 and len(res[r[0]]) > 1)
    one_column = sum(1 for ss in res.values() for s in ss[:-1] if bin(O.legal_mask(O.Pos(s.mask, s.value))).count("1") == 1)
    assert full >= 8 and drawn >= 16 and neg_zero >= 1 and disagree >= 100 and one_column >= 42
    for r, s, p in zip(reqs, starts, part):
        ss = res[r[0]]
        assert (ss[0].mask, ss[0].value) == s and len(ss) <= 43 - PLY(s[0])
        if p == "line":   # k moves down the one open column to the draw: k + 1 samples, q = +0 / -0 alternating from the end
            k = 42 - PLY(s[0])
            assert len(ss) == k + 1 and [_bits(x.q_penalty) for x in ss] == [0x80000000 if (k - i) & 1 else 0 for i in range(k + 1)]
        if O.terminal_state(O.Pos(*s)) != 0:
            assert len(ss) == 1 and ss[0].policy == tuple([float(np.float32(1.0) / np.float32(7.0))] * 7)
    n_term = sum(1 for s in starts if O.terminal_state(O.Pos(*s)) != 0)
    assert st["sims_terminal_root"] >= n_term * n_iter
    evidence(f"start positions, oracle alone, {ev_name} n = {n_iter}: {st['n_samples']} samples, {st['moves']} moves; {full} random games end on the "
             f"full board, {drawn} games drawn, {neg_zero} records with q = -0.0, {disagree} first moves where the temperature rules "
             f"disagree, {one_column} moves from a root with one legal column")


# --------------------------------------------------------------------------------------------- twin mutants
def test_twin_mutants_of_the_loop_change_the_job():
    """each confusion of the ply with n_moves, and of the ordinal with the slot, changes at least one game of the job"""
    reqs, starts, _part = start_job()
    n_iter = 24
    want = oracle_samples_by_game(O.play_from(reqs, starts, n_iter, 6.6, 0.01, "hash")[0])
    assert _loop_samples(reqs, starts, n_iter, 6.6) == want
    # a refilled slot that took its start by SLOT: ordinal o lands on some slot < N_START_SLOTS; o % N_START_SLOTS stands for it
    by_slot = [starts[o % N_START_SLOTS] for o in range(len(starts))]
    mutants = {
        "temperature from n_moves": _loop_samples(reqs, starts, n_iter, 6.6, temperature_from="n_moves"),
        "seed from the ply": _loop_samples(reqs, starts, n_iter, 6.6, seed_from="ply"),
        "q sign from the ply": _loop_samples(reqs, starts, n_iter, 6.6, sign_from="ply"),
        "start position by slot": _loop_samples(reqs, by_slot, n_iter, 6.6),
    }
    changed = {name: sum(1 for g in want if got[g] != want[g]) for name, got in mutants.items()}
    assert all(v >= 1 for v in changed.values()), changed
    # from the empty board none of the first three can be seen
    rq = [(g, 0, 0) for g in range(1000, 1012)]
    plain = _loop_samples(rq, [(0, 0)] * len(rq), n_iter, 6.6)
    for kw in (dict(temperature_from="n_moves"), dict(seed_from="ply"), dict(sign_from="ply")):
        assert _loop_samples(rq, [(0, 0)] * len(rq), n_iter, 6.6, **kw) == plain
    evidence("start positions, twin mutants of the reference's loop (games of 495 changed): " + ", ".join(f"{k} {v}" for k, v in changed.items()))
