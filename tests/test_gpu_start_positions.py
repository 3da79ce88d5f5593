"""Whole games from given start positions (c4_session_set_games' start_masks / start_values, MctsGame::new_from_pos, mcts.rs:48-56)
on the device against the oracle, bit for bit.  From the empty board the ply of the root and the number of moves a game has
recorded are one number, and every other whole-game test starts there; the step kernel keeps them apart as the reference does --
popcount(root) for the temperature, the ply penalty and the leaf's model; n_moves for the move seed, the key of the Dirichlet stream,
the record index and the sign of every sample's q -- and a kernel that read the wrong one passes all of those tests.  Here the job
of tests.helpers.start_job (495 games on 128 slots: odd-ply, late and terminal starts, lines that end drawn on the full board;
tests/test_start_positions.py holds it to its floors on the oracle alone) goes through

  T1      every launch form of DeviceSession under the hash and sharp evaluators (tests.helpers.START_JOBS): eager, HIP graph, bf16
          and f32 planes, evaluation cache, Dirichlet noise, reclaimed arenas, compact() during the tail, the gather step kernel
          (c4_session_unique_leaves + c4_session_step_gather); pack_samples_device() == drain_samples() on the way;
  models  leaf_models after start() and after every step of a run with two players, slot by slot;
  T3      the sharpened bf16 4 x 32 network: an eager run logs every evaluator row, the oracle replays the job from those answers,
          and the fused output + step launch in a HIP graph must return the same bytes; once more with the f32 chain;
  ends    a session of terminal starts alone (kinds 1, 2, 3), more games than slots.

What the reference does with a terminal start is n simulations on a terminal root and one sample; the device closes the game in
the first launch that sees it and counts the n simulations in ref_skipped_sims.  The kernel before this file ran them and counted
them in sims / backup_nodes: against it the T1 cases and both terminal-start cases fail on `ref_skipped_sims == sims_terminal_root`
(0 against 2 160 for the 90 terminal starts at n = 24) with every sample equal -- the one mismatch the file found.

Measured on one MI355X: the file's 19 cases take 6.6 s together, the slowest 1.1 s.  tests/test_start_positions.py shows on the
oracle alone that the job tells the ply from n_moves (twin mutants of the reference's loop: temperature from n_moves changes 279
of the 495 games, the seed from the ply 312, the q sign from the ply 196, the start taken by slot 367)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import (N_START_SLOTS, START_EVALS, START_JOBS, GraphSafeHashEval, GraphSafeSharpEval, evidence, hash_eval_np,   # noqa: E402
                           hash_eval_torch, oracle_samples_by_game, samples_by_game, sharp_eval_np, sharp_eval_torch, start_job)

DEV = "cuda:0"
_ORACLE = {}


def _oracle(ev_name, n_iter, noise=None):
    """the oracle's games of the job under one setting, computed once and shared: (samples by game, counts in request order, statistics)"""
    key = (ev_name, n_iter, noise)
    if key not in _ORACLE:
        from oracle import c4oracle as O

        reqs, starts, _part = start_job()
        ev, c_expl, _ = START_EVALS[ev_name]
        res, st = O.play_from(reqs, starts, n_iter, c_expl, 0.01, ev, dirichlet=noise or (0.0, 0.0))
        _ORACLE[key] = (oracle_samples_by_game(res), [len(res[g]) for g, _a, _b in reqs], st)
    return _ORACLE[key]


def _evaluator(ev_name, form):
    sharp = START_EVALS[ev_name][2]
    if form == "graph":
        return GraphSafeHashEval() if sharp is None else GraphSafeSharpEval(*sharp)
    if form == "numpy":
        return hash_eval_np if sharp is None else sharp_eval_np(*sharp)
    return hash_eval_torch if sharp is None else sharp_eval_torch(*sharp)


def _check_records(recs, counts, want, want_counts):
    got = samples_by_game(recs)
    assert set(got) == set(want)
    for gid in want:
        assert got[gid] == want[gid], f"game {gid} differs"
    assert np.array_equal(counts, want_counts)
    # meta = the record's index in its game | terminal flag << 16 (c4a0_hip.h): the index is n_moves, not the ply
    order = np.lexsort((recs["meta"] & 0xFFFF, recs["game_id"]))
    r = recs[order]
    first = np.r_[True, r["game_id"][1:] != r["game_id"][:-1]]
    last = np.r_[first[1:], True]
    idx = np.arange(len(r)) - np.maximum.accumulate(np.where(first, np.arange(len(r)), 0))
    assert np.array_equal(r["meta"] & 0xFFFF, idx) and np.array_equal((r["meta"] >> 16) & 1, last.astype(np.uint32))


def _run_compacting(s, ev, every, n_games):
    """eager rounds with compact(8) every `every`-th step (a no-op while requests are queued, then it narrows the tail)"""
    s.bind()
    s.start()
    widths = []
    for step in range(1, 100_000):
        s.evaluate(ev)
        s.step()
        if step % every == 0:
            act, rows = s.compact(8)
            widths.append(rows)
            assert act <= rows == s.rows and rows % 8 == 0
            if s.counters()["games_done"] >= n_games:
                break
    assert widths[0] == N_START_SLOTS and widths[-1] == 8 and sorted(widths, reverse=True) == widths
    return widths


def _run_gather(s, np_eval):
    """the callback mode's round, driven directly: c4_session_unique_leaves builds the batch of distinct leaves in pinned host
    memory, the answers go back inside the step's launch (c4_session_step_gather)"""
    from c4a0_amd._lib import check

    g = s.n_slots
    s.bind()
    s.start()
    inverse = torch.zeros(g, dtype=torch.int32, device=s.device)
    h_planes = torch.zeros((g, 2, 6, 7), dtype=torch.float32).pin_memory()
    h_count = torch.zeros(1, dtype=torch.int32).pin_memory()
    h_out = torch.zeros((g, 9), dtype=torch.float32).pin_memory()
    rows = 0
    for _ in range(100_000):
        check(s.L.c4_session_unique_leaves(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(h_planes.data_ptr()), None, C.c_void_p(h_count.data_ptr())))
        s._bound_stream.synchronize()
        n_u = int(h_count[0])
        if n_u == 0:   # every game has finished
            return rows
        lp, qp, qn = np_eval(0, h_planes.numpy()[:n_u])
        out = h_out.numpy()   # the previous launch that read it precedes the synchronisation above
        out[:n_u, :7], out[:n_u, 7], out[:n_u, 8] = lp, qp, qn
        check(s.L.c4_session_step_gather(s._h, C.c_void_p(inverse.data_ptr()), C.c_void_p(h_out.data_ptr()), n_u))
        rows += n_u
    raise AssertionError("the job did not end")


# --------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("job", START_JOBS, ids=[j[0] for j in START_JOBS])
def test_games_from_start_positions_bit_identical(job):
    """T1: every sample of every game, the per-game counts and the work counters equal the oracle's; 495 games on 128 slots, so
    three starts in four are handed to a refilled slot."""
    from c4a0_amd.session import SAMPLE_DTYPE, DeviceSession
    from tests.test_gpu_reclaim import _half_min
    from tests.test_gpu_sharp_regime import _assert_counters

    name, ev_name, n, planes, opt = job
    reqs, starts, _part = start_job()
    c_expl = START_EVALS[ev_name][1]
    noise = opt.get("dirichlet")
    want, want_counts, ost = _oracle(ev_name, n, noise)
    kw = {}
    if "reclaim" in opt:      # the tightest halves the library accepts, looked at every `period`-th launch
        kw = dict(reclaim=True, reclaim_period=opt["reclaim"], blocks_per_slot=2 * _half_min(n, opt["reclaim"]))
    s = DeviceSession(N_START_SLOTS, n, c_expl, 0.01, device=torch.device(DEV), planes_dtype=torch.float32 if planes == "f32" else torch.bfloat16, **kw)
    s.set_games(reqs, starts)
    if noise:
        s.set_dirichlet(*noise)
    if "cache" in opt:
        s.set_eval_cache(*opt["cache"])
    extra = ""
    if "graph" in opt:
        s.run(_evaluator(ev_name, "graph"), steps_per_graph=opt["graph"])
    elif "compact" in opt:
        widths = _run_compacting(s, _evaluator(ev_name, "eager"), opt["compact"], len(reqs))
        extra = f", widths {sorted(set(widths), reverse=True)}"
    elif "gather" in opt:
        rows = _run_gather(s, _evaluator(ev_name, "numpy"))
        assert 0 < rows < ost["sims"]
        extra = f", {rows} distinct leaves answered"
    else:
        s.run(_evaluator(ev_name, "eager"))
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    packed = s.pack_samples_device().cpu().numpy().reshape(-1).view(SAMPLE_DTYPE)
    s.close()
    _check_records(recs, counts, want, want_counts)
    assert packed.tobytes() == recs.tobytes()
    assert c["games_done"] == c["games_started"] == len(reqs) and c["samples"] == ost["n_samples"] == len(recs)
    _assert_counters(c, ost)
    if "cache" in opt:
        assert 0 < c["eval_cache_hits"] <= c["eval_cache_probes"]
        extra += f", {c['eval_cache_hits']} cache hits"
    if "reclaim" in opt:
        assert c["reclaim_passes"] > 0, "the job does not need its arenas reclaimed"
        extra += f", {c['reclaim_passes']} reclaim passes"
    evidence(f"start positions T1 {name}: {len(reqs)} games, {len(recs)} samples == oracle bit for bit, packed == drained, counters equal "
             f"({c['sims']} sims + {c['ref_skipped_sims']} skipped, {c['moves']} moves){extra}")


# --------------------------------------------------------------------------------------------- leaf models
def test_leaf_models_follow_the_ply_of_the_leaf_on_every_slot():
    """mcts.rs:70-76: player 0's model evaluates leaves of even ply, player 1's of odd ply -- the ply of the LEAF, whatever the
    game has played.  One simulation per game per step, so that a step is one c4o_game_step; the oracle's game of every slot is
    stepped beside the device, and after start() and every step each slot's leaf and leaf_models entry must be the oracle's."""
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O

    reqs, starts, _part = start_job()
    n_iter, n_steps = 24, 160
    s = DeviceSession(N_START_SLOTS, n_iter, 6.6, 0.01, device=torch.device(DEV), one_sim_per_step=True)
    s.set_games(reqs, starts)
    models = s.bind_leaf_models()
    s.bind()
    s.start()
    games, seen, checked, odd, refilled = {}, set(), 0, 0, 0
    for step in range(n_steps + 1):
        if step:
            s.evaluate(hash_eval_torch)
            s.step()
        mask, value, status, ordinal = s.leaves(with_ordinals=True)
        got = models.cpu().numpy().view(np.uint64)
        for g in range(N_START_SLOTS):
            if status[g] != 1:   # the request list is exhausted
                assert step > 0
                games.pop(g, None)
                continue
            o = int(ordinal[g])
            if g not in games or games[g][0] != o:      # a new game on the slot: its leaf is its start position
                assert o not in seen and (o == g if step == 0 else o >= N_START_SLOTS)
                seen.add(o)
                refilled += step > 0
                games[g] = (o, O.Game(O.Pos(*starts[o]), *reqs[o]))
            else:
                og = games[g][1]
                leaf = og.leaf_pos()
                assert og.step(*O.hash_eval_pos(leaf.mask, leaf.value), n_iter, 6.6, 0.01) == 0, (step, g, o)
            og = games[g][1]
            assert og.leaf_pos().key() == (int(mask[g]), int(value[g])), (step, g, o)
            assert int(got[g]) == og.leaf_model_id() == reqs[o][1 + (bin(int(mask[g])).count("1") & 1)], (step, g, o)
            checked += 1
            odd += bin(int(mask[g])).count("1") & 1
    c = s.counters()
    s.close()
    assert c["error"] == 0 and refilled >= N_START_SLOTS and odd >= checked // 4
    evidence(f"start positions, leaf models: {checked} (slot, step) pairs over {n_steps} steps == c4o_game_leaf_model_id, leaf positions too; "
             f"{odd} leaves at odd ply, {refilled} games on refilled slots")


# --------------------------------------------------------------------------------------------- T3
def _t3(net, planes_dtype):
    """the eager run (separate output and step launches) logs every evaluator row; the oracle replays the job from those answers"""
    from oracle import c4oracle as O
    from tests.test_gpu_baseline_configs import _run_logging_every_row
    from tests.test_gpu_sharp_regime import _assert_counters

    reqs, starts, _part = start_job()
    reqs = [(g, 0, 0) for g, _a, _b in reqs]
    recs, counts, ctr, table, (n_rows, _n_dup) = _run_logging_every_row(net, [g for g, _a, _b in reqs], N_START_SLOTS, 100, planes_dtype=planes_dtype, starts=starts)
    assert ctr["games_done"] == len(reqs) and ctr["error"] == 0
    ores, ost = O.play_from(reqs, starts, 100, 6.6, 0.01, ("table",) + table)
    _check_records(recs, counts, oracle_samples_by_game(ores), [len(ores[g]) for g, _a, _b in reqs])
    _assert_counters(ctr, ost)
    return reqs, starts, recs, counts, n_rows


def test_fused_launch_from_start_positions_t3(monkeypatch):
    """sharp_model(4, 32) as a bf16 InferenceNet: T3, then the same job through HIP graphs of the fused output + step launch
    (c4_session_step_head_out) -- the same bytes."""
    from c4a0_amd.session import DeviceSession
    from tests.test_gpu_sharp_regime import _sharp_net

    net = _sharp_net(4, 32)
    assert net.gemm == "hip" and net.fused_step_ok
    reqs, starts, recs, counts, n_rows = _t3(net, torch.bfloat16)
    for spg in (2, 16):
        s = DeviceSession(N_START_SLOTS, 100, 6.6, 0.01, device=torch.device(DEV), planes_dtype=torch.bfloat16)
        fused = []
        entry = s.L.c4_session_step_head_out
        monkeypatch.setattr(s.L, "c4_session_step_head_out", lambda *a: (fused.append(1), entry(*a))[1])
        s.set_games(reqs, starts)
        s.run(net, steps_per_graph=spg)
        r2, c2 = s.drain_samples(), s.sample_counts()
        s.close()
        monkeypatch.undo()
        assert len(fused) == spg, "the graph did not capture the fused launch"
        assert r2.tobytes() == recs.tobytes() and np.array_equal(c2, counts), spg
    evidence(f"start positions T3, bf16 4x32 sharpened network: {len(reqs)} games, {len(recs)} samples == oracle replay of {n_rows} logged "
             f"evaluator rows; fused output + step launch in graphs of 2 and 16 rounds byte-identical")


def test_f32_chain_from_start_positions_t3():
    from tests.test_gpu_sharp_regime import _sharp_net

    net = _sharp_net(4, 32, dtype=torch.float32, hip_tower=True, strict=True)
    reqs, _starts, recs, _counts, n_rows = _t3(net, torch.float32)
    evidence(f"start positions T3, f32 4x32 sharpened network: {len(reqs)} games, {len(recs)} samples == oracle replay of {n_rows} logged rows")


# --------------------------------------------------------------------------------------------- terminal starts
@pytest.mark.parametrize("graph", [0, 2], ids=["eager", "graph"])
def test_a_session_of_terminal_starts_alone(graph):
    """every game's start is terminal (kinds 1, 2, 3), 90 games on 16 slots: the session finishes, every game yields its one record
    -- the start position, the uniform policy, the terminal value -- and the n simulations the reference runs on each such root
    are the device's ref_skipped_sims"""
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.test_gpu_sharp_regime import _assert_counters

    _reqs, all_starts, _part = start_job()
    starts = [p for p in all_starts if O.terminal_state(O.Pos(*p)) != 0] * 2
    kinds = [O.terminal_state(O.Pos(*p)) for p in starts]
    assert len(starts) == 90 and {1, 2, 3} == set(kinds)
    reqs = [(g, 0, 0) for g in [0, 42, 43, 1 << 40, (1 << 64) - 1] + list(range(500, 585))]
    n_iter = 24
    ores, ost = O.play_from(reqs, starts, n_iter, 6.6, 0.01, "hash")
    s = DeviceSession(16, n_iter, 6.6, 0.01, device=torch.device(DEV))
    s.set_games(reqs, starts)
    steps = s.run(GraphSafeHashEval() if graph else hash_eval_torch, steps_per_graph=graph, max_steps=4000)
    recs, counts, c = s.drain_samples(), s.sample_counts(), s.counters()
    s.close()
    assert c["games_done"] == len(reqs) == len(recs) and steps < 4000
    _check_records(recs, counts, oracle_samples_by_game(ores), [1] * len(reqs))
    assert np.array_equal(np.ascontiguousarray(recs["policy"]).view(np.uint32), np.full((len(reqs), 7), np.float32(1.0) / np.float32(7.0), dtype=np.float32).view(np.uint32))
    by_id = {int(r["game_id"]): r for r in recs}
    for (g, _a, _b), p in zip(reqs, starts):
        _t, qp, qn = O.terminal_value(O.Pos(*p), 0.01)
        r = by_id[g]
        assert (int(r["mask"]), int(r["value"])) == p and r["meta"] == 1 << 16
        assert np.float32(r["q_penalty"]).tobytes() == np.float32(qp).tobytes() and np.float32(r["q_no_penalty"]).tobytes() == np.float32(qn).tobytes()
    _assert_counters(c, ost)
    assert c["ref_skipped_sims"] == ost["sims_terminal_root"] == n_iter * len(reqs) and c["moves"] == 0
    evidence(f"start positions, terminal starts alone ({'graph' if graph else 'eager'}): {len(reqs)} games of kinds {sorted(set(kinds))} on 16 slots, "
             f"one record each == oracle, {c['ref_skipped_sims']} skipped simulations == the oracle's terminal-root simulations, {steps} steps")
