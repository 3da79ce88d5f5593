"""The regime a trained network puts the tree in -- peaked priors, saturated values -- on the CPU: the sharp evaluators' twins agree
bit for bit, the oracle's depth counters equal their derivation through the Game API, and the oracle ALONE, on exactly the jobs
tests/test_gpu_sharp_regime.py plays on the device, reaches the code the hash evaluator and a default-initialised network do not:
path levels 16..42 (the slot's second line), priors of exactly 0 and subnormal ones, moves that follow a move with no search
between (VERDICT weak 5).  The floors are conditions on the test jobs, set well under what the oracle measures (32 games, n = 100,
logits x 16: 40 % of the simulations at depth >= 16, 35 % ending on a terminal leaf, max depth 32, 46 % / 52 % of the used rows
with a zero / subnormal legal prior, 86 of 652 moves straight after a move; the hash evaluator itself: 0.02 %, depth 17, none)."""
import numpy as np
import pytest

from oracle import c4oracle as O
from tests.helpers import (N_SHARP_GAMES, SHARP_EVALS, SHARP_JOBS, SHARP_MODEL_K, sharp_eval_np, sharp_job_reqs, sharp_model)

# the constant evaluator of the line KAT (found by random search on the oracle): the search from the empty board walks one line
# to the full board -- 42 levels, every level of Slot::path_deep -- within 500 iterations
LINE_KAT = dict(logits=[-6.0, 0.0, -4.25, 7.75, 6.25, 7.0, 4.0], q=(1.0, 1.0), c_exploration=1.4, c_ply_penalty=0.01)
LINE_KAT_ITERATIONS = (200, 500, 1500)


def _planes(mask: np.ndarray, value: np.ndarray) -> np.ndarray:
    """c4r.rs:378-392 for arrays of positions -> float32[B, 2, 6, 7]"""
    bits = np.arange(42, dtype=np.uint64)[None, :]
    p0 = ((value[:, None] >> bits) & np.uint64(1)).astype(np.float32)
    p1 = (((mask & ~value)[:, None] >> bits) & np.uint64(1)).astype(np.float32)
    return np.concatenate([p0, p1], axis=1).reshape(-1, 2, 6, 7)


@pytest.mark.parametrize("name", sorted(SHARP_EVALS))
def test_sharp_evaluator_twins_agree_bit_for_bit(name):
    """numpy twin == torch twin (CPU tensors) == c4o_eval_sharp on 120 000 reachable positions, for every parameter set the GPU
    file uses; and the parameters do what they say (exact scaling of the hash logits, sign(q), seven equal logits on h % 8 == 0)."""
    torch = pytest.importorskip("torch")
    from tests.helpers import _hash_h_np, hash_eval_np, sharp_eval_torch

    (k, q_mode, ties), _c = SHARP_EVALS[name]
    mask, value = O.random_positions_np(120_000, seed=7 + k)
    x = _planes(mask, value)
    lp_n, qp_n, qn_n = sharp_eval_np(k, q_mode, ties)(0, x)
    lp_t, q_t = sharp_eval_torch(k, q_mode, ties)(torch.from_numpy(x))
    lp_c, qp_c, qn_c, tally = O.sharp_eval_batch(x, k, q_mode, ties)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert lp_t.dtype == torch.float32 and q_t.dtype == torch.float32
    for a, b in ((lp_n, lp_c), (qp_n, qp_c), (qn_n, qn_c), (lp_t.numpy(), lp_c), (q_t[:, 0].numpy(), qp_c), (q_t[:, 1].numpy(), qn_c)):
        assert np.array_equal(bits(a), bits(b))
    assert tally["rows"] == len(x)
    h_lp, h_qp, h_qn = hash_eval_np(0, x)
    tied = (_hash_h_np(x) % 8 == 0) if ties else np.zeros(len(x), dtype=bool)
    assert np.array_equal(lp_c[~tied].astype(np.float64), h_lp[~tied].astype(np.float64) * 2.0 ** k)   # exact in f32: no rounding happened
    if ties:
        assert 0.08 < tied.mean() < 0.17 and np.all(lp_c[tied] == 0.0)
    if q_mode == "sat":
        assert np.array_equal(qp_c, np.sign(h_qp)) and np.array_equal(qn_c, np.sign(h_qn)) and set(np.unique(qp_c)) == {-1.0, 0.0, 1.0}
    else:
        assert np.array_equal(bits(qp_c), bits(h_qp)) and np.array_equal(bits(qn_c), bits(h_qn))
    # the evaluator's own tallies against the oracle's softmax, row by row, on a slice
    zero = sub = used = 0
    for i in range(3000):
        p = O.Pos(int(mask[i]), int(value[i]))
        if O.terminal_state(p) != 0:
            continue
        legal = O.legal_mask(p)
        pr = O.softmax7([float(v) if (legal >> c) & 1 else float("-inf") for c, v in enumerate(lp_c[i])])
        pl = pr[[c for c in range(7) if (legal >> c) & 1]]
        used += 1
        zero += bool((pl == 0.0).any())
        sub += bool(((pl > 0.0) & (pl < np.finfo(np.float32).tiny)).any())
    t3 = O.sharp_eval_batch(x[:3000], k, q_mode, ties)[3]
    assert (t3["rows_used"], t3["rows_zero_prior"], t3["rows_subnormal_prior"]) == (used, zero, sub)


def test_depth_counters_equal_their_derivation_through_the_game_api():
    """sims_deep, sims_deep_terminal, max_depth and moves_without_search from what the Game API shows from outside: the depth of the
    leaf a c4o_game_step call backs up from is the select_levels delta of the select that found it (the previous call's; after a
    move, the part of the delta that was not discarded), its kind is terminal_state(leaf_pos), a move is an n_moves delta.  The sums
    over the games equal c4o_self_play's and c4o_self_play_async's statistics for the same games."""
    (k, q_mode, ties), c_expl = SHARP_EVALS["k4sat"]
    ev = sharp_eval_np(k, q_mode, ties)
    n_iter, gids = 120, [0, 42, 1001, 1002, 1003, 1 << 40]
    want = dict(sims_deep=0, sims_deep_terminal=0, max_depth=0, moves_without_search=0)
    for gid in gids:
        g = O.Game(game_id=gid)
        mine = dict(sims_deep=0, sims_deep_terminal=0, max_depth=0, moves_without_search=0)
        leaf_depth, prev_moved = 0, False
        for _ in range(100_000):
            before, leaf, nm = g.counters(), g.leaf_pos(), g.n_moves()
            mine["max_depth"] = max(mine["max_depth"], leaf_depth)
            if leaf_depth >= 16:
                mine["sims_deep"] += 1
                mine["sims_deep_terminal"] += O.terminal_state(leaf) != 0
            lp, qp, qn = ev(0, O.planes(leaf)[None])
            r = g.step(lp[0], float(qp[0]), float(qn[0]), n_iter, c_expl, 0.01)
            assert r >= 0
            after = g.counters()
            d_sel = after["select_levels"] - before["select_levels"]
            d_disc = after["select_levels_discarded"] - before["select_levels_discarded"]
            moved = g.n_moves() > nm
            leaf_depth = d_sel - d_disc if moved else d_sel
            mine["moves_without_search"] += moved and prev_moved
            prev_moved = moved
            if r == 1:
                break
        c = g.counters()
        assert {x: c[x] for x in mine} == mine, gid
        for x in mine:
            want[x] = max(want[x], mine[x]) if x == "max_depth" else want[x] + mine[x]
    assert want["sims_deep"] > 200 and want["sims_deep_terminal"] > 100 and want["max_depth"] >= 24 and want["moves_without_search"] > 5
    reqs = [(g, 0, 0) for g in gids]
    for topology, threads in (("lockstep", 1), ("async", 3)):
        for evaluator in (("sharp", k, q_mode, ties), ev):
            _res, st = O.self_play(reqs, 64, n_iter, c_expl, 0.01, evaluator, n_threads=threads, topology=topology)
            assert {x: st[x] for x in want} == want, (topology, evaluator)


@pytest.mark.parametrize("job", SHARP_JOBS, ids=[j[0] for j in SHARP_JOBS])
def test_oracle_alone_reaches_the_coverage_floors_on_the_gpu_matrix(job):
    """Each job of the device matrix, played by the oracle alone: it must be IN the regime (floors from the issue; the parameters
    bend, the floors do not).  rows_used = the evaluator's rows whose answer the tree used (a terminal leaf's answer is ignored)."""
    name, ev_name, n, _planes_dtype, first_id, opt = job
    ev, c_expl = SHARP_EVALS[ev_name]
    _res, st = O.self_play(sharp_job_reqs(first_id), 4096, n, c_expl, 0.01, ("sharp",) + ev, n_threads=4, topology="async",
                           dirichlet=opt.get("dirichlet", (0.0, 0.0)))
    assert st["n_games"] == N_SHARP_GAMES >= 512
    print(name, {x: st[x] for x in ("sims", "sims_deep", "sims_deep_terminal", "max_depth", "moves", "moves_without_search",
                                    "rows_used", "rows_zero_prior", "rows_subnormal_prior")})
    if n >= 100:
        assert st["sims_deep"] >= 0.10 * st["sims"]
        assert st["sims_deep_terminal"] >= 0.05 * st["sims"]
        assert st["max_depth"] >= 24
        assert st["moves_without_search"] >= 0.05 * st["moves"]
    assert st["rows_zero_prior"] >= 0.25 * st["rows_used"] and st["rows_subnormal_prior"] >= 0.25 * st["rows_used"]


def test_matrix_holds_what_it_has_to():
    """every evaluator, every n, both plane types, and each extension and launch form somewhere (the product is not needed)"""
    assert {j[1] for j in SHARP_JOBS} == set(SHARP_EVALS) and {j[2] for j in SHARP_JOBS} == {24, 100, 400}
    assert {j[3] for j in SHARP_JOBS} == {"f32", "bf16"} and len({j[0] for j in SHARP_JOBS}) == len(SHARP_JOBS)
    opts = [j[5] for j in SHARP_JOBS]
    assert any(o.get("dirichlet") == (0.3, 0.25) and "cache" not in o for o in opts)
    assert any(o.get("cache") == (1024, 8) for o in opts) and any(o.get("cache", (0,))[0] >= 1 << 16 and "dirichlet" not in o for o in opts)
    assert any("dirichlet" in o and "cache" in o for o in opts)
    assert {o["reclaim"] for o in opts if "reclaim" in o} == {1, 3}
    assert any("graph" in o for o in opts) and any(not o for o in opts) and any(o.get("callback") for o in opts)


def test_line_kat_reaches_the_bottom_of_the_board():
    """Constant logits whose search from the empty board goes down ONE line to the full board: 42 levels, every entry of the deep
    path, at 500 and at 1 500 iterations (24 levels at 200)."""
    depths = {}
    for n in LINE_KAT_ITERATIONS:
        _pol, _qp, _qn, g = O.run_mcts(O.Pos(0, 0), n, LINE_KAT["c_exploration"], LINE_KAT["c_ply_penalty"], LINE_KAT["logits"], LINE_KAT["q"])
        c = g.counters()
        depths[n] = c["max_depth"]
        assert c["sims"] == n
    assert depths[200] >= 16 and depths[500] >= 40 and depths[1500] >= 40, depths
    pr = O.softmax7(LINE_KAT["logits"])
    assert (pr > 0).all() and pr.max() < 0.6          # nothing underflows here: the line is deep because q = +1 pulls it down


def test_sharpened_network_searches_deep():
    """sharp_model(4, 32, k) as the oracle's callback evaluator (the f32 PyTorch model), 32 games at n = 100: at least 10 % of the
    simulations back up from depth >= 16 (measured: 15.7 % at k = 8, 29 % at k = 9, 38 % at k = 10; 2.4 select levels per
    simulation unsharpened).  SHARP_MODEL_K is what the GPU file uses."""
    torch = pytest.importorskip("torch")
    model = sharp_model(4, 32, SHARP_MODEL_K)
    base = sharp_model(4, 32, 0)
    with torch.no_grad():   # powers of two: the sharpened output layers are exact scalings, also after rounding to bf16
        assert torch.equal(model.fc_policy[-2].weight.bfloat16().float(), base.fc_policy[-2].weight.bfloat16().float() * 2.0 ** SHARP_MODEL_K)
        assert torch.equal(model.fc_policy[-2].bias, base.fc_policy[-2].bias * 2.0 ** SHARP_MODEL_K)
        assert torch.equal(model.fc_value[-2].weight, base.fc_value[-2].weight * 2.0 ** (SHARP_MODEL_K // 2))

    def cb(_model_id, x):
        with torch.no_grad():
            lp, a, b = model(torch.from_numpy(x))
        return lp.numpy(), a.numpy().copy(), b.numpy().copy()

    _res, st = O.self_play([(g, 0, 0) for g in range(32)], 4096, 100, 6.6, 0.01, cb)
    print({x: st[x] for x in ("sims", "sims_deep", "sims_deep_terminal", "max_depth", "select_levels", "moves", "moves_without_search")})
    assert 8 <= SHARP_MODEL_K <= 10 and st["sims_deep"] >= 0.10 * st["sims"]
