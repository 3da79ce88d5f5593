"""`c4a0_amd.Engine` -- GPU-resident interactive play on a hold session (C4_FLAG_HOLD): trees that persist across moves from
outside -- against tests/engine_ref.py, the oracle's MctsGame driven as the reference's InteractivePlay drives it
(rust/src/interactive_play.rs), bit for bit.  tests/test_engine_ref.py holds that reference to its floors on the oracle alone.

40 games on 40 slots (five stepping wavefronts, a partial third 16-board workgroup of the fused launch) and one run with 1 game;
tests.engine_ref.engine_positions: the empty board, won / lost / drawn roots, roots with one legal column, odd plies; the hash
evaluator and the sharp k4sat one; targets 8, 24 and 100.

  T1  search to 8, snapshot, raise to 24, snapshot: records, visit counts and statuses; no root beyond its target; terminal roots
      parked with 0 visits;
  T2  the move script (forced moves, refusals of every kind, second moves under a pending leaf) to the end of every game: the
      result codes, every snapshot and pending leaf on the way, result() == to_result sample for sample (-0.0 included);
  T3  sampled moves at temperatures 1.0, 0.5 and 0.0 against make_random_move on the oracle;
  T4  moves applied three rounds into a search, stepping eagerly;
  T5  launch forms with a sharp bf16 network: eager stand-alone step, graph replay, the fused output + step launch (eager and
      replayed): the same bytes; (the stand-alone form under the hash evaluator against the oracle is T1 / T2);
  T6  the reference's KAT `forcing_position` at 10 000 iterations, bit-equal to the oracle at all three stages;
  T7  every refused combination, and a search session and a default session created afterwards behave as before;
  T8  a match: two engines with different evaluators exchange moves over 16 games.

Without the feature every test here fails at the import of `Engine` or at `hold=True`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.engine_ref import (ACTIVE, C_PLY_PENALTY, PARKED, RefEngine, assert_forcing_thresholds, c_exploration,   # noqa: E402
                              engine_positions, forcing_position, forcing_stages, legal_columns, oracle_evaluator, run_script, uniform_evaluator)
from tests.helpers import (SHARP_MODEL_K, START_EVALS, GraphSafeHashEval, GraphSafeSharpEval, evidence, hash_eval_torch,   # noqa: E402
                           samples_by_game, sharp_eval_torch, sharp_model)

DEV = "cuda:0"
EVALS = ["hash", "k4sat"]


def _evaluator(ev_name, graph=False):
    sharp = START_EVALS[ev_name][2]
    if graph:
        return GraphSafeHashEval() if sharp is None else GraphSafeSharpEval(*sharp)
    return hash_eval_torch if sharp is None else sharp_eval_torch(*sharp)


def _engine(ev, max_n, c_expl, positions, ids=None, **kw):
    from c4a0_amd import Engine

    kw.setdefault("steps_per_graph", 0)
    return Engine(ev, max_n, c_expl, C_PLY_PENALTY, positions=positions, game_ids=ids, device=torch.device(DEV), **kw)


def _pair(ev_name, max_n, graph=False, positions=None, ids=None):
    """(Engine, RefEngine) over the same games"""
    if positions is None:
        positions, ids, _kinds = engine_positions()
    e = _engine(_evaluator(ev_name, graph), max_n, c_exploration(ev_name), positions, ids, steps_per_graph=8 if graph else 0)
    return e, RefEngine(oracle_evaluator(ev_name), max_n, c_exploration(ev_name), positions=positions, game_ids=ids)


def assert_same_state(e, r, tag, leaves=True):
    """the engine's snapshot == the reference's: every record field bit for bit, visit counts, statuses; the pending leaf of every
    active game"""
    got, want = e.snapshot(), r.snapshot()
    for name in ("game_id", "mask", "value", "meta", "policy", "q_penalty", "q_no_penalty"):
        a, b = np.ascontiguousarray(got.records[name]), np.ascontiguousarray(want.records[name])
        bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
        assert bad.size == 0, f"{tag}: {name} differs at {bad.size} games, first {int(bad[0])}: {a[bad[0]]} != {b[bad[0]]}"
    assert np.array_equal(got.visits, want.visits), (tag, got.visits, want.visits)
    assert np.array_equal(got.status, want.status), (tag, got.status, want.status)
    assert np.array_equal(got.terminal, want.terminal) and np.array_equal(got.n_moves, want.n_moves)
    if leaves:
        m, v, status = e.session.leaves()
        assert np.array_equal(status, want.status)
        ref_leaves = r.leaves()
        for i in np.flatnonzero(want.status == ACTIVE):
            assert (int(m[i]), int(v[i])) == ref_leaves[i], (tag, int(i))
    return got


def assert_same_results(e, r):
    """Engine.result() == the oracle's to_result of every finished game, sample for sample (bytes: -0.0 is not 0.0)"""
    res = e.result()
    recs, counts = res.to_records()
    got, want = samples_by_game(recs), r.result()
    assert len(res) == len(want) == int((counts > 0).sum())
    assert got == {r.ids[i]: s for i, s in want.items()}
    return int(counts.sum())


# --------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("ev_name", EVALS)
def test_search_in_instalments_and_snapshot(ev_name):
    e, r = _pair(ev_name, 24)
    assert e.session.arena() == {"bytes": 40 * (43 * 24 + 8) * 128, "blocks_per_slot": 43 * 24 + 8, "reclaim_half_blocks": 0}
    assert_same_state(e, r, "start")
    for target in (8, 24):
        rounds = e.search(target)
        r.search(target)
        s = assert_same_state(e, r, f"search({target})", leaves=False)
        assert rounds >= r.rounds and int(s.visits.max()) == target                      # no root beyond its target
        assert bool((s.status == PARKED).all())
        assert bool((s.visits[s.terminal] == 0).all()) and int(s.terminal.sum()) >= 5     # terminal roots: never searched
        assert bool((s.visits[~s.terminal] == target).all())
    e.search(24)
    assert_same_state(e, r, "again", leaves=False)                                        # nothing to do: no visit is added
    p0 = e.snapshot(player0_perspective=True).records
    assert p0.tobytes() == r.snapshot(player0_perspective=True).records.tobytes()
    assert len(e.result()) == int(s.terminal.sum())                                       # terminal starts are finished games
    assert_same_results(e, r)
    c = e.session.counters()
    assert c["error"] == 0 and c["games_done"] == int(s.terminal.sum()) and c["moves"] == 0 and c["ref_skipped_sims"] == 0
    e.close()
    evidence(f"engine T1 {ev_name}: 40 games to 8 then 24 visits == oracle bit for bit (records, visits, status), {int(s.terminal.sum())} terminal roots parked unsearched")


def test_one_game_to_100():
    positions, ids, kinds = engine_positions()
    i = kinds.index("random")
    e, r = _pair("hash", 100, positions=[positions[i]], ids=[ids[i]])
    for target in (8, 24, 100):
        e.search(target)
        r.search(target)
        s = assert_same_state(e, r, f"search({target})", leaves=False)
        assert int(s.visits[0]) == target and int(s.status[0]) == PARKED
    e.add_iterations(-50)
    e.search()
    assert int(e.snapshot().visits[0]) == 100                           # a lowered target takes no visit away and adds none
    e.close()


# --------------------------------------------------------------------------------------------- T2
@pytest.mark.parametrize("ev_name", EVALS)
def test_scripted_games_with_forced_moves(ev_name):
    e, r = _pair(ev_name, 24)
    want = []
    ref_log = run_script(r, 24, check=lambda tag: want.append((tag, r.snapshot(), r.leaves())))
    seen = [0]

    def check(tag):
        wtag, wsnap, wleaves = want[seen[0]]
        seen[0] += 1
        assert tag == wtag
        got = e.snapshot()
        assert got.records.tobytes() == wsnap.records.tobytes(), tag
        assert np.array_equal(got.visits, wsnap.visits) and np.array_equal(got.status, wsnap.status), tag
        m, v, _status = e.session.leaves()
        for i in np.flatnonzero(wsnap.status == ACTIVE):
            assert (int(m[i]), int(v[i])) == wleaves[i], (tag, int(i))

    log = run_script(e, 24, check=check)
    assert seen[0] == len(want) and [t for t, _ in log] == [t for t, _ in ref_log]
    for (tag, got), (_t, pred) in zip(log, ref_log):
        assert np.array_equal(got, pred), (tag, got, pred)                  # the results array == the prediction
    n_samples = assert_same_results(e, r)
    c = e.session.counters()
    assert c["error"] == 0 and c["games_done"] == 40 and c["moves"] == len(r.retained) and c["samples"] == n_samples
    e.close()
    codes = np.concatenate([g for _t, g in log])
    evidence(f"engine T2 {ev_name}: 40 scripted games, {len(log)} move calls ({len(r.retained)} moves, refusals "
             f"{[int((codes == k).sum()) for k in (1, 2, 3, 4)]}), {len(want)} snapshots + pending leaves and {n_samples} samples == oracle bit for bit")


def test_a_refused_move_leaves_the_slot_as_it_was():
    """the slot's state line, the arena's bump pointer and the evaluator's input row, byte for byte, across refusals of three
    kinds asked while a search is under way"""
    e, r = _pair("hash", 24)
    s = e.session
    e.search(8)
    s.set_iterations(24)
    s.hold_resume()
    s.round(e.evaluator)
    torch.cuda.synchronize()
    before = (e.snapshot().records.tobytes(), [a.tobytes() for a in s.leaves()], s.planes.cpu().numpy().tobytes(), s.counters()["select_levels"])
    snap = e.snapshot()
    cols = [7 if i % 2 else -3 for i in range(40)]
    assert not e.make_moves(cols).any()
    assert set(e.last_results.tolist()) == {1, 2}
    after = (e.snapshot().records.tobytes(), [a.tobytes() for a in s.leaves()], s.planes.cpu().numpy().tobytes(), s.counters()["select_levels"])
    assert before == after and c_no_error(s)
    assert int((snap.status == ACTIVE).sum()) >= 30
    e.close()


def c_no_error(s):
    return s.counters()["error"] == 0


# --------------------------------------------------------------------------------------------- T3
@pytest.mark.parametrize("ev_name", EVALS)
def test_sampled_moves(ev_name):
    e, r = _pair(ev_name, 24)
    per_game = np.array([(1.0, 0.5, 0.0, 2.0)[i % 4] for i in range(40)], dtype=np.float32)
    where = np.arange(40) % 3 != 0
    made = 0
    for tag, temperature, sel in (("t=1", 1.0, None), ("t=0.5", 0.5, None), ("t=0", 0.0, None), ("per game", per_game, where), ("t=1 again", 1.0, where)):
        e.search(24)
        r.search(24)
        assert_same_state(e, r, f"{tag}: search", leaves=False)
        got, pred = e.make_random_moves(temperature, sel), r.make_random_moves(temperature, sel)
        assert np.array_equal(got, pred) and np.array_equal(e.last_results, r.last_results), (tag, e.last_results, r.last_results)
        assert_same_state(e, r, tag)
        made += int(got.sum())
    assert made >= 100
    assert_same_results(e, r)
    e.close()
    evidence(f"engine T3 {ev_name}: {made} sampled moves at temperatures 1.0 / 0.5 / 0.0 / per game == make_random_move on the oracle")


# --------------------------------------------------------------------------------------------- T4
@pytest.mark.parametrize("ev_name", EVALS)
def test_moves_in_the_middle_of_a_search(ev_name):
    e, r = _pair(ev_name, 100)
    e.search(8)
    r.search(8)
    s = e.session
    e.target = r.target = 100
    s.set_iterations(100)
    s.hold_resume()
    for i in range(40):
        r._resume(i)
    for _ in range(3):                       # three of the 92 rounds needed, stepping eagerly
        s.round(e.evaluator)
        r.round()
    snap = assert_same_state(e, r, "3 rounds in")
    assert int((snap.status == ACTIVE).sum()) >= 30 and 11 <= int(snap.visits.max()) <= 15
    cols = [legal_columns(m)[i % len(legal_columns(m))] if legal_columns(m) else 0 for i, m in enumerate(snap.records["mask"])]
    got, pred = e.make_moves(cols), r.make_moves(cols)
    assert np.array_equal(got, pred) and np.array_equal(e.last_results, r.last_results) and int(got.sum()) >= 30
    assert r.moves_under_pending_leaf >= 30
    assert_same_state(e, r, "moved")
    e.search()
    r.search()
    assert_same_state(e, r, "searched on", leaves=False)
    e.close()


# --------------------------------------------------------------------------------------------- T5
def _network_script(e):
    """a short game fragment through every operation; returns every snapshot's bytes and the finished games' records"""
    out = []

    def snap():
        s = e.snapshot()
        out.append(s.records.tobytes() + s.visits.tobytes() + s.status.tobytes())
        return s

    e.search(8)
    snap()
    for t in range(3):
        s = e.snapshot()
        cols = [legal_columns(m)[(i + t) % len(legal_columns(m))] if legal_columns(m) else 0 for i, m in enumerate(s.records["mask"])]
        e.make_moves(cols)
        out.append(e.last_results.tobytes())
        e.search(24)
        snap()
        e.make_random_moves(1.0, np.arange(e.n_games) % 2 == 0)
        out.append(e.last_results.tobytes())
        e.search(16 if t == 1 else 24)
        snap()
    recs, counts = e.result().to_records()
    return out, recs.tobytes(), counts.tobytes()


class _CountingLib:
    """the library, counting the fused output + step launches asked of it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "c4_session_step_head_out":
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)

        return counted


def test_launch_forms_same_bytes():
    from c4a0_amd.nn import InferenceNet
    from c4a0_amd.session import DeviceSession

    net = InferenceNet(sharp_model(4, 32, SHARP_MODEL_K), torch.device(DEV), dtype=torch.bfloat16)
    assert net.path == "hip" and net.batch_invariant and net.fused_step_ok and net.graph_safe
    positions, ids, _kinds = engine_positions()
    outs = {}
    fused_calls = {}
    for form, spg, fuse in (("eager stand-alone", 0, False), ("graph stand-alone", 8, False), ("eager fused", 0, True), ("graph fused", 8, True)):
        e = _engine(net, 24, 6.6, positions, ids, steps_per_graph=spg)
        e.session.fuse_output_step = fuse
        assert e.session.planes.dtype == torch.bfloat16 and not e.session._timing
        lib = e.session.L
        e.session.L = counting = _CountingLib(lib)
        try:
            outs[form] = _network_script(e)
        finally:
            e.session.L = lib
        fused_calls[form] = counting.calls
        assert e.session.counters()["error"] == 0
        e.close()
    assert DeviceSession.fuse_output_step is True
    assert fused_calls["eager stand-alone"] == fused_calls["graph stand-alone"] == 0 and fused_calls["eager fused"] > 100 and fused_calls["graph fused"] >= 8
    base = outs["eager stand-alone"]
    for form, got in outs.items():
        assert got == base, form
    evidence(f"engine T5: 40 games under a sharp bf16 network, {len(base[0])} snapshots / result arrays and {len(base[1]) // 64} samples: eager stand-alone == graph == fused "
             f"({fused_calls['eager fused']} fused launches) == fused in graphs, byte for byte")


# --------------------------------------------------------------------------------------------- T6
class GraphSafeUniformEval:
    """self_play.rs:391-403 UniformEvalPos written into the bound tensors"""
    graph_safe = True
    dtype = None

    def __call__(self, planes, out_logprobs=None, out_q=None):
        if out_logprobs is None:
            g = planes.shape[0]
            return (torch.full((g, 7), float(np.float32(1.0) / np.float32(7.0)), dtype=torch.float32, device=planes.device),
                    torch.zeros((g, 2), dtype=torch.float32, device=planes.device))
        out_logprobs.fill_(float(np.float32(1.0) / np.float32(7.0)))
        out_q.zero_()
        return out_logprobs, out_q


def test_forcing_position_kat_on_the_device():
    pos = forcing_position()
    r = RefEngine(uniform_evaluator, 10_000, 4.0, 0.01, positions=[pos])
    want = forcing_stages(r)
    e = _engine(GraphSafeUniformEval(), 10_000, 4.0, [pos], blocks_per_slot=30_000, steps_per_graph=32)
    got = forcing_stages(e)
    assert_forcing_thresholds(got)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.records.tobytes() == w.records.tobytes() and np.array_equal(g.visits, w.visits), k
    c = e.session.counters()
    assert c["error"] == 0 and c["moves"] == 2 and c["sims"] == 30_000 - sum(kept for kept, _ in r.retained)
    e.close()
    evidence(f"engine T6: forcing_position at 10 000 iterations == oracle bit for bit at all three stages, visits retained {[k for k, _ in r.retained]}")


# --------------------------------------------------------------------------------------------- T7
def test_refusals_and_sessions_afterwards():
    import c4a0_amd
    from c4a0_amd import _lib
    from c4a0_amd._lib import C4Error
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.helpers import oracle_samples_by_game
    from tests.search_ref import assert_records_equal, search

    dev = torch.device(DEV)

    def refused(fn, *words):
        with pytest.raises(C4Error) as ex:
            fn()
        assert ex.value.status == _lib.ERR_BAD_ARG, ex.value
        for w in words:
            assert w in str(ex.value), (w, str(ex.value))

    refused(lambda: DeviceSession(8, 24, 6.6, 0.01, device=dev, hold=True, search=True), "C4_FLAG_HOLD", "C4_FLAG_SEARCH")
    refused(lambda: DeviceSession(8, 24, 6.6, 0.01, device=dev, hold=True, no_moves=True), "C4_FLAG_HOLD", "C4_FLAG_NO_MOVES")
    refused(lambda: DeviceSession(8, 24, 6.6, 0.01, device=dev, hold=True, reclaim=True), "C4_FLAG_HOLD", "reclaim")
    refused(lambda: DeviceSession(8, 0, 6.6, 0.01, device=dev, hold=True), "n_mcts_iterations >= 1")
    refused(lambda: DeviceSession(8, 1524, 6.6, 0.01, device=dev, hold=True), "1523")
    s = DeviceSession(8, 1400, 6.6, 0.01, device=dev, hold=True)         # above the automatic reclaim's 1 000: never reclaimed all the same
    assert s.arena()["reclaim_half_blocks"] == 0 and s.arena()["blocks_per_slot"] == 43 * 1400 + 8
    s.close()
    s = DeviceSession(8, 24, 6.6, 0.01, device=dev, hold=True)
    refused(lambda: s.set_games([(i, 0, 0) for i in range(9)]), "9 games", "8 slots")
    s.set_games([(i, 0, 0) for i in range(8)])
    s.bind()
    refused(lambda: s.set_iterations(25), "24")
    refused(lambda: s.set_iterations(0), "between 1")
    refused(lambda: s.set_dirichlet(0.3, 0.25), "C4_FLAG_HOLD")
    refused(lambda: s.set_eval_cache(1024), "C4_FLAG_HOLD")
    refused(lambda: s.bind_leaf_models(), "C4_FLAG_HOLD")
    refused(lambda: s.compact(8), "C4_FLAG_HOLD")
    inv = torch.zeros(8, dtype=torch.int32, device=dev)
    ans = torch.zeros((8, 9), dtype=torch.float32, device=dev)
    refused(lambda: _lib.check(s.L.c4_session_step_gather(s._h, C.c_void_p(inv.data_ptr()), C.c_void_p(ans.data_ptr()), 8)), "C4_FLAG_HOLD")
    rows = torch.zeros((8, 84), dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    refused(lambda: _lib.check(s.L.c4_session_unique_leaves(s._h, C.c_void_p(inv.data_ptr()), C.c_void_p(rows.data_ptr()), None, C.c_void_p(cnt.data_ptr()))), "C4_FLAG_HOLD")
    cols = torch.zeros(8, dtype=torch.int32, device=dev)
    refused(lambda: s.hold_resume(None, None, cols), "go with cols")
    s.start()                                   # ... and the session works
    s.set_iterations(8)
    s.hold_resume()
    for _ in range(10):
        s.round(hash_eval_torch)
    recs, visits, status = s.snapshot()
    assert list(visits) == [8] * 8 and list(status) == [PARKED] * 8 and s.counters()["error"] == 0
    # the arrays of c4_session_hold_resume in ordinary host memory
    host_cols = np.array([3, 7, -1, -2, 0, 1, 2, 6], dtype=np.int32)
    host_res = np.full(8, 99, dtype=np.int32)
    _lib.check(s.L.c4_session_hold_resume(s._h, host_cols.ctypes.data, None, host_res.ctypes.data))
    assert list(host_res) == [0, 2, 0, 0, 0, 0, 0, 0]
    s.close()
    plain = DeviceSession(8, 24, 6.6, 0.01, device=dev)
    for call in (lambda: plain.set_iterations(8), lambda: plain.hold_resume(), lambda: plain.snapshot(), lambda: plain.hold_poll()):
        refused(call, "not a hold session")
    plain.close()
    # a search job and a default job afterwards
    pos = [(0, 0), (0b1, 0b1), (0b10000001, 0b1), (0b1111, 0b1111)]
    got = c4a0_amd.search_positions(pos, 16, 6.6, 0.01, evaluator=hash_eval_torch)
    assert_records_equal(got.records, search(pos, 16, oracle_evaluator("hash"), 6.6), pos)
    reqs = [c4a0_amd.GameMetadata(500 + i, 0, 0) for i in range(12)]
    games = c4a0_amd.play_games(reqs, 64, 10, 6.6, 0.01, evaluator=hash_eval_torch, resident_games=8)
    want, _ = O.self_play([(500 + i, 0, 0) for i in range(12)], 64, 10, 6.6, 0.01, "hash")
    assert samples_by_game(games.to_records()[0]) == oracle_samples_by_game(want)


# --------------------------------------------------------------------------------------------- T8
def test_a_match_between_two_engines():
    """engine A (hash evaluator) moves on even plies, engine B (k4sat) on odd ones; both search their own tree every turn, the
    mover's best column (the first maximum of its root policy) is made on both"""
    positions, ids = [(0, 0)] * 16, [7_700 + 3 * i for i in range(16)]
    ea, ra = _pair("hash", 24, positions=positions, ids=ids)
    eb, rb = _pair("k4sat", 24, positions=positions, ids=ids)

    def play(a, b):
        moves = []
        for turn in range(43):
            a.search(24)
            b.search(24)
            mover = a if turn % 2 == 0 else b
            s = mover.snapshot()
            if bool(s.terminal.all()):
                break
            cols = np.where(s.terminal, -1, np.argmax(s.records["policy"], axis=1))
            ok_a, ok_b = a.make_moves(cols), b.make_moves(cols)
            assert np.array_equal(ok_a, ok_b) and np.array_equal(ok_a, ~s.terminal)
            moves.append(cols.tolist())
        else:
            raise AssertionError("a game of Connect Four has 42 plies")
        return moves

    want = play(ra, rb)
    got = play(ea, eb)
    assert got == want and len(got) >= 7
    n = assert_same_results(ea, ra)
    assert assert_same_results(eb, rb) == n
    assert ea.result().to_records()[0].tobytes() != b"" and len(ea.result()) == 16
    assert ea.session.counters()["error"] == 0 and eb.session.counters()["error"] == 0
    ea.close()
    eb.close()
    evidence(f"engine T8: 16 games between two engines (hash vs k4sat), {len(got)} plies, move lists and {n} samples per side == two oracle games driven the same way")
