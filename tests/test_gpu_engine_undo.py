"""`Engine.undo_moves` / `Engine.reset_games` (c4_session_hold_undo: MctsGame::undo_move / reset_game, mcts.rs:225-245, on a hold
session) against tests/engine_undo_ref.py, bit for bit.  tests/test_engine_undo_ref.py holds that model to the oracle.

Shapes and evaluators are tests/test_gpu_engine.py's: the 40 games of engine_positions (five stepping wavefronts, a partial third
16-board workgroup of the fused launch) and one game alone; targets 8 and 24; the hash evaluator and the sharp k4sat one.

  U1  scripted games with undos on the way (a third of the games after every turn, finished ones among them), to the end of every
      game: result codes, every snapshot and pending leaf, result() sample for sample (-0.0 included), the counters;
  U2  refusals: undo and reset before any move (code 6, the slot byte for byte as it was, the search goes on as an untouched
      engine's), a request that is none (code 7), a terminal start position keeps its one sample;
  U3  finished games undone: out of result(), sample count 0, games_done and samples down by their share in the counters and in
      the polled word; replayed: finished again, records == the model's;
  U4  reset: the games equal a fresh Engine's on the same positions, device against device, and the model; the others unaffected;
  U5  sampled moves after an undo at temperatures 1.0, 0.5, 0.0 (the five special ids among the games): the shortened move count seeds;
  U6  an undo three eager rounds into a search, under a pending leaf;
  U7  launch forms with a sharp bf16 network: eager / graph replay x stand-alone step / fused output + step: the same bytes, and
      the graph captured before the first undo is the one replayed after it;
  U8  the arena is given back: 60 cycles of search, move, search, undo in an arena of 1 040 blocks;
  U9  argument errors, arrays in ordinary host memory, and a hold session afterwards.

Without the feature every test here fails at `Engine.undo_moves` or at `hold_undo`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.engine_ref import ACTIVE, PARKED, c_exploration, engine_positions, legal_columns, oracle_evaluator   # noqa: E402
from tests.engine_undo_ref import (REFUSED_NO_MOVES, REFUSED_REQUEST, UNDO_ALL, UNDO_NONE, UNDO_ONE, RefEngineUndo,   # noqa: E402
                                   run_undo_script)
from tests.helpers import SHARP_MODEL_K, evidence, hash_eval_torch, sharp_model   # noqa: E402
from tests.test_gpu_engine import DEV, _engine, _evaluator, assert_same_results, assert_same_state   # noqa: E402

SPECIAL_IDS = (0, 42, 43, 1 << 40, 2 ** 64 - 1)


def _pair(ev_name, max_n, positions=None, ids=None):
    """(Engine, RefEngineUndo) over the same games"""
    if positions is None:
        positions, ids, _kinds = engine_positions()
    e = _engine(_evaluator(ev_name), max_n, c_exploration(ev_name), positions, ids)
    return e, RefEngineUndo(oracle_evaluator(ev_name), max_n, c_exploration(ev_name), positions=positions, game_ids=ids)


def _both(e, r, op, *a):
    """the same call on the engine and on the model: same answer, same result codes"""
    got, want = getattr(e, op)(*a), getattr(r, op)(*a)
    assert np.array_equal(got, want), (op, got, want)
    assert np.array_equal(e.last_results, r.last_results), (op, e.last_results, r.last_results)
    return got


def _walk(snap, t):
    return [legal_columns(m)[(i + t) % len(legal_columns(m))] if legal_columns(m) else 0 for i, m in enumerate(snap.records["mask"])]


def _turn(e, r, t, target=24):
    e.search(target)
    r.search(target)
    return _both(e, r, "make_moves", _walk(r.snapshot(), t))


def _polled_done(s):
    """the polled games_done word as it stands now (the probe is asynchronous: ask, wait, take)"""
    s.poll()
    torch.cuda.synchronize()
    s.poll()
    torch.cuda.synchronize()
    return s.poll()[0]


# --------------------------------------------------------------------------------------------- U1
def _scripted(e, r, target):
    want = []
    ref_log = run_undo_script(r, target, check=lambda tag: want.append((tag, r.snapshot(), r.leaves())))
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

    log = run_undo_script(e, target, check=check)
    assert seen[0] == len(want) and [t for t, _ in log] == [t for t, _ in ref_log]
    for (tag, got), (_t, pred) in zip(log, ref_log):
        assert np.array_equal(got, pred), (tag, got, pred)
    n_samples = assert_same_results(e, r)
    c = e.session.counters()
    assert c["error"] == 0 and c["games_done"] == e.n_games and c["moves"] == len(r.retained) and c["samples"] == n_samples
    assert _polled_done(e.session) == e.n_games
    return log, len(want), n_samples


@pytest.mark.parametrize("ev_name,target", [("hash", 24), ("k4sat", 8)])
def test_scripted_games_with_undos(ev_name, target):
    e, r = _pair(ev_name, 24)
    log, n_states, n_samples = _scripted(e, r, target)
    e.close()
    assert r.undone >= 300 and r.undone_finished >= 10
    evidence(f"engine undo U1 {ev_name}/{target}: 40 scripted games, {len(log)} calls, {r.undone} undos ({r.undone_finished} of finished games), "
             f"{n_states} snapshots + pending leaves and {n_samples} samples == model bit for bit")


def test_one_game_alone_with_undos():
    positions, ids, kinds = engine_positions()
    i = kinds.index("random")
    e, r = _pair("hash", 24, positions=[positions[i]], ids=[ids[i]])
    _scripted(e, r, 24)
    e.close()
    assert r.undone >= 3


# --------------------------------------------------------------------------------------------- U2
def test_refusals_leave_the_slot_as_it_was():
    from c4a0_amd import _lib

    e, r = _pair("hash", 24)
    e2 = _engine(_evaluator("hash"), 24, c_exploration("hash"), *engine_positions()[:2])
    s = e.session
    for x in (e, e2):
        x.search(8)
        x.session.set_iterations(24)
        x.session.hold_resume()
        x.session.round(x.evaluator)
    r.search(8)
    r.target = 24
    for i in range(40):
        r._resume(i)
    r.round()
    torch.cuda.synchronize()

    def state():
        return (e.snapshot().records.tobytes(), [a.tobytes() for a in s.leaves()], s.planes.cpu().numpy().tobytes(), s.counters()["select_levels"],
                s.sample_counts().tobytes(), e.result().to_records()[0].tobytes())

    before = state()
    snap = e.snapshot()
    assert int((snap.status == ACTIVE).sum()) >= 30
    assert not _both(e, r, "undo_moves").any() and list(e.last_results) == [REFUSED_NO_MOVES] * 40
    assert not _both(e, r, "reset_games").any() and list(e.last_results) == [REFUSED_NO_MOVES] * 40
    req = torch.tensor([5, -1, 3, 1 << 20] * 10, dtype=torch.int32, device=DEV)
    res = torch.full((40,), 99, dtype=torch.int32, device=DEV)
    s.hold_undo(req, res)
    assert res.cpu().tolist() == [REFUSED_REQUEST] * 40 == list(r.undo_requests(req.cpu().numpy()))
    s.hold_undo(torch.zeros(40, dtype=torch.int32, device=DEV), res)
    assert res.cpu().tolist() == [_lib.HOLD_OK] * 40
    s.hold_undo(req)                                                    # (results may be NULL)
    assert state() == before and s.counters()["error"] == 0
    assert_same_state(e, r, "refused")
    # a terminal start position keeps its one-sample result
    n_term = int(snap.terminal.sum())
    assert n_term >= 5 and len(e.result()) == n_term and s.counters()["games_done"] == n_term == s.counters()["samples"]
    assert_same_results(e, r)
    # ... and the search goes on as an untouched engine's
    for x in (e, e2, r):
        x.search(24)
    a, b = e.snapshot(), e2.snapshot()
    assert a.records.tobytes() == b.records.tobytes() and np.array_equal(a.visits, b.visits) and np.array_equal(a.status, b.status)
    assert e.session.counters()["select_levels"] == e2.session.counters()["select_levels"]
    assert_same_state(e, r, "searched on", leaves=False)
    e.close()
    e2.close()


# --------------------------------------------------------------------------------------------- U3
def test_finished_games_undone_and_replayed():
    positions, ids, kinds = engine_positions()
    one = np.array([k == "one" for k in kinds])
    assert int(one.sum()) >= 4
    e, r = _pair("k4sat", 24)
    s = e.session
    for _ in range(4):                                                  # the one-legal-column roots: at most three moves to the end
        e.search(24)
        r.search(24)
        snap = r.snapshot()
        if bool(snap.terminal[one].all()):
            break
        _both(e, r, "make_moves", [legal_columns(m)[0] if o and legal_columns(m) else -1 for m, o in zip(snap.records["mask"], one)])
    snap = assert_same_state(e, r, "played out", leaves=False)
    assert bool(snap.terminal[one].all())
    assert_same_results(e, r)
    n_done = len(e.result())
    counts = s.sample_counts().copy()
    c0, polled0 = s.counters(), _polled_done(s)
    assert c0["games_done"] == n_done == polled0 and c0["samples"] == int(counts.sum()) and bool((counts[one] >= 2).all())

    assert np.array_equal(_both(e, r, "undo_moves", one), one)
    after = assert_same_state(e, r, "undone")
    assert not after.terminal[one].any() and bool((after.status[one] == ACTIVE).all()) and bool((after.visits[one] == 0).all())
    assert np.array_equal(after.n_moves[one], counts[one].astype(np.int64) - 2)
    res = e.result()
    gone = {ids[i] for i in np.flatnonzero(one)}
    assert len(res) == n_done - int(one.sum()) and not gone & {int(g) for g in res.to_records()[0]["game_id"]}
    c1 = s.counters()
    now = s.sample_counts()
    assert bool((now[one] == 0).all()) and np.array_equal(now[~one], counts[~one])
    assert c1["games_done"] == n_done - int(one.sum()) == _polled_done(s) and c1["samples"] == c0["samples"] - int(counts[one].sum())
    assert_same_results(e, r)

    e.search(24)                                                        # replay the move: finished again
    r.search(24)
    snap = assert_same_state(e, r, "searched again", leaves=False)
    assert np.array_equal(_both(e, r, "make_moves", [legal_columns(m)[0] if o else -1 for m, o in zip(snap.records["mask"], one)]), one)
    assert_same_state(e, r, "replayed")
    assert_same_results(e, r)
    c2 = s.counters()
    assert c2["games_done"] == n_done == _polled_done(s) and c2["samples"] == c0["samples"] and c2["error"] == 0
    assert np.array_equal(s.sample_counts(), counts)
    e.close()
    evidence(f"engine undo U3: {int(one.sum())} finished games undone (out of result(), games_done {c0['games_done']} -> {c1['games_done']}, samples "
             f"{c0['samples']} -> {c1['samples']}, counters and polled word) and replayed to the same records")


# --------------------------------------------------------------------------------------------- U4
def test_reset_games_equal_fresh_games():
    positions, ids, _kinds = engine_positions()
    e, r = _pair("hash", 24)
    for t in range(3):
        _turn(e, r, t)
    even = np.arange(40) % 2 == 0
    before = e.snapshot()
    was = _both(e, r, "reset_games", even)
    assert np.array_equal(was, even & (before.n_moves > 0)) and int(was.sum()) >= 15
    fresh = _engine(_evaluator("hash"), 24, c_exploration("hash"), positions, ids)
    got = assert_same_state(e, r, "reset")
    f = fresh.snapshot()
    assert got.records[even].tobytes() == f.records[even].tobytes() and np.array_equal(got.visits[even], f.visits[even])
    assert np.array_equal(got.status[even], f.status[even])
    assert got.records[~even].tobytes() == before.records[~even].tobytes() and np.array_equal(got.visits[~even], before.visits[~even])   # the odd games
    lm, lv, _ = e.session.leaves()
    fm, fv, _ = fresh.session.leaves()
    assert np.array_equal(lm[even], fm[even]) and np.array_equal(lv[even], fv[even])
    for target in (8, 24):
        for x in (e, r, fresh):
            x.search(target)
        got, f = assert_same_state(e, r, f"reset, search({target})", leaves=False), fresh.snapshot()
        assert got.records[even].tobytes() == f.records[even].tobytes() and np.array_equal(got.visits[even], f.visits[even])
    assert bool((got.n_moves[~even & ~got.terminal] >= 1).all())
    assert not _both(e, r, "reset_games", even).any()                   # no moves made: the tree is kept
    assert e.snapshot().records.tobytes() == got.records.tobytes() and np.array_equal(e.snapshot().visits, got.visits)
    assert e.session.counters()["error"] == 0
    e.close()
    fresh.close()


# --------------------------------------------------------------------------------------------- U5
@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_sampled_moves_after_an_undo(ev_name):
    from oracle import c4oracle as O

    e, r = _pair(ev_name, 24)
    special = [i for i, g in enumerate(r.ids) if g in SPECIAL_IDS]
    assert len(special) == 5
    made, reseeded = 0, 0
    for temperature in (1.0, 0.5, 0.0):
        for tag in ("first", "second"):
            e.search(24)
            r.search(24)
            _both(e, r, "make_random_moves", temperature)
            assert_same_state(e, r, f"t={temperature} {tag}")
        undone = _both(e, r, "undo_moves")
        assert_same_state(e, r, f"t={temperature} undone")
        e.search(24)
        r.search(24)
        snap = assert_same_state(e, r, f"t={temperature} searched", leaves=False)
        for i in np.flatnonzero(undone & ~snap.terminal):               # would the unshortened count have sampled another column?
            pol, n = r.games[i].root_policy(), r.true_count(i)
            reseeded += int(O.sample_move(r.ids[i], n, pol, temperature) != O.sample_move(r.ids[i], n + 1, pol, temperature))
        got = _both(e, r, "make_random_moves", temperature)
        assert bool(got[special].any())
        assert_same_state(e, r, f"t={temperature} sampled after the undo")
        made += int(got.sum())
    assert made >= 60 and reseeded >= 3
    assert_same_results(e, r)
    assert e.session.counters()["error"] == 0
    e.close()
    evidence(f"engine undo U5 {ev_name}: {made} sampled moves after an undo at temperatures 1.0 / 0.5 / 0.0 == the model (seed = id * (42 + shortened count); "
             f"{reseeded} of them differ from what the unshortened count samples)")


# --------------------------------------------------------------------------------------------- U6
@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_undo_in_the_middle_of_a_search(ev_name):
    e, r = _pair(ev_name, 100)
    for t in range(2):
        _turn(e, r, t, 8)
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
    assert int((snap.status == ACTIVE).sum()) >= 25 and int(snap.visits.max()) >= 11
    where = np.arange(40) % 3 != 1
    undone = _both(e, r, "undo_moves", where)
    assert int((undone & (snap.status == ACTIVE)).sum()) >= 15          # undone under a pending leaf
    after = assert_same_state(e, r, "undone")
    assert bool((after.visits[undone] == 0).all()) and np.array_equal(after.visits[~undone], snap.visits[~undone])
    for _ in range(2):
        s.round(e.evaluator)
        r.round()
    assert_same_state(e, r, "2 rounds on")
    e.search()
    r.search()
    assert_same_state(e, r, "searched on", leaves=False)
    assert e.session.counters()["error"] == 0
    e.close()


# --------------------------------------------------------------------------------------------- U7
def _network_script(e):
    """a game fragment with undos and a reset at a constant target; returns every snapshot's bytes, the result codes, the records"""
    out = []
    n = e.n_games

    def snap():
        s = e.snapshot()
        out.append(s.records.tobytes() + s.visits.tobytes() + s.status.tobytes())
        return s

    e.search(24)
    graph = e._graph
    s = snap()
    for t in range(4):
        e.make_moves(_walk(s, t))
        out.append(e.last_results.tobytes())
        e.search(24)
        snap()
        e.undo_moves((np.arange(n) + t) % 3 == 0)
        out.append(e.last_results.tobytes())
        snap()
        e.search(24)
        snap()
        e.make_random_moves(1.0, np.arange(n) % 2 == 0)
        out.append(e.last_results.tobytes())
        if t == 2:
            e.reset_games(np.arange(n) % 4 == 1)
            out.append(e.last_results.tobytes())
        e.search(24)
        s = snap()
    recs, counts = e.result().to_records()
    return (out, recs.tobytes(), counts.tobytes()), graph, e._graph


def test_launch_forms_same_bytes_with_undos():
    from c4a0_amd.nn import InferenceNet

    net = InferenceNet(sharp_model(4, 32, SHARP_MODEL_K), torch.device(DEV), dtype=torch.bfloat16)
    assert net.path == "hip" and net.fused_step_ok and net.graph_safe
    positions, ids, _kinds = engine_positions()
    outs = {}
    for form, spg, fuse in (("eager stand-alone", 0, False), ("graph stand-alone", 8, False), ("eager fused", 0, True), ("graph fused", 8, True)):
        e = _engine(net, 24, 6.6, positions, ids, steps_per_graph=spg)
        e.session.fuse_output_step = fuse
        outs[form], g0, g1 = _network_script(e)
        assert (g0 is not None) == (spg > 0) and g1 is g0                 # the graph captured before the first undo is replayed after it
        assert e.session.counters()["error"] == 0
        e.close()
    base = outs["eager stand-alone"]
    codes = np.frombuffer(b"".join(x for x in base[0] if len(x) == 40 * 4), dtype=np.int32)
    assert int((codes == REFUSED_NO_MOVES).sum()) >= 1 and len(base[1]) // 64 >= 5
    for form, got in outs.items():
        assert got == base, form
    evidence(f"engine undo U7: 40 games under a sharp bf16 network, a script with undos and a reset, {len(base[0])} snapshots / result arrays: eager == graph == "
             f"fused == fused in graphs, byte for byte; one graph per engine")


# --------------------------------------------------------------------------------------------- U8
def test_the_arena_is_given_back():
    e, r = _pair("hash", 24, positions=[(0, 0)], ids=[77])
    assert e.session.arena()["blocks_per_slot"] == 43 * 24 + 8 == 1040
    for cycle in range(60):
        for x in (e, r):
            x.search(24)
        _both(e, r, "make_moves", [cycle % 7])
        for x in (e, r):
            x.search(24)
        assert _both(e, r, "undo_moves").all()
        snap = assert_same_state(e, r, f"cycle {cycle}")
        assert int(snap.n_moves[0]) == 0 and int(snap.visits[0]) == 0 and int(snap.status[0]) == ACTIVE
    c = e.session.counters()
    assert c["error"] == 0 and c["expansions"] >= 1560 and c["moves"] == 60 and c["games_done"] == 0
    e.close()
    evidence(f"engine undo U8: 60 cycles of search, move, search, undo in a 1 040-block arena: {c['expansions']} expansions, no overflow")


# --------------------------------------------------------------------------------------------- U9
def test_argument_errors_and_a_hold_session_afterwards():
    from c4a0_amd import _lib
    from c4a0_amd._lib import C4Error
    from c4a0_amd.session import DeviceSession

    dev = torch.device(DEV)
    req = torch.ones(8, dtype=torch.int32, device=dev)
    for kw in ({}, {"search": True}):
        s = DeviceSession(8, 24, 6.6, 0.01, device=dev, **kw)
        with pytest.raises(C4Error) as ex:
            s.hold_undo(req)
        assert ex.value.status == _lib.ERR_BAD_ARG and "C4_FLAG_HOLD" in str(ex.value)
        s.close()
    s = DeviceSession(8, 24, 6.6, 0.01, device=dev, hold=True)
    s.set_games([(i, 0, 0) for i in range(6)])
    s.bind()
    with pytest.raises(C4Error) as ex:
        s.hold_undo(None)
    assert ex.value.status == _lib.ERR_BAD_ARG and "C4_FLAG_HOLD" in str(ex.value)
    s.start()
    s.set_iterations(8)
    s.hold_resume()
    for _ in range(10):
        s.round(hash_eval_torch)
    cols = torch.tensor([3, 3, 3, -1, 3, 3, -1, -1], dtype=torch.int32, device=dev)
    s.hold_resume(cols, None, None)
    for _ in range(10):
        s.round(hash_eval_torch)
    # the arrays in ordinary host memory; slots 6 and 7 hold no game
    host_req = np.array([UNDO_ONE, UNDO_ALL, UNDO_NONE, UNDO_ONE, 9, UNDO_ONE, UNDO_ONE, UNDO_NONE], dtype=np.int32)
    host_res = np.full(8, 99, dtype=np.int32)
    _lib.check(s.L.c4_session_hold_undo(s._h, host_req.ctypes.data, host_res.ctypes.data))
    assert list(host_res) == [0, 0, 0, REFUSED_NO_MOVES, REFUSED_REQUEST, 0, _lib.HOLD_NO_GAME, 0]
    recs, visits, status = s.snapshot()
    assert list(recs["meta"] & 0xFFFF) == [0, 0, 1, 0, 1, 0, 0, 0] and list(visits) == [0, 0, 8, 8, 8, 0, 0, 0]
    assert list(status) == [ACTIVE, ACTIVE, PARKED, PARKED, PARKED, ACTIVE, 0, 0]
    assert list(recs["mask"][:6]) == [0, 0, 1 << 3, 0, 1 << 3, 0]
    for _ in range(10):
        s.round(hash_eval_torch)
    recs, visits, status = s.snapshot()
    assert list(visits) == [8] * 6 + [0, 0] and list(status) == [PARKED] * 6 + [0, 0] and s.counters()["error"] == 0
    s.close()
