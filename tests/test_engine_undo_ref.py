"""tests/engine_undo_ref.py -- RefEngine with MctsGame::undo_move / reset_game on top, the reference of every `Engine.undo_moves` /
`Engine.reset_games` comparison on the GPU (tests/test_gpu_engine_undo.py) -- held to the oracle wherever the oracle can speak:

  1  without any undo the model IS RefEngine: engine_ref.run_script gives the same log, every snapshot and pending leaf, and
     result() byte for byte -- which pins the restated to_result on every game the script finishes;
  2  after an undo and search(t) a game's snapshot is that of a fresh RefEngine at the same position searched to t, in every field
     but the move count in meta;
  3  reset_games == undoing until refused;
  4  the refusal codes;
  5  the C ABI: the header declares c4_session_hold_undo and the constants, _lib mirrors them, the library exports the symbol, the
     ABI number stays 14.  (Fails without the feature.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.engine_ref import ACTIVE, PARKED, RefEngine, c_exploration, engine_positions, legal_columns, oracle_evaluator, run_script
from tests.engine_undo_ref import (REFUSED_NO_MOVES, REFUSED_REQUEST, UNDO_ALL, UNDO_NONE, UNDO_ONE, RefEngineUndo, run_undo_script)
from tests.helpers import evidence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(ev_name, max_n=24, cls=RefEngineUndo, positions=None, ids=None):
    if positions is None:
        positions, ids, _kinds = engine_positions()
    return cls(oracle_evaluator(ev_name), max_n, c_exploration(ev_name), positions=positions, game_ids=ids)


def _state(r):
    s = r.snapshot()
    return s.records.tobytes(), s.visits.tobytes(), s.status.tobytes(), s.terminal.tobytes(), r.leaves()


def _turn(r, t, target=24):
    r.search(target)
    snap = r.snapshot()
    cols = [legal_columns(m)[(i + t) % len(legal_columns(m))] if legal_columns(m) else 0 for i, m in enumerate(snap.records["mask"])]
    return r.make_moves(cols)


# --------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_without_an_undo_the_model_is_ref_engine(ev_name):
    a, b = _model(ev_name), _model(ev_name, cls=RefEngine)
    seen_a, seen_b = [], []
    log_a = run_script(a, 24, check=lambda tag: seen_a.append((tag,) + _state(a)))
    log_b = run_script(b, 24, check=lambda tag: seen_b.append((tag,) + _state(b)))
    assert seen_a == seen_b and len(seen_a) >= 20
    assert [t for t, _ in log_a] == [t for t, _ in log_b] and all(np.array_equal(x, y) for (_t, x), (_u, y) in zip(log_a, log_b))
    got, want = a.result(), b.result()
    assert got == want and len(want) == 40                             # the restated to_result == the oracle's, -0.0 included
    n_samples = sum(len(v) for v in want.values())
    assert any(np.frombuffer(s[3], np.float32)[0] < 0 for v in want.values() for s in v) and n_samples >= 300
    assert [a.true_count(i) for i in range(40)] == [len(h) for h in a.history] == [g.n_moves() for g in b.games]
    evidence(f"engine undo model ({ev_name}): run_script without undos == RefEngine, {len(seen_a)} states and {n_samples} samples of 40 games byte for byte")


# --------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_an_undone_game_is_a_fresh_game_at_that_position(ev_name):
    positions, ids, _kinds = engine_positions()
    r = _model(ev_name)
    for t in range(3):
        _turn(r, t)
    before = r.snapshot()
    hist = [list(h) for h in r.history]
    undone = r.undo_moves()
    assert np.array_equal(undone, np.array([len(h) > 0 for h in hist])) and int(undone.sum()) >= 30
    mid = r.snapshot()
    idx = np.flatnonzero(undone)
    for i in idx:
        assert (int(mid.records["mask"][i]), int(mid.records["value"][i])) == hist[i][-1][0] == r.leaves()[i]
        assert int(mid.n_moves[i]) == len(hist[i]) - 1 == int(before.n_moves[i]) - 1
    assert bool((mid.visits[idx] == 0).all()) and bool((mid.status[idx] == ACTIVE).all())
    keep = np.flatnonzero(~undone)                                      # terminal starts: not touched
    assert mid.records[keep].tobytes() == before.records[keep].tobytes() and bool((mid.status[keep] == PARKED).all())
    r.search(16)
    got = r.snapshot()
    fresh = _model(ev_name, cls=RefEngine, positions=[hist[i][-1][0] for i in idx], ids=[ids[i] for i in idx])
    fresh.search(16)
    want = fresh.snapshot()
    for name in ("game_id", "mask", "value", "policy", "q_penalty", "q_no_penalty"):
        assert np.ascontiguousarray(got.records[name][idx]).tobytes() == np.ascontiguousarray(want.records[name]).tobytes(), name
    assert np.array_equal(got.visits[idx], want.visits) and np.array_equal(got.status[idx], want.status) and bool((want.visits == 16).all())
    assert np.array_equal(got.n_moves[idx], [len(hist[i]) - 1 for i in idx]) and bool((want.n_moves == 0).all())


# --------------------------------------------------------------------------------------------- 3
def test_reset_is_undo_until_refused():
    a, b = _model("hash"), _model("hash")
    for t in range(3):
        _turn(a, t)
        _turn(b, t)
    start = _model("hash", cls=RefEngine)
    where = np.arange(40) % 2 == 0
    was = a.reset_games(where)
    steps = 0
    while b.undo_moves(where).any():
        steps += 1
    assert steps == 3 and bool((b.last_results[where] == REFUSED_NO_MOVES).all())
    assert np.array_equal(was, where & ~start.snapshot().terminal)
    assert _state(a) == _state(b)
    for x, y in zip(a.history, b.history):
        assert len(x) == len(y) and all(p == q and np.array_equal(u, v) for (p, u), (q, v) in zip(x, y))
    sa = a.snapshot()
    s0 = start.snapshot()
    assert sa.records[where].tobytes() == s0.records[where].tobytes() and bool((sa.n_moves[~where & ~sa.terminal] == 3).all())
    a.search(24)
    b.search(24)
    start.search(24)
    assert _state(a) == _state(b)
    assert a.snapshot().records[where].tobytes() == start.snapshot().records[where].tobytes()
    # a reset of a game without moves does nothing: the tree is kept
    visits = a.snapshot().visits.copy()
    assert not a.reset_games(where).any() and np.array_equal(a.snapshot().visits, visits) and bool((visits[where & ~sa.terminal] == 24).all())


# --------------------------------------------------------------------------------------------- 4
def test_refusal_codes():
    r = _model("hash")
    before = _state(r)
    assert not r.undo_moves().any() and list(r.last_results) == [REFUSED_NO_MOVES] * 40
    assert not r.reset_games().any() and list(r.last_results) == [REFUSED_NO_MOVES] * 40
    assert list(r.undo_requests([5] * 40)) == [REFUSED_REQUEST] * 40 and list(r.undo_requests([-1, 3] * 20)) == [REFUSED_REQUEST] * 40
    assert list(r.undo_requests([UNDO_NONE] * 40)) == [0] * 40
    assert _state(r) == before
    made = _turn(r, 0)
    res = r.undo_requests([UNDO_ONE if i % 2 else UNDO_ALL for i in range(40)])
    assert np.array_equal(res == 0, made) and set(res[~made].tolist()) == {REFUSED_NO_MOVES}
    assert list(r.undo_requests([UNDO_ONE] * 40)) == [REFUSED_NO_MOVES] * 40
    # a game finished at its start keeps its one sample
    term = np.flatnonzero(r.snapshot().terminal)
    assert len(term) >= 5 and sorted(r.result()) == term.tolist() and all(len(v) == 1 for v in r.result().values())


def test_undo_script_covers_its_ground():
    r = _model("hash")
    log = run_undo_script(r, 24)
    assert bool(r.snapshot().terminal.all()) and len(r.result()) == 40
    undo = np.concatenate([c for t, c in log if t.endswith("undo")])
    assert r.undone >= 300 and r.undone_finished >= 10 and int((undo == REFUSED_NO_MOVES).sum()) >= 20
    evidence(f"engine undo script (oracle): {len(log)} calls, {r.undone} undos ({r.undone_finished} of finished games), {int((undo == REFUSED_NO_MOVES).sum())} refused")


# --------------------------------------------------------------------------------------------- 5
def test_entry_point_is_declared_bound_and_exported_and_the_abi_number_stays():
    from c4a0_amd import _lib
    from c4a0_amd.csrc import build

    header = open(os.path.join(ROOT, "include", "c4a0_hip.h")).read()
    assert re.search(r"\bint\s+c4_session_hold_undo\s*\(\s*c4_session\s*\*\s*s\s*,\s*const\s+int32_t\s*\*\s*requests\s*,\s*int32_t\s*\*\s*results\s*\)\s*;", header)
    for name, value in (("C4_HOLD_UNDO_NONE", 0), ("C4_HOLD_UNDO_ONE", 1), ("C4_HOLD_UNDO_ALL", 2), ("C4_HOLD_REFUSED_NO_MOVES", 6), ("C4_HOLD_REFUSED_REQUEST", 7)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
        assert getattr(_lib, name[3:]) == value
    assert (UNDO_NONE, UNDO_ONE, UNDO_ALL, REFUSED_NO_MOVES, REFUSED_REQUEST) == (0, 1, 2, 6, 7)
    assert len(_lib.SIGNATURES["c4_session_hold_undo"][1]) == 3
    assert re.search(r"#define\s+C4_ABI_VERSION\s+14\b", header) and _lib.ABI_VERSION == 14
    lib = C.CDLL(build.build())
    assert hasattr(lib, "c4_session_hold_undo") and lib.c4_abi_version() == 14
    from c4a0_amd import Engine
    from c4a0_amd.session import DeviceSession

    assert callable(Engine.undo_moves) and callable(Engine.reset_games) and callable(DeviceSession.hold_undo)
