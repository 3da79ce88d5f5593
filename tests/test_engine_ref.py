"""tests/engine_ref.py -- the oracle's MctsGame driven as the reference's InteractivePlay drives it, the reference of every `Engine`
comparison on the GPU (tests/test_gpu_engine.py) -- held to its own floors on the oracle alone:

  1  the reference's KAT for this engine (interactive_play.rs:272-303 `forcing_position`): uniform evaluator, 10 000 iterations,
     its three stages and thresholds, on the player-0 snapshot the reference's test reads;
  2  a search in instalments (to 8, then to 24) ends where a search in one go (24) ends: root policy, q, visits, pending leaf;
  3  the move script of the scripted-games test finishes every game that started non-terminal and covers what it is there for:
     at least 30 finished games, at least 3 refusals of each of the four kinds, at least 3 moves made while a leaf was pending,
     and subtrees kept by the moves."""
import numpy as np
import pytest

from tests.engine_ref import (ACTIVE, PARKED, REFUSED_COLUMN, REFUSED_SAMPLE, REFUSED_TERMINAL, REFUSED_UNSEARCHED, RefEngine, assert_forcing_thresholds,
                              c_exploration, engine_positions, forcing_position, forcing_stages, oracle_evaluator, run_script, uniform_evaluator)
from tests.helpers import evidence


def test_forcing_position_kat():
    e = RefEngine(uniform_evaluator, 10_000, 4.0, 0.01, positions=[forcing_position()])
    stages = forcing_stages(e)
    assert_forcing_thresholds(stages)
    assert len(e.retained) == 2 and all(0 < kept < had for kept, had in e.retained)
    s0, s1, s2 = (s.records[0] for s in stages)
    evidence(f"engine KAT (oracle): {s0['policy'][1] + s0['policy'][4]:.4f} / {s0['q_penalty']:.4f} / {s0['q_no_penalty']:.4f}; after 1: "
             f"{s1['q_penalty']:.4f} / {s1['q_no_penalty']:.4f}; after 0: policy[4] {s2['policy'][4]:.4f}, {s2['q_penalty']:.4f} / {s2['q_no_penalty']:.4f}; "
             f"visits retained {[k for k, _ in e.retained]}")


@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_instalments_equal_one_go(ev_name):
    positions, ids, _kinds = engine_positions()
    a = RefEngine(oracle_evaluator(ev_name), 24, c_exploration(ev_name), positions=positions, game_ids=ids)
    b = RefEngine(oracle_evaluator(ev_name), 24, c_exploration(ev_name), positions=positions, game_ids=ids)
    a.search(8)
    mid = a.snapshot()
    assert int(mid.visits.max()) == 8 and bool(((mid.visits == 8) | mid.terminal).all())
    a.search(24)
    b.search(24)
    sa, sb = a.snapshot(), b.snapshot()
    assert sa.records.tobytes() == sb.records.tobytes() and np.array_equal(sa.visits, sb.visits)
    assert a.leaves() == b.leaves()
    assert bool((sa.status == PARKED).all()) and bool(((sa.visits == 24) | (sa.terminal & (sa.visits == 0))).all())


@pytest.mark.parametrize("ev_name", ["hash", "k4sat"])
def test_move_script_covers_its_ground(ev_name):
    positions, ids, kinds = engine_positions()
    assert kinds.count("empty") == 1 and kinds.count("won") + kinds.count("lost") >= 2 and kinds.count("drawn") >= 2 and kinds.count("one") >= 4
    assert sum(k in ("won", "lost", "drawn") for k in kinds) >= 4
    assert any(bin(m).count("1") % 2 == 1 for (m, _v), k in zip(positions, kinds) if k == "random")
    e = RefEngine(oracle_evaluator(ev_name), 24, c_exploration(ev_name), positions=positions, game_ids=ids)
    start = e.snapshot()
    assert bool((start.status[start.terminal] == PARKED).all()) and bool((start.status[~start.terminal] == ACTIVE).all())
    log = run_script(e, 24)
    end = e.snapshot()
    assert bool(end.terminal.all())                                   # every game that started non-terminal was finished by the script
    finished = int((~start.terminal).sum())
    assert finished >= 30 and len(e.result()) == len(positions)
    codes = np.concatenate([r for _tag, r in log])
    n_ref = {k: int((codes == k).sum()) for k in (REFUSED_TERMINAL, REFUSED_COLUMN, REFUSED_UNSEARCHED, REFUSED_SAMPLE)}
    assert min(n_ref.values()) >= 3, n_ref
    assert e.moves_under_pending_leaf >= 3
    kept = [k for k, _had in e.retained]
    assert sum(k > 0 for k in kept) >= 30                              # subtrees were kept, not rebuilt
    evidence(f"engine script ({ev_name}, oracle): {finished} games finished in {len(log)} move calls, {len(e.retained)} moves, refusals {n_ref}, "
             f"{e.moves_under_pending_leaf} moves under a pending leaf, {sum(k > 0 for k in kept)} moves kept visits (up to {max(kept)})")
