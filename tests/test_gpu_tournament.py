"""Tournaments with built-in players on the device: a round robin of anchors alone and one of networks and anchors run on the
grouped path (HIP graph, routed leaves), give the oracle's games with the numpy twin of the anchors (tests/builtin_players_ref.py)
as its callback and the eager per-model path's records byte for byte; one `BuiltinEvaluator` is a valid single evaluator of
`play_games` and `search_positions`; `play_tournament` with `gen_players` ranks a training folder."""
from datetime import datetime

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import builtin_players_ref as R

BIG = (1 << 63) + 7
ANCHORS = {3: ("random", 0), 5: ("uniform", 0), BIG: ("random", 9)}
N_ITER = 12
_NETS, _PLAYERS = {}, []


def _anchor_players(spec=ANCHORS):
    from c4a0_amd.tournament import RandomPlayer, UniformPlayer

    return [RandomPlayer(mid, seed=seed) if kind == "random" else UniformPlayer(mid) for mid, (kind, seed) in spec.items()]


def _models():
    """two networks, seeded as tests/test_gpu_grouped_tournament.py seeds its own"""
    from c4a0_amd.nn import ConnectFourNet, ModelConfig

    if not _NETS:
        for i, mid in enumerate((21, 22)):
            torch.manual_seed(7000 + 32 + i)
            _NETS[mid] = ConnectFourNet(ModelConfig(1, 32, 2, 2))
    return _NETS


def _triples(games):
    return [(r.metadata.game_id, r.metadata.player0_id, r.metadata.player1_id) for r in games.results]


def test_all_built_in_tournament_is_grouped_and_plays_the_oracles_games():
    from c4a0_amd.tournament import play_tournament
    from tests.helpers import oracle_samples_by_game, samples_by_game

    st = {}
    t = play_tournament(_anchor_players(), 2, 64, N_ITER, 1.4, resident_games=4, stats=st, device="cuda:0")
    assert st["multi_model"] == "grouped" and "multi_model_reason" not in st and st["phases"]["graph_captures"] >= 1
    reqs, played = R.oracle_games(ANCHORS, 2, N_ITER)
    assert t.model_ids == list(ANCHORS) and _triples(t.games) == reqs and st["games_done"] == len(reqs) == 6
    assert samples_by_game(t.games.to_records()[0]) == oracle_samples_by_game(played)
    assert sum(s for _, s in t.get_scores()) == 6 and t.score_matrix().sum() == 6


def test_all_built_in_rounds_play_the_same_games_eagerly_and_from_a_graph():
    from c4a0_amd.api import _GroupedModelEvaluator
    from c4a0_amd.builtin import GroupedPlayers
    from c4a0_amd.session import DeviceSession
    from tests.helpers import oracle_samples_by_game, samples_by_game

    reqs, played = R.oracle_games(ANCHORS, 2, N_ITER)
    grouped = GroupedPlayers({p.model_id: p.device_evaluator("cuda:0") for p in _anchor_players()})
    out = []
    for spg, gather in ((0, True), (8, True), (0, False), (8, False)):
        s = DeviceSession(4, N_ITER, 1.4, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16)
        try:
            s.set_games(reqs)
            ev = _GroupedModelEvaluator(s, grouped)
            ev.gather_step = gather
            s.run(ev, steps_per_graph=spg)
            recs = s.drain_samples()
            out.append(recs.tobytes())
            assert s.counters()["games_done"] == len(reqs) and int(ev.n_unrouted.item()) == 0
        finally:
            s.close()
    assert out[0] == out[1] == out[2] == out[3]
    assert samples_by_game(recs) == oracle_samples_by_game(played)


def _mixed_players():
    from c4a0_amd.tournament import ModelPlayer, RandomPlayer, UniformPlayer

    if not _PLAYERS:
        _PLAYERS.extend([ModelPlayer(mid, m, torch.device("cuda:0"), dtype=torch.bfloat16, strict=True) for mid, m in _models().items()])
        _PLAYERS.extend([RandomPlayer(BIG, seed=9), UniformPlayer(5)])
    return _PLAYERS


def test_mixed_tournament_records_equal_the_eager_path_byte_for_byte():
    import c4a0_amd
    from c4a0_amd.nn import GroupedNets
    from c4a0_amd.tournament import play_tournament, tournament_requests

    players = _mixed_players()
    assert [p.name for p in players] == ["gen21", "gen22", "random", "uniform"]
    st_g, st_e = {}, {}
    t = play_tournament(players, 2, 64, N_ITER, 1.4, resident_games=8, stats=st_g)
    got = t.games
    assert st_g["multi_model"] == "grouped" and "multi_model_reason" not in st_g and st_g["phases"]["graph_captures"] >= 1
    evs = {p.model_id: p.device_evaluator("cuda:0") for p in players}
    assert GroupedNets.refusal(evs) is None
    wrapped = {mid: (lambda planes, ev=ev: ev(planes)) for mid, ev in evs.items()}     # what play_games cannot group: the eager path plays them
    reqs = tournament_requests([p.model_id for p in players], 2)
    want = c4a0_amd.play_games(reqs, 64, N_ITER, 1.4, 0.01, evaluator=wrapped, resident_games=8, stats=st_e)
    assert st_e["multi_model"] == "eager" and "InferenceNet" in st_e["multi_model_reason"] and st_e["phases"]["graph_captures"] == 0
    assert got == want and got.to_cbor() == want.to_cbor() and len(got) == 12
    assert _triples(got) == R.round_robin([21, 22, BIG, 5], 2)
    assert st_g["games_done"] == st_e["games_done"] == 12 and st_g["samples"] == st_e["samples"] and st_g["sims"] == st_e["sims"]
    # a dict of the two networks alone still plays what it played: the grouped and the eager path agree there too
    nets = {mid: ev for mid, ev in evs.items() if mid in (21, 22)}
    reqs2 = tournament_requests([21, 22], 4)
    st_n = {}
    a = c4a0_amd.play_games(reqs2, 64, N_ITER, 1.4, 0.01, evaluator=nets, resident_games=4, stats=st_n)
    b = c4a0_amd.play_games(reqs2, 64, N_ITER, 1.4, 0.01, evaluator={mid: wrapped[mid] for mid in nets}, resident_games=4)
    assert st_n["multi_model"] == "grouped" and a == b and a.to_cbor() == b.to_cbor()


def test_mixed_tournament_t3_parity_with_the_oracle():
    """Every routed row's position and answer is logged per player; the oracle replays the games with the networks' logged answers
    and the numpy twin for the anchors (tests/test_gpu_grouped_tournament.py's T3, with anchors)."""
    from c4a0_amd.api import _GroupedModelEvaluator
    from c4a0_amd.builtin import GroupedPlayers
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.helpers import oracle_samples_by_game, planes_to_pos_np, pos_to_planes_np, samples_by_game

    players = _mixed_players()
    evs = {p.model_id: p.device_evaluator("cuda:0") for p in players}
    anchors = {BIG: ("random", 9), 5: ("uniform", 0)}
    reqs = R.round_robin([p.model_id for p in players], 2)
    s = DeviceSession(8, N_ITER, 1.4, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16)
    try:
        s.set_games(reqs)
        ev = _GroupedModelEvaluator(s, GroupedPlayers(evs))
        table = {}

        def log(_step):
            _m, _v, status = s.leaves()
            models = ev.models.cpu().numpy().view(np.uint64)
            mask, value = planes_to_pos_np(s.planes.float().cpu().numpy())
            lp, q = s.logprobs.cpu().numpy(), s.q.cpu().numpy()
            assert int(ev.n_unrouted.item()) == 0
            for g in np.nonzero(status == 1)[0]:
                key = (int(models[g]), int(mask[g]), int(value[g]))
                val = (lp[g].tobytes(), q[g].tobytes())
                assert table.setdefault(key, val) == val, "a player's answer must be a function of the position"

        s.run(ev, on_step=log)
        got = samples_by_game(s.drain_samples())
    finally:
        s.close()
    assert {k[0] for k in table} == set(evs)
    # the anchors' logged answers are the twin's, bit for bit
    for mid, (kind, seed) in anchors.items():
        keys = [k for k in table if k[0] == mid]
        lg, qp, qn = R.answers(kind, seed, mid, np.array([k[1] for k in keys], np.uint64), np.array([k[2] for k in keys], np.uint64))
        assert all(table[k] == (lg[i].tobytes(), np.array([qp[i], qn[i]], np.float32).tobytes()) for i, k in enumerate(keys)) and keys
    zeros = (np.zeros(7, np.float32).tobytes(), np.zeros(2, np.float32).tobytes())
    twin = R.twin_callback(anchors)

    def lookup(model_id, x):
        mid = int(model_id) & ((1 << 64) - 1)
        if mid in anchors:
            return twin(mid, x)
        mask, value = planes_to_pos_np(x)
        ans = []
        for m, v in zip(mask, value):
            key = (mid, int(m), int(v))
            if key not in table:   # the device never shows a terminal leaf to the evaluator; the reference asks and ignores the answer
                assert O.terminal_state(O.Pos(int(m), int(v))) != 0, "a non-terminal leaf the device never evaluated"
                ans.append(zeros)
            else:
                ans.append(table[key])
        lp = np.stack([np.frombuffer(a[0], dtype=np.float32) for a in ans])
        q = np.stack([np.frombuffer(a[1], dtype=np.float32) for a in ans])
        return np.ascontiguousarray(lp), np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])

    want, _ = O.self_play(reqs, 64, N_ITER, 1.4, 0.01, lookup)
    assert got == oracle_samples_by_game(want)
    # ... and each network's logged answer is what its own InferenceNet computes for that position, bit for bit
    for mid in (21, 22):
        keys = [k for k in table if k[0] == mid]
        planes = pos_to_planes_np(np.array([k[1] for k in keys], dtype=np.uint64), np.array([k[2] for k in keys], dtype=np.uint64))
        lp, q = evs[mid](torch.from_numpy(planes).to("cuda:0", torch.bfloat16))
        lp, q = lp.cpu().numpy(), q.cpu().numpy()
        assert all(table[k] == (lp[i].tobytes(), q[i].tobytes()) for i, k in enumerate(keys))


def test_one_built_in_evaluator_plays_and_searches_like_the_oracle():
    import c4a0_amd
    from c4a0_amd.builtin import BuiltinEvaluator
    from tests.helpers import oracle_samples_by_game, random_positions, samples_by_game
    from tests.search_ref import assert_records_equal, search
    from oracle import c4oracle as O

    ev = BuiltinEvaluator("random", 7, seed=4, device="cuda:0")
    triples = [(900 + 3 * i, 7, 7) for i in range(12)]
    reqs = [c4a0_amd.GameMetadata(*r) for r in triples]
    st = {}
    got = c4a0_amd.play_games(reqs, 64, 10, 1.4, 0.01, evaluator=ev, resident_games=8, stats=st)
    want, _ = O.self_play(triples, 64, 10, 1.4, 0.01, R.twin_callback({7: ("random", 4)}))
    assert samples_by_game(got.to_records()[0]) == oracle_samples_by_game(want)
    assert st["phases"]["graph_captures"] >= 1 and st["concurrent_sessions"] == 1
    st2 = {}
    two = c4a0_amd.play_games(reqs, 64, 10, 1.4, 0.01, evaluator=ev, resident_games=8, concurrent_sessions=2, stats=st2)
    assert st2["concurrent_sessions"] == 2 and two == got and two.to_cbor() == got.to_cbor()
    bf16 = c4a0_amd.play_games(reqs, 64, 10, 1.4, 0.01, evaluator=ev, resident_games=8, planes_dtype=torch.bfloat16)
    assert bf16.to_cbor() == got.to_cbor()
    # searches of given positions: the oracle's run_mcts with the twin
    pos = random_positions(16, seed=99)
    twin = lambda leaves: R.answers("random", 4, 7, np.array([p.mask for p in leaves], np.uint64), np.array([p.value for p in leaves], np.uint64))
    r = c4a0_amd.search_positions(pos, 10, 1.4, 0.01, evaluator=ev)
    assert_records_equal(r.records, search(pos, 10, twin, 1.4), pos)
    uni = c4a0_amd.search_positions(pos, 10, 1.4, 0.01, evaluator=BuiltinEvaluator("uniform", 0, device="cuda:0"))
    assert_records_equal(uni.records, search(pos, 10, lambda leaves: R.answers("uniform", 0, 0, [p.mask for p in leaves], [p.value for p in leaves]), 1.4), pos)


def test_one_built_in_evaluator_drives_the_engine_like_the_oracle():
    """`main.py play --model random|uniform` is the reference's use of the anchors as ONE evaluator of interactive play."""
    import c4a0_amd
    from c4a0_amd.builtin import BuiltinEvaluator
    from tests.engine_undo_ref import RefEngineUndo

    pos = [(0, 0), (0b1, 0b1), (0b10000001, 0b1), (0b1111, 0b1111)]
    twin = lambda leaves: R.answers("random", 4, 7, [p.mask for p in leaves], [p.value for p in leaves])
    eng = c4a0_amd.Engine(BuiltinEvaluator("random", 7, seed=4, device="cuda:0"), 16, 1.4, 0.01, positions=pos)
    ref = RefEngineUndo(twin, 16, 1.4, positions=pos)
    try:
        for e in (eng, ref):
            e.search(8)
            e.make_moves([3, 7, 2, 0])
            e.search(16)
        assert eng.snapshot().records.tobytes() == ref.snapshot().records.tobytes() and list(eng.last_results) == list(ref.last_results)
    finally:
        eng.close()


def test_play_tournament_ranks_a_training_folder(tmp_path):
    from c4a0_amd.nn import ConnectFourNet, ModelConfig
    from c4a0_amd.tournament import RandomPlayer, UniformPlayer, gen_players, play_tournament
    from c4a0_amd.training import TrainingGen

    base = str(tmp_path)
    for gen_n in (1, 0):   # (written newest first: gen_players orders by gen_n)
        torch.manual_seed(300 + gen_n)
        TrainingGen(created_at=datetime(2024, 5, 1 + gen_n), gen_n=gen_n, n_mcts_iterations=N_ITER, c_exploration=1.4, c_ply_penalty=0.01,
                    self_play_batch_size=64, training_batch_size=64).save_all(base, None, ConnectFourNet(ModelConfig(1, 32, 2, 2)))
    gens = gen_players(base, "cuda:0", strict=True)
    assert [(p.name, p.model_id) for p in gens] == [("gen0", 0), ("gen1", 1)]
    assert [p.name for p in gen_players(base, "cuda:0", gens=[1])] == ["gen1"]
    with pytest.raises(FileNotFoundError):
        gen_players(base, "cuda:0", gens=[4])
    players = gens + [RandomPlayer(100), UniformPlayer(101)]
    st = {}
    t = play_tournament(players, 2, 64, N_ITER, 1.4, resident_games=8, stats=st)
    assert st["multi_model"] == "grouped" and st["games_done"] == 12
    assert t.model_ids == [0, 1, 100, 101] and _triples(t.games) == R.round_robin([0, 1, 100, 101], 2)
    # the scores are the per-game definition's, in its order
    scores = {}
    for r in t.games.results:
        p0 = r.player0_score()
        scores[r.metadata.player0_id] = scores.get(r.metadata.player0_id, 0.0) + p0
        scores[r.metadata.player1_id] = scores.get(r.metadata.player1_id, 0.0) + 1 - p0
    want = sorted(scores.items(), key=lambda x: x[1], reverse=True)
    assert t.get_scores() == want and t.get_top_models() == [m for m, _ in want] and sum(scores.values()) == 12
    assert np.array_equal(t.score_matrix().sum(axis=1), [scores[m] for m in t.model_ids])
    names = {p.model_id: p.name for p in players}
    text = [format(s, "g") for _, s in want]
    after = [len(x) - x.index(".") if "." in x else 0 for x in text]
    text = [x + " " * (max(after) - a) for x, a in zip(text, after)]
    lines = ["| Player   |   Score |", "|----------|---------|"] + [f"| {names[m]:<8} | {x:>7} |" for (m, _), x in zip(want, text)]
    assert t.scores_table(names.get) == "\n".join(lines)
    # the same tournament through the numpy callback (a player that offers forward_numpy only sends the whole job there): same games

    class Numpy(UniformPlayer):
        def device_evaluator(self, device):
            return None

    st_cb = {}
    t_cb = play_tournament(gens + [RandomPlayer(100), Numpy(101)], 2, 64, N_ITER, 1.4, resident_games=8, stats=st_cb)
    assert "multi_model" not in st_cb and st_cb["nn_positions"] > 0 and t_cb.games == t.games
