"""CPU-side checks of tournaments with built-in players: the host twin of the two anchors (c4_builtin_eval_host) against their
definition restated in numpy (tests/builtin_players_ref.py), the round robin's schedule, `TournamentResult`'s scores from the packed
records against the per-GameResult definition on games the oracle played, and what `GroupedNets.refusal` lets through.  No GPU."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import builtin_players_ref as R
from tests.helpers import pos_to_planes_np, random_positions

BIG = (1 << 63) + 7
PLAYERS = {3: ("random", 0), 5: ("uniform", 0), BIG: ("random", 9)}   # the all-built-in tournament of the GPU tests
_CACHE = {}


def _planes():
    if "planes" not in _CACHE:
        pos = np.array(random_positions(2000), dtype=np.uint64)
        _CACHE["planes"] = pos_to_planes_np(pos[:, 0], pos[:, 1])
    return _CACHE["planes"]


@pytest.mark.parametrize("kind", R.KINDS)
def test_host_twin_equals_the_definition_bit_for_bit(kind):
    from c4a0_amd.builtin import builtin_eval_numpy

    planes = _planes()
    seen = set()
    for mid, seed in itertools.product(R.IDS, R.SEEDS):
        got, want = builtin_eval_numpy(planes, kind, seed, mid), R.forward_numpy(kind, seed, mid, planes)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.shape == w.shape and g.flags["C_CONTIGUOUS"]
            assert g.tobytes() == w.tobytes()
        lg, qp, qn = got
        assert np.array_equal(qp, qn)
        if kind == "uniform":
            assert np.all(lg == 1.0) and np.all(qp == 0.0)
        else:
            assert lg.min() >= 0.0 and lg.max() < 1.0 and qp.min() >= -1.0 and qp.max() < 1.0
            assert len(np.unique(lg)) > 3500 and qp.min() < -0.9 and qp.max() > 0.9       # draws, not a constant
        seen.add(lg.tobytes() + qp.tobytes())
    assert len(seen) == (1 if kind == "uniform" else len(R.IDS) * len(R.SEEDS))            # every id and every seed is another player


def test_the_position_is_read_as_nonzero_cells_and_the_answer_is_a_function_of_the_row():
    from c4a0_amd.builtin import builtin_eval_numpy

    planes = _planes()[:64].copy()
    want = builtin_eval_numpy(planes, "random", 7, 11)
    scaled = planes * np.float32(-2.5)                 # != 0 is what counts, not 1.0
    scaled[planes == 0] = -0.0                         # and a negative zero is a zero
    got = builtin_eval_numpy(scaled, "random", 7, 11)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    perm = np.random.default_rng(0).permutation(64)
    got = builtin_eval_numpy(planes[perm][:17], "random", 7, 11)                            # another batch, another order
    assert all(g.tobytes() == w[perm][:17].tobytes() for g, w in zip(got, want))
    empty = builtin_eval_numpy(np.zeros((0, 2, 6, 7), np.float32), "random", 0, 0)
    assert [a.shape for a in empty] == [(0, 7), (0,), (0,)]
    with pytest.raises(ValueError):
        builtin_eval_numpy(planes, "best", 0, 0)


def test_players_answer_through_the_host_twin():
    from c4a0_amd.tournament import Player, RandomPlayer, UniformPlayer

    planes = _planes()[:100]
    r, u = RandomPlayer(BIG, seed=9), UniformPlayer(5)
    assert (r.name, r.model_id, u.name, u.model_id) == ("random", BIG, "uniform", 5)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(r.forward_numpy(planes), R.forward_numpy("random", 9, BIG, planes)))
    assert all(g.tobytes() == w.tobytes() for g, w in zip(u.numpy_callback()(5, planes), R.forward_numpy("uniform", 0, 5, planes)))
    assert Player("me", 1).device_evaluator("cuda:0") is None
    with pytest.raises(NotImplementedError):
        Player("me", 1).forward_numpy(planes)


@pytest.mark.parametrize("ids", [(3, 5, BIG), (10, 0, 7, 2)])
def test_the_schedule_is_the_references(ids):
    from c4a0_amd.tournament import tournament_requests

    for games_per_match in (2, 6):
        pairings = list(itertools.permutations(ids, 2)) * int(games_per_match / 2)          # tournament.py:128
        reqs = tournament_requests(ids, games_per_match)
        assert [(r.game_id, r.player0_id, r.player1_id) for r in reqs] == [(i, p0, p1) for i, (p0, p1) in enumerate(pairings)]
        assert len(reqs) == len(ids) * (len(ids) - 1) * games_per_match // 2


def test_odd_games_per_match_and_duplicate_ids_are_refused():
    from c4a0_amd.tournament import RandomPlayer, UniformPlayer, play_tournament

    with pytest.raises(ValueError, match="even"):
        play_tournament([RandomPlayer(1), UniformPlayer(2)], 3, 64, 12, 1.4)
    with pytest.raises(ValueError, match="duplicate"):
        play_tournament([RandomPlayer(1), UniformPlayer(2), RandomPlayer(1, seed=4)], 2, 64, 12, 1.4)


def oracle_tournament():
    """(reqs, PlayGamesResult) of the round robin of PLAYERS (games_per_match = 2, n = 12) as the oracle plays it with the twin"""
    if "tournament" not in _CACHE:
        import c4a0_amd

        reqs, played = R.oracle_games(PLAYERS, 2, 12)
        results = [c4a0_amd.GameResult(c4a0_amd.GameMetadata(*r), [c4a0_amd.Sample(s.mask, s.value, s.policy, s.q_penalty, s.q_no_penalty) for s in played[r[0]]])
                   for r in reqs]
        _CACHE["tournament"] = (reqs, c4a0_amd.PlayGamesResult(results))
    return _CACHE["tournament"]


def _reference_scores(games):
    """tournament.py:88-98, as written there"""
    scores = {}
    for result in games.results:
        p0 = result.player0_score()
        scores[result.metadata.player0_id] = scores.get(result.metadata.player0_id, 0.0) + p0
        scores[result.metadata.player1_id] = scores.get(result.metadata.player1_id, 0.0) + 1 - p0
    ret = list(scores.items())
    ret.sort(key=lambda x: x[1], reverse=True)
    return ret


def test_scores_from_the_packed_records_equal_the_per_game_definition():
    import c4a0_amd
    from c4a0_amd.tournament import TournamentResult, player0_scores

    reqs, games = oracle_tournament()
    assert len(games) == 6
    t = TournamentResult(model_ids=list(PLAYERS), games=c4a0_amd.PlayGamesResult.from_cbor(games.to_cbor()))       # (held as packed records)
    assert t.games._lazy is not None
    ids, s0 = player0_scores(t.games)
    assert t.games._lazy is not None, "the scores are computed without building Sample objects"
    assert s0.tolist() == [r.player0_score() for r in games.results] and ids.tolist() == [list(r) for r in reqs]
    want = _reference_scores(games)
    assert t.get_scores() == want and t.get_top_models() == [m for m, _ in want]
    assert sum(s for _, s in t.get_scores()) == len(reqs)
    m = t.score_matrix()
    assert m.shape == (3, 3) and m.dtype == np.float64 and np.all(np.diag(m) == 0)
    assert m.sum() == len(reqs) and np.all(m + m.T + 2 * np.eye(3) == 2)                      # every pair played games_per_match = 2 games
    assert {mid: s for mid, s in want} == {mid: m[i].sum() for i, mid in enumerate(PLAYERS)}
    by_pair = {}
    for r in games.results:
        a, b, p0 = r.metadata.player0_id, r.metadata.player1_id, r.player0_score()
        by_pair[(a, b)] = by_pair.get((a, b), 0.0) + p0
        by_pair[(b, a)] = by_pair.get((b, a), 0.0) + 1 - p0
    idx = {mid: i for i, mid in enumerate(PLAYERS)}
    assert all(m[idx[a], idx[b]] == v for (a, b), v in by_pair.items())
    # the same result held as objects
    assert TournamentResult(model_ids=list(PLAYERS), games=games).get_scores() == want


def test_equal_scores_keep_first_seen_order():
    """the same game under both colour assignments: each player takes one point whoever won, and the order is who appears first"""
    import c4a0_amd
    from c4a0_amd.tournament import TournamentResult

    _reqs, games = oracle_tournament()
    samples = next(r.samples for r in games.results if r.player0_score() != 0.5)
    for first, second in ((3, 9), (9, 3)):
        tied = c4a0_amd.PlayGamesResult([c4a0_amd.GameResult(c4a0_amd.GameMetadata(0, first, second), samples),
                                         c4a0_amd.GameResult(c4a0_amd.GameMetadata(1, second, first), samples),
                                         c4a0_amd.GameResult(c4a0_amd.GameMetadata(2, 4, first), samples),
                                         c4a0_amd.GameResult(c4a0_amd.GameMetadata(3, first, 4), samples)])
        t = TournamentResult(model_ids=[3, 4, 9], games=tied)
        assert t.get_scores() == _reference_scores(tied) == [(first, 2.0), (second, 1.0), (4, 1.0)]
        assert t.scores_table(lambda i: f"gen{i}") == "\n".join([
            "| Player   |   Score |",
            "|----------|---------|",
            f"| gen{first}     |       2 |",
            f"| gen{second}     |       1 |",
            "| gen4     |       1 |"])
    half = TournamentResult(model_ids=[1, 2], games=c4a0_amd.PlayGamesResult([c4a0_amd.GameResult(c4a0_amd.GameMetadata(0, 1, 2), samples)]))
    lines = half.scores_table({1: "a-rather-long-name", 2: "b"}.get).split("\n")
    assert len({len(x) for x in lines}) == 1 and lines[0].startswith("| Player ") and lines[1].startswith("|---")
    with pytest.raises(RuntimeError, match="unfinished"):
        TournamentResult(model_ids=[1, 2], games=c4a0_amd.PlayGamesResult([c4a0_amd.GameResult(c4a0_amd.GameMetadata(0, 1, 2), samples[:1])])).get_scores()


def test_scores_table_aligns_halves_at_the_decimal_point():
    import c4a0_amd
    from c4a0_amd.tournament import TournamentResult

    # a drawn game: the full board of tests.helpers.DRAWN_LINE, 42 stones and no four
    from oracle import c4oracle as O
    from tests.helpers import DRAWN_LINE
    full = O.from_moves(DRAWN_LINE)
    assert O.terminal_state(full) == 3
    drawn = [c4a0_amd.Sample(int(full.mask), int(full.value), [0] * 7, 0.0, 0.0)]
    _reqs, games = oracle_tournament()
    won = next(r.samples for r in games.results if r.player0_score() == 1.0)
    res = c4a0_amd.PlayGamesResult([c4a0_amd.GameResult(c4a0_amd.GameMetadata(0, 1, 2), won), c4a0_amd.GameResult(c4a0_amd.GameMetadata(1, 1, 2), drawn)])
    t = TournamentResult(model_ids=[1, 2], games=res)
    assert t.get_scores() == [(1, 1.5), (2, 0.5)]
    assert t.scores_table({1: "gen1", 2: "uniform"}.get) == "\n".join([
        "| Player   |   Score |",
        "|----------|---------|",
        "| gen1     |     1.5 |",
        "| uniform  |     0.5 |"])


def test_refusal_lets_built_in_players_through_and_still_names_its_reasons():
    from c4a0_amd import _lib
    from c4a0_amd.builtin import BuiltinEvaluator
    from c4a0_amd.nn import ConnectFourNet, GroupedNets, InferenceNet, ModelConfig

    cpu = torch.device("cpu")
    rnd, uni = BuiltinEvaluator("random", 3, seed=9, device=cpu), BuiltinEvaluator("uniform", 5, device=cpu)
    assert (rnd.graph_safe, rnd.batch_invariant, rnd.dtype) == (True, True, None)
    assert GroupedNets.refusal({3: rnd, 5: uni}) is None and GroupedNets.refusal({5: uni}) is None
    assert "different devices" in GroupedNets.refusal({3: rnd, 5: BuiltinEvaluator("uniform", 5, device="cuda:0")})
    assert "more than" in GroupedNets.refusal({i: uni for i in range(_lib.ROUTE_MAX_MODELS + 1)})
    assert GroupedNets.refusal({}) == "no evaluators"

    def net(channels=32, seed=0):
        torch.manual_seed(seed)
        return InferenceNet(ConnectFourNet(ModelConfig(1, channels, 2, 2)), cpu, dtype=torch.bfloat16)

    a, b = net(seed=1), net(seed=2)
    # with networks: a built-in player is never the reason, the networks' reasons stand as they were
    assert GroupedNets.refusal({1: a, 2: b, 3: rnd, 5: uni}) == GroupedNets.refusal({1: a, 2: b}) and "hand-written" in GroupedNets.refusal({1: a, 2: b})
    assert "channels" in GroupedNets.refusal({3: rnd, 1: a, 2: net(64)})
    assert "not a c4a0_amd.nn.InferenceNet" in GroupedNets.refusal({1: a, 3: rnd, 4: lambda planes: rnd(planes)})
    assert "different devices" in GroupedNets.refusal({1: a, 3: BuiltinEvaluator("random", 3, device="cuda:0")})
    assert "more than" in GroupedNets.refusal({**{i: a for i in range(_lib.ROUTE_MAX_MODELS)}, 99: uni})
    with pytest.raises(ValueError):
        GroupedNets({3: rnd, 5: uni})           # GroupedNets stacks networks; the built-in players' home is builtin.GroupedPlayers
