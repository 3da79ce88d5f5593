"""Tournaments from a HIP graph: `play_games(evaluator={model_id: InferenceNet})` on the grouped path (device-side router, grouped
bf16 chain, answers handed over inside the step launch) gives the records of the eager per-model path byte for byte, agrees with
the oracle replaying the games from the logged answers (T3), falls back to the eager path with the reason in `stats`, and plays
the same games whether its rounds run eagerly or from a graph."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BIG = (1 << 63) + 7
IDS = (3, 5, BIG)
N_ITER, N_SLOTS = 12, 8
_NETS = {}


def _nets(channels=32):
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    if channels not in _NETS:
        nets = {}
        for i, mid in enumerate(IDS):
            torch.manual_seed(7000 + channels + i)
            nets[mid] = InferenceNet(ConnectFourNet(ModelConfig(1, channels, 2, 2)), torch.device("cuda:0"), dtype=torch.bfloat16, strict=True)
        _NETS[channels] = nets
    return _NETS[channels]


def _reqs():
    """the round robin twice over plus three games of a model against itself: 15 games on 8 slots, so slots are refilled and the
    tail has idle slots"""
    pairs = list(itertools.permutations(IDS, 2)) * 2 + [(m, m) for m in IDS]
    return [(500 + 7 * i, p0, p1) for i, (p0, p1) in enumerate(pairs)]


def _wrapped(nets):
    """the same networks as plain callables: what `play_games` cannot stack, so the eager per-model path plays them"""
    return {mid: (lambda planes, net=net: net(planes)) for mid, net in nets.items()}


def _play(evaluator, stats):
    import c4a0_amd

    reqs = [c4a0_amd.GameMetadata(*r) for r in _reqs()]
    return c4a0_amd.play_games(reqs, 64, N_ITER, 1.4, 0.01, evaluator=evaluator, resident_games=N_SLOTS, stats=stats)


def test_grouped_tournament_records_equal_the_eager_path_byte_for_byte():
    nets = _nets()
    st_g, st_e = {}, {}
    got = _play(nets, st_g)
    want = _play(_wrapped(nets), st_e)
    assert st_g["multi_model"] == "grouped" and "multi_model_reason" not in st_g and st_g["phases"]["graph_captures"] >= 1
    assert st_e["multi_model"] == "eager" and "InferenceNet" in st_e["multi_model_reason"] and st_e["phases"]["graph_captures"] == 0
    assert got == want and got.to_cbor() == want.to_cbor()
    assert [(r.metadata.game_id, r.metadata.player0_id, r.metadata.player1_id) for r in got.results] == _reqs()
    assert st_g["games_done"] == st_e["games_done"] == len(_reqs()) and st_g["samples"] == st_e["samples"] and st_g["sims"] == st_e["sims"]
    # the three networks do play differently: a game's records depend on who plays it
    firsts = {r.samples[1].policy.tobytes() for r in got.results if len(r.samples) > 1}
    assert len(firsts) > 1


def test_grouped_tournament_t3_parity_with_the_oracle():
    """Every routed row's position and answer is logged per model; the oracle replays the games with one table evaluator per model."""
    from c4a0_amd.api import _GroupedModelEvaluator
    from c4a0_amd.nn import GroupedNets
    from c4a0_amd.session import DeviceSession
    from oracle import c4oracle as O
    from tests.helpers import oracle_samples_by_game, planes_to_pos_np, samples_by_game

    nets = _nets()
    s = DeviceSession(N_SLOTS, N_ITER, 1.4, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16)
    try:
        s.set_games(_reqs())
        ev = _GroupedModelEvaluator(s, GroupedNets(nets))
        table = {}

        def log(_step):
            # planes hold the leaves, leaf_models who must answer, logprobs / q the grouped chain's answers (scattered back to the slots)
            _m, _v, status = s.leaves()
            models = ev.models.cpu().numpy().view(np.uint64)
            mask, value = planes_to_pos_np(s.planes.float().cpu().numpy())
            lp, q = s.logprobs.cpu().numpy(), s.q.cpu().numpy()
            assert int(ev.n_unrouted.item()) == 0
            for g in np.nonzero(status == 1)[0]:
                key = (int(models[g]), int(mask[g]), int(value[g]))
                val = (lp[g].tobytes(), q[g].tobytes())
                assert table.setdefault(key, val) == val, "a model's answer must be a function of the position"

        s.run(ev, on_step=log)
        got = samples_by_game(s.drain_samples())
    finally:
        s.close()
    assert {k[0] for k in table} == set(IDS)
    zeros = (np.zeros(7, np.float32).tobytes(), np.zeros(2, np.float32).tobytes())

    def lookup(model_id, x):
        mask, value = planes_to_pos_np(x)
        ans = []
        for m, v in zip(mask, value):
            key = (int(model_id) & ((1 << 64) - 1), int(m), int(v))
            if key not in table:   # the device never shows a terminal leaf to the evaluator; the reference asks and ignores the answer
                assert O.terminal_state(O.Pos(int(m), int(v))) != 0, "a non-terminal leaf the device never evaluated"
                ans.append(zeros)
            else:
                ans.append(table[key])
        lp = np.stack([np.frombuffer(a[0], dtype=np.float32) for a in ans])
        q = np.stack([np.frombuffer(a[1], dtype=np.float32) for a in ans])
        return np.ascontiguousarray(lp), np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])

    want, _ = O.self_play(_reqs(), 64, N_ITER, 1.4, 0.01, lookup)
    assert got == oracle_samples_by_game(want)
    # ... and each logged answer is what the model's own InferenceNet computes for that position, bit for bit
    for mid, net in nets.items():
        keys = [k for k in table if k[0] == mid]
        from tests.helpers import pos_to_planes_np
        planes = pos_to_planes_np(np.array([k[1] for k in keys], dtype=np.uint64), np.array([k[2] for k in keys], dtype=np.uint64))
        lp, q = net(torch.from_numpy(planes).to("cuda:0", torch.bfloat16))
        lp, q = lp.cpu().numpy(), q.cpu().numpy()
        assert all(table[k] == (lp[i].tobytes(), q[i].tobytes()) for i, k in enumerate(keys))


def test_networks_of_different_widths_fall_back_to_the_eager_path():
    mixed = dict(_nets())
    mixed[5] = _nets(64)[5]
    st, st_w = {}, {}
    got = _play(mixed, st)
    assert st["multi_model"] == "eager" and "channels" in st["multi_model_reason"] and st["phases"]["graph_captures"] == 0
    want = _play(_wrapped(mixed), st_w)
    assert got == want and st["games_done"] == len(_reqs())


def test_eager_and_graphed_rounds_play_the_same_games():
    from c4a0_amd.api import _GroupedModelEvaluator
    from c4a0_amd.nn import GroupedNets
    from c4a0_amd.session import DeviceSession

    grouped = GroupedNets(_nets())
    out = []
    for spg, gather in ((0, True), (8, True), (0, False), (8, False)):
        s = DeviceSession(N_SLOTS, N_ITER, 1.4, 0.01, device=torch.device("cuda:0"), planes_dtype=torch.bfloat16)
        try:
            s.set_games(_reqs())
            ev = _GroupedModelEvaluator(s, grouped)
            ev.gather_step = gather
            s.run(ev, steps_per_graph=spg)
            out.append(s.drain_samples().tobytes())
            assert s.counters()["games_done"] == len(_reqs())
        finally:
            s.close()
    assert out[0] == out[1] == out[2] == out[3]
