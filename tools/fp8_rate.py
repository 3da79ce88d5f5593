"""The opt-in fp8 hidden layers against the bf16 ones, on the GPU -> profiles/fp8_heads.json.

    python tools/fp8_rate.py [out.json]          (a) + (b) below
    python tools/fp8_rate.py --pmc-target        ten launches of the 2 048 x 2 688 x 1 344 fp8 layer (config 3): the program of a `rocprofv3 --pmc`
                                                 run of its own (no tracing combined)
    python tools/fp8_rate.py --pmc-summarize DIR [out.json]    means per launch of the counters such a run left under DIR

(a) c4_linear_fp8 against c4_linear_bf16 for m in {512, 2048, 4096} and (n, k) in {(2688, 1344), (1344, 1344), (5376, 2688),
    (2688, 2688)}, and c4_quantize_bf16_fp8 alone: device-event timing of HIP graphs of 20 launches, warmed up, the two sides
    ALTERNATING, medians of 7 pairs.  The headline: at 2 048 rows, the three fp8 launches + the quantise launch against the three
    bf16 launches of the 4 x 32 network's heads (2F-wide, F-wide, F-wide).
(b) a whole play_games call at BASELINE config 2's shape (4 096 games on 4 096 slots, n = 100, 4 x 32 network), the fp8 net against
    the bf16 net, BOTH with host_loop="python" (the same loop drives both); the bf16 side is the baseline.
Speed is recorded here, never asserted in a test."""
import ctypes as C
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c4a0_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
p = lambda t: C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def graph_of(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g, per_graph=20, replays=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (replays * per_graph) * 1e3


def ab(ga, gb, pairs=7):
    """medians (us per launch) of `pairs` alternating timings of two graphs, and their spreads"""
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(time_us(ga))
        tb.append(time_us(gb))
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def operands(m, n, k):
    g = torch.Generator().manual_seed(m + n + k)
    x = torch.relu(torch.randn(m, k, generator=g)).bfloat16().to(dev)
    w = (torch.randn(n, k, generator=g) / k ** 0.5)
    b = torch.zeros(n, dtype=torch.float32, device=dev)
    from c4a0_amd.nn import quantize_head_weights
    wq, e_w = quantize_head_weights(w)
    dq = torch.ldexp(torch.ones(n, dtype=torch.float64), -4 - e_w.to(torch.int64)).float().to(dev)
    x8 = torch.empty((m, k), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    _lib.check(L.c4_quantize_bf16_fp8(p(x), p(x8), m, k, k, k, 16.0, stream()))
    return {"x": x, "w": w.bfloat16().to(dev), "b": b, "x8": x8, "wq": wq.to(dev), "dq": dq,
            "y": torch.empty((m, n), dtype=torch.bfloat16, device=dev), "y8": torch.empty((m, n), dtype=torch.uint8, device=dev)}


def fp8_launch(o, m, n, k, out_fp8=1, config=0):
    L = _lib.lib()
    return lambda: _lib.check(L.c4_linear_fp8(p(o["x8"]), p(o["wq"]), p(o["dq"]), p(o["b"]), p(o["y8"] if out_fp8 else o["y"]), m, n, k, k, n, 1, out_fp8, 16.0, config,
                                              stream()))


def bf16_launch(o, m, n, k):
    L = _lib.lib()
    return lambda: _lib.check(L.c4_linear_bf16(p(o["x"]), p(o["w"]), p(o["b"]), p(o["y"]), m, n, k, k, n, 1, 0, stream()))


def part_a():
    L = _lib.lib()
    rows = []
    for m in (512, 2048, 4096):
        for n, k in ((2688, 1344), (1344, 1344), (5376, 2688), (2688, 2688)):
            o = operands(m, n, k)
            f, b, fs, bs = ab(graph_of(fp8_launch(o, m, n, k)), graph_of(bf16_launch(o, m, n, k)))
            rows.append({"m": m, "n": n, "k": k, "fp8_us": round(f, 2), "bf16_us": round(b, 2), "fp8_min_max_us": [round(v, 2) for v in fs],
                         "bf16_min_max_us": [round(v, 2) for v in bs], "fp8_over_bf16": round(f / b, 3),
                         "fp8_TMACs_per_s": round(m * n * k / f / 1e6, 1), "bf16_TMACs_per_s": round(m * n * k / b / 1e6, 1)})
            if m == 2048:     # every explicit configuration once (same bits; c4_fp8_gemm.hip)
                rows[-1]["fp8_us_by_config"] = {str(c): round(statistics.median(time_us(gc) for _ in range(5)), 2)
                                                for c in (1, 2, 3, 4) for gc in [graph_of(fp8_launch(o, m, n, k, config=c))]}
            print(rows[-1], flush=True)
        for k in (1344, 2688):
            o = operands(m, 192, k)
            q = graph_of(lambda: _lib.check(L.c4_quantize_bf16_fp8(p(o["x"]), p(o["x8"]), m, k, k, k, 16.0, stream())))
            t = statistics.median(time_us(q) for _ in range(7))
            rows.append({"m": m, "k": k, "quantize_us": round(t, 2), "GBps_read_plus_written": round(m * k * 3 / t / 1e3, 1)})
            print(rows[-1], flush=True)
    at = lambda n, k, key: next(r[key] for r in rows if r.get("m") == 2048 and r.get("n") == n and r["k"] == k)
    fp8_sum = at(2688, 1344, "fp8_us") + 2 * at(1344, 1344, "fp8_us") + next(r["quantize_us"] for r in rows if r["m"] == 2048 and r["k"] == 1344 and "quantize_us" in r)
    bf16_sum = at(2688, 1344, "bf16_us") + 2 * at(1344, 1344, "bf16_us")
    return {"layers": rows, "headline_2048_rows": {"fp8_three_gemms_plus_quantize_us": round(fp8_sum, 2), "bf16_three_gemms_us": round(bf16_sum, 2),
                                                   "target_met": bool(fp8_sum < bf16_sum)}}


def part_b():
    import c4a0_amd
    from c4a0_amd.nn import ConnectFourNet, InferenceNet, ModelConfig

    torch.manual_seed(1337)
    model = ConnectFourNet(ModelConfig(4, 32, 4, 2)).eval()
    nets = {"bf16": InferenceNet(model, dev), "fp8": InferenceNet(model, dev, head_dtype=torch.float8_e4m3fn)}
    reqs = [c4a0_amd.GameMetadata(10_000 + i, 0, 0) for i in range(4096)]
    times = {"bf16": [], "fp8": []}
    info = {}
    for rep in range(4):          # the first pair is the warm-up
        for name in ("bf16", "fp8"):
            stats = {}
            t0 = time.perf_counter()
            c4a0_amd.play_games(reqs, 1, 100, 4.0, 0.01, None, evaluator=nets[name], resident_games=4096, host_loop="python", stats=stats)
            dt = time.perf_counter() - t0
            assert stats["host_loop"] == "python" and stats["error"] == 0
            if rep:
                times[name].append(dt)
            info[name] = {"steps": stats["steps"], "sims": stats["sims"], "concurrent_sessions": stats["concurrent_sessions"]}
    out = {"shape": "4 096 games on 4 096 slots, n = 100, 4 x 32 network, host_loop='python' for both", "scales": nets["fp8"].fp8_scales}
    for name in times:
        out[name] = {"wall_s_median_of_3": round(statistics.median(times[name]), 4), "wall_s_all": [round(t, 4) for t in times[name]],
                     "games_per_s": round(4096 / statistics.median(times[name]), 1), **info[name]}
    out["fp8_over_bf16_wall"] = round(out["fp8"]["wall_s_median_of_3"] / out["bf16"]["wall_s_median_of_3"], 3)
    return out


def pmc_target():
    m, n, k = 2048, 2688, 1344
    o = operands(m, n, k)
    fn = fp8_launch(o, m, n, k, config=3)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()


def pmc_summarize(d):
    sums, launches = {}, {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "c4_fp8_gemm" not in r.get("Kernel_Name", ""):
                continue
            c = r["Counter_Name"]
            sums[c] = sums.get(c, 0.0) + float(r["Counter_Value"])
            launches[c] = launches.get(c, 0) + 1
    return {"kernel": "c4_linear_fp8 config 3 (c4_fp8_gemm_lds_kernel<128>: 224 workgroups), m 2048 n 2688 k 1344", "source": "rocprofv3 --pmc passes of their own over tools/fp8_rate.py --pmc-target",
            "mean_per_launch": {c: sums[c] / launches[c] for c in sorted(sums)}}


if __name__ == "__main__":
    if "--pmc-target" in sys.argv:
        pmc_target()
    elif "--pmc-summarize" in sys.argv:
        i = sys.argv.index("--pmc-summarize")
        res = pmc_summarize(sys.argv[i + 1])
        print(json.dumps(res, indent=1))
        if len(sys.argv) > i + 2:
            json.dump(res, open(sys.argv[i + 2], "w"), indent=1)
    else:
        res = {"device": torch.cuda.get_device_name(0), "method": "HIP graphs of 20 launches, device events, alternating pairs, medians of 7", "a": part_a(), "b": part_b()}
        print(json.dumps(res["a"]["headline_2048_rows"]), json.dumps(res["b"]))
        json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "profiles/fp8_heads.json", "w"), indent=1)
