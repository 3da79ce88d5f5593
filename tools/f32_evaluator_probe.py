#!/usr/bin/env python3
"""The f32 evaluator (InferenceNet(dtype=torch.float32, hip_tower=True)) measured: per-kernel time at 256 / 1 024 / 2 048 / 4 096 rows
for the reference's default net (1 x 32, 4 / 2 head layers) and the bench net (4 x 32, 4 / 2), their TFLOP/s against the f32 MFMA
peak (157.3 TF), forward() against the same model on PyTorch's f32 path (hip_tower=False), and play_games games/s for 4 096 games at
n = 100 with the bench net on both paths.  Prints ONE JSON line.

    python tools/f32_evaluator_probe.py [reps]"""
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from c4a0_amd.nn import ConnectFourNet, EvaluatorFallbackWarning, InferenceNet, ModelConfig, flops_per_leaf  # noqa: E402

PEAK_TF = 157.3
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = torch.device("cuda:0")


def timed(fn, reps=REPS):
    """Median microseconds of `fn` over `reps` runs, each bracketed by events on the current stream (after 3 warm-up runs)."""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def entry(us, flops):
    tf = flops / us / 1e6
    return {"us": round(us, 1), "tflops": round(tf, 2), "of_peak": round(tf / PEAK_TF, 3)}


def kernels(cfg, rows):
    torch.manual_seed(1337)
    model = ConnectFourNet(ModelConfig(*cfg)).eval()
    net = InferenceNet(model, DEV, dtype=torch.float32, hip_tower=True, strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", EvaluatorFallbackWarning)
        ref = InferenceNet(model, DEV, dtype=torch.float32, hip_tower=False)
    cp, hp = net.cp, net.hp
    x = (torch.rand(rows, 2, 6, 7, device=DEV) > 0.6).float()
    feat = net.tower(x)
    h = net._linear_relu(feat, net.merged_w1, net.merged_b1)
    p, v = h[:, :hp], h[:, hp:]
    out = {}
    tower_flops = rows * 42 * 2 * (cp * 32 + cfg[0] * 2 * cp * 9 * cp)     # as computed (padded k of conv0, padded channels)
    out["tower"] = entry(timed(lambda: net.tower(x)), tower_flops)
    out["linear_2F"] = entry(timed(lambda: net._linear_relu(feat, net.merged_w1, net.merged_b1)), 2 * rows * 2 * hp * 42 * cp)
    if len(net.pol_w) > 2:
        w, b = net.pol_w[1], net.pol_b[1]
        out["linear_F"] = entry(timed(lambda: net._linear_relu(p, w, b)), 2 * rows * hp * hp)
    out["head_out"] = entry(timed(lambda: net._head_out_f32(p, v)), 2 * rows * 16 * 2 * hp)
    lp = torch.empty((rows, 7), device=DEV)
    q = torch.empty((rows, 2), device=DEV)
    flops = rows * flops_per_leaf(ModelConfig(*cfg))
    out["forward_hip"] = entry(timed(lambda: net(x, out_logprobs=lp, out_q=q)), flops)
    out["forward_torch_f32"] = entry(timed(lambda: ref(x, out_logprobs=lp, out_q=q)), flops)
    return out


def gemm_4096_1344():
    torch.manual_seed(1)
    net = InferenceNet(ConnectFourNet(ModelConfig(1, 32, 4, 2)).eval(), DEV, dtype=torch.float32, hip_tower=True, strict=True)
    x = torch.rand(4096, 1344, device=DEV)
    w, b = net.pol_w[1], net.pol_b[1]
    return entry(timed(lambda: net._linear_relu(x, w, b)), 2 * 4096 * 1344 * 1344)


def play(hip: bool):
    import c4a0_amd

    torch.manual_seed(1337)
    model = ConnectFourNet(ModelConfig(4, 32, 4, 2)).eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", EvaluatorFallbackWarning)
        net = InferenceNet(model, DEV, dtype=torch.float32, hip_tower=hip)
    reqs = [c4a0_amd.GameMetadata(i, 0, 0) for i in range(4096)]
    c4a0_amd.play_games(reqs[:64], 4096, 8, 6.6, 0.01, evaluator=net)   # warm-up: module loads, graph pools
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c4a0_amd.play_games(reqs, 4096, 100, 6.6, 0.01, evaluator=net)
    return round(4096 / (time.perf_counter() - t0), 1)


def main():
    res = {"peak_tflops_f32_mfma": PEAK_TF, "device": torch.cuda.get_device_name(DEV), "reps": REPS}
    for name, cfg in (("default_1x32", (1, 32, 4, 2)), ("bench_4x32", (4, 32, 4, 2))):
        res[name] = {str(rows): kernels(cfg, rows) for rows in (256, 1024, 2048, 4096)}
    res["gemm_4096x1344x1344"] = gemm_4096_1344()
    res["play_games_4096_n100_games_per_s"] = {"hip_f32": play(True), "torch_f32": play(False)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
