"""bench.py's plain run (no --full): it sets up, warms up, times the steps, writes --dump-outputs and prints the
headline line, and runs nothing else -- no instrumented launches, CPU baseline or other shapes (those are --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_plain_run_prints_the_headline_alone(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "C4_BENCH_FORCE_DIST", "C4_BENCH_SAME_DEVICE", "C4_BENCH_BACKEND"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--rounds-per-step", "128",
           "--preroll", "1600", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "games/s" and out["higher_is_better"] is True and out["dtype"] == "bf16" and out["metric"].startswith("self-play games/sec")
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 1 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["games_completed"] > 0 and out["nn"]["achieved"] > 0
    for k in ("roofline", "cpu_baseline", "other_configs", "sample_allgather"):
        assert k not in out, k
    d = out["dump_outputs"]
    assert d["samples_written"] > 0 and d["games"] > 0
    assert np.load(dump / "samples_policy.npy").shape == (d["samples_written"], 7)
