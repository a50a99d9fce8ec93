"""GPU: a plain `bench.py` run - headline line only - and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(lib, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert d["prefetch_dropped"] == 0
    for k in ("roofline", "stages_ms", "other_conv_mode", "cpu_baseline", "parity", "decoder_roofline_batch256"):
        assert k not in d, k                      # --full only
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert {"loss.npy", "parameters.npy", "alphas.npy"} <= set(files), sorted(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert abs(float(files["loss.npy"][0]) - d["loss"]) <= 1e-5
