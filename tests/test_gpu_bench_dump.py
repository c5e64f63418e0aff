"""bench.py --dump-outputs: every config writes the arrays of its last timed step (float32, seeded samples of the large outputs), the inputs are
the same on every run, and --steps is the number of timed steps the JSON line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("config,log2n,shapes", [
    ("filtwelch", 24, {"filt": (1 << 22,), "welch_power": (2049,), "welch_mean": (2049,)}),   # 2^24 outputs -> a 2^22 sample
    ("stft", 18, {"stft": (4096, 1024, 2)}),                                                  # 8 x 1021 frames -> 4096 of them
    ("resample", 22, {"resample": (4, 1 << 21), "resample_avg": (1024,)}),                    # 4 x ~4.57 M outputs -> 2^21 per channel
])
def test_bench_dumps_the_last_step(tmp_path, config, log2n, shapes):
    runs = []
    for steps in (2, 3):
        d = tmp_path / str(steps)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--config", config,
                            "--log2n", str(log2n), "--no-rows", "--no-host", "--no-cpu-baseline", "--no-live-pmc", "--dump-outputs", str(d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == steps
        runs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    for got in runs:
        assert {k: v.shape for k, v in got.items()} == shapes
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    for name in shapes:
        assert relerr(runs[1][name], runs[0][name]) < 1e-6, name        # same inputs, whatever the number of steps
    if config == "filtwelch":
        assert relerr(runs[0]["welch_mean"], runs[0]["welch_power"]) < 1e-6  # one rank: the mean over ranks is this rank's PSD
