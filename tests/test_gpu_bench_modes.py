"""bench.py's two kinds of run: a plain run reports the headline and what its timed steps measured, nothing that takes runs of its own;
--full adds the copy yardsticks, the CPU baseline and the collective self-check (the rows, the host path and the live PMC passes are
left out here with their --no-* options: they take minutes at their fixed sizes)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2n", "22", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_and_full_runs():
    plain = _line([])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2
    assert "cpu_baseline" not in plain and "host_path" not in plain
    assert set(plain["kernels"]) == {"other"}                                   # the step's second kernel, from the step's own events
    assert plain["config"]["collective_check"].startswith("not run")

    full = _line(["--full", "--no-rows", "--no-host", "--no-live-pmc", "--cpu-log2n", "18"])
    assert full["metric"] == plain["metric"] and full["unit"] == plain["unit"] and full["dtype"] == plain["dtype"]
    assert full["config"]["collective_check"].startswith("ok")
    assert full["kernels"]["copy_best_GBps"] > 0 and full["kernels"]["read_nt_GBps"] > 0
    assert full["cpu_baseline"]["value"] > 0 and "host_path" not in full
