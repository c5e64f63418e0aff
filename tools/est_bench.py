"""Time the quinn pass, quinn and jacobsen (mdsp_quinn_*, mdsp_est_*, src/estimation.jl:93-220) on the device.

    python tools/est_bench.py [--reps R] [--warmup W] [--cases pass32,pass64,calls32,calls64] [--out profiles/est_bench.json] [--small]

Cases:  pass32 / pass64    one quinn pass (alpha = 2 cos(2 pi 0.283)) over one Float32 / Float64 column of 2^28 samples, device-resident
        calls32 / calls64  one jacobsen(x) call and one whole quinn(x, f0, 1.0) call (f0 = that jacobsen estimate; the tone is at 0.283) on 2^24 samples
Per pass case, after warm-up, the MEDIAN of R >= 10 device-event-timed calls (no profiler):
    ms           the time of one mdsp_quinn_pass_exec (S > 1: its four launches)
    GBps         sizeof(T) bytes per sample over that time (a cut signal is read twice: 2 x as much moves)
    reduce_frac  the time of a SUMABS2 reduction (mdsp_reduce_exec) of the SAME array over ms
    copy_frac    the time of mdsp_copy_bench of the same array into a second buffer over ms
    S, seglen    from mdsp_quinn_plan_info
and the record of the timed size equals mdsp_quinn_pass_emulate_host of the same array bit for bit.
Per calls case the MEDIAN wall-clock time of R calls on a device tensor (each call ends in a copy to the host, so it is timed on the host), the
iterations quinn took, and both estimates.  --small divides every length by 64 (a dry run of the tool itself).  Each case runs in a child process under
a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"pass32": ("float32", 1 << 28), "pass64": ("float64", 1 << 28), "calls32": ("float32", 1 << 24), "calls64": ("float64", 1 << 24)}
TONE = 0.283


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, reps, warmup, small):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev
    from dsp_jl_amd.util import ReducePlan

    dtype, n = CASES[name]
    if small:
        n //= 64
    dt = np.dtype(dtype)
    _lib.check(_lib.lib().mdsp_init(0))
    g = torch.Generator(device="cuda")
    g.manual_seed(1776)
    tdt = getattr(torch, dtype)
    x = torch.cos(2 * np.pi * TONE * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4).to(tdt)
    x += 0.1 * torch.randn(n, generator=g, device="cuda", dtype=tdt)
    lib, stream = _lib.lib(), _dev.stream_ptr()
    row = {"case": name, "dtype": dtype, "n": n, "reps": reps}
    if name.startswith("calls"):
        def wall(fn):
            for _ in range(warmup):
                fn()
            t = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
            return median(t)
        row["jacobsen_ms"] = round(wall(lambda: d.jacobsen(x)), 4)
        row["jacobsen"] = d.jacobsen(x)
        f0 = row["jacobsen"]
        row["quinn_ms"] = round(wall(lambda: d.quinn(x, f0, 1.0)), 4)
        plan = d.QuinnPlan(dt, n)
        est, reached, iters = plan.estimate(x.data_ptr(), f0, 1.0)
        row.update(quinn=est, reached_maxiters=reached, iterations=iters, S=plan.segments, seglen=plan.seglen)
        return [row]

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def bench(fn):
        for _ in range(warmup):
            fn()
        t = []
        for _ in range(reps):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]))
        return median(t)

    nbytes = x.numel() * x.element_size()
    y = torch.empty_like(x)
    copy_ms = bench(lambda: _lib.check(lib.mdsp_copy_bench(y.data_ptr(), x.data_ptr(), nbytes, stream)))
    del y
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    red = ReducePlan(1, n, 1, _lib.REDUCE_SUMABS2, dt)
    reduce_ms = bench(lambda: red.exec(x.data_ptr(), out.data_ptr(), stream))
    alpha, mean = 2 * np.cos(2 * np.pi * TONE), 0.001
    plan = d.QuinnPlan(dt, n)
    ms = bench(lambda: plan.pass_exec(x.data_ptr(), mean, alpha, out.data_ptr(), stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    xh = np.ascontiguousarray(x.cpu().numpy())
    want = np.zeros(4)
    mu = (C.c_double * 2)(mean, 0.0)
    _lib.check(lib.mdsp_quinn_pass_emulate_host(xh.ctypes.data, _dev.md_dtype(dt), n, 0, mu, float(alpha), want.ctypes.data_as(_lib.pdbl)))
    row.update(S=plan.segments, seglen=plan.seglen, workspace_bytes=plan.workspace_bytes, copy_ms=round(copy_ms, 4), reduce_ms=round(reduce_ms, 4), ms=round(ms, 4),
               GBps=round(nbytes / ms / 1e6, 1), reduce_frac=round(reduce_ms / ms, 3), copy_frac=round(copy_ms / ms, 3),
               record_equal_to_emulation=bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))))
    assert row["record_equal_to_emulation"], f"{name}: the device record {got} differs from the host emulation {want}"
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "est_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", default="")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    if args.case:
        for row in run_case(args.case, args.reps, args.warmup, args.small):
            print(json.dumps(row), flush=True)
        return
    rows = []
    for name in args.cases.split(","):
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"case {name} failed with status {r.returncode}: stopping (no further GPU steps)")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
    if not args.small:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/est_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
