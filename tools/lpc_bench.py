"""Time Burg's recursion (mdsp_burg_*, src/lpc.jl:53-92) on the device, per order.

    python tools/lpc_bench.py [--reps R] [--warmup W] [--cases f32_24,f64_24,f32_26,f64_26] [--out profiles/lpc_bench.json] [--small]

A case is one Float32 / Float64 column of 2^24 / 2^26 samples of coloured noise, device-resident.  Per case, after warm-up, the MEDIAN of R >= 10
device-event-timed calls (no profiler) of mdsp_burg_exec at p = 2 and at p = 10:
    ms_p2, ms_p10   the whole call (2 p launches)
    ms_per_order    (ms_p10 - ms_p2) / 8: one finish and one sweep, which reads and writes both work arrays: 4 sizeof(T) bytes per sample
    GBps            those bytes over ms_per_order
    copy_ms         mdsp_copy_bench of 2 n sizeof(T) bytes into a second buffer: the same bytes read and the same bytes written as one sweep
    copy_frac       copy_ms / ms_per_order
    S, seglen       from mdsp_burg_plan_info
and the record at p = 10 equals mdsp_burg_emulate_host of the same array bit for bit.  --small divides every length by 64 (a dry run of the tool itself).
Each case runs in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"f32_24": ("float32", 1 << 24), "f64_24": ("float64", 1 << 24), "f32_26": ("float32", 1 << 26), "f64_26": ("float64", 1 << 26)}
P_LO, P_HI = 2, 10


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, reps, warmup, small):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev

    dtype, n = CASES[name]
    if small:
        n //= 64
    dt = np.dtype(dtype)
    _lib.check(_lib.lib().mdsp_init(0))
    rng = np.random.default_rng(1776)
    s = rng.standard_normal(n + 2)
    xh = s[2:] + 0.6 * s[1:-1] + 0.3 * s[:-2]                    # coloured noise: reflection coefficients that are not zero
    xh = xh.astype(dt)
    x = torch.from_numpy(xh).cuda()
    lib, stream = _lib.lib(), _dev.stream_ptr()
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

    nbytes = 2 * n * dt.itemsize
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    copy_ms = bench(lambda: _lib.check(lib.mdsp_copy_bench(dst.data_ptr(), src.data_ptr(), nbytes, stream)))
    del src, dst
    plan = d.BurgPlan(dt, n)
    rec = torch.zeros(2 * P_HI + 2, dtype=x.dtype, device="cuda")
    ms_lo = bench(lambda: plan.exec(x.data_ptr(), P_LO, rec.data_ptr(), stream))
    ms_hi = bench(lambda: plan.exec(x.data_ptr(), P_HI, rec.data_ptr(), stream))
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    want = np.zeros(2 * P_HI + 2, dtype=dt)
    _lib.check(lib.mdsp_burg_emulate_host(xh.ctypes.data, _dev.md_dtype(dt), n, 0, P_HI, want.ctypes.data))
    per = (ms_hi - ms_lo) / (P_HI - P_LO)
    row = {"case": name, "dtype": dtype, "n": n, "reps": reps, "S": plan.segments, "seglen": plan.seglen, "workspace_bytes": plan.workspace_bytes,
           "ms_p2": round(ms_lo, 4), "ms_p10": round(ms_hi, 4), "ms_per_order": round(per, 4), "GBps": round(2 * nbytes / per / 1e6, 1),
           "copy_ms": round(copy_ms, 4), "copy_frac": round(copy_ms / per, 3), "record_equal_to_emulation": bool(got.tobytes() == want.tobytes())}
    assert row["record_equal_to_emulation"], f"{name}: the device record {got} differs from the host emulation {want}"
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpc_bench.json"))
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
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
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
            json.dump({"tool": "tools/lpc_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
