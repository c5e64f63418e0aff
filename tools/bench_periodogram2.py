"""Time the 2-D periodogram (periodogram(s::AbstractMatrix{<:Real}; nfft, radialsum / radialavg), periodograms.jl:473-509) on the device.

    python tools/bench_periodogram2.py [--steps K] [--warmup W] [--sizes 2048,4096,...] [--profile OUTDIR]

Sizes: 2048^2, 4096^2, 8192^2 and 3000 x 2000 (nfft = nextfastfft of each dimension); Float32 and Float64; full and radialsum; the
fused engine and rocFFT.  One table row per case: ms per call (device events around K back-to-back calls on a cached plan, device-resident
input and output), and the effective rate (input bytes + output bytes) / time.  The traffic the route itself moves is larger (DESIGN.md
"2-D periodogram").  With --profile OUTDIR the same cases run again, each in a child process under
``timeout -k 10 600 rocprofv3 --kernel-trace --stats -f csv`` writing to OUTDIR/<case>, and the per-kernel split (time share of each kernel name)
is printed after the table.  Every GPU step is a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"2048": (2048, 2048), "4096": (4096, 4096), "8192": (8192, 8192), "3000x2000": (3000, 2000)}
DTYPES = ("float32", "float64")
MODES = ("full", "radialsum")
ENGINES = {"fused": 1, "rocfft": 2}


def run_case(size, dtype, mode, engine, steps, warmup):
    """One case in this process: returns a dict row."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsp_jl_amd as d
    n1, n2 = SIZES[size]
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((n2, n1), generator=g, device="cuda", dtype=getattr(torch, dtype)).t()    # (n1, n2), first axis contiguous
    kw = {"radialsum": True} if mode == "radialsum" else {}
    p = d.periodogram(x, engine=ENGINES[engine], **kw)
    for _ in range(warmup):
        p = d.periodogram(x, engine=ENGINES[engine], **kw)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        p = d.periodogram(x, engine=ENGINES[engine], **kw)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    nbytes = x.numel() * x.element_size() + p.power.numel() * p.power.element_size()
    N1, N2 = d.nextfastfft((n1, n2))
    return {"size": size, "nfft": [N1, N2], "dtype": dtype, "mode": mode, "engine": engine, "ms": round(ms, 4),
            "TBps": round(nbytes / (ms * 1e-3) / 1e12, 3), "bytes": int(nbytes)}


def child(args, case, extra=()):
    cmd = ["timeout", "-k", "10", "600", *extra, sys.executable, os.path.abspath(__file__), "--case", ",".join(case),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"case {case} failed with status {r.returncode}: stopping (no further GPU steps)")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def kernel_split(outdir):
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    return sorted(((r["Name"][:70], int(r["Calls"]), float(r["TotalDurationNs"]) / total) for r in rows), key=lambda t: -t[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(SIZES))
    ap.add_argument("--profile", default="")
    ap.add_argument("--case", default="")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(*args.case.split(","), args.steps, args.warmup)), flush=True)
        return
    cases = [(s, dt, m, e) for s in args.sizes.split(",") for dt in DTYPES for m in MODES for e in ENGINES]
    print(f"{'size':>10} {'nfft':>12} {'dtype':>8} {'mode':>10} {'engine':>7} {'ms':>9} {'TB/s':>7}")
    for case in cases:
        for r in child(args, case):
            print(f"{r['size']:>10} {'x'.join(map(str, r['nfft'])):>12} {r['dtype']:>8} {r['mode']:>10} {r['engine']:>7} {r['ms']:>9.3f} {r['TBps']:>7.3f}", flush=True)
    if args.profile:
        for case in cases:
            out = os.path.join(args.profile, "_".join(case))
            child(args, case, ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "p2", "--"])
            print(f"-- {' '.join(case)}: kernel time shares")
            for name, calls, share in kernel_split(out)[:8]:
                print(f"   {share * 100:5.1f} %  {calls:6d}  {name}")


if __name__ == "__main__":
    main()
