"""Time esprit (mdsp_hankel_gram_*, src/estimation.jl:67-75) on the device, beside the SVD route on the host.

    python tools/esprit_bench.py [--reps R] [--warmup W] [--cases ref,mid,wide,long,real,big] [--out profiles/esprit_bench.json] [--small]

A case is one device-resident signal of N samples (three cisoids, or three real tones, in noise of 0.1) and a matrix size M; p = 3 (6 for the real
signal).  Per case, after warm-up:
    gram_ms      the MEDIAN of R >= 10 device-event-timed calls (no profiler) of mdsp_hankel_gram_exec: the body launch and the assembly
    Gterms       N M / gram_ms: products x[k + d] conj(x[k]) per second, in 1e9
    esprit_ms    the median wall-clock time of R whole esprit(x, M, p) calls on the device tensor: the two launches, the copy of R, eigh, lstsq, eigvals
    svd_ms       ONE wall-clock run of the reference's route with numpy on the host for the same samples (the Hankel matrix, numpy.linalg.svd, lstsq,
                 eigvals; tests/esprit_ref.py restates the same lines); null where the M x (N - M + 1) matrix would exceed 1 GiB
    route_diff   max |f_device - f_svd| / Fs, both sorted (Fs = 1)
    S, seglen    from mdsp_hankel_gram_plan_info
and R equals mdsp_hankel_gram_emulate_host of the same array bit for bit where N M <= 2e8 (the emulation is one host thread).  --small divides every
length by 16 (a dry run of the tool itself).  Each case runs in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"ref": ("complex128", 10000, 300), "mid": ("complex128", 1 << 16, 64), "wide": ("complex128", 1 << 17, 256), "long": ("complex128", 1 << 20, 16),
         "real": ("float32", 1 << 20, 64), "big": ("complex128", 1 << 20, 1024)}
SVD_MAX_BYTES = 1 << 30
EMULATE_MAX_TERMS = 2e8


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, reps, warmup, small):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev

    dtype, n, M = CASES[name]
    if small:
        n = max(n // 16, 2 * M - 1)
    dt = np.dtype(dtype)
    cplx = dt.kind == "c"
    p = 3 if cplx else 6
    _lib.check(_lib.lib().mdsp_init(0))
    rng = np.random.default_rng(1986)
    t = np.arange(n)
    tones = ((1.0, 0.0731, 0.1), (0.5, 0.2917, 0.7), (0.25, 0.4113, -0.3))
    if cplx:
        xh = sum(a * np.exp(2j * np.pi * (f * t + ph)) for a, f, ph in tones) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    else:
        xh = sum(a * np.cos(2 * np.pi * (f * t + ph)) for a, f, ph in tones) + 0.1 * rng.standard_normal(n)
    xh = xh.astype(dt)
    x = torch.from_numpy(xh).cuda()
    stream = _dev.stream_ptr()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    plan = d.GramPlan(dt, n, M)
    r = torch.zeros((M, M), dtype=_dev.torch_dtype(plan.out_dtype), device="cuda")
    for _ in range(warmup):
        plan.exec(x.data_ptr(), r.data_ptr(), M, stream)
    times = []
    for _ in range(reps):
        ev[0].record()
        plan.exec(x.data_ptr(), r.data_ptr(), M, stream)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    gram_ms = median(times)
    equal = None
    if n * M <= EMULATE_MAX_TERMS:
        want = np.zeros((M, M), dtype=plan.out_dtype)
        _lib.check(_lib.lib().mdsp_hankel_gram_emulate_host(xh.ctypes.data, _dev.md_dtype(dt), n, M, 0, want.ctypes.data, M))
        equal = bool(r.cpu().numpy().tobytes() == want.tobytes())
        assert equal, f"{name}: the device Gram matrix differs from the host emulation"
    for _ in range(warmup):
        f_dev = d.esprit(x, M, p)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f_dev = d.esprit(x, M, p)
        times.append(1e3 * (time.perf_counter() - t0))
    esprit_ms = median(times)
    svd_ms = route_diff = None
    if M * (n - M + 1) * 16 <= SVD_MAX_BYTES:
        t0 = time.perf_counter()
        X = np.lib.stride_tricks.sliding_window_view(xh.astype(np.complex128 if cplx else np.float64), n - M + 1)[:M]
        U = np.linalg.svd(X, full_matrices=False)[0]
        f_svd = np.angle(np.linalg.eigvals(np.linalg.lstsq(U[:-1, :p], U[1:, :p], rcond=None)[0])) / (2 * np.pi)
        svd_ms = 1e3 * (time.perf_counter() - t0)
        route_diff = float(np.max(np.abs(np.sort(f_dev) - np.sort(f_svd))))
    row = {"case": name, "dtype": dtype, "n": n, "M": M, "p": p, "reps": reps, "S": plan.segments, "seglen": plan.seglen, "workspace_bytes": plan.workspace_bytes,
           "gram_ms": round(gram_ms, 4), "Gterms": round(n * M / gram_ms / 1e6, 2), "esprit_ms": round(esprit_ms, 3),
           "svd_ms": None if svd_ms is None else round(svd_ms, 1), "route_diff": route_diff, "gram_equal_to_emulation": equal}
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esprit_bench.json"))
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
            json.dump({"tool": "tools/esprit_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
