"""Time filt(sos, x) (mdsp_sos_*, Filters/filt.jl:35-65) on the device.

    python tools/sos_bench.py [--reps R] [--warmup W] [--cases one32,one64,many32,many64] [--sections 1,2,4,8] [--out profiles/sos_bench.json] [--small]

Cases:  one32 / one64    one Float32 / Float64 column of 2^28 samples          (cut into segments: reduce, carries, apply)
        many32 / many64  64 columns of 2^22 samples                            (plan_info says whether it is cut)
Per case and section count K (Butterworth low-pass of order 2K at 0.2, designed here with numpy), after warm-up, the
MEDIAN of R >= 10 device-event-timed calls (no profiler), out of place on device-resident columns:
    ms          the time of one mdsp_sos_exec
    GBps_alg    2 sizeof(T) bytes per sample over that time (what a single pass must move; a cut line moves 1.5 x as much)
    copy_frac   that rate as a fraction of mdsp_copy_bench on the SAME two buffers in the same process
    S, seglen   from mdsp_sos_plan_info
    forced1_ms  a cut case of at least 64 columns once more with the cut forced to 1 segment per column
Correctness at the timed size: the first 2^16 samples of column 0 equal mdsp_sos_emulate_host of that prefix bit for bit where the column is not cut
(a cut changes the start states by rounding), and agree with it to 1e-4 relative where it is.  --small divides every length by 64 (a dry run of the tool
itself).  Each case runs in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"one32": ("float32", 1 << 28, 1), "one64": ("float64", 1 << 28, 1), "many32": ("float32", 1 << 22, 64), "many64": ("float64", 1 << 22, 64)}


def butter_sections(K, wn=0.2):
    """Butterworth low-pass of order 2K at wn (x pi rad/sample) as K sections and a gain: analog prototype, pre-warped, bilinear transform."""
    import numpy as np
    N = 2 * K
    warped = 4.0 * np.tan(np.pi * wn / 2.0)
    p = warped * np.exp(1j * np.pi * (2 * np.arange(K) + N + 1) / (2 * N))        # the upper half of the analog poles
    pz = (4.0 + p) / (4.0 - p)
    rows, g = [], 1.0
    for q in pz:
        a1, a2 = -2.0 * q.real, abs(q) ** 2
        rows.append((1.0, 2.0, 1.0, a1, a2))
        g *= (1.0 + a1 + a2) / 4.0                                                  # unit gain at 0
    return np.array(rows), g


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, sections, reps, warmup, small):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev

    def emulate(tb, gain, xh):
        """mdsp_sos_emulate_host on one host column, uncut"""
        tb = np.ascontiguousarray(tb, np.float64)
        yh = np.empty_like(xh)
        _lib.check(_lib.lib().mdsp_sos_emulate_host(xh.ctypes.data_as(C.c_void_p), len(xh), yh.ctypes.data_as(C.c_void_p), len(xh), None,
                                                    tb.ctypes.data_as(_lib.pdbl), len(tb), float(gain), 1, _dev.md_dtype(xh.dtype), len(xh), 1, 1, 0))
        return yh
    dtype, n, ncols = CASES[name]
    if small:
        n //= 64
    dt = np.dtype(dtype)
    _lib.check(_lib.lib().mdsp_init(0))
    g = torch.Generator(device="cuda")
    g.manual_seed(1776)
    x = torch.randn((ncols, n), generator=g, device="cuda", dtype=getattr(torch, dtype))
    y = torch.empty_like(x)
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

    nbytes = x.numel() * x.element_size()
    copy_ms = bench(lambda: _lib.check(lib.mdsp_copy_bench(y.data_ptr(), x.data_ptr(), nbytes, stream)))
    rows = []
    for K in sections:
        tb, gain = butter_sections(K)
        plan = d.SosPlan(tb, gain, dt, n, ncols)
        ms = bench(lambda: plan.exec(x.data_ptr(), n, y.data_ptr(), n, None, False, stream))
        row = {"case": name, "dtype": dtype, "K": K, "n": n, "ncols": ncols, "reps": reps, "bytes_alg": 2 * nbytes, "copy_ms": round(copy_ms, 4),
               "copy_GBps": round(2 * nbytes / copy_ms / 1e6, 1), "S": plan.segments, "seglen": plan.seglen, "workspace_bytes": plan.workspace_bytes,
               "ms": round(ms, 4), "GBps_alg": round(2 * nbytes / ms / 1e6, 1), "copy_frac": round(copy_ms / ms, 3)}
        if plan.segments > 1 and ncols >= 64:       # (one wavefront walking a whole 2^28-sample column alone takes seconds: not timed)
            p1 = d.SosPlan(tb, gain, dt, n, ncols, 1)
            row["forced1_ms"] = round(bench(lambda: p1.exec(x.data_ptr(), n, y.data_ptr(), n, None, False, stream)), 4)
        plan.exec(x.data_ptr(), n, y.data_ptr(), n, None, False, stream)
        torch.cuda.synchronize()
        take = min(n, 1 << 16)
        want = emulate(tb, gain, np.ascontiguousarray(x[0, :take].cpu().numpy()))
        got = y[0, :take].cpu().numpy()
        if plan.segments == 1 or plan.seglen >= take:
            row["prefix_equal_to_emulation"] = bool(np.array_equal(got, want))
            assert row["prefix_equal_to_emulation"], f"{name} K {K}: device result differs from the host emulation"
        else:
            err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            row["prefix_rel_err"] = err
            assert err < 1e-4, f"{name} K {K}: {err}"
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--sections", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sos_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", default="")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    sections = [int(k) for k in args.sections.split(",")]
    if args.case:
        for row in run_case(args.case, sections, args.reps, args.warmup, args.small):
            print(json.dumps(row), flush=True)
        return
    rows = []
    for name in args.cases.split(","):
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--sections", args.sections]
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
            json.dump({"tool": "tools/sos_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
