"""Time the filter-response kernels (mdsp_resp_*, Filters/response.jl:27-52) on the device.

    python tools/response_bench.py [--reps R] [--warmup W] [--cases poly_long,poly_square,poly_short,sections8] [--dtype float64] [--out profiles/response_bench.json] [--small]

Cases (coefficients nb, points nw):
        poly_long    POLY  2^19 x 257     the shape the cut exists for: the default 257 points of freqresp(f) on the longest filter the library takes
        poly_square  POLY  2^16 x 2^16
        poly_short   POLY  64 x 2^20
        sections8    SECTIONS  K = 8 x 2^20
each with the automatic cut and with chunks = 1 (for SECTIONS, which is never cut, the second run is the same plan again).  Per run, after warm-up, the
MEDIAN of R >= 10 device-event-timed calls (no profiler), POINTS input and COMPLEX output on device-resident arrays:
    ms            the time of one mdsp_resp_exec
    Gstep_per_s   nb x nw complex multiply-adds (K x nw biquad values) over that time
    C, L          from mdsp_resp_plan_info
    copy_GBps     mdsp_copy_bench over 256 MiB in the same process: the yardstick of the box the numbers come from
Correctness at the timed size: the first 64 points equal mdsp_resp_emulate_host with the same cut bit for bit.  --small divides nb and nw by 64 (a dry
run of the tool itself).  Each case runs in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"poly_long": ("poly", 1 << 19, 257), "poly_square": ("poly", 1 << 16, 1 << 16), "poly_short": ("poly", 64, 1 << 20), "sections8": ("sections", 8, 1 << 20)}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, dtype, reps, warmup, small):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ctypes as C
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev
    from sos_bench import butter_sections

    kind, nb, nw = CASES[name]
    if small:
        nb, nw = (max(nb // 64, 17) if kind == "poly" else nb), max(nw // 64, 65)
    R = np.dtype(dtype)
    ct = np.dtype(np.complex64 if R == np.dtype(np.float32) else np.complex128)
    _lib.check(_lib.lib().mdsp_init(0))
    lib, stream = _lib.lib(), _dev.stream_ptr()
    rng = np.random.default_rng(1776)
    if kind == "poly":
        form, gain = _lib.RESP_POLY, 1.0
        k = np.arange(nb) - (nb - 1) / 2
        num = (0.4 * np.sinc(0.4 * k) * np.hamming(nb)).astype(R).astype(np.float64)       # a windowed-sinc low-pass of nb taps
    else:
        form = _lib.RESP_SECTIONS
        num, gain = butter_sections(nb)
        num = num.reshape(-1)
    pts = np.exp(-1j * np.sort(rng.uniform(0, np.pi, nw))).astype(ct)
    x = torch.from_numpy(pts).cuda()
    y = torch.empty_like(x)
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

    cb = 256 << 20
    ca, cbuf = torch.empty(cb, dtype=torch.uint8, device="cuda"), torch.empty(cb, dtype=torch.uint8, device="cuda")
    copy_ms = bench(lambda: _lib.check(lib.mdsp_copy_bench(cbuf.data_ptr(), ca.data_ptr(), cb, stream)))
    rows = []
    for chunks in (0, 1):
        plan = d.RespPlan(form, R, num, None, gain, nw, 0, _lib.RESP_COMPLEX, _lib.RESP_POINTS, 0.0, chunks)
        ms = bench(lambda: plan.exec(x.data_ptr(), y.data_ptr(), stream))
        row = {"case": name, "dtype": dtype, "form": kind, "nb": nb, "nw": nw, "chunks_arg": chunks, "C": plan.chunks, "L": plan.chunk_len,
               "workspace_bytes": plan.workspace_bytes, "reps": reps, "ms": round(ms, 4), "Gstep_per_s": round(nb * nw / ms / 1e6, 2),
               "copy_ms_256MiB": round(copy_ms, 4), "copy_GBps": round(2 * cb / copy_ms / 1e6, 1)}
        take = min(nw, 64)
        want = np.zeros(take, ct)
        head = np.ascontiguousarray(pts[:take])
        nv = np.ascontiguousarray(num, np.float64)
        # the emulation cuts by the same rule only when it is told the plan's own cut (the automatic one depends on nw)
        _lib.check(lib.mdsp_resp_emulate_host(head.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p), form, 0, _lib.RESP_COMPLEX, _dev.md_dtype(R),
                                              nv.ctypes.data_as(_lib.pdbl), nb, None, 0, float(gain), 0.0, take, plan.chunks))
        torch.cuda.synchronize()
        row["prefix_equal_to_emulation"] = bool(np.array_equal(y[:take].cpu().numpy().view(np.uint8), want.view(np.uint8)))
        assert row["prefix_equal_to_emulation"], f"{name} chunks {chunks}: device result differs from the host emulation"
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "response_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", default="")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    if args.case:
        for row in run_case(args.case, args.dtype, args.reps, args.warmup, args.small):
            print(json.dumps(row), flush=True)
        return
    rows = []
    for name in args.cases.split(","):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--dtype", args.dtype]
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
            json.dump({"tool": "tools/response_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
