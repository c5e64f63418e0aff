"""Time rms, meanfreq, finddelay and the in-place shiftsignal_ (dsp.jl_amd/util.py; mdsp_reduce_*, mdsp_shift_*) on the device.

    python tools/util_bench.py [--reps R] [--warmup W] [--cases rms_line,...] [--out profiles/util_bench.json] [--small]

Cases:  rms_line            rms of one Float32 line of 2^28 samples                                   (contiguous, cut into segments, then the finish)
        rms_rows, rms_cols  rms along each axis of a 4096 x 2^16 Float32 matrix: dims=1 (contiguous lines) and dims=0 (strided)
        meanfreq            meanfreq of 2^24 Float32 samples (transform, then one SUMABS2_W pass over the bins)
        finddelay           two Float32 lines of 2^22 samples, split into the correlation (xcorr) and the arg-max (ABSARGMAX)
        shift_halo, shift_quarter, shift_disjoint   shiftsignal_ in place on 2^28 Float32 samples, s = 100, 2^26 and 2^27 + 1
Per case, after warm-up, the MEDIAN of R >= 10 device-event-timed calls (no profiler) on device-resident arrays, alternated call by call with the torch
composition of the same result (x.square().mean().sqrt(); abs().argmax(); clone and slice-assign; rfft, abs, square, two sums):
    ms, torch_ms       one call of ours / of the composition
    bytes_per_sample   what our kernels move per input sample (reads + writes, workspace traffic included), from the plan
    GBps, copy_frac    that over the time, and as a fraction of the rate of mdsp_copy_bench (read + write) on buffers of the same size in the same process
Each case checks its result against the composition at the timed size.  --small divides every size by 64 (a dry run of the tool itself).  Each case runs
in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rms_line", "rms_rows", "rms_cols", "meanfreq", "finddelay", "shift_halo", "shift_quarter", "shift_disjoint")


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, reps, warmup, small):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev
    _lib.check(_lib.lib().mdsp_init(0))
    lib, stream = _lib.lib(), _dev.stream_ptr()
    div = 64 if small else 1
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def bench(fn, other=None):
        for _ in range(warmup):
            fn()
            if other:
                other()
        a, b = [], []
        for _ in range(reps):
            a.append(timed(fn))
            if other:
                b.append(timed(other))
        return median(a), (median(b) if other else None)

    def copy_rate(nbytes):
        """GB/s (read + write) of the library's best copy kernel on two buffers of nbytes"""
        nbytes -= nbytes % 16
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ms, _ = bench(lambda: _lib.check(lib.mdsp_copy_bench(dst.data_ptr(), src.data_ptr(), nbytes, stream)))
        return 2 * nbytes / ms / 1e6, ms

    row = {"case": name, "reps": reps}
    hold = []

    def finish(samples, nbytes_in, bytes_moved, ms, torch_ms, extra=None):
        rate, copy_ms = copy_rate(nbytes_in)
        row.update(samples=samples, ms=round(ms, 4), torch_ms=round(torch_ms, 4), bytes_per_sample=round(bytes_moved / samples, 3),
                   GBps=round(bytes_moved / ms / 1e6, 1), copy_ms=round(copy_ms, 4), copy_GBps=round(rate, 1), copy_frac=round(bytes_moved / ms / 1e6 / rate, 3),
                   faster_than_torch=bool(ms < torch_ms))
        row.update(extra or {})
        return row

    if name.startswith("rms"):
        shape, dims = {"rms_line": (((1 << 28) // div,), None), "rms_rows": ((4096 // div, 1 << 16), 1), "rms_cols": ((4096 // div, 1 << 16), 0)}[name]
        x = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
        n = x.numel()

        def ours():
            hold[:] = [d.rms(x, dims=dims)]

        def comp():
            hold[:] = [x.square().mean().sqrt() if dims is None else x.square().mean(dim=dims, keepdim=True).sqrt()]

        ms, torch_ms = bench(ours, comp)
        ours()
        got = hold[0].double().cpu().numpy()
        comp()
        ref = hold[0].double().cpu().numpy()
        err = float(np.max(np.abs(got - ref) / ref))
        assert err < 1e-5, err
        inner, length, outer = (1, n, 1) if dims is None else (1, shape[1], shape[0]) if dims == 1 else (shape[1], shape[0], 1)
        route, S, seglen, depth, ws = d.reduce_geometry(inner, length, outer, _lib.REDUCE_SUMABS2, np.float32)
        moved = 4 * n + (2 * ws if S > 1 else 0) + 8 * inner * outer
        return finish(n, 4 * n, moved, ms, torch_ms, dict(route="contiguous" if route == 0 else "strided", S=S, seglen=seglen, depth=depth, max_rel_diff_to_torch=err))
    if name == "meanfreq":
        n = (1 << 24) // div
        x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32) + torch.sin(0.3 * torch.arange(n, device="cuda", dtype=torch.float32))
        f = torch.arange(n // 2 + 1, device="cuda", dtype=torch.float64) * (2 * np.pi / n)

        def ours():
            hold[:] = [d.meanfreq(x)]

        def comp():
            p = torch.fft.rfft(x).abs().square()
            hold[:] = [(p * f).sum() / p.sum()]

        ms, torch_ms = bench(ours, comp)
        ours()
        got = hold[0].item()
        comp()
        ref = hold[0].item()
        assert abs(got - ref) < 2e-5 * abs(ref), (got, ref)
        plan = d.ReducePlan(1, n // 2 + 1, 1, _lib.REDUCE_SUMABS2_W, np.complex64, step=2 * np.pi / n)
        bins = torch.randn(n // 2 + 1, generator=g, device="cuda", dtype=torch.float32).to(torch.complex64)
        out = torch.empty(2, dtype=torch.float64, device="cuda")
        red_ms, _ = bench(lambda: plan.exec(bins.data_ptr(), out.data_ptr(), stream))
        return finish(n, 4 * n, 8 * (n // 2 + 1) + 2 * plan.workspace_bytes, red_ms, torch_ms,
                      dict(whole_call_ms=round(ms, 4), reduction_ms=round(red_ms, 4), S=plan.segments, value=got, torch_value=ref,
                           note="ms, GBps and copy_frac are the SUMABS2_W pass over the bins alone; whole_call_ms includes the transform and is what torch_ms is compared with (faster_than_torch)",
                           faster_than_torch=bool(ms < torch_ms)))
    if name == "finddelay":
        n, delay = (1 << 22) // div, 12345 // div
        y = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
        x = torch.zeros_like(y)
        x[delay:] = y[:n - delay]
        x += 0.1 * torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
        corr_ms, _ = bench(lambda: hold.__setitem__(slice(None), [d.xcorr(y, x)]))
        s = d.xcorr(y, x).contiguous()
        plan = d.ReducePlan(1, s.numel(), 1, _lib.REDUCE_ABSARGMAX, np.float32, centre=n - 1)
        rec = torch.empty(2, dtype=torch.int64, device="cuda")
        arg_ms, torch_ms = bench(lambda: plan.exec(s.data_ptr(), rec.data_ptr(), stream), lambda: hold.__setitem__(slice(None), [s.abs().argmax()]))
        whole_ms, _ = bench(lambda: d.finddelay(x, y))
        assert d.finddelay(x, y) == delay and int(s.abs().argmax().item()) == n - 1 - delay
        return finish(s.numel(), 4 * s.numel(), 4 * s.numel() + 2 * plan.workspace_bytes, arg_ms, torch_ms,
                      dict(correlation_ms=round(corr_ms, 4), argmax_ms=round(arg_ms, 4), whole_call_ms=round(whole_ms, 4), S=plan.segments,
                           note="ms and torch_ms are the arg-max over the 2n-1 correlation samples alone; the correlation is the existing xcorr"))
    n = (1 << 28) // div
    s = {"shift_halo": 100, "shift_quarter": n // 4, "shift_disjoint": n // 2 + 1}[name]
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    route, tile, chunk, ntiles, ws = d.shift_geometry(n, s, 4, True)

    def comp():
        t = x.clone()
        x[s:] = t[:n - s]
        x[:s] = 0

    ms, torch_ms = bench(lambda: d.shiftsignal_(x, s), comp)
    x0 = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    x.copy_(x0)
    d.shiftsignal_(x, s)
    assert bool((x[s:] == x0[:n - s]).all()) and bool((x[:s] == 0).all())
    moved = {_lib.SHIFT_DISJOINT: 4 * (n - s) * 2 + 4 * s + 4 * min(n - s, s), _lib.SHIFT_HALO: 8 * n + 2 * ws, _lib.SHIFT_STAGED: 4 * (n - s) * 2 + 8 * n - 4 * s}[route]
    return finish(n, 4 * n, moved, ms, torch_ms, dict(s=s, route={1: "DISJOINT", 2: "HALO", 3: "STAGED"}[route], tile=tile, chunk=chunk, ntiles=ntiles, workspace_bytes=ws))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "util_bench.json"))
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--case", default="")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("--reps must be at least 10")
    if args.case:
        print(json.dumps(run_case(args.case, args.reps, args.warmup, args.small)), flush=True)
        return
    rows = []
    for name in args.cases.split(","):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"case {name} failed with status {r.returncode}: stopping (no further GPU steps)")
        row = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")][-1]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not args.small:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/util_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")
    slow = [r["case"] for r in rows if not r["faster_than_torch"]]
    print("every case faster than the torch composition" if not slow else f"NOT faster than the torch composition: {slow}")


if __name__ == "__main__":
    main()
