"""Time unwrap along one dimension (mdsp_unwrap_*, src/unwrap.jl:17-34) on the device.

    python tools/unwrap_bench.py [--reps R] [--warmup W] [--cases a,b,c,da,dc] [--out profiles/unwrap_bench.json] [--small]

Cases:  a   one Float32 line of 2^28 samples                                   (contiguous, cut into segments)
        b   phases of 4 channels x (1024 bins x 262141 frames) Float32, unwrapped across frames  (strided; plan_info says whether it is cut)
        c   the same array along frequency                                     (contiguous, a million short lines, single pass)
        da  case a in Float64          dc  case c in Float64
Per case, after warm-up, the MEDIAN of R >= 10 device-event-timed calls (no profiler), out of place on device-resident arrays:
    ms          the time of one mdsp_unwrap_exec
    GBps_alg    2 sizeof(T) bytes per sample over that time (what a single pass must move; the segmented route moves 1.5 x as much)
    copy_frac   that rate as a fraction of mdsp_copy_bench on the SAME two buffers in the same process (a segmented case cannot pass 2/3)
    route, S    from mdsp_unwrap_plan_info
    torch_ms    the composition a user has today on the device, m - range * cumsum(round(diff(m) / range)) with torch, alternated call by call with ours
    forced      case a and b also with the cut forced to 1 (and b to the automatic S of a, where that differs), to compare the routes
Correctness at the timed size: case c (and dc) whole and a 2^26 prefix of case a (and da) equal unwrap_scan (tests/unwrap_ref.py) on the host, bit for
bit; the inputs satisfy the exactness condition of tests/unwrap_cases.py (asserted on the compared part).  --small divides every size by 64 (a dry run of
the tool itself).  Each case runs in a child process under a time limit; the tool stops at the first that fails.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, BINS, CHANNELS = 262_141, 1024, 4
# dtype, the (outer, len, inner) array that is generated, and the axis of it that is unwrapped (1: len, 2: inner -- the same memory read along bins)
CASES = {"a": ("float32", (1, 1 << 28, 1), 1), "b": ("float32", (CHANNELS, FRAMES, BINS), 1), "c": ("float32", (CHANNELS, FRAMES, BINS), 2),
         "da": ("float64", (1, 1 << 28, 1), 1), "dc": ("float64", (CHANNELS, FRAMES, BINS), 2)}


def phases(torch, shape, dtype, seed):
    """Wrapped phases on the device whose increments are +-2.0 +- 0.4 rad along axis 1 (a triangle of period 2^20 samples, so |K| stays below 1.7e5 and
    inside the Float32 range) and -1.7 +- 0.4 rad along axis 2: tie margin >= 0.118 along both."""
    outer, n, inner = shape
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    P = 1 << 20
    j = torch.arange(n, device="cuda", dtype=torch.float64)
    tri = (torch.remainder(j, P) - P / 2).abs()
    out = torch.empty(shape, device="cuda", dtype=dtype)
    two_pi = 2 * torch.pi
    for o in range(outer):                                  # a channel at a time: the Float64 temporaries stay small
        u = 2.0 * tri[:, None] - 1.7 * torch.arange(inner, device="cuda", dtype=torch.float64)[None, :]
        u += (torch.rand((n, inner), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 0.4
        out[o] = (u - two_pi * torch.round(u / two_pi)).to(dtype)
        del u
    return out


def torch_composition(torch, m, r):
    k = torch.cumsum(torch.round(torch.diff(m, dim=1) / r), dim=1)
    y = m.clone()
    y[:, 1:] -= r * k
    return y


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run_case(name, reps, warmup, small):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import dsp_jl_amd as d
    from dsp_jl_amd import _lib, _dev
    import unwrap_ref as ur
    dtype, gen, axis = CASES[name]
    if small:
        gen = (gen[0], gen[1] // 64, gen[2])
    dt = np.dtype(dtype)
    tdt = getattr(torch, dtype)
    _lib.check(_lib.lib().mdsp_init(0))
    m = phases(torch, gen, tdt, 7)
    if axis == 2:
        m = m.view(gen[0] * gen[1], gen[2], 1)                # the same memory, the bins of every frame as lines
    outer, n, inner = m.shape
    y = torch.empty_like(m)
    r = float(ur.default_range(dt))
    lib, stream = _lib.lib(), _dev.stream_ptr()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def bench(fn, other=None):
        """median ms of fn (and of `other`, alternated with it call by call)"""
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

    nbytes = m.numel() * m.element_size()
    row = {"case": name, "dtype": dtype, "inner": inner, "len": n, "outer": outer, "reps": reps, "bytes_alg": 2 * nbytes}
    copy_ms, _ = bench(lambda: _lib.check(lib.mdsp_copy_bench(y.data_ptr(), m.data_ptr(), nbytes, stream)))
    row["copy_ms"], row["copy_GBps"] = round(copy_ms, 4), round(2 * nbytes / copy_ms / 1e6, 1)
    plan = d.UnwrapPlan(inner, n, outer, dt, r)
    hold = []

    def torch_call():
        hold[:] = [torch_composition(torch, m, r)]

    ours_ms, torch_ms = bench(lambda: plan.exec(m.data_ptr(), y.data_ptr(), stream), torch_call)
    hold.clear()
    row.update(route="contiguous" if plan.route == _lib.UNWRAP_CONTIGUOUS else "strided", S=plan.segments, seglen=plan.seglen,
               workspace_bytes=plan.workspace_bytes, ms=round(ours_ms, 4), GBps_alg=round(2 * nbytes / ours_ms / 1e6, 1),
               copy_frac=round(copy_ms / ours_ms, 3), torch_ms=round(torch_ms, 4), faster_than_torch=bool(ours_ms < torch_ms))
    forced = {}
    for seg in ([1] if plan.segments > 1 else []) + ([64, 512] if inner > 1 else []):
        p2 = d.UnwrapPlan(inner, n, outer, dt, r, seg)
        if p2.segments != plan.segments:
            forced[str(p2.segments)] = round(bench(lambda: p2.exec(m.data_ptr(), y.data_ptr(), stream))[0], 4)
    row["forced_segments_ms"] = forced
    # correctness at the timed size
    plan.exec(m.data_ptr(), y.data_ptr(), stream)
    torch.cuda.synchronize()
    if inner == 1:
        take = min(n, 1 << 26) if outer == 1 else n
        worst, ok, lines = 0.5, True, max(1, (1 << 24) // take)
        for o0 in range(0, outer, lines):                   # a slab of lines at a time through the host
            mh, yh = m[o0:o0 + lines, :take, 0].cpu().numpy(), y[o0:o0 + lines, :take, 0].cpu().numpy()
            need = 0.01 + 4 * float(np.finfo(dt).eps) * ur.max_count(mh, 1, r)
            worst = min(worst, ur.tie_margin(mh, 1, r))
            assert worst >= need, f"input near a tie: margin {worst} < {need}"
            ok = ok and ur.equal(yh, ur.unwrap_scan(mh, 1, r))
        row.update(checked_samples=int(take * outer), equal_to_host_scan=bool(ok), tie_margin=round(worst, 4))
        assert ok, f"case {name}: device result differs from unwrap_scan on the host"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unwrap_bench.json"))
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
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
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
            json.dump({"tool": "tools/unwrap_bench.py", "rows": rows}, f, indent=1)
            f.write("\n")
    slow = [r["case"] for r in rows if not r["faster_than_torch"]]
    print("every case faster than the torch composition" if not slow else f"NOT faster than the torch composition: {slow}")


if __name__ == "__main__":
    main()
