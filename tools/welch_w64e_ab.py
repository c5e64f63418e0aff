#!/usr/bin/env python3
"""The counted-wait Welch kernel (variant 45, tools/gen_welch_asm_e.py) against variant 44, the Welch launch alone, in one process.
W64E_AB_VARIANTS (default 44,45) names the MDSP_WELCH_VARIANT values compared; profiles/welch_w64e_ab.json was measured with an experimental build that
also carried the streaming form of the kernel as 46 (plain) / 47 (`nt` sample loads).

    python tools/welch_w64e_ab.py sizes     the LAST TWO variants, alternating, W64E_AB_ROUNDS rounds (6) at 2^26, 2^27 and 2^28 Float32 samples
                                            (W64E_AB_LOG2N, comma separated).  Back-to-back launches on one signal: the next launch is the consumer that
                                            may still find the signal in cache (the protocol of ols_stream_rule's 512 MiB line)
    python tools/welch_w64e_ab.py forms     all variants, alternating, at 2^30 samples (W64E_AB_LOG2N) of random data (the kernel runs at the package
                                            power cap) and of zeros (it does not)

Every figure: ten timed launches after three, one hip event pair per launch; median, min, max in ms.  All variants must give the same bits.  Writes
W64E_AB_OUT/welch_w64e_<mode>.json (W64E_AB_OUT: a directory, default the system's temporary one)."""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import dsp_jl_amd as d
from dsp_jl_amd import _lib

mode = sys.argv[1] if len(sys.argv) > 1 else "sizes"
lib = _lib.lib()
_lib.check(lib.mdsp_init(0))
stream = torch.cuda.current_stream().cuda_stream
WARM, TIMED = 3, 10
events = []
for _ in range(TIMED + 1):
    e = C.c_void_p()
    _lib.check(lib.mdsp_event_create(C.byref(e)))
    events.append(e)


def timed(fn):
    for _ in range(WARM):
        fn()
    _lib.check(lib.mdsp_event_record(events[0], stream))
    for k in range(TIMED):
        fn()
        _lib.check(lib.mdsp_event_record(events[k + 1], stream))
    torch.cuda.synchronize()
    ms = []
    for k in range(TIMED):
        v = C.c_float()
        _lib.check(lib.mdsp_event_elapsed_ms(events[k], events[k + 1], C.byref(v)))
        ms.append(v.value)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def plan(n, variant):
    _lib.set_tunable("MDSP_WELCH_VARIANT", str(variant))
    try:
        return d.WelchConfig(n, np.float32, n=4096, noverlap=2048, window=d.hanning, engine=d.ENGINE_FUSED)
    finally:
        _lib.set_tunable("MDSP_WELCH_VARIANT", None)


def series(x, variants, rounds):
    n = x.numel()
    psd = torch.empty(2049, dtype=torch.float32, device="cuda")
    plans = {v: plan(n, v) for v in variants}
    row = {str(v): [] for v in variants}
    ref, same = None, True
    for r in range(rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            row[str(v)].append(timed(lambda: _lib.check(lib.mdsp_welch_exec(plans[v]._h, x.data_ptr(), n, 1, n, psd.data_ptr(), 2049, stream))))
            if ref is None:
                ref = psd.clone()
            same = same and torch.equal(psd, ref)
    row["bit_identical"] = bool(same)
    for v in variants:
        row[f"{v}_median_of_medians_ms"] = float(np.median([e["median_ms"] for e in row[str(v)]]))
    return row


rounds = int(os.environ.get("W64E_AB_ROUNDS", "6"))
VARIANTS = [int(v) for v in os.environ.get("W64E_AB_VARIANTS", "44,45").split(",")]
res = {"mode": mode, "rounds": rounds, "variants": VARIANTS}
out = os.path.join(os.environ.get("W64E_AB_OUT") or tempfile.gettempdir(), f"welch_w64e_{mode}.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
if mode == "sizes":
    res["sizes"] = {}
    for log2n in [int(v) for v in os.environ.get("W64E_AB_LOG2N", "26,27,28").split(",")]:
        x = torch.randn(1 << log2n, device="cuda")
        a, b = VARIANTS[-2:]
        row = series(x, [a, b], rounds)
        row["rounds_lost_by_the_last_variant"] = sum(1 for p, s in zip(row[str(a)], row[str(b)]) if s["median_ms"] > p["median_ms"])
        res["sizes"][str(log2n)] = row
        print(log2n, {k: v for k, v in row.items() if not isinstance(v, list)}, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del x
        torch.cuda.empty_cache()
elif mode == "forms":
    log2n = int(os.environ.get("W64E_AB_LOG2N", "30"))
    res["log2n"] = log2n
    for name, make in (("random", lambda: torch.randn(1 << log2n, device="cuda")), ("zeros", lambda: torch.zeros(1 << log2n, device="cuda"))):
        x = make()
        res[name] = series(x, VARIANTS, rounds)
        print(name, {k: v for k, v in res[name].items() if not isinstance(v, list)}, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del x
        torch.cuda.empty_cache()
else:
    sys.exit(f"unknown mode {mode!r}")
json.dump(res, open(out, "w"), indent=1)
print("wrote", out)
