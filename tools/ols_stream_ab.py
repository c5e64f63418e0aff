#!/usr/bin/env python3
"""Cache policy of the tiled overlap-save kernel (MDSP_OLS_STREAM, and MDSP_OLS_AUX of -DMDSP_DEBUG_KNOBS builds), measured in one process.

    python tools/ols_stream_ab.py sizes      plain (MDSP_OLS_STREAM=0) against streaming (=2), alternating, OLS_AB_ROUNDS rounds (6) at 2^24, 2^25, 2^26,
                                             2^28 and 2^30 Float32 samples (OLS_AB_LOG2N, comma separated): where the footprint threshold belongs
    python tools/ols_stream_ab.py matrix     MDSP_LIB_TAG=dbg: every combination loads {0, 2, 3} x stores {0, 2, 17, 18} at 2^30 samples, transforms skipped
                                             (MDSP_ABLATE=2: the memory side alone) and whole, beside the three float4 copy yardsticks of bench.py

Every figure: ten timed launches after three, one hip event pair per launch; median, min, max in ms.  Writes OLS_AB_OUT/ols_stream_<mode>.json (OLS_AB_OUT: a directory, default the system's temporary one)."""
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
from dsp_jl_amd.dspbase import OlsPlan

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


taps = (np.hanning(256) / 128).astype(np.float32)
res = {"mode": mode, "library": os.environ.get("MDSP_LIB_TAG", ""), "debug_knobs": int(lib.mdsp_debug_knobs())}
out = os.path.join(os.environ.get("OLS_AB_OUT") or tempfile.gettempdir(), f"ols_stream_{mode}.json")
os.makedirs(os.path.dirname(out), exist_ok=True)

if mode == "sizes":
    rounds = int(os.environ.get("OLS_AB_ROUNDS", "6"))
    res["sizes"] = {}
    for log2n in [int(v) for v in os.environ.get("OLS_AB_LOG2N", "24,25,26,28,30").split(",")]:
        n = 1 << log2n
        x = torch.randn(n, device="cuda")
        y = torch.empty_like(x)
        plan = OlsPlan(taps, 2048, n, 0, d.ENGINE_FUSED)
        run = lambda: _lib.check(lib.mdsp_ols_exec(plan._h, x.data_ptr(), n, 1, n, y.data_ptr(), n, n, stream))
        row = {"plain": [], "streaming": []}
        ref = None
        for r in range(rounds):
            for name, knob in (("plain", 0), ("streaming", 2)):
                _lib.set_tunable("MDSP_OLS_STREAM", knob)
                row[name].append(timed(run))
                if ref is None:
                    ref = y.clone()
                row.setdefault("bit_identical", True)
                row["bit_identical"] = bool(row["bit_identical"] and torch.equal(y, ref))
        _lib.set_tunable("MDSP_OLS_STREAM", None)
        row["streaming_not_slower_in_any_round"] = all(s["median_ms"] <= p["median_ms"] for p, s in zip(row["plain"], row["streaming"]))
        for name in ("plain", "streaming"):
            row[name + "_median_of_medians_ms"] = float(np.median([e["median_ms"] for e in row[name]]))
        res["sizes"][str(log2n)] = row
        print(log2n, {k: v for k, v in row.items() if not isinstance(v, list)}, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del x, y, ref, plan
        torch.cuda.empty_cache()
elif mode == "matrix":
    if not lib.mdsp_debug_knobs():
        sys.exit("the matrix needs a -DMDSP_DEBUG_KNOBS build (MDSP_LIB_TAG)")
    log2n = int(os.environ.get("OLS_AB_LOG2N", "30"))
    n = 1 << log2n
    x = torch.randn(n, device="cuda")
    y = torch.empty_like(x)
    plan = OlsPlan(taps, 2048, n, 0, d.ENGINE_FUSED)
    run = lambda: _lib.check(lib.mdsp_ols_exec(plan._h, x.data_ptr(), n, 1, n, y.data_ptr(), n, n, stream))
    res["log2n"] = log2n
    res["matrix"] = {}
    for ablate in (2, 0):
        _lib.set_tunable("MDSP_ABLATE", ablate)
        for loads in (0, 2, 3):
            for stores in (0, 2, 17, 18):
                _lib.set_tunable("MDSP_OLS_AUX", 100 * loads + stores)
                e = timed(run)
                e["GBps_of_8_bytes_per_sample"] = round(8.0 * n / e["median_ms"] / 1e6, 1)
                res["matrix"].setdefault(f"ablate_{ablate}", {})[f"loads_{loads}_stores_{stores}"] = e
                print("ablate", ablate, "loads", loads, "stores", stores, e, flush=True)
                json.dump(res, open(out, "w"), indent=1)
    _lib.set_tunable("MDSP_ABLATE", None)
    _lib.set_tunable("MDSP_OLS_AUX", None)
    nb = n * 4
    res["copies"] = {}
    for name, fn in (("copy_GBps", lambda: _lib.check(lib.mdsp_copy_bench(y.data_ptr(), x.data_ptr(), nb, stream))),
                     ("copy_nt_4wg_GBps", lambda: _lib.check(lib.mdsp_copy_bench_mode(y.data_ptr(), x.data_ptr(), nb, 2, 4, stream))),
                     ("copy_ntload_sc_store_GBps", lambda: _lib.check(lib.mdsp_copy_bench_mode(y.data_ptr(), x.data_ptr(), nb, 6, 2, stream)))):
        e = timed(fn)
        res["copies"][name] = round(2.0 * nb / e["median_ms"] / 1e6, 1)
        print(name, res["copies"][name], e, flush=True)
else:
    sys.exit(f"unknown mode {mode!r}")
json.dump(res, open(out, "w"), indent=1)
print("wrote", out)
