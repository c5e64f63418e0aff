#!/usr/bin/env python3
"""Run schedule of the streaming tiled overlap-save kernel (DESIGN.md 4.2 *Run schedule*; knob MDSP_OLS_RUN_LEN), measured in one process.

    python tools/ols_runs_ab.py sweep      MDSP_LIB_TAG=dbg: forced run lengths OLS_AB_LENGTHS (1,2,4,8,16,32,73 and 0 = whole, one run per slot) at 2^OLS_AB_LOG2N
                                           (30) Float32 samples, 256 taps, whole and with the transforms skipped (MDSP_ABLATE=2: the memory side alone);
                                           OLS_AB_ROUNDS rounds (6), the order of the lengths reversed from round to round, whole in every round
    python tools/ols_runs_ab.py sizes      the run rule's own choice (knob unset) against whole at OLS_AB_LOG2N (27,28,30) samples, alternating: where the rule
                                           may switch.  Any build.  OLS_AB_RULE_LEN=n: a candidate length in place of the rule's.  OLS_AB_WARM_ROUNDS (2)
                                           rounds of both schedules run first on every size's fresh buffers and are not counted.

Every figure: ten timed launches after three, one hip event pair per launch; median, min, max in ms.  Outputs are compared bit for bit with whole's.
Writes OLS_AB_OUT/ols_runs_<mode>.json (OLS_AB_OUT: a directory, default the system's temporary one)."""
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

mode = sys.argv[1] if len(sys.argv) > 1 else "sweep"
lib = _lib.lib()
_lib.check(lib.mdsp_init(0))
stream = torch.cuda.current_stream().cuda_stream
WARM, TIMED = 3, 10
WHOLE = 1 << 20          # MDSP_OLS_RUN_LEN is clamped to one run per slot
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


def schedule(n):
    """The schedule of the whole-column streaming launch of n samples on four workgroups per CU, under the knobs as they stand."""
    units = (-(-n // 1792) + 1) // 2          # pairs of tiles of 1792 outputs
    slots = min(units, 4 * torch.cuda.get_device_properties(0).multi_processor_count)
    rl, ni = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.mdsp_ols_run_for(units, slots, 1, C.byref(rl), C.byref(ni)))
    return {"units": units, "slots": slots, "run_len": rl.value, "niter": ni.value}


taps = (np.hanning(256) / 128).astype(np.float32)
rounds = int(os.environ.get("OLS_AB_ROUNDS", "6"))
res = {"mode": mode, "library": os.environ.get("MDSP_LIB_TAG", ""), "debug_knobs": int(lib.mdsp_debug_knobs()), "rounds": rounds}
out = os.path.join(os.environ.get("OLS_AB_OUT") or tempfile.gettempdir(), f"ols_runs_{mode}.json")
os.makedirs(os.path.dirname(out), exist_ok=True)


def problem(log2n):
    n = 1 << log2n
    x = torch.randn(n, device="cuda")
    y = torch.empty_like(x)
    plan = OlsPlan(taps, 2048, n, 0, d.ENGINE_FUSED)
    s = C.c_int(0)
    _lib.check(lib.mdsp_ols_stream_for(n, n, 1, _lib.F32, C.byref(s)))
    assert s.value == 1, "not a streaming launch"
    return n, x, y, plan, (lambda: _lib.check(lib.mdsp_ols_exec(plan._h, x.data_ptr(), n, 1, n, y.data_ptr(), n, n, stream)))


if mode == "sweep":
    if not lib.mdsp_debug_knobs():
        sys.exit("the sweep needs a -DMDSP_DEBUG_KNOBS build (MDSP_LIB_TAG)")
    lengths = [int(v) for v in os.environ.get("OLS_AB_LENGTHS", "1,2,4,8,16,32,73,0").split(",")]
    log2n = int(os.environ.get("OLS_AB_LOG2N", "30"))
    n, x, y, plan, run = problem(log2n)
    res["log2n"] = log2n
    res["bytes_per_launch"] = 8 * n
    _lib.set_tunable("MDSP_OLS_RUN_LEN", WHOLE)
    run()
    ref = y.clone()
    for ablate, key in ((2, "memory_side"), (0, "kernel")):
        _lib.set_tunable("MDSP_ABLATE", ablate)
        tab = {("whole" if L == 0 else str(L)): {"rounds": []} for L in lengths}
        for r in range(rounds):
            for L in (lengths if r % 2 == 0 else lengths[::-1]):
                name = "whole" if L == 0 else str(L)
                _lib.set_tunable("MDSP_OLS_RUN_LEN", WHOLE if L == 0 else L)
                tab[name].setdefault("schedule", schedule(n))
                tab[name]["rounds"].append(timed(run))
                if ablate == 0:
                    tab[name]["bit_identical"] = bool(tab[name].get("bit_identical", True) and torch.equal(y, ref))
        for name, row in tab.items():
            med = [e["median_ms"] for e in row["rounds"]]
            row["median_of_medians_ms"] = round(float(np.median(med)), 4)
            row["TBps_of_8_bytes_per_sample"] = round(8.0 * n / row["median_of_medians_ms"] / 1e9, 3)
            row["beats_whole_in_every_round"] = name != "whole" and all(a < b["median_ms"] for a, b in zip(med, tab["whole"]["rounds"]))
            print(key, name, {k: v for k, v in row.items() if k != "rounds"}, med, flush=True)
        res[key] = tab
        json.dump(res, open(out, "w"), indent=1)
    _lib.set_tunable("MDSP_ABLATE", None)
    _lib.set_tunable("MDSP_OLS_RUN_LEN", None)
elif mode == "sizes":
    RULE = int(os.environ["OLS_AB_RULE_LEN"]) if os.environ.get("OLS_AB_RULE_LEN") else None   # a candidate length in place of the rule's own
    WARM_ROUNDS = int(os.environ.get("OLS_AB_WARM_ROUNDS", "2"))
    res["sizes"] = {}
    for log2n in [int(v) for v in os.environ.get("OLS_AB_LOG2N", "27,28,30").split(",")]:
        n, x, y, plan, run = problem(log2n)
        row = {"whole": [], "rule": [], "warmup_rounds_discarded": WARM_ROUNDS}
        ref = None
        for _ in range(WARM_ROUNDS):                 # fresh buffers, a fresh process: the first launches of either schedule run slow
            for knob in (WHOLE, RULE):
                _lib.set_tunable("MDSP_OLS_RUN_LEN", knob)
                timed(run)
        for r in range(rounds):
            for name, knob in ((("whole", WHOLE), ("rule", RULE)) if r % 2 == 0 else (("rule", RULE), ("whole", WHOLE))):
                _lib.set_tunable("MDSP_OLS_RUN_LEN", knob)
                row.setdefault(name + "_schedule", schedule(n))
                row[name].append(timed(run))
                if ref is None:
                    ref = y.clone()
                row["bit_identical"] = bool(row.get("bit_identical", True) and torch.equal(y, ref))
        _lib.set_tunable("MDSP_OLS_RUN_LEN", None)
        row["rule_loses_no_round"] = all(s["median_ms"] <= p["median_ms"] for p, s in zip(row["whole"], row["rule"]))
        for name in ("whole", "rule"):
            row[name + "_median_of_medians_ms"] = float(np.median([e["median_ms"] for e in row[name]]))
        res["sizes"][str(log2n)] = row
        print(log2n, {k: v for k, v in row.items() if not isinstance(v, list)}, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        del x, y, ref, plan, run
        torch.cuda.empty_cache()
else:
    sys.exit(f"unknown mode {mode!r}")
json.dump(res, open(out, "w"), indent=1)
print("wrote", out)
