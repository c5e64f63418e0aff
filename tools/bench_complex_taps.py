#!/usr/bin/env python3
"""Complex FIR taps, one pass against the composition of two real-tap passes (profiles/complex_taps.json).

    python tools/bench_complex_taps.py [--compose] [--runs 11] [--log2n 26] [--nch 4] [--out FILE]

Signal: 4 channels x 2^26 samples, device resident; filters pre-built; median of --runs timed runs after a warm-up run, with the spread (min, max).
Shapes: the decimating channelizer 1//8 (8 x 37 taps: a windowed-sinc low-pass shifted to a channel centre), 160//147, 441//160 and 3//8 with
resample_filter-length banks shifted the same way, for ComplexF32 and ComplexF64 signals with taps of the signal's precision; and a real Float32
signal under ComplexF32 taps at 1//8 and 160//147.

Default mode: FIRFilter with the complex taps, one mdsp_fir_exec.  --compose: what gives the same result without complex taps -- FIRFilter(real(h)) and
FIRFilter(imag(h)) over x, then yr + im yi with torch -- and needs nothing but real-tap filters, so it also runs on a checkout that predates complex
taps.  Algorithmic bytes per input sample: sizeof(x) + sizeof(y) L / M.  Writes --out (default complex_taps_one_pass_results.json or
complex_taps_compose_results.json in the working directory): per shape the times, GB/s, the fraction of 8 TB/s and the kernel path(s) taken."""
import argparse
import ctypes as C
import json
import os
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import dsp_jl_amd as d
from dsp_jl_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--compose", action="store_true")
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--nch", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.runs < 10:
    ap.error("--runs must be at least 10")

lib = _lib.lib()
_lib.check(lib.mdsp_init(0))
nch, n = args.nch, 1 << args.log2n
stream = torch.cuda.current_stream().cuda_stream
gen = torch.Generator(device="cuda"); gen.manual_seed(1776)
# signal dtype -> (torch dtype, real numpy type of that precision, complex numpy type, bytes per sample, library dtype)
TYPES = {"f32": (torch.float32, np.float32, np.complex64, 4, _lib.F32), "c32": (torch.complex64, np.float32, np.complex64, 8, _lib.C32),
         "c64": (torch.complex128, np.float64, np.complex128, 16, _lib.C64)}
MD = {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64, np.dtype(np.complex64): _lib.C32, np.dtype(np.complex128): _lib.C64}
SHAPES = [("c32", 1, 8), ("c32", 160, 147), ("c32", 441, 160), ("c32", 3, 8), ("c64", 1, 8), ("c64", 160, 147), ("c64", 441, 160), ("c64", 3, 8),
          ("f32", 1, 8), ("f32", 160, 147)]


def taps(L, M):
    """A real low-pass prototype (1//8: 8 x 37 taps of a Hamming-windowed sinc; otherwise DSP.jl's default resampling filter), shifted to a channel centre."""
    if (L, M) == (1, 8):
        k = np.arange(8 * 37) - (8 * 37 - 1) / 2
        h = np.sinc(k / 8) / 8 * np.hamming(8 * 37)
    else:
        h = np.asarray(d.resample_filter(Fraction(L, M)), dtype=np.float64)
    return h * np.exp(2j * np.pi * 0.1 * np.arange(len(h)) / L)


def ev():
    e = C.c_void_p(); _lib.check(lib.mdsp_event_create(C.byref(e))); return e


e0, e1 = ev(), ev()


def create(h, L, M, lx):
    fh = C.c_void_p()
    h = np.ascontiguousarray(h)
    _lib.check(lib.mdsp_fir_create(C.byref(fh), h.ctypes.data_as(C.c_void_p), len(h), L, M, MD[h.dtype], lx, nch))
    return fh


out = {"note": f"tools/bench_complex_taps.py{' --compose' if args.compose else ''}: {nch} channels x 2^{args.log2n} samples, median of {args.runs} after warm-up",
       "mode": "compose" if args.compose else "one_pass", "cells": {}}
x, xkey = None, None
for dt, L, M in SHAPES:
    tdt, rnp, cnp, esz, lx = TYPES[dt]
    ctd = torch.complex128 if dt == "c64" else torch.complex64
    osz = 16 if dt == "c64" else 8
    if xkey != dt:
        del x
        x = torch.randn((nch, n), generator=gen, device="cuda", dtype=tdt)
        xkey = dt
    h = taps(L, M)
    if args.compose:
        filters = [create(h.real.astype(rnp), L, M, lx), create(h.imag.astype(rnp), L, M, lx)]
    else:
        filters = [create(h.astype(cnp), L, M, lx)]
    ol = C.c_int64(); _lib.check(lib.mdsp_fir_outputlength(filters[0], n, C.byref(ol)))
    ys = [torch.empty((nch, ol.value), dtype=(tdt if args.compose else ctd), device="cuda") for _ in filters]
    y = torch.empty((nch, ol.value), dtype=ctd, device="cuda") if args.compose else ys[0]
    nw = C.c_int64()

    def run():
        for fh, yy in zip(filters, ys):
            _lib.check(lib.mdsp_fir_reset(fh))
            _lib.check(lib.mdsp_fir_exec(fh, x.data_ptr(), n, n, yy.data_ptr(), ol.value, ol.value, C.byref(nw), stream))
        if args.compose:                                      # yr + im yi in one pass
            if ys[0].is_complex():
                torch.add(ys[0], ys[1], alpha=1j, out=y)
            else:
                torch.complex(ys[0], ys[1], out=y)

    run(); torch.cuda.synchronize()                           # warm-up
    paths = []
    for fh in filters:
        p = C.c_int(-1); _lib.check(lib.mdsp_fir_kernel_path(fh, n, C.byref(p))); paths.append(p.value)
    ms = []
    for _ in range(args.runs):
        _lib.check(lib.mdsp_event_record(e0, stream)); run(); _lib.check(lib.mdsp_event_record(e1, stream))
        torch.cuda.synchronize()
        t = C.c_float(); _lib.check(lib.mdsp_event_elapsed_ms(e0, e1, C.byref(t)))
        ms.append(round(t.value, 4))
    bytes_alg = (esz + osz * L / M) * n * nch
    med = float(np.median(ms))
    key = f"{dt}_{L}_{M}"
    out["cells"][key] = {"taps": len(h), "signal": dt, "ratio": f"{L}//{M}", "ms": ms, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms),
                         "GBps": round(bytes_alg / med / 1e6, 1), "frac_of_8TBps": round(bytes_alg / med / 1e6 / 8000, 3), "kernel_path": paths,
                         "checksum": float(y.abs().sum(dtype=torch.float64))}
    print(key, out["cells"][key]["median_ms"], (min(ms), max(ms)), out["cells"][key]["frac_of_8TBps"], paths, flush=True)
    for fh in filters:
        _lib.check(lib.mdsp_fir_destroy(fh))
    del ys, y
name = args.out or ("complex_taps_compose_results.json" if args.compose else "complex_taps_one_pass_results.json")
if os.path.dirname(name):
    os.makedirs(os.path.dirname(name), exist_ok=True)
json.dump(out, open(name, "w"), indent=1)
