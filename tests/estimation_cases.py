"""Shared inputs and library wrappers of the estimation tests (tests/test_estimation_cpu.py, test_gpu_estimation.py, test_gpu_guard_estimation.py).
Nothing here needs a device: the emulations are host code of the library."""
import ctypes as C
import functools

import numpy as np

from dsp_jl_amd import _dev, _lib

import estimation_ref as ref

RUN, TILE = 16, 1024
FS = 100.0
DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
# lengths at which the tiling takes another path
PASS_LENGTHS = (2, 3, RUN - 1, RUN, RUN + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
PASS_TONES = (28.3, 0.37, 49.2)
PASS_CUTS = (1, 3)                 # forced segments
CARRY_CASE = (130, 65)             # n, forced segments: the second group of 64 carries
REDUCE_LENGTHS = (1, 2, 63, 64, 65, 257, TILE + 1, 4 * TILE + 5)
REDUCE_CUTS = (1, 2, 3)

# e_scan <= PASS_C * e_serial: e_scan the largest relative error of an emulated record's sums against the long-double restatement,
# e_serial that of the Float64 serial restatement, taken as the maximum over the table's rows of one frequency.  The worst ratio measured over the table
# (three tones, four types, nine lengths, cuts of 1 and 3, and 130 samples in 65 segments) is 2.35 (tone 0.37, Float32, 2051 samples in 3 segments:
# e_scan 1.35e-13 against e_serial 5.76e-14; the other tones: 1.03 and 1.31); twice that, rounded up to a power of two -- headroom for another seed,
# not for another algorithm.
PASS_C = 8.0
# |estimate - Float64 restatement| in Hz at fs = 100: at most 3.55e-15 (one ulp of 28.3) measured over the reference's calls and both cuts; twice that,
# which is a power of two.  tol = 1e-6 in beta is 8e-6 Hz at 28.3 of 100: far above.
AGREE_TOL = 2.0 ** -47


def tone(n, f, dtype, noise=0.1, seed=1776):
    """A tone at f of FS with noise and a mean to remove."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    if dtype.kind == "c":
        x = np.exp(2j * np.pi * (f * t + 0.13)) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + (0.3 - 0.2j)
    else:
        x = np.cos(2 * np.pi * (f * t + 0.13)) + noise * rng.standard_normal(n) + 0.3
    return x.astype(dtype)


def pass_param(f, dtype):
    """alpha (real) or omega (complex) at the tone's frequency."""
    w = 2 * np.pi * f / FS
    return w if np.dtype(dtype).kind == "c" else 2 * np.cos(w)


def mean_of(x):
    """What the library's loop removes: the Float64 quotient of the (here: long double, correctly rounded) sum."""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        s = x.astype(np.clongdouble).sum()
        return complex(float(s.real) / len(x), float(s.imag) / len(x))
    return float(x.astype(np.longdouble).sum()) / len(x)


def reference_signals():
    """test/estimation.jl:62-65, :73-74."""
    t = np.arange(501) / FS
    sr = np.cos(np.pi * (2 * 28.3 * t + 1 / 4.2))
    sc = np.exp(1j * np.pi * (2 * -40.3 * t + 1 / 1.4))
    return sr, sc


def jacobsen_cases():
    """test/estimation.jl:32-51: (signal, true frequency)."""
    t = np.arange(501) / FS
    out = []
    for fc, ph in ((-40.3, 1 / 1.4), (14.3, 1 / 3), (49.90019, 0), (-49.90019, 0), (0.04, 0), (-0.1, 0)):
        out.append((np.exp(1j * np.pi * (2 * fc * t + ph)), fc))
    out.append((np.cos(np.pi * (2 * 28.3 * t + 1 / 4.2)), 28.3))
    out.append((np.sin(np.pi * (2 * 23.45 * t + 3 / 2.2)), 23.45))
    return out


# ---- the library's host emulations ------------------------------------------------------------------------------------------------------------------
def pass_emulate(x, mean, param, segments):
    """The record of mdsp_quinn_pass_emulate_host as float64: 4 values (real) or 3 (complex)."""
    x = np.ascontiguousarray(x)
    cplx = x.dtype.kind == "c"
    out = np.full(4, np.nan)
    mu = (C.c_double * 2)(float(np.real(mean)), float(np.imag(mean)))
    _lib.check(_lib.lib().mdsp_quinn_pass_emulate_host(x.ctypes.data, _dev.md_dtype(x.dtype), len(x), int(segments), mu, float(param),
                                                       out.ctypes.data_as(C.POINTER(C.c_double))))
    return out[:3] if cplx else out


def est_reduce_emulate(x, op, segments=0, phase=0):
    """mdsp_est_reduce_emulate on a host vector, or on an (outer, len, inner) array reduced along len: float64 sums (SUM) or int64 (index, flag)
    records (ABS2ARGMAX), one row per line."""
    x = np.ascontiguousarray(x)
    if x.ndim == 1:
        inner_, length, outer_ = 1, x.size, 1
    else:
        outer_, length, inner_ = x.shape
    words = 1 if (op == _lib.EST_SUM and x.dtype.kind != "c") else 2
    out = np.zeros((inner_ * outer_, words), dtype=np.int64 if op == _lib.EST_ABS2ARGMAX else np.float64)
    _lib.check(_lib.lib().mdsp_est_reduce_emulate(x.ctypes.data, out.ctypes.data, inner_, length, outer_, op, _dev.md_dtype(x.dtype), int(segments), int(phase), None))
    return out


def peak_emulate(bins, n, onesided, argmax):
    bins = np.ascontiguousarray(bins)
    argmax = np.ascontiguousarray(argmax, dtype=np.int64)
    out = np.zeros(8, dtype=np.int64)
    _lib.check(_lib.lib().mdsp_est_peak_emulate(bins.ctypes.data, len(bins), int(n), int(onesided), _dev.md_dtype(bins.dtype), argmax.ctypes.data, out.ctypes.data))
    return out


def emulated_quinn(x, f0, fs, tol=1e-6, maxiters=20, segments=0):
    """The loop of mdsp_quinn_estimate restated over the emulated passes: (estimate, reached_maxiters, iterations)."""
    x = np.ascontiguousarray(x)
    mean = mean_of(x)
    fn = fs / 2
    w = np.pi * f0 / fn
    it = 0
    if x.dtype.kind != "c":
        alpha, beta = 2 * np.cos(w), 0.0
        for it in range(1, maxiters + 1):
            num, den, xi1, xi2 = pass_emulate(x, mean, alpha, segments)
            beta = (xi2 / xi1 + num) / den
            if abs(alpha - beta) < tol:
                break
            alpha = 2 * beta - alpha
        return float(fn * np.arccos(0.5 * beta) / np.pi), it == maxiters, it
    for it in range(1, maxiters + 1):
        sre, sim, den = pass_emulate(x, mean, w, segments)
        step = 2 * (sim * np.cos(w) - sre * np.sin(w)) / den
        w += step
        if abs(step) < tol:
            break
    return float(fn * w / np.pi), it == maxiters, it


# ---- one pass against the long-double restatement --------------------------------------------------------------------------------------------------
def _sums(rec, cplx):
    """The record's sums as comparable numbers: (num, den) or (S, den)."""
    return (complex(rec[0], rec[1]), rec[2]) if cplx else (rec[0], rec[1])


@functools.lru_cache(maxsize=None)
def pass_references(n, f, dtype_name):
    """(x, mean, param, long-double sums, relative error of the Float64 serial sums) of one row of the table; computed once, shared by the cuts."""
    dtype = np.dtype(dtype_name)
    cplx = dtype.kind == "c"
    x = tone(n, f, dtype)
    mean, param = mean_of(x), pass_param(f, dtype)
    if cplx:
        ld = ref.quinn_pass_complex(x, mean, param, np.longdouble)
        f64 = ref.quinn_pass_complex(x, mean, param, np.float64)
    else:
        ld = ref.quinn_pass_real(x, mean, param, np.longdouble)[:2]
        f64 = ref.quinn_pass_real(x, mean, param, np.float64)[:2]
    return x, mean, param, ld, relative_error(f64, ld)


def relative_error(sums, ld):
    """The largest relative error of the sums against the long-double ones; a sum that is exactly zero there (no terms) must be zero."""
    worst = 0.0
    for got, want in zip(sums, ld):
        if want == 0:
            assert got == 0
            continue
        worst = max(worst, float(abs(type(want)(got) - want) / abs(want)))
    return worst


def pass_error(n, f, dtype, segments):
    """(e_scan, e_serial) of one row and cut."""
    x, mean, param, ld, e_serial = pass_references(n, f, np.dtype(dtype).name)
    rec = pass_emulate(x, mean, param, segments)
    return relative_error(_sums(rec, x.dtype.kind == "c"), ld), e_serial
