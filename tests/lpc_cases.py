"""Shared inputs, case lists and library wrappers of the lpc tests (tests/test_lpc_cpu.py, test_gpu_lpc.py, test_gpu_guard_lpc.py).  Nothing here needs a
device: the emulation is host code of the library."""
import functools

import numpy as np

from dsp_jl_amd import _dev, _lib

import lpc_ref as ref

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
FAMILIES = ("ar3", "tone")
ORDERS = (0, 1, 2, 3, 17)
CUTS = (1, 3)                                   # forced segments
COEFFS = {"f": np.array([1, 0.5, 0.3, 0.2]), "c": np.array([1, 0.5 + 0.2j, 0.3 - 0.5j, 0.2])}      # test/lpc.jl:5

# e_emul <= BURG_C * e_serial.  e: the largest of the relative errors of a, of the reflection coefficients (each max |got - want| over
# max |want|: a coefficient that cancels to nearly zero is measured against the size of its vector) and of prediction_err, against the long-double
# restatement.  e_emul is that of the library's emulation, e_serial that of the working-precision restatement with sequential sums, taken as the maximum
# over all rows of one signal family and type.  The worst ratio measured over the table below (two families, four types, five orders, the lengths of
# lengths_for, cuts of 1 and 3, and the 65-segment row) is 5.37 (the tone family in Float32, 18 samples at p = 17 in one segment: e_emul 0.259 against
# e_serial 0.0482 -- at p = N - 1 the last orders divide by an error energy that has all but vanished, and every implementation loses its digits there;
# the other seven families and types: 0.03 .. 1.49); twice that, rounded up to a power of two -- headroom for another seed, not for another algorithm.
BURG_C = 16.0
# The p = N - 1 rows carry every family's e_serial above (18.7 for the complex AR(3) family in ComplexF32), so that bound says little about the rows where
# the problem is posed well.  A second bound over the LONG rows alone -- N >= tile - 1 -- with e_serial the maximum over the long rows of the family and
# type: e_emul <= BURG_C_LONG * e_serial_long.  The worst ratio measured over the 41 long rows of each family and type is 1.61 (the tone family in
# Float64, 128 samples at p = 17 in one segment: 6.76e-14 against 4.21e-14; the other seven: 0.11 .. 0.94); the same rule: twice that, rounded up.
BURG_C_LONG = 4.0

# test/lpc.jl:3-15 with numpy's generator: a seed at which the Float64 restatement sits below HALF of each of the reference's bounds for both types and
# both methods (1792: |ar - coeffs| <= 0.0039 real, 0.0020 complex, of 0.01; e within 0.0015 of var(s), of 0.01.  1776 leaves the real case at 0.0046)
STAT_SEED = 1792
STAT_N, STAT_SKIP = 50000, 999                  # x[1000:end]


def tile_of(dtype):
    return 64 * (16 // np.dtype(dtype).itemsize)


def signal(family, n, dtype, seed=1776):
    """n samples of a family in dtype: AR(3) noise through COEFFS (its complex twin for a complex type), or a tone in noise."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    cplx = dtype.kind == "c"
    s = (rng.standard_normal(n + 64) + 1j * rng.standard_normal(n + 64)) / np.sqrt(2) if cplx else rng.standard_normal(n + 64)
    if family == "ar3":
        return ref.lfilter_ar(COEFFS["c" if cplx else "f"], s)[64:].astype(dtype)
    t = np.arange(n)
    x = np.exp(2j * np.pi * (0.0731 * t + 0.13)) if cplx else np.cos(2 * np.pi * (0.0731 * t + 0.13))
    return (x + 0.1 * s[:n]).astype(dtype)


def lengths_for(p, dtype):
    """The lengths at which the tiling takes another path, and the shortest ones; only those that admit the order (p <= N - 1)."""
    t = tile_of(dtype)
    return sorted({n for n in (2, 3, p + 1, t - 1, t, t + 1, 2 * t + 3) if n >= max(p + 1, 2)})


def table(dtype):
    """(family, n, p, segments) of every row for one type."""
    rows = []
    for fam in FAMILIES:
        for p in ORDERS:
            for n in lengths_for(p, dtype):
                rows += [(fam, n, p, S) for S in CUTS]
        for n in (2, 3):                                                   # the small lengths also at p = N - 1
            rows += [(fam, n, n - 1, S) for S in CUTS if (fam, n, n - 1, S) not in rows]
        rows.append((fam, 2 * tile_of(dtype) + 3, 3, 65))                  # the fold reaches its second group of 64
    return rows


def geometry(dtype, n, segments=0):
    """(segments, seglen, tile, workspace_bytes)"""
    import dsp_jl_amd as d
    return d.burg_geometry(dtype, n, segments)


def split_record(rec, p):
    """(a, prediction_err, reflection_coeffs) of a record: a (p + 1), the reflection coefficients (p), prediction_err in the real part of the last."""
    rec = np.asarray(rec)
    return rec[:p + 1].copy(), rec[2 * p + 1].real, rec[p + 1:2 * p + 1].copy()


def emulate_record(x, p, segments=0):
    """The record of mdsp_burg_emulate_host: 2 p + 2 elements of x's type."""
    x = np.ascontiguousarray(x)
    rec = np.zeros(2 * p + 2, dtype=x.dtype)
    _lib.check(_lib.lib().mdsp_burg_emulate_host(x.ctypes.data, _dev.md_dtype(x.dtype), len(x), int(segments), int(p), rec.ctypes.data))
    return rec


def emulate(x, p, segments=0):
    """(a, prediction_err, reflection_coeffs) of the emulation."""
    return split_record(emulate_record(x, p, segments), p)


def burg_error(got, want):
    """e of the comment above: got and want are (a, prediction_err, reflection_coeffs)."""
    worst = 0.0
    for g, w in ((got[0], want[0]), (got[2], want[2])):
        if len(w):
            w = np.asarray(w)
            worst = max(worst, float(np.max(np.abs(np.asarray(g).astype(w.dtype) - w)) / np.max(np.abs(w))))
    we = np.longdouble(want[1])
    worst = max(worst, float(abs(np.longdouble(got[1]) - we) / abs(we)))
    return worst


@functools.lru_cache(maxsize=None)
def references(family, n, p, dtype_name):
    """(x, long-double result, e of the working-precision restatement) of one row; computed once, shared by the cuts and the tests."""
    x = signal(family, n, dtype_name)
    x.setflags(write=False)
    ld = ref.arburg_longdouble(x, p)
    return x, ld, burg_error(ref.arburg_pushpop(x, p), ld)


@functools.lru_cache(maxsize=None)
def serial_error_of_family(family, dtype_name):
    """e_serial: the maximum over all rows of the family and type."""
    return max(references(fam, n, p, dtype_name)[2] for fam, n, p, S in table(dtype_name) if fam == family)


def is_long(n, dtype):
    return n >= tile_of(dtype) - 1


@functools.lru_cache(maxsize=None)
def serial_error_of_long_rows(family, dtype_name):
    """e_serial_long: the maximum over the long rows of the family and type."""
    return max(references(fam, n, p, dtype_name)[2] for fam, n, p, S in table(dtype_name) if fam == family and is_long(n, dtype_name))


def stat_case(cplx, seed=None):
    """test/lpc.jl:5-10: (x[1000:end], coeffs, var(s)) in Float64 / ComplexF64."""
    rng = np.random.default_rng(STAT_SEED if seed is None else seed)
    s = (rng.standard_normal(STAT_N) + 1j * rng.standard_normal(STAT_N)) / np.sqrt(2) if cplx else rng.standard_normal(STAT_N)
    coeffs = COEFFS["c" if cplx else "f"]
    return ref.lfilter_ar(coeffs, s)[STAT_SKIP:], coeffs, float(np.var(s))


@functools.lru_cache(maxsize=None)
def stat_cached(cplx):
    x, coeffs, var = stat_case(cplx)
    x.setflags(write=False)
    return x, coeffs, var
