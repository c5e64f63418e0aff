"""Shared inputs, case lists and library wrappers of the esprit tests (tests/test_esprit_cpu.py, test_gpu_esprit.py, test_gpu_guard_esprit.py).  Nothing
here needs a device: the emulation is host code of the library."""
import functools

import numpy as np

from dsp_jl_amd import _dev, _lib

import esprit_ref as ref

DTYPES = (np.float32, np.float64, np.complex64, np.complex128)
CUTS = (1, 3, 0)                                # forced segments; 0: the automatic cut

# e_emul <= GRAM_C * max(e_serial, eps): e = max |R - R_ld| / max |R_ld| against the long-double Gram matrix, e_emul that of the library's
# emulation, e_serial that of the serial Float64 loop in index order, eps = 2^-52.  The worst ratio measured over grid() below (four types, six M, five
# n, three cuts: 360 rows) is 1.49 (ComplexF64, n = 17, M = 9, one segment: 3.31e-16 against 2.06e-16, a window of nine products where either order is
# within two units of roundoff; the other types: 1.00, 0.83, 0.99, all at n = 2 M - 1 or 2 M with M = 19); twice that, rounded up to a power of two.
GRAM_C = 4.0

# |f_gram - f_svd| / Fs over route_cases(), frequencies sorted: the finish on the emulated Gram matrix against the SVD restatement.  Measured: the
# reference's test case 9.1e-17, the docstring case 7.1e-18, two real tones and one cisoid 0, four cisoids (sigma_p / sigma_1 = 0.01) 2.11e-15; twice
# the worst, rounded up to a power of two.
ROUTE_BOUND = 2.0 ** -47
ROUTE_MIN_SV_RATIO = 1e-3                       # every route case has sigma_p / sigma_1 of its Hankel matrix at least this


@functools.lru_cache(maxsize=None)
def tile_and_group():
    """(T, G) of the library: the samples a workgroup stages at a time and the lags a lane accumulates at a time."""
    import dsp_jl_amd as d
    _, _, tile, group, _ = d.hankel_gram_geometry(np.float32, 1, 1)
    return tile, group


def m_values():
    _, G = tile_and_group()
    return (1, 2, 5, G, G + 1, 2 * G + 3)


def n_values(M):
    T, _ = tile_and_group()
    return (2 * M - 1, 2 * M, M - 1 + T, M + T, 3 * T + 5 + 2 * M)


def grid(dtype):
    """(n, M, segments) of every row for one type."""
    return [(n, M, S) for M in m_values() for n in n_values(M) for S in CUTS]


def signal(n, dtype, seed=1776):
    """n samples in dtype: two tones (cisoids for a complex type) of amplitudes 1 and 0.4 in noise of 0.05."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed + n)
    t = np.arange(n)
    if dtype.kind == "c":
        x = np.exp(2j * np.pi * (0.0731 * t + 0.13)) + 0.4 * np.exp(2j * np.pi * (0.2917 * t - 0.4))
        x = x + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    else:
        x = np.cos(2 * np.pi * (0.0731 * t + 0.13)) + 0.4 * np.cos(2 * np.pi * (0.2917 * t - 0.4)) + 0.05 * rng.standard_normal(n)
    return x.astype(dtype)


def out_dtype(dtype):
    return np.dtype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)


def emulate(x, M, segments=0, ldr=None):
    """R of mdsp_hankel_gram_emulate_host as an (M, M) array (ldr given: the whole (M, ldr) buffer, rows = the library's columns, NaN where untouched)."""
    x = np.ascontiguousarray(x)
    ld = M if ldr is None else ldr
    buf = np.full((M, ld), np.nan, dtype=out_dtype(x.dtype))
    _lib.check(_lib.lib().mdsp_hankel_gram_emulate_host(x.ctypes.data, _dev.md_dtype(x.dtype), len(x), int(M), int(segments), buf.ctypes.data, int(ld)))
    return buf.T.copy() if ldr is None else buf


@functools.lru_cache(maxsize=None)
def references(n, M, dtype_name):
    """(x, long-double Gram matrix, e_serial) of one (n, M, type); computed once, shared by the cuts and the tests."""
    x = signal(n, dtype_name)
    x.setflags(write=False)
    ld = ref.gram_longdouble(x, M)
    return x, ld, ref.gram_error(ref.gram_serial(x, M), ld)


# ---- the route cases: (name, x, M, p, Fs, true frequencies or None)
ROUTE_SEED = 1986


def _cnoise(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def reference_case():
    """test/estimation.jl:5-19 with numpy's generator (the phases sit in the exponent beside the imaginary argument, as written there)."""
    rng = np.random.default_rng(ROUTE_SEED)
    Fs, n = 10000.0, 10000
    t = np.arange(1, n + 1) / Fs
    x = 2.0 * np.exp(2j * np.pi * t * 1000.0 + 0.7) + 1.5 * np.exp(2j * np.pi * t * 1250.0 - 1.0)
    return "reference", x + 0.1 * _cnoise(rng, n), 300, 2, Fs, (1000.0, 1250.0)


def docstring_case():
    """estimation.jl:46-60."""
    rng = np.random.default_rng(ROUTE_SEED + 1)
    Fs = 8000
    t = np.arange(1, Fs + 1) / Fs
    x = 2 * np.exp(2j * np.pi * 2500 * t) + 5 * np.exp(2j * np.pi * 400 * t)
    return "docstring", x + _cnoise(rng, Fs), 5, 2, float(Fs), None


def two_tone_case():
    rng = np.random.default_rng(ROUTE_SEED + 2)
    n, Fs = 2000, 1000.0
    t = np.arange(n) / Fs
    x = np.cos(2 * np.pi * 123.4 * t + 0.3) + 0.5 * np.cos(2 * np.pi * 217.0 * t - 1.1) + 0.01 * rng.standard_normal(n)
    return "two real tones", x, 40, 4, Fs, None


def one_cisoid_case():
    """M = (N + 1) / 3, the choice the reference's docstring names for one cisoid."""
    rng = np.random.default_rng(ROUTE_SEED + 3)
    n = 599
    x = np.exp(2j * np.pi * (0.1234 * np.arange(n) + 0.2)) + 0.05 * _cnoise(rng, n)
    return "one cisoid", x, (n + 1) // 3, 1, 1.0, None


def four_cisoid_case():
    rng = np.random.default_rng(ROUTE_SEED + 4)
    n = 4000
    t = np.arange(n)
    x = sum(a * np.exp(2j * np.pi * (f * t + ph)) for a, f, ph in ((1.0, 0.05, 0.1), (0.3, 0.11, 0.7), (0.1, -0.2, -0.3), (1e-2, 0.31, 0.5)))
    return "four cisoids", x + 1e-3 * _cnoise(rng, n), 64, 4, 1.0, None


@functools.lru_cache(maxsize=None)
def route_cases():
    """Each case with its SVD restatement: (name, x, M, p, Fs, truth, sorted f_svd, sigma_p / sigma_1); computed once."""
    rows = []
    for name, x, M, p, Fs, truth in (reference_case(), docstring_case(), two_tone_case(), one_cisoid_case(), four_cisoid_case()):
        x.setflags(write=False)
        f, sv = ref.esprit_svd(x, M, p, Fs)
        rows.append((name, x, M, p, Fs, truth, np.sort(f), float(sv[p - 1] / sv[0])))
    return tuple(rows)
