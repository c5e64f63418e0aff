"""Case lists and inputs of tests/test_gpu_ct_schedules.py: every compile-time spectral schedule a default call can reach.  Pure Python: no GPU, no library.

The lists are derived from spectral_route_cases.expected_default() at engine AUTO (key (kind, dtype, 0)) -- the route table test_spectral_route_cpu.py
holds the library to -- so the sweep follows that table.  Per kind (0 Welch sums, 1 STFT columns) and dtype (MDSP_F32 .. MDSP_C64), four families:

    welch_direct     kind 0: every size on MDSP_ROUTE_CTBIG (4), one workgroup per frame pair
    cols_direct      kind 1: every size on MDSP_ROUTE_CTBIG_COLS (5)
    fused_rows       kind 0, per route 6 / 7 / 8 (nfft = r0 x row, fused column step): for every distinct row S = nfft / r0 the smallest nfft with that
                     row, and for every distinct r0 the smallest nfft with that r0
    two_kernel_rows  kind 0, route 9 (nfft = r0 x S in two kernels): for every distinct r0 the smallest nfft with that r0

Kernels reachable only under an MDSP_GX setting are not in here.  tests/test_ct_schedule_cases_cpu.py holds the lists to the X-macro tables of
dsp.jl_amd/csrc/ctbig_sizes.h and to the counts below, so the sweep cannot shrink unnoticed.

Inputs: signal() carries the amplitude ramp of tests/test_gpu_run_schedules.py (a frame built from another frame's samples is wrong in level as well as
phase) and a tone that is no bin centre of any size; window() is a VECTOR and asymmetric (a kernel that reads the window mirrored, or from the wrong
frame half, passes every symmetric window).  Each case runs in the two configurations of configs().
"""
import functools
from collections import namedtuple

import numpy as np

import spectral_route_cases as routes

F32, F64, C32, C64 = 0, 1, 2, 3          # MDSP_F32 .. MDSP_C64
DTYPES = (F32, F64, C32, C64)
NP_DTYPES = {F32: np.dtype(np.float32), F64: np.dtype(np.float64), C32: np.dtype(np.complex64), C64: np.dtype(np.complex128)}
AUTO, FUSED = 0, 1                        # MDSP_ENGINE_AUTO, MDSP_ENGINE_FUSED
WELCH, STFT = 0, 1                        # kind

ROUTE_CTBIG, ROUTE_CTBIG_COLS = 4, 5
FUSED_ROW_ROUTES = (6, 7, 8)              # MDSP_ROUTE_CTCOLS_BIG, _CTCOLS_F64, _CTCOLS
ROUTE_CTROWS = 9

FAMILIES = ("welch_direct", "cols_direct", "fused_rows", "two_kernel_rows")

Case = namedtuple("Case", "kind dtype nfft route r0")

# what the committed tables give (F32, F64, C32, C64): the CPU test asserts these
WELCH_COUNTS = {F32: 275, F64: 196, C32: 275, C64: 196}
COLS_COUNTS = {F32: 170, F64: 113, C32: 170, C64: 113}
WELCH_LARGEST = {F32: 497664, F64: 276480, C32: 497664, C64: 276480}
TOTAL_CASES = 1508


@functools.lru_cache(maxsize=None)
def _table(kind, dtype):
    """((nfft, route, r0), ...) over spectral_route_cases.SIZES at engine AUTO; sizes where plan creation fails are left out"""
    rs, zs = routes.expected_default()[(kind, dtype, AUTO)]
    return tuple((n, int(r, 36), int(z, 36)) for n, r, z in zip(routes.SIZES, rs, zs) if r != "-")


def on_route(kind, dtype, route):
    """every Case of the route table on `route`, by size"""
    return [Case(kind, dtype, n, r, z) for n, r, z in _table(kind, dtype) if r == route]


def direct(kind, dtype):
    return on_route(kind, dtype, ROUTE_CTBIG if kind == WELCH else ROUTE_CTBIG_COLS)


def _smallest_per(cases, key):
    first = {}
    for c in cases:                        # by size: the first one seen is the smallest
        first.setdefault(key(c), c)
    return set(first.values())


def rows(dtype, route):
    """route 6 / 7 / 8: the smallest nfft of every distinct row size, and of every distinct r0"""
    cs = on_route(WELCH, dtype, route)
    assert all(c.r0 > 1 and c.nfft % c.r0 == 0 for c in cs)
    return sorted(_smallest_per(cs, lambda c: c.nfft // c.r0) | _smallest_per(cs, lambda c: c.r0), key=lambda c: c.nfft)


def fused_rows(dtype):
    return [c for route in FUSED_ROW_ROUTES for c in rows(dtype, route)]


def two_kernel_rows(dtype):
    cs = on_route(WELCH, dtype, ROUTE_CTROWS)
    assert all(c.r0 > 1 and c.nfft % c.r0 == 0 for c in cs)
    return sorted(_smallest_per(cs, lambda c: c.r0), key=lambda c: c.nfft)


def family_cases(family, dtype):
    if family == "welch_direct":
        return direct(WELCH, dtype)
    if family == "cols_direct":
        return direct(STFT, dtype)
    if family == "fused_rows":
        return fused_rows(dtype)
    if family == "two_kernel_rows":
        return two_kernel_rows(dtype)
    raise ValueError(family)


def welch_cases(dtype):
    return direct(WELCH, dtype) + fused_rows(dtype) + two_kernel_rows(dtype)


def all_cases():
    return [c for dtype in DTYPES for family in FAMILIES for c in family_cases(family, dtype)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
TONE = 0.775     # radians per sample: 0.775 / 2 pi cycles per sample is irrational, no bin centre of any nfft

Config = namedtuple("Config", "name n noverlap window frames channels length")


def signal(seed, length, dtype):
    """(length,) host array of `dtype` (Float32-rounded for the Float32 types): seeded noise plus a tone, under the ramp 1 + 0.5 k / length.  Complex
    types get an independent imaginary part.  `seed` is an int or a sequence of ints (a channel is (seed, channel))."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    k = np.arange(length)
    s = rng.standard_normal(length) + 0.5 * np.sin(TONE * k)
    if dtype.kind == "c":
        s = s + 1j * (rng.standard_normal(length) + 0.5 * np.cos(TONE * k + 0.3))
    return (s * (1.0 + 0.5 * k / length)).astype(dtype)


def window(n):
    """Float64 vector: Hann times the ramp 0.75 + 0.5 k / n, deliberately asymmetric"""
    k = np.arange(n)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * k / (n - 1))) * (0.75 + 0.5 * k / n)


def configs(nfft):
    """A: whole frames at 50 % overlap under the window vector, 3 frames (real signals: one full frame pair and one lone frame; an odd frame count).
    B: n = nfft - 7 with a zero tail, a hop that is no multiple of anything convenient, no window, 4 frames, 2 channels.
    The signal is 5 samples longer than the frames need: a ragged tail that must be ignored."""
    out = []
    for name, n, noverlap, win, frames, channels in (("A", nfft, nfft // 2, True, 3, 1), ("B", nfft - 7, (nfft - 7) // 3, False, 4, 2)):
        out.append(Config(name, n, noverlap, window(n) if win else None, frames, channels, (frames - 1) * (n - noverlap) + n + 5))
    return out


def case_signal(case, cfg):
    """(length,) for one channel, (length, channels) otherwise; seeded by the case and the configuration"""
    cols = [signal((case.kind, case.dtype, case.nfft, ord(cfg.name), c), cfg.length, NP_DTYPES[case.dtype]) for c in range(cfg.channels)]
    return cols[0] if cfg.channels == 1 else np.stack(cols, axis=1)
