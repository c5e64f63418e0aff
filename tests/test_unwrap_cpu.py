"""unwrap along one dimension without a device: the numpy restatement against the reference's own test literals (test/unwrap.jl:6-58), the scan form
against the serial recurrence, the plan geometry, the host emulation of the device code (same geometry, same operator and per-segment walk:
csrc/unwrap_scan.h) against the serial recurrence for every cut, in place and out of place, and the argument checks of the Python layer."""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
import unwrap_cases as uc
import unwrap_ref as ur

CODE = {np.dtype(np.float32): _lib.F32, np.dtype(np.float64): _lib.F64}
CASES = uc.cpu_cases()


@pytest.fixture(scope="module")
def serial():
    """unwrap_serial of every case, computed once."""
    return {c.name: ur.unwrap_serial(c.m, 1, c.range) for c in CASES}


def emulate(m, range=None, segments=0, in_place=False):
    """mdsp_unwrap_emulate_host on an (outer, len, inner) array."""
    m = np.ascontiguousarray(m)
    outer, n, inner = m.shape
    r = float(ur.default_range(m.dtype) if range is None else m.dtype.type(range))
    src = m.copy()
    dst = src if in_place else np.full_like(m, 12345.0)
    _lib.check(_lib.lib().mdsp_unwrap_emulate_host(src.ctypes.data, dst.ctypes.data, inner, n, outer, CODE[m.dtype], r, segments))
    if not in_place:
        assert np.array_equal(src, m, equal_nan=True), "input modified"
    return dst


# ---- the restatement against the reference's literals (test/unwrap.jl:6-58) ----------------------------------------------------------------------------
def test_serial_reproduces_the_reference_literals(approx):
    pi = np.pi
    unwrapped = np.array([0.1, 0.2, 0.3, 0.4])
    for w in ([0.1, 0.2, 0.3, 0.4], [0.1, 0.2 + 2 * pi, 0.3, 0.4], [0.1, 0.2 - 2 * pi, 0.3, 0.4], [0.1, 0.2 - 2 * pi, 0.3 - 2 * pi, 0.4],
              [0.1, 0.2 + 6 * pi, 0.3, 0.4]):
        assert approx(ur.unwrap_serial(np.array(w)), unwrapped)                                   # :8-11, :13
    assert approx(ur.unwrap_serial(np.array([0.1 + 2 * pi, 0.2, 0.3, 0.4])), unwrapped + 2 * pi)  # :12
    test_v = np.array([0.1, 0.2, 0.3 + 2 * pi, 0.4])
    assert approx(ur.unwrap_serial(test_v), unwrapped)
    assert np.array_equal(test_v, [0.1, 0.2, 0.3 + 2 * pi, 0.4])                                  # :18 input left unmodified
    wrapped = np.repeat(np.array([0.1, 0.2 + 2 * pi, 0.3, 0.4])[:, None], 2, axis=1)              # :29-34
    assert approx(ur.unwrap_serial(wrapped, 1), wrapped)
    assert approx(ur.unwrap_serial(wrapped, 0), np.stack([unwrapped, unwrapped], axis=1))
    un = np.arange(1.0, 101.0)
    assert approx(ur.unwrap_serial(un % 10, 0, 10), un)                                           # :40-42
    for T in (np.float32, np.float64):                                                            # :45-58
        a_un = np.linspace(T(0), T(4) * T(np.pi), 10, dtype=T)
        a_w = np.fmod(a_un, T(2) * T(np.pi)).astype(T)
        got = ur.unwrap_serial(a_w)
        assert got.dtype == T and approx(got, a_un)
        r_un = np.linspace(0, 4, 10).astype(T)
        assert approx(ur.unwrap_serial(np.fmod(r_un, T(2)), 0, T(2)), r_un)


def test_scan_form_equals_the_serial_recurrence(serial):
    for c in CASES:
        if np.isfinite(c.m).all():
            assert ur.equal(ur.unwrap_scan(c.m, 1, c.range), serial[c.name]), c.name


def test_non_finite_rules_of_the_recurrence():
    inf, nan = np.inf, np.nan
    for T in (np.float32, np.float64):
        got = ur.unwrap_serial(np.array([0.1, 3, -3, inf, 0.2, 0.3], T))
        assert ur.equal(got, np.array([0.1, 3, T(-3) + ur.default_range(T), nan, nan, nan], T))
        assert ur.equal(ur.unwrap_serial(np.array([inf, 3, -3, 0.2], T)), np.full(4, inf, T))
        assert ur.equal(ur.unwrap_serial(np.array([-inf, 3, -3, 0.2], T)), np.full(4, -inf, T))
        assert ur.equal(ur.unwrap_serial(np.array([nan, 3, -3, 0.2], T)), np.full(4, nan, T))
        for bad in (nan, inf, -inf):                                   # a non-finite m[i], i >= 1: the rest of the line is NaN
            m = uc.walk(9, 1, 40, 1, T).ravel()
            clean = ur.unwrap_serial(m)
            m[17] = bad
            got = ur.unwrap_serial(m)
            assert ur.equal(got[:17], clean[:17]) and np.isnan(got[17:]).all()
    assert np.float32(3.2831855) == ur.unwrap_serial(np.array([0.1, 3, -3], np.float32))[2]
    z = ur.unwrap_serial(np.array([0.5, -0.0, 0.0, -0.0]))            # signed zeros: equal() compares them equal, as the issue of this feature found
    assert ur.equal(z, np.array([0.5, 0.0, 0.0, 0.0]))


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------------
def test_geometry_tiles_every_line_exactly_once():
    REC = 24                                                           # bytes per segment record (csrc/unwrap_scan.h Rec)
    for inner in (1, 3, 64, 65, 1025):
        for n in (1, 2, 63, 64, 65, 1000, 262_141, 2 ** 28):
            for outer in (1, 3, 8):
                for dt in (np.float32, np.float64):
                    for seg in (0, 1, 3, 7):
                        route, S, seglen, ws = d.unwrap_geometry(inner, n, outer, dt, seg)
                        what = (inner, n, outer, np.dtype(dt).name, seg, route, S, seglen, ws)
                        assert route == (_lib.UNWRAP_CONTIGUOUS if inner == 1 else _lib.UNWRAP_STRIDED), what
                        assert 1 <= S <= n and seglen >= 1, what
                        # segments s = 0 .. S-1 are [s seglen, min(len, (s + 1) seglen)): non-empty, adjacent, and the last one ends at len
                        assert (S - 1) * seglen < n <= S * seglen, what
                        if n <= 2:
                            assert S == 1, what
                        elif seg > 0:
                            assert S == min(seg, n), what              # a forced cut is honoured after clamping
                        assert ws == (inner * outer * S * REC if S > 1 else 0), what
    # what the automatic cut does with the shapes it was made for
    assert d.unwrap_geometry(1, 2 ** 28, 1, np.float32)[1] > 1000                   # one long line: cut to fill the device
    assert d.unwrap_geometry(1025, 262_141, 8, np.float32)[1] > 1                   # 8 x 1025 frequency lines across frames: cut
    assert d.unwrap_geometry(1, 1024, 4 * 262_141, np.float32)[1] == 1              # a million short lines: single pass
    assert d.unwrap_geometry(1, 10_007, 1, np.float32)[1] == 2                      # tests/test_gpu_unwrap.py relies on this one being cut
    for bad in ((-1, 4, 1, np.float32, 0), (1, -4, 1, np.float32, 0), (1, 4, -1, np.float64, 0), (1, 4, 1, np.float32, -1)):
        with pytest.raises(d.ArgumentError):
            d.unwrap_geometry(*bad)
    for dtc in (_lib.C32, _lib.C64, 7):
        assert _lib.lib().mdsp_unwrap_geometry_for(1, 4, 1, dtc, 0, None, None, None, None) == _lib.ERR_ARGUMENT
    assert d.unwrap_geometry(0, 5, 3, np.float32)[3] == 0 and d.unwrap_geometry(3, 0, 3, np.float32)[3] == 0


# ---- the host emulation of the device code -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_emulation_equals_the_serial_recurrence(serial, segments, in_place):
    for c in CASES:
        got = emulate(c.m, c.range, segments, in_place)
        assert ur.equal(got, serial[c.name]), (c.name, segments)


def test_emulation_keeps_negative_zero_and_handles_the_stated_cases():
    got = emulate(np.array([0.5, -0.0, 0.0, -0.0]).reshape(1, 4, 1)).ravel()
    assert np.array_equal(np.signbit(got), [False, True, False, True])            # the integer form keeps -0.0 (K = 0: m - 0 range)
    for seg in (1, 2, 3):
        got = emulate(np.array([0.1, 3, -3, np.inf, 0.2, 0.3], np.float32).reshape(1, 6, 1), None, seg).ravel()
        assert ur.equal(got, np.array([0.1, 3, 3.2831855, np.nan, np.nan, np.nan], np.float32)), seg
        got = emulate(np.array([np.inf, 3, -3, 0.2], np.float32).reshape(1, 4, 1), None, seg).ravel()
        assert ur.equal(got, np.full(4, np.inf, np.float32)), seg


def test_emulation_argument_errors():
    lib = _lib.lib()
    x = np.zeros(8, np.float32)
    p = x.ctypes.data
    assert lib.mdsp_unwrap_emulate_host(p, p, 1, -8, 1, _lib.F32, 1.0, 0) == _lib.ERR_ARGUMENT
    for r in (0.0, np.inf, np.nan, 1e-60):                                         # 1e-60 is 0 in Float32
        assert lib.mdsp_unwrap_emulate_host(p, p, 1, 8, 1, _lib.F32, r, 0) == _lib.ERR_ARGUMENT, r
    assert lib.mdsp_unwrap_emulate_host(p, p, 1, 8, 1, _lib.C32, 1.0, 0) == _lib.ERR_ARGUMENT
    assert lib.mdsp_unwrap_emulate_host(None, None, 1, 0, 1, _lib.F32, 1.0, 0) == _lib.OK       # a size of 0: nothing to do
    h = C.c_void_p()
    for r in (0.0, np.inf, np.nan):
        assert lib.mdsp_unwrap_plan_create(C.byref(h), 1, 8, 1, _lib.F32, r, 0) == _lib.ERR_ARGUMENT
    assert lib.mdsp_unwrap_plan_create(C.byref(h), 1, 8, 1, _lib.C64, 1.0, 0) == _lib.ERR_ARGUMENT
    assert lib.mdsp_unwrap_plan_create(C.byref(h), 1, -1, 1, _lib.F32, 1.0, 0) == _lib.ERR_ARGUMENT


# ---- the Python layer: every argument error before device work -------------------------------------------------------------------------------------------
def test_argument_and_type_errors_come_before_device_work():
    m1, m2 = np.zeros(8), np.zeros((4, 3))
    with pytest.raises(d.ArgumentError):
        d.unwrap(m2)                                                   # src/unwrap.jl:19-21: N-d without dims
    with pytest.raises(d.ArgumentError):
        d.unwrap_(m2.copy(), m2)
    for all_axes in (range(2), (0, 1), [0, 1]):
        with pytest.raises(d.UnsupportedError, match="N-d"):
            d.unwrap(m2, dims=all_axes)                                # :26-27, not accelerated
    for bad in ((1, 0), (0,), "a", 1.0, range(1, 2), 2, -3):
        with pytest.raises(d.ArgumentError):
            d.unwrap(m2, dims=bad)                                     # :28-29
    for dt in (np.int32, np.int64, np.complex64, np.complex128):
        with pytest.raises(TypeError):
            d.unwrap(np.zeros(8, dt))
    with pytest.raises(d.ArgumentError):
        d.unwrap_(np.zeros(7), m1)                                     # shapes differ
    with pytest.raises(d.ArgumentError):
        d.unwrap_(np.zeros(8, np.float32), m1)                         # element types differ
    for r in (0, np.inf, np.nan):
        with pytest.raises(d.ArgumentError):
            d.unwrap(m1, range=r)
    if _lib.device_count() == 0:
        with pytest.raises(d.DeviceError):
            d.unwrap(m1)
        with pytest.raises(d.DeviceError):
            d.unwrap_(m2, dims=1)
        with pytest.raises(d.DeviceError):
            d.unwrap(m2, dims=-1, range=10)
