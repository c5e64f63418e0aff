"""Biquad / SecondOrderSections filtering without a device: the host emulation (mdsp_sos_emulate_host: the text, cut, tiles and scan order of the
kernels) against plain numpy restatements of the reference (tests/sos_ref.py), the coefficient conversions, the geometry and the argument checks.

Accuracy.  For every table of sos_cases.ACCURACY and both real types, n = 3 tiles + 5, the cut forced to 3 segments:
    e_scan   = max |emulation - longdouble restatement| / max |longdouble restatement|
    e_serial = the same for the restatement in the working precision
and the bound is e_scan <= C e_serial, C = 8: twice the worst measured ratio, rounded up to a power of two.  Measured ratios e_scan / e_serial
(Float32, Float64) with this emulation:
    butter2_02 1.63 1.39 | butter5_02 0.82 1.51 | butter8_02 1.06 1.33 | ellip6_001 0.89 1.96 | butter_bp4_030_031 1.00 0.62 |
    butter2_0001 1.06 3.64 | butter32_02 0.72 0.83        (one uncut segment: 0.97 1.00 | 0.88 1.51 | 1.54 1.33 | 0.96 1.81 | 1.05 0.52 | 1.06 3.56 | 0.65 0.70)
"""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib

import sos_cases as sc
import sos_ref as sr

C_BOUND = 8.0
REAL = (np.float32, np.float64)


def _geometry(K=1, dt=np.float32):
    S, seglen, tile, run, ws = d.sos_geometry(K, dt, 1, 1)
    return tile, run


def _lengths():
    tile, P = _geometry()
    return [1, 2, P - 1, P, P + 1, tile - 1, tile, tile + 1, 2 * tile + 3]


CUTS = (1, 3)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", REAL, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("segments", CUTS)
def test_exact_integer_cases(dt, segments):
    conv = np.array([1.0, 2.0, 3.0])
    for n in _lengths():
        x = sc.small_integers(n, 2, dt, salt=n)
        y, _ = sc.emulate([sc.INTEGRATOR], None, x, dt, segments)
        assert np.array_equal(y, np.cumsum(x, axis=0, dtype=np.float64).astype(dt)), ("integrator", n)
        y, _ = sc.emulate([sc.FIR_ONLY], None, x, dt, segments)
        want = np.stack([np.convolve(x[:, c].astype(np.float64), conv)[:n] for c in range(2)], axis=1).astype(dt)
        assert np.array_equal(y, want), ("fir", n)
        xr = sc.signal(n, 2, dt, salt=n)
        y, _ = sc.emulate([sc.IDENTITY] * 3, 1.0, xr, dt, segments)
        assert np.array_equal(y, xr), ("identity", n)
        y, _ = sc.emulate([sc.INTEGRATOR], None, x, dt, segments, reverse=True)
        assert np.array_equal(y, np.cumsum(x[::-1], axis=0, dtype=np.float64)[::-1].astype(dt)), ("integrator reversed", n)


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_refs():
    """(longdouble restatement, working-precision restatement and its end state) per table and type, computed once."""
    tile, P = _geometry()
    n = 3 * tile + 5
    refs = {}
    for name in sc.ACCURACY:
        tb, g = sc.table(name)
        for dt in REAL:
            x = sc.signal(n, 1, dt)
            ref, st_ref = sr.sos_filt(tb, g, x, np.longdouble)
            ser, st_ser = sr.sos_filt(tb, g, x, dt)
            refs[name, np.dtype(dt).name] = (x, ref, ser, st_ref, st_ser)
    return refs


@pytest.mark.parametrize("dt", REAL, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("name", sc.ACCURACY)
def test_accuracy_against_the_reference_arithmetic(accuracy_refs, name, dt):
    tb, g = sc.table(name)
    x, ref, ser, _, _ = accuracy_refs[name, np.dtype(dt).name]
    y, _ = sc.emulate(tb, g, x, dt, segments=3)
    e_scan, e_serial = sr.rel_err(y, ref), sr.rel_err(ser, ref)
    print(f"{name} {np.dtype(dt).name}: e_scan {e_scan:.3e} e_serial {e_serial:.3e} ratio {e_scan / e_serial:.2f}")
    assert e_scan <= C_BOUND * e_serial
    again, _ = sc.emulate(tb, g, x, dt, segments=3)
    assert np.array_equal(y, again)


# ---- streaming --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", REAL, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("name", ["butter5_02", "ellip6_001", "butter32_02"])
def test_streaming_pieces_carry_the_state(accuracy_refs, name, dt):
    tile, P = _geometry()
    tb, g = sc.table(name)
    K = len(tb)
    x, ref, ser, st_ref, st_ser = accuracy_refs[name, np.dtype(dt).name]
    n = len(x)
    e_serial = sr.rel_err(ser, ref)
    e_state_serial = sr.rel_err(st_ser, st_ref)
    for split in (1, P - 1, P, tile + 1, n - 1):
        st = np.zeros((2, K, 1), dt)
        y1, st = sc.emulate(tb, g, x[:split], dt, state=st)
        y2, st = sc.emulate(tb, g, x[split:], dt, state=st)
        y = np.concatenate([y1, y2])
        assert sr.rel_err(y, ref) <= C_BOUND * e_serial, split
        assert sr.rel_err(st, st_ref) <= C_BOUND * max(e_state_serial, float(np.finfo(dt).eps)), split
        again, _ = sc.emulate(tb, g, x[:split], dt, state=np.zeros((2, K, 1), dt))
        assert np.array_equal(again, y1)


# ---- filtfilt ---------------------------------------------------------------------------------------------------------------------------------------
def _filtfilt_emulated(tb, g, x, dt):
    """filtfilt(sos, x) as filters._filtfilt_sections composes it, on the host: extrapolate, a forward pass, a reverse walk, trim."""
    K = len(tb)
    x = np.asarray(x, dt)
    flat = x.reshape(x.shape[0], -1)
    n = flat.shape[0]
    pad = min(6 * K, n - 1)
    sos = d.SecondOrderSections([d.Biquad(*row) for row in tb], g)
    zi = d.filt_stepstate(sos).astype(dt)
    out = np.empty_like(flat)
    for c in range(flat.shape[1]):
        ext = sr.extrapolate(flat[:, c], pad)
        ext, _ = sc.emulate(tb, g, ext, dt, state=(zi * ext[0])[:, :, None])
        ext, _ = sc.emulate(tb, g, ext, dt, state=(zi * ext[-1])[:, :, None], reverse=True)
        out[:, c] = ext[pad:pad + n]
    return out.reshape(x.shape)


@pytest.mark.parametrize("name", ["butter2_02", "butter5_02", "butter8_02"])
def test_filtfilt_matches_the_restatement_and_the_direct_form(name):
    tb, g = sc.table(name)
    K = len(tb)
    sos = d.SecondOrderSections([d.Biquad(*row) for row in tb], g)
    b, a = d.coefb(sos), d.coefa(sos)
    for n, ncols in ((2, 1), (6 * K, 1), (6 * K + 1, 1), (300, 1), (300, 2)):
        x = sc.signal(n, ncols, np.float64, salt=n)
        want = sr.sos_filtfilt(tb, g, x, np.float64)
        ref = sr.sos_filtfilt(tb, g, x, np.longdouble)
        got = _filtfilt_emulated(tb, g, x, np.float64)
        e_serial = max(sr.rel_err(want, ref), float(np.finfo(np.float64).eps))
        assert sr.rel_err(got, ref) <= C_BOUND * e_serial, n
        # test/filt.jl:293-303: filtfilt(sos, x) ~ filtfilt(pr, x).  The two extend the signal by min(6K, n - 1) and min(3 order, n - 1) samples: the same
        # number for an even order (6K = 3 order) and whenever n - 1 is the smaller; for the odd order 5 (K = 3) they are 18 and 15 from n = 17 on,
        # two different extended signals, whose results differ by the filter's response to the extension -- at n = 6K and 6K + 1 that is no rounding
        # error and the comparison does not apply; at n = 300 it has decayed below the tolerance.
        order = len(a) - 1
        if min(6 * K, n - 1) == min(3 * order, n - 1) or n == 300:
            assert np.allclose(got, sr.iir_filtfilt(b, a, x), rtol=1e-6, atol=1e-8), n
        else:
            assert name == "butter5_02" and n in (6 * K, 6 * K + 1)


# ---- conversions ------------------------------------------------------------------------------------------------------------------------------------
def _resp_sos(sos, w):
    z1 = np.exp(-1j * w)
    h = np.full(len(w), complex(sos.g))
    for q in sos.biquads:
        h = h * (float(q.b0) + float(q.b1) * z1 + float(q.b2) * z1 * z1) / (1 + float(q.a1) * z1 + float(q.a2) * z1 * z1)
    return h


def _resp_zpk(z, p, k, w):
    e = np.exp(1j * w)
    return k * np.prod(e[:, None] - np.asarray(z)[None, :], axis=1) / np.prod(e[:, None] - np.asarray(p)[None, :], axis=1)


@pytest.mark.parametrize("zpk", [sc.ZPK_BUTTER5, sc.ZPK_ELLIP6], ids=["butter5", "ellip6"])
def test_sections_from_zpk_keep_the_transfer_function(zpk):
    z, p, k = zpk
    sos = d.SecondOrderSections(d.ZeroPoleGain(np.array(z), np.array(p), k))
    w = np.pi * (np.arange(64) + 0.5) / 64
    assert np.allclose(_resp_sos(sos, w), _resp_zpk(z, p, k, w), rtol=1e-12, atol=1e-12)
    assert sos.g == k and sos.dtype == np.dtype(np.float64) and len(sos.biquads) == (len(p) + 1) // 2


def test_pole_order_and_odd_pole_placement():
    z, p, k = sc.ZPK_BUTTER5
    sos = d.SecondOrderSections(d.ZeroPoleGain(np.array(z), np.array(p), k))
    first = sos.biquads[0]
    assert first.a2 == 0 and first.b2 == 0                      # the odd (real) pole and its zero come first (:474-478)
    assert np.isclose(-float(first.a1), max(v.real for v in p if v.imag == 0))
    dist = [abs(abs(np.roots([1.0, float(q.a1), float(q.a2)])[0]) - 1) for q in sos.biquads[1:]]
    assert dist == sorted(dist, reverse=True)                   # built in reverse: the poles nearest the unit circle last (:440, :464-472)
    # PolynomialRatio -> ZeroPoleGain -> sections keeps the response too
    pr = d.PolynomialRatio(d.coefb(sos), d.coefa(sos))
    w = np.pi * (np.arange(64) + 0.5) / 64
    assert np.allclose(_resp_sos(d.SecondOrderSections(pr), w), _resp_zpk(z, p, k, w), rtol=1e-7, atol=1e-9)


def test_conversion_errors_and_types():
    with pytest.raises(d.ArgumentError):
        d.SecondOrderSections(d.ZeroPoleGain(np.array([0.1, 0.2, 0.3]), np.array([0.5, 0.4]), 1.0))          # :435
    with pytest.raises(d.ArgumentError):
        d.SecondOrderSections(d.ZeroPoleGain(np.array([0.5j]), np.array([0.5, 0.4]), 1.0))                   # :439
    with pytest.raises(d.ArgumentError):
        d.SecondOrderSections(d.ZeroPoleGain(np.array([0.5]), np.array([0.5j, 0.4]), 1.0))                   # :441
    with pytest.raises(d.ArgumentError):
        d.Biquad(d.PolynomialRatio([1.0, 2.0, 3.0, 4.0], [1.0, 0.5]))                                        # :267-269
    with pytest.raises(d.ArgumentError):
        d.PolynomialRatio([1.0], [0.0, 1.0])
    with pytest.raises(d.UnsupportedError):
        d.Biquad(1.0 + 1j, 0.0, 0.0, 0.0, 0.0)
    q = d.Biquad(d.PolynomialRatio([2.0, 1.0], [2.0, 1.0, 0.5]))
    assert q.coefficients() == (1.0, 0.5, 0.0, 0.5, 0.25)
    assert d.Biquad(2.0, 4.0, 6.0, 2.0, 1.0, 0.5, 3).coefficients() == (3.0, 6.0, 9.0, 0.5, 0.25)           # :246-247
    assert d.Biquad(np.float32(1), np.float32(0), np.float32(0), np.float32(0.5), np.float32(0)).dtype == np.dtype(np.float32)
    assert d.Biquad(1, 0, 0, -1, 0).dtype == np.dtype(np.float64)
    one = d.SecondOrderSections(q)
    assert one.g == 1 and len(one.biquads) == 1
    assert np.array_equal(d.coefb(q), [1.0, 0.5, 0.0]) and np.array_equal(d.coefa(q), [1.0, 0.5, 0.25])


@pytest.mark.parametrize("name", ["butter2_02", "butter5_02", "ellip6_001"])
def test_stepstate_holds_a_constant(name):
    tb, g = sc.table(name)
    sos = d.SecondOrderSections([d.Biquad(*row) for row in tb], g)
    zi = d.filt_stepstate(sos)
    assert np.allclose(zi, sr.filt_stepstate(tb), rtol=1e-13, atol=0)
    x = np.full(200, 2.5)
    y, _ = sr.sos_filt(tb, g, x, np.float64, state=(zi * 2.5)[:, :, None])
    assert np.allclose(y, y[0], rtol=1e-9, atol=0)


# ---- geometry, errors and checks --------------------------------------------------------------------------------------------------------------------
def test_geometry_equals_plan_info():
    tile, P = _geometry()
    assert tile == 64 * P
    tb, g = sc.table("butter5_02")
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        for n, ncols, seg in ((3 * tile + 5, 1, 3), (3 * tile + 5, 2, 0), (5, 1, 9), (1 << 24, 1, 0), (1 << 24, 4096, 0), (0, 3, 0), (7, 0, 2)):
            plan = d.SosPlan(tb, g, dt, n, ncols, seg)
            geo = d.sos_geometry(len(tb), dt, n, ncols, seg)
            assert geo == (plan.segments, plan.seglen, plan.tile, plan.run, plan.workspace_bytes)
            S, seglen, _, _, ws = geo
            if n and ncols:
                assert (S - 1) * seglen < n <= S * seglen
                if seg:
                    assert S == min(seg, n)                       # the forced cut is honoured, and clamped to the length
                lines = ncols * (2 if np.dtype(dt).kind == "c" else 1)
                assert ws == (lines * S * 2 * len(tb) * (4 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 8) if S > 1 else 0)
    assert d.sos_geometry(3, np.float32, 1 << 24, 1)[0] > 1       # one long column is cut
    assert d.sos_geometry(3, np.float32, 1 << 24, 4096)[0] == 1   # many columns are not


def _create(tb, K=None, gain=1.0, dtype=_lib.F32, n=8, ncols=1, segments=0):
    tb = np.ascontiguousarray(tb, np.float64)
    h = C.c_void_p()
    st = _lib.lib().mdsp_sos_plan_create(C.byref(h), tb.ctypes.data_as(_lib.pdbl), len(tb) if K is None else K, gain, 1, dtype, n, ncols, segments)
    if h:
        _lib.lib().mdsp_sos_plan_destroy(h)
    return st


def test_argument_errors_raised_before_device_work():
    tb, g = sc.table("butter5_02")
    assert _create(tb) == _lib.OK
    assert _create(tb, n=-1) == _lib.ERR_ARGUMENT
    assert _create(tb, ncols=-1) == _lib.ERR_ARGUMENT
    assert _create(tb, K=0) == _lib.ERR_ARGUMENT
    assert _create(tb, dtype=7) == _lib.ERR_ARGUMENT
    assert _create(tb, segments=-1) == _lib.ERR_ARGUMENT
    bad = tb.copy()
    bad[1, 3] = np.nan
    assert _create(bad) == _lib.ERR_ARGUMENT
    bad[1, 3] = np.inf
    assert _create(bad) == _lib.ERR_ARGUMENT
    assert _create(tb, gain=np.nan) == _lib.ERR_ARGUMENT
    assert _create(tb * 1e300, dtype=_lib.F32) == _lib.ERR_ARGUMENT          # not finite in the working type
    assert _create(tb, n=0) == _lib.OK and _create(tb, ncols=0) == _lib.OK
    # exec: ld < n and a partial overlap are refused before the plan touches a device (the addresses are never used)
    plan = d.SosPlan(tb, g, np.float32, 8, 2)
    with pytest.raises(d.ArgumentError):
        plan.exec(0x10000, 7, 0x20000, 8, stream=0)
    with pytest.raises(d.ArgumentError):
        plan.exec(0x10000, 8, 0x20000, 7, stream=0)
    with pytest.raises(d.ArgumentError):
        plan.exec(0x10000, 8, 0x10004, 8, stream=0)
    with pytest.raises(d.ArgumentError):
        plan.exec(0x10000, 8, 0x10000, 9, stream=0)
    with pytest.raises(d.ArgumentError):
        plan.exec(0, 8, 0x10000, 8, stream=0)
    x = np.zeros(8, np.float32)
    with pytest.raises(d.ArgumentError):
        sc.emulate(tb, g, x, np.float32, ld=7)
    d.SosPlan(tb, g, np.float32, 0, 2).exec(0, 0, 0, 0, stream=0)                       # empty: nothing to check, nothing to launch


def test_unsupported_cascades():
    tb17, g17 = sc.table("butter34_02")
    assert len(tb17) == 17
    x = sc.signal(32)
    with pytest.raises(d.UnsupportedError):
        d.SosPlan(tb17, g17, np.float64, 32, 1)
    with pytest.raises(d.UnsupportedError):
        d.filt(d.SecondOrderSections([d.Biquad(*row) for row in tb17], g17), x)
    r = 1.01
    unstable = d.Biquad(1.0, 0.0, 0.0, -2 * r * np.cos(0.3), r * r)
    with pytest.raises(d.UnsupportedError):
        d.filt(unstable, x)
    with pytest.raises(d.UnsupportedError):
        d.filtfilt(d.SecondOrderSections(d.Biquad(1.0, 0.0, 0.0, -1.01, 0.0)), x)
    with pytest.raises(d.UnsupportedError):
        d.DF2TFilter(unstable)
    # poles ON the unit circle run: the integrator, a resonator, a double pole at 1
    for row in (sc.INTEGRATOR, (1.0, 0.0, 0.0, -2 * np.cos(0.3), 1.0), (1.0, 0.0, 0.0, -2.0, 1.0)):
        y, _ = sc.emulate([row], None, sc.small_integers(100), np.float64, segments=3)
        assert np.all(np.isfinite(y))
    # the direct forms keep raising what they raised
    with pytest.raises(d.UnsupportedError):
        d.filt(np.ones(2), np.array([1.0, -0.5]), x)
    with pytest.raises(d.UnsupportedError):
        d.DF2TFilter(np.ones(2), np.array([1.0, -0.5]))
    with pytest.raises(d.UnsupportedError):
        d.filtfilt(np.ones(2), np.array([1.0, -0.5]), x)


def test_a_nan_sample_spreads_as_in_the_reference():
    tile, P = _geometry()
    n, i = 2 * tile + 3, tile + 5
    for rows, g in (([sc.FIR_ONLY, sc.FIR_ONLY], 0.5), (sc.table("butter5_02")[0], 1.0), ([sc.FIR_ONLY, sc.table("butter2_02")[0][0]], 1.0)):
        for dt in REAL:
            x = sc.signal(n, 2, dt)
            clean, _ = sc.emulate(rows, g, x, dt, segments=3)
            x[i, 1] = np.nan
            ref, _ = sr.sos_filt(rows, g, x, dt)
            for seg in CUTS:
                y, _ = sc.emulate(rows, g, x, dt, segments=seg)
                assert np.array_equal(np.isfinite(y), np.isfinite(ref))
                assert np.array_equal(y[:, 0], clean[:, 0]) and np.array_equal(y[:i, 1], clean[:i, 1]) if seg == 3 else True
