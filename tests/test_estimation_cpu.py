"""jacobsen / quinn without a device: the geometry, the host emulations of the two reductions and of a quinn pass (the text the kernels compile) against
their serial definitions and the long-double restatement of estimation.jl (tests/estimation_ref.py), the whole estimator over emulated passes, and
jacobsen's host arithmetic from emulated peak records.  DESIGN.md 4.15 holds the measured tables the bounds PASS_C and AGREE_TOL (tests/estimation_cases.py) come from."""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib, estimation as est

import estimation_cases as ec
import estimation_ref as ref

from estimation_cases import AGREE_TOL, PASS_C


def _quinn_geo(dt, n, segments=0):
    return d.quinn_geometry(dt, n, segments)


def test_quinn_geometry():
    for dt in ec.DTYPES:
        per_seg = 40 if np.dtype(dt).kind == "c" else 32
        assert _quinn_geo(dt, 501) == (1, 501, ec.TILE, ec.RUN, 0)
        assert _quinn_geo(dt, 4 * ec.TILE * 2 - 1) == (1, 8 * ec.TILE - 1, ec.TILE, ec.RUN, 0)          # under two shortest segments: no cut
        assert _quinn_geo(dt, 4 * ec.TILE * 2) == (2, 4 * ec.TILE, ec.TILE, ec.RUN, 2 * per_seg)
        S, seglen, _, _, ws = _quinn_geo(dt, 1 << 28)
        assert (S, seglen, ws) == (2048, 1 << 17, 2048 * per_seg)                                        # 256 x 8 wavefronts
        S, seglen, _, _, _ = _quinn_geo(dt, (1 << 24) + 5)
        assert seglen % ec.TILE == 0 and (S - 1) * seglen < (1 << 24) + 5 <= S * seglen                 # an automatic cut falls on tile boundaries
        assert _quinn_geo(dt, 130, 65)[:2] == (65, 2)                                                    # forced: ceil(n / segments)
        assert _quinn_geo(dt, 2 * ec.TILE + 3, 3)[:2] == (3, 684)
        assert _quinn_geo(dt, 3, 7)[:2] == (3, 1)                                                        # clamped to n
        assert _quinn_geo(dt, 10, 4)[:2] == (4, 3)                                                       # ceil(10 / 4) = 3: no empty segment
    for bad in ((np.float32, 1, 0), (np.float32, 0, 0), (np.float64, -5, 0), (np.complex64, 100, -1)):
        with pytest.raises(d.ArgumentError):
            _quinn_geo(*bad)
    with pytest.raises(d.ArgumentError):
        _lib.check(_lib.lib().mdsp_quinn_geometry_for(7, 100, 0, None, None, None, None, None))


def test_est_reduce_geometry():
    geo = est.est_reduce_geometry
    assert geo(1, 1 << 20, 1, _lib.EST_SUM, np.float32) == d.reduce_geometry(1, 1 << 20, 1, _lib.REDUCE_SUMABS2, np.float32)[:4] + ((1 << 20) // 8192 * 8,)
    route, S, seglen, depth, ws = geo(1, 1 << 20, 1, _lib.EST_SUM, np.complex64)
    assert (route, S, seglen, ws) == (_lib.REDUCE_CONTIGUOUS, 128, 8192, 128 * 16)
    assert geo(1, 1 << 20, 1, _lib.EST_ABS2ARGMAX, np.complex128)[4] == 128 * 24
    assert geo(1, 1000, 1, _lib.EST_ABS2ARGMAX, np.complex64, 3)[1:3] == (3, 334)
    assert geo(1, 1000, 1, _lib.EST_SUM, np.float64)[1:3] + (geo(1, 1000, 1, _lib.EST_SUM, np.float64)[4],) == (1, 1000, 0)
    assert geo(4, 1000, 2, _lib.EST_SUM, np.float64, 2)[:3] == (_lib.REDUCE_STRIDED, 2, 500)
    assert geo(1, 0, 1, _lib.EST_SUM, np.float32)[1] == 1
    for bad in ((1, -1, 1, _lib.EST_SUM, np.float32, 0), (1, 8, 1, 2, np.float32, 0), (1, 8, 1, -1, np.complex64, 0),
                (1, 8, 1, _lib.EST_ABS2ARGMAX, np.float32, 0), (1, 8, 1, _lib.EST_ABS2ARGMAX, np.float64, 0), (1, 8, 1, _lib.EST_SUM, np.float32, -1)):
        with pytest.raises(d.ArgumentError):
            geo(*bad)


def _serial_sum(x):
    """SUM's definition: every element exactly in Float64; the emulation's order differs, so compare against the exact sum with the bound of the depth."""
    return x.astype(np.clongdouble if x.dtype.kind == "c" else np.longdouble).sum()


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_sum_emulation_against_its_definition(dt):
    dt = np.dtype(dt)
    V = 16 // dt.itemsize
    rng = np.random.default_rng(3)
    for n in ec.REDUCE_LENGTHS:
        x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if dt.kind == "c" else 0)
        x = x.astype(dt)
        # integers small enough for every partial sum to be exact: any order gives the same bits as the definition
        xi = rng.integers(-1000, 1000, n).astype(dt) + ((1j * rng.integers(-1000, 1000, n)).astype(dt) if dt.kind == "c" else 0)
        for S in ec.REDUCE_CUTS:
            for phase in range(V):
                got = ec.est_reduce_emulate(x, _lib.EST_SUM, S, phase)[0]
                want = _serial_sum(x)
                got = complex(got[0], got[1]) if dt.kind == "c" else got[0]
                scale = float(np.abs(x.astype(np.complex128 if dt.kind == "c" else np.float64)).sum())
                assert abs(got - complex(want) if dt.kind == "c" else got - float(want)) <= 64 * 2.0 ** -53 * scale, (n, S, phase)   # depth <= 64 additions here
                goti = ec.est_reduce_emulate(xi.astype(dt), _lib.EST_SUM, S, phase)[0]
                wanti = _serial_sum(xi.astype(dt))
                assert (complex(goti[0], goti[1]) == complex(wanti)) if dt.kind == "c" else (goti[0] == float(wanti)), (n, S, phase)
    # lines of an (outer, len, inner) array: the strided route
    a = rng.integers(-50, 50, (2, 37, 3)).astype(dt)
    got = ec.est_reduce_emulate(a, _lib.EST_SUM, 2)
    want = a.astype(np.complex128 if dt.kind == "c" else np.float64).sum(axis=1).reshape(-1)
    got = got[:, 0] + 1j * got[:, 1] if dt.kind == "c" else got[:, 0]
    assert np.array_equal(got, want)


def _serial_argmax(X):
    """ABS2ARGMAX's definition: the first maximum of the Float64 |X|^2 (re*re + im*im, each operation rounded) among the bins that are not NaN."""
    re, im = X.real.astype(np.float64), X.imag.astype(np.float64)
    p = re * re + im * im
    nan = np.isnan(p)
    if nan.all():
        return -1, int(nan.any())
    return int(np.argmax(np.where(nan, -1.0, p))), int(nan.any())


@pytest.mark.parametrize("dt", [np.complex64, np.complex128], ids=lambda t: np.dtype(t).name)
def test_abs2argmax_emulation_against_its_definition(dt):
    dt = np.dtype(dt)
    V = 16 // dt.itemsize
    rng = np.random.default_rng(4)
    for n in ec.REDUCE_LENGTHS:
        base = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)
        variants = [base]
        # ties: the same largest bin (and bins of equal |X|^2 with other signs) planted across lane, vector, tile and segment boundaries
        for places in ((0, n - 1), (n // 2, n // 2 + 1), (n // 3, 2 * n // 3), (min(n - 1, 64 * V - 1), min(n - 1, 64 * V)), (min(n - 1, V - 1), min(n - 1, V))):
            t = base.copy()
            for k, p in enumerate(places):
                t[min(p, n - 1)] = (7 - 24j) if k % 2 == 0 else (-24 + 7j)           # |.|^2 = 625 both, exactly
            variants.append(t)
        t = variants[-1].copy()
        t[n // 2] = complex(np.nan, 1.0)                                 # a NaN bin raises the flag and does not compete
        variants.append(t)
        variants.append(np.full(n, complex(np.nan, np.nan), dtype=dt))   # nothing competes
        variants.append(np.zeros(n, dtype=dt))                           # all equal: index 0
        for X in variants:
            want = _serial_argmax(X)
            for S in ec.REDUCE_CUTS:
                for phase in range(V):
                    got = ec.est_reduce_emulate(X, _lib.EST_ABS2ARGMAX, S, phase)[0]
                    assert tuple(got) == want, (n, S, phase)
    a = (rng.integers(-9, 9, (2, 41, 3)) + 1j * rng.integers(-9, 9, (2, 41, 3))).astype(dt)
    got = ec.est_reduce_emulate(a, _lib.EST_ABS2ARGMAX, 3)
    want = np.argmax(np.abs(a.astype(np.complex128)) ** 2, axis=1).reshape(-1)
    assert np.array_equal(got[:, 0], want) and not got[:, 1].any()


def _table():
    rows = [(f, dt, n, S) for f in ec.PASS_TONES for dt in ec.DTYPES for n in ec.PASS_LENGTHS for S in ec.PASS_CUTS]
    rows += [(f, dt) + ec.CARRY_CASE for f in ec.PASS_TONES for dt in ec.DTYPES]
    return rows


@pytest.fixture(scope="module")
def pass_errors():
    """(e_scan, e_serial) of every row of the table, computed once."""
    return {row: ec.pass_error(row[2], row[0], row[1], row[3]) for row in _table()}


@pytest.mark.parametrize("f", ec.PASS_TONES)
def test_quinn_pass_emulation_against_long_double(pass_errors, f):
    rows = [r for r in pass_errors if r[0] == f]
    e_serial = max(pass_errors[r][1] for r in rows)
    assert 0 < e_serial < 1e-9
    worst = max(rows, key=lambda r: pass_errors[r][0])
    print(f"tone {f}: e_serial {e_serial:.3g}, worst e_scan {pass_errors[worst][0]:.3g} at {worst}, ratio {pass_errors[worst][0] / e_serial:.3g}")
    for r in rows:
        assert pass_errors[r][0] <= PASS_C * e_serial, (r, pass_errors[r], e_serial)


def test_quinn_pass_first_states_and_cut_independence_of_exact_cases():
    """xi_1, xi_2 of the record are the recurrence's own first two values whatever the cut; on small integers every operation is exact and every cut
    gives the bits of the serial restatement."""
    rng = np.random.default_rng(5)
    for dt in (np.float32, np.float64):
        x = rng.integers(-3, 4, 40).astype(dt)
        want = ref.quinn_pass_real(x, 1.0, -1.0)
        for S in (1, 2, 3, 40):
            rec = ec.pass_emulate(x, 1.0, -1.0, S)
            assert tuple(rec) == tuple(float(v) for v in want), S
    for dt in (np.complex64, np.complex128):
        x = (rng.integers(-3, 4, 40) + 1j * rng.integers(-3, 4, 40)).astype(dt)
        S_, den = ref.quinn_pass_complex(x, 1 - 2j, 0.0)                 # c = 1: exact
        for S in (1, 2, 3, 40):
            rec = ec.pass_emulate(x, 1 - 2j, 0.0, S)
            assert (complex(rec[0], rec[1]), rec[2]) == (complex(S_), float(den)), S
    x = ec.tone(2 * ec.TILE + 3, 28.3, np.float64)
    recs = [ec.pass_emulate(x, ec.mean_of(x), ec.pass_param(28.3, np.float64), S) for S in (1, 3, 65)]
    assert all(r[2] == recs[0][2] and r[3] == recs[0][3] for r in recs)


def test_quinn_pass_argument_errors_and_overflow():
    x = np.ones(8)
    out, mu = (C.c_double * 4)(), (C.c_double * 2)(0.0, 0.0)
    call = _lib.lib().mdsp_quinn_pass_emulate_host
    for args in ((x.ctypes.data, _lib.F64, 1, 0, mu, 1.0, out), (x.ctypes.data, 9, 8, 0, mu, 1.0, out), (x.ctypes.data, _lib.F64, 8, -1, mu, 1.0, out),
                 (None, _lib.F64, 8, 0, mu, 1.0, out), (x.ctypes.data, _lib.F64, 8, 0, None, 1.0, out), (x.ctypes.data, _lib.F64, 8, 0, mu, 1.0, None)):
        with pytest.raises(d.ArgumentError):
            _lib.check(call(*args))
    big = np.ones(70000)
    with pytest.raises(d.UnsupportedError):                              # |alpha| > 2: the powers of A grow like 2.6^n
        _lib.check(call(big.ctypes.data, _lib.F64, len(big), 0, mu, 3.0, out))
    with pytest.raises(d.UnsupportedError):
        _lib.check(call(big.ctypes.data, _lib.F64, len(big), 0, mu, float("nan"), out))
    _lib.check(call(big.ctypes.data, _lib.F64, len(big), 0, mu, 2.0, out))   # a double pole at 1 runs: linear growth


def _hz_of_tol(beta_tol, f):
    """tol in beta as a frequency: f = fn acos(beta / 2) / pi."""
    return (ec.FS / 2) / np.pi * 0.5 / abs(np.sin(2 * np.pi * f / ec.FS)) * beta_tol


@pytest.mark.parametrize("segments", [0, 3])
def test_quinn_over_emulated_passes(segments):
    sr, sc = ec.reference_signals()
    assert AGREE_TOL <= _hz_of_tol(1e-6, 28.3)
    for x, truth, f0 in ((sr, 28.3, 50.0), (sr, 28.3, None), (sc, -40.3, -20.0), (sc, -40.3, None)):
        guess = ref.jacobsen(x, ec.FS) if f0 is None else f0
        got = ec.emulated_quinn(x, guess, ec.FS, segments=segments)
        want = ref.quinn(x, guess, ec.FS)
        print(f"truth {truth} f0 {f0}: {got} against {want}: differ by {abs(got[0] - want[0]):.3g} Hz")
        assert abs(got[0] - truth) <= 1e-3 and not got[1]                # test/estimation.jl:57-58
        assert got[1] == want[1] and got[2] == want[2]
        assert abs(got[0] - want[0]) <= AGREE_TOL
    assert ref.quinn(sr, 50.0, ec.FS)[2] == 17                           # the slow start from fs / 2
    # fs = 1.0, the guess from jacobsen (:70, :79)
    for x, truth in ((sr, 28.3 / ec.FS), (sc, -40.3 / ec.FS)):
        got = ec.emulated_quinn(x, ref.jacobsen(x, 1.0), 1.0, segments=segments)
        want = ref.quinn(x, ref.jacobsen(x, 1.0), 1.0)
        assert abs(got[0] - truth) <= 1e-3 and got[1:] == want[1:] and abs(got[0] - want[0]) <= AGREE_TOL / ec.FS


def _emulated_jacobsen(x, fs):
    x = np.asarray(x)
    n, real = len(x), x.dtype.kind != "c"
    X = np.fft.rfft(x) if real else np.fft.fft(x)
    arg = ec.est_reduce_emulate(X, _lib.EST_ABS2ARGMAX)[0]
    return est.jacobsen_from_record(ec.peak_emulate(X, n, real, arg), n, fs, real)


def test_jacobsen_arithmetic_from_emulated_peak_records():
    for x, fc in ec.jacobsen_cases():
        got = _emulated_jacobsen(x, ec.FS)
        assert abs(got - fc) <= 1e-5, (fc, got)                          # test/estimation.jl:29, :47, :51
        assert abs(got - ref.jacobsen(x, ec.FS)) <= 1e-9, fc
    # the wrap-around of a full transform and the mirrored ends of a one-sided one, bin by bin
    rng = np.random.default_rng(6)
    for n in (2, 3, 8, 9):
        x = rng.standard_normal(n)
        full, half = np.fft.fft(x), np.fft.rfft(x)
        for k in range(n):
            rec = ec.peak_emulate(full, n, False, [k, 0])
            assert np.array_equal(rec[2:].view(np.complex128), full[[(k - 1) % n, k, (k + 1) % n]]), (n, k)
        for k in range(n // 2 + 1):
            rec = ec.peak_emulate(half, n, True, [k, 0]).copy()
            assert np.allclose(rec[2:].view(np.complex128), full[[(k - 1) % n, k, (k + 1) % n]], rtol=0, atol=1e-14), (n, k)
    # a peak at DC and at the Nyquist bin of an even length, real signals
    assert _emulated_jacobsen(np.ones(16) + 1e-3 * np.cos(np.arange(16)), 1.0) < 1e-3
    assert abs(_emulated_jacobsen(np.cos(np.pi * np.arange(16)), 1.0) - 0.5) < 1e-12
    # a NaN flag or no candidate gives NaN; a bad record is refused
    assert np.isnan(est.jacobsen_from_record(np.array([3, 1, 0, 0, 0, 0, 0, 0], dtype=np.int64), 16, 1.0, True))
    assert np.isnan(est.jacobsen_from_record(ec.peak_emulate(np.full(9, np.nan + 0j), 16, True, [-1, 1]), 16, 1.0, True))
    with pytest.raises(d.ArgumentError):
        ec.peak_emulate(np.zeros(8, dtype=np.complex128), 16, True, [0, 0])
    with pytest.raises(d.ArgumentError):
        ec.peak_emulate(np.zeros(1, dtype=np.complex128), 1, False, [0, 0])


def test_argument_errors_come_before_device_work():
    for fn in (d.jacobsen, d.quinn):
        with pytest.raises(TypeError):
            fn(np.ones((4, 4)))
        with pytest.raises(TypeError):
            fn(np.array(["a", "b"]))
        with pytest.raises(d.ArgumentError):
            fn(np.ones(1))
        with pytest.raises(d.ArgumentError):
            fn(np.ones(0, dtype=np.complex64))
        with pytest.raises(d.UnsupportedError):
            fn(np.ones(8, dtype=np.float16))
        with pytest.raises(TypeError):
            fn(np.ones(8), "fast")
    with pytest.raises(TypeError):
        d.quinn(np.ones(8), 1.0, 2.0, 3.0)
    with pytest.raises(TypeError):
        d.quinn(np.ones(8), maxiters=2.5)
    with pytest.raises(d.ArgumentError):
        d.QuinnPlan(np.float32, 1)
    if _lib.device_count() == 0:
        with pytest.raises(d.DeviceError):
            d.jacobsen(np.ones(8))
        with pytest.raises(d.DeviceError):
            d.quinn(np.ones(8), 0.1, 1.0)
