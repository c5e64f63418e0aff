"""Filter responses without a device: the host emulation of the response kernels (mdsp_resp_emulate_host: the same cut, chunk order, squaring chain and
operators as the device code, csrc/resp_op.h) against the long-double restatement of tests/response_ref.py, the geometry rule, the reference's exact
cases and MATLAB goldens, and the argument errors of the ABI and of the public functions."""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
import response_cases as rc
import response_ref as rr
from conftest import isapprox

# the worst measured e_cut / e_serial over the case table is 2.30 (Float64, 4101 taps with the derivative weights in 257 chunks of 16);
# twice that, rounded up to a power of two.  The yardstick of both errors is the long-double restatement, not the code under test.
RATIO_BOUND = 8.0


@pytest.fixture(scope="module")
def rgolden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "response_golden.npz"))


def test_emulation_is_as_accurate_as_a_serial_chain():
    rows = rc.accuracy_table()
    assert len(rows) > 60
    for label, tname, e_cut, e_serial, ratio in rows:
        print(f"{label:40s} {tname:8s} e_cut {e_cut:.3e} e_serial {e_serial:.3e} ratio {ratio:.3f}")
    worst = max(rows, key=lambda r: r[4])
    assert worst[4] <= RATIO_BOUND, worst


def test_geometry_of_forced_and_automatic_cuts():
    P, F32, F64 = rc.POLY, np.float32, np.float64
    # forced: L = the power of two >= ceil(n / chunks), at least 16; C = ceil(n / L); workspace = polynomials x C x nw complex values
    assert rc.geometry(P, F64, 53, False, 257, 1) == (1, 64, 0)
    assert rc.geometry(P, F64, 53, False, 257, 2) == (2, 32, 2 * 257 * 16)
    assert rc.geometry(P, F64, 53, True, 257, 3) == (2, 32, 2 * 2 * 257 * 16)          # n = 53 is no multiple of L: the last chunk holds 21
    assert rc.geometry(P, F32, 53, True, 257, 3) == (2, 32, 2 * 2 * 257 * 8)
    assert rc.geometry(P, F64, 53, False, 65, 1000) == (4, 16, 4 * 65 * 16)            # the forced L stops at 16
    assert rc.geometry(P, F64, 4101, False, 7, rc.max_chunks(4101)) == (257, 16, 257 * 7 * 16)
    for n, want in ((15, 1), (16, 1), (17, 2), (31, 2), (32, 2), (33, 3)):              # L - 1, L and L + 1 coefficients
        assert rc.geometry(P, F64, n, True, 64, 1000)[:2] == (want, 16), n
    assert rc.geometry(P, F64, 1, False, 1, 3) == (1, 16, 0)
    # automatic: a single chain unless the points alone leave the device empty and the polynomial is long
    assert rc.geometry(P, F64, 53, True, 257)[0] == 1 and rc.geometry(P, F64, 53, True, 257)[2] == 0
    assert rc.geometry(P, F64, 64, False, 1 << 20) == (1, 64, 0)
    assert rc.geometry(P, F64, 1 << 19, False, 257) == (256, 2048, 256 * 257 * 16)     # 5 tiles x 256 chunks of 2048
    assert rc.geometry(P, F32, 4101, False, 257) == (17, 256, 17 * 257 * 8)            # chunks of at least 256
    assert rc.geometry(P, F64, 1 << 16, True, 1 << 16) == (2, 1 << 15, 2 * 2 * (1 << 16) * 16)
    assert rc.geometry(P, F64, 1 << 16, True, 1 << 17)[0] == 1                          # 2048 tiles fill the device
    assert rc.geometry(P, F64, 4101, False, 0)[0] == 1
    # SECTIONS and ZPK are never cut
    assert rc.geometry(rc.SECTIONS, F64, 16, False, 257, 3) == (1, 16, 0)
    assert rc.geometry(rc.ZPK, F32, 4000, True, 257, 3) == (1, 16, 0)
    with pytest.raises(d.ArgumentError):
        rc.geometry(P, F64, 53, False, 257, -1)
    with pytest.raises(d.ArgumentError):
        rc.geometry(P, np.complex64, 53, False, 257)
    assert d.resp_geometry(P, F64, 53, True, 257, 3) == rc.geometry(P, F64, 53, True, 257, 3)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_cut_handles_unequal_lengths_and_an_absent_denominator(R):
    """nb != na, n no multiple of L, an absent den: every forced cut stays within a few roundings of the single chain."""
    rng = np.random.default_rng(11)
    y = rc.points(np.linspace(0.1, 3.0, 67), R, neg=True)
    for nb, na in ((53, 17), (17, 53), (33, 1), (16, 16), (15, 33)):
        b, a = rng.standard_normal(nb).astype(R), np.concatenate([[1.0], 0.01 * rng.standard_normal(na - 1)]).astype(R)
        for den in (a, None):
            ld = rr.poly_ld(b, den, y, R)
            for chunks in (1, 2, 3, 1000):
                got = rc.emulate(rc.POLY, R, b, den, y, chunks=chunks)
                assert rr.max_error(got, ld) <= 64 * np.finfo(R).eps, (nb, na, den is None, chunks)


@pytest.mark.parametrize("R", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_exact_cases_of_the_reference(R):
    x = rc.points(np.linspace(0, 2 * np.pi, 50), R)
    want = np.full(50, 42.0, dtype=rc.ctype(R))
    got = rc.emulate(rc.ZPK, R, np.zeros(0, complex), np.zeros(0, complex), x, gain=42.0)          # test/filter_response.jl:58
    assert np.array_equal(got, want) and not np.signbit(got.imag).any()
    got = rc.emulate(rc.SECTIONS, R, np.zeros((0, 5)), None, x, gain=42.0)                           # :59
    assert np.array_equal(got, want)
    # DERIV: the numerator's coefficients are the host's arange(n) * c, bit for bit
    c = rc.windowed_sinc(53).astype(R)
    kc = (np.arange(53).astype(R) * c).astype(R)
    y = rc.points(np.linspace(0, np.pi, 65), R, neg=True)
    for chunks in (1, 3):
        a = rc.emulate(rc.POLY, R, c, None, y, flags=rc.DERIV, chunks=chunks)
        b = rc.emulate(rc.POLY, R, kc, None, y, chunks=chunks)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        a = rc.emulate(rc.POLY, R, c, c, y, flags=rc.DERIV, out_mode=rc.REAL_MINUS, cminus=3.0, chunks=chunks)
        b = rc.emulate(rc.POLY, R, kc, c, y, out_mode=rc.REAL_MINUS, cminus=3.0, chunks=chunks)
        assert a.dtype == np.dtype(R) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_goldens_through_the_emulation(rgolden):
    """test/filter_response.jl:15-37, :87-112, :199-212 at the reference's own tolerance (norm-wise rtol sqrt(eps))."""
    R, b, a = np.float64, rc.GOLDEN_B, rc.GOLDEN_A
    fz = rgolden["freqz_eg1"]
    w = np.linspace(0, 6.280045284537, 2001)
    h = rc.emulate(rc.POLY, R, b, a, rc.points(w, R, neg=True))
    assert isapprox(np.abs(h), fz[:, 1])
    resp = rgolden["responses_eg1"]
    w = resp[:, 0]
    h = rc.emulate(rc.POLY, R, b, a, rc.points(w, R, neg=True))
    assert isapprox(np.abs(h), resp[:, 3])
    assert isapprox(np.unwrap(np.angle(h)), resp[:, 4])
    assert isapprox(np.unwrap(rc.emulate(rc.POLY, R, b, a, rc.points(w, R, neg=True), out_mode=rc.ANGLE)), resp[:, 4])
    sos = d.SecondOrderSections(d.PolynomialRatio(b, a))
    assert isapprox(np.abs(rc.emulate(rc.SECTIONS, R, sos.table(), None, rc.points(w, R), gain=sos.g)), resp[:, 3])
    zpk = d.ZeroPoleGain(d.PolynomialRatio(b, a))
    assert isapprox(np.abs(rc.emulate(rc.ZPK, R, zpk.z, zpk.p, rc.points(w, R), gain=zpk.k)), resp[:, 3])
    gd = rgolden["grpdelay_eg1"]
    c = np.convolve(b, a[::-1])                                   # xcorr(b, a; padmode = :none)
    for chunks in (1, 1000):
        tau = rc.emulate(rc.POLY, R, c, c, rc.points(gd[:, 0], R, neg=True), flags=rc.DERIV, out_mode=rc.REAL_MINUS, cminus=len(a) - 1, chunks=chunks)
        assert isapprox(tau, gd[:, 1])


def test_delay_filter_converts_between_all_four_types():
    """test/filter_response.jl:76-79: what grpdelay does first (coefb / coefa); a ZeroPoleGain without zeros used to fail in the conversion."""
    Hdelay = d.PolynomialRatio([0.0, 1.0], [1.0])
    y = np.exp(-0.7j)
    for Tf in (d.PolynomialRatio, d.ZeroPoleGain, d.Biquad, d.SecondOrderSections):
        b, a = d.coefb(Tf(Hdelay)), d.coefa(Tf(Hdelay))
        assert a[0] == 1 and abs(np.polyval(b[::-1], y) / np.polyval(a[::-1], y) - y) < 1e-15, Tf


def test_argument_errors_at_the_abi():
    lib = _lib.lib()
    one = np.ones(5)
    pts, out = np.ones(4, np.complex128), np.zeros(4, np.complex128)

    def emu(form, flags=0, out_mode=rc.COMPLEX, dtype=_lib.F64, nnum=1, nden=0, den=None, chunks=0, points=pts, res=out):
        _lib.check(lib.mdsp_resp_emulate_host(points.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), form, flags, out_mode, dtype,
                                              one.ctypes.data_as(_lib.pdbl), nnum, None if den is None else den.ctypes.data_as(_lib.pdbl), nden, 1.0, 0.0, 4, chunks))

    emu(rc.POLY)
    for kw in (dict(form=rc.SECTIONS, flags=rc.DERIV), dict(form=rc.ZPK, flags=rc.DERIV),      # a form / flag mismatch
               dict(form=rc.SECTIONS, nden=1, den=one), dict(form=3), dict(form=rc.POLY, flags=4), dict(form=rc.POLY, out_mode=3),
               dict(form=rc.POLY, dtype=_lib.C64), dict(form=rc.POLY, nnum=0), dict(form=rc.POLY, nnum=-1), dict(form=rc.POLY, chunks=-1),
               dict(form=rc.POLY, nden=2, den=None), dict(form=rc.POLY, res=pts)):
        with pytest.raises(d.ArgumentError):
            emu(**kw)
    big = np.ones(5 * 17)
    with pytest.raises(d.UnsupportedError):
        _lib.check(lib.mdsp_resp_emulate_host(pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rc.SECTIONS, 0, 0, _lib.F64,
                                              big.ctypes.data_as(_lib.pdbl), 17, None, 0, 1.0, 0.0, 4, 0))
    nan = np.array([1.0, np.nan])
    with pytest.raises(d.ArgumentError):
        _lib.check(lib.mdsp_resp_emulate_host(pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), rc.POLY, 0, 0, _lib.F64,
                                              nan.ctypes.data_as(_lib.pdbl), 2, None, 0, 1.0, 0.0, 4, 0))
    h = C.c_void_p()
    with pytest.raises(d.ArgumentError):
        _lib.check(lib.mdsp_resp_plan_create(C.byref(h), rc.SECTIONS, rc.DERIV, 0, 0, _lib.F64, one.ctypes.data_as(_lib.pdbl), 1, None, 0, 1.0, 0.0, 4, 0))
    assert not h.value
    plan = d.RespPlan(rc.POLY, np.float64, np.ones(600), None, nw=8, chunks=0)                # a plan needs no device
    assert (plan.chunks, plan.chunk_len, plan.workspace_bytes) == (3, 256, 3 * 8 * 16)
    with pytest.raises(d.ArgumentError):
        plan.exec(0, 0, 0)                                                                     # NULL buffers: refused before any device work


def test_argument_errors_of_the_public_functions_come_before_device_work():
    df = d.PolynomialRatio(rc.GOLDEN_B, rc.GOLDEN_A)
    for fn in (d.freqresp, d.phaseresp, d.grpdelay):
        with pytest.raises(d.UnsupportedError):
            fn(df, np.array([0.1 + 0.2j]))                                                     # a complex w
        with pytest.raises(TypeError):
            fn([1.0, 2.0], np.ones(3))                                                         # not a filter
    with pytest.raises(d.UnsupportedError):
        d.PolynomialRatio(np.array([1.0 + 1j, 2.0]), np.array([1.0]))                          # a complex coefficient
    with pytest.raises(d.UnsupportedError):
        d.RespPlan(rc.POLY, np.float64, np.array([1.0 + 1j, 2.0]), None, nw=4)
    for fn in (d.impresp, d.stepresp):
        with pytest.raises(d.ArgumentError):
            fn(df, -1)                                                                         # n < 0
        with pytest.raises(TypeError):
            fn(df, 2.5)
    if _lib.device_count() == 0:
        biq = d.Biquad(1.0, 0.5, 0.25, -0.1, 0.2)
        for f in (df, biq, d.SecondOrderSections(biq), d.ZeroPoleGain(biq), d.PolynomialRatio([1.0, 2.0, 1.0])):
            for fn in (d.freqresp, d.phaseresp, d.grpdelay):
                with pytest.raises(d.DeviceError):
                    fn(f)
                with pytest.raises(d.DeviceError):
                    fn(f, np.zeros(0))                                                         # an empty w too: there is no CPU path
            for fn in (d.impresp, d.stepresp):
                with pytest.raises(d.DeviceError):
                    fn(f, 10)
