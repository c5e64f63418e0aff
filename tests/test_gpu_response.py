"""Filter responses on the device: mdsp_resp_exec equals the host emulation bit for bit (POINTS input; every form, both types, point counts around the
tile of 64, coefficient counts around the forced chunk of 16, with and without a denominator and the derivative weights); the W input and the ANGLE
output -- the device's sincos and atan2 -- against the long-double restatement and numpy's arctan2; and the public functions freqresp, phaseresp,
grpdelay, impresp, stepresp on the reference's own test blocks (test/filter_response.jl) and MATLAB goldens."""
import os

import numpy as np
import pytest

import response_cases as rc
import response_ref as rr
import sos_cases as sc
from conftest import isapprox

pytestmark = pytest.mark.gpu

RATIO_BOUND = 8.0     # tests/test_response_cpu.py: twice the worst measured e_cut / e_serial, rounded up to a power of two
# errors in units of (unit roundoff of the working type x the largest magnitude of the result), twice the worst value observed over
# the cases of the two tests below, rounded up to a power of two
W_INPUT_ULPS = 64.0
ANGLE_ULPS = 4.0
PHASE_MARGIN = 0.1     # radians every phase case keeps from the cut at +-pi, by construction (asserted on numpy's own value)
TYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def rgolden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "response_golden.npz"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _device(d, form, R, num, den, arg, gain=1.0, flags=0, out_mode=rc.COMPLEX, in_mode=rc.POINTS, cminus=0.0, chunks=0):
    import torch
    arg = np.ascontiguousarray(np.asarray(arg).astype(rc.ctype(R) if in_mode == rc.POINTS else np.dtype(R)))
    plan = d.RespPlan(form, R, num, den, gain, arg.size, flags, out_mode, in_mode, cminus, chunks)
    odt = rc.ctype(R) if out_mode == rc.COMPLEX else np.dtype(R)
    tin = torch.from_numpy(arg).cuda()
    out = torch.zeros(arg.size, dtype=torch.from_numpy(np.zeros(1, odt)).dtype, device="cuda")
    plan.exec(tin.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), plan


def _points(nw, R, salt):
    """nw points of the unit circle and a few off it (POINTS takes any contour)"""
    rng = np.random.default_rng(100 + salt)
    p = np.exp(1j * rng.uniform(0, 2 * np.pi, nw)) * np.where(rng.random(nw) < 0.2, rng.uniform(0.8, 1.1, nw), 1.0)
    return p.astype(rc.ctype(R))


NWS = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("R", TYPES, ids=lambda t: np.dtype(t).name)
def test_poly_equals_the_host_emulation_bit_for_bit(d, R):
    rng = np.random.default_rng(3)
    for n in (1, 2, 15, 16, 17, 53):
        b = rng.standard_normal(n).astype(R)
        a = np.concatenate([[1.0], 0.05 * rng.standard_normal(n - 1)]).astype(R)
        for chunks in (0, 1, 3):
            for den in (None, a):
                for deriv in (False, True):
                    for nw in NWS:
                        what = f"n {n} chunks {chunks} den {den is not None} deriv {deriv} nw {nw}"
                        pts = _points(nw, R, n + nw)
                        flags = rc.DERIV if deriv else 0
                        out_mode, cm = (rc.REAL_MINUS, 2.0) if (deriv and den is not None) else (rc.COMPLEX, 0.0)
                        got, plan = _device(d, rc.POLY, R, b, den, pts, flags=flags, out_mode=out_mode, cminus=cm, chunks=chunks)
                        assert (plan.chunks, plan.chunk_len) == rc.geometry(rc.POLY, R, n, den is not None, nw, chunks)[:2], what
                        assert plan.chunks == (2 if chunks == 3 and n > 16 else 1), what
                        want = rc.emulate(rc.POLY, R, b, den, pts, flags=flags, out_mode=out_mode, cminus=cm, chunks=chunks)
                        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), what
    # one vector for both polynomials (what grpdelay passes)
    c = rng.standard_normal(53).astype(R)
    pts = _points(65, R, 9)
    for chunks in (1, 3):
        got, _ = _device(d, rc.POLY, R, c, c, pts, flags=rc.DERIV, out_mode=rc.REAL_MINUS, cminus=4.0, chunks=chunks)
        assert np.array_equal(_bits(got), _bits(rc.emulate(rc.POLY, R, c, c, pts, flags=rc.DERIV, out_mode=rc.REAL_MINUS, cminus=4.0, chunks=chunks)))


@pytest.mark.parametrize("R", TYPES, ids=lambda t: np.dtype(t).name)
def test_sections_and_zpk_equal_the_host_emulation_bit_for_bit(d, R):
    tb32, _ = sc.table("butter32_02")
    for K, (tb, g) in ((1, sc.table("butter2_02")), (2, (tb32[:2], 0.25)), (5, (tb32[:5], 0.0625)), (16, (tb32, 3.0e-5))):
        for nw in NWS:
            pts = _points(nw, R, K + nw)
            for out_mode in (rc.COMPLEX, rc.REAL_MINUS):
                got, plan = _device(d, rc.SECTIONS, R, tb, None, pts, gain=g, out_mode=out_mode, cminus=0.5, chunks=3)
                assert plan.chunks == 1 and plan.workspace_bytes == 0
                assert np.array_equal(_bits(got), _bits(rc.emulate(rc.SECTIONS, R, tb, None, pts, gain=g, out_mode=out_mode, cminus=0.5))), (K, nw, out_mode)
    rng = np.random.default_rng(5)
    for nz, npol in ((0, 0), (1, 0), (0, 1), (1, 1), (15, 15), (15, 1), (0, 15)):
        z = 0.9 * np.exp(1j * rng.uniform(0, 2 * np.pi, nz))
        p = 0.7 * np.exp(1j * rng.uniform(0, 2 * np.pi, npol))
        for nw in NWS:
            pts = _points(nw, R, nz + npol + nw)
            got, _ = _device(d, rc.ZPK, R, z, p, pts, gain=1.5)
            assert np.array_equal(_bits(got), _bits(rc.emulate(rc.ZPK, R, z, p, pts, gain=1.5))), (nz, npol, nw)
    x = rc.points(np.linspace(0, 2 * np.pi, 50), R)
    for form, num, den in ((rc.ZPK, np.zeros(0, complex), np.zeros(0, complex)), (rc.SECTIONS, np.zeros((0, 5)), None)):
        got, _ = _device(d, form, R, num, den, x, gain=42.0)                                     # test/filter_response.jl:58-59
        assert np.array_equal(got, np.full(50, 42.0, dtype=rc.ctype(R)))


def _w_cases(R):
    """(label, form, num, den, gain, flags, long double restatement at given points)"""
    b, a = np.asarray(rc.GOLDEN_B, R), np.asarray(rc.GOLDEN_A, R)
    h = rc.windowed_sinc(53).astype(R)
    m = (0.5 ** np.arange(12)).astype(R)            # minimum phase, no zero near the unit circle: the ratio of the derivative case stays well conditioned
    cases = [("poly golden", rc.POLY, b, a, 1.0, rc.NEG, lambda p: rr.poly_ld(b, a, p, R)),
             ("poly sinc53", rc.POLY, h, None, 1.0, rc.NEG, lambda p: rr.poly_ld(h, None, p, R)),
             ("poly geometric12 deriv", rc.POLY, m, m, 1.0, rc.NEG | rc.DERIV, lambda p: rr.poly_ld(m, m, p, R, deriv=True))]
    for name in ("butter2_02", "butter8_02"):
        tb, g = sc.table(name)
        cases.append((f"sections {name}", rc.SECTIONS, tb, None, g, 0, lambda p, tb=tb, g=g: rr.sections_ld(tb, g, p, R)))
    z, p_, k = rc.cancellation_zpk(R)
    cases.append(("zpk cancel", rc.ZPK, z, p_, k, 0, lambda p: rr.zpk_ld(z, p_, k, p, R)))
    return cases


@pytest.mark.parametrize("R", TYPES, ids=lambda t: np.dtype(t).name)
def test_w_input_against_the_long_double_restatement(d, R):
    """The point is formed by the device's sincos: not bit-comparable.  The yardstick is the long-double restatement at exp(+-iw) of the SAME rounded w,
    itself formed in long double.  An error of the point is multiplied by the filter's group delay, so the cases are filters of modest delay (at most
    26 samples, the 53-tap FIR); a narrow band-pass or a ratio with a zero of the denominator on the circle measures its own conditioning instead."""
    w = np.linspace(0.0, np.pi, 257).astype(R)
    u = float(np.finfo(R).eps) / 2
    worst = 0.0
    for label, form, num, den, gain, flags, ld_of in _w_cases(R):
        pts_ld = np.exp((-1j if flags & rc.NEG else 1j) * w.astype(np.longdouble).astype(np.clongdouble))
        ld = ld_of(pts_ld)
        for chunks in (1, 3):
            got, _ = _device(d, form, R, num, den, w, gain=gain, flags=flags, in_mode=rc.W, chunks=chunks)
            ulps = rr.max_error(got, ld) / u
            print(f"W input  {label:32s} {np.dtype(R).name} chunks {chunks}: {ulps:.2f} ulps")
            worst = max(worst, ulps)
    assert worst <= W_INPUT_ULPS, worst


@pytest.mark.parametrize("R", TYPES, ids=lambda t: np.dtype(t).name)
def test_angle_output_against_numpy_arctan2_of_the_devices_own_values(d, R):
    w = np.linspace(0.0, 2.5, 257).astype(R)
    u = float(np.finfo(R).eps) / 2
    tb, g = sc.table("butter2_02")
    cases = [("poly [1, 0.5]", rc.POLY, np.array([1.0, 0.5]), None, 1.0, rc.NEG),
             ("sections butter2_02", rc.SECTIONS, tb, None, g, 0),
             ("zpk (x - 0.5) / (x + 0.3)", rc.ZPK, np.array([0.5 + 0j]), np.array([-0.3 + 0j]), 2.0, 0)]
    worst = 0.0
    for label, form, num, den, gain, flags in cases:
        for in_mode, arg in ((rc.W, w), (rc.POINTS, rc.points(w, R, neg=bool(flags & rc.NEG)))):
            H, _ = _device(d, form, R, num, den, arg, gain=gain, flags=flags, in_mode=in_mode)
            phi, _ = _device(d, form, R, num, den, arg, gain=gain, flags=flags, in_mode=in_mode, out_mode=rc.ANGLE)
            want = np.arctan2(H.imag.astype(np.longdouble), H.real.astype(np.longdouble))
            assert np.max(np.abs(want)) <= np.pi - PHASE_MARGIN, label                            # the cases keep their distance from the cut
            ulps = float(np.max(np.abs(phi.astype(np.longdouble) - want)) / (u * np.max(np.abs(want))))
            print(f"ANGLE    {label:32s} {np.dtype(R).name} in_mode {in_mode}: {ulps:.2f} ulps")
            worst = max(worst, ulps)
            assert phi.dtype == np.dtype(R)
    assert worst <= ANGLE_ULPS, worst


# ---- the public functions ---------------------------------------------------------------------------------------------------------------------------
def _golden_filter(d):
    return d.PolynomialRatio(rc.GOLDEN_B, rc.GOLDEN_A)


def test_delay_filter_in_all_four_coefficient_types(d):
    """test/filter_response.jl:76-85"""
    Hdelay = d.PolynomialRatio([0.0, 1.0], [1.0])
    W = np.linspace(0, 2 * np.pi, 100)
    for Tf in (d.PolynomialRatio, d.ZeroPoleGain, d.Biquad, d.SecondOrderSections):
        H = Tf(Hdelay)
        assert isapprox(d.freqresp(H, W), np.exp(-1j * W)), Tf
        assert isapprox(d.phaseresp(H, W), -W), Tf
        assert isapprox(d.grpdelay(H, W), np.ones(100)), Tf
        assert np.array_equal(d.impresp(H, 10), [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]), Tf
        assert np.array_equal(d.stepresp(H, 10), [0, 1, 1, 1, 1, 1, 1, 1, 1, 1]), Tf
        assert d.impresp(H, 10).dtype == np.float64


def test_pole_zero_cancellation_runs_through_each_types_own_form(d):
    """test/filter_response.jl:45-60: through a conversion to PolynomialRatio these lose every digit"""
    w = np.linspace(0, 2 * np.pi, 50)
    z, p, k = rc.cancellation_zpk(np.float64)
    assert isapprox(d.freqresp(d.ZeroPoleGain(z.real, p.real, k), w), np.full(50, 42.0))
    tb, _ = rc.cancellation_biquad()
    assert isapprox(d.freqresp(d.Biquad(*tb[0]), w), np.full(50, 42.0))
    tb, g = rc.cancellation_sos()
    assert isapprox(d.freqresp(d.SecondOrderSections([d.Biquad(*row) for row in tb], g), w), np.full(50, 42.0))
    assert np.array_equal(d.freqresp(d.ZeroPoleGain(np.zeros(0), np.zeros(0), 42.0), w), np.full(50, 42.0 + 0j))
    assert np.array_equal(d.freqresp(d.SecondOrderSections([], 42.0), w), np.full(50, 42.0 + 0j))


def test_goldens_through_the_public_functions(d, rgolden):
    """test/filter_response.jl:15-37, :87-128"""
    df = _golden_filter(d)
    fz = rgolden["freqz_eg1"]
    w = np.linspace(0, 6.280045284537, 2001)
    h = d.freqresp(df, w)
    assert isapprox(np.abs(h), fz[:, 1])
    y = np.exp(-1j * w)
    assert isapprox(h, 0.05634 * (1 + y) * (1 - 1.0166 * y + y * y) / ((1 - 0.683 * y) * (1 - 1.4461 * y + 0.7957 * y * y)))
    resp = rgolden["responses_eg1"]
    w = resp[:, 0]
    assert isapprox(d.impresp(df, 512), resp[:, 1])
    assert isapprox(d.stepresp(df, 512), resp[:, 2])
    assert isapprox(np.abs(d.freqresp(df, w)), resp[:, 3])
    assert isapprox(np.abs(d.freqresp(d.SecondOrderSections(df), w)), resp[:, 3])
    assert isapprox(np.abs(d.freqresp(d.ZeroPoleGain(df), w)), resp[:, 3])
    assert isapprox(d.phaseresp(df, w), resp[:, 4])
    for fn in (d.freqresp, d.phaseresp):
        H, w1 = fn(df)
        assert np.array_equal(_bits(H), _bits(fn(df, w1)))
        assert w1.min() <= 0 and w1.max() >= np.pi and np.max(np.abs(np.diff(w1))) < 0.03 and len(w1) == 257
    assert isapprox(np.cumsum(d.impresp(df)), d.stepresp(df))
    assert len(d.impresp(df)) == 100 and len(d.stepresp(df)) == 100


def test_grpdelay_block(d, rgolden):
    """test/filter_response.jl:199-225"""
    gd = rgolden["grpdelay_eg1"]
    assert isapprox(d.grpdelay(_golden_filter(d), gd[:, 0]), gd[:, 1])
    for b, want in (([1, 1, 1, 1, 1], 2.0), ([1, 1, 1, 1, 1, 1], 2.5), ([1, 0, -1], 1.0), ([1, -1], 0.5)):       # linear phase, types I - IV
        tau, w = d.grpdelay(d.PolynomialRatio(np.array(b, dtype=np.float64), [1.0]))
        assert np.array_equal(tau, np.full(len(w), want)), b
        assert w.min() <= 0 and w.max() >= np.pi and np.max(np.abs(np.diff(w))) < 0.03
    # not linear phase: the general path, against the derivative of the phase of a one-zero filter, tau = (r^2 - r cos w) / (1 + r^2 - 2 r cos w) at b = [1, -r]
    r, w = 0.5, np.linspace(0, np.pi, 33)
    assert isapprox(d.grpdelay(d.PolynomialRatio([1.0, -r], [1.0]), w), (r * r - r * np.cos(w)) / (1 + r * r - 2 * r * np.cos(w)))


@pytest.mark.parametrize("R", TYPES, ids=lambda t: np.dtype(t).name)
def test_long_fir_with_the_automatic_cut(d, R):
    """4101 taps at 257 points: the automatic cut (17 chunks of 256) against the long-double restatement, under the bound of tests/test_response_cpu.py.
    The points are exact inputs of that protocol: here they are the device's own exp(-iw), read back through the delay filter (H = y, exact)."""
    h = rc.windowed_sinc(4101).astype(R)
    w = np.linspace(0, np.pi, 257).astype(R)
    assert d.resp_geometry(rc.POLY, R, 4101, False, 257)[:2] == (17, 256)
    pts = d.freqresp(d.PolynomialRatio(np.array([0, 1], dtype=R), np.array([1], dtype=R)), w)
    assert pts.dtype == rc.ctype(R) and np.max(np.abs(np.abs(pts.astype(complex)) - 1)) < 4 * np.finfo(R).eps
    H = d.freqresp(d.PolynomialRatio(h, np.array([1], dtype=R)), w)
    assert H.dtype == rc.ctype(R)
    ld = rr.poly_ld(h, None, pts, R)
    e, e_serial = rr.max_error(H, ld), rr.max_error(rr.poly_serial(h, None, pts, R), ld)
    print(f"4101 taps {np.dtype(R).name}: e {e:.3e} e_serial {e_serial:.3e}")
    assert e <= RATIO_BOUND * max(e_serial, float(np.finfo(R).eps) / 2)


def test_where_the_result_lives_and_its_shape(d):
    import torch
    df = _golden_filter(d)
    w = np.linspace(0.1, 3.0, 24)
    wd = torch.from_numpy(w).cuda()
    keep = wd.clone()
    for fn in (d.freqresp, d.phaseresp, d.grpdelay):
        host, dev = fn(df, w), fn(df, wd)
        assert isinstance(host, np.ndarray) and isinstance(dev, torch.Tensor) and dev.is_cuda
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(host)), fn
        assert torch.equal(wd, keep)                                                              # the input is unchanged
        nd = fn(df, w.reshape(2, 3, 4))
        assert nd.shape == (2, 3, 4)
        if fn is not d.phaseresp:                                                                 # (unwrap runs along the last dimension only)
            assert np.array_equal(_bits(nd.ravel()), _bits(host))
        assert fn(df, wd.reshape(4, 6)).shape == (4, 6)
        assert fn(df, list(w[:3])).shape == (3,)
        e = fn(df, np.zeros((0, 3)))
        assert isinstance(e, np.ndarray) and e.shape == (0, 3)
        e = fn(df, wd[:0])
        assert isinstance(e, torch.Tensor) and tuple(e.shape) == (0,)
    assert np.array_equal(d.phaseresp(df, w.reshape(2, 12))[1], d.phaseresp(df, w[12:]))
    lin = d.grpdelay(d.PolynomialRatio([1.0, 2.0, 1.0], [1.0]), wd)
    assert isinstance(lin, torch.Tensor) and lin.is_cuda and torch.all(lin == 1.0)
    # Float32 coefficients and a Float32 w work in ComplexF32; anything else in ComplexF64
    f32 = d.PolynomialRatio(np.array([1, 0.5], np.float32), np.array([1, -0.25], np.float32))
    assert d.freqresp(f32, w.astype(np.float32)).dtype == np.complex64 and d.freqresp(f32, w).dtype == np.complex128
    assert d.grpdelay(f32, w.astype(np.float32)).dtype == np.float32 and d.phaseresp(df, w.astype(np.float32)).dtype == np.float64
    y = d.impresp(df, 16, device=True)
    assert isinstance(y, torch.Tensor) and y.is_cuda and np.array_equal(y.cpu().numpy(), d.impresp(df, 16))
    assert d.impresp(df, 0).shape == (0,) and d.stepresp(df, 0).shape == (0,)


def test_what_the_section_kernels_refuse_surfaces_unchanged(d):
    tb, g = sc.table("butter34_02")                                                               # 17 sections
    big = d.SecondOrderSections([d.Biquad(*row) for row in tb], g)
    with pytest.raises(d.UnsupportedError):
        d.impresp(big, 10)
    with pytest.raises(d.UnsupportedError):
        d.freqresp(big, np.ones(3))
    with pytest.raises(d.UnsupportedError):
        d.stepresp(d.PolynomialRatio([1.0], [1.0, -1.5]), 10)                                     # a pole outside the unit circle
