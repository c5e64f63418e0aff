"""Filter design without a device: the prototypes, analog and digital designs against scipy.signal's (tests/golden/design_golden.npz) under the reference's
own criterion, closed forms of the classical magnitude responses that involve no other tool, the project's own literals (tests/sos_cases.py), window FIR
taps against the reference's data, the ``"s"`` domain of the coefficient types, and the analog responses through the host emulation of the response
kernels at the points i w."""
import os

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
import design_cases as dc
import response_cases as rc
import sos_cases as sc
from conftest import isapprox

EPS = dc.EPS


# ---- designs against the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_prototypes_equal_scipys(family):
    for n in dc.PROTOTYPE_ORDERS:
        f = dc.prototype(d, family, n, digital=False)
        assert isinstance(f, d.ZeroPoleGain) and f.domain == "s" and f.dtype == np.float64 and len(f.p) == n
        assert dc.zpkfilter_eq(f, dc.golden_zpk(f"ap_{family}_{n}")) == [], (family, n)


@pytest.mark.parametrize("band", list(dc.BANDS))
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_analog_and_digital_designs_equal_scipys(family, band):
    ftype = dc.response_type(d, band)
    for n in dc.DESIGN_ORDERS:
        proto = dc.prototype(d, family, n)
        dig = d.digitalfilter(ftype, proto)
        assert isinstance(dig, d.ZeroPoleGain) and dig.domain == "z"
        assert dc.zpkfilter_eq(dig, dc.golden_zpk(f"dig_{family}_{band}_{n}")) == [], (family, band, n)
        warped = d.prewarp(ftype, 2)
        edges = [warped.w] if band in ("lowpass", "highpass") else [warped.w1, warped.w2]
        assert np.allclose(edges, dc.golden()[f"ana_edges_{band}"], rtol=4 * EPS, atol=0)
        ana = d.analogfilter(warped, proto)
        assert isinstance(ana, d.ZeroPoleGain) and ana.domain == "s"
        assert dc.zpkfilter_eq(ana, dc.golden_zpk(f"ana_{family}_{band}_{n}")) == [], (family, band, n, "analog")
        # digitalfilter is bilinear(transform_prototype(prewarp(ftype, fs), proto), 2), and fs rescales the edges only
        again = d.bilinear(ana, 2)
        assert np.array_equal(again.z, dig.z) and np.array_equal(again.p, dig.p) and again.k == dig.k
        scaled = d.digitalfilter(type(ftype)(*(500 * np.atleast_1d(dc.BANDS[band]))), proto, fs=1000)
        assert dc.zpkfilter_eq(scaled, (dig.z, dig.p, dig.k)) == []


def test_element_type_of_the_prototypes():
    for make in (lambda *t: d.Butterworth(*t, 5), lambda *t: d.Chebyshev1(*t, 5, 1), lambda *t: d.Chebyshev2(*t, 5, 40), lambda *t: d.Elliptic(*t, 5, 0.5, 40)):
        f64, f32 = make(), make(np.float32)
        assert make(np.float64).dtype == f64.dtype == np.float64 and f64.kdtype == np.float64
        assert f32.dtype == np.float32 and f32.kdtype == np.float32 and f32.domain == "s"
        assert np.array_equal(f32.p, f64.p.astype(np.complex64).astype(np.complex128)) and f32.k == np.float32(f64.k)
        dig = d.digitalfilter(d.Lowpass(0.2), f32)
        assert dig.dtype == np.float32 and dig.kdtype == np.float32
        for bad in (np.float16, np.longdouble, np.int32, complex, "float64", 64):
            with pytest.raises(TypeError):
                make(bad)


def test_design_errors():
    """test/filter_design.jl:948-962 and the checks of design.jl:235-245, :278, :294, :310."""
    for bad in (lambda: d.Butterworth(0), lambda: d.Chebyshev1(0, 1), lambda: d.Chebyshev2(0, 1), lambda: d.Elliptic(0, 0.1, 0.5),
                lambda: d.Elliptic(2, 0.5, 0.1), lambda: d.Chebyshev1(2, -1), lambda: d.Chebyshev2(2, -1), lambda: d.Elliptic(2, 0.1, -0.5)):
        with pytest.raises(d.DomainError):
            bad()
    for T in (d.Bandpass, d.Bandstop, d.ComplexBandpass):
        with pytest.raises(d.ArgumentError, match="w1 must be less than w2"):
            T(2, 1)
        with pytest.raises(d.ArgumentError, match="w1 must be less than w2"):
            T(0.3, 0.3)
    proto = d.Butterworth(3)
    d.Lowpass(1.5), d.Highpass(-1), d.Bandpass(-1, 7)                                       # frequencies are checked at design time, not here
    for ftype in (d.Lowpass(1.0), d.Lowpass(0), d.Highpass(-0.1), d.Bandpass(0.1, 1.0), d.Bandstop(0.0, 0.5)):
        with pytest.raises(d.DomainError):
            d.digitalfilter(ftype, proto)
        with pytest.raises(d.DomainError):
            d.digitalfilter(ftype, d.FIRWindow(d.hamming(11)))
    d.digitalfilter(d.Lowpass(400), proto, fs=1000)
    with pytest.raises(d.DomainError):
        d.digitalfilter(d.Lowpass(500), proto, fs=1000)
    with pytest.raises(d.DomainError):
        d.digitalfilter(d.ComplexBandpass(0.5, 2.0), d.FIRWindow(d.hamming(11)))
    d.digitalfilter(d.ComplexBandpass(-0.5, 1.0), d.FIRWindow(d.hamming(11)))                # a negative edge is a frequency of a complex filter
    for bad in (lambda: d.iirnotch(0, 0.1), lambda: d.iirnotch(0.2, 1.0), lambda: d.iirnotch(600, 1, fs=1000)):
        with pytest.raises(d.DomainError):
            bad()
    with pytest.raises(TypeError):
        d.digitalfilter(d.ComplexBandpass(0.1, 0.2), proto)                                 # no prewarp method
    with pytest.raises(TypeError):
        d.digitalfilter(d.Lowpass(0.2), d.ZeroPoleGain(proto.z, proto.p, proto.k))          # a "z" filter is no prototype
    with pytest.raises(TypeError):
        d.bilinear(d.digitalfilter(d.Lowpass(0.2), proto), 2)
    with pytest.raises(TypeError):
        d.digitalfilter(0.2, proto)
    with pytest.raises(TypeError):
        d.Lowpass(0.2 + 0j)
    with pytest.raises(d.ArgumentError, match="must specify transitionwidth"):
        d.FIRWindow()
    with pytest.raises(d.ArgumentError, match="odd number of coefficients"):
        d.digitalfilter(d.Highpass(0.25), d.FIRWindow(d.hamming(128), scale=False))         # test/filter_design.jl:998
    with pytest.raises(d.ArgumentError, match="odd number of coefficients"):
        d.digitalfilter(d.Bandstop(0.1, 0.2), d.FIRWindow(d.hamming(128), scale=False), fs=1)   # :1045


def test_a_prototype_of_another_coefficient_type_is_converted_first():
    """design.jl:424-425, :445"""
    proto = d.Butterworth(4)
    want = d.digitalfilter(d.Lowpass(0.3), proto)
    for T in (d.PolynomialRatio, d.SecondOrderSections):
        got = d.digitalfilter(d.Lowpass(0.3), T(proto))
        assert dc.zpkfilter_eq(got, (want.z, want.p, want.k)) == [], T


def test_a_design_the_cascades_refuse_is_designed_and_still_refused():
    f = d.digitalfilter(d.Bandpass(0.2, 0.5), d.Butterworth(20))                            # 40 poles: 20 sections
    assert len(f.p) == 40 and len(d.SecondOrderSections(f).biquads) == 20
    with pytest.raises(d.UnsupportedError):
        d.filt(f, np.ones(8))
    with pytest.raises(d.UnsupportedError):                                                 # filt(b, a, x) with a vector a
        d.filt(d.PolynomialRatio(d.digitalfilter(d.Lowpass(0.2), d.Butterworth(2))), np.ones(8))


# ---- conventions and the project's own literals -----------------------------------------------------------------------------------------------------------
def _ulps(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)) / np.spacing(np.abs(np.asarray(want)))


def test_the_recipe_in_plain_numpy_reproduces_the_projects_literal():
    """Butterworth poles, pre-warping and the bilinear transform written out here, independent of the package: the literal ZPK_BUTTER5 of tests/sos_cases.py
    (typed in from scipy.signal.butter(5, 0.2, output="zpk")) follows the reference's conventions."""
    z, p, k = sc.ZPK_BUTTER5
    n, wn = 5, 0.2
    s = np.array([np.exp(1j * np.pi * (2 * i + n - 1) / (2 * n)) for i in range(1, n + 1)]) * 4 * np.tan(np.pi * wn / 2)
    pz = (2 + s / 2) / (2 - s / 2)
    kz = (4 * np.tan(np.pi * wn / 2)) ** n / np.real(np.prod(4 - s))
    assert np.max(np.abs(dc.sort_roots(pz) - dc.sort_roots(p))) <= 4 * EPS
    assert abs(kz - k) / k <= 4 * EPS
    assert np.array_equal(np.asarray(z), -np.ones(5))


def test_digitalfilter_equals_the_projects_literals():
    z, p, k = sc.ZPK_BUTTER5
    f = d.digitalfilter(d.Lowpass(0.2), d.Butterworth(5))
    assert np.array_equal(f.z, -np.ones(5))
    got, want = dc.sort_roots(f.p), dc.sort_roots(p)
    print("poles, ulp:", _ulps(got, want), "gain, ulp:", _ulps(f.k, k))
    assert np.all(_ulps(got, want) <= 4) and _ulps(f.k, k) <= 4
    # its sections have the poles of table butter5_02 (the order of the sections is the conversion's own: the table lists them as scipy cut them)
    sos = d.SecondOrderSections(f)
    tb, g = sc.table("butter5_02")
    assert len(sos.biquads) == 3 and sos.domain == "z" and _ulps(sos.g, g) <= 4
    got = sorted((float(q.a1), float(q.a2)) for q in sos.biquads)
    assert np.allclose(got, sorted((r[3], r[4]) for r in tb), rtol=0, atol=8 * EPS)
    assert sorted(len(np.flatnonzero(q.coefficients()[:3])) for q in sos.biquads) == [2, 3, 3]    # (1 + z^-1) once, (1 + z^-1)^2 twice


def test_iirnotch_equals_scipys_at_q_equal_w_over_bandwidth():
    g = dc.golden()
    q = d.iirnotch(0.2, 0.05)
    assert isinstance(q, d.Biquad) and q.domain == "z" and q.dtype == np.float64
    assert np.allclose([q.b0, q.b1, q.b2], g["iirnotch_b"], rtol=4 * EPS, atol=0)
    assert np.allclose([1.0, q.a1, q.a2], g["iirnotch_a"], rtol=4 * EPS, atol=0)
    q2 = d.iirnotch(100.0, 25.0, fs=1000)
    assert np.allclose(q2.coefficients(), q.coefficients(), rtol=4 * EPS, atol=0)
    assert q.b1 == q.a1 and q.b0 == q.b2                                                    # design.jl:538


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,ripple,n", [(f, r, n) for f, r in (("butter", None), ("cheby1", 1), ("cheby2", 40)) for n in (4, 5, 7)] + [("butter", None, 20)])
def test_magnitude_responses_meet_their_closed_forms(family, ripple, n):
    """64 eps absolute on |H|^2 <= 1 (the scipy designs of the fixture meet the first two forms to 1.6e-15 at n = 4, 5, 7).  Butterworth(20) at 0.5 is the
    design test/filter_design.jl:752-780 compares with MATLAB's; W^40 is as well conditioned as W^8.  The Chebyshev forms stop at n = 7: T_n(W) near
    W = 1 amplifies the rounding of W itself by n^2, so at n = 20 the closed form is no yardstick at 64 eps."""
    wn = 0.5 if n == 20 else 0.2
    proto = {"butter": lambda: d.Butterworth(n), "cheby1": lambda: d.Chebyshev1(n, ripple), "cheby2": lambda: d.Chebyshev2(n, ripple)}[family]()
    f = d.digitalfilter(d.Lowpass(wn), proto)
    w = dc.closed_form_grid()
    got = np.abs(dc.zpk_response(f.z, f.p, f.k, w)) ** 2
    err = np.max(np.abs(got - dc.closed_form_mag2(family, n, wn, w, ripple)))
    print(f"{family} n {n}: {err:.3e} = {err / EPS:.1f} eps")
    assert err <= 64 * EPS


def test_elliptic_ripples():
    """Elliptic(6, 0.5, 40) at 0.3: equiripple -0.5 dB in the pass band (its minimum is at the edge, a grid point) and -40 dB in the stop band (an even
    order ends at -40 dB at w = pi, a grid point); 1e-9 dB (the scipy design of the fixture meets both to 8e-14 dB)."""
    f = d.digitalfilter(d.Lowpass(0.3), d.Elliptic(6, 0.5, 40))
    w = np.linspace(0, np.pi, 20001)
    db = 20 * np.log10(np.abs(dc.zpk_response(f.z, f.p, f.k, w)))
    edge = 6000
    assert w[edge] == np.float64(0.3 * np.pi) or abs(w[edge] - 0.3 * np.pi) <= 2 * np.spacing(0.3 * np.pi)
    passband = db[:edge + 1]
    print(f"pass band min {passband.min() + 0.5:.3e} max {passband.max():.3e}")
    assert abs(passband.min() + 0.5) <= 1e-9
    assert passband.max() <= 1e-9
    first = edge + int(np.argmax(db[edge:] <= -40 + 1e-9))                                  # the stop band starts where the response first reaches -40 dB
    assert edge < first < len(w) - 1
    stopband = db[first:]
    print(f"stop band from w = {w[first] / np.pi:.4f} pi, max {stopband.max() + 40:.3e}")
    assert abs(stopband.max() + 40) <= 1e-9
    assert np.all(np.diff(db[edge:first + 1]) < 0)                                          # monotone through the transition band


# ---- window FIR designs -----------------------------------------------------------------------------------------------------------------------------------
def test_fir_window_taps_equal_the_references_data():
    """test/filter_design.jl:988-1080 (SciPy firwin)."""
    g = dc.golden()
    low = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsp_golden.npz"))
    for scaled, tag in ((False, ""), (True, "_scaled")):
        for n in (128, 129):
            taps = d.digitalfilter(d.Lowpass(0.25), d.FIRWindow(d.hamming(n), scale=scaled), fs=1)
            assert taps.dtype == np.float64 and isapprox(taps, low[f"digitalfilter_hamming_{n}_lowpass{tag}_fc0p25_fs1p0"]), (n, scaled)
            assert isapprox(taps, d.design.lowpass_firwindow(0.25, d.hamming(n), fs=1, scale=scaled))
            taps = d.digitalfilter(d.Bandpass(0.1, 0.2), d.FIRWindow(d.hamming(n), scale=scaled), fs=1)
            assert isapprox(taps, g[f"digitalfilter_hamming_{n}_bandpass{tag}_fc0p1_0p2_fs1p0"]), (n, scaled)
        taps = d.digitalfilter(d.Highpass(0.25), d.FIRWindow(d.hamming(129), scale=scaled), fs=1)
        assert isapprox(taps, g[f"digitalfilter_hamming_129_highpass{tag}_fc0p25_fs1p0"]), scaled
        taps = d.digitalfilter(d.Bandstop(0.1, 0.2), d.FIRWindow(d.hamming(129), scale=scaled), fs=1)
        assert isapprox(taps, g[f"digitalfilter_hamming_129_bandstop{tag}_fc0p1_0p2_fs1p0"]), scaled
    # the Kaiser form: the window of kaiserord
    fw = d.FIRWindow(transitionwidth=0.1, attenuation=60)
    assert fw.scale and np.array_equal(fw.window, d.kaiser(*d.kaiserord(0.1, 60)))
    assert not d.FIRWindow(d.hamming(5), False).scale


def test_complex_bandpass_taps():
    """design.jl:614-621, :659-667; test/filter_design.jl:1017-1043."""
    for (w1, w2, fs, n) in ((0.1, 0.2, 2, 128), (30, 40, 100, 511), (0.2, 0.6, 2, 65)):
        taps = d.digitalfilter(d.ComplexBandpass(w1, w2), d.FIRWindow(d.hamming(n)), fs=fs)
        assert taps.dtype == np.complex128 and taps.shape == (n,)
        f1, f2 = 2 * w1 / fs, 2 * w2 / fs
        centre = (f1 + f2) / 2
        k = np.arange(n)
        assert abs(abs(np.sum(taps * np.exp(-1j * np.pi * np.fmod(centre * k, 2.0)))) - 1) <= 64 * EPS    # unity at the band centre
        raw = d.digitalfilter(d.ComplexBandpass(w1, w2), d.FIRWindow(d.hamming(n), scale=False), fs=fs)
        proto = d.digitalfilter(d.Lowpass((f2 - f1) / 2), d.FIRWindow(d.hamming(n), scale=False))
        turn = np.exp(1j * np.pi * np.fmod(centre * k, 2.0))                                # cispi(w_center k): the product reduced before pi comes in
        assert isapprox(raw, proto * turn, rtol=64 * EPS)                                   # the real low-pass prototype turned to the band centre
        db = 20 * np.log10(np.abs(np.fft.fft(np.concatenate([taps, np.zeros(400)]))))
        f = 2.0 * np.arange(len(db)) / len(db)
        assert db[(f > f1) & (f < f2)].min() > -6.02 and db[~((f > f1) & (f < f2))].max() < -6.02


# ---- the "s" domain of the coefficient types ------------------------------------------------------------------------------------------------------------
def test_s_polynomial_ratio_keeps_its_coefficients():
    f = d.PolynomialRatio([2.0, 3.0, 4.0], [2.0, 3.0, 4.0, 5.0], domain="s")
    assert f.domain == "s" and np.array_equal(d.coefb(f), [2.0, 3.0, 4.0]) and np.array_equal(d.coefa(f), [2.0, 3.0, 4.0, 5.0])   # highest power first, a[0] kept
    assert d.PolynomialRatio([1, 2, 3], [2, 3, 4]).domain == "z" and np.array_equal(d.coefa(d.PolynomialRatio([1, 2, 3], [2, 3, 4])), [1.0, 1.5, 2.0])
    f = d.PolynomialRatio([0, 0, 1], [2, 10], domain="s")                                   # leading zeros are no coefficients
    assert np.array_equal(d.coefb(f), [1.0]) and np.array_equal(d.coefa(f), [2.0, 10.0]) and f.dtype == np.float64
    f = d.PolynomialRatio([1, 0], [1], domain="s")                                          # s
    assert np.array_equal(d.coefb(f), [1.0, 0.0]) and np.array_equal(d.coefa(f), [1.0])
    f = d.PolynomialRatio([1, 0, 0], [1, 2, 0], domain="s")                                 # a common factor s goes (coefficients.jl:87-89)
    assert np.array_equal(d.coefb(f), [1.0, 0.0]) and np.array_equal(d.coefa(f), [1.0, 2.0])
    assert d.PolynomialRatio(np.float32([1, 2]), np.float32([3]), domain="s").dtype == np.float32
    with pytest.raises(d.ArgumentError, match="filter must have non-zero denominator"):
        d.PolynomialRatio([1.0, 2.0], [0.0, 0.0], domain="s")
    with pytest.raises(d.ArgumentError, match="non-zero leading denominator coefficient"):
        d.PolynomialRatio([1.0, 2.0], [0.0, 1.0])                                           # "z": as before
    d.PolynomialRatio([1.0, 2.0], [0.0, 1.0], domain="s")
    with pytest.raises(d.UnsupportedError):
        d.PolynomialRatio([1.0 + 1j, 2.0], [1.0], domain="s")
    with pytest.raises(d.ArgumentError):
        d.PolynomialRatio([1.0], [1.0], domain="w")


def _value(f, x):
    """The transfer function of any coefficient object at the point x, from its own numbers."""
    if isinstance(f, d.PolynomialRatio):
        return np.polyval(f.b, x) / np.polyval(f.a, x)
    if isinstance(f, d.ZeroPoleGain):
        return f.k * np.prod(x - f.z) / np.prod(x - f.p)
    if isinstance(f, d.Biquad):
        return ((f.b0 * x + f.b1) * x + f.b2) / ((x + f.a1) * x + f.a2)
    return f.g * np.prod([_value(q, x) for q in f.biquads])


def test_s_conversions_keep_the_domain_and_the_function():
    x = 0.3 + 1.7j
    pr = d.PolynomialRatio([0.2, 0.3, 1.0], [1.0, 0.4, 1.0], domain="s")
    want = _value(pr, x)
    zpk, bq = d.ZeroPoleGain(pr), d.Biquad(pr)
    sos = d.SecondOrderSections(pr)
    for f in (zpk, bq, sos, d.PolynomialRatio(zpk), d.PolynomialRatio(bq), d.PolynomialRatio(sos), d.ZeroPoleGain(sos), d.ZeroPoleGain(bq),
              d.SecondOrderSections(zpk), d.SecondOrderSections(bq), d.Biquad(sos), d.Biquad(zpk), d.PolynomialRatio(pr), d.SecondOrderSections(sos),
              d.Biquad(bq), d.ZeroPoleGain(zpk)):
        assert f.domain == "s", type(f)
        assert abs(_value(f, x) - want) <= 1e-14 * abs(want), type(f)
    assert zpk.k == 0.2 and np.array_equal(d.coefa(bq), [1.0, 0.4, 1.0])
    # a fifth-order analog design through all three forms and back
    ana = d.analogfilter(d.Bandpass(0.5, 2.0), d.Chebyshev1(3, 1))
    want = _value(ana, x)
    for f in (d.PolynomialRatio(ana), d.SecondOrderSections(ana), d.ZeroPoleGain(d.PolynomialRatio(ana)), d.ZeroPoleGain(d.SecondOrderSections(ana)),
              d.SecondOrderSections(d.PolynomialRatio(ana)), d.PolynomialRatio(d.SecondOrderSections(ana))):
        assert f.domain == "s" and abs(_value(f, x) - want) <= 1e-10 * abs(want), type(f)
    assert len(d.SecondOrderSections(ana).biquads) == 3
    # the rational functions of test/filter_response.jl:141-160 that have no section form
    with pytest.raises(d.ArgumentError, match="leading denominator coefficient of a Biquad must be one"):
        d.Biquad(d.PolynomialRatio([0, 0, 1], [2, 10], domain="s"))
    with pytest.raises(d.ArgumentError):
        d.Biquad(d.PolynomialRatio([1, 0, 1], [2, 10], domain="s"))
    with pytest.raises(d.ArgumentError, match="more zeros than poles"):
        d.SecondOrderSections(d.PolynomialRatio([1, 0], [1], domain="s"))
    one_over_s = d.Biquad(d.PolynomialRatio([1], [1, 0], domain="s"))
    assert abs(_value(one_over_s, x) - 1 / x) <= 1e-15
    with pytest.raises(d.ArgumentError, match="length > 3"):
        d.Biquad(d.PolynomialRatio([1.0], [1.0, 2.0, 3.0, 4.0], domain="s"))


def test_domains_do_not_mix():
    qs, qz = d.Biquad(1.0, 2.0, 3.0, 4.0, 5.0, domain="s"), d.Biquad(1.0, 2.0, 3.0, 4.0, 5.0)
    assert qs.domain == "s" and qz.domain == "z" and d.Biquad(1.0, 2.0, 3.0, 2.0, 4.0, 5.0, 2.0, domain="s").domain == "s"
    assert d.SecondOrderSections([qs, qs], 2.0).domain == "s" and d.SecondOrderSections([qs], 2.0, domain="s").domain == "s"
    assert d.SecondOrderSections([qz], 2.0).domain == "z" and d.SecondOrderSections([], 2.0).domain == "z"
    assert d.ZeroPoleGain([1j, -1j], [-1.0], 2.0, domain="s").domain == "s" and d.ZeroPoleGain([1j, -1j], [-1.0], 2.0).domain == "z"
    for bad in (lambda: d.SecondOrderSections([qs, qz], 1.0), lambda: d.SecondOrderSections([qz], 1.0, domain="s"),
                lambda: d.SecondOrderSections([qs], 1.0, domain="z")):
        with pytest.raises(d.ArgumentError):
            bad()
    for T in (d.PolynomialRatio, d.ZeroPoleGain, d.Biquad, d.SecondOrderSections):           # a conversion between domains does not exist
        with pytest.raises(TypeError):
            T(qs, domain="z")
        with pytest.raises(TypeError):
            T(qz, domain="s")
        assert T(qs, domain="s").domain == "s" and T(qz).domain == "z"


def test_an_s_filter_does_not_filter():
    """filt, filt!, filtfilt, DF2TFilter, impresp, stepresp, filt_stepstate have {:z} methods only: TypeError, before any device work (no DeviceError on a
    machine without a device, no launch on one with)."""
    x = np.ones(16)
    q = d.Biquad(1.0, 0.5, 0.25, 0.1, 0.2, domain="s")
    filters = (q, d.SecondOrderSections([q], 1.0), d.ZeroPoleGain(q), d.PolynomialRatio(q), d.Butterworth(3), d.PolynomialRatio([1.0, 2.0], [1.0], domain="s"))
    for f in filters:
        for call in (lambda: d.filt(f, x), lambda: d.filt_(np.empty(16), f, x), lambda: d.filtfilt(f, x), lambda: d.DF2TFilter(f),
                     lambda: d.impresp(f), lambda: d.stepresp(f, 10)):
            with pytest.raises(TypeError):
                call()
    with pytest.raises(TypeError):
        d.filt_stepstate(d.SecondOrderSections([q], 1.0))
    if _lib.device_count() == 0:                                                            # the responses of an "s" filter do run on the device
        for f in filters:
            for fn in (d.freqresp, d.phaseresp, d.grpdelay):
                with pytest.raises(d.DeviceError):
                    fn(f, np.ones(3))


# ---- analog responses through the host emulation ----------------------------------------------------------------------------------------------------------
def test_analog_rational_functions_through_the_emulation():
    """test/filter_response.jl:140-161."""
    w = dc.freqs_w()
    s = 1j * w
    for b, a, H in (([1, 0], [1], s), ([1], [1, 0], 1 / s), ([0, 0, 1], [2, 10], 1 / (2 * s + 10)), ([1, 0, 1], [2, 10], (1 - w ** 2) / (2 * s + 10))):
        pr = d.PolynomialRatio(b, a, domain="s")
        assert isapprox(dc.emulated_analog_freqresp(pr, w), H), (b, a)
        assert isapprox(dc.emulated_analog_freqresp(d.ZeroPoleGain(pr), w), H), (b, a)
        proper = len(np.trim_zeros(b, "f")) <= len(a)
        if proper and a[0] == 1:
            assert isapprox(dc.emulated_analog_freqresp(d.Biquad(pr), w), H), (b, a)
        if proper:
            assert isapprox(dc.emulated_analog_freqresp(d.SecondOrderSections(pr), w), H), (b, a)


def test_freqs_eg1_through_the_emulation():
    """test/filter_response.jl:164-186: MATLAB's freqs."""
    eg = dc.golden()["freqs_eg1"]
    w = dc.freqs_w()
    assert isapprox(w, eg[:, 0])
    pr = d.PolynomialRatio(dc.FREQS_B, dc.FREQS_A, domain="s")
    h = dc.emulated_analog_freqresp(pr, w)
    assert isapprox(h, np.polyval(dc.FREQS_B, 1j * w) / np.polyval(dc.FREQS_A, 1j * w))
    assert isapprox(np.abs(h), eg[:, 1])
    phi = np.unwrap(dc.emulated_analog_freqresp(pr, w, out_mode=rc.ANGLE))
    assert isapprox(180 / np.pi * phi, eg[:, 2])
    assert isapprox(h, dc.emulated_analog_freqresp(d.ZeroPoleGain(pr), w))
    assert isapprox(h, dc.emulated_analog_freqresp(d.SecondOrderSections(pr), w))
    assert isapprox(h, dc.emulated_analog_freqresp(d.Biquad(pr), w))
    w32 = w.astype(np.float32)
    h32 = dc.emulated_analog_freqresp(d.PolynomialRatio(np.float32(dc.FREQS_B), np.float32(dc.FREQS_A), domain="s"), w32)
    assert h32.dtype == np.complex64 and isapprox(h32, h, rtol=np.sqrt(np.finfo(np.float32).eps))


def test_analog_group_delays_through_the_emulation():
    """test/filter_response.jl:228-231 at the frequencies of grpdelay_eg1."""
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "response_golden.npz"))["grpdelay_eg1"][:, 0]
    for b, a, tau in dc.ANALOG_GRPDELAY:
        pr = d.PolynomialRatio(b, a, domain="s")
        assert isapprox(dc.emulated_analog_grpdelay(d, pr, w), tau(w)), (b, a)
        assert isapprox(dc.emulated_analog_grpdelay(d, d.ZeroPoleGain(pr), w), tau(w)), (b, a)


def test_default_frequencies_of_an_analog_filter():
    """response.jl:159-175, test/filter_response.jl:232-240."""
    from dsp_jl_amd.response import _freqrange
    assert np.array_equal(_freqrange(d.PolynomialRatio([1.0, 2.0], [1.0])), np.linspace(0, np.pi, 257))
    w = _freqrange(d.PolynomialRatio([1, 2], [123], domain="s"))
    assert len(w) == 200 and w.min() < 2 < w.max() and np.isclose(w[0], 0.2) and np.isclose(w[-1], 20.0)
    w = _freqrange(d.PolynomialRatio([1, 2], [3, 9], domain="s"))
    assert w.min() < 2 and 3 < w.max() and np.isclose(w[0], 0.2) and np.isclose(w[-1], 30.0)
    w = _freqrange(d.PolynomialRatio([1, 0], [1, 2], domain="s"))                           # a zero at 0 puts w = 0 in front
    assert len(w) == 201 and w[0] == 0 and np.isclose(w[1], 0.2)
    assert np.array_equal(_freqrange(d.PolynomialRatio([5.0], [1.0], domain="s")), [0.0, 1.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6])
    w = _freqrange(d.PolynomialRatio([4.0], [1.0, 0.0], domain="s"))                        # 4 / s: up to ten times where |H| = 1
    assert len(w) == 200 and w[0] == 0 and w[-1] == 40.0
