"""Designed filters on the device: cascades from ``digitalfilter`` through filt, filtfilt and DF2TFilter against the long-double restatement of the same
designed sections (tests/sos_ref.py) under the bound of tests/test_sos_cpu.py, an ``iirnotch`` on the tone it removes, window FIR designs against
numpy's convolution at the bars of tests/test_gpu_complex_taps.py, the device responses of digital designs against their closed forms, and the analog
(``"s"``) responses: bit for bit the host emulation at the points i w, the reference's MATLAB data and closed-form group delays at its own tolerance."""
import os

import numpy as np
import pytest

import design_cases as dc
import response_cases as rc
import sos_cases as sc
import sos_ref as sr
from conftest import isapprox, relerr

pytestmark = pytest.mark.gpu

C_BOUND = 8.0          # tests/test_sos_cpu.py: twice the worst measured e_scan / e_serial, rounded up to a power of two
TOL64 = 1e-12          # tests/test_gpu_complex_taps.py (tests/test_gpu_parity.py): norm-wise, Float64 results
N = 3 * 1024 + 5       # three tiles plus five samples: the smallest shape that crosses tile seams
EPS = dc.EPS


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


DESIGNS = {
    "butter5_low": lambda d: d.digitalfilter(d.Lowpass(0.2), d.Butterworth(5)),
    "ellip6_low": lambda d: d.digitalfilter(d.Lowpass(0.3), d.Elliptic(6, 0.5, 40)),
    "cheby1_4_band": lambda d: d.digitalfilter(d.Bandpass(0.1, 0.4), d.Chebyshev1(4, 1)),
}


def _typed(d, sos, dt):
    """The designed cascade with its coefficients held in ``dt``."""
    t = np.dtype(dt).type
    return d.SecondOrderSections([d.Biquad(*(t(v) for v in row)) for row in sos.table()], t(sos.g))


@pytest.fixture(scope="module")
def refs(d):
    """Per design and real type, computed once: (the design, its cascade in that type, x, the long-double restatement, e_serial)."""
    out = {}
    for name, make in DESIGNS.items():
        f = make(d)
        sos = d.SecondOrderSections(f)
        for dt in (np.float32, np.float64):
            typed = _typed(d, sos, dt)
            tb, g = typed.table(), float(typed.g)
            x = sc.signal(N, 2, dt)
            ref, _ = sr.sos_filt(tb, g, x, np.longdouble)
            ser, _ = sr.sos_filt(tb, g, x, dt)
            out[name, np.dtype(dt).name] = (f, typed, x, ref, sr.rel_err(ser, ref))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("name", list(DESIGNS))
def test_filt_of_a_designed_cascade(d, refs, name, dt):
    f, typed, x, ref, e_serial = refs[name, np.dtype(dt).name]
    y = d.filt(typed, x)
    assert y.dtype == np.dtype(dt) and y.shape == x.shape
    e = sr.rel_err(y, ref)
    print(f"{name} {np.dtype(dt).name}: e {e:.3e} e_serial {e_serial:.3e} ratio {e / e_serial:.2f}")
    assert e <= C_BOUND * e_serial
    if np.dtype(dt) == np.float64:                                       # the design itself, as a user passes it: converted to the same sections first
        assert np.array_equal(d.filt(f, x), y)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_df2tfilter_and_filtfilt_of_a_designed_cascade(d, refs, dt):
    f, typed, x, ref, e_serial = refs["butter5_low", np.dtype(dt).name]
    sf = d.DF2TFilter(typed, coldims=(2,))
    y = np.concatenate([sf.filt(x[:1000]), sf.filt(x[1000:])])
    assert y.dtype == np.dtype(dt) and sr.rel_err(y, ref) <= C_BOUND * e_serial
    tb, g = typed.table(), float(typed.g)
    want = sr.sos_filtfilt(tb, g, x, np.longdouble, coef_dtype=dt)
    e_ff = max(sr.rel_err(sr.sos_filtfilt(tb, g, x, dt, coef_dtype=dt), want), float(np.finfo(dt).eps))
    got = d.filtfilt(typed, x)
    print(f"filtfilt {np.dtype(dt).name}: e {sr.rel_err(got, want):.3e} e_serial {e_ff:.3e}")
    assert got.dtype == np.dtype(dt) and sr.rel_err(got, want) <= C_BOUND * e_ff


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_iirnotch_removes_its_tone(d, dt):
    """A unit sinusoid at the notch: what is left after the transient (|pole|^3072 < 1e-100) is the rounding of the coefficients and of the arithmetic
    (8.5e-14 in Float64, 5e-7 in Float32), next to nothing of the signal, so the rms of the last 1024 outputs is compared on the scale of the input, 1:
    |rms - rms_ld| <= C_BOUND max(|rms_serial - rms_ld|, eps)."""
    t = np.dtype(dt).type
    q = d.iirnotch(0.2, 0.05)
    q = d.Biquad(*(t(v) for v in q.coefficients()))
    row = np.array([[float(v) for v in q.coefficients()]])
    x = np.sin(np.pi * 0.2 * np.arange(4096)).astype(dt)
    rms = lambda v: float(np.sqrt(np.mean(np.asarray(v[-1024:], np.longdouble) ** 2)))
    ref, _ = sr.sos_filt(row, 1.0, x, np.longdouble, has_gain=False)
    ser, _ = sr.sos_filt(row, 1.0, x, dt, has_gain=False)
    y = d.filt(q, x)
    print(f"notch {np.dtype(dt).name}: rms {rms(y):.3e} serial {rms(ser):.3e} long double {rms(ref):.3e}")
    assert y.dtype == np.dtype(dt)
    assert abs(rms(y) - rms(ref)) <= C_BOUND * max(abs(rms(ser) - rms(ref)), float(np.finfo(dt).eps))
    assert rms(x) > 0.7 and rms(y[:1024]) > 1e-3                         # the tone is there, and so is the transient


def test_fir_window_designs_filter(d):
    x = sc.signal(2000, 1, np.float64)
    hp = d.digitalfilter(d.Highpass(0.25), d.FIRWindow(d.hamming(129)))                     # 129 real taps: overlap-save
    y = d.filt(hp, x)
    assert y.dtype == np.float64 and relerr(y, np.convolve(x, hp)[:2000]) < TOL64
    cb = d.digitalfilter(d.ComplexBandpass(0.2, 0.6), d.FIRWindow(d.hamming(65)))           # 65 complex taps: time domain
    y = d.filt(cb, x)
    assert y.dtype == np.complex128 and relerr(y, np.convolve(x, cb)[:2000]) < TOL64


@pytest.mark.parametrize("family,n,ripple", [("butter", 5, None), ("cheby1", 4, 1)])
def test_device_response_of_a_design_meets_the_closed_form(d, family, n, ripple):
    """nw = 65: one tile of lanes plus one.  The tolerance is 16 times what numpy's Float64 evaluation of the same z, p, k deviates from the closed form on
    the same grid (four bits for the device's other product order and its sincos), at least 64 eps."""
    f = d.digitalfilter(d.Lowpass(0.2), d.Butterworth(n) if family == "butter" else d.Chebyshev1(n, ripple))
    w = dc.closed_form_grid(65)
    want = dc.closed_form_mag2(family, n, 0.2, w, ripple)
    e_numpy = np.max(np.abs(np.abs(dc.zpk_response(f.z, f.p, f.k, w)) ** 2 - want))
    tol = max(16 * e_numpy, 64 * EPS)
    for form in (f, d.SecondOrderSections(f)):
        h = d.freqresp(form, w)
        assert h.dtype == np.complex128 and h.shape == (65,)
        e = np.max(np.abs(np.abs(h) ** 2 - want))
        print(f"{family} {type(form).__name__}: device {e:.3e} numpy {e_numpy:.3e} tolerance {tol:.3e}")
        assert e <= tol


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("nw", [50, 65])
def test_analog_freqresp_equals_the_host_emulation_bit_for_bit(d, nw):
    """The stated property of POINTS mode, through the public functions."""
    w = 10.0 ** np.linspace(-1, 1, nw)
    pr = d.PolynomialRatio(dc.FREQS_B, dc.FREQS_A, domain="s")
    ana = d.analogfilter(d.Bandpass(0.5, 2.0), d.Chebyshev1(3, 1))
    filters = [pr, d.ZeroPoleGain(pr), d.SecondOrderSections(pr), d.Biquad(pr), ana, d.SecondOrderSections(ana), d.PolynomialRatio(ana),
               d.PolynomialRatio([1, 2], [123], domain="s"), d.PolynomialRatio([1, 0], [1], domain="s")]
    for f in filters:
        got = d.freqresp(f, w)
        assert got.dtype == np.complex128 and got.shape == (nw,)
        assert np.array_equal(_bits(got), _bits(dc.emulated_analog_freqresp(f, w))), type(f)
        tau = d.grpdelay(f, w)
        assert tau.dtype == np.float64 and np.array_equal(_bits(tau), _bits(dc.emulated_analog_grpdelay(d, f, w))), type(f)
    w32 = w.astype(np.float32)
    pr32 = d.PolynomialRatio(np.float32(dc.FREQS_B), np.float32(dc.FREQS_A), domain="s")
    for f in (pr32, d.ZeroPoleGain(pr32), d.SecondOrderSections(pr32)):
        got = d.freqresp(f, w32)
        assert got.dtype == np.complex64 and np.array_equal(_bits(got), _bits(dc.emulated_analog_freqresp(f, w32))), type(f)


def test_analog_responses_against_the_references_data(d):
    """test/filter_response.jl:164-186 (MATLAB's freqs) and :228-240 (closed-form group delays)."""
    import torch
    eg = dc.golden()["freqs_eg1"]
    w = dc.freqs_w()
    pr = d.PolynomialRatio(dc.FREQS_B, dc.FREQS_A, domain="s")
    for f in (pr, d.ZeroPoleGain(pr), d.SecondOrderSections(pr), d.Biquad(pr)):
        assert isapprox(np.abs(d.freqresp(f, w)), eg[:, 1]), type(f)
        assert isapprox(180 / np.pi * d.phaseresp(f, w), eg[:, 2]), type(f)
    wg = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "response_golden.npz"))["grpdelay_eg1"][:, 0]
    for b, a, tau in dc.ANALOG_GRPDELAY:
        f = d.PolynomialRatio(b, a, domain="s")
        assert isapprox(d.grpdelay(f, wg), tau(wg)), (b, a)
        got, wdef = d.grpdelay(f)                                        # the default frequencies cover the pole and the zero
        assert isapprox(got, tau(wdef)) and wdef.min() < 2 < wdef.max()
    h, wdef = d.freqresp(pr)
    assert len(wdef) == 200 and np.array_equal(h, d.freqresp(pr, wdef))
    # a device tensor w gives a device tensor
    wd = torch.from_numpy(w).cuda()
    for fn in (d.freqresp, d.phaseresp, d.grpdelay):
        dev = fn(pr, wd)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == (50,)
        assert np.array_equal(dev.cpu().numpy(), fn(pr, w))
    assert torch.equal(wd, torch.from_numpy(w).cuda())
    w2 = w.reshape(5, 10)
    assert d.freqresp(pr, w2).shape == (5, 10) and np.array_equal(d.freqresp(pr, w2).ravel(), d.freqresp(pr, w))
