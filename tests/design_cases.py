"""What the filter-design tests share: the fixture, the reference's comparison of two zero-pole-gain filters, the closed forms of the classical
magnitude responses, and the analog responses through the host emulation of the response kernels.  Nothing here is the code under test except where a
function says so."""
import functools
import os

import numpy as np

import response_cases as rc
from conftest import isapprox

BANDS = {"lowpass": 0.2, "highpass": 0.3, "bandpass": (0.1, 0.4), "bandstop": (0.25, 0.35)}
FAMILIES = ("butter", "cheby1", "cheby2", "ellip")
PROTOTYPE_ORDERS = (1, 2, 5, 8)
DESIGN_ORDERS = (4, 7)
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "design_golden.npz")))


def golden_zpk(name):
    g = golden()
    return g[name + "_z"], g[name + "_p"], float(g[name + "_k"])


def response_type(d, band):
    wn = BANDS[band]
    return {"lowpass": d.Lowpass, "highpass": d.Highpass, "bandpass": d.Bandpass, "bandstop": d.Bandstop}[band](*np.atleast_1d(wn))


def prototype(d, family, n, digital=True):
    """The prototype behind a fixture entry: 1 dB Chebyshev I ripple, (0.5, 40) dB elliptic; Chebyshev II 1 dB as a bare prototype, 40 dB in a design."""
    if family == "butter":
        return d.Butterworth(n)
    if family == "cheby1":
        return d.Chebyshev1(n, 1)
    if family == "cheby2":
        return d.Chebyshev2(n, 40 if digital else 1)
    return d.Elliptic(n, 0.5, 40)


def _lt(a, b):
    """``lt`` of test/FilterTestHelpers.jl:10-16."""
    if abs(a.real - b.real) > 1e-10:
        return -1 if a.real < b.real else 1
    return -1 if a.imag < b.imag else (1 if a.imag > b.imag else 0)


def sort_roots(v):
    return np.array(sorted(np.atleast_1d(np.asarray(v, dtype=np.complex128)).tolist(), key=functools.cmp_to_key(_lt)), dtype=np.complex128)


def zpkfilter_eq(f, zpk):
    """``zpkfilter_eq`` of test/FilterTestHelpers.jl:25-31: sorted zeros and poles and the gain, each norm-wise at rtol sqrt(eps(Float64)).  Returns the
    list of what differs (empty: equal)."""
    z, p, k = zpk
    bad = []
    if len(f.z) or len(z):
        if not isapprox(sort_roots(f.z), sort_roots(z)):
            bad.append("z")
    if not isapprox(sort_roots(f.p), sort_roots(p)):
        bad.append("p")
    if not isapprox(np.float64(f.k), np.float64(k)):
        bad.append("k")
    return bad


def zpk_response(z, p, k, w):
    """H(e^{iw}) of a digital zero-pole-gain filter in numpy Float64: k prod(x - z) / prod(x - p)."""
    x = np.exp(1j * np.asarray(w, dtype=np.float64))
    num = np.prod(x[:, None] - np.asarray(z, np.complex128)[None, :], axis=1) if len(z) else np.ones_like(x)
    den = np.prod(x[:, None] - np.asarray(p, np.complex128)[None, :], axis=1)
    return k * num / den


def _cheb_t(n, x):
    """T_n(x) for real x."""
    x = np.asarray(x, dtype=np.float64)
    inside = np.abs(x) <= 1
    xi = np.where(inside, x, 0.0)
    xo = np.where(inside, 1.0, np.abs(x))
    return np.where(inside, np.cos(n * np.arccos(xi)), np.cosh(n * np.arccosh(xo)) * np.where((x < 0) & (n % 2 == 1), -1.0, 1.0))


def closed_form_mag2(family, n, wn, w, ripple=None):
    """|H(e^{iw})|^2 of the bilinear low-pass designs with cut-off wn (half-cycles per sample), no design tool involved:
    butter 1 / (1 + W^2n), cheby1 1 / (1 + e^2 T_n^2(W)), cheby2 1 / (1 + 1 / (e^2 T_n^2(1 / W))), W = tan(w / 2) / tan(pi wn / 2)."""
    W = np.tan(np.asarray(w, np.float64) / 2) / np.tan(np.pi * wn / 2)
    if family == "butter":
        return 1 / (1 + W ** (2 * n))
    if family == "cheby1":
        return 1 / (1 + (10 ** (ripple / 10) - 1) * _cheb_t(n, W) ** 2)
    if family == "cheby2":
        return 1 / (1 + 1 / (_cheb_t(n, 1 / W) ** 2 / (10 ** (ripple / 10) - 1)))
    raise ValueError(family)


def closed_form_grid(nw=200):
    return np.linspace(0.01, 3.1, nw)


def analog_points(w, R=np.float64):
    """The points i w as the library forms them: real part zero, imaginary part w in the working type."""
    w = np.asarray(w, dtype=R)
    pts = np.zeros(w.shape, dtype=rc.ctype(R))
    pts.imag = w
    return pts


def emulated_analog_freqresp(f, w, out_mode=rc.COMPLEX):
    """freqresp / angle of an ``"s"`` filter on the host: the form and the arrays the public function hands to its plan (dsp.jl_amd/response.py, the code
    under test), evaluated by mdsp_resp_emulate_host at the points i w -- in POINTS mode the device computes the same bits."""
    from dsp_jl_amd import response as resp
    w = np.asarray(w)
    R = np.dtype(np.float32) if w.dtype == np.float32 else np.dtype(np.float64)
    assert resp._in_mode(f) == rc.POINTS
    form, Rf, num, den, gain, flags = resp._form_of(f, R)
    return rc.emulate(form, Rf, num, den, analog_points(w, Rf), gain=gain, flags=flags, out_mode=out_mode)


def emulated_analog_grpdelay(d, f, w):
    from dsp_jl_amd import response as resp
    num, den = resp._analog_grpdelay_polys(d.coefb(f), d.coefa(f))
    return rc.emulate(rc.POLY, np.float64, num, den, analog_points(w), out_mode=rc.REAL_MINUS, cminus=0.0)


# test/filter_response.jl:229-231: (b, a, closed form of the group delay)
ANALOG_GRPDELAY = (
    ([1, 2], [123], lambda w: 0.5 / (1 + w ** 2 / 4)),
    ([123], [1, 2], lambda w: -0.5 / (1 + w ** 2 / 4)),
    ([1, 2], [3, 9], lambda w: 0.5 / (1 + w ** 2 / 4) - 1 / 3 / (1 + w ** 2 / 9)),
)

# test/filter_response.jl:164-165, the filter of freqs-eg1
FREQS_B, FREQS_A = [0.2, 0.3, 1.0], [1.0, 0.4, 1.0]


def freqs_w():
    return 10.0 ** np.linspace(-1, 1, 50)
