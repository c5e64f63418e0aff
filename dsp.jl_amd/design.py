"""Filter design of DSP.jl ``src/Filters/design.jl``: host arithmetic in Float64, O(order) per design.

The FIR tap generators the hot path needs as *inputs* (``kaiserord``, ``lowpass_firwindow``, ``resample_filter``), and the designs a user filters with:
the analog prototypes ``Butterworth``, ``Chebyshev1``, ``Chebyshev2``, ``Elliptic`` (``ZeroPoleGain`` in the ``"s"`` domain), the response types
``Lowpass``, ``Highpass``, ``Bandpass``, ``Bandstop``, ``ComplexBandpass``, ``analogfilter``, ``bilinear``, ``prewarp``, ``digitalfilter`` for a prototype
(a ``"z"`` ``ZeroPoleGain``) and for a ``FIRWindow`` (a tap vector), and ``iirnotch``.  What filters with a design -- ``filt``, ``filtfilt``, ``DF2TFilter``,
``freqresp`` ... -- runs on the device; nothing here does.
"""
from __future__ import annotations

import cmath
import functools
import math
import numbers
from fractions import Fraction

import numpy as np

from . import windows
from ._lib import ArgumentError, DomainError
from .coefficients import Biquad, FilterCoefficients, ZeroPoleGain


def kaiserord(transitionwidth, attenuation=60):
    """design.jl:547-559 -> (n, alpha)."""
    n = int(math.ceil((attenuation - 7.95) / (math.pi * 2.285 * transitionwidth))) + 1
    if attenuation > 50:
        beta = 0.1102 * (attenuation - 8.7)
    elif attenuation >= 21:
        beta = 0.5842 * (attenuation - 21) ** 0.4 + 0.07886 * (attenuation - 21)
    else:
        beta = 0.0
    return n, beta / math.pi


def lowpass_firwindow(w, window, fs=2, scale=True) -> np.ndarray:
    """``digitalfilter(Lowpass(w), FIRWindow(window; scale); fs)`` (design.jl:235-240, :598-602, :642, :669-674)."""
    if w <= 0:
        raise DomainError("frequencies must be positive")
    f = 2 * w / fs
    if f >= 1:
        raise DomainError("frequencies must be less than the Nyquist frequency")
    window = np.asarray(window, dtype=np.float64)
    n = len(window)
    k = np.arange(1, n + 1)
    taps = f * np.sinc(f * (k - (n + 1) / 2)) * window
    return taps / taps.sum() if scale else taps


def resample_filter(rate, *args) -> np.ndarray:
    """design.jl:683-720.  Rational/integer ``rate`` -> (rel_bw=1.0, attenuation=60); float -> (Nphi=32, rel_bw, att).
    The design (a Kaiser window of a few thousand points) is memoised per argument tuple: ``resample(x, rate)`` redesigns the same
    filter on every call."""
    try:
        return _resample_filter_cached(rate if isinstance(rate, float) else Fraction(rate), tuple(args)).copy()
    except TypeError:           # unhashable argument: design without the memo
        return _resample_filter(rate, *args)


@functools.lru_cache(maxsize=32)
def _resample_filter_cached(rate, args):
    return _resample_filter(rate, *args)


def _resample_filter(rate, *args) -> np.ndarray:
    if isinstance(rate, float):
        nphi = int(args[0]) if len(args) > 0 else 32
        rel_bw = args[1] if len(args) > 1 else 1.0
        att = args[2] if len(args) > 2 else 60
        f_nyq = 1.0 / nphi if rate >= 1.0 else rate / nphi
    else:
        r = Fraction(rate)
        nphi = r.numerator
        rel_bw = args[0] if len(args) > 0 else 1.0
        att = args[1] if len(args) > 1 else 60
        f_nyq = min(1 / nphi, 1 / r.denominator)
    cutoff = f_nyq * rel_bw
    hlen, alpha = kaiserord(cutoff * 0.2, att)
    hlen = nphi * int(math.ceil(hlen / nphi))
    if hlen % 2 == 0:
        hlen += 1
    return lowpass_firwindow(cutoff, windows.kaiser(hlen, alpha)) * nphi


# ---- sinpi / cospi --------------------------------------------------------------------------------------------------------------------------------
def _sincospi(x):
    """(sin(pi x), cos(pi x)) of real x (scalar or array) as the reference's ``sincospi``: the argument is reduced exactly to [-1/4, 1/4] first, so
    multiples of 1/2 give exact zeros and ones."""
    x = np.asarray(x, dtype=np.float64)
    r = np.fmod(np.abs(x), 2.0)                                          # exact
    q = np.rint(2.0 * r)
    t = r - q / 2.0                                                      # exact, in [-1/4, 1/4]
    s, c = np.sin(np.pi * t), np.cos(np.pi * t)
    q = q.astype(np.int64) % 4
    sn = np.choose(q, [s, c, -s, -c]) * np.where(np.signbit(x), -1.0, 1.0)
    cs = np.choose(q, [c, -s, -c, s])
    return (float(sn), float(cs)) if sn.ndim == 0 else (sn, cs)


def _sinpi(u):
    """``sinpi`` of a real or complex scalar."""
    u = complex(u)
    s, c = _sincospi(u.real)
    return s if u.imag == 0 else complex(s * math.cosh(math.pi * u.imag), c * math.sinh(math.pi * u.imag))


def _cospi(u):
    """``cospi`` of a real or complex scalar."""
    u = complex(u)
    s, c = _sincospi(u.real)
    return c if u.imag == 0 else complex(c * math.cosh(math.pi * u.imag), -s * math.sinh(math.pi * u.imag))


def _tanpi(x):
    s, c = _sincospi(x)
    return s / c


def _abs2(v):
    v = complex(v)
    return v.real * v.real + v.imag * v.imag


# ---- prototypes (design.jl:11-228) ----------------------------------------------------------------------------------------------------------------
def _proto_args(name, args, nargs):
    """``Butterworth(n)`` / ``Butterworth(T, n)``: (element type, the remaining arguments).  T is Float32 or Float64."""
    T = np.dtype(np.float64)
    if len(args) == nargs + 1:
        if not (isinstance(args[0], (type, np.dtype)) and np.dtype(args[0]) in (np.dtype(np.float32), np.dtype(np.float64))):
            raise TypeError(f"{name}: the element type must be numpy.float32 or numpy.float64, got {args[0]!r}")
        T, args = np.dtype(args[0]), args[1:]
    if len(args) != nargs:
        raise TypeError(f"{name} takes {nargs} argument{'s' if nargs > 1 else ''} after an optional element type")
    n = args[0]
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"{name}: n must be an integer")
    for v in args[1:]:
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise TypeError(f"{name}: the ripples must be real numbers")
    return T, (int(n),) + tuple(float(v) for v in args[1:])


def _proto(T, z, p, k):
    """``ZeroPoleGain{:s}(z, p, k)`` with element type T: the Float64 results rounded once to T."""
    C = np.complex64 if T == np.dtype(np.float32) else np.complex128
    return ZeroPoleGain(np.array(z, dtype=C), np.array(p, dtype=C), T.type(k), domain="s")


def Butterworth(*args):
    """``Butterworth([T,] n)``: ``n`` pole Butterworth prototype (design.jl:11-33)."""
    T, (n,) = _proto_args("Butterworth", args, 1)
    if n <= 0:
        raise DomainError(f"n must be positive, got {n}")
    poles = [0j] * n
    for i in range(1, n // 2 + 1):
        s, c = _sincospi((2 * i - 1) / (2 * n))
        poles[2 * i - 2] = complex(-s, c)
        poles[2 * i - 1] = complex(-s, -c)
    if n % 2:
        poles[-1] = complex(-1.0, 0.0)
    return _proto(T, [], poles, 1.0)


def _chebyshev_poles(n, eps):
    """design.jl:39-57"""
    p = [0j] * n
    mu = math.asinh(1.0 / eps) / n
    b, c = -math.sinh(mu), math.cosh(mu)
    for i in range(1, n // 2 + 1):
        sw, cw = _sincospi((2 * i - 1) / (2 * n))
        p[2 * i - 2] = complex(b * sw, c * cw)
        p[2 * i - 1] = complex(b * sw, -(c * cw))
    if n % 2:
        p[-1] = complex(b * _sincospi((2 * (n // 2) + 1) / (2 * n))[0], 0.0)
    return p


def Chebyshev1(*args):
    """``Chebyshev1([T,] n, ripple)``: ``n`` pole Chebyshev type I prototype with ``ripple`` dB ripple in the passband (design.jl:59-83)."""
    T, (n, ripple) = _proto_args("Chebyshev1", args, 2)
    if n <= 0:
        raise DomainError(f"n must be positive, got {n}")
    if not ripple >= 0:
        raise DomainError(f"ripple must be non-negative, got {ripple}")
    eps = math.sqrt(10.0 ** (ripple / 10) - 1)
    p = _chebyshev_poles(n, eps)
    k = 1.0
    for i in range(1, n // 2 + 1):
        k *= _abs2(p[2 * i - 1])
    if n % 2 == 0:
        k /= math.sqrt(1 + eps * eps)
    else:
        k *= -p[-1].real
    return _proto(T, [], p, k)


def Chebyshev2(*args):
    """``Chebyshev2([T,] n, ripple)``: ``n`` pole Chebyshev type II prototype with ``ripple`` dB ripple in the stopband (design.jl:85-113)."""
    T, (n, ripple) = _proto_args("Chebyshev2", args, 2)
    if n <= 0:
        raise DomainError(f"n must be positive, got {n}")
    if not ripple >= 0:
        raise DomainError(f"ripple must be non-negative, got {ripple}")
    eps = 1 / math.sqrt(10.0 ** (ripple / 10) - 1)
    p = [1 / v for v in _chebyshev_poles(n, eps)]
    z = [0j] * (n - n % 2)
    k = 1.0
    for i in range(1, n // 2 + 1):
        ze = complex(0.0, -1 / _sincospi((2 * i - 1) / (2 * n))[1])
        z[2 * i - 2] = ze
        z[2 * i - 1] = ze.conjugate()
        k *= _abs2(p[2 * i - 1]) / _abs2(ze)
    if n % 2:
        k *= -p[-1].real
    return _proto(T, z, p, k)


def _landen(k):
    """The Landen sequence for the evaluation of elliptic functions, Orfanidis eq. (50) (design.jl:122-130)."""
    kn = []
    for _ in range(7):
        k = (k / (1 + math.sqrt(1 - k * k))) ** 2
        kn.append(k)
    return kn


def _ellip(init, landen):
    """design.jl:135-142, eq. (55): cd(u K, k) from ``init = cospi(u / 2)``, sn(u K, k) from ``sinpi(u / 2)``."""
    winv = 1 / init
    for x in reversed(landen):
        winv = 1 / (1 + x) * (winv + x / winv)
    return 1 / winv


def _cde(u, landen):
    return _ellip(_cospi(u / 2), landen)


def _sne(u, landen):
    return _ellip(_sinpi(u / 2), landen)


def _asne(w, k):
    """The inverse of sn, eqs. (50) and (56) (design.jl:147-158); ``w`` complex."""
    w, oldw = complex(w), None
    while w != oldw and w == w:
        oldw, kold = w, k
        k = (k / (1 + math.sqrt(1 - k * k))) ** 2
        w = 2 * w / ((1 + k) * (1 + cmath.sqrt(-(kold * kold) * (w * w) + 1)))
    return 2 * cmath.asin(w) / math.pi


def Elliptic(*args):
    """``Elliptic([T,] n, rp, rs)``: ``n`` pole elliptic (Cauer) prototype with ``rp`` dB ripple in the passband and ``rs`` dB attenuation in the stopband
    (design.jl:160-228; Orfanidis, Lecture notes on elliptic filter design, 2007)."""
    T, (n, rp, rs) = _proto_args("Elliptic", args, 3)
    if n <= 0:
        raise DomainError(f"n must be positive, got {n}")
    if not rp > 0:
        raise DomainError(f"rp must be positive, got {rp}")
    if not rp < rs:
        raise DomainError(f"rp must be less than rs, got {rp} and {rs}")
    ep = math.sqrt(10.0 ** (rp / 10) - 1)                                # eq. (2)
    es = math.sqrt(10.0 ** (rs / 10) - 1)
    k1 = ep / es                                                         # eq. (3)
    if k1 >= 1:
        raise ArgumentError("filter order is too high for parameters")
    k1p2 = 1 - k1 * k1                                                   # eq. (20)
    k1p_landen = _landen(math.sqrt(k1p2))
    kp = 1.0                                                             # eq. (47)
    for i in range(1, n // 2 + 1):
        kp *= _sne((2 * i - 1) / n, k1p_landen)
    kp = k1p2 ** (n / 2) * kp ** 4
    k = math.sqrt(1 - kp * kp)
    k_landen = _landen(k)
    v0 = -1j / n * _asne(1j / ep, k1)                                    # eq. (65)
    z, p = [0j] * (2 * (n // 2)), [0j] * n
    gain = 1.0
    for i in range(1, n // 2 + 1):
        w = (2 * i - 1) / n                                              # eq. (43)
        ze = complex(0.0, -1 / (k * _cde(w, k_landen)))                  # eq. (62)
        z[2 * i - 2] = ze
        z[2 * i - 1] = ze.conjugate()
        pole = 1j * _cde(w - 1j * v0, k_landen)                          # eq. (64)
        p[2 * i - 2] = pole.conjugate()
        p[2 * i - 1] = pole
        gain *= _abs2(pole) / _abs2(ze)
    if n % 2:
        pole = 1j * _sne(1j * v0, k_landen)
        p[-1] = pole
        gain *= abs(pole)
    else:
        gain *= 10.0 ** (-rp / 20)
    return _proto(T, z, p, gain)


# ---- response types (design.jl:235-315) -----------------------------------------------------------------------------------------------------------
def normalize_freq(w, fs):
    """Frequency in half-cycles per sample, in (0, 1) (design.jl:235-240)."""
    if w <= 0:
        raise DomainError("frequencies must be positive")
    f = 2 * w / fs
    if f >= 1:
        raise DomainError(f"frequencies must be less than the Nyquist frequency {fs / 2}")
    return f


def normalize_complex_freq(w, fs):
    """design.jl:241-245"""
    f = 2 * w / fs
    if f >= 2:
        raise DomainError(f"frequencies must be less than the sampling frequency {fs}")
    return f


def _real_arg(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise TypeError(f"{what} must be a real number")
    return v / 1


class FilterType:
    """``FilterType``: what a prototype is transformed to."""


class _OneEdge(FilterType):
    def __init__(self, w):
        self.w = _real_arg(w, "Wn")

    def __repr__(self):
        return f"{type(self).__name__}({self.w!r})"


class Lowpass(_OneEdge):
    """``Lowpass(Wn)``: low pass filter with cutoff frequency ``Wn``."""


class Highpass(_OneEdge):
    """``Highpass(Wn)``: high pass filter with cutoff frequency ``Wn``."""


class _TwoEdges(FilterType):
    def __init__(self, w1, w2):
        w1, w2 = _real_arg(w1, "Wn1"), _real_arg(w2, "Wn2")
        if not w1 < w2:
            raise ArgumentError("w1 must be less than w2")
        self.w1, self.w2 = w1, w2

    def __repr__(self):
        return f"{type(self).__name__}({self.w1!r}, {self.w2!r})"


class Bandpass(_TwoEdges):
    """``Bandpass(Wn1, Wn2)``: band pass filter with pass band frequencies (``Wn1``, ``Wn2``)."""


class Bandstop(_TwoEdges):
    """``Bandstop(Wn1, Wn2)``: band stop filter with stop band frequencies (``Wn1``, ``Wn2``)."""


class ComplexBandpass(_TwoEdges):
    """``ComplexBandpass(Wn1, Wn2)``: complex band pass filter with pass band frequencies (``Wn1``, ``Wn2``); ``FIRWindow`` designs only."""


# ---- prototype transformations (design.jl:326-434) ------------------------------------------------------------------------------------------------
def _snap(v, npoles):
    """``abs(real(v) - 1) < np * eps(real(v)) && (v = 1)`` (design.jl:353-354, :419-420)."""
    return 1.0 if abs(v.real - 1) < npoles * np.spacing(abs(v.real)) else v.real


def _like(proto, z, p, k):
    """An ``"s"`` ``ZeroPoleGain`` of the prototype's element types: ``oftype(k, ...)`` and the roots' own type."""
    C = np.complex64 if proto.dtype == np.dtype(np.float32) else np.complex128
    kd = proto.kdtype if proto.kdtype.kind == "f" else np.dtype(np.float64)
    return ZeroPoleGain(np.array(z, dtype=np.complex128).astype(C), np.array(p, dtype=np.complex128).astype(C), kd.type(k), domain="s")


def transform_prototype(ftype, proto):
    """``transform_prototype(ftype, proto)`` (design.jl:326-425): the analog filter of response type ``ftype`` from the low-pass prototype ``proto``, an ``"s"``
    filter (converted to ``ZeroPoleGain`` first).  The formulas are those of Octave's ``sftrans`` documentation, as in the reference."""
    if not isinstance(proto, FilterCoefficients) or proto.domain != "s":
        raise TypeError("the prototype must be a filter coefficient object in the s domain")
    if not isinstance(ftype, (Lowpass, Highpass, Bandpass, Bandstop)):
        raise TypeError("the response type must be Lowpass, Highpass, Bandpass or Bandstop")
    if not isinstance(proto, ZeroPoleGain):
        proto = ZeroPoleGain(proto)
    z, p, k = [complex(v) for v in proto.z], [complex(v) for v in proto.p], float(proto.k)
    nz, npl = len(z), len(p)
    if isinstance(ftype, Highpass):                                      # :331-356
        newz, newp = [0j] * max(nz, npl), [0j] * max(nz, npl)
        num = 1 + 0j
        for i in range(nz):
            num *= -z[i]
            newz[i] = ftype.w / z[i]
        den = 1 + 0j
        for i in range(npl):
            den *= -p[i]
            newp[i] = ftype.w / p[i]
        return _like(proto, newz, newp, k * _snap(num, npl) / _snap(den, npl))
    if isinstance(ftype, Lowpass):                                       # :326-328
        return _like(proto, [ftype.w * v for v in z], [ftype.w * v for v in p], k * ftype.w ** (npl - nz))
    w1, w2 = ftype.w1, ftype.w2
    if isinstance(ftype, Bandstop):                                      # :381-422
        npairs = max(nz, npl)
        newz, newp = [0j] * (2 * npairs), [0j] * (2 * npairs)
        prods = []
        for old, new in ((z, newz), (p, newp)):
            prod = 1 + 0j
            for i, v in enumerate(old):
                prod *= -v
                b = (w2 - w1) / (2 * v)
                pm = cmath.sqrt(-w2 * w1 + b * b)
                new[2 * i], new[2 * i + 1] = b - pm, b + pm
            prods.append(prod)
            npm = cmath.sqrt(complex(-(w2 * w1), -0.0))                  # any remaining poles / zeros are real and not cancelled
            for i in range(len(old), npairs):
                new[2 * i], new[2 * i + 1] = -npm, npm
        return _like(proto, newz, newp, k * _snap(prods[0], npl) / _snap(prods[1], npl))
    ncommon = min(nz, npl)                                               # Bandpass, :359-378
    newz, newp = [0j] * (2 * nz + npl - ncommon), [0j] * (2 * npl + nz - ncommon)
    for old, new in ((p, newp), (z, newz)):
        for i, v in enumerate(old):
            b = v * ((w2 - w1) / 2)
            pm = cmath.sqrt(-w2 * w1 + b * b)
            new[2 * i], new[2 * i + 1] = b + pm, b - pm
    return _like(proto, newz, newp, k * (w2 - w1) ** (npl - nz))


def analogfilter(ftype, proto):
    """``analogfilter(responsetype, designmethod)`` (design.jl:433-434): an analog filter, a ``ZeroPoleGain`` in the ``"s"`` domain."""
    return transform_prototype(ftype, proto)


def bilinear(f, fs):
    """``bilinear(f, fs)`` (design.jl:445-495): the ``"z"`` ``ZeroPoleGain`` of an ``"s"`` filter by the bilinear transform with sampling frequency ``fs``;
    with fewer zeros than poles the missing zeros go to z = -1."""
    if not isinstance(f, FilterCoefficients) or f.domain != "s":
        raise TypeError("bilinear takes a filter coefficient object in the s domain")
    fs = _real_arg(fs, "fs")
    if not isinstance(f, ZeroPoleGain):
        f = ZeroPoleGain(f)
    z = [complex(-1.0)] * max(len(f.p), len(f.z))
    p = [0j] * len(f.p)
    num = 1 + 0j
    for i, v in enumerate(f.z):
        v = complex(v)
        z[i] = (2 + v / fs) / (2 - v / fs)
        num *= 2 * fs - v
    den = 1 + 0j
    for i, v in enumerate(f.p):
        v = complex(v)
        p[i] = (2 + v / fs) / (2 - v / fs)
        den *= 2 * fs - v
    single = f.dtype == np.dtype(np.float32)
    C = np.complex64 if single else np.complex128
    kd = f.kdtype if f.kdtype.kind == "f" else np.dtype(np.float64)
    return ZeroPoleGain(np.array(z, dtype=np.complex128).astype(C), np.array(p, dtype=np.complex128).astype(C), kd.type(float(f.k) * num.real / den.real))


def prewarp(ftype, fs=None):
    """``prewarp(ftype, fs)`` (design.jl:498-501): the response type with its frequencies normalised and pre-warped for the bilinear transform at a sampling
    frequency of 2; ``prewarp(f)`` of a frequency in half-cycles per sample is ``4 tanpi(f / 2)`` (:503)."""
    if fs is None and not isinstance(ftype, FilterType):
        return 4 * _tanpi(_real_arg(ftype, "f") / 2)
    if not isinstance(ftype, (Lowpass, Highpass, Bandpass, Bandstop)) or fs is None:
        raise TypeError("prewarp(ftype, fs) takes a Lowpass, Highpass, Bandpass or Bandstop and a sampling frequency")
    if isinstance(ftype, _OneEdge):
        return type(ftype)(prewarp(normalize_freq(ftype.w, fs)))
    return type(ftype)(prewarp(normalize_freq(ftype.w1, fs)), prewarp(normalize_freq(ftype.w2, fs)))


def iirnotch(w, bandwidth, fs=2):
    """``iirnotch(Wn, bandwidth; fs=2)`` (design.jl:529-539): second-order digital notch at ``Wn`` with bandwidth ``bandwidth`` (Orfanidis, Introduction to
    signal processing, 1996, p. 370), a ``Biquad``."""
    w = normalize_freq(_real_arg(w, "Wn"), fs)
    bandwidth = normalize_freq(_real_arg(bandwidth, "bandwidth"), fs)
    b = 1 / (1 + _tanpi(bandwidth / 2))                                  # eq. 8.2.23
    b1 = -2 * b * _sincospi(w)[1]                                        # eq. 8.2.22
    return Biquad(b, b1, b, b1, 2 * b - 1)


# ---- window FIR design (design.jl:561-674) --------------------------------------------------------------------------------------------------------
class FIRWindow:
    """``FIRWindow(window; scale=true)``: FIR design with the window ``window``, a vector as long as the filter has taps;
    ``FIRWindow(; transitionwidth, attenuation=60, scale=true)``: a Kaiser window from ``kaiserord`` (design.jl:561-595).

    With ``scale`` the response is unity at 0 for ``Lowpass`` and ``Bandstop``, at the Nyquist frequency for ``Highpass``, in the centre of the passband
    for ``Bandpass`` and ``ComplexBandpass``."""

    def __init__(self, window=None, scale=True, *, transitionwidth=None, attenuation=60):
        if window is None:
            if transitionwidth is None:
                raise ArgumentError("must specify transitionwidth")
            window = windows.kaiser(*kaiserord(transitionwidth, attenuation))
        elif transitionwidth is not None:
            raise TypeError("FIRWindow takes a window or a transition width, not both")
        if not isinstance(scale, (bool, np.bool_)):
            raise TypeError("scale must be a Bool")
        window = np.asarray(window.cpu().numpy() if hasattr(window, "cpu") else window)
        if window.ndim != 1 or window.dtype.kind not in "fiu":
            raise TypeError("window must be a vector of real numbers")
        self.window, self.scale = window.astype(np.float64), bool(scale)


def _firprototype(n, ftype, fs):
    """design.jl:598-640"""
    m = np.arange(1, n + 1) - (n + 1) / 2
    if isinstance(ftype, ComplexBandpass):                               # :614-621: the real low-pass prototype turned to the band centre
        w1, w2 = normalize_complex_freq(ftype.w1, fs), normalize_complex_freq(ftype.w2, fs)
        w_center, w_cutoff = (w2 + w1) / 2, (w2 - w1) / 2
        w = normalize_freq(w_cutoff, 2)
        s, c = _sincospi(w_center * np.arange(n))
        return (w * np.sinc(w * m)).astype(np.complex128) * (c + 1j * s)
    if isinstance(ftype, _TwoEdges):
        w1, w2 = normalize_freq(ftype.w1, fs), normalize_freq(ftype.w2, fs)
        if isinstance(ftype, Bandstop):
            if n % 2 == 0:
                raise ArgumentError("FIRWindow bandstop filters must have an odd number of coefficients")
            out = w1 * np.sinc(w1 * m) - w2 * np.sinc(w2 * m)
            out[n // 2] += 1
            return out
        return w2 * np.sinc(w2 * m) - w1 * np.sinc(w1 * m)
    w = normalize_freq(ftype.w, fs)
    if isinstance(ftype, Highpass):
        if n % 2 == 0:
            raise ArgumentError("FIRWindow highpass filters must have an odd number of coefficients")
        out = -w * np.sinc(w * m)
        out[n // 2] += 1
        return out
    return w * np.sinc(w * m)


def _scalefactor(coefs, ftype, fs):
    """design.jl:642-667"""
    n = len(coefs)
    m = np.arange(1, n + 1) - (n + 1) / 2
    if isinstance(ftype, ComplexBandpass):
        s, c = _sincospi(-normalize_complex_freq(ftype.w1 / 2 + ftype.w2 / 2, fs) * m)
        return abs(np.sum(coefs * (c + 1j * s)))
    if isinstance(ftype, Bandstop):
        return np.sum(coefs)
    if isinstance(ftype, Bandpass):
        return np.sum(coefs * _sincospi(normalize_freq(ftype.w1 / 2 + ftype.w2 / 2, fs) * m)[1])
    if isinstance(ftype, Highpass):
        return np.sum(coefs[0::2]) - np.sum(coefs[1::2])
    return np.sum(coefs)


def digitalfilter(ftype, proto, fs=2):
    """``digitalfilter(responsetype, designmethod; fs=2)``.

    A prototype (design.jl:512-513): ``bilinear(transform_prototype(prewarp(ftype, fs), proto), 2)``, a ``ZeroPoleGain`` in the ``"z"`` domain.
    A ``FIRWindow`` (:669-674): the windowed ideal response of all five response types, a Float64 vector (ComplexF64 for a ``ComplexBandpass``)."""
    if not isinstance(ftype, (_OneEdge, _TwoEdges)):
        raise TypeError("the response type must be Lowpass, Highpass, Bandpass, Bandstop or ComplexBandpass")
    fs = _real_arg(fs, "fs")
    if isinstance(proto, FIRWindow):
        out = _firprototype(len(proto.window), ftype, fs) * proto.window
        return out * (1 / _scalefactor(out, ftype, fs)) if proto.scale else out
    if not isinstance(proto, FilterCoefficients):
        raise TypeError("the design method must be a prototype (a filter coefficient object in the s domain) or a FIRWindow")
    return bilinear(transform_prototype(prewarp(ftype, fs), proto), 2)
