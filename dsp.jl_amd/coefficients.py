"""Filter coefficient types of DSP.jl ``src/Filters/coefficients.jl``, real coefficients: host objects only.

``Biquad``, ``SecondOrderSections``, ``ZeroPoleGain`` and a minimal ``PolynomialRatio``, with the conversions between them.  The element type of a
coefficient object is Float32 or Float64 (``.dtype``); anything else real is taken to Float64.  Complex coefficients raise ``UnsupportedError``.

Every object has a ``.domain``: ``"z"`` (the default of every constructor) or ``"s"``, the reference's type parameter ``Domain``.  A conversion keeps
the domain (coefficients.jl:29-34, :93, :160-175, :244-481); none exists between the two, and only ``"z"`` filters filter.
"""
from __future__ import annotations

import math
import numbers

import numpy as np

from . import util
from ._lib import ArgumentError, UnsupportedError

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


def _dtype_of(v) -> np.dtype:
    if isinstance(v, (np.ndarray, np.generic)):
        return v.dtype
    if isinstance(v, bool):
        return np.dtype(np.bool_)
    if isinstance(v, numbers.Integral):
        return np.dtype(np.int64)
    if isinstance(v, numbers.Real):
        return _F64
    if isinstance(v, numbers.Complex):
        return np.dtype(np.complex128)
    return np.asarray(v).dtype


def _float_type(*vals) -> np.dtype:
    """Float32 when every value is, Float64 otherwise (``typeof(one(T) / one(T))`` restricted to the two element types of this library)."""
    dts = [_dtype_of(v) for v in vals]
    if any(d.kind == "c" for d in dts):
        raise UnsupportedError("complex filter coefficients are not accelerated: use DSP.jl's CPU path")
    if any(d.kind not in "fiub" for d in dts):
        raise TypeError("filter coefficients must be numbers")
    return _F32 if dts and all(d == _F32 for d in dts) else _F64


def _real_vec(v, what):
    a = np.atleast_1d(np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v))
    if a.ndim != 1:
        raise ArgumentError(f"{what} must be a vector")
    return a


class FilterCoefficients:
    """``FilterCoefficients{Domain}``: ``.domain`` is ``"z"`` or ``"s"``."""
    domain = "z"


def _domain_arg(domain, src=None):
    """The domain of a constructor call: the keyword (default ``"z"``), or for a conversion the source's own -- another one is no method."""
    if domain is not None and domain not in ("z", "s"):
        raise ArgumentError(f'domain must be "z" or "s", got {domain!r}')
    if src is not None:
        if domain is not None and domain != src.domain:
            raise TypeError(f"no conversion from the {src.domain} domain to the {domain} domain")
        return src.domain
    return "z" if domain is None else domain


def require_z(f, what):
    """The reference has only ``{:z}`` methods of what filters (filt.jl, response.jl:127-140): a ``MethodError`` there, a ``TypeError`` here."""
    if isinstance(f, FilterCoefficients) and f.domain != "z":
        raise TypeError(f"{what} has no method for a filter in the s domain")


class PolynomialRatio(FilterCoefficients):
    """``PolynomialRatio(b, a)``: ``b`` and ``a`` in powers of z^-1 (what ``filt(b, a, x)`` takes), normalised by ``a[0]`` (coefficients.jl:146-151).

    ``PolynomialRatio(b, a, domain="s")``: highest power of s first, not normalised (:83-91, :152-153).  As the reference's polynomials, ``b`` and ``a`` drop
    their leading zeros, and the zeros that end both (a common factor s^i, :87-89); ``.b`` and ``.a`` are then what ``coefb`` / ``coefa`` return."""

    def __init__(self, b, a=None, domain=None):
        if a is None and isinstance(b, FilterCoefficients):
            self.domain = _domain_arg(domain, b)
            src = b if isinstance(b, PolynomialRatio) else _pr_from(b)
            self.b, self.a, self.dtype = src.b.copy(), src.a.copy(), src.dtype
            return
        self.domain = _domain_arg(domain)
        bv, av = _real_vec(b, "b"), _real_vec(1.0 if a is None else a, "a")
        self.dtype = _float_type(bv, av)
        if self.domain == "s":
            if not av.any():
                raise ArgumentError("filter must have non-zero denominator")                  # :84-86
            bv, av = (v[np.flatnonzero(v)[0]:] if v.any() else np.zeros(1, v.dtype) for v in (bv, av))
            if bv.any():                                                                      # i = min(firstindex(a), firstindex(b)), :87
                cut = min(len(v) - 1 - np.flatnonzero(v)[-1] for v in (bv, av))
                bv, av = bv[:len(bv) - cut], av[:len(av) - cut]
            self.b, self.a = bv.astype(self.dtype), av.astype(self.dtype)
            return
        if av.size == 0 or av[0] == 0:
            raise ArgumentError("filter must have non-zero leading denominator coefficient")
        self.b = (bv / av[0]).astype(self.dtype)
        self.a = (av / av[0]).astype(self.dtype)


class Biquad(FilterCoefficients):
    """``Biquad(b0, b1, b2, a1, a2)`` / ``Biquad(b0, b1, b2, a0, a1, a2, g=1)`` (coefficients.jl:244-247); ``Biquad(f)`` converts a filter of order <= 2."""

    def __init__(self, *args, domain=None):
        if len(args) == 1 and isinstance(args[0], FilterCoefficients):
            f = args[0]
            self.domain = _domain_arg(domain, f)
            if isinstance(f, SecondOrderSections):                     # :344-349
                if len(f.biquads) != 1:
                    raise ArgumentError("only a single second order section may be converted to a biquad")
                q = f.biquads[0]
                dt = util.promote_type(f.dtype, f.gdtype)
                dt = dt if dt in (_F32, _F64) else _F64
                vals = (q.b0 * f.g, q.b1 * f.g, q.b2 * f.g, q.a1, q.a2)
            elif isinstance(f, Biquad):
                dt, vals = f.dtype, f.coefficients()
            else:
                pr = f if isinstance(f, PolynomialRatio) else _pr_from(f)
                n = max(len(pr.b), len(pr.a))
                if n > 3:                                              # :267-269
                    raise ArgumentError("cannot convert a filter of length > 3 to Biquad")
                b, a = np.zeros(3, pr.dtype), np.zeros(3, pr.dtype)
                if f.domain == "s":                                    # both from the highest power present in either, b[lastidx] ... (:265, :273)
                    b[n - len(pr.b):n], a[n - len(pr.a):n] = pr.b, pr.a
                    if a[0] != 1:                                      # :270-272
                        raise ArgumentError("leading denominator coefficient of a Biquad must be one")
                else:
                    b[:len(pr.b)], a[:len(pr.a)] = pr.b, pr.a
                dt, vals = pr.dtype, (b[0], b[1], b[2], a[1], a[2])
        elif len(args) == 5:
            self.domain = _domain_arg(domain)
            dt, vals = _float_type(*args), args
        elif len(args) in (6, 7):
            self.domain = _domain_arg(domain)
            b0, b1, b2, a0, a1, a2 = args[:6]
            g = args[6] if len(args) == 7 else 1
            dt = _float_type(*args)
            t = dt.type
            if t(a0) == 0:
                raise ArgumentError("filter must have non-zero leading denominator coefficient")
            vals = (t(g) * t(b0) / t(a0), t(g) * t(b1) / t(a0), t(g) * t(b2) / t(a0), t(a1) / t(a0), t(a2) / t(a0))
        else:
            raise TypeError("Biquad(b0, b1, b2, a1, a2), Biquad(b0, b1, b2, a0, a1, a2[, g]) or Biquad(filter)")
        self.dtype = dt
        self.b0, self.b1, self.b2, self.a1, self.a2 = (dt.type(v) for v in vals)

    def coefficients(self):
        return (self.b0, self.b1, self.b2, self.a1, self.a2)

    def __repr__(self):
        return f"Biquad{{{':s,' if self.domain == 's' else ''}{self.dtype.name}}}({', '.join(repr(float(v)) for v in self.coefficients())})"


class ZeroPoleGain(FilterCoefficients):
    """``ZeroPoleGain(z, p, k)``; ``ZeroPoleGain(f)`` converts (a ``PolynomialRatio`` by ``numpy.roots``)."""

    def __init__(self, z, p=None, k=None, domain=None):
        if p is None and isinstance(z, FilterCoefficients):
            self.domain = _domain_arg(domain, z)
            src = z if isinstance(z, ZeroPoleGain) else _zpk_from(z)
            self.z, self.p, self.k, self.dtype, self.kdtype = src.z.copy(), src.p.copy(), src.k, src.dtype, src.kdtype
            return
        self.domain = _domain_arg(domain)
        zv, pv = _real_vec(z, "z"), _real_vec(p, "p")
        single = all(v.size == 0 or v.dtype in (_F32, np.dtype(np.complex64)) for v in (zv, pv)) and (zv.size or pv.size)
        self.dtype = _F32 if single else _F64                        # promote_type(real(Z), real(P))
        if _dtype_of(k).kind == "c":
            raise UnsupportedError("complex filter coefficients are not accelerated: use DSP.jl's CPU path")
        self.z, self.p = zv.astype(np.complex128), pv.astype(np.complex128)
        self.k, self.kdtype = k, _dtype_of(k)


class SecondOrderSections(FilterCoefficients):
    """``SecondOrderSections(biquads, g)`` (coefficients.jl:300); ``SecondOrderSections(f)`` converts a ``Biquad``, a ``ZeroPoleGain`` (:430-481) or a
    ``PolynomialRatio`` (through ``ZeroPoleGain``)."""

    def __init__(self, biquads, g=None, domain=None):
        if g is None and isinstance(biquads, FilterCoefficients):
            f = biquads
            self.domain = _domain_arg(domain, f)
            if isinstance(f, SecondOrderSections):
                self.biquads, self.g, self.dtype, self.gdtype = list(f.biquads), f.g, f.dtype, f.gdtype
            elif isinstance(f, Biquad):                                # :308, :311: g = one(Int)
                self.biquads, self.g, self.dtype, self.gdtype = [f], 1, f.dtype, np.dtype(np.int64)
            else:
                zpk = f if isinstance(f, ZeroPoleGain) else _zpk_from(f)
                self.biquads, self.g, self.dtype, self.gdtype = _sections_from_zpk(zpk), zpk.k, zpk.dtype, zpk.kdtype
            return
        if g is None:
            raise TypeError("SecondOrderSections(biquads, g)")
        biquads = list(biquads)
        if not all(isinstance(q, Biquad) for q in biquads):
            raise TypeError("biquads must be a vector of Biquad")
        if _dtype_of(g).kind == "c":
            raise UnsupportedError("complex filter coefficients are not accelerated: use DSP.jl's CPU path")
        self.domain = _domain_arg(domain) if domain is not None or not biquads else biquads[0].domain    # Vector{Biquad{D,T}}: one domain, :295-301
        if any(q.domain != self.domain for q in biquads):
            raise ArgumentError("the sections of a SecondOrderSections must all be in its own domain")
        self.dtype = _F32 if biquads and all(q.dtype == _F32 for q in biquads) else _F64
        self.biquads = [q if q.dtype == self.dtype else Biquad(*(self.dtype.type(v) for v in q.coefficients()), domain=self.domain) for q in biquads]
        self.g, self.gdtype = g, _dtype_of(g)

    def table(self) -> np.ndarray:
        """K x 5 Float64: b0 b1 b2 a1 a2 per section (the values are exact: Float32 widens without rounding)."""
        return np.array([[float(v) for v in q.coefficients()] for q in self.biquads], dtype=np.float64).reshape(len(self.biquads), 5)


# ---- conversions ------------------------------------------------------------------------------------------------------------------------------------
def _pr_from(f) -> PolynomialRatio:
    if isinstance(f, Biquad):                                          # :256-260
        return PolynomialRatio(np.array([f.b0, f.b1, f.b2], f.dtype), np.array([1, f.a1, f.a2], f.dtype), domain=f.domain)
    if isinstance(f, SecondOrderSections):                             # :367
        return _pr_from(_zpk_from(f))
    if isinstance(f, ZeroPoleGain):                                    # :160-164: b = real(k fromroots(z)), a = real(fromroots(p)), shifted to z^-1
        dt = util.promote_type(f.dtype, f.kdtype)
        dt = dt if dt in (_F32, _F64) else _F64
        b, a = np.atleast_1d(np.real(f.k * np.poly(f.z))), np.atleast_1d(np.real(np.poly(f.p)))   # (np.poly of no roots is the scalar 1)
        if f.domain == "s":                                            # highest power first as it stands; the constructor drops a common s^i
            pr = PolynomialRatio(b, a, domain="s")
            pr.b, pr.a, pr.dtype = pr.b.astype(dt), pr.a.astype(dt), dt
            return pr
        n = max(len(b), len(a))
        b, a = np.concatenate([np.zeros(n - len(b)), b]), np.concatenate([np.zeros(n - len(a)), a])
        lead = next((i for i in range(n) if a[i] != 0 or b[i] != 0), 0)   # the highest power present becomes z^0
        pr = PolynomialRatio(b[lead:], a[lead:])
        pr.b, pr.a, pr.dtype = pr.b.astype(dt), pr.a.astype(dt), dt
        return pr
    raise TypeError("not a filter coefficient object")


def _zpk_from(f) -> ZeroPoleGain:
    if isinstance(f, PolynomialRatio) and f.domain == "s":             # :170-175: roots of both, k = b[end] / a[end], the leading coefficients
        zpk = ZeroPoleGain(np.roots(f.b) if f.b.any() else np.zeros(0), np.roots(f.a), f.dtype.type(f.b[0] / f.a[0]), domain="s")
        zpk.dtype = f.dtype
        return zpk
    if isinstance(f, PolynomialRatio):                                 # :170-175
        n = max(len(f.b), len(f.a))
        b, a = np.zeros(n), np.zeros(n)
        b[:len(f.b)], a[:len(f.a)] = f.b, f.a
        nz = np.flatnonzero(b)
        k = f.dtype.type(b[nz[0]]) if nz.size else f.dtype.type(0)
        zpk = ZeroPoleGain(np.roots(b) if nz.size else np.zeros(0), np.roots(a), k)
        zpk.dtype = f.dtype
        return zpk
    if isinstance(f, Biquad):
        return _zpk_from(_pr_from(f))
    if isinstance(f, SecondOrderSections):                             # :352-363
        z, p, k = [], [], f.g
        for q in f.biquads:
            one = _zpk_from(q)
            z.extend(one.z)
            p.extend(one.p)
            k = k * one.k
        zpk = ZeroPoleGain(np.array(z, np.complex128), np.array(p, np.complex128), k, domain=f.domain)
        zpk.dtype = f.dtype
        return zpk
    raise TypeError("not a filter coefficient object")


def _split_real_complex(x, sortby=None):
    """coefficients.jl:392-426: (complex values, each followed by its conjugate; real values; matched).  The reference walks a Dict, whose order is
    arbitrary; here the keys keep the order of first appearance (and a stable sort)."""
    d: dict = {}
    for v in x:
        vn = complex(abs(v.real) if v.real == 0 else v.real, abs(v.imag) if v.imag == 0 else v.imag)
        d[vn] = d.get(vn, 0) + 1
    ks = list(d)
    if sortby is not None:
        ks.sort(key=sortby)
    c, r = [], []
    for k in ks:
        if k.imag != 0:
            kc = k.conjugate()
            if kc not in d or d[k] != d[kc]:
                return c, r, False
            if k.imag > 0:
                for _ in range(d[k]):
                    c.extend((k, kc))
        else:
            r.extend([k.real] * d[k])
    return c, r, True


def _groupzp(z: list, p: list):
    """coefficients.jl:372-387: every pole with its closest zero; both lists lose what was paired."""
    n = min(len(z), len(p))
    grouped = [None] * n
    i = 0
    while i < n:
        idx = min(range(len(z)), key=lambda j: abs(z[j] - p[i]))
        grouped[i] = z.pop(idx)
        if complex(grouped[i]).imag != 0:
            i += 1
            if i >= n:
                raise ArgumentError("complex zeros could not be paired with the poles")   # a BoundsError in the reference
            grouped[i] = z.pop(idx)
        i += 1
    paired = p[:n]
    del p[:n]
    return grouped, paired


def _biquad_from_roots(z, p, dt, domain="z") -> Biquad:
    """convert(Biquad, ZeroPoleGain{D}(z, p, one(T))) for at most two zeros and one or two poles: in either domain the numerator is aligned with the
    denominator's highest power (:265, :273), and what ends both with zeros is a common factor of z^-1 or s."""
    a = np.real(np.poly(np.array(p, np.complex128)))
    b = np.real(np.poly(np.array(z, np.complex128))) if len(z) else np.ones(1)
    b = np.concatenate([np.zeros(len(a) - len(b)), b])
    b3, a3 = np.zeros(3), np.zeros(3)
    b3[:len(b)], a3[:len(a)] = b, a
    return Biquad(*(dt.type(v) for v in (b3[0], b3[1], b3[2], a3[1], a3[2])), domain=domain)


def _sections_from_zpk(f: ZeroPoleGain) -> list:
    """coefficients.jl:430-481."""
    z, p = list(f.z), list(f.p)
    nz, n = len(z), len(p)
    if nz > n:
        raise ArgumentError("ZeroPoleGain must not have more zeros than poles")
    complexz, realz, matched = _split_real_complex(z)
    if not matched:
        raise ArgumentError("complex zeros could not be matched to their conjugates")
    complexp, realp, matched = _split_real_complex(p, sortby=lambda v: abs(abs(v) - 1))
    if not matched:
        raise ArgumentError("complex poles could not be matched to their conjugates")
    z1, p1 = _groupzp(complexz, complexp)      # complex poles with the closest complex zeros
    z2, p2 = _groupzp(complexz, realp)         # real poles with the remaining complex zeros
    z3, p3 = _groupzp(realz, complexp)         # remaining complex poles with the closest real zeros
    z4, p4 = _groupzp(realz, realp)            # remaining real poles with the closest real zeros
    assert not complexz and not realz
    gz = z1 + z2 + z3 + z4
    gp = p1 + p2 + p3 + p4 + complexp + realp
    assert len(gz) == nz and len(gp) == n
    npairs, odd = n >> 1, n & 1
    biquads = [None] * (npairs + odd)
    for i in range(1, npairs + 1):             # sections are built in reverse, complete pairs first
        k = 2 * (npairs - i)
        biquads[odd + i - 1] = _biquad_from_roots(gz[k:min(k + 2, len(gz))], gp[k:k + 2], f.dtype, f.domain)
    if odd:                                    # the remaining pole and (maybe) zero come first
        biquads[0] = _biquad_from_roots(gz[n - 1:], [gp[-1]], f.dtype, f.domain)
    return biquads


def coefb(f) -> np.ndarray:
    """Numerator coefficients in powers of z^-1: the ``b`` of ``filt(b, a, x)``; of an ``"s"`` filter highest power of s first (coefficients.jl:195-206)."""
    return (f if isinstance(f, PolynomialRatio) else _pr_from(f)).b.copy()


def coefa(f) -> np.ndarray:
    """Denominator coefficients in powers of z^-1: the ``a`` of ``filt(b, a, x)``; of an ``"s"`` filter highest power of s first (:195-216)."""
    return (f if isinstance(f, PolynomialRatio) else _pr_from(f)).a.copy()


def _fma(dt, a, b, c):
    """``muladd(a, b, c)`` as one fused operation in dtype ``dt``: Float32 through the exact Float64 product, Float64 through ``math.fma`` where Python
    has it (3.13), else through longdouble."""
    if dt == _F32:
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    if hasattr(math, "fma"):
        return np.float64(math.fma(float(a), float(b), float(c)))
    return np.float64(np.longdouble(a) * np.longdouble(b) + np.longdouble(c))


def filt_stepstate(f: SecondOrderSections) -> np.ndarray:
    """``filt_stepstate(f::SecondOrderSections)`` (filt.jl:403-423): the (2, K) state with which a unit step leaves every section in steady state,
    evaluated in the coefficients' type."""
    require_z(f, "filt_stepstate")
    dt, t = f.dtype, f.dtype.type
    si = np.zeros((2, len(f.biquads)), dtype=dt)
    y = t(1)
    for i, q in enumerate(f.biquads):
        b0, b1, b2, a1, a2 = q.coefficients()
        den = t(1) + a1 + a2
        with np.errstate(divide="ignore", invalid="ignore"):
            si[0, i] = _fma(dt, a1 + a2, -b0, b1 + b2) / den * y
            si[1, i] = _fma(dt, a1, b2, _fma(dt, -a2, b0 + b1, b2)) / den * y
            y = y * ((b0 + b1 + b2) / den)
    return si
