"""The three forms of the filter-response kernels (csrc/resp_op.h) restated in numpy, twice:

* ``*_ld``: in ``np.longdouble`` / ``np.clongdouble`` (x87 extended: 64 bits of significand), the evaluation points and the coefficients taken as EXACT
  inputs -- the yardstick every accuracy figure is measured against;
* ``*_serial``: a serial single-chain Horner, product or ratio in the working precision (numpy's own complex arithmetic: no fma, no cut) -- what a
  straightforward host implementation gives, the denominator of the error ratios.

POLY: num(y) / den(y), num = sum b[k] y^k; ``deriv``: the numerator's coefficients are ``arange(n) * b`` rounded once in the working real type (an exact
input of both restatements).  SECTIONS: g prod biquad_k(x).  ZPK: k prod (x - z) / prod (x - p)."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble


def _ctype(R):
    return np.complex64 if np.dtype(R) == np.dtype(np.float32) else np.complex128


def deriv_coefficients(c, R):
    """k c[k], the product rounded once in R."""
    c = np.asarray(c, dtype=R)
    return (np.arange(len(c)).astype(R) * c).astype(R)


def _horner(c, y, ctype, rtype):
    acc = np.zeros(y.shape, dtype=ctype)
    for v in np.asarray(c, dtype=rtype)[::-1]:
        acc = acc * y + rtype(v)
    return acc


def poly_ld(b, a, pts, R, deriv=False):
    y = np.asarray(pts).astype(CLD)
    num = _horner(deriv_coefficients(b, R) if deriv else np.asarray(b, dtype=R), y, CLD, LD)
    return num if a is None else num / _horner(np.asarray(a, dtype=R), y, CLD, LD)


def poly_serial(b, a, pts, R, deriv=False):
    ct = _ctype(R)
    y = np.asarray(pts).astype(ct)
    rt = np.dtype(R).type
    num = _horner(deriv_coefficients(b, R) if deriv else np.asarray(b, dtype=R), y, ct, rt)
    return num if a is None else (num / _horner(np.asarray(a, dtype=R), y, ct, rt)).astype(ct)


def _sections(table, g, x, ctype, rtype):
    acc = np.ones(x.shape, dtype=ctype)
    for b0, b1, b2, a1, a2 in np.asarray(table, dtype=rtype).reshape(-1, 5):
        acc = acc * (((rtype(b0) * x + rtype(b1)) * x + rtype(b2)) / ((x + rtype(a1)) * x + rtype(a2)))
    return rtype(g) * acc


def sections_ld(table, g, pts, R):
    rt = np.dtype(R).type
    return _sections(np.asarray(table, dtype=R).astype(LD), LD(rt(g)), np.asarray(pts).astype(CLD), CLD, LD)


def sections_serial(table, g, pts, R):
    ct = _ctype(R)
    return _sections(np.asarray(table, dtype=R), np.dtype(R).type(g), np.asarray(pts).astype(ct), ct, np.dtype(R).type).astype(ct)


def _zpk(z, p, k, x, ctype):
    a, b = np.ones(x.shape, dtype=ctype), np.ones(x.shape, dtype=ctype)
    for r in z:
        a = a * (x - ctype(r))
    for r in p:
        b = b * (x - ctype(r))
    return (ctype(k) * a) / b


def zpk_ld(z, p, k, pts, R):
    ct = _ctype(R)
    return _zpk(np.asarray(z, dtype=ct).astype(CLD), np.asarray(p, dtype=ct).astype(CLD), LD(np.dtype(R).type(k)), np.asarray(pts).astype(CLD), CLD)


def zpk_serial(z, p, k, pts, R):
    ct = _ctype(R)
    return _zpk(np.asarray(z, dtype=ct), np.asarray(p, dtype=ct), np.dtype(R).type(k), np.asarray(pts).astype(ct), ct).astype(ct)


def max_error(got, want_ld):
    """largest |got - long double| / largest |long double|"""
    want_ld = np.asarray(want_ld)
    return float(np.max(np.abs(np.asarray(got).astype(want_ld.dtype) - want_ld)) / np.max(np.abs(want_ld)))
