"""Filters, evaluation points and the ctypes wrappers of the filter-response tests (no scipy: everything is a literal or a formula)."""
import ctypes as C

import numpy as np

import sos_cases as sc

POLY, SECTIONS, ZPK = 0, 1, 2
DERIV, NEG = 1, 2
COMPLEX, ANGLE, REAL_MINUS = 0, 1, 2
W, POINTS = 0, 1

# the filter behind the reference's goldens (test/filter_response.jl:21-27)
GOLDEN_B = 0.05634 * np.convolve([1.0, 1.0], [1.0, -1.0166, 1.0])
GOLDEN_A = np.convolve([1.0, -0.683], [1.0, -1.4461, 0.7957])


def ctype(R):
    return np.dtype(np.complex64 if np.dtype(R) == np.dtype(np.float32) else np.complex128)


def windowed_sinc(n, fc=0.2):
    """n taps of a Hamming-windowed sinc low-pass, cut-off fc (cycles per sample), unit gain at 0."""
    k = np.arange(n) - (n - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * k) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / max(n - 1, 1)))
    return h / h.sum()


def points(w, R, neg=False):
    """e^{+-iw} computed in Float64 and rounded to the working type: from there on an exact input."""
    w = np.asarray(w, dtype=np.float64)
    return np.exp((-1j if neg else 1j) * w).astype(ctype(R))


def cancellation_zpk(R):
    """test/filter_response.jl:46-47; in Float32 the roots 1 - 10^-n stay distinct from 1 up to n = 6 only (a pole at 1 would sit on the point w = 0)."""
    rs = [1 - 10.0 ** -n for n in range(1, 16 if np.dtype(R) == np.dtype(np.float64) else 7)]
    return np.array(rs, dtype=np.complex128), np.array(rs[::-1], dtype=np.complex128), 42.0


def cancellation_biquad():
    """test/filter_response.jl:49"""
    r = 0.999999
    return np.array([[42.0, 84.0 * (r * np.exp(1j)).real, 42.0 * r ** 2, 2.0 * (r * np.exp(1j)).real, r ** 2]]), 1.0


def cancellation_sos():
    """test/filter_response.jl:52-55"""
    pr = [1 - 10.0 ** -n for n in range(1, 11)]
    zr = pr[::-1]
    tb = np.array([[42.0, 84.0 * (z * np.exp(1j)).real, 42.0 * z ** 2, 2.0 * (p * np.exp(1j)).real, p ** 2] for z, p in zip(zr, pr)])
    return tb, 42.0 ** -9


def sections_cases():
    """name -> (K x 5 table, gain): the accuracy tables of tests/sos_cases.py and the reference's cancellation cascades."""
    out = {name: sc.table(name) for name in sc.ACCURACY}
    out["cancel_biquad"] = cancellation_biquad()
    out["cancel_sos"] = cancellation_sos()
    return out


def accuracy_table():
    """The protocol of DESIGN.md 4.14: rows (label, type name, e_cut, e_serial, ratio).  e_cut: largest |emulation - long double| / largest |long double|,
    e_serial the same for the serial restatement in the working precision (tests/response_ref.py); ratio = e_cut / max(e_serial, u), u the unit roundoff
    of the working type (an error below one rounding of the result's scale is not resolved)."""
    import response_ref as rr
    rows = []
    w_half, w_full = np.linspace(0.0, np.pi, 257), np.linspace(0.0, 2 * np.pi, 50)
    for R in (np.float32, np.float64):
        u = float(np.finfo(R).eps) / 2

        def row(label, got, ld, serial):
            e_cut, e_serial = rr.max_error(got, ld), rr.max_error(serial, ld)
            rows.append((label, np.dtype(R).name, e_cut, e_serial, e_cut / max(e_serial, u)))

        y = points(w_half, R, neg=True)
        for name, b, a in (("golden", GOLDEN_B, GOLDEN_A), ("sinc53", windowed_sinc(53), None), ("sinc4101", windowed_sinc(4101), None)):
            b = np.asarray(b, dtype=R)
            a = None if a is None else np.asarray(a, dtype=R)
            for deriv in (False, True):
                ld, serial = rr.poly_ld(b, a, y, R, deriv), rr.poly_serial(b, a, y, R, deriv)
                for chunks in sorted({1, 2, 3, max_chunks(len(b))}):
                    got = emulate(POLY, R, b, a, y, flags=DERIV if deriv else 0, chunks=chunks)
                    row(f"poly {name}{' deriv' if deriv else ''} chunks {chunks}", got, ld, serial)
        for name, (tb, g) in sections_cases().items():
            x = points(w_full if name.startswith("cancel") else w_half, R)
            row(f"sections {name}", emulate(SECTIONS, R, tb, None, x, gain=g), rr.sections_ld(tb, g, x, R), rr.sections_serial(tb, g, x, R))
        z, p, k = cancellation_zpk(R)
        x = points(w_full, R)
        row("zpk cancel", emulate(ZPK, R, z, p, x, gain=k), rr.zpk_ld(z, p, k, x, R), rr.zpk_serial(z, p, k, x, R))
    return rows


def max_chunks(n):
    """the forced cut with the most chunks: L = 16"""
    return max(1, -(-n // 16))


def geometry(form, R, ncoef, has_den, nw, chunks=0):
    from dsp_jl_amd import _dev, _lib
    c, ln, ws = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_resp_geometry_for(form, _dev.md_dtype(R), ncoef, 1 if has_den else 0, nw, chunks, C.byref(c), C.byref(ln), C.byref(ws)))
    return c.value, ln.value, ws.value


def flat(form, v):
    if v is None:
        return None, 0
    if form == ZPK:
        a = np.ascontiguousarray(np.asarray(v, dtype=np.complex128).reshape(-1))
        return a.view(np.float64), a.size
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    return a, (a.size // 5 if form == SECTIONS else a.size)


def emulate(form, R, num, den, pts, gain=1.0, flags=0, out_mode=COMPLEX, cminus=0.0, chunks=0):
    """mdsp_resp_emulate_host at the points ``pts`` (cast to the working type): the complex or real result, shaped like pts."""
    from dsp_jl_amd import _dev, _lib
    ct = ctype(R)
    p = np.ascontiguousarray(np.asarray(pts).astype(ct))
    out = np.zeros(p.shape, dtype=ct if out_mode == COMPLEX else np.dtype(R))
    nv, nn = flat(form, num)
    dv, nd = (nv, nn) if den is num and den is not None else flat(form, den)
    _lib.check(_lib.lib().mdsp_resp_emulate_host(p.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), form, flags, out_mode, _dev.md_dtype(R),
                                                 None if nv is None else nv.ctypes.data_as(_lib.pdbl), nn,
                                                 None if dv is None or nd == 0 else dv.ctypes.data_as(_lib.pdbl), nd, float(gain), float(cminus), p.size, chunks))
    return out
