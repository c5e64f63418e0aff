"""Plain numpy restatements of the reference's second-order-section code, the yardstick of the sos tests (never the code under test):

    sos_filt        _filt! (Filters/filt.jl:35-51, :70-80) in Float32, Float64 or np.longdouble, vectorised over columns
    filt_stepstate  filt.jl:403-423
    sos_filtfilt    filt.jl:341-360
    iir_filtfilt    filt.jl:261-280 with filt_stepstate(b, a) (:370-398) and _filt_iir! (dspbase.jl), for the reference's own cross-check

muladd is a fused multiply-add here: Float32 through the exact Float64 product (one rounding of the sum, then one to Float32 -- a double rounding that
differs from the fused result only in ties of the second step), Float64 and longdouble through math.fma where Python has it, else through longdouble."""
import math

import numpy as np

_HAS_FMA = hasattr(math, "fma")


def _fma(a, b, c, dt):
    """a * b + c in dtype dt, vectorised."""
    dt = np.dtype(dt)
    if dt == np.dtype(np.float32):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    if dt == np.dtype(np.float64):
        a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
        if _HAS_FMA:
            return np.array([math.fma(p, q, r) for p, q, r in zip(a.ravel(), b.ravel(), c.ravel())], np.float64).reshape(a.shape)
        return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(np.float64)
    return np.asarray(a, dt) * np.asarray(b, dt) + np.asarray(c, dt)     # longdouble: the yardstick's own precision


def _parts(x, dt):
    """(n, ncols) real lines of dtype dt from a real or complex (n,) / (n, cols...) array, and how to put them back."""
    x = np.asarray(x)
    n = x.shape[0]
    flat = x.reshape(n, -1)
    if x.dtype.kind == "c":
        lines = np.concatenate([flat.real, flat.imag], axis=1)
    else:
        lines = flat
    return lines.astype(dt), x.shape, x.dtype.kind == "c"


def _join(lines, shape, cplx):
    if cplx:
        h = lines.shape[1] // 2
        return (lines[:, :h] + 1j * lines[:, h:]).reshape(shape)
    return lines.reshape(shape)


def sos_filt(table, g, x, dtype, state=None, has_gain=True):
    """filt!(out, f, x) in `dtype` (the real working type).  table: K x 5 rows of b0 b1 b2 a1 a2.  state: None (zeros) or (2, K, lines) of dtype, where
    the lines are the flattened columns (real parts first, then imaginary parts, for a complex x).  Returns (y, end state (2, K, lines))."""
    dt = np.dtype(dtype)
    tb = np.asarray(table, np.float64).reshape(-1, 5).astype(dt)
    lines, shape, cplx = _parts(x, dt)
    n, m = lines.shape
    K = len(tb)
    si = np.zeros((2, K, m), dt) if state is None else np.array(state, dt).reshape(2, K, m)
    out = np.empty((n, m), dt)
    gg = dt.type(g)
    for i in range(n):
        yi = lines[i]
        for k in range(K):
            b0, b1, b2, a1, a2 = tb[k]
            xi = yi
            yi = _fma(b0, xi, si[0, k], dt)
            si[0, k] = _fma(a1, -yi, _fma(b1, xi, si[1, k], dt), dt)
            si[1, k] = _fma(b2, xi, (-a2 * yi).astype(dt), dt)
        out[i] = (gg * yi).astype(dt) if has_gain else yi
    res = _join(out, shape, cplx)
    return res, si


def end_state_columns(si, cplx):
    """(2, K, lines) of sos_filt -> (2, K, cols) in the working type (complex when the signal was)."""
    if not cplx:
        return si
    h = si.shape[2] // 2
    return si[:, :, :h] + 1j * si[:, :, h:]


def filt_stepstate(table, dtype=np.float64):
    dt = np.dtype(dtype)
    tb = np.asarray(table, np.float64).reshape(-1, 5).astype(dt)
    si = np.zeros((2, len(tb)), dt)
    y = dt.type(1)
    for i, (b0, b1, b2, a1, a2) in enumerate(tb):
        den = dt.type(1) + a1 + a2
        si[0, i] = _fma(a1 + a2, -b0, b1 + b2, dt) / den * y
        si[1, i] = _fma(a1, b2, _fma(-a2, b0 + b1, b2, dt), dt) / den * y
        y = y * ((b0 + b1 + b2) / den)
    return si


def extrapolate(sig, pad):
    """extrapolate_signal! (filt.jl:245-258) for one column."""
    n = len(sig)
    out = np.empty(n + 2 * pad, sig.dtype)
    k = np.arange(pad)
    out[:pad] = 2 * sig[0] - sig[pad - k]
    out[pad:pad + n] = sig
    out[pad + n:] = 2 * sig[n - 1] - sig[n - 2 - k]
    return out


def sos_filtfilt(table, g, x, dtype, coef_dtype=np.float64):
    """filtfilt(f::SecondOrderSections, x) in the real working type `dtype`."""
    dt = np.dtype(dtype)
    K = len(np.asarray(table).reshape(-1, 5))
    zi = filt_stepstate(table, coef_dtype).astype(dt)
    lines, shape, cplx = _parts(x, dt)
    n, m = lines.shape
    pad = min(6 * K, n - 1)
    out = np.empty((n, m), dt)
    for c in range(m):
        ext = extrapolate(lines[:, c], pad)
        ext, _ = sos_filt(table, g, ext, dt, state=(zi * ext[0])[:, :, None])
        ext = ext[::-1].copy()
        ext, _ = sos_filt(table, g, ext, dt, state=(zi * ext[0])[:, :, None])
        out[:, c] = ext[::-1][pad:pad + n]
    return _join(out, shape, cplx)


def _filt_iir(b, a, x, si):
    """_filt_iir! (dspbase.jl) for one column in Float64, transposed direct form II; si is updated."""
    n = len(si)
    out = np.empty_like(x)
    for i in range(len(x)):
        xi = x[i]
        val = si[0] + b[0] * xi
        for j in range(n - 1):
            si[j] = si[j + 1] + b[j + 1] * xi - a[j + 1] * val
        si[n - 1] = b[n] * xi - a[n] * val
        out[i] = val
    return out


def iir_filtfilt(b, a, x):
    """iir_filtfilt(b, a, x) (filt.jl:261-280) in Float64; x is (n,) or (n, cols)."""
    b, a = np.asarray(b, np.float64) / a[0], np.asarray(a, np.float64) / a[0]
    sz = max(len(b), len(a))
    b, a = np.concatenate([b, np.zeros(sz - len(b))]), np.concatenate([a, np.zeros(sz - len(a))])
    A = np.zeros((sz - 1, sz - 1))
    A[:, 0] = -a[1:]
    A[:sz - 2, 1:] = np.eye(sz - 2)
    zi = np.linalg.solve(np.eye(sz - 1) - A, b[1:] - a[1:] * b[0])
    x = np.asarray(x, np.float64)
    flat = x.reshape(x.shape[0], -1)
    n = flat.shape[0]
    pad = min(3 * (sz - 1), n - 1)
    out = np.empty_like(flat)
    for c in range(flat.shape[1]):
        ext = extrapolate(flat[:, c], pad)
        ext = _filt_iir(b, a, ext, zi * ext[0])
        ext = ext[::-1].copy()
        ext = _filt_iir(b, a, ext, zi * ext[0])
        out[:, c] = ext[::-1][pad:pad + n]
    return out.reshape(x.shape)


def rel_err(got, ref):
    """largest |got - ref| over largest |ref|, in longdouble."""
    got, ref = np.asarray(got), np.asarray(ref)
    cast = np.clongdouble if (got.dtype.kind == "c" or ref.dtype.kind == "c") else np.longdouble
    return float(np.max(np.abs(got.astype(cast) - ref.astype(cast))) / np.max(np.abs(ref.astype(cast))))
