"""Extended-precision reference for FIRFilter with COMPLEX taps (standard, interpolator, decimator, rational): ``filt!`` of
stream_filt.jl:409-558 with the generic ``unsafe_dot`` (util.jl:225-283: tap times sample, no conjugate) evaluated in ``np.clongdouble``
from the filter state.  Modelled on tests/polyphase_ref.py, whose closed-form windows it shares.

Per output and per REAL component it returns ``absdot``, the scale of that component's rounding error -- each component of a complex dot
product is a real dot product:

    absdot_re = sum_k (|h_re| |x_re| + |h_im| |x_im|)            (real part of the returned array)
    absdot_im = sum_k (|h_re| |x_im| + |h_im| |x_re|)            (imaginary part)

and the bound the tests apply is

    |y - ref| <= 2 (n + 1) u absdot + 4 u_min      per real component,   n = 2 tp for complex signals, tp for real ones

-- polyphase_ref.error_bound with the term count of a complex product: a component is a sum of n real products (one rounding per product, at
most n per sum, first order); the factor 2 covers second-order terms and a different order, 4 u_min underflow.  u and u_min are those of the
kernels' arithmetic: double whenever taps or signal are double (promote_type), single otherwise.  Derived, not measured.
"""
from __future__ import annotations

import numpy as np

from oracle.stream_filt import polyphase_closed_form, taps2pfb
from polyphase_ref import CLD, LD, error_bound, outputlength

_DOUBLE = (np.dtype(np.float64), np.dtype(np.complex128))


def accumulation_unit(taps_dtype, x_dtype):
    """(u, u_min) of the kernels' arithmetic: Float64 whenever taps or signal are double precision, Float32 otherwise."""
    dbl = np.dtype(taps_dtype) in _DOUBLE or np.dtype(x_dtype) in _DOUBLE
    t = np.float64 if dbl else np.float32
    return float(np.finfo(t).eps) / 2, float(np.finfo(t).tiny)


def terms(tp, x_dtype):
    """Real products per component of one output: 2 tp for a complex signal, tp for a real one."""
    return (2 if np.dtype(x_dtype).kind == "c" else 1) * tp


def complex_taps_ref(h, L, M, x, phi_idx=1, input_deficit=1, history=None):
    """One ``filt!`` call of FIRFilter(h, L//M) with complex h (L, M coprime) on x of shape (n,) or (nch, n), real or complex.

    State in: 1-based ``phi_idx`` and ``input_deficit``, ``history`` (nch, tapsPerPhi - 1) in x's dtype (zeros if None).  Returns
    ``(y, absdot, (phi_idx, input_deficit, history))``: y (nch, nout) clongdouble, absdot complex of y's shape (module docstring), the state
    after the chunk with the history in x's dtype, bit for bit what the filter keeps."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    nch, xlen = x2.shape
    pfb = taps2pfb(np.asarray(h), L).astype(CLD)
    tp = pfb.shape[0]
    hl = tp - 1
    if history is None:
        history = np.zeros((nch, hl), dtype=x.dtype)
    history = np.asarray(history).reshape(nch, hl)
    z = np.concatenate([history.astype(x.dtype), x2], axis=1)        # [history ; x] per channel
    new_hist = z[:, z.shape[1] - hl:].copy() if hl > 0 else np.zeros((nch, 0), dtype=x.dtype)   # shiftin!
    nout = outputlength(xlen, L, M, phi_idx, input_deficit)
    if nout == 0:                                                      # stream_filt.jl:483-487: the chunk only feeds the deficit
        y = np.zeros((nch, 0), dtype=CLD)
        ad = y.copy()
        state = (phi_idx, input_deficit - xlen, new_hist)
    else:
        phi, idx = polyphase_closed_form(phi_idx, input_deficit, L, M, np.arange(nout, dtype=np.int64))
        assert idx[-1] <= xlen and idx[0] >= 1
        zl = z.astype(CLD)
        zr, zi = np.abs(zl.real), np.abs(zl.imag)
        y = np.zeros((nch, nout), dtype=CLD)
        ad_re = np.zeros((nch, nout), dtype=LD)
        ad_im = np.zeros((nch, nout), dtype=LD)
        col = phi - 1
        start = idx - 1                                                # window of output m: z[idx_m - 1 + k], k = 0 .. tp - 1
        for k in range(tp):
            hk = pfb[k, col]
            hr, hi = np.abs(hk.real), np.abs(hk.imag)
            w = start + k
            y += hk * zl[:, w]
            ad_re += hr * zr[:, w] + hi * zi[:, w]
            ad_im += hr * zi[:, w] + hi * zr[:, w]
        ad = (ad_re + 1j * ad_im).astype(CLD)
        p_end = (phi_idx - 1) + nout * M
        state = (p_end % L + 1, input_deficit + p_end // L - xlen, new_hist)
    if one:
        y, ad, state = y[0], ad[0], (state[0], state[1], state[2][0])
    return y, ad, state


def excess(y, ref, absdot, n, u, u_min):
    """max over elements and real components of |y - ref| / bound (<= 1 passes), and the largest |y - ref| / (u absdot), the margin figure.
    ``n``: real products per component (``terms``).  NaN in y counts as failing."""
    y = np.asarray(y)
    if ref.size == 0:
        return 0.0, 0.0
    worst, ratio = 0.0, 0.0
    for yy, rr, aa in ((y.real, ref.real, absdot.real), (y.imag, ref.imag, absdot.imag)):
        err = np.abs(yy.astype(LD) - rr)
        b = error_bound(aa, n, u, u_min)
        if np.isnan(err).any():
            return float("inf"), float("inf")
        worst = max(worst, float(np.max(err / b)))                     # (b >= 4 u_min > 0)
        pos = aa > 0
        if pos.any():
            ratio = max(ratio, float(np.max(err[pos] / (u * aa[pos]))))
    return worst, ratio
