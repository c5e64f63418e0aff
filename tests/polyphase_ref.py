"""Extended-precision reference for FIRFilter's polyphase kernels (interpolator, decimator, rational): ``filt!`` of
stream_filt.jl:435-558 evaluated in ``np.longdouble`` / ``np.clongdouble`` from the filter state.

Output m (0-based) of a chunk uses phase phi_m and the window that ends at input position idx_m, both from the closed form
``oracle.stream_filt.polyphase_closed_form``; the window runs over [history ; x].  The taps and samples enter in their stored
precision (Float32 values widened exactly), so the reference is the exact dot product up to 2^-64 relative rounding per term.

Besides the outputs it returns, per output, ``absdot = sum_k |h_k| |x_k|`` (per real component for complex signals: the real part
of ``absdot`` bounds the real part of the output, the imaginary part the imaginary one) -- the scale of any dot product's rounding
error -- and the filter state after the chunk.
"""
from __future__ import annotations

import numpy as np

from oracle.stream_filt import polyphase_closed_form, taps2pfb

# 64-bit mantissa on x86-64 (x87 extended): 11 bits below Float64's, which the bounds of the tests take for exact
assert np.finfo(np.longdouble).nmant == 63, "the polyphase reference needs 80-bit long doubles (x86-64)"

LD, CLD = np.longdouble, np.clongdouble


def phase_bank(h, L):
    """taps2pfb(h, L) (tapsPerPhi x L, each column a flipped phase filter) in long double, from the taps as stored."""
    return taps2pfb(np.asarray(h), L).astype(LD)


def outputlength(xlen, L, M, phi_idx, input_deficit):
    """Outputs of one chunk of xlen samples from state (phi_idx, input_deficit): stream_filt.jl:317-338 in integer arithmetic."""
    if xlen < input_deficit:
        return 0
    return -(-((xlen - input_deficit + 1) * L - phi_idx + 1) // M)


def polyphase_ref(h, L, M, x, phi_idx=1, input_deficit=1, history=None):
    """One ``filt!`` call of FIRFilter(h, L//M) (L, M coprime; L = 1 decimator, M = 1 interpolator) on x of shape (n,) or (nch, n).

    State in: 1-based ``phi_idx`` and ``input_deficit`` as the reference keeps them, ``history`` (nch, tapsPerPhi - 1) in x's dtype
    (zeros if None).  Returns ``(y, absdot, (phi_idx, input_deficit, history))``: y (nch, nout) long-double (complex) outputs, absdot
    of y's shape (see the module docstring), the state after the chunk with the history in x's dtype (bit for bit what the filter keeps)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    nch, xlen = x2.shape
    pfb = phase_bank(h, L)
    tp = pfb.shape[0]
    hl = tp - 1
    if history is None:
        history = np.zeros((nch, hl), dtype=x.dtype)
    history = np.asarray(history).reshape(nch, hl)
    z = np.concatenate([history.astype(x.dtype), x2], axis=1)        # [history ; x] per channel
    new_hist = z[:, z.shape[1] - hl:].copy() if hl > 0 else np.zeros((nch, 0), dtype=x.dtype)   # shiftin!
    cplx = x.dtype.kind == "c"
    nout = outputlength(xlen, L, M, phi_idx, input_deficit)
    if nout == 0:                                                      # stream_filt.jl:483-487: the chunk only feeds the deficit
        y = np.zeros((nch, 0), dtype=CLD if cplx else LD)
        state = (phi_idx, input_deficit - xlen, new_hist)
    else:
        phi, idx = polyphase_closed_form(phi_idx, input_deficit, L, M, np.arange(nout, dtype=np.int64))
        assert idx[-1] <= xlen and idx[0] >= 1
        zl = z.astype(CLD if cplx else LD)
        za = (np.abs(zl.real) + 1j * np.abs(zl.imag)).astype(CLD) if cplx else np.abs(zl)
        y = np.zeros((nch, nout), dtype=zl.dtype)
        ad = np.zeros((nch, nout), dtype=zl.dtype)
        col = phi - 1
        start = idx - 1                                                # window of output m: z[idx_m - 1 + k], k = 0 .. tp - 1
        for k in range(tp):
            hk = pfb[k, col]
            y += hk * zl[:, start + k]
            ad += np.abs(hk) * za[:, start + k]
        p_end = (phi_idx - 1) + nout * M
        state = (p_end % L + 1, input_deficit + p_end // L - xlen, new_hist)
    if one:
        y, state = y[0], (state[0], state[1], state[2][0])
        if nout:
            ad = ad[0]
    if nout == 0:
        ad = y.copy()
    return y, ad, state


def accumulation_unit(taps_dtype, x_dtype):
    """(u, u_min) of the kernels' arithmetic: Float64 whenever taps or signal are Float64 (promote_type), Float32 otherwise."""
    dbl = np.dtype(taps_dtype) == np.float64 or np.dtype(x_dtype) in (np.dtype(np.float64), np.dtype(np.complex128))
    t = np.float64 if dbl else np.float32
    return float(np.finfo(t).eps) / 2, float(np.finfo(t).tiny)


def error_bound(absdot, tp, u, u_min):
    """|y - ref| <= 2 (tp + 1) u absdot + 4 u_min per (real) component: any order of tp products summed in precision u is within
    (tp + 1) u absdot of the exact dot product (one rounding per product, at most tp per sum, first order); the factor 2 covers the
    second-order terms and a different summation order of the kernel (the decimator kernel sums phases first), 4 u_min underflow."""
    return 2.0 * (tp + 1) * u * absdot + 4.0 * u_min


def excess(y, ref, absdot, tp, u, u_min):
    """max over elements (and real components) of |y - ref| / bound: <= 1 passes.  Also returns the largest |y - ref| / (u absdot),
    the margin figure.  NaN in y counts as failing."""
    y = np.asarray(y)
    if ref.size == 0:
        return 0.0, 0.0
    parts = [(y.real, ref.real, absdot.real)]
    if np.iscomplexobj(ref):
        parts.append((y.imag, ref.imag, absdot.imag))
    worst, ratio = 0.0, 0.0
    for yy, rr, aa in parts:
        err = np.abs(yy.astype(LD) - rr)
        b = error_bound(aa, tp, u, u_min)
        if np.isnan(err).any():
            return float("inf"), float("inf")
        worst = max(worst, float(np.max(np.where(err == 0, 0, err / np.where(b > 0, b, 1)) + np.where((err > 0) & (b == 0), np.inf, 0))))
        pos = aa > 0
        if pos.any():
            ratio = max(ratio, float(np.max(err[pos] / (u * aa[pos]))))
    return worst, ratio
