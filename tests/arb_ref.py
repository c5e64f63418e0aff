"""Extended-precision reference for the arbitrary-rate resampler, FIRFilter(h, rate::Float64, Nphi): ``filt!`` of stream_filt.jl:579-625
evaluated in ``np.longdouble`` / ``np.clongdouble`` from the filter state.

The trajectory is ``update!`` (stream_filt.jl:567-577) in plain Python floats from ``x_idx = input_deficit`` -- independent of the library, whose
serial loop and scan tests/test_abi_cpu.py pins to the oracle.  Output m has f = floor(acc_m), alpha = acc_m - f (exact) and the window
z[x_idx_m - 1 + k], k = 0 .. tp - 1, of [history ; x]:

    y_m = sum_k pfb[k, f] z + alpha sum_k dpfb[k, f] z

with both banks built as the reference builds them, in the taps' own precision (dpfb from [diff(h); 0] in eltype(h)), then widened exactly.
Besides the outputs it returns ``absdot_m = sum_k |pfb z| + alpha sum_k |dpfb z|`` (per real component for complex signals), the scale of the
rounding error of any evaluation of y_m, and the filter state after the chunk.
"""
from __future__ import annotations

import numpy as np

from oracle.stream_filt import taps2pfb
from polyphase_ref import CLD, LD, accumulation_unit   # noqa: F401  (re-exported: the tests take the unit from here)


def banks(h, nphi):
    """(pfb, dpfb) of FIRArbitrary(h, rate, nphi) (stream_filt.jl:106-109) in long double, from the taps as stored."""
    h = np.asarray(h)
    dh = np.concatenate([np.diff(h), np.zeros(1, dtype=h.dtype)]).astype(h.dtype)
    return taps2pfb(h, nphi).astype(LD), taps2pfb(dh, nphi).astype(LD)


def trajectory(phi_acc, input_deficit, rate, nphi, xlen):
    """(x_idx[], phi_acc[]) of every output of one chunk of xlen samples, and the state after it: the loop of stream_filt.jl:593-622 with
    update! (:567-577) in Python floats (IEEE doubles, one rounding per operation as in the reference)."""
    if xlen < input_deficit:                                           # :586-590
        return np.zeros(0, np.int64), np.zeros(0), float(phi_acc), input_deficit - xlen
    fn = float(nphi)
    delta = fn / float(rate)                                           # :114
    acc = float(phi_acc)
    x_idx = int(input_deficit)
    xs, accs = [], []
    while x_idx <= xlen:
        xs.append(x_idx)
        accs.append(acc)
        acc += delta
        if acc >= fn:
            dx, acc = divmod(acc, fn)                                  # divrem(acc, Nphi): both positive, the remainder is exact (fmod)
            x_idx += int(dx)
    return np.asarray(xs, np.int64), np.asarray(accs, np.float64), acc, x_idx - xlen


def arb_ref(h, rate, nphi, x, phi_acc=0.0, input_deficit=1, history=None):
    """One ``filt!`` call of FIRFilter(h, rate, nphi) on x of shape (n,) or (nch, n).

    State in: ``phi_acc`` (phiAccumulator) and 1-based ``input_deficit`` as the reference keeps them, ``history`` (nch, tapsPerPhi - 1) in x's
    dtype (zeros if None).  Returns ``(y, absdot, (phi_acc, input_deficit, history))``: y (nch, nout) long-double (complex) outputs, absdot of
    y's shape, the state after the chunk with the history in x's dtype (bit for bit what the filter keeps)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x[None, :] if one else x
    nch, xlen = x2.shape
    pfb, dpfb = banks(h, nphi)
    tp = pfb.shape[0]
    hl = tp - 1
    if history is None:
        history = np.zeros((nch, hl), dtype=x.dtype)
    history = np.asarray(history).reshape(nch, hl)
    z = np.concatenate([history.astype(x.dtype), x2], axis=1)          # [history ; x] per channel
    new_hist = z[:, z.shape[1] - hl:].copy() if hl > 0 else np.zeros((nch, 0), dtype=x.dtype)   # shiftin!
    cplx = x.dtype.kind == "c"
    xs, accs, acc_end, def_end = trajectory(phi_acc, input_deficit, rate, nphi, xlen)
    nout = len(xs)
    wide = CLD if cplx else LD
    y = np.zeros((nch, nout), dtype=wide)
    ad = np.zeros((nch, nout), dtype=wide)
    if nout:
        assert xs[0] >= 1 and xs[-1] <= xlen
        col = np.floor(accs).astype(np.int64)
        assert col.min() >= 0 and col.max() < nphi
        alpha = (accs - np.floor(accs)).astype(LD)                     # exact: the fractional part of a double
        zl = z.astype(wide)
        za = (np.abs(zl.real) + 1j * np.abs(zl.imag)).astype(CLD) if cplx else np.abs(zl)
        lo, up = np.zeros_like(y), np.zeros_like(y)
        alo, aup = np.zeros_like(y), np.zeros_like(y)
        start = xs - 1                                                 # window of output m: z[x_idx_m - 1 + k], k = 0 .. tp - 1
        for k in range(tp):
            pk, dk = pfb[k, col], dpfb[k, col]
            zk, zak = zl[:, start + k], za[:, start + k]
            lo += pk * zk
            up += dk * zk
            alo += np.abs(pk) * zak
            aup += np.abs(dk) * zak
        y = lo + alpha * up
        ad = alo + alpha * aup
    state = (acc_end, def_end, new_hist)
    if one:
        y, ad, state = y[0], ad[0], (state[0], state[1], state[2][0])
    return y, ad, state


def error_bound(absdot, tp, u, u_min):
    """|y - ref| <= 2 (tp + 2) u absdot + 4 u_min per (real) component: polyphase_ref.error_bound's derivation (one rounding per product, at most
    tp per sum, first order; the factor 2 for the second-order terms and any other order of summation; 4 u_min underflow) with one more rounding
    for the combination of the two sums, yUpper * alpha + yLower."""
    return 2.0 * (tp + 2) * u * absdot + 4.0 * u_min


def excess(y, ref, absdot, tp, u, u_min):
    """max over elements (and real components) of |y - ref| / bound: <= 1 passes.  Also returns the largest |y - ref| / (u absdot), the margin
    figure.  NaN in y counts as failing."""
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
