"""Float64 reference of the 2-D periodogram: ``periodogram(s::AbstractMatrix{<:Real}; nfft, fs, radialsum, radialavg)``
(DSP.jl src/periodograms.jl:473-509) with its kernels ``fft2pow2!`` (:175-182) and ``fft2pow2radial!`` (:184-232), restated in numpy.

The transforms are numpy's Float64 FFTs of the zero-padded input (``fft`` for the full PSD, ``rfft`` along dimension 1 for the radial
forms, as the reference).  The radial loop is the reference's, vectorised: the bin of (i, j) is
``round(Int, sqrt(muladd(c1 (i-1), c1 (i-1), (kj c2)^2))) + 1`` with the fused multiply-add evaluated exactly where it can matter (see
``_fma``), the weights m1 / m2 and wave counts of :203-225, bins above ``kmax`` dropped, and the division by ``wc`` of :227-231.  The sums
run in Float64 (the reference accumulates in the output type; the tests' bounds cover the difference).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def _fma(a, b, c):
    """a * b + c rounded once (Julia's ``muladd`` fuses on FMA hardware), elementwise in Float64.  numpy has no fma: the unfused value is
    exact wherever it is the same as the fused one up to a ulp, and a ulp only moves ``round(sqrt(.))`` next to a half-integer, so those
    elements are recomputed in exact rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    x = a * b + c
    r = np.sqrt(x)
    near = np.abs(r - np.floor(r) - 0.5) < 1e-6
    if np.any(near):
        x = x.copy()
        for idx in zip(*np.nonzero(near)):
            x[idx] = float(Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return x


def scale(n1: int, n2: int):
    """(c1, c2) of :191-197 (n1, n2 = nfft)."""
    nmin = min(n1, n2)
    if n1 == nmin:
        return 1.0, n1 / n2
    return n2 / n1, 1.0


def radial_bins(n1: int, n2: int):
    """wavenum[i, j] (1-based, as the reference) for the (n1 >> 1 + 1, n2) rfft grid, kmax, and the weight of each row (1 or 2: :203-225)."""
    n1max = (n1 >> 1) + 1
    kmax = (min(n1, n2) >> 1) + 1
    c1, c2 = scale(n1, n2)
    j = np.arange(1, n2 + 1)
    kj1 = np.where(j <= (n2 >> 1) + 1, j - 1, -n2 + j - 1)
    kj2 = (kj1 * c2) ** 2
    a = c1 * np.arange(n1max, dtype=np.float64)                 # c1 * (i - 1), i = 1 .. n1max
    wavenum = np.rint(np.sqrt(_fma(a[:, None], a[:, None], kj2[None, :]))).astype(np.int64) + 1   # round(Int, .): ties to even
    weight = np.full(n1max, 2, dtype=np.int64)
    weight[0] = 1
    weight[-1] = 1 if n1 % 2 == 0 else 2
    return wavenum, kmax, weight


def wave_counts(n1: int, n2: int):
    """(kmax, wc) of fft2pow2radial!: the literal index loop's counts."""
    wavenum, kmax, weight = radial_bins(n1, n2)
    keep = wavenum <= kmax
    wc = np.bincount(wavenum[keep], weights=np.broadcast_to(weight[:, None], wavenum.shape)[keep], minlength=kmax + 1)
    return kmax, np.rint(wc[1:]).astype(np.int64)


def periodogram2_ref(s, nfft=None, fs=1.0, radialsum=False, radialavg=False):
    """periodograms.jl:473-509 in Float64.  ``s`` is the (n1, n2) matrix with Julia's index order.  Returns the (nfft1, nfft2) power, or
    the kmax radial values."""
    s = np.asarray(s)
    n1, n2 = s.shape
    N1, N2 = nfft if nfft is not None else s.shape
    if not (n1 <= N1 and n2 <= N2):
        raise ValueError("nfft must be >= size(s)")
    if not (n1 > 1 and n2 > 1):
        raise ValueError("dimensions of s must be > 1")
    if radialsum and radialavg:
        raise ValueError("radialsum and radialavg are mutually exclusive")
    r = fs * n1 * n2                                                         # norm2 = length(s)
    x = np.zeros((N1, N2), dtype=np.float64)
    x[:n1, :n2] = s
    if not (radialsum or radialavg):
        return np.abs(np.fft.fft2(x)) ** 2 * (1.0 / r)                       # fft2pow2!
    X = np.fft.rfft2(x, axes=(1, 0))                                         # rfft along dimension 1, then fft along dimension 2
    wavenum, kmax, weight = radial_bins(N1, N2)
    p = np.abs(X) ** 2 * (weight[:, None] / r)
    keep = wavenum <= kmax
    out = np.bincount(wavenum[keep], weights=p[keep], minlength=kmax + 1)[1:]
    if radialavg:
        out = out / wave_counts(N1, N2)[1]
    return out
