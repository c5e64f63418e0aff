"""Extended-precision reference of the multitaper cross-spectral family, stage by stage, restated from multitaper.jl:551-616 (mt_cross_power_spectra!,
mt_fft_tapered_multichannel!, cs_inner!) and :704-723 (coherence_from_cs!) in np.longdouble -- the yardstick of tests/test_gpu_mt_cross.py; plain numpy,
held to oracle.multitaper by tests/test_mt_cross_ref_cpu.py.

  demean(sig, R)                              signal .- mean(signal, dims=2), reproduced bit for bit (see below)
  tapered_spectra(sig, tapers, nfft, demean, R)   x_mt[f, k, c] = rfft(tapers[:, k] .* sig[c, :], zero-padded to nfft)
  cross_spectra(x_mt, w, freq_inds, nfft)     out[l, m, fi] = sum_k w_k x_mt[f, k, l] conj(x_mt[f, k, m]) after the 1 / sqrt(2) of row 0 and, for even
                                              nfft only, of the last row; with the |.| sums the element-wise bound is stated in
  coherence(cs)                               lower triangle |cs[c1, c2]| / sqrt(real(cs[c1, c1] cs[c2, c2])), mirrored, diagonal exactly 1

The transform is a direct DFT in long double (no FFT, so no FFT error) up to DFT_MAX points; above, numpy's Float64 rfft of the Float64 product, which
carries no long-double claim.

Demean is exact, not bounded: demean_kernel sums a channel in Float64, m = R(fl64(S / n)), out_j = R(s_j - m).  With the samples on a dyadic grid
(dyadic_signal) every partial sum is exact in Float64 in ANY order, so S is the one exact sum, and s_j - m is one correctly rounded subtraction in R."""
from functools import lru_cache

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
DFT_MAX = 2187
SQRT2 = np.sqrt(LD(2))
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than Float64 here: the reference would claim precision it does not have"


# ---- the sizes of tests/test_gpu_mt_cross.py: (engine, nfft, route character of tests/spectral_route_cases.py) per real dtype ------------------------------
# Under engine AUTO the smallest nfft >= 8 of every route of real STFT columns and the smallest odd size of every route that has one within DFT_MAX, one
# size under engine ROCFFT.  tests/test_mt_cross_ref_cpu.py holds this to guard_cases.spectral_cases and the committed route table.
F32, F64 = 0, 1
AUTO, FUSED, ROCFFT = 0, 1, 2
MULTIPASS_ROUTE = "a"
MT_CASES = {
    F32: [(AUTO, 8, "2"), (AUTO, 9, "2"), (AUTO, 11, "0"), (AUTO, 64, "3"), (AUTO, 75, "3"), (AUTO, 256, "1"), (AUTO, 2100, "5"), (AUTO, 2187, "5"),
          (AUTO, 32768, "a"), (ROCFFT, 1024, "0")],
    F64: [(AUTO, 8, "2"), (AUTO, 9, "2"), (AUTO, 11, "0"), (AUTO, 64, "3"), (AUTO, 75, "3"), (AUTO, 256, "1"), (AUTO, 2100, "5"), (AUTO, 2187, "5"),
          (AUTO, 16384, "a"), (ROCFFT, 1024, "0")],
}
NP_REAL = {F32: np.float32, F64: np.float64}


def frame_lengths(nfft, route):
    """n per size: a frame that fills the transform and one whose tail is zero padding; the multi-pass size runs full frames only."""
    return (nfft,) if route == MULTIPASS_ROUTE else (nfft, nfft - nfft // 4 - 1)


def random_tapers(rng, n, ntapers):
    """(n, ntapers) Float64 unit-norm columns without symmetry, and distinct normalisations r_k = 1 + 0.37 k."""
    t = rng.standard_normal((n, ntapers))
    return np.asfortranarray(t / np.linalg.norm(t, axis=0)), 1.0 + 0.37 * np.arange(ntapers)


def unit(R):
    """(u, u_min): unit roundoff and smallest normal number of the real type R."""
    f = np.finfo(R)
    return float(f.eps) / 2, float(f.tiny)


def dyadic_signal(rng, nch, n, R, offset=8.0):
    """(nch, n) samples on the grid on which Float64 sums are exact: multiples of 2^-12 below 2^4 (Float32) / of 2^-20 below 2^10 (Float64), plus `offset`."""
    bits, top = (12, 4) if np.dtype(R) == np.float32 else (20, 10)
    k = rng.integers(-(1 << (bits + top)) + 1, 1 << (bits + top), size=(nch, n))
    s = (k.astype(np.float64) / (1 << bits) + offset).astype(R)
    assert np.array_equal(s.astype(np.float64), k.astype(np.float64) / (1 << bits) + offset)
    return s


def demean(sig, R):
    """(nch, n) in R: exactly what demean_kernel stores for samples on the dyadic grid (and its correctly rounded model elsewhere)."""
    s = np.ascontiguousarray(sig, dtype=R)
    S = s.astype(np.float64).sum(axis=1)
    m = (S / np.float64(s.shape[1])).astype(R)
    return (s - m[:, None]).astype(R)


@lru_cache(maxsize=4)
def _dft(nfft, n):
    """(cos, sin) of 2 pi f j / nfft, f < nfft // 2 + 1, j < n, in long double; the angle is reduced in integers first."""
    two_pi = 8 * np.arctan(LD(1))
    ang = two_pi * np.arange(nfft, dtype=LD) / LD(nfft)
    ct, st = np.cos(ang), np.sin(ang)
    idx = (np.arange(nfft // 2 + 1, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % nfft
    return ct[idx], st[idx]


def tapered_spectra(sig, tapers, nfft, demean_first=False, R=np.float64):
    """x_mt[f, k, c], complex long double, of sig (nch, n) in R and tapers (n, ntapers) Float64 (mt_fft_tapered!, :143-153: the taper product, zero padding
    to nfft, rfft).  The product is taken exactly; its rounding to R on the device is one of the roundings the per-bin bound allows for."""
    s = np.ascontiguousarray(sig, dtype=R)
    if demean_first:
        s = demean(s, R)
    tapers = np.asarray(tapers, dtype=np.float64)
    nch, n = s.shape
    assert tapers.shape[0] == n and nfft >= n
    ntap = tapers.shape[1]
    if nfft > DFT_MAX:
        prod = tapers.T[None, :, :] * s.astype(np.float64)[:, None, :]                      # (nch, ntapers, n) Float64
        X = np.fft.rfft(prod, n=nfft, axis=2)
        return np.ascontiguousarray(X.transpose(2, 1, 0)).astype(CLD)
    prod = (tapers.astype(LD).T[None, :, :] * s.astype(LD)[:, None, :]).reshape(nch * ntap, n)
    c, sn = _dft(nfft, n)
    X = np.empty((nfft // 2 + 1, nch * ntap), dtype=CLD)
    X.real = c @ prod.T
    X.imag = -(sn @ prod.T)
    return np.ascontiguousarray(X.reshape(nfft // 2 + 1, nch, ntap).transpose(0, 2, 1))


def cross_spectra(x_mt, w, freq_inds, nfft):
    """(cs, absdot): cs[l, m, fi] complex long double; absdot[l, m, fi] complex, its real part sum_k w_k (|a.x| |b.x| + |a.y| |b.y|) -- the terms of
    real(cs) in absolute value -- and its imaginary part sum_k w_k (|a.y| |b.x| + |a.x| |b.y|), with a = x_mt[f, k, l], b = x_mt[f, k, m] AFTER the scaling
    of the DC row and (even nfft only) the Nyquist row by 1 / sqrt(2) (:579-582)."""
    x = np.array(x_mt, dtype=CLD)
    nout = x.shape[0]
    assert nout == nfft // 2 + 1
    x[0] = x[0] / SQRT2
    if nfft % 2 == 0:
        x[-1] = x[-1] / SQRT2
    fi = np.asarray(freq_inds, dtype=np.int64)
    assert fi.size == 0 or (fi.min() >= 0 and fi.max() < nout)
    xs = x[fi]                                                                              # (nfi, ntapers, nch)
    w = np.asarray(w, dtype=np.float64).astype(LD)
    ax, ay = xs.real, xs.imag
    aax, aay = np.abs(ax), np.abs(ay)
    e = "k,fkl,fkm->lmf"
    cs = np.empty((x.shape[2], x.shape[2], fi.size), dtype=CLD)
    cs.real = np.einsum(e, w, ax, ax) + np.einsum(e, w, ay, ay)
    cs.imag = np.einsum(e, w, ay, ax) - np.einsum(e, w, ax, ay)
    absdot = np.empty_like(cs)
    absdot.real = np.einsum(e, np.abs(w), aax, aax) + np.einsum(e, np.abs(w), aay, aay)
    absdot.imag = np.einsum(e, np.abs(w), aay, aax) + np.einsum(e, np.abs(w), aax, aay)
    return cs, absdot


def cross_bound(absdot_part, ntapers, R):
    """|got - ref| <= (ntapers + 8) u absdot + 2 u_min per real component: four roundings per term (two products or a product and an fma, the sum inside
    the complex product, the weight product with the weight's own rounding to R), ntapers - 1 of the accumulation, about three of the two divisions by the
    rounded sqrt(2) (each operand: the division, and the constant's own half ulp shared by both) -- first order, 4 + ntapers - 1 + 3 < ntapers + 8."""
    u, u_min = unit(R)
    return (ntapers + 8) * LD(u) * absdot_part + 2 * LD(u_min)


def cross_excess(got, ref, absdot, ntapers, R):
    """max over elements and real components of |got - ref| / bound (<= 1 passes; NaN fails), and the largest |got - ref| / (u absdot)."""
    got = np.asarray(got)
    if ref.size == 0:
        return 0.0, 0.0
    u, _ = unit(R)
    worst = ratio = 0.0
    for g, r, a in ((got.real, ref.real, absdot.real), (got.imag, ref.imag, absdot.imag)):
        err = np.abs(g.astype(LD) - r)
        if np.isnan(err).any():
            return float("inf"), float("inf")
        worst = max(worst, float(np.max(err / cross_bound(a, ntapers, R))))
        pos = a > 0
        if pos.any():
            ratio = max(ratio, float(np.max(err[pos] / (LD(u) * a[pos]))))
    return worst, ratio


def coherence(cs):
    """(nch, nch, nf) long double from cs[l, m, f] (coherence_from_cs!, :704-723): the lower triangle, its mirror, a diagonal of exactly 1.  0 / 0 is NaN."""
    cs = np.asarray(cs).astype(CLD)
    nch, _, nf = cs.shape
    out = np.zeros((nch, nch, nf), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c2 in range(nch):
            for c1 in range(c2 + 1, nch):
                v = cs[c1, c2]
                out[c1, c2] = np.sqrt(v.real * v.real + v.imag * v.imag) / np.sqrt((cs[c1, c1] * cs[c2, c2]).real)
                out[c2, c1] = out[c1, c2]
    for i in range(nch):
        out[i, i] = 1
    return out


def hermitian_input(cs_ld, R):
    """A long-double cross-spectral matrix rounded to complex R with exactly real diagonals: the input of the coherence cases."""
    cs = np.asarray(cs_ld).astype(np.complex64 if np.dtype(R) == np.float32 else np.complex128)
    for i in range(cs.shape[0]):
        cs[i, i] = cs[i, i].real
    return cs


def coherence_excess(got, ref, R, c=6):
    """max over the off-diagonal, finite-reference entries of |got - ref| / (c u |ref|): <= 1 passes.  NaN in got where ref is finite counts as failing.
    c = 6: numerator two products, a sum, a square root; denominator a product and a square root; one division -- 7 correctly rounded operations, the two
    under a square root halved, 5.5 u to first order."""
    u, _ = unit(R)
    got = np.asarray(got)
    nch = ref.shape[0]
    off = ~np.eye(nch, dtype=bool)[:, :, None] & np.isfinite(ref)
    if not off.any():
        return 0.0
    err = np.abs(got.astype(LD) - ref)[off]
    if np.isnan(err).any():
        return float("inf")
    b = c * LD(u) * np.abs(ref[off])
    return float(np.max(np.where(err == 0, 0, err / np.where(b > 0, b, 1)) + np.where((err > 0) & (b == 0), np.inf, 0)))


def column_excess(got, ref, nfft, R):
    """Per (taper, channel) column of x_mt[f, k, c]: max_f |got - ref| / (8 log2(nfft) u max_f |ref|); returns the largest over the columns (< 1 passes)
    and the largest max_f |got - ref| / (u max_f |ref|), the figure to record."""
    u, _ = unit(R)
    err = np.abs(np.asarray(got).astype(CLD) - ref).max(axis=0)
    scale = np.abs(ref).max(axis=0)
    if np.isnan(err).any():
        return float("inf"), float("inf")
    ulps = err / (LD(u) * scale)
    return float(np.max(ulps) / (8 * np.log2(nfft))), float(np.max(ulps))
