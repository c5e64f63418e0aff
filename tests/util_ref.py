"""numpy restatements of the COMMON DSP TOOLS and DELAY FINDING UTILITIES of the reference (src/util.jl:138-220, :316-430) for the util tests.

The sums are taken in numpy's extended precision (np.longdouble: a 64-bit significand, pairwise summation), whose own error -- below log2(n) 2^-64 relative
for sums of non-negative terms -- is far under every bound the tests state.  The arg-max rule is the reference's text, statement by statement."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision long double"


# ---- util.jl:154-178
def db2pow(a):
    return 10.0 ** (a / 10)


def db2amp(a):
    return 10.0 ** (a / 20)


def pow2db(a):
    return 10 * math.log10(a)


def amp2db(a):
    return 20 * math.log10(a)


def abs2_ld(x):
    """abs2 of every element, exact products rounded once to extended precision (Float32 products are exact there)."""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        return x.real.astype(LD) ** 2 + x.imag.astype(LD) ** 2
    return x.astype(LD) ** 2


def sumabs2(x, axis=None):
    return np.sum(abs2_ld(x), axis=axis, keepdims=axis is not None)


def rms(s, axis=None):
    """sqrt(mean(abs2, s; dims)) (util.jl:186-192), in extended precision; `axis` is kept with size 1."""
    s = np.asarray(s)
    n = s.size if axis is None else s.shape[axis]
    return np.sqrt(sumabs2(s, axis) / LD(n))


def rmsfft(f):
    """sqrt(sum(abs2, f)) / length(f) (util.jl:200)."""
    f = np.asarray(f)
    return np.sqrt(sumabs2(f)) / LD(f.size)


def abs2_own(X):
    """abs2.(X) as the reference rounds it: re*re + im*im in the element's real type, one rounding per operation."""
    X = np.asarray(X)
    re, im = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    return (re * re).astype(re.dtype) + (im * im).astype(re.dtype)


def weighted_sums(X, step):
    """The two sums of meanfreq over bins X_k (util.jl:212-218) with the terms rounded as the reference's -- pxx in the bins' real type, freqrg = step * k and
    pxx .* freqrg in Float64 -- and the additions in extended precision."""
    p = abs2_own(X).astype(np.float64)
    f = np.float64(step) * np.arange(len(p), dtype=np.float64)
    return np.sum((p * f).astype(LD)), np.sum(p.astype(LD))


def meanfreq(x, fs=2 * np.pi):
    """util.jl:211-220 with a Float64 transform of x."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    pxx = np.abs(np.fft.rfft(x)).astype(LD) ** 2
    freqrg = LD(fs) / LD(n) * np.arange(n // 2 + 1).astype(LD)
    return np.sum(pxx * freqrg) / np.sum(pxx)


def xcorr(u, v):
    """xcorr(u, v; padmode=:none) = conv(u, reverse(conj(v))) (dspbase.jl:867-898)."""
    return np.convolve(np.asarray(u), np.conj(np.asarray(v))[::-1])


def peak_rule(s, centre):
    """util.jl:338-346 on a correlation `s`, 0-based: the index of max |s|; of several, the nearest to `centre`; of two equally near, the first
    (findall lists indices in ascending order and argmin returns the first minimum).  A NaN makes maximum() NaN, findall empty and argmin throw."""
    s = np.asarray(s)
    if s.size == 0 or np.isnan(s).any():
        raise ValueError("reducing over an empty collection is not allowed")
    a = np.abs(s)
    max_idxs = np.flatnonzero(a == a.max())
    return int(max_idxs[np.argmin(np.abs(centre - max_idxs))])


def absargmax(s, centre):
    """(index, flag) as the library's ABSARGMAX reports them: flag = a NaN was seen; the index by peak_rule over the samples that are not NaN (-1: none)."""
    s = np.asarray(s)
    nan = np.isnan(s)
    if nan.all():
        return -1, int(nan.any())
    a = np.where(nan, -1.0, np.abs(s.astype(np.float64)))
    max_idxs = np.flatnonzero(a == a.max())
    return int(max_idxs[np.argmin(np.abs(centre - max_idxs))]), int(nan.any())


def finddelay(x, y):
    """util.jl:336-347; center_idx = length(x) is 1-based: len(x) - 1 here."""
    centre = len(x) - 1
    return centre - peak_rule(xcorr(y, x), centre)


def shiftsignal(x, s):
    """util.jl:357-395."""
    x = np.array(x, copy=True)
    l = len(x)
    if abs(s) > l:
        raise ValueError("The absolute value of s must not be greater than the length of x")
    y = np.zeros_like(x)
    if s >= 0:
        y[s:] = x[:l - s]
    else:
        y[:l + s] = x[-s:]
    return y


def alignsignals(x, y):
    """util.jl:404-430."""
    d = finddelay(x, y)
    return shiftsignal(x, -d), d


def absargmax_lines(x, centre):
    """absargmax of every line of an (outer, len, inner) array along axis 1, vectorised: (outer, inner, 2) of (index, flag)."""
    x = np.asarray(x)
    outer, n, inner = x.shape
    nan = np.isnan(x)
    a = np.where(nan, -1.0, np.abs(x.astype(np.float64)))
    j = np.arange(n, dtype=np.int64).reshape(1, n, 1)
    score = np.where(a == a.max(axis=1, keepdims=True), np.abs(j - centre) * (n + 1) + j, np.iinfo(np.int64).max)   # distance first, then the index
    idx = np.where(nan.all(axis=1), -1, np.argmin(score, axis=1))
    return np.stack([idx, nan.any(axis=1).astype(np.int64)], axis=-1)
