"""src/lpc.jl restated in numpy, citing file:line of the reference: Burg's method in its push/pop form and in the index form the device uses, and
Levinson's recursion.  Each once in the working precision -- with SEQUENTIAL sums, because the order of the reference's BLAS dot is not pinned -- and once
in np.longdouble.  muladd is a product and a sum (Julia leaves the fusing to the compiler); nothing here touches the library."""
import numpy as np


def work_dtype(dtype):
    """F of lpc.jl:57-58: a Float32 signal stays Float32, integers become Float64."""
    dtype = np.dtype(dtype)
    if dtype in (np.dtype(np.float32), np.dtype(np.complex64), np.dtype(np.float64), np.dtype(np.complex128), np.dtype(np.longdouble), np.dtype(np.clongdouble)):
        return dtype
    return np.dtype(np.complex128 if dtype.kind == "c" else np.float64)


def real_dtype(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def _seqsum(v):
    """A sequential sum in the dtype of v (np.cumsum adds one element after the other)."""
    return np.cumsum(v)[-1] if len(v) else v.dtype.type(0)


def _abs2(z):
    return z.real * z.real + z.imag * z.imag


def _finish(a, err, refl):
    return np.conj(a), err, refl                                                        # :91


def arburg_pushpop(x, p, dtype=None):
    """arburg (lpc.jl:53-92), literally: ef loses its last element and eb its first at every order.  dtype: the precision everything runs in (default: F)."""
    F = work_dtype(x.dtype if dtype is None else dtype)
    R = real_dtype(F)
    x = np.asarray(x).astype(F)
    with np.errstate(all="ignore"):
        unnormed = abs(_seqsum(np.conj(x) * x))                                         # :55
        err = R.type(unnormed) / R.type(len(x))                                         # :56
        ef, eb = x.copy(), x.copy()                                                     # :60-61
        a = np.zeros(p + 1, dtype=F)                                                    # :62
        a[0] = 1
        refl = np.zeros(p, dtype=F)                                                     # :64
        den = R.type(2) * R.type(unnormed)                                              # :66
        ratio = R.type(1)                                                               # :67
        for m in range(1, p + 1):                                                       # :69
            cf, ef = ef[-1], ef[:-1]                                                    # :70
            cb, eb = eb[0], eb[1:]                                                      # :71
            den = ratio * den + -(_abs2(cf) + _abs2(cb))                                # :72
            k = F.type(-2) * _seqsum(np.conj(eb) * ef) / den                            # :74
            refl[m - 1] = k                                                             # :75
            rev = a[m - 1::-1].copy() if m > 1 else a[:1].copy()                        # :77
            a[1:m + 1] = k * np.conj(rev) + a[1:m + 1]                                  # :78
            ef, eb = k * eb + ef, np.conj(k) * ef + eb                                  # :81-85
            ratio = R.type(1) - _abs2(k)                                                # :87
            err = err * ratio                                                           # :88
    return _finish(a, R.type(err), refl)


def arburg_index(x, p, dtype=None):
    """The same recursion with arrays that do not move: at order m element i of ef pairs with element i + m of eb, i = 0 .. N-m-1; cf = ef[N-m],
    cb = eb[m-1]."""
    F = work_dtype(x.dtype if dtype is None else dtype)
    R = real_dtype(F)
    x = np.asarray(x).astype(F)
    n = len(x)
    with np.errstate(all="ignore"):
        unnormed = abs(_seqsum(np.conj(x) * x))
        err = R.type(unnormed) / R.type(n)
        ef, eb = x.copy(), x.copy()
        a = np.zeros(p + 1, dtype=F)
        a[0] = 1
        refl = np.zeros(p, dtype=F)
        den = R.type(2) * R.type(unnormed)
        ratio = R.type(1)
        for m in range(1, p + 1):
            cf, cb = ef[n - m], eb[m - 1]
            den = ratio * den + -(_abs2(cf) + _abs2(cb))
            e, b = ef[:n - m], eb[m:]                                                   # views: pair i is (e[i], b[i])
            k = F.type(-2) * _seqsum(np.conj(b) * e) / den
            refl[m - 1] = k
            rev = a[m - 1::-1].copy() if m > 1 else a[:1].copy()
            a[1:m + 1] = k * np.conj(rev) + a[1:m + 1]
            e[:], b[:] = k * b + e, np.conj(k) * e + b
            ratio = R.type(1) - _abs2(k)
            err = err * ratio
    return _finish(a, R.type(err), refl)


def arburg_longdouble(x, p):
    x = np.asarray(x)
    return arburg_pushpop(x, p, np.clongdouble if x.dtype.kind == "c" else np.longdouble)


def levinson(r, p, dtype=None):
    """levinson (lpc.jl:122-145) with the generic dotu of :150-156 (a sequential muladd)."""
    r = np.asarray(r)
    F = work_dtype(r.dtype if dtype is None else dtype)
    R = real_dtype(F)
    r = r.astype(F)
    with np.errstate(all="ignore"):
        k = -r[1] / r[0]                                                                # :124
        err = (r[0] * (R.type(1) - _abs2(k))).real                                      # :126
        a = np.zeros(p, dtype=F)                                                        # :130
        refl = np.zeros(p, dtype=F)
        a[0] = refl[0] = k                                                              # :132
        for m in range(2, p + 1):                                                       # :135
            rev = a[m - 2::-1].copy()                                                   # :136
            dotu = F.type(0)
            for i in range(m - 1):                                                      # :152-154
                dotu = r[1 + i] * rev[i] + dotu
            k = -(r[m] + dotu) / err                                                    # :137
            a[:m - 1] = k * np.conj(rev) + a[:m - 1]                                    # :138
            a[m - 1] = refl[m - 1] = k                                                  # :139
            err = err * (R.type(1) - _abs2(k))                                          # :140
    return a, R.type(err), refl


def xcorr_biased_lags(x, p, dtype=None):
    """xcorr(x; scaling=:biased)[length(x):end][1:p+1] (lpc.jl:95): lags 0 .. p, r[l] = sum_i x[i+l] conj(x[i]) / N."""
    x = np.asarray(x)
    F = work_dtype(x.dtype if dtype is None else dtype)
    x = x.astype(F)
    n = len(x)
    return np.array([np.sum(x[l:] * np.conj(x[:n - l])) for l in range(p + 1)], dtype=F) / real_dtype(F).type(n)


def lpc_levinson(x, p, dtype=None):
    a, err, _ = levinson(xcorr_biased_lags(x, p, dtype), p, dtype)
    return a, err


def lfilter_ar(coeffs, s):
    """filt(1, coeffs, s) (test/lpc.jl:7): x[t] = s[t] - sum_j coeffs[j] x[t-j]."""
    coeffs = np.asarray(coeffs)
    x = np.zeros(len(s), dtype=np.result_type(coeffs.dtype, s.dtype))
    q = len(coeffs) - 1
    for t in range(len(s)):
        acc = s[t]
        for j in range(1, min(q, t) + 1):
            acc = acc - coeffs[j] * x[t - j]
        x[t] = acc
    return x
