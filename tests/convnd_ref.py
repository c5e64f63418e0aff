"""Extended-precision reference of the N-d array convolution (dspbase.jl:646-660, _conv_td!: out[k] = sum_m u[m] v[k - m]) -- the yardstick of
tests/test_gpu_convnd.py for mdsp_convnd_direct and mdsp_convnd_fft; plain numpy in np.longdouble, complex operands included, held to the Float64 oracle
by tests/test_convnd_ref_cpu.py.  With each output the sum of its terms in absolute value, per real component, which the element-wise bound of the
direct kernel is stated in.  The case tables of the GPU file live here too, so that the CPU file can check what they claim about the padded sizes."""
import itertools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than Float64 here: the reference would claim precision it does not have"

F32, F64, C32, C64 = 0, 1, 2, 3
NP_DTYPE = {F32: np.float32, F64: np.float64, C32: np.complex64, C64: np.complex128}

# mdsp_convnd_direct: 1-d; 2-d and the operands swapped (u smaller than v); the equal-count tie of u_big; 3-d; 8-d (MAXD)
DIRECT_SHAPES = [
    ((7,), (3,)),
    ((37, 21), (5, 9)),
    ((5, 9), (37, 21)),
    ((4, 6), (6, 4)),
    ((8, 13, 11), (3, 4, 2)),
    ((2, 1, 3, 1, 2, 2, 1, 2), (1, 2, 1, 2, 2, 1, 3, 1)),
]
# mdsp_convnd_fft: (su, sv, padded sizes of the non-trivial dimensions).  Dimension 0 padded to an ODD nextfastfft length (Hermitian length n0 / 2 + 1 of
# an odd n0) in 2-d and 3-d; a singleton in both operands, dropped; all singletons; five dimensions of which two are common singletons
FFT_SHAPES = [
    ((40, 9), (6, 5), (45, 14)),
    ((60, 4, 3), (4, 2, 2), (63, 5, 4)),
    ((5, 1, 17), (2, 1, 3), (6, 20)),
    ((1, 1, 1), (1, 1, 1), (1,)),
    ((6, 1, 5, 1, 4), (3, 1, 2, 1, 3), (8, 6, 6)),
]
FFT_UNSUPPORTED = ((2, 3, 2, 3), (2, 2, 2, 2))          # four non-trivial dimensions
# the cache: sizes A, A, B, A, then A on a second stream right after B
CACHE_A = ((40, 9), (6, 5))
CACHE_B = ((23, 12), (4, 3))


def nextfastfft(n):
    """Smallest 7-smooth integer >= n (nextfastfft, util.jl)."""
    while True:
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def padded(su, sv):
    """The transform sizes mdsp_convnd_fft plans: nextfastfft of the output extent of every dimension that is not a singleton in both operands."""
    n = tuple(nextfastfft(a + b - 1) for a, b in zip(su, sv) if not (a == 1 and b == 1))
    return n or (1,)


def operands(rng, su, sv, dtype):
    """Noise operands of the C ABI's dtype code, Fortran order (first dimension fastest, as the library reads them)."""
    T = np.dtype(NP_DTYPE[dtype])
    out = []
    for s in (su, sv):
        a = rng.standard_normal(s)
        if T.kind == "c":
            a = a + 1j * rng.standard_normal(s)
        out.append(np.asfortranarray(a.astype(T)))
    return out


def convnd_ref(u, v):
    """(out, absdot) of shape size(u) + size(v) - 1.  Real operands: long double, absdot = sum |u| |v|.  Complex: complex long double, absdot complex
    with real part sum |u.x| |v.x| + |u.y| |v.y| (the terms of the real part) and imaginary part sum |u.x| |v.y| + |u.y| |v.x|."""
    u, v = np.asarray(u), np.asarray(v)
    assert u.ndim == v.ndim
    cplx = u.dtype.kind == "c" or v.dtype.kind == "c"
    so = tuple(a + b - 1 for a, b in zip(u.shape, v.shape))
    small, big = (v, u) if v.size <= u.size else (u, v)
    if cplx:
        bx, by = big.real.astype(LD), big.imag.astype(LD)
        re, im, are, aim = (np.zeros(so, dtype=LD) for _ in range(4))
    else:
        bx = big.astype(LD)
        re, are = np.zeros(so, dtype=LD), np.zeros(so, dtype=LD)
    for m in itertools.product(*(range(e) for e in small.shape)):
        at = tuple(slice(i, i + e) for i, e in zip(m, big.shape))
        if cplx:
            sx, sy = LD(small[m].real), LD(small[m].imag)
            re[at] += sx * bx - sy * by
            im[at] += sx * by + sy * bx
            are[at] += abs(sx) * np.abs(bx) + abs(sy) * np.abs(by)
            aim[at] += abs(sx) * np.abs(by) + abs(sy) * np.abs(bx)
        else:
            s = LD(small[m])
            re[at] += s * bx
            are[at] += abs(s) * np.abs(bx)
    if not cplx:
        return re, are
    out, absdot = np.empty(so, dtype=CLD), np.empty(so, dtype=CLD)
    out.real, out.imag, absdot.real, absdot.imag = re, im, are, aim
    return out, absdot


def direct_factor(u, v):
    """The constant of the direct kernel's bound |got - ref| <= c u absdot: the kernel is a chain of m fused multiply-adds (2 m for complex operands:
    two per term and component), m the element count of the smaller operand; gamma_m = m u / (1 - m u) <= (m + 1) u."""
    m = min(np.asarray(u).size, np.asarray(v).size)
    return (2 * m + 1) if (np.asarray(u).dtype.kind == "c" or np.asarray(v).dtype.kind == "c") else (m + 1)


def direct_excess(got, ref, absdot, factor, u):
    """max over elements and real components of |got - ref| / (factor u absdot): <= 1 passes, NaN fails; and the largest |got - ref| / (u absdot)."""
    got = np.asarray(got)
    parts = [(got.real, ref.real, absdot.real)] + ([(got.imag, ref.imag, absdot.imag)] if np.iscomplexobj(ref) else [])
    worst = 0.0
    for g, r, a in parts:
        err = np.abs(g.astype(LD) - r)
        if np.isnan(err).any():
            return float("inf"), float("inf")
        if np.any((a == 0) & (err > 0)):
            return float("inf"), float("inf")
        pos = a > 0
        if pos.any():
            worst = max(worst, float(np.max(err[pos] / (LD(u) * a[pos]))))
    return worst / factor, worst
