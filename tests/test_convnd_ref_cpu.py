"""CPU checks of tests/convnd_ref.py, the long-double reference of the N-d convolution sweep (tests/test_gpu_convnd.py):

  * it agrees with the Float64 oracle (oracle.dspbase.conv_nd, direct) on every shape of the sweep and on random ones, real and complex;
  * the direct kernel's element-wise bound, (m + 1) u absdot (real) / (2 m + 1) u absdot (complex), passes an emulation of the fused multiply-add chain
    in Float32 and Float64 and fails three wrong ones (a dropped term, a correlation in place of the convolution along one dimension, the two operands'
    extents swapped in the index arithmetic of the equal-count tie);
  * the case tables say what they claim: the odd padded first dimensions, the dropped singletons, the dimension counts."""
import itertools

import numpy as np
import pytest

import convnd_ref as cr
from conftest import relerr
from oracle import dspbase as odsp
from oracle.util import nextfastfft as oracle_nextfastfft

LD = cr.LD
ALL_SHAPES = cr.DIRECT_SHAPES + [(su, sv) for su, sv, _ in cr.FFT_SHAPES] + [cr.FFT_UNSUPPORTED, cr.CACHE_A, cr.CACHE_B]


def _wide(a):
    return a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)


def emu_direct(u, v, defect=None):
    """direct_nd_kernel: per output element a chain of fused multiply-adds over the smaller operand (u_big = count(u) >= count(v)).  The fma is emulated
    in the next wider format: exact products for Float32 in Float64; for Float64 the long double product is rounded once more, well inside the bound."""
    T = u.dtype
    R = T.type(0).real.dtype
    W = np.float64 if R == np.float32 else LD
    big, small = (u, v) if u.size >= v.size else (v, u)
    if defect == "tie-swapped-extents" and u.size == v.size:
        big, small = big.reshape(small.shape, order="F"), small.reshape(big.shape, order="F")
    so = tuple(a + b - 1 for a, b in zip(big.shape, small.shape))
    cplx = T.kind == "c"
    accx, accy = np.zeros(so, dtype=R), np.zeros(so, dtype=R)
    terms = list(itertools.product(*(range(e) for e in small.shape[::-1])))           # first dimension fastest
    if defect == "dropped-term":
        terms = terms[:-1]
    for m in terms:
        m = m[::-1]
        src = tuple((e - 1 - i) if (defect == "correlation" and d == 0) else i for d, (i, e) in enumerate(zip(m, small.shape)))
        at = tuple(slice(i, i + e) for i, e in zip(m, big.shape))
        s = small[src]
        if cplx:
            sx, sy, bx, by = W(s.real), W(s.imag), big.real.astype(W), big.imag.astype(W)
            inner = (-sy * by + accx[at].astype(W)).astype(R)
            accx[at] = (sx * bx + inner.astype(W)).astype(R)
            inner = (sy * bx + accy[at].astype(W)).astype(R)
            accy[at] = (sx * by + inner.astype(W)).astype(R)
        else:
            accx[at] = (W(s) * big.astype(W) + accx[at].astype(W)).astype(R)
    return (accx + 1j * accy).astype(T) if cplx else accx


@pytest.mark.parametrize("dtype", [cr.F64, cr.C64])
@pytest.mark.parametrize("su,sv", ALL_SHAPES)
def test_reference_equals_the_oracle(su, sv, dtype):
    rng = np.random.default_rng(sum(su) + 7 * sum(sv) + dtype)
    u, v = cr.operands(rng, su, sv, dtype)
    ref, absdot = cr.convnd_ref(u, v)
    want = odsp.conv_nd(_wide(u), _wide(v), "direct")
    assert ref.shape == want.shape == tuple(a + b - 1 for a, b in zip(su, sv))
    assert relerr(ref.astype(want.dtype), want) < 1e-14
    m = min(u.size, v.size)
    worst, _ = cr.direct_excess(want, ref, absdot, 2 * cr.direct_factor(u, v), 2.0 ** -53)    # the oracle: products and sums, no fma
    assert worst <= 1.0, (su, sv, m, worst)
    assert np.all(absdot.real >= np.abs(ref.real) * (1 - 1e-15))


def test_reference_on_the_literal_table():
    import conv_cases as cc
    ref, absdot = cr.convnd_ref(cc.A2, cc.B2)
    assert np.array_equal(ref.astype(np.int64), cc.EXP2)
    ref, _ = cr.convnd_ref(cc.B2, cc.A2)
    assert np.array_equal(ref.astype(np.int64), cc.EXP2)
    ref, _ = cr.convnd_ref(cc.A3, cc.B3)
    assert np.array_equal(ref.astype(np.int64), cc.EXP3)


@pytest.mark.parametrize("dtype", [cr.F32, cr.F64, cr.C32, cr.C64])
@pytest.mark.parametrize("su,sv", cr.DIRECT_SHAPES)
def test_direct_bound_passes_a_correct_emulation(su, sv, dtype):
    rng = np.random.default_rng(100 + sum(su) + dtype)
    u, v = cr.operands(rng, su, sv, dtype)
    ref, absdot = cr.convnd_ref(u, v)
    unit = float(np.finfo(u.dtype).eps) / 2
    worst, ratio = cr.direct_excess(emu_direct(u, v), ref, absdot, cr.direct_factor(u, v), unit)
    assert worst <= 1.0, (su, sv, worst, ratio)


@pytest.mark.parametrize("dtype", [cr.F32, cr.F64, cr.C32, cr.C64])
@pytest.mark.parametrize("defect,su,sv", [("dropped-term", (37, 21), (5, 9)), ("dropped-term", (2, 1, 3, 1, 2, 2, 1, 2), (1, 2, 1, 2, 2, 1, 3, 1)),
                                          ("correlation", (8, 13, 11), (3, 4, 2)), ("correlation", (7,), (3,)), ("tie-swapped-extents", (4, 6), (6, 4))])
def test_direct_bound_fails_each_wrong_emulation(defect, su, sv, dtype):
    rng = np.random.default_rng(200 + sum(su) + dtype)
    u, v = cr.operands(rng, su, sv, dtype)
    ref, absdot = cr.convnd_ref(u, v)
    unit = float(np.finfo(u.dtype).eps) / 2
    bad = emu_direct(u, v, defect)
    assert bad.shape == ref.shape
    worst, _ = cr.direct_excess(bad, ref, absdot, cr.direct_factor(u, v), unit)
    assert worst > 1.0, (defect, su, sv, worst)


def test_case_tables_say_what_they_claim():
    for su, sv, n in cr.FFT_SHAPES:
        assert cr.padded(su, sv) == n, (su, sv, cr.padded(su, sv))
        assert all(oracle_nextfastfft(a + b - 1) == cr.nextfastfft(a + b - 1) for a, b in zip(su, sv))
        assert 1 <= len(n) <= 3
    # dimension 0 padded to an odd length, in two and in three dimensions: the Hermitian length of an odd n0
    assert [n[0] for su, sv, n in cr.FFT_SHAPES[:2]] == [45, 63] and [len(n) for su, sv, n in cr.FFT_SHAPES[:2]] == [2, 3]
    # a common singleton dropped; nothing but singletons; five dimensions, two of them common singletons, three left
    assert len(cr.FFT_SHAPES[2][0]) == 3 and len(cr.FFT_SHAPES[2][2]) == 2
    assert cr.FFT_SHAPES[3][2] == (1,) and set(cr.FFT_SHAPES[3][0]) == {1}
    su, sv, n = cr.FFT_SHAPES[4]
    assert len(su) == 5 and sum(a == 1 and b == 1 for a, b in zip(su, sv)) == 2 and len(n) == 3
    assert len(cr.padded(*cr.FFT_UNSUPPORTED)) == 4
    assert cr.padded(*cr.CACHE_A) != cr.padded(*cr.CACHE_B) and cr.padded(*cr.CACHE_A) == cr.FFT_SHAPES[0][2]
    # direct: the operands swapped, the equal-count tie, the largest dimension count the kernel takes
    shapes = cr.DIRECT_SHAPES
    assert (shapes[2][1], shapes[2][0]) == shapes[1]
    assert np.prod(shapes[3][0]) == np.prod(shapes[3][1]) and shapes[3][0] != shapes[3][1]
    assert len(shapes[5][0]) == 8 and np.prod(shapes[5][0]) > np.prod(shapes[5][1])
    # more than one 256-thread block somewhere, and sizes that are no multiple of it
    assert max(np.prod([a + b - 1 for a, b in zip(su, sv)]) for su, sv in shapes) > 256
