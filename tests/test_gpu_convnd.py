"""N-d array convolution on the device through the C ABI -- mdsp_convnd_direct (direct_nd_kernel) and mdsp_convnd_fft (pad_nd_kernel, the rocFFT N-d
plans of the ConvCache, spectrum_product_kernel, crop_nd_kernel) -- against the long-double convolution sum of tests/convnd_ref.py, all four dtypes.
Operands and output are dense (the entry points take no leading dimension): each is ONE guard_bands column, 0, 1 and 3 elements off a 128-byte line,
the inputs surrounded by a quiet-NaN poison, the output pre-filled with another; check_output holds both entry points to INTEGRATION.md "What a call
touches".  Arrays are column-major, as the library reads them.

direct   shapes convnd_ref.DIRECT_SHAPES: 1-d, 2-d and the operands swapped, the equal-count tie of u_big, 3-d, 8-d.  Element-wise
         |got - ref| <= (m + 1) u absdot (real) / (2 m + 1) u absdot (complex), m the element count of the smaller operand: the kernel is a chain of
         fused multiply-adds (tests/test_convnd_ref_cpu.py: a dropped term, a flipped dimension and swapped extents all exceed it).
         ndim = 9 is MDSP_ERR_UNSUPPORTED, an extent 0 MDSP_ERR_ARGUMENT, with the output untouched.
fft      shapes convnd_ref.FFT_SHAPES: dimension 0 padded to an odd nextfastfft length (45, 63: Hermitian length n0 / 2 + 1 of an odd n0), a common
         singleton dropped, nothing but singletons, five dimensions with two common singletons; four non-trivial dimensions are
         MDSP_ERR_UNSUPPORTED.  relerr < 2e-6 / 1e-13 (the figures of test_array_convolution) and max |got - ref| < 8 log2(padded element count)
         u max |ref|, u = 2^-24 / 2^-53.  The all-singleton pair pads to ONE element: log2 is 0 and no transform rounds anything, so there the output
         is held to what is left, the spectrum product, by the direct bound with m = 1.
cache    sizes A, A, B, A on every dtype -- the cached plans replaced and restored -- then A on a second stream right after B on the current one with no
         synchronisation in between: the four A results bit-identical and within the bounds.

Measured on MI355X, max |got - ref| / (u max |ref|) of the FFT path per padded size (bar 8 log2(count) = 55 ... 82):

                 (45, 14)   (63, 5, 4)   (6, 20)   (8, 6, 6)   (1,): u absdot, bar 2 / 3
    Float32      3.06       3.11         3.17      2.74        0.42
    Float64      4.84       5.03         3.90      2.75        0.20
    ComplexF32   3.67       2.81         2.59      2.14        0.51
    ComplexF64   3.69       3.80         2.35      3.01        0.47

and of the direct kernel at most 2.92 u absdot (bars 4 ... 91).  The A results of the cache test were bit-identical on every dtype.
"""
import ctypes as C

import numpy as np
import pytest

import convnd_ref as cr
import guard_bands as gb
from conftest import relerr, ulps_of_max

pytestmark = pytest.mark.gpu

DTYPES = [cr.F32, cr.F64, cr.C32, cr.C64]
OUT_SHIFT = {0: 1, 1: 3, 3: 0}
_REF = {}


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _name(dtype):
    return np.dtype(cr.NP_DTYPE[dtype]).name


def _unit(dtype):
    return float(np.finfo(cr.NP_DTYPE[dtype]).eps) / 2


def _case(su, sv, dtype):
    """(u, v, ref, absdot), computed once per (shape, dtype) and shared by the tests; nothing writes to them."""
    key = (su, sv, dtype)
    if key not in _REF:
        rng = np.random.default_rng(1000 * dtype + sum(su) + 13 * sum(sv) + len(su))
        u, v = cr.operands(rng, su, sv, dtype)
        ref, absdot = cr.convnd_ref(u, v)
        for a in (u, v, ref, absdot):
            a.setflags(write=False)
        _REF[key] = (u, v, ref, absdot)
    return _REF[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


class Buffers:
    """The three guarded columns of one call: u and v uploaded, the output filled."""

    def __init__(self, u, v, shift):
        T = u.dtype
        self.su, self.sv = np.array(u.shape, dtype=np.int64), np.array(v.shape, dtype=np.int64)
        self.so = tuple(int(a + b - 1) for a, b in zip(u.shape, v.shape))
        self.lu = gb.layout(u.size, 1, u.size, gb.MIN_GUARD, gb.MIN_GUARD, shift, T)
        self.lv = gb.layout(v.size, 1, v.size, gb.MIN_GUARD, gb.MIN_GUARD, OUT_SHIFT[shift], T)
        count = int(np.prod(self.so))
        self.lo = gb.layout(count, 1, count, gb.MIN_GUARD, gb.MIN_GUARD, OUT_SHIFT[OUT_SHIFT[shift]], T)
        self.ud = gb.to_device(gb.new_input(self.lu, u.ravel(order="F")))
        self.vd = gb.to_device(gb.new_input(self.lv, v.ravel(order="F")))
        self.od = gb.to_device(gb.new_output(self.lo))

    def call(self, fn, dtype, stream, ndim=None, su=None, sv=None):
        su = self.su if su is None else np.array(su, dtype=np.int64)
        sv = self.sv if sv is None else np.array(sv, dtype=np.int64)
        return fn(gb.ptr(self.ud, self.lu), su.ctypes.data_as(C.POINTER(C.c_int64)), gb.ptr(self.vd, self.lv), sv.ctypes.data_as(C.POINTER(C.c_int64)),
                  len(su) if ndim is None else ndim, dtype, gb.ptr(self.od, self.lo), stream)

    def result(self, what, written=True):
        after = gb.from_device(self.od)
        gb.check_output(after, self.lo, self.lo.n if written else 0, what)
        return gb.columns(after, self.lo)[0].reshape(self.so, order="F")


def _run(entry, su, sv, dtype, shift, what):
    from dsp_jl_amd import _lib, _dev
    u, v, ref, absdot = _case(su, sv, dtype)
    b = Buffers(u, v, shift)
    _lib.check(b.call(getattr(_lib.lib(), entry), dtype, _dev.stream_ptr()))
    return b.result(what), u, v, ref, absdot


def _fft_checks(got, u, v, ref, absdot, dtype, what):
    """-> max |got - ref| / (u max |ref|).  Asserts the bounds of the FFT path."""
    single = dtype in (cr.F32, cr.C32)
    count = int(np.prod(cr.padded(u.shape, v.shape)))
    wide = ref.astype(np.complex128 if np.iscomplexobj(ref) else np.float64)
    e = relerr(got, wide)
    assert e < (2e-6 if single else 1e-13), (what, "relerr", e)
    if count == 1:
        worst, ratio = cr.direct_excess(got, ref, absdot, cr.direct_factor(u, v), _unit(dtype))
        assert worst <= 1.0, (what, "one padded element: the spectrum product alone, error in u absdot", ratio)
        return ratio
    if single:
        ulps = ulps_of_max(got, wide)
    else:
        ulps = float(np.max(np.abs(got.astype(ref.dtype) - ref)) / (cr.LD(2.0) ** -53 * np.max(np.abs(ref))))
    assert ulps < 8 * np.log2(count), (what, "ulps of the maximum", ulps, "bar", 8 * np.log2(count))
    return ulps


# ---- direct --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("su,sv", cr.DIRECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_direct_against_the_long_double_sum(d, dtype, su, sv):
    worst = 0.0
    for shift in (0, 1, 3):
        what = f"convnd direct {_name(dtype)} {su} * {sv} shift {shift}"
        got, u, v, ref, absdot = _run("mdsp_convnd_direct", su, sv, dtype, shift, what)
        ex, ratio = cr.direct_excess(got, ref, absdot, cr.direct_factor(u, v), _unit(dtype))
        worst = max(worst, ratio)
        assert ex <= 1.0, (what, "error in u absdot", ratio, "allowed", cr.direct_factor(u, v))
    print(f"MEASURED convnd direct {_name(dtype)} {su} * {sv} worst error {worst:.2f} u absdot, bar {cr.direct_factor(u, v)}")


@pytest.mark.parametrize("entry", ["mdsp_convnd_direct", "mdsp_convnd_fft"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_argument_errors_leave_the_output_untouched(d, dtype, entry):
    from dsp_jl_amd import _lib, _dev
    fn = getattr(_lib.lib(), entry)
    u, v, _, _ = _case((7,), (3,), dtype)
    b = Buffers(u, v, 1)
    sm = _dev.stream_ptr()
    assert b.call(fn, dtype, sm, su=(7,) + (1,) * 8, sv=(3,) + (1,) * 8) == _lib.ERR_UNSUPPORTED            # ndim = 9
    assert b.call(fn, dtype, sm, su=(7, 0), sv=(3, 1)) == _lib.ERR_ARGUMENT
    assert b.call(fn, dtype, sm, su=(7, 1), sv=(0, 1)) == _lib.ERR_ARGUMENT
    assert b.call(fn, dtype, sm, ndim=0) == _lib.ERR_UNSUPPORTED
    assert b.call(fn, 4, sm) == _lib.ERR_ARGUMENT                                                            # no such dtype
    b.result(f"{entry} {_name(dtype)} argument errors", written=False)


# ---- fft -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("su,sv,n", cr.FFT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fft_against_the_long_double_sum(d, dtype, su, sv, n):
    assert cr.padded(su, sv) == n
    worst = 0.0
    for shift in (0, 1, 3):
        what = f"convnd fft {_name(dtype)} {su} * {sv} padded {n} shift {shift}"
        got, u, v, ref, absdot = _run("mdsp_convnd_fft", su, sv, dtype, shift, what)
        worst = max(worst, _fft_checks(got, u, v, ref, absdot, dtype, what))
    count = int(np.prod(n))
    bar = f"{8 * np.log2(count):.1f} u max|ref|" if count > 1 else f"{cr.direct_factor(u, v)} u absdot"
    print(f"MEASURED convnd fft {_name(dtype)} {su} * {sv} padded {n} worst error {worst:.2f}, bar {bar}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fft_over_four_dimensions_is_unsupported(d, dtype):
    from dsp_jl_amd import _lib, _dev
    su, sv = cr.FFT_UNSUPPORTED
    u, v, ref, absdot = _case(su, sv, dtype)
    b = Buffers(u, v, 3)
    assert b.call(_lib.lib().mdsp_convnd_fft, dtype, _dev.stream_ptr()) == _lib.ERR_UNSUPPORTED
    b.result(f"convnd fft {_name(dtype)} over four dimensions", written=False)
    # the direct algorithm, which the message points to, takes the pair
    _lib.check(b.call(_lib.lib().mdsp_convnd_direct, dtype, _dev.stream_ptr()))
    ex, ratio = cr.direct_excess(b.result("convnd direct over four dimensions"), ref, absdot, cr.direct_factor(u, v), _unit(dtype))
    assert ex <= 1.0, ratio


# ---- the cache -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fft_cache_replaced_restored_and_handed_between_streams(d, dtype):
    import torch
    from dsp_jl_amd import _lib, _dev
    fn = _lib.lib().mdsp_convnd_fft
    ua, va, ra, aa = _case(*cr.CACHE_A, dtype)
    ub, vb, rb, ab = _case(*cr.CACHE_B, dtype)
    runs = [("A", ua, va, 0), ("A", ua, va, 1), ("B", ub, vb, 3), ("A", ua, va, 3)]
    results = []
    for i, (name, u, v, shift) in enumerate(runs):
        b = Buffers(u, v, shift)
        _lib.check(b.call(fn, dtype, _dev.stream_ptr()))
        results.append((name, b.result(f"convnd fft cache {_name(dtype)} run {i} size {name}")))
    # A on a second stream right after B on the current one: the buffers are made first, nothing waits in between but the library itself
    bb, ba = Buffers(ub, vb, 1), Buffers(ua, va, 0)
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    st_b = bb.call(fn, dtype, _dev.stream_ptr())
    st_a = ba.call(fn, dtype, other.cuda_stream)
    _lib.check(st_b)
    _lib.check(st_a)
    results.append(("B", bb.result(f"convnd fft cache {_name(dtype)} size B before the stream change")))
    results.append(("A", ba.result(f"convnd fft cache {_name(dtype)} size A on a second stream")))
    first = {}
    for i, (name, got) in enumerate(results):
        u, v, ref, absdot = (ua, va, ra, aa) if name == "A" else (ub, vb, rb, ab)
        _fft_checks(got, u, v, ref, absdot, dtype, f"convnd fft cache {_name(dtype)} result {i} size {name}")
        if name in first:
            same = _bits(got) == _bits(first[name])
            assert same.all(), (f"cache {_name(dtype)}: result {i} of size {name} differs from the first", int((~same).sum()))
        else:
            first[name] = got
    # leave the library's stream bookkeeping on the current stream, which outlives `other`
    torch.cuda.synchronize()
    bc = Buffers(ua, va, 0)
    _lib.check(bc.call(fn, dtype, _dev.stream_ptr()))
    same = _bits(bc.result("convnd fft cache: back on the current stream")) == _bits(first["A"])
    assert same.all()
