"""Complex FIR taps on the device, through the C ABI and through the Python names.

Per row of tests/complex_tap_cases.py (as tests/test_gpu_polyphase_paths.py does for real taps): the filter reports the row's kernel path (so
no comparison here is a kernel against itself), and a stream of 3 channels (ldx > xlen) cut at {0, 1, an odd point, one before the input
deficit, n} -- with setphase on a seeded third of the cases -- gives, for every output of every channel and per real component,

    |y - ref| <= 2 (n + 1) u absdot + 4 u_min,     n = 2 tp for complex signals, tp for real ones

against the extended-precision reference of tests/complex_taps_ref.py (tests/test_complex_taps_cpu.py shows four wrong evaluations fail it).
The output buffers start as NaN with ldy > nout: the tail stays NaN, the body has none, nwritten == outputlength; after every chunk
(phi_idx, input_deficit) equal the reference's and the history is bit-identical.

Then: one NaN sample on an `exact` row leaves exactly the reference's hole; the complex-tap result equals the composition of two real-tap
filters, filt(FIRFilter(real(h)), x) + im filt(FIRFilter(imag(h)), x), within twice the bound; the Python names against the oracle norm-wise
with tests/test_gpu_parity.py's TOL32 / TOL64; large host arrays through mdsp_fir_exec_host bit-identical to the device call.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from complex_tap_cases import CASES
from complex_taps_ref import accumulation_unit, complex_taps_ref, excess, terms
from conftest import relerr
from polyphase_ref import error_bound, outputlength
from test_complex_taps_cpu import NP, case_id, case_signal, case_taps

pytestmark = pytest.mark.gpu

NCH = 3
BUDGET = 6e6           # long-double complex multiply-adds of the reference per case (tp x outputs x channels)
TOL64 = 1e-12         # tests/test_gpu_parity.py
TOL32 = 5e-6
PAIRS = [(t, x) for t in ("c32", "c64") for x in ("f32", "f64", "c32", "c64")]


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _lt():
    from dsp_jl_amd import _lib
    return {"f32": _lib.F32, "f64": _lib.F64, "c32": _lib.C32, "c64": _lib.C64}


def _out_np(td, xd):
    return np.complex128 if td == "c64" or xd in ("f64", "c64") else np.complex64


def _tol(td, xd):
    return TOL64 if _out_np(td, xd) == np.complex128 else TOL32


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_complex_tap_path_against_extended_precision_reference(d, torch, case):
    from dsp_jl_amd import _lib
    from oracle import stream_filt as osf
    lib = _lib.lib()
    L, M, hlen, td, xd, knobs, taps, expect = case
    seed = L * 7919 + M * 104729 + hlen * 31 + len(knobs) * 7 + "f32 f64 c32 c64".index(xd) + 5 * (td == "c64")
    rng = np.random.default_rng(seed)
    h = case_taps(L, M, hlen, td, taps, rng)
    xnp, ynp = NP[xd], _out_np(td, xd)
    rdt = np.float64 if ynp == np.complex128 else np.float32
    tdev = {np.complex64: torch.complex64, np.complex128: torch.complex128}
    tp = -(-hlen // L)
    # stream length: several tiles where the reference's cost allows, and always past the history and a few decimation steps
    n = int(min(200_000, max(BUDGET / (tp * NCH) * M / L, tp + 4 * M + 300)))
    x = case_signal(xd, (NCH, n), rng)
    ldx = n + 7
    xpad = np.zeros((NCH, ldx), dtype=xnp)
    xpad[:, :n] = x
    xd_dev = torch.from_numpy(xpad).to("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    u, umin = accumulation_unit(h.dtype, xnp)
    nterms = terms(tp, xnp)
    worst_ratio = 0.0
    fh = C.c_void_p()
    lt = _lt()
    try:
        _lib.check(lib.mdsp_fir_create(C.byref(fh), h.ctypes.data_as(C.c_void_p), hlen, L, M, lt[td], lt[xd], NCH))
        if dict(knobs).get("exact", 0):
            _lib.check(lib.mdsp_fir_set_exact(fh, 1))
        od = C.c_int(-1)
        _lib.check(lib.mdsp_fir_info(fh, None, None, None, None, None, C.byref(od)))
        assert od.value == (_lib.C64 if ynp == np.complex128 else _lib.C32)
        of = osf.FIRFilter(h.astype(np.complex128), Fraction(L, M))
        if seed % 3 == 0 and (L, M) != (1, 1):                       # setphase (resample's undelay! on half of them)
            phi = of.timedelay() if seed % 2 else float(rng.uniform(0, 3))
            of.setphase(phi)
            _lib.check(lib.mdsp_fir_setphase(fh, C.c_double(phi)))
        st_phi, st_def, hist = of.phi_idx, of.input_deficit, None
        path = C.c_int(-1)
        _lib.check(lib.mdsp_fir_kernel_path(fh, n, C.byref(path)))
        assert path.value == expect, f"kernel path {path.value}, the table says {expect}"
        odd = (n // 3) | 1
        hl = tp - 1
        a = 0
        for b in (0, 1, odd, None, n):
            if b is None:                                            # a chunk one sample short of the input deficit: no outputs, deficit 1
                b = odd + st_def - 1
            b = min(max(b, a), n)
            xlen = b - a
            nout = outputlength(xlen, L, M, st_phi, st_def)
            ol = C.c_int64()
            _lib.check(lib.mdsp_fir_outputlength(fh, xlen, C.byref(ol)))
            assert max(ol.value, 0) == nout
            ldy = nout + 5
            y = torch.full((NCH, ldy), complex(float("nan"), float("nan")), dtype=tdev[ynp], device="cuda")
            nw = C.c_int64(-1)
            _lib.check(lib.mdsp_fir_exec(fh, xd_dev[:, a:].data_ptr(), xlen, ldx, y.data_ptr(), nout, ldy, C.byref(nw), stream))
            torch.cuda.synchronize()
            assert nw.value == nout
            yh = y.cpu().numpy()
            assert np.isnan(yh[:, nout:].view(rdt)).all()
            ref, ad, (st_phi, st_def, hist) = complex_taps_ref(h, L, M, x[:, a:b], st_phi, st_def, hist)
            body = yh[:, :nout]
            assert not np.isnan(np.ascontiguousarray(body).view(rdt)).any()
            worst, ratio = excess(body, ref, ad, nterms, u, umin)
            worst_ratio = max(worst_ratio, ratio)
            if worst > 1.0:
                err = np.abs(body.astype(ref.dtype) - ref)
                ch, m = np.unravel_index(int(np.argmax(err)), err.shape)
                pytest.fail(f"chunk [{a}, {b}): {worst:.3g} x the bound; worst output channel {ch} index {m} of {nout}: {body[ch, m]} vs {ref[ch, m]}")
            p_, d_ = C.c_int64(), C.c_int64()
            hd = np.empty((NCH, max(hl, 1)), dtype=xnp)
            _lib.check(lib.mdsp_fir_get_state(fh, C.byref(p_), C.byref(d_), hd.ctypes.data_as(C.c_void_p)))
            assert (p_.value, d_.value) == (st_phi, st_def), (a, b)
            if hl > 0:
                assert np.array_equal(hd.view(np.uint8), np.ascontiguousarray(hist).view(np.uint8)), (a, b)
            a = b
    finally:
        if fh.value:
            _lib.check(lib.mdsp_fir_destroy(fh))
    print(f"\nmargin path={expect} taps={td} x={xd} L={L} M={M} tp={tp} max|y-ref|/(u absdot)={worst_ratio:.3f} bound/(u absdot)={2 * (nterms + 1)}")


@pytest.mark.parametrize("case", [c for c in CASES if c[5]], ids=[case_id(c) for c in CASES if c[5]])
def test_one_nan_sample_on_an_exact_row_leaves_exactly_the_reference_hole(d, torch, case):
    L, M, hlen, td, xd, knobs, taps, expect = case
    rng = np.random.default_rng(hlen + L)
    h = case_taps(L, M, hlen, td, taps, rng)
    tp = -(-hlen // L)
    n = tp + 40 * M + 500
    x = case_signal(xd, n, rng)
    k = n // 2
    x[k] = np.nan
    f = d.FIRFilter(h, Fraction(L, M), exact=True)
    y = f.filt(x)
    # the reference's windows: output m reads [history ; x] at positions idx_m - 1 .. idx_m - 1 + tp - 1, i.e. x[idx_m - tp .. idx_m - 1]
    from oracle.stream_filt import polyphase_closed_form, taps2pfb
    nout = len(y)
    phi, idx = polyphase_closed_form(1, 1, L, M, np.arange(nout, dtype=np.int64))
    pfb = taps2pfb(h, L)
    # the window of output m holds the sample (a zero tap of the bank's last, partly filled row still multiplies it: NaN either way)
    holds = (idx - tp <= k) & (k <= idx - 1)
    assert holds.any() and not holds.all()
    assert np.isnan(y.real[holds]).all() and np.isnan(y.imag[holds]).all()
    assert np.isfinite(y.real[~holds]).all() and np.isfinite(y.imag[~holds]).all()
    x0 = x.copy()
    x0[k] = 0
    ref, ad, _ = complex_taps_ref(h, L, M, x0)
    u, umin = accumulation_unit(h.dtype, x.dtype)
    assert excess(y[~holds], ref[~holds], ad[~holds], terms(tp, x.dtype), u, umin)[0] <= 1.0
    assert pfb.shape[0] == tp


@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
@pytest.mark.parametrize("L,M,hlen", [(160, 147, 5921), (1, 4, 37), (3, 1, 50), (441, 160, 16317)])
def test_complex_taps_equal_the_composition_of_two_real_tap_filters(d, torch, td, xd, L, M, hlen):
    # does not use the reference for the values: filt(FIRFilter(real(h)), x) + im filt(FIRFilter(imag(h)), x) from the real-tap kernels
    rng = np.random.default_rng(L + 13 * M + hlen + "f32 f64 c32 c64".index(xd))
    h = case_taps(L, M, hlen, td, "rand", rng)
    tp = -(-hlen // L)
    n = 6000
    x = case_signal(xd, (n, 2), rng)
    xt = torch.from_numpy(x).to("cuda")
    rt = np.float32 if td == "c32" else np.float64
    yc = d.FIRFilter(h, Fraction(L, M)).filt(xt)
    yr = d.FIRFilter(np.ascontiguousarray(h.real).astype(rt), Fraction(L, M)).filt(xt)
    yi = d.FIRFilter(np.ascontiguousarray(h.imag).astype(rt), Fraction(L, M)).filt(xt)
    assert yc.dtype == {np.complex64: torch.complex64, np.complex128: torch.complex128}[_out_np(td, xd)]
    comp = (yr + 1j * yi).cpu().numpy()
    got = yc.cpu().numpy()
    assert got.shape == comp.shape
    _, ad, _ = complex_taps_ref(h, L, M, x.T.copy())
    u, umin = accumulation_unit(h.dtype, x.dtype)
    bound_re = 2 * error_bound(ad.real.T, terms(tp, x.dtype), u, umin)
    bound_im = 2 * error_bound(ad.imag.T, terms(tp, x.dtype), u, umin)
    assert (np.abs(got.real.astype(np.longdouble) - comp.real) <= bound_re).all()
    assert (np.abs(got.imag.astype(np.longdouble) - comp.imag) <= bound_im).all()


# --- the Python names against the oracle --------------------------------------------------------------------------------------------------------

def _ctaps(rng, n, td):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(n)).astype(NP[td])


def _wide(x):
    return np.asarray(x).astype(np.complex128 if np.asarray(x).dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
def test_filt_b_a_x_and_tdfilt_with_complex_coefficients(d, torch, td, xd):
    from oracle.dspbase import filt_ba
    rng = np.random.default_rng(3 + PAIRS.index((td, xd)))
    tol = _tol(td, xd)
    b = _ctaps(rng, 23, td)
    for shape in ((500,), (500, 2)):
        x = case_signal(xd, shape, rng)
        for a in (1.0, 2.0 - 0.5j, np.array([0.5 + 0.25j])):
            av = np.atleast_1d(np.asarray(a, dtype=np.complex128))
            ref = filt_ba(b.astype(np.complex128) / av[0], np.ones(1), _wide(x))
            y = d.filt(b, a, x)
            assert isinstance(y, np.ndarray) and y.shape == x.shape
            assert relerr(y, ref) < tol, (shape, a)
            assert y.dtype == np.dtype(np.complex128)                    # (a Float64 / ComplexF64 `a` widens Float32 operands: promote_type of all three)
        y = d.filt(b, np.ones(1, dtype=b.dtype), x)
        assert y.dtype == np.dtype(_out_np(td, xd))
        yd = d.filt(b, np.ones(1, dtype=b.dtype), torch.from_numpy(x).to("cuda"))   # device in -> device out
        assert yd.is_cuda and relerr(yd.cpu().numpy(), filt_ba(b.astype(np.complex128), np.ones(1), _wide(x))) < tol
        t = d.tdfilt(b, x)
        assert t.dtype == np.dtype(_out_np(td, xd)) and relerr(t, filt_ba(b.astype(np.complex128), np.ones(1), _wide(x))) < tol
        out = np.empty(x.shape, dtype=_out_np(td, xd))
        assert d.tdfilt_(out, b, x) is out and np.array_equal(out, t)
        out2 = np.empty(x.shape, dtype=_out_np(td, xd))
        assert d.filt_(out2, b, np.ones(1, dtype=b.dtype), x) is out2 and np.array_equal(out2, t)
    with pytest.raises(d.ArgumentError):
        d.filt_(np.empty(3, dtype=np.complex128), b, 1.0, x)


@pytest.mark.parametrize("nb", [7, 66, 67, 1025])
@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
def test_filt_b_x_with_complex_taps(d, torch, td, xd, nb):
    # 7 and 66 taps: time domain, as the reference; 67 and 1025: the complex overlap-save plan (the reference stays in the time domain, filt.jl:553)
    from oracle.dspbase import filt_ba
    rng = np.random.default_rng(nb + PAIRS.index((td, xd)))
    b = _ctaps(rng, nb, td)
    for shape in ((5000,), (3000, 2)):
        x = case_signal(xd, shape, rng)
        ref = filt_ba(b.astype(np.complex128), np.ones(1), _wide(x))
        y = d.filt(b, x)
        assert isinstance(y, np.ndarray) and y.dtype == np.dtype(_out_np(td, xd)) and y.shape == x.shape
        assert relerr(y, ref) < _tol(td, xd)
        yd = d.filt(b, torch.from_numpy(x).to("cuda"))
        assert yd.is_cuda and relerr(yd.cpu().numpy(), ref) < _tol(td, xd)
        out = np.empty(x.shape, dtype=y.dtype)
        assert d.filt_(out, b, x) is out and np.array_equal(out, y)


@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
def test_df2tfilter_carries_a_complex_state(d, torch, td, xd):
    from oracle import filt as of
    from oracle.dspbase import filt_ba
    rng = np.random.default_rng(40 + PAIRS.index((td, xd)))
    tol = _tol(td, xd)
    for nb in (2, 12, 67):
        b = _ctaps(rng, nb, td)
        x = case_signal(xd, (400, 3), rng)
        f, o = d.DF2TFilter(b, dtype=NP[xd], coldims=(3,)), of.DF2TFilterFIR(b, dtype=NP[xd], coldims=(3,))
        ys, yo = [], []
        for chunk in (x[:50], x[50:51], x[51:]):                         # two chunks around a single sample
            ys.append(d.filt(f, chunk)); yo.append(o.filt(chunk))
            st = f.state.cpu().numpy()
            assert st.shape == o.state.shape and st.dtype.kind == "c" and relerr(st, o.state) < tol
        y = np.concatenate(ys)
        assert y.dtype == np.dtype(_out_np(td, xd)) and relerr(y, np.concatenate(yo)) < tol
        assert relerr(y, filt_ba(b.astype(np.complex128), np.ones(1), _wide(x))) < tol
    b = _ctaps(rng, 8, td)
    f, o = d.DF2TFilter(b, 2.0), of.DF2TFilterFIR(b / np.float64(2.0))   # (ComplexF32 ./ Float64 is ComplexF64, as in the reference)
    x = case_signal(xd, 64, rng)
    y = np.concatenate([d.filt(f, x[i:i + 1]) for i in range(64)])       # one sample at a time
    assert relerr(y, np.concatenate([o.filt(x[i:i + 1]) for i in range(64)])) < tol
    assert relerr(f.state.cpu().numpy(), o.state) < tol
    one = d.DF2TFilter(np.array([2.0 - 1j], dtype=NP[td]))              # a one-tap filter scales: mul!(out, x, b[1])
    assert relerr(d.filt(one, x), _wide(x) * (2.0 - 1j)) < tol


@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
def test_filtfilt_with_complex_taps(d, torch, td, xd):
    from oracle import filt as of
    rng = np.random.default_rng(60 + PAIRS.index((td, xd)))
    tol = _tol(td, xd)
    for nb in (10, 40):           # newb of 19 taps: time domain; of 79: the overlap-save plan
        b = _ctaps(rng, nb, td)
        for shape in ((300,), (300, 2)):
            x = case_signal(xd, shape, rng)
            y = d.filtfilt(b, x)
            assert y.shape == x.shape and y.dtype == np.dtype(_out_np(td, xd))
            assert relerr(y, of.filtfilt(b, _wide(x))) < tol                 # (newb in the taps' precision, as the reference builds it)
            y2 = d.filtfilt(b, [2.0], x)
            assert relerr(y2, of.filtfilt(b.astype(np.complex128) / 2.0, _wide(x))) < tol
            yd = d.filtfilt(b, torch.from_numpy(x).to("cuda"))
            assert yd.is_cuda and relerr(yd.cpu().numpy(), of.filtfilt(b, _wide(x))) < tol


@pytest.mark.parametrize("td,xd", PAIRS, ids=[f"{t}_{x}" for t, x in PAIRS])
def test_resample_and_stateless_filt_with_complex_taps(d, torch, td, xd):
    from oracle import design as odes, stream_filt as osf
    rng = np.random.default_rng(80 + PAIRS.index((td, xd)))
    tol = _tol(td, xd)

    def shifted(ratio):
        h = np.asarray(odes.resample_filter(ratio), dtype=np.float64)
        return (h * np.exp(2j * np.pi * 0.07 * np.arange(len(h)))).astype(NP[td])

    x = case_signal(xd, 2000, rng)
    h = shifted(Fraction(3, 2))
    y = d.resample(x, Fraction(3, 2), h)
    assert isinstance(y, np.ndarray) and y.dtype == np.dtype(_out_np(td, xd))
    assert relerr(y, osf.resample(_wide(x), Fraction(3, 2), h.astype(np.complex128))) < tol
    yd = d.resample(torch.from_numpy(x).to("cuda"), Fraction(3, 2), h)
    assert yd.is_cuda and np.array_equal(yd.cpu().numpy(), y)
    # a real filter of the same length and rate is another plan: the cache key tells them apart
    yr = d.resample(x, Fraction(3, 2), np.ascontiguousarray(h.real))
    assert relerr(yr, osf.resample(_wide(x), Fraction(3, 2), h.real.astype(np.float64))) < tol
    h = shifted(Fraction(2, 3))
    A2 = case_signal(xd, (600, 4), rng)
    A3 = case_signal(xd, (3, 500, 2), rng)
    for A, dims in ((A2, 0), (A2.T.copy(), 1), (A3, 1)):
        got = d.resample(A, Fraction(2, 3), h, dims=dims)
        want = np.apply_along_axis(lambda v: osf.resample(v, Fraction(2, 3), h.astype(np.complex128)), dims, _wide(A))
        assert got.shape == want.shape and got.dtype == np.dtype(_out_np(td, xd)) and relerr(got, want) < tol
    h = shifted(Fraction(5, 7))
    got = d.filt(h, x, Fraction(5, 7))
    assert got.dtype == np.dtype(_out_np(td, xd)) and relerr(got, osf.filt_stateless(h.astype(np.complex128), _wide(x), Fraction(5, 7))) < tol
    with pytest.raises(d.UnsupportedError, match="FIRArbitrary"):
        d.resample(x, 1.37, h)


@pytest.mark.parametrize("td,xd", [("c32", "c32"), ("c64", "f32")])
def test_large_host_arrays_take_the_host_pipeline_bit_identically(d, torch, td, xd):
    from dsp_jl_amd import _dev
    rng = np.random.default_rng(7)
    n = _dev.HOST_PIPELINE_MIN_BYTES // np.dtype(NP[xd]).itemsize + 4097
    x = case_signal(xd, n, rng)
    assert _dev.host_columns(x, NP[xd]) is not None
    h = case_taps(3, 8, 295, td, "rsf", rng)
    f1, f2 = d.FIRFilter(h, Fraction(3, 8)), d.FIRFilter(h, Fraction(3, 8))
    yh = f1.filt(x)                                                     # numpy in: mdsp_fir_exec_host
    yd = f2.filt(torch.from_numpy(x).to("cuda"))                        # the device call on a copy
    assert isinstance(yh, np.ndarray) and yh.dtype == np.dtype(_out_np(td, xd))
    assert np.array_equal(yh.view(np.uint8), yd.cpu().numpy().view(np.uint8))
    assert (f1.phi_idx, f1.input_deficit) == (f2.phi_idx, f2.input_deficit)
    assert np.array_equal(f1.history, f2.history)
