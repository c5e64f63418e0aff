"""Guard-band tests of the spectral entry points (INTEGRATION.md "What a call touches"; tests/guard_bands.py): mdsp_welch_exec and the streaming
protocol, mdsp_stft_exec (raw columns and psd_only) and mdsp_mt_psd_exec through the C ABI with pointers INTO larger allocations.

Sizes come from the committed route table (tests/guard_cases.py spectral_cases; tests/test_guard_bands_cpu.py holds them to it): per (kind, dtype) the
smallest nfft >= 8 of every route under engine AUTO, every size of the register-resident power-of-two route, the sizes engine FUSED routes differently,
one size under engine ROCFFT.  Each plan is asked with mdsp_spectral_route_for that it takes the route the table names.

Shape per size: n = nfft and n = nfft - nfft // 4 - 1 (the frame tail is zero padding, not the following samples), noverlap = n // 2, Hanning window,
three channels of three whole frames plus hop - 1 samples that belong to no frame (an odd frame count: the last unit of a real signal has no second
frame), lds = len + 5, the input shifted by 3 elements off a 128-byte line and the output by 1, a quiet-NaN poison in front of, between and behind the
channels, another NaN pattern all over the output buffer, guards of max(4096, nfft) elements.  Welch: ldp = nout + 3.  STFT and multitaper: column stride
ldo = nout + 3, channel stride chs = K ldo + 11.  Multitaper: 5 dpss tapers (nw = 3) at three sizes per dtype.

Per call: nothing outside the outputs changed, every output written and none NaN (a sample used from outside a channel poisons a whole frame); the
bar of test_welch_vs_oracle / test_stft_spectrogram_vs_oracle / test_mt_pgram_spectrogram_vs_oracle (TOL32 / TOL64 of tests/test_gpu_parity.py,
norm-wise against the Float64 oracle); every channel bit-identical to the compact single-channel call (lds = len, ldp / ldo = nout, straight from the
allocator).  Two Welch sizes per dtype also go through reset / accumulate in two slices (2 + 1 frames: the pairs of the one-shot call) / finalize into the same
layout: bit-identical to the one-shot call on the fused kernels; the rocFFT pipeline at that size sums the frames of a call in an order that depends on
the call (tests/test_gpu_boundary.py holds it to 1e-6 / 1e-13 against the one-shot call, and so does this file; measured: Float64 differs in the last bits).

Measured on MI355X, worst norm-wise error over all sizes and routes against the bar:

                 Float32    ComplexF32   bar      Float64    ComplexF64   bar
    Welch        2.3e-7     1.8e-7       5e-6     7.3e-16    3.8e-16      1e-12
    STFT         2.0e-7     1.6e-7       5e-6     5.3e-16    4.1e-16      1e-12
    multitaper   1.3e-7     1.3e-7       5e-6     3.4e-16    2.6e-16      1e-12

Every channel was bit-identical to its compact single-channel call on every route, the rocFFT pipeline included."""
import ctypes as C

import numpy as np
import pytest

import guard_bands as gb
import guard_cases as gc
from conftest import relerr
from test_gpu_parity import TOL32, TOL64

pytestmark = pytest.mark.gpu

NCH, PAD_S, PAD_O, PAD_CH = 3, 5, 3, 11
SHIFT_IN, SHIFT_OUT = 3, 1
ENG_NAME = {gc.AUTO: "auto", gc.FUSED: "fused", gc.ROCFFT: "rocfft"}
STREAMED = (1024, 64)             # the Welch sizes that also run reset / accumulate / accumulate / finalize


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _cases(kind):
    return [pytest.param(dt, e, n, c, id=f"{np.dtype(gc.NP_DTYPE[dt]).name}-{ENG_NAME[e]}-{n}") for dt in (gc.F32, gc.F64, gc.C32, gc.C64)
            for e, n, c in gc.spectral_cases(kind, dt)]


def _signal(dt, length, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    t = np.arange(length)
    s = rng.standard_normal((NCH, length)) + 0.5 * np.sin(2 * np.pi * 0.1234 * t)
    if dt.kind == "c":
        s = s + 1j * rng.standard_normal((NCH, length))
    return s.astype(dt)


def _assert_route(kind, dtype, nfft, engine, c):
    import spectral_route_cases as src
    from dsp_jl_amd import _lib
    assert src.encode(_lib.lib(), kind, dtype, engine, [nfft])[0] == c, (kind, dtype, nfft, engine)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


def _same(a, b, what):
    same = _bits(a) == _bits(b)
    assert same.all(), (what, "first word that differs from the compact run", int(np.flatnonzero(~same.ravel())[0]))


def _in(s, length, guard):
    lay = gb.layout(length, NCH, length + PAD_S, guard, guard, SHIFT_IN, s.dtype)
    return lay, gb.to_device(gb.new_input(lay, s))


@pytest.mark.parametrize("dtype,engine,nfft,route", _cases(gc.KIND_WELCH))
def test_welch_stays_inside_its_arrays(d, dtype, engine, nfft, route):
    import torch
    from dsp_jl_amd import _lib, _dev
    from oracle import periodograms as opg, windows as ow
    lib = _lib.lib()
    dt = np.dtype(gc.NP_DTYPE[dtype])
    odt = dt.type(0).real.dtype
    tol = TOL32 if odt == np.float32 else TOL64
    _assert_route(gc.KIND_WELCH, dtype, nfft, engine, route)
    guard = max(gb.MIN_GUARD, nfft)
    worst = 0.0
    for n, nov, hop, length in gc.spectral_shapes(nfft):
        s = _signal(dt, length, nfft + n)
        cfg = d.WelchConfig(length, dt, n=n, noverlap=nov, nfft=nfft, window=d.hanning, engine=engine)
        assert cfg.engine == (gc.ROCFFT if route == "0" else gc.FUSED) and d.frame_count(length, n, nov) == 3
        nout = cfg.nout
        what = f"welch {dt.name} nfft {nfft} n {n}"
        ls, sd = _in(s, length, guard)
        lp = gb.layout(nout, NCH, nout + PAD_O, guard, guard, SHIFT_OUT, odt)
        pd = gb.to_device(gb.new_output(lp))
        _lib.check(lib.mdsp_welch_exec(cfg._h, gb.ptr(sd, ls), length, NCH, ls.ld, gb.ptr(pd, lp), lp.ld, _dev.stream_ptr()))
        after = gb.from_device(pd)
        gb.check_output(after, lp, nout, what)
        P = gb.columns(after, lp)
        for c in range(NCH):
            ref = opg.welch_pgram(s[c], n, nov, nfft=nfft, window=ow.hanning, dtype=np.float64).power
            e = relerr(P[c], ref)
            worst = max(worst, e)
            assert e < tol, (what, c, e)
            one = torch.from_numpy(np.ascontiguousarray(s[c])).cuda()
            out = torch.empty(nout, dtype=_dev.torch_dtype(odt), device="cuda")
            _lib.check(lib.mdsp_welch_exec(cfg._h, one.data_ptr(), length, 1, length, out.data_ptr(), nout, _dev.stream_ptr()))
            torch.cuda.synchronize()
            _same(P[c], out.cpu().numpy(), (what, "channel", c))
        if nfft in STREAMED:
            # the same frames in two slices of whole frames, into a fresh layout: 2 + 1 (consecutive slices overlap by n - hop samples), which keeps the
            # one-shot call's pairs -- two frames of a real signal share a transform, and another pairing rounds differently
            pd2 = gb.to_device(gb.new_output(lp))
            _lib.check(lib.mdsp_welch_reset(cfg._h))
            _lib.check(lib.mdsp_welch_accumulate(cfg._h, gb.ptr(sd, ls), n + hop, NCH, ls.ld, _dev.stream_ptr()))
            _lib.check(lib.mdsp_welch_accumulate(cfg._h, gb.ptr(sd, ls, 0, 2 * hop), n, NCH, ls.ld, _dev.stream_ptr()))
            k = C.c_int64()
            _lib.check(lib.mdsp_welch_frames_accumulated(cfg._h, C.byref(k)))
            assert k.value == 3
            _lib.check(lib.mdsp_welch_finalize(cfg._h, 0, gb.ptr(pd2, lp), lp.ld, _dev.stream_ptr()))
            after2 = gb.from_device(pd2)
            gb.check_output(after2, lp, nout, what + " streamed")
            if cfg.engine == gc.ROCFFT:
                # the rocFFT pipeline deals the frames of ONE call over 32 Float64 partial sums (abs2_accum_kernel), so frame 2 joins frame 0's partial
                # when it arrives in a call of its own: another summation order.  Held to the bar of test_welch_streaming_accumulate_equals_one_shot.
                es = relerr(gb.columns(after2, lp), P)
                assert es < (1e-6 if odt == np.float32 else 1e-13), (what, "streamed", es)
            else:
                _same(gb.columns(after2, lp), P, what + " streamed against one-shot")
    print(f"MEASURED welch {dt.name} {ENG_NAME[engine]} nfft {nfft} route {route} relerr {worst:.2e} bar {tol:.0e}")


@pytest.mark.parametrize("dtype,engine,nfft,route", _cases(gc.KIND_STFT))
def test_stft_stays_inside_its_arrays(d, dtype, engine, nfft, route):
    import torch
    from dsp_jl_amd import _lib, _dev
    from dsp_jl_amd.periodograms import _StftPlan, compute_window
    from oracle import periodograms as opg, windows as ow
    lib = _lib.lib()
    dt = np.dtype(gc.NP_DTYPE[dtype])
    cplx = dt.kind == "c"
    rdt = dt.type(0).real.dtype
    cdt = np.dtype(np.complex64 if rdt == np.float32 else np.complex128)
    tol = TOL32 if rdt == np.float32 else TOL64
    _assert_route(gc.KIND_STFT, dtype, nfft, engine, route)
    guard = max(gb.MIN_GUARD, nfft)
    worst = 0.0
    for n, nov, hop, length in gc.spectral_shapes(nfft):
        s = _signal(dt, length, nfft + n + 1)
        win, norm2 = compute_window(d.hanning, n)
        K = d.frame_count(length, n, nov)
        assert K == 3
        ls, sd = _in(s, length, guard)
        for psd_only in (0, 1):
            plan = _StftPlan(n, nov, nfft, win, 1.0 * norm2, not cplx, psd_only, dt, engine)
            assert plan.engine == (gc.ROCFFT if route == "0" else gc.FUSED)
            nout, odt = plan.nout, (rdt if psd_only else cdt)
            what = f"stft {dt.name} nfft {nfft} n {n} psd_only {psd_only}"
            ldo = nout + PAD_O
            lo = gb.layout_nested(nout, K, ldo, NCH, K * ldo + PAD_CH, guard, guard, SHIFT_OUT, odt)
            od = gb.to_device(gb.new_output(lo))
            _lib.check(lib.mdsp_stft_exec(plan._h, gb.ptr(sd, ls), length, NCH, ls.ld, gb.ptr(od, lo), ldo, K * ldo + PAD_CH, _dev.stream_ptr()))
            after = gb.from_device(od)
            gb.check_output(after, lo, nout, what)
            S = gb.columns(after, lo).reshape(NCH, K, nout)
            for c in range(NCH):
                ref = opg.stft(s[c], n, nov, psdonly=bool(psd_only), nfft=nfft, onesided=not cplx, fs=1.0, window=ow.hanning, dtype=np.float64)
                e = relerr(S[c].T, ref)
                worst = max(worst, e)
                assert e < tol, (what, c, e)
                one = torch.from_numpy(np.ascontiguousarray(s[c])).cuda()
                out = torch.empty((K, nout), dtype=_dev.torch_dtype(odt), device="cuda")
                _lib.check(lib.mdsp_stft_exec(plan._h, one.data_ptr(), length, 1, length, out.data_ptr(), nout, K * nout, _dev.stream_ptr()))
                torch.cuda.synchronize()
                _same(S[c], out.cpu().numpy(), (what, "channel", c))
            _lib.check(lib.mdsp_stft_plan_destroy(plan._h))
            plan._h = None
    print(f"MEASURED stft {dt.name} {ENG_NAME[engine]} nfft {nfft} route {route} relerr {worst:.2e} bar {tol:.0e}")


@pytest.mark.parametrize("dtype,nfft,route", [pytest.param(dt, n, c, id=f"{np.dtype(gc.NP_DTYPE[dt]).name}-{n}") for dt in (gc.F32, gc.F64, gc.C32, gc.C64)
                                              for n, c in gc.mt_sizes(dt)])
def test_multitaper_psd_stays_inside_its_arrays(d, dtype, nfft, route):
    import torch
    from dsp_jl_amd import _lib, _dev
    from oracle import multitaper as omt
    lib = _lib.lib()
    dt = np.dtype(gc.NP_DTYPE[dtype])
    odt = dt.type(0).real.dtype
    wide = np.complex128 if dt.kind == "c" else np.float64
    tol = TOL32 if odt == np.float32 else TOL64
    _assert_route(gc.KIND_STFT, dtype, nfft, gc.AUTO, route)
    guard = max(gb.MIN_GUARD, nfft)
    worst = 0.0
    for n, nov, hop, length in gc.spectral_shapes(nfft):
        s = _signal(dt, length, nfft + n + 2)
        cfg = d.MTConfig(dt, n, nfft=nfft, nw=3)
        assert cfg.ntapers == 5 and cfg.engine == gc.FUSED
        K, nout = d.frame_count(length, n, nov), cfg.nout
        assert K == 3
        what = f"multitaper {dt.name} nfft {nfft} n {n}"
        ls, sd = _in(s, length, guard)
        ldo = nout + PAD_O
        lo = gb.layout_nested(nout, K, ldo, NCH, K * ldo + PAD_CH, guard, guard, SHIFT_OUT, odt)
        od = gb.to_device(gb.new_output(lo))
        _lib.check(lib.mdsp_mt_psd_exec(cfg._h, gb.ptr(sd, ls), length, nov, NCH, ls.ld, gb.ptr(od, lo), ldo, K * ldo + PAD_CH, _dev.stream_ptr()))
        after = gb.from_device(od)
        gb.check_output(after, lo, nout, what)
        P = gb.columns(after, lo).reshape(NCH, K, nout)
        for c in range(NCH):
            ref = omt.mt_spectrogram(s[c].astype(wide), n, nov, fs=1, nfft=nfft, nw=3)[0]
            e = relerr(P[c].T, ref)
            worst = max(worst, e)
            assert e < tol, (what, c, e)
            one = torch.from_numpy(np.ascontiguousarray(s[c])).cuda()
            out = torch.empty((K, nout), dtype=_dev.torch_dtype(odt), device="cuda")
            _lib.check(lib.mdsp_mt_psd_exec(cfg._h, one.data_ptr(), length, nov, 1, length, out.data_ptr(), nout, K * nout, _dev.stream_ptr()))
            torch.cuda.synchronize()
            _same(P[c], out.cpu().numpy(), (what, "channel", c))
    print(f"MEASURED multitaper {dt.name} nfft {nfft} route {route} relerr {worst:.2e} bar {tol:.0e}")
