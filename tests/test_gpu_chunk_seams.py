"""Every chunked engine loop run across its chunk seams (tests/chunk_cases.py; tests/test_chunk_cases_cpu.py holds the table to the library's own chunk
arithmetic): a unit offset into the frame or block grid, a shorter last chunk, a last unit that holds one real frame, a chunk that starts in one channel and
ends in the next, the accumulate flag that flips behind the first chunk, a plan whose cached batch size changes between calls.  A dropped, doubled or
misplaced unit at a seam shows here; under the default budgets every other test of the suite runs these loops in one chunk.

Every call goes through the C ABI with pointers INTO larger allocations (tests/guard_bands.py): a quiet-NaN poison around the input columns, another NaN
pattern all over the output, so that per call nothing outside the outputs changed, every output was written and no poisoned sample was used.

Per case, under the case's budget:
  1. against the Float64 oracle at the suite's bars -- TOL32 / TOL64 norm-wise (tests/test_gpu_parity.py), PER COLUMN for STFT / spectrogram / multitaper /
     hilbert and PER BLOCK of L outputs for overlap-save, so that one bad unit is not averaged away; Float32 on the multi-pass engine also element-wise,
     ulps_of_max < 8 log2 nfft (tests/test_gpu_bigfft.py); frame counts and frequency / time axes exact;
  2. against the same call under the default budget, which mdsp_chunk_units_for says is one chunk:
       multi-pass STFT, spectrogram, multitaper and overlap-save outputs: bit for bit -- our own kernels do the arithmetic, and nothing is summed across
       units (a multitaper column adds its tapers in taper order whatever the chunk);
       multi-pass Welch sums: every bin is a sum of K non-negative doubles, (double)(Z.x^2 + Z.y^2) of bigfft.hip's last pass and of the Welch kernel the
       rows form runs (nothing signed is accumulated: read in big_pass_kernel / big_fast_kernel OUT 1, big_reduce_kernel, big_rows_to_natural_kernel,
       welch_fused_kernel), taken in two orders: per bin 1 ulp of a Float32 output, (2 K + 4) 2^-53 relative of a Float64 output;
       rocFFT paths: no assertion -- rocFFT's arithmetic is not known to be independent of the batch count; whether the results matched is printed.
     The two fixed budgets (rocFFT overlap-save, hilbert) have no other budget to compare against.
  3. overlap-save block ranges (mdsp_ols_exec_range) that start inside the whole call's second chunk: bit-identical to the whole-column call.

Plan re-use: the rocFFT Welch, STFT and overlap-save plans and hilbert's cached transforms run a short call, the long one and the short one again; every
result meets the oracle bar.

Measured on MI355X, worst over the cases of a family (norm-wise per channel / column / block; ulps_of_max where it is asserted, bar 8 log2 nfft = 112 .. 152):

    loop                                     Float32 / ComplexF32          Float64 / ComplexF64     bar
    rocFFT Welch                             8.9e-8 .. 1.3e-7              3.6e-16 .. 4.6e-16       5e-6 / 1e-12
    rocFFT STFT, spectrogram, multitaper     1.4e-7 .. 2.7e-7              3.6e-16 .. 6.8e-16
    rocFFT overlap-save (per block)          2.7e-7                        1.2e-15
    hilbert (per column)                     2.3e-7 .. 2.9e-7              6.7e-16 .. 6.8e-16
    multi-pass Welch sums, rows form         8.7e-8 .. 1.5e-7, 2.5 ulps    8.3e-17 .. 2.4e-16
    multi-pass columns, multitaper           1.4e-7 .. 3.2e-7, 5.8 ulps    3.7e-16 .. 4.8e-16
    multi-pass overlap-save (per block)      2.4e-7                        --

Against one chunk: every multi-pass result was bit for bit, the Welch sums included (at these shapes the groups of a launch hold one unit each, so both
budgets add the units in the same order; the bound is what the arithmetic guarantees).  On the rocFFT engine the STFT, spectrogram, multitaper and Float32
Welch results matched in bits; the Float64 and ComplexF64 Welch sums differed in the last bits (1.0e-16 .. 2.1e-16 norm-wise), the 32 partial sums of a
launch being dealt per chunk.  The two short calls of every re-used plan matched in bits.

With five seam defects planted in a scratch build -- the last frame of every later chunk left out of the rocFFT Welch sums, `add` not set behind the first
chunk of the multi-pass Welch sums, big_untangle_kernel given c0 = 0, hilbert's and the rocFFT overlap-save's later chunks stored one unit off -- every
case that runs one of those lines failed (25 of 56: 6 + 7 + 6 + 2 + 4; "unwritten: column 16, element 0" for the columns, 2 % .. 97 % norm-wise for the
sums) and no other.
"""
import ctypes as C
import math
import zlib

import numpy as np
import pytest

import chunk_cases as cc
import guard_bands as gb
from conftest import relerr, ulps_of_max
from test_gpu_parity import TOL32, TOL64

pytestmark = pytest.mark.gpu

SHIFT_IN, SHIFT_OUT = 3, 1            # base offsets in elements off a 128-byte line
PAD_CH = 11                           # extra elements between the channels of a strided STFT output
REUSE = dict(cc.REUSE)
BUDGET_KNOBS = ("MDSP_ROCFFT_CHUNK_MIB", "MDSP_BIG_CHUNK_MIB")


def _default_budget(launch):
    """A case's launch knobs without the budget: the call the chunked one is compared against differs from it in the budget alone."""
    return {k: v for k, v in launch.items() if k not in BUDGET_KNOBS}


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


class _Knobs:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        from dsp_jl_amd import _lib
        for k, v in self.knobs.items():
            _lib.set_tunable(k, v)

    def __exit__(self, *exc):
        from dsp_jl_amd import _lib
        for k in self.knobs:
            _lib.set_tunable(k, None)


def _chunks(case, n, units, cap=None):
    """Chunks of a loop over `units` units under the tunables as they stand (the library's own query)."""
    from dsp_jl_amd import _lib
    c = C.c_int64()
    _lib.check(_lib.lib().mdsp_chunk_units_for(cc.LOOP_KIND[case.loop], case.dtype, n, units if cap is None else cap, C.byref(c)))
    return -(-units // c.value)


def _rng(case):
    return np.random.default_rng(zlib.crc32(case.id.encode()))


def _tol(dtype):
    return TOL64 if cc.is_double(dtype) else TOL32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


def _same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _assert_same(a, b, what):
    same = _bits(a) == _bits(b)
    assert same.all(), (what, "first word that differs", int(np.flatnonzero(~same.ravel())[0]), "of", same.size, "differing", int((~same).sum()))


def _rowwise_relerr(got, ref):
    """Worst norm-wise relative error over the rows of two (rows, n) arrays."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    wide = np.complex128 if (got.dtype.kind == "c" or ref.dtype.kind == "c") else np.float64
    num = np.linalg.norm(got.astype(wide) - ref.astype(wide), axis=1)
    den = np.linalg.norm(ref.astype(wide), axis=1)
    assert (den > 0).all()
    return float(np.max(num / den))


# ======================================================================================================================================================
# Welch / STFT / spectrogram / multitaper
# ======================================================================================================================================================
def _spectral_signal(case):
    sh = case.shape
    dt = np.dtype(cc.NP_DTYPE[case.dtype])
    length = cc.spectral_length(sh)
    rng = _rng(case)
    s = rng.standard_normal((sh["nch"], length)) + 0.5 * np.sin(2 * np.pi * 0.1234 * np.arange(length))
    if dt.kind == "c":
        s = s + 1j * rng.standard_normal((sh["nch"], length))
    return s.astype(dt)


_TAPERS = {}


def _tapers(sh):
    """(n, ntapers) dpss tapers, shared by the plan and the oracle."""
    from oracle import windows as ow
    key = (sh["n"], sh["nw"], sh["ntapers"])
    if key not in _TAPERS:
        _TAPERS[key] = np.ascontiguousarray(ow.dpss(*key))
    return _TAPERS[key]


def _spectral_plan(d, case):
    """The plan of a case, made under its `create` knobs; the engine and the route are what the table names (tests/test_chunk_cases_cpu.py)."""
    from dsp_jl_amd.periodograms import _StftPlan, compute_window
    sh = case.shape
    dt = np.dtype(cc.NP_DTYPE[case.dtype])
    engine = cc.ROCFFT if case.loop.startswith("rocfft") else cc.FUSED
    with _Knobs(case.create):
        if case.op in ("welch", "stream"):
            plan = d.WelchConfig(cc.spectral_length(sh), dt, n=sh["n"], noverlap=sh["noverlap"], nfft=sh["nfft"], window=d.hanning, onesided=sh["onesided"], fs=1,
                                 engine=engine)
        elif case.op == "mt":
            plan = d.MTConfig(dt, sh["n"], nfft=sh["nfft"], window=_tapers(sh), nw=sh["nw"], ntapers=sh["ntapers"], onesided=sh["onesided"], engine=engine)
        else:
            win, norm2 = compute_window(d.hanning, sh["n"])
            plan = _StftPlan(sh["n"], sh["noverlap"], sh["nfft"], win, 1.0 * norm2, sh["onesided"], int(case.op == "psd"), dt, engine)
    assert plan.engine == engine, (case.id, plan.engine)
    return plan


def _spectral_call(d, case, plan, s, K):
    """The case's call on the first K frames of every channel of s; returns (nch, nout) for Welch, (nch, K, nout) for columns."""
    from dsp_jl_amd import _lib, _dev
    lib = _lib.lib()
    sh = case.shape
    dt = s.dtype
    rdt = dt.type(0).real.dtype
    cdt = np.dtype(np.complex64 if rdt == np.float32 else np.complex128)
    nch, n, nov, hop = sh["nch"], sh["n"], sh["noverlap"], sh["n"] - sh["noverlap"]
    length = cc.spectral_length(sh, K)
    assert d.frame_count(length, n, nov) == K
    guard = max(gb.MIN_GUARD, sh["nfft"])
    ls = gb.layout(length, nch, length + 5, guard, guard, SHIFT_IN, dt)
    sd = gb.to_device(gb.new_input(ls, s[:, :length]))
    nout = plan.nout
    what = f"{case.id} K {K}"
    if case.op in ("welch", "stream"):
        lp = gb.layout(nout, nch, nout + 3, guard, guard, SHIFT_OUT, rdt)
        pd = gb.to_device(gb.new_output(lp))
        if case.op == "welch":
            _lib.check(lib.mdsp_welch_exec(plan._h, gb.ptr(sd, ls), length, nch, ls.ld, gb.ptr(pd, lp), lp.ld, _dev.stream_ptr()))
        else:
            assert nch == 1 and K == sum(sh["slices"])
            _lib.check(lib.mdsp_welch_reset(plan._h))
            f0 = 0
            for k in sh["slices"]:      # whole frames: consecutive slices overlap by n - hop samples
                _lib.check(lib.mdsp_welch_accumulate(plan._h, gb.ptr(sd, ls, 0, f0 * hop), (k - 1) * hop + n, 1, ls.ld, _dev.stream_ptr()))
                f0 += k
            got = C.c_int64()
            _lib.check(lib.mdsp_welch_frames_accumulated(plan._h, C.byref(got)))
            assert got.value == K
            _lib.check(lib.mdsp_welch_finalize(plan._h, 0, gb.ptr(pd, lp), lp.ld, _dev.stream_ptr()))
        after = gb.from_device(pd)
        gb.check_output(after, lp, nout, what)
        return gb.columns(after, lp)
    odt = cdt if case.op == "stft" else rdt
    ldo = nout + sh["ldo_pad"]
    chs = K * ldo + (PAD_CH if sh["ldo_pad"] else 0)
    lo = gb.layout_nested(nout, K, ldo, nch, chs, guard, guard, SHIFT_OUT, odt)
    od = gb.to_device(gb.new_output(lo))
    if case.op == "mt":
        _lib.check(lib.mdsp_mt_psd_exec(plan._h, gb.ptr(sd, ls), length, nov, nch, ls.ld, gb.ptr(od, lo), ldo, chs, _dev.stream_ptr()))
    else:
        _lib.check(lib.mdsp_stft_exec(plan._h, gb.ptr(sd, ls), length, nch, ls.ld, gb.ptr(od, lo), ldo, chs, _dev.stream_ptr()))
    after = gb.from_device(od)
    gb.check_output(after, lo, nout, what)
    return gb.columns(after, lo).reshape(nch, K, nout)


def _spectral_oracle(case, s, K):
    from oracle import multitaper as omt, periodograms as opg, windows as ow
    sh = case.shape
    length = cc.spectral_length(sh, K)
    n, nov, nfft = sh["n"], sh["noverlap"], sh["nfft"]
    assert opg.frame_count(length, n, nov) == K
    out = []
    if case.op == "mt":
        wide = np.complex128 if s.dtype.kind == "c" else np.float64
        mc = omt.MTConfig(wide, n, fs=1, nfft=nfft, window=_tapers(sh), ntapers=sh["ntapers"], onesided=sh["onesided"])
    for c in range(sh["nch"]):
        x = s[c, :length]
        if case.op in ("welch", "stream"):
            out.append(opg.welch_pgram(x, n, nov, nfft=nfft, window=ow.hanning, onesided=sh["onesided"], fs=1.0, dtype=np.float64).power)
        elif case.op == "mt":
            out.append(omt.mt_spectrogram(x.astype(wide), config=omt.MTSpectrogramConfig(length, mc, nov))[0].T)
        else:
            out.append(opg.stft(x, n, nov, psdonly=case.op == "psd", nfft=nfft, onesided=sh["onesided"], fs=1.0, window=ow.hanning, dtype=np.float64).T)
    return np.stack(out)


def _spectral_check(case, got, ref):
    """The oracle bars; returns (worst norm-wise error, worst ulps_of_max or 0)."""
    f32 = not cc.is_double(case.dtype)
    big = case.loop.startswith("big")
    tol = _tol(case.dtype)
    assert got.shape == ref.shape, (case.id, got.shape, ref.shape)
    assert got.dtype == np.dtype(cc.NP_DTYPE[case.dtype]).type(0).real.dtype or case.op == "stft"
    if got.ndim == 2:                                        # Welch: per channel
        e = _rowwise_relerr(got, ref)
        u = max(ulps_of_max(got[c], ref[c]) for c in range(got.shape[0])) if f32 and big else 0.0
    else:                                                    # columns: per column of every channel
        g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
        e = _rowwise_relerr(g2, r2)
        u = ulps_of_max(g2, r2, axis=1) if f32 and big else 0.0
    assert e < tol, (case.id, "norm-wise", e)
    if f32 and big:
        assert u < 8.0 * math.log2(case.shape["nfft"]), (case.id, "ulps of max", u)
    return e, u


@pytest.mark.parametrize("cid", [c.id for c in cc.SPECTRAL])
def test_spectral_loop_across_chunk_seams(d, cid):
    from oracle import util as outil
    case = cc.BY_ID[cid]
    sh = case.shape
    K = sh["K"]
    s = _spectral_signal(case)
    plan = _spectral_plan(d, case)
    freq = outil.rfftfreq(sh["nfft"], 1.0) if sh["onesided"] else outil.fftfreq(sh["nfft"], 1.0)
    assert np.array_equal(plan.freq, freq) if hasattr(plan, "freq") else True
    units = cc.spectral_units(case)
    shorts = []
    with _Knobs(case.launch):
        assert max(_chunks(case, sh["nfft"], u) for u in units) == case.expect["chunks"], cid
        if cid in REUSE:            # the plan's cached batch: short, long, short again
            shorts.append(_spectral_call(d, case, plan, s, REUSE[cid]))
        got = _spectral_call(d, case, plan, s, K)
        if cid in REUSE:
            shorts.append(_spectral_call(d, case, plan, s, REUSE[cid]))
    ref = _spectral_oracle(case, s, K)
    e, u = _spectral_check(case, got, ref)
    for sg in shorts:
        _spectral_check(case, sg, _spectral_oracle(case, s, REUSE[cid]))
    if shorts:
        print(f"MEASURED chunk-seams {cid} re-used plan: the two short calls {'matched' if _same(*shorts) else 'differ in bits'}")
    # the same call under the default budget: one chunk
    with _Knobs(_default_budget(case.launch)):
        assert all(_chunks(case, sh["nfft"], u) == 1 for u in units), cid
        one = _spectral_call(d, case, plan, s, K)
    _spectral_check(case, one, ref)
    if case.loop.startswith("rocfft"):
        verdict = "matched" if _same(got, one) else f"differ in bits (relerr {relerr(got, one):.1e})"
    elif case.op in ("welch", "stream"):
        a, b = got.astype(np.float64), one.astype(np.float64)
        if cc.is_double(case.dtype):
            bound = (2 * K + 4) * 2.0 ** -53 * np.abs(b)
        else:
            bound = np.spacing(np.maximum(np.abs(got), np.abs(one))).astype(np.float64)      # 1 ulp of the Float32 output
        worst = float(np.max(np.abs(a - b) / np.where(bound > 0, bound, 1.0)))
        assert (np.abs(a - b) <= bound).all(), (cid, "Welch sums against one chunk, in units of the bound", worst)
        verdict = f"within {worst:.2f} of the per-bin bound" + (", bit for bit" if _same(got, one) else "")
    else:
        _assert_same(got, one, (cid, "against one chunk"))
        verdict = "bit for bit"
    print(f"MEASURED chunk-seams {cid} chunks {case.expect['chunks']} relerr {e:.2e} ulps {u:.1f} bar {_tol(case.dtype):.0e}; one chunk: {verdict}")


def test_spectrogram_axes_are_exact_under_a_small_budget(d):
    """spectrogram() itself on the rocFFT engine across chunk seams: power as the C ABI call gives it, time and freq exactly the oracle's."""
    from oracle import periodograms as opg, windows as ow
    case = cc.BY_ID["rocfft-psd-float32"]
    sh = case.shape
    s = _spectral_signal(case)[0]
    with _Knobs(case.launch):
        sp = d.spectrogram(s, sh["n"], sh["noverlap"], nfft=sh["nfft"], window=d.hanning, fs=3.0, engine=d.ENGINE_ROCFFT)
    rs = opg.spectrogram(s, sh["n"], sh["noverlap"], nfft=sh["nfft"], window=ow.hanning, fs=3.0, dtype=np.float64)
    assert sp.power.shape == rs.power.shape == (sh["nfft"] // 2 + 1, sh["K"])
    assert np.array_equal(sp.time, rs.time) and np.array_equal(sp.freq, rs.freq)
    assert _rowwise_relerr(np.asarray(sp.power).T, rs.power.T) < TOL32


# ======================================================================================================================================================
# overlap-save
# ======================================================================================================================================================
def _ols_reference(b, x, nout):
    wide = np.complex128 if b.dtype.kind == "c" else np.float64
    xc, bw = x.astype(wide), b.astype(wide)
    if len(b) < 64:
        return np.convolve(xc, bw)[:nout]
    nf = 1 << int(np.ceil(np.log2(len(x) + len(b) - 1)))
    if wide is np.float64:
        return np.fft.irfft(np.fft.rfft(xc, nf) * np.fft.rfft(bw, nf), nf)[:nout]
    return np.fft.ifft(np.fft.fft(xc, nf) * np.fft.fft(bw, nf))[:nout]


def _blockwise_relerr(y, ref, L):
    """Worst norm-wise relative error over the blocks of L outputs (the last one shorter)."""
    full = (len(ref) // L) * L
    e = _rowwise_relerr(y[:full].reshape(-1, L), ref[:full].reshape(-1, L)) if full else 0.0
    return max(e, relerr(y[full:], ref[full:])) if full < len(ref) else e


def _ols_call(case, plan, x, nout, guard):
    from dsp_jl_amd import _lib, _dev
    ncols, nx = x.shape
    pad = case.shape["ld_pad"]
    lx = gb.layout(nx, ncols, nx + pad, guard, guard, SHIFT_IN, x.dtype)
    ly = gb.layout(nout, ncols, nout + pad + 2, guard, guard, SHIFT_OUT, x.dtype)
    xd, yd = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(ly))
    _lib.check(_lib.lib().mdsp_ols_exec(plan._h, gb.ptr(xd, lx), nx, ncols, lx.ld, gb.ptr(yd, ly), nout, ly.ld, _dev.stream_ptr()))
    after = gb.from_device(yd)
    gb.check_output(after, ly, nout, f"{case.id} nx {nx}")
    return gb.columns(after, ly)


def _ols_range_call(case, plan, x, nout, L, g0, guard):
    """Blocks g0 .. of one column from the slice of the signal they read, into a buffer of their own."""
    from dsp_jl_amd import _lib, _dev
    nx, nb = len(x), case.shape["nb"]
    nblocks = -(-nout // L)
    lo, hi = max(0, g0 * L - (nb - 1)), min(nx, nblocks * L)
    o0 = g0 * L
    lx = gb.layout(hi - lo, 1, hi - lo + 5, guard, guard, SHIFT_IN, x.dtype)
    ly = gb.layout(nout - o0, 1, nout - o0 + 7, guard, guard, SHIFT_OUT, x.dtype)
    xd, yd = gb.to_device(gb.new_input(lx, x[lo:hi])), gb.to_device(gb.new_output(ly))
    _lib.check(_lib.lib().mdsp_ols_exec_range(plan._h, gb.ptr(xd, lx), lo, hi - lo, nx, gb.ptr(yd, ly), g0, nblocks - g0, nout, _dev.stream_ptr()))
    after = gb.from_device(yd)
    gb.check_output(after, ly, nout - o0, f"{case.id} blocks from {g0}")
    return gb.columns(after, ly)[0]


@pytest.mark.parametrize("cid", [c.id for c in cc.OLS])
def test_overlap_save_loop_across_chunk_seams(d, cid):
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    case = cc.BY_ID[cid]
    sh = case.shape
    dt = np.dtype(cc.NP_DTYPE[case.dtype])
    rdt = dt.type(0).real.dtype
    tol = _tol(case.dtype)
    rng = _rng(case)
    nx, nout = cc.ols_sizes(case)
    b = (rng.standard_normal(sh["nb"]) / np.sqrt(sh["nb"])).astype(rdt)
    x = rng.standard_normal((sh["ncols"], nx)).astype(rdt)
    if dt.kind == "c":
        b = (b + 1j * (rng.standard_normal(sh["nb"]) / np.sqrt(sh["nb"]))).astype(dt)
        x = (x + 1j * rng.standard_normal((sh["ncols"], nx))).astype(dt)
    with _Knobs(case.create):
        plan = OlsPlan(b, sh["nfft"], sh["nx_hint"], sh["mode"], sh["engine"])
    en, el, ep = C.c_int64(), C.c_int64(), C.c_int()
    _lib.check(_lib.lib().mdsp_ols_plan_geometry(plan._h, C.byref(en), C.byref(el), C.byref(ep)))
    assert (en.value, el.value, ep.value, plan.engine) == case.expect["geometry"][:4], cid
    N, L = en.value, el.value
    guard = max(gb.MIN_GUARD, N)
    walk, cap = cc.ols_units(case)
    shorts = []
    if cid in REUSE:
        nshort = REUSE[cid] * L - 11
    with _Knobs(case.launch):
        assert _chunks(case, N, walk, cap) == case.expect["chunks"], cid
        if cid in REUSE:
            shorts.append(_ols_call(case, plan, x[:, :nshort], nshort, guard))
        y = _ols_call(case, plan, x, nout, guard)
        if cid in REUSE:
            shorts.append(_ols_call(case, plan, x[:, :nshort], nshort, guard))
        yr = _ols_range_call(case, plan, x[0], nout, L, sh["range_from"], guard) if sh["range_from"] is not None else None
    refs = [_ols_reference(b, x[c], nout) for c in range(sh["ncols"])]
    worst = max(_blockwise_relerr(y[c], refs[c], L) for c in range(sh["ncols"]))
    assert worst < tol, (cid, "per block of L outputs", worst)
    for ys in shorts:
        for c in range(sh["ncols"]):
            assert _blockwise_relerr(ys[c], refs[c][:nshort], L) < tol, (cid, "short call of the re-used plan", c)
    verdict = ""
    if shorts:
        verdict += f"; re-used plan: the two short calls {'matched' if _same(*shorts) else 'differ in bits'}"
    if case.loop != "rocfft_ols":
        with _Knobs(_default_budget(case.launch)):
            assert _chunks(case, N, walk, cap) == 1, cid
            one = _ols_call(case, plan, x, nout, guard)
            yr1 = _ols_range_call(case, plan, x[0], nout, L, sh["range_from"], guard) if yr is not None else None
        _assert_same(y, one, (cid, "against one chunk"))
        verdict += "; one chunk: bit for bit"
        if yr is not None:
            g0 = sh["range_from"]
            _assert_same(yr, y[0, g0 * L:], (cid, "block range against the whole column"))
            _assert_same(yr1, yr, (cid, "block range against one chunk"))
            verdict += f"; blocks from {g0}: bit for bit"
    print(f"MEASURED chunk-seams {cid} chunks {case.expect['chunks']} worst block relerr {worst:.2e} bar {tol:.0e}{verdict}")


# ======================================================================================================================================================
# hilbert
# ======================================================================================================================================================
def _hilbert_call(case, x, guard):
    from dsp_jl_amd import _lib, _dev
    ncols, n = x.shape
    pad = case.shape["ld_pad"]
    cdt = np.dtype(np.complex64 if x.dtype == np.float32 else np.complex128)
    lx = gb.layout(n, ncols, n + pad, guard, guard, SHIFT_IN if pad else 0, x.dtype)
    lo = gb.layout(n, ncols, n + (3 if pad else 0), guard, guard, SHIFT_OUT if pad else 0, cdt)
    xd, od = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(lo))
    _lib.check(_lib.lib().mdsp_hilbert(gb.ptr(xd, lx), n, ncols, lx.ld, _lib.F64 if x.dtype == np.float64 else _lib.F32, gb.ptr(od, lo), lo.ld, _dev.stream_ptr()))
    after = gb.from_device(od)
    del xd, od
    gb.check_output(after, lo, n, f"{case.id} {ncols} columns")
    return gb.columns(after, lo)


def _hilbert_worst(got, x):
    """Worst per-column norm-wise error against the Float64 analytic signal (util.jl:31-87), a slab of columns at a time."""
    n = x.shape[1]
    worst = 0.0
    for c0 in range(0, x.shape[0], 4096):
        X = np.zeros((min(4096, x.shape[0] - c0), n), dtype=np.complex128)
        X[:, : n // 2 + 1] = np.fft.rfft(x[c0:c0 + 4096].astype(np.float64), axis=1)
        X[:, 1: n // 2 + (n & 1)] *= 2
        worst = max(worst, _rowwise_relerr(got[c0:c0 + 4096], np.fft.ifft(X, axis=1)))
    return worst


@pytest.mark.parametrize("cid", [c.id for c in cc.HILBERT])
def test_hilbert_loop_across_batch_seams(d, cid):
    case = cc.BY_ID[cid]
    sh = case.shape
    rdt = np.dtype(cc.NP_DTYPE[case.dtype])
    tol = _tol(case.dtype)
    assert _chunks(case, sh["n"], sh["ncols"]) == case.expect["chunks"], cid
    x = _rng(case).standard_normal((sh["ncols"], sh["n"])).astype(rdt)
    guard = gb.MIN_GUARD
    shorts = []
    if cid in REUSE:          # the cached transforms are keyed by (length, batch): short, long, short again rebuilds them twice
        shorts.append(_hilbert_call(case, x[:REUSE[cid]], guard))
    got = _hilbert_call(case, x, guard)
    if cid in REUSE:
        shorts.append(_hilbert_call(case, x[:REUSE[cid]], guard))
    worst = _hilbert_worst(got, x)
    assert worst < tol, (cid, "per column", worst)
    for hs in shorts:
        assert _hilbert_worst(hs, x[:REUSE[cid]]) < tol, (cid, "short call")
    verdict = f"; the two short calls {'matched' if _same(*shorts) else 'differ in bits'}" if shorts else ""
    print(f"MEASURED chunk-seams {cid} chunks {case.expect['chunks']} worst column relerr {worst:.2e} bar {tol:.0e}{verdict}")
