"""Multitaper cross-spectra and coherence on the device, stage by stage through the C ABI, against the long-double reference of tests/mt_cross_ref.py
(written from multitaper.jl:551-616 and :704-723; tests/test_mt_cross_ref_cpu.py shows that every bound used here fails a subtly wrong computation).
Every device buffer is a guard_bands layout: quiet-NaN poison around and between the input columns, another NaN pattern all over the output, guards of
max(4096, nfft) elements, the first element 0, 1 and 3 elements off a 128-byte line -- INTEGRATION.md "What a call touches".

a. mdsp_mt_spectra_exec (demean_kernel + the STFT dispatch with K = 1 frame per channel, channel stride nout * ntapers, one launch per taper) at the
   sizes of mt_cross_ref.MT_CASES: the smallest nfft of every route of real STFT columns, the smallest odd one, 1024 under engine ROCFFT; the route is
   read back from mdsp_spectral_route_for.  Tapers are seeded noise of unit norm -- no symmetry, so a window read back to front shows -- with
   distinct r_k.  n = nfft and n = nfft - nfft // 4 - 1, lds = n + 5, every pair of ntapers in {1, 3, 7} and nch in {1, 2, 5} with demean and the
   alignment rotating.  Per (taper, channel) column max_f |got - ref| < 8 log2(nfft) u max_f |ref|; every channel bit-identical to the channel passed
   alone and compact; demean = 1 bit-identical to demean = 0 on the reference's demeaned samples (dyadic-grid samples: the mean is exact).  The
   multi-pass size (n = nfft, one taper, two channels) is held to the norm-wise project tolerance and 8 log2(nfft) Float32 ulps of the column maximum
   against a Float64 reference.  PSD, spectra, PSD on one plan: bit-identical to fresh plans.
b. mdsp_mt_cross_spectra on synthetic x_mt, even and odd nfft, nch in {1, 2, 5, 9}, four forms of freq_inds: per real component
   |got - ref| <= (ntapers + 8) u absdot + 2 u_min.
c. mdsp_coherence_from_cs on a rounded long-double cross-spectral matrix with real diagonals: diagonal exactly 1, exactly symmetric, off the diagonal
   |got - ref| <= 6 u |ref|; with an all-zero channel NaN exactly where the reference has it.
d. The error codes, each leaving the guarded output at its fill.
e. mt_cross_power_spectra / mt_coherence, their _ forms, config and keyword forms with DPSS tapers at nfft 75, 2187, 2100, 1024: the tolerances of
   test_mt_cross_spectra_and_coherence (1e-11 / 2e-5 norm-wise) against the long-double reference.

Measured on MI355X (worst over all cases; "ulps" = max_f |got - ref| / (u max_f |ref|) per column, u = 2^-24 / 2^-53):

    a. spectra, ulps     nfft 8     9      11     64     75     256    2100   2187   1024 (rocFFT)   bar 8 log2(nfft) = 24 ... 89
       Float32           2.04   2.15   4.00   2.20   2.33   2.99   3.22   3.00   3.45
       Float64           1.99   2.60   3.06   2.48   3.11   2.70   2.83   3.98   5.52
       multi-pass        Float32 nfft 32768: relerr 1.3e-7, 2.84 Float32 ulps of the column maximum; Float64 nfft 16384: relerr 3.2e-16
    b. cross spectra     worst error 3.01 (Float32) / 3.46 (Float64) u absdot against ntapers + 8 = 9 ... 15; at most 0.34 of the bound
    c. coherence         worst error 2.89 (Float32) / 2.75 (Float64) u |ref| against 6
    e. Python API        worst relerr 2.7e-7 (Float32) / 1.3e-15 (Float64)

The Float64 columns stay as far below 8 log2(nfft) x 2^-53 as the Float32 ones below 8 log2(nfft) x 2^-24: the same constant holds in both formats.
Every channel was bit-identical to its compact single-channel call, demean = 1 to the reference's demeaned samples, and PSD / spectra / PSD on one
plan to fresh plans, on every route.
"""
import ctypes as C

import numpy as np
import pytest

import guard_bands as gb
import guard_cases as gc
import mt_cross_ref as mr
from conftest import relerr, ulps_of_max
from test_gpu_parity import TOL32, TOL64

pytestmark = pytest.mark.gpu

PAD_S = 5
OUT_SHIFT = {0: 1, 1: 3, 3: 0}
ENG_NAME = {gc.AUTO: "auto", gc.FUSED: "fused", gc.ROCFFT: "rocfft"}
# (ntapers, nch, demean, input offset from a 128-byte line): every pair (ntapers, nch); demean and the three alignments rotate through them
COMBOS = [(1, 1, 1, 3), (1, 2, 0, 1), (1, 5, 1, 0), (3, 1, 0, 1), (3, 2, 1, 0), (3, 5, 0, 3), (7, 1, 1, 0), (7, 2, 0, 3), (7, 5, 1, 1)]
COMBOS_MULTIPASS = [(1, 2, 0, 3), (1, 2, 1, 1)]
assert max(t * c for t, c, _, _ in COMBOS) <= 35


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _cdt(R):
    return np.dtype(np.complex64 if np.dtype(R) == np.float32 else np.complex128)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


def _same(a, b, what):
    same = _bits(a) == _bits(b)
    assert same.all(), (what, "first word that differs", int(np.flatnonzero(~same.ravel())[0]), int((~same).sum()))


def _assert_route(dtype, nfft, engine, c):
    import spectral_route_cases as src
    from dsp_jl_amd import _lib
    assert src.encode(_lib.lib(), gc.KIND_STFT, dtype, engine, [nfft])[0] == c, (dtype, nfft, engine)


class Plan:
    """mdsp_mt_plan_create with the test's own tapers (n, ntapers) and normalisations r."""

    def __init__(self, n, nfft, tapers, r, dtype, engine=gc.AUTO, onesided=1):
        from dsp_jl_amd import _lib
        self.lib = _lib.lib()
        self.tapers = np.asfortranarray(tapers, dtype=np.float64)
        self.r = np.ascontiguousarray(r, dtype=np.float64)
        self.n, self.nfft, self.ntap, self.dtype = n, nfft, self.tapers.shape[1], dtype
        self.h = C.c_void_p()
        _lib.check(self.lib.mdsp_mt_plan_create(C.byref(self.h), n, nfft, self.tapers.ctypes.data_as(C.c_void_p), self.ntap,
                                                self.r.ctypes.data_as(C.c_void_p), onesided, dtype, engine))
        no, nt, eng = C.c_int64(), C.c_int64(), C.c_int()
        _lib.check(self.lib.mdsp_mt_plan_info(self.h, C.byref(no), C.byref(nt), C.byref(eng)))
        assert nt.value == self.ntap
        self.nout, self.engine = no.value, eng.value

    def close(self):
        if self.h:
            self.lib.mdsp_mt_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _guarded_in(cols, n, ld, guard, shift, dtype):
    cols = np.ascontiguousarray(cols, dtype=dtype).reshape(-1, n)
    lay = gb.layout(n, cols.shape[0], ld, guard, guard, shift, dtype)
    return lay, gb.to_device(gb.new_input(lay, cols))


def _guarded_out(count, guard, shift, dtype):
    lay = gb.layout(count, 1, max(count, 1), guard, guard, shift, dtype)
    return lay, gb.to_device(gb.new_output(lay))


def _spectra(plan, s, demean, shift, guard, what, lds=None):
    """mdsp_mt_spectra_exec on the channels s (nch, n) in a guarded layout; returns X[c, k, f] after check_output."""
    from dsp_jl_amd import _lib, _dev
    nch, n = s.shape
    li, sd = _guarded_in(s, n, n + PAD_S if lds is None else lds, guard, shift, s.dtype)
    tot = nch * plan.ntap * plan.nout
    lo, od = _guarded_out(tot, guard, OUT_SHIFT[shift], _cdt(s.dtype))
    _lib.check(plan.lib.mdsp_mt_spectra_exec(plan.h, gb.ptr(sd, li), nch, li.ld, int(demean), gb.ptr(od, lo), _dev.stream_ptr()))
    after = gb.from_device(od)
    gb.check_output(after, lo, tot, what)
    return gb.columns(after, lo)[0].reshape(nch, plan.ntap, plan.nout)


def _psd(plan, s, length, nov, K, shift, guard, what):
    """mdsp_mt_psd_exec, guarded: (nch, K, nout)."""
    from dsp_jl_amd import _lib, _dev
    nch = s.shape[0]
    li, sd = _guarded_in(s, length, length + PAD_S, guard, shift, s.dtype)
    ldo = plan.nout + 3
    chs = K * ldo + 11
    lo = gb.layout_nested(plan.nout, K, ldo, nch, chs, guard, guard, OUT_SHIFT[shift], s.dtype)
    od = gb.to_device(gb.new_output(lo))
    _lib.check(plan.lib.mdsp_mt_psd_exec(plan.h, gb.ptr(sd, li), length, nov, nch, li.ld, gb.ptr(od, lo), ldo, chs, _dev.stream_ptr()))
    after = gb.from_device(od)
    gb.check_output(after, lo, plan.nout, what)
    return gb.columns(after, lo).reshape(nch, K, plan.nout)


def _size_cases():
    return [pytest.param(dt, e, n, c, id=f"{np.dtype(mr.NP_REAL[dt]).name}-{ENG_NAME[e]}-{n}") for dt in (mr.F32, mr.F64) for e, n, c in mr.MT_CASES[dt]]


# ---- a. mdsp_mt_spectra_exec ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,engine,nfft,route", _size_cases())
def test_tapered_spectra_every_route(d, dtype, engine, nfft, route):
    R = np.dtype(mr.NP_REAL[dtype])
    _assert_route(dtype, nfft, engine, route)
    guard = max(gb.MIN_GUARD, nfft)
    multipass = route == mr.MULTIPASS_ROUTE
    worst_ulps = worst_rel = 0.0
    for n in mr.frame_lengths(nfft, route):
        rng = np.random.default_rng(31 * nfft + n + dtype)
        combos = COMBOS_MULTIPASS if multipass else COMBOS
        ntap_max, nch_max = max(c[0] for c in combos), max(c[1] for c in combos)
        tapers, r = mr.random_tapers(rng, n, ntap_max)
        sig = {0: mr.dyadic_signal(rng, nch_max, n, R, offset=0.0), 1: mr.dyadic_signal(rng, nch_max, n, R, offset=8.0)}
        ref = {dm: mr.tapered_spectra(sig[dm], tapers, nfft, bool(dm), R) for dm in sorted({c[2] for c in combos})}      # [f, k, c]
        plans = {}
        for ntap, nch, demean, shift in combos:
            if ntap not in plans:
                plans[ntap] = Plan(n, nfft, tapers[:, :ntap], r[:ntap], dtype, engine)
                assert plans[ntap].engine == (gc.ROCFFT if route == "0" else gc.FUSED) and plans[ntap].nout == nfft // 2 + 1
            plan = plans[ntap]
            what = f"mt spectra {R.name} nfft {nfft} n {n} ntapers {ntap} nch {nch} demean {demean} shift {shift}"
            s = sig[demean][:nch]
            X = _spectra(plan, s, demean, shift, guard, what)
            got, want = X.transpose(2, 1, 0), ref[demean][:, :ntap, :nch]
            if multipass:
                e = relerr(got, want.astype(np.complex128))
                ulps = max(ulps_of_max(got[:, k, c], want[:, k, c].astype(np.complex128)) for k in range(ntap) for c in range(nch))
                worst_rel, worst_ulps = max(worst_rel, e), max(worst_ulps, ulps)
                assert e < (TOL32 if R == np.float32 else TOL64), (what, e)
                assert ulps < 8 * np.log2(nfft), (what, ulps)
            else:
                excess, ulps = mr.column_excess(got, want, nfft, R)
                worst_ulps = max(worst_ulps, ulps)
                assert excess < 1.0, (what, "ulps of the column maximum", ulps, "bar", 8 * np.log2(nfft))
            # every channel alone and compact: the same bits
            for c in range(nch):
                one = _spectra(plan, np.ascontiguousarray(s[c:c + 1]), demean, 0, guard, what + f" channel {c} alone", lds=n)
                _same(X[c], one[0], (what, "channel", c))
            # demean_kernel, bit for bit: its output is what the reference's demean stores, so the spectra are those of that signal without demean
            if demean:
                pre = _spectra(plan, mr.demean(s, R), 0, shift, guard, what + " demeaned by the reference", lds=n)
                _same(X, pre, (what, "demean"))
        for p in plans.values():
            p.close()
    unit = "Float32 ulps of max (Float64 reference)" if multipass else "ulps"
    print(f"MEASURED mt_spectra {R.name} {ENG_NAME[engine]} nfft {nfft} route {route} {unit} {worst_ulps:.2f} bar {8 * np.log2(nfft):.1f}"
          + (f" relerr {worst_rel:.2e}" if multipass else ""))


@pytest.mark.parametrize("dtype,engine,nfft,route", _size_cases())
def test_psd_and_spectra_share_one_plan(d, dtype, engine, nfft, route):
    """mdsp_mt_psd_exec, mdsp_mt_spectra_exec, mdsp_mt_psd_exec on ONE plan (they share psd_only / noverlap / accumulate / the rocFFT batch): both PSDs
    bit-identical to a fresh plan's, the spectra bit-identical to those of a plan that never ran the PSD."""
    R = np.dtype(mr.NP_REAL[dtype])
    _assert_route(dtype, nfft, engine, route)
    guard = max(gb.MIN_GUARD, nfft)
    multipass = route == mr.MULTIPASS_ROUTE
    ntap, nch = (1, 2) if multipass else (3, 2)
    n, nov, hop, length = gc.spectral_shapes(nfft)[0 if multipass else 1]
    K = 3
    rng = np.random.default_rng(17 * nfft + dtype)
    tapers, r = mr.random_tapers(rng, n, ntap)
    long = mr.dyadic_signal(rng, nch, length, R, offset=0.0)
    frame = np.ascontiguousarray(long[:, hop:hop + n])
    what = f"mt psd/spectra/psd {R.name} nfft {nfft} n {n}"
    shared, fresh_psd, fresh_spec = (Plan(n, nfft, tapers, r, dtype, engine) for _ in range(3))
    p1 = _psd(shared, long, length, nov, K, 3, guard, what + " first psd")
    x = _spectra(shared, frame, 1, 1, guard, what + " spectra")
    p2 = _psd(shared, long, length, nov, K, 3, guard, what + " second psd")
    pf = _psd(fresh_psd, long, length, nov, K, 3, guard, what + " fresh psd")
    xf = _spectra(fresh_spec, frame, 1, 1, guard, what + " fresh spectra")
    _same(p1, pf, what + ": first psd against a fresh plan")
    _same(p2, pf, what + ": psd after spectra against a fresh plan")
    _same(x, xf, what + ": spectra after psd against a plan that never ran the psd")
    # and the PSD is the PSD: sum_k |x_k|^2 / r_k of the middle frame, one-sided (multitaper.jl:241-242), against the spectra stage's reference
    ref = mr.tapered_spectra(frame, tapers, nfft, False, R)
    pw = (np.abs(ref) ** 2 / r[None, :, None].astype(mr.LD)).sum(axis=1)                 # [f, c]
    pw[1:(nfft + 1) // 2] *= 2
    assert relerr(p1[:, 1, :].T, pw.astype(np.float64)) < (TOL32 if R == np.float32 else TOL64), what
    for p in (shared, fresh_psd, fresh_spec):
        p.close()


# ---- b. mdsp_mt_cross_spectra ---------------------------------------------------------------------------------------------------------------------------
def _freq_forms(rng, nout, nch):
    sub = 7 if nout >= 7 else nout
    assert (sub * nch * nch) % 256 != 0
    mid = rng.permutation(np.arange(1, nout - 1))[:sub - 2]
    shuffled = rng.permutation(np.concatenate([[0, nout - 1], mid]))
    return [("all", np.arange(nout)), ("dc", np.array([0])), ("last", np.array([nout - 1])), ("shuffled", shuffled)]


@pytest.mark.parametrize("nfft", [64, 75])
@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_cross_spectra_on_synthetic_spectra(d, dtype, nfft):
    from dsp_jl_amd import _lib, _dev
    R = np.dtype(mr.NP_REAL[dtype])
    cdt = _cdt(R)
    _assert_route(dtype, nfft, gc.AUTO, "3")
    nout = nfft // 2 + 1
    guard = gb.MIN_GUARD
    worst = worst_ratio = 0.0
    case = 0
    for ntap in (1, 3, 7):
        rng = np.random.default_rng(900 + nfft + ntap + dtype)
        tapers, r = mr.random_tapers(rng, nfft, ntap)
        plan = Plan(nfft, nfft, tapers, r, dtype)
        for nch in (1, 2, 5, 9):
            x = (rng.standard_normal((nout, ntap, nch)) + 1j * rng.standard_normal((nout, ntap, nch))).astype(cdt)        # x_mt[f, k, c], f fastest
            for name, fi in _freq_forms(rng, nout, nch):
                shift = (0, 1, 3)[case % 3]
                case += 1
                what = f"mt cross spectra {R.name} nfft {nfft} ntapers {ntap} nch {nch} freq_inds {name}"
                li, xd = _guarded_in(x.ravel(order="F"), x.size, x.size, guard, shift, cdt)
                tot = nch * nch * fi.size
                lo, od = _guarded_out(tot, guard, OUT_SHIFT[shift], cdt)
                fi64 = np.ascontiguousarray(fi, dtype=np.int64)
                _lib.check(plan.lib.mdsp_mt_cross_spectra(plan.h, gb.ptr(xd, li), nch, fi64.ctypes.data_as(C.c_void_p), fi.size, gb.ptr(od, lo),
                                                          _dev.stream_ptr()))
                after = gb.from_device(od)
                gb.check_output(after, lo, tot, what)
                got = gb.columns(after, lo)[0].reshape((nch, nch, fi.size), order="F")                                     # out[l, m, fi], l fastest
                ref, absdot = mr.cross_spectra(x, 2.0 / r, fi, nfft)
                ex, ratio = mr.cross_excess(got, ref, absdot, ntap, R)
                worst, worst_ratio = max(worst, ex), max(worst_ratio, ratio)
                assert ex <= 1.0, (what, "error over bound", ex, "error in u absdot", ratio, "allowed", ntap + 8)
        plan.close()
    print(f"MEASURED mt_cross_spectra {R.name} nfft {nfft} worst error / bound {worst:.3f}, worst error {worst_ratio:.2f} u absdot (bar ntapers + 8)")


# ---- c. mdsp_coherence_from_cs --------------------------------------------------------------------------------------------------------------------------
def _coherence_input(rng, nch, nf, R, zero_channel=None):
    ntap = 3
    x = rng.standard_normal((nf, ntap, nch)) + 1j * rng.standard_normal((nf, ntap, nch))
    if zero_channel is not None:
        x[:, :, zero_channel] = 0
    cs, _ = mr.cross_spectra(x, [1.0, 0.7, 1.3], np.arange(nf), 2 * nf - 1)
    return mr.hermitian_input(cs, R)


def _coherence(cs, R, shift, what, real_dtype=None):
    from dsp_jl_amd import _lib, _dev
    nch, _, nf = cs.shape
    li, cd = _guarded_in(cs.ravel(order="F"), cs.size, cs.size, gb.MIN_GUARD, shift, cs.dtype)
    lo, od = _guarded_out(cs.size, gb.MIN_GUARD, OUT_SHIFT[shift], R)
    _lib.check(_lib.lib().mdsp_coherence_from_cs(gb.ptr(cd, li), nch, nf, _dev.md_dtype(R) if real_dtype is None else real_dtype, gb.ptr(od, lo),
                                                  _dev.stream_ptr()))
    return gb.from_device(od), lo


@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_coherence_on_synthetic_cross_spectra(d, dtype):
    R = np.dtype(mr.NP_REAL[dtype])
    worst = 0.0
    case = 0
    for nch in (2, 5, 9):
        for nf in (1, 7, 300):
            rng = np.random.default_rng(40 + nch + nf + dtype)
            cs = _coherence_input(rng, nch, nf, R)
            what = f"coherence {R.name} nch {nch} nf {nf}"
            after, lo = _coherence(cs, R, (0, 1, 3)[case % 3], what)
            case += 1
            gb.check_output(after, lo, cs.size, what)
            got = gb.columns(after, lo)[0].reshape((nch, nch, nf), order="F")
            assert np.all(got[np.arange(nch), np.arange(nch)] == 1), what
            _same(got, np.ascontiguousarray(got.transpose(1, 0, 2)), what + ": symmetry")
            ex = mr.coherence_excess(got, mr.coherence(cs), R)
            worst = max(worst, ex)
            assert ex <= 1.0, (what, "error over 6 u |ref|", ex)
    print(f"MEASURED coherence {R.name} worst error {6 * worst:.2f} u |ref| (bar 6)")


@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_coherence_with_an_all_zero_channel(d, dtype):
    R = np.dtype(mr.NP_REAL[dtype])
    nch, nf, z = 5, 7, 2
    cs = _coherence_input(np.random.default_rng(77 + dtype), nch, nf, R, zero_channel=z)
    ref = mr.coherence(cs)
    what = f"coherence {R.name} with channel {z} zero"
    after, lo = _coherence(cs, R, 1, what)
    got = gb.columns(after, lo)[0].reshape((nch, nch, nf), order="F")
    nan = np.isnan(ref)
    assert nan.sum() == 2 * (nch - 1) * nf and np.array_equal(np.isnan(got), nan), what
    # check_output counts NaN as a poisoned read: hold it on the buffer with the expected NaN replaced, so that the guards are still checked
    w = after.copy()
    el = w.view(R)
    flat = np.flatnonzero(nan.ravel(order="F")) + lo.starts[0]
    assert np.isnan(el[flat]).all()
    el[flat] = 0
    gb.check_output(w, lo, cs.size, what)
    assert np.all(got[np.arange(nch), np.arange(nch)] == 1), what
    assert mr.coherence_excess(got, ref, R) <= 1.0, what


# ---- d. error codes -------------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_output_untouched(d):
    from dsp_jl_amd import _lib, _dev
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    n = nfft = 64
    nout, ntap, nch = nfft // 2 + 1, 3, 2
    tapers, r = mr.random_tapers(rng, n, ntap)
    guard = gb.MIN_GUARD
    sm = _dev.stream_ptr()

    def untouched(od, lo, what):
        gb.check_output(gb.from_device(od), lo, 0, what)

    for dtype in (mr.F32, mr.F64):
        R = np.dtype(mr.NP_REAL[dtype])
        cdt = _cdt(R)
        _assert_route(dtype, nfft, gc.AUTO, "3")
        plan = Plan(n, nfft, tapers, r, dtype)
        x = (rng.standard_normal(nout * ntap * nch) + 1j * rng.standard_normal(nout * ntap * nch)).astype(cdt)
        li, xd = _guarded_in(x, x.size, x.size, guard, 1, cdt)
        lo, od = _guarded_out(nch * nch * nout, guard, 3, cdt)
        for bad in (-1, nout):
            fi = np.array([0, bad, 1], dtype=np.int64)
            st = lib.mdsp_mt_cross_spectra(plan.h, gb.ptr(xd, li), nch, fi.ctypes.data_as(C.c_void_p), 3, gb.ptr(od, lo), sm)
            assert st == _lib.ERR_ARGUMENT, (R.name, "frequency index", bad, st)
            untouched(od, lo, f"frequency index {bad}")
        fi = np.arange(nout, dtype=np.int64)
        assert lib.mdsp_mt_cross_spectra(plan.h, gb.ptr(xd, li), nch, fi.ctypes.data_as(C.c_void_p), 0, gb.ptr(od, lo), sm) == _lib.OK
        assert lib.mdsp_mt_cross_spectra(plan.h, gb.ptr(xd, li), 0, fi.ctypes.data_as(C.c_void_p), nout, gb.ptr(od, lo), sm) == _lib.OK
        untouched(od, lo, "cross spectra with nfi = 0 / nch = 0")
        # spectra: a channel stride below the frame length; no channels
        s = mr.dyadic_signal(rng, nch, n, R)
        ls, sd = _guarded_in(s, n, n + PAD_S, guard, 3, R)
        lx, xo = _guarded_out(nch * ntap * nout, guard, 1, cdt)
        st = lib.mdsp_mt_spectra_exec(plan.h, gb.ptr(sd, ls), nch, n - 1, 0, gb.ptr(xo, lx), sm)
        assert st == _lib.ERR_DIMENSION, (R.name, "lds < n", st)
        assert lib.mdsp_mt_spectra_exec(plan.h, gb.ptr(sd, ls), 0, ls.ld, 1, gb.ptr(xo, lx), sm) == _lib.OK
        untouched(xo, lx, "spectra with lds < n / nch = 0")
        # coherence: a complex code for the real dtype; no channels, no frequencies
        lc, co = _guarded_out(nch * nch * nout, guard, 0, R)
        for code in (_lib.C32, _lib.C64):
            assert lib.mdsp_coherence_from_cs(gb.ptr(xd, li), nch, nout, code, gb.ptr(co, lc), sm) == _lib.ERR_ARGUMENT
        assert lib.mdsp_coherence_from_cs(gb.ptr(xd, li), 0, nout, dtype, gb.ptr(co, lc), sm) == _lib.OK
        assert lib.mdsp_coherence_from_cs(gb.ptr(xd, li), nch, 0, dtype, gb.ptr(co, lc), sm) == _lib.OK
        untouched(co, lc, "coherence with a complex dtype code / nch = 0 / nf = 0")
        plan.close()
        # a two-sided real plan and a complex plan: neither entry point takes them (check_onesided_real, multitaper.jl:417-422)
        for pdt, onesided in ((dtype, 0), (dtype + 2, 0)):
            other = Plan(n, nfft, tapers, r, pdt, onesided=onesided)
            st = lib.mdsp_mt_spectra_exec(other.h, gb.ptr(sd, ls), nch, ls.ld, 0, gb.ptr(xo, lx), sm)
            assert st == _lib.ERR_ARGUMENT, (pdt, onesided, st)
            st = lib.mdsp_mt_cross_spectra(other.h, gb.ptr(xd, li), nch, fi.ctypes.data_as(C.c_void_p), nout, gb.ptr(od, lo), sm)
            assert st == _lib.ERR_ARGUMENT, (pdt, onesided, st)
            untouched(xo, lx, "spectra on a two-sided / complex plan")
            untouched(od, lo, "cross spectra on a two-sided / complex plan")
            other.close()


# ---- e. the Python API, end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,route", [(75, "3"), (2187, "5"), (2100, "5"), (1024, "1")])
@pytest.mark.parametrize("dtype", [mr.F32, mr.F64])
def test_python_api_against_the_long_double_reference(d, dtype, nfft, route):
    R = np.dtype(mr.NP_REAL[dtype])
    cdt = _cdt(R)
    tol = 2e-5 if R == np.float32 else 1e-11
    _assert_route(dtype, nfft, gc.AUTO, route)
    n, fs, nw, ntap, nch_max = nfft, 1000.0, 2, 3, 5
    rng = np.random.default_rng(nfft + dtype)
    sig = (rng.standard_normal((nch_max, n)) + 3.0).astype(R)
    mc = d.dpss_config(R, n, nw=nw, ntapers=ntap, fs=fs, nfft=nfft)
    assert mc.ntapers == ntap and mc.nout == nfft // 2 + 1
    kw = dict(fs=fs, nfft=nfft, nw=nw, ntapers=ntap)
    mk = d.MTConfig(R, n, **kw)                                       # what the keyword forms build: dpss tapers, r = fs / weights
    nout = mc.nout
    x = {dm: mr.tapered_spectra(sig, mc.window, nfft, dm, R) for dm in (False, True)}
    assert np.array_equal(mk.window, mc.window)
    band = (mc.freq[0], mc.freq[-1])                                  # open ends: exactly DC and the last row (Nyquist on even nfft) fall out
    worst = 0.0
    for nch in (1, 2, 5):
        s = np.ascontiguousarray(sig[:nch])
        for demean in (False, True):
            for fr in (None, band):
                fi = np.arange(nout) if fr is None else np.arange(1, nout - 1)
                what = f"{R.name} nfft {nfft} nch {nch} demean {demean} band {fr is not None}"
                opts = dict(demean=demean, freq_range=fr)
                if nch == 2:      # keyword forms
                    cs, _ = mr.cross_spectra(x[demean][:, :, :nch], 2.0 / mk.r, fi, nfft)
                    got = d.mt_cross_power_spectra(s, **kw, **opts)
                    coh = d.mt_coherence(s, **kw, **opts)
                    out_cs = d.mt_cross_power_spectra_(np.zeros(cs.shape, dtype=cdt), s, **kw, **opts)
                    out_coh = d.mt_coherence_(np.zeros(cs.shape, dtype=R), s, **kw, **opts)
                else:             # config forms
                    cs, _ = mr.cross_spectra(x[demean][:, :, :nch], 2.0 / mc.r, fi, nfft)
                    cfg = d.MTCrossSpectraConfig(nch, mc, **opts)
                    assert np.array_equal(cfg.freq_inds, fi)
                    got = d.mt_cross_power_spectra(s, cfg)
                    coh = d.mt_coherence(s, d.MTCoherenceConfig(cfg))
                    out_cs = d.mt_cross_power_spectra_(np.zeros(cs.shape, dtype=cdt), s, cfg)
                    out_coh = d.mt_coherence_(np.zeros(cs.shape, dtype=R), s, d.MTCoherenceConfig(nch, mc, **opts))
                assert got.power.shape == cs.shape and got.power.dtype == cdt and np.array_equal(got.freq, mc.freq[fi]), what
                assert coh.coherence.shape == cs.shape and coh.coherence.dtype == R and np.array_equal(coh.freq, mc.freq[fi]), what
                e = relerr(got.power, cs.astype(np.complex128))
                ec = relerr(coh.coherence, mr.coherence(cs).astype(np.float64))
                worst = max(worst, e, ec)
                assert e < tol and ec < tol, (what, e, ec)
                _same(out_cs.power, got.power, what + ": mt_cross_power_spectra!")
                _same(out_coh.coherence, coh.coherence, what + ": mt_coherence!")
    print(f"MEASURED mt python api {R.name} nfft {nfft} route {route} worst relerr {worst:.2e} bar {tol:.0e}")
