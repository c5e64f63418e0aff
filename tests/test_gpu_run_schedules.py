"""GPU tests of the fused spectral and overlap-save kernels when every transform slot walks SEVERAL consecutive units.

The kernels are persistent and the host sizes their grid as min(work, CUs x workgroups per CU), so at the shapes the rest of the suite uses a slot
gets one unit and everything between two units of a run never executes (tests/run_schedule_cases.py has the arithmetic).  Here MDSP_WG_PER_CU=1
and two channels shrink the grid, and the signals are just long enough that every slot walks a run of three units, the last run is partial and one slot
idles; with MDSP_RUNS_PER_SLOT=2 the runs are two units long and about half of the slots walk a second one.

    (a) stft / spectrogram, ComplexF32, every SHIFT instantiation of stft_fused_kernel's register carry: the Float64 oracle, and BIT identity with the
        same frames computed one unit per slot (a carried frame moves samples between registers and does no arithmetic)
    (b) welch_pgram, ComplexF32, every SHIFT instantiation of welch_fused_kernel: the oracle, and the default schedule to 1e-6
    (c) the dispatch edge (no overlap, hop no multiple of T, n < nfft, E = 4, ComplexF64): the same run walk on the kernels without the carry
    (d) real signals: stft_pair_kernel (raw and PSD, one- and two-sided), welch_half_kernel, welch_fused_kernel, Float32 and Float64, odd frame counts
    (e) overlap-save, four dtypes: the oracle, and bit identity of four schedules (a unit's arithmetic does not depend on who runs it),
        among them MDSP_OLS_PREFETCH=1, which carries the next unit's samples across iterations

Tolerances are the suite's: norm-wise 5e-6 (Float32) / 1e-12 (Float64) against the Float64 oracle on the same Float32-rounded input, and for Float32
STFT columns |err| < 8 log2(nfft) ulp of the column's largest bin (tests/test_gpu_gx.py _ulp_bound).  The signals are noise plus a tone under a slow
amplitude ramp, so a frame assembled from another frame's samples is wrong in level as well as in phase."""
import contextlib
import math

import numpy as np
import pytest

import run_schedule_cases as rs
from conftest import relerr, ulps_of_max

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 5e-6, 1e-12
RUNS = (1, 2)


def _tol(dt):
    return TOL64 if np.dtype(dt) in (rs.F64, rs.C64) else TOL32


def _ulp_bound(nfft):
    return 8.0 * math.log2(nfft)          # tests/test_gpu_gx.py


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def cu(d):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _tunables(**kw):
    """Set tuning variables for the duration of a block; the defaults come back whatever happens inside."""
    from dsp_jl_amd import _lib
    try:
        for name, value in kw.items():
            _lib.set_tunable(name, value)
        yield
    finally:
        for name in kw:
            _lib.set_tunable(name, None)


def _small_grid(runs=1, **more):
    return _tunables(MDSP_WG_PER_CU=1, MDSP_RUNS_PER_SLOT=runs, **more)


def _signal(seed, length, dt, nch=rs.NCH):
    """(length, nch) host array of `dt` (Float32-rounded for the Float32 types): seeded noise plus a tone, under the ramp 1 + 0.5 k / length."""
    dt = np.dtype(dt)
    k = np.arange(length)
    ramp = 1.0 + 0.5 * k / length
    cols = []
    for c in range(nch):
        rng = np.random.default_rng([seed, c])
        s = rng.standard_normal(length) + 0.5 * np.sin(2 * np.pi * (0.1234 + 0.01 * c) * k)
        if dt.kind == "c":
            s = s + 1j * (rng.standard_normal(length) + 0.5 * np.cos(2 * np.pi * (0.1234 + 0.01 * c) * k))
        cols.append(s * ramp)
    return np.stack(cols, axis=1).astype(dt)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _spectral_shape(op_kind, dt, nfft, n, hop, cu):
    """(slots, frames, signal length) of a complex case: a unit is a frame."""
    _, _, G = rs.geometry(op_kind, dt, nfft)
    ns = rs.slots(cu, rs.NCH, G, op_kind)
    K = rs.units_for(ns)
    return ns, K, (K - 1) * hop + n + 5


def _check_stft(d, x, xd, dt, nfft, n, hop, onesided, runs, K):
    """Raw STFT and spectrogram of both channels on the small grid against the oracle; returns the raw STFT (host)."""
    from oracle import periodograms as opg, windows as ow
    tol, f32 = _tol(dt), _tol(dt) == TOL32
    kw = dict(nfft=nfft, window=d.hanning, onesided=onesided, engine=d.ENGINE_FUSED)
    with _small_grid(runs):
        got = _host(d.stft(xd, n, n - hop, **kw))
        psd = _host(d.spectrogram(xd, n, n - hop, fs=2.0, **kw).power)
    nout = nfft // 2 + 1 if onesided else nfft
    assert got.shape == psd.shape == (nout, K, rs.NCH)
    for c in range(rs.NCH):
        ref = opg.stft(x[:, c], n, n - hop, nfft=nfft, window=ow.hanning, onesided=onesided, dtype=np.float64)
        assert ref.shape == (nout, K)
        e = relerr(got[:, :, c], ref)
        assert e < tol, ("stft", runs, c, e)
        if f32:
            u = ulps_of_max(got[:, :, c], ref, axis=0)
            assert u < _ulp_bound(nfft), ("stft column", runs, c, u)
        rp = opg.spectrogram(x[:, c], n, n - hop, nfft=nfft, window=ow.hanning, onesided=onesided, fs=2.0, dtype=np.float64).power
        e = relerr(psd[:, :, c], rp)
        assert e < tol, ("spectrogram", runs, c, e)
    return got


def _check_welch(d, x, xd, dt, nfft, n, hop, onesided, K):
    """welch_pgram of both channels on the small grid (one and two runs per slot) against the oracle and against the default schedule."""
    from oracle import periodograms as opg, windows as ow
    tol = _tol(dt)
    cfg = d.WelchConfig(x.shape[0], dt, n=n, noverlap=n - hop, nfft=nfft, window=d.hanning, onesided=onesided, fs=2.0, engine=d.ENGINE_FUSED)
    assert cfg.engine == d.ENGINE_FUSED
    assert d.frame_count(x.shape[0], n, n - hop) == K
    dflt = _host(d.welch_pgram(xd, cfg).power)
    ref = np.stack([opg.welch_pgram(x[:, c], n, n - hop, nfft=nfft, window=ow.hanning, onesided=onesided, fs=2.0, dtype=np.float64).power
                    for c in range(rs.NCH)], axis=1)
    assert dflt.shape == ref.shape
    e = relerr(dflt, ref)
    assert e < tol, ("default schedule", e)
    for runs in RUNS:
        with _small_grid(runs):
            got = _host(d.welch_pgram(xd, cfg).power)
        for c in range(rs.NCH):
            e = relerr(got[:, c], ref[:, c])
            assert e < tol, ("welch", runs, c, e)
        # the partial sums are added in another order under another schedule: close, not bit for bit
        e = relerr(got, dflt.astype(np.float64))
        assert e < (1e-6 if tol == TOL32 else tol), ("welch against the default schedule", runs, e)


# ============================================================================================ (a) STFT, ComplexF32 register carry
@pytest.mark.parametrize("nfft,shift", rs.STFT_SHIFT_CASES, ids=lambda v: str(v))
def test_stft_complex_register_carry(d, cu, nfft, shift):
    dt, _, n, hop = rs.shift_case("stft", nfft, shift)
    assert rs.carry_shift("stft", dt, nfft, n, hop) == shift
    ns, K, length = _spectral_shape("stft", dt, nfft, n, hop, cu)
    assert rs.schedule(K, ns, 1)[0] == 3 and rs.schedule(K, ns, 2)[0] == 2
    x = _signal(1000 * nfft + shift, length, dt)
    xd = _dev(x)
    # the same frames, at most one per slot (run_len == 1: every frame is loaded whole), in slices of `ns` frames at the default schedule
    pieces = []
    for f0 in range(0, K, ns):
        f1 = min(K, f0 + ns)
        assert rs.schedule(f1 - f0, ns, 1) == (1, 1)
        pieces.append(_host(d.stft(xd[f0 * hop:(f1 - 1) * hop + n], n, n - hop, nfft=nfft, window=d.hanning, onesided=False, engine=d.ENGINE_FUSED)))
    whole = np.concatenate(pieces, axis=1)
    assert whole.shape == (nfft, K, rs.NCH)
    for runs in RUNS:
        got = _check_stft(d, x, xd, dt, nfft, n, hop, False, runs, K)
        # a carried frame moves samples between registers and does no arithmetic: every frame of every run -- first, second, last, and the first
        # of a slot's second run -- is bit for bit the frame computed on its own
        same = np.all(got == whole, axis=(0, 2))
        assert same.all(), ("frames that differ from the one-unit-per-slot STFT", runs, np.flatnonzero(~same)[:16].tolist())


# ============================================================================================ (b) Welch, ComplexF32 register carry
@pytest.mark.parametrize("nfft,shift", rs.WELCH_SHIFT_CASES, ids=lambda v: str(v))
def test_welch_complex_register_carry(d, cu, nfft, shift):
    dt, _, n, hop = rs.shift_case("welch", nfft, shift)
    assert rs.carry_shift("welch", dt, nfft, n, hop) == shift
    ns, K, length = _spectral_shape("welch", dt, nfft, n, hop, cu)
    assert rs.schedule(K, ns, 1)[0] == 3 and rs.schedule(K, ns, 2)[0] == 2
    x = _signal(2000 * nfft + shift, length, dt)
    _check_welch(d, x, _dev(x), dt, nfft, n, hop, False, K)


# ============================================================================================ (c) the dispatch edge
@pytest.mark.parametrize("cid,dt,nfft,n,hop", rs.control_cases("stft"), ids=[c[0] for c in rs.control_cases("stft")])
def test_stft_complex_controls(d, cu, cid, dt, nfft, n, hop):
    assert rs.carry_shift("stft", dt, nfft, n, hop) == 0
    ns, K, length = _spectral_shape("stft", dt, nfft, n, hop, cu)
    x = _signal(3000 + nfft + hop, length, dt)
    xd = _dev(x)
    for runs in RUNS:
        _check_stft(d, x, xd, dt, nfft, n, hop, False, runs, K)


@pytest.mark.parametrize("cid,dt,nfft,n,hop", rs.control_cases("welch"), ids=[c[0] for c in rs.control_cases("welch")])
def test_welch_complex_controls(d, cu, cid, dt, nfft, n, hop):
    assert rs.carry_shift("welch", dt, nfft, n, hop) == 0
    ns, K, length = _spectral_shape("welch", dt, nfft, n, hop, cu)
    x = _signal(4000 + nfft + hop, length, dt)
    _check_welch(d, x, _dev(x), dt, nfft, n, hop, False, K)


# ============================================================================================ (d) real signals: the run walk
def _real_shape(kind, dt, nfft, n, hop, cu):
    _, _, G = rs.geometry(kind, dt, nfft)
    ns = rs.slots(cu, rs.NCH, G, kind)
    K = rs.real_frames(ns)                        # odd: units are frame pairs and the last one carries a single frame
    return ns, K, (K - 1) * hop + n + 5


@pytest.mark.parametrize("dt,nfft", rs.REAL_CASES, ids=lambda v: rs.case_id(v))
def test_stft_real_pairs_run_walk(d, cu, dt, nfft):
    for fid, n, hop, onesided in rs.real_stft_forms(nfft):
        ns, K, length = _real_shape("stft", dt, nfft, n, hop, cu)
        assert K % 2 == 1 and rs.schedule((K + 1) // 2, ns, 1)[0] == 3
        x = _signal(5000 + nfft + n, length, dt)
        xd = _dev(x)
        for runs in RUNS:
            _check_stft(d, x, xd, dt, nfft, n, hop, onesided, runs, K)


@pytest.mark.parametrize("dt,nfft", rs.REAL_CASES, ids=lambda v: rs.case_id(v))
def test_welch_real_run_walk(d, cu, dt, nfft):
    """Float32 nfft 4096 at hop = n/2 is welch_half3_kernel with its handed-over half frame; nothing is asserted about the variant, the oracle checks it."""
    for i, (fid, kind, n, hop) in enumerate(rs.real_welch_forms(nfft)):
        ns, K, length = _real_shape(kind, dt, nfft, n, hop, cu)
        assert K % 2 == 1 and rs.schedule((K + 1) // 2, ns, 1)[0] == 3
        x = _signal(6000 + nfft + n + hop, length, dt)
        _check_welch(d, x, _dev(x), dt, nfft, n, hop, i % 2 == 0, K)


# ============================================================================================ (e) overlap-save
def _filt_oracle(b, xc, nfft):
    from oracle import filt as ofilt
    b64 = b.astype(np.float64)
    if xc.dtype.kind == "c":       # the oracle's overlap-save is written for real signals; real taps filter the two parts independently
        return ofilt.fftfilt(b64, xc.real.astype(np.float64), nfft) + 1j * ofilt.fftfilt(b64, xc.imag.astype(np.float64), nfft)
    return ofilt.fftfilt(b64, xc.astype(np.float64), nfft)


@pytest.mark.parametrize("dt,nfft", rs.OLS_CASES, ids=lambda v: rs.case_id(v))
def test_overlap_save_run_walk_and_prefetch(d, cu, dt, nfft):
    """fftfilt on the fused engine: d.fftfilt for the real types; the complex types go through the same plan object (OlsPlan in FILT mode), which
    d.fftfilt does not expose for complex signals."""
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    dt = np.dtype(dt)
    cplx = dt.kind == "c"
    rdt = np.float32 if dt in (rs.F32, rs.C32) else np.float64
    tol = _tol(dt)
    nb, L, nblocks, nx, upc, ns = rs.ols_shape(dt, nfft, cu)
    total = upc * rs.OLS_NCOLS
    assert rs.schedule(total, ns, 1)[0] >= 3 and total % rs.schedule(total, ns, 1)[0] != 0
    rng = np.random.default_rng(7000 + nfft)
    b = (rng.standard_normal(nb) / np.sqrt(nb)).astype(rdt)
    x = _signal(7000 + nfft + nb, nx, dt, nch=rs.OLS_NCOLS)
    xd = _dev(x)
    plan = OlsPlan(b.astype(dt), nfft, nx, _lib.OLS_FILT, d.ENGINE_FUSED)
    assert (plan.nfft, plan.block_len, plan.engine) == (nfft, L, d.ENGINE_FUSED)
    cols = xd.t().contiguous()

    def run():
        return _host(plan.exec(cols, nx).t())

    out = {"default": run()}
    with _small_grid(1):
        out["one workgroup per CU"] = run()
        if not cplx:
            api = _host(d.fftfilt(b, xd, nfft, engine=d.ENGINE_FUSED))
            assert np.array_equal(api, out["one workgroup per CU"])
    with _small_grid(rs.OLS_RUNS):
        out["three runs per slot"] = run()
    with _small_grid(1, MDSP_OLS_PREFETCH=1):
        out["prefetch"] = run()
    edge = 2 * L
    for c in range(rs.OLS_NCOLS):
        ref = _filt_oracle(b, x[:, c], nfft)
        for name, y in out.items():
            e = relerr(y[:, c], ref)
            assert e < tol, (name, c, e)
            # the edges carry the zero padding in front of the signal and the clamped last block
            e0, e1 = relerr(y[:edge, c], ref[:edge]), relerr(y[-edge:, c], ref[-edge:])
            assert e0 < 5 * tol and e1 < 5 * tol, (name, c, e0, e1)
    # a unit's arithmetic does not depend on the schedule, nor on when its samples were loaded
    for name, y in out.items():
        same = np.array_equal(y, out["default"])
        if not same:
            bad = np.argwhere(y != out["default"])
            assert same, (name, "first differing (sample, column)", bad[0].tolist(), "of", len(bad))
