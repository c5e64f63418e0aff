"""Every compile-time spectral schedule a default call can reach, run on the device against the Float64 oracle (oracle/periodograms.py): the 177 single-workgroup
schedules of csrc/ctbig_sizes.h as Welch sums (MDSP_ROUTE_CTBIG) and as STFT / spectrogram / periodogram columns (MDSP_ROUTE_CTBIG_COLS), every distinct row and every
R0 of nfft = R0 x row with the fused column step (routes 6 / 7 / 8), and every R0 of the two-kernel form (MDSP_ROUTE_CTROWS), in Float32, Float64, ComplexF32 and
ComplexF64.  tests/ct_schedule_cases.py derives the cases from the route table and holds the inputs: a ramped signal, an ASYMMETRIC window vector, and two
configurations per case (A: whole frames at 50 % overlap under the window, 3 frames; B: n = nfft - 7, hop 2/3 n, no window, 4 frames, 2 channels).
tests/test_ct_schedule_cases_cpu.py keeps those lists complete.

    Float32 / ComplexF32 Welch sums and STFT columns:  norm-wise < 5e-6 and element-wise |err| < 8 log2(nfft) ulp of the largest bin (per column for the STFT)
    Float32 / ComplexF32 spectrogram and periodogram:  norm-wise < 5e-6
    Float64 / ComplexF64:                              norm-wise < 1e-12
the bounds of tests/test_gpu_gx.py; frequencies, times and shapes bit-exact; a second call on the same WelchConfig bit-identical.  Each case asserts the route and R0
mdsp_spectral_route_for reports, so none can pass on another kernel.  An item runs all its cases and lists every failing one."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import relerr, ulps_of_max

import ct_schedule_cases as ct

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
TOL32 = 5e-6

# one item per family and type; the longest is the two-kernel rows in Float32 (to 497 664 points), a few seconds
ITEMS = [pytest.param(family, dtype, id=f"{family}-{ct.NP_DTYPES[dtype].name}") for family in ct.FAMILIES for dtype in ct.DTYPES]


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _ulp_bound(nfft):
    return 8.0 * math.log2(nfft)


class _Report:
    """failures of an item, and the figures recorded for the next reader: the largest ulp figure relative to its bound and the largest Float64 error"""

    def __init__(self):
        self.bad = []
        self.ulp_ratio = (0.0, None)
        self.err64 = (0.0, None)
        self.checks = 0

    def fail(self, case, cfg, mode, what, value):
        self.bad.append(f"{_name(case, cfg)[:-1]}, {mode}, {what} = {value})")

    def norm(self, case, cfg, mode, got, ref):
        """the norm-wise bound of the case's precision"""
        f32 = case.dtype in (ct.F32, ct.C32)
        got = np.asarray(got)
        self.checks += 1
        if got.shape != ref.shape:
            return self.fail(case, cfg, mode, "shape", f"{got.shape}, oracle {ref.shape}")
        want = np.dtype(np.float32 if f32 else np.float64) if got.dtype.kind == "f" else np.dtype(np.complex64 if f32 else np.complex128)
        if got.dtype != want:
            self.fail(case, cfg, mode, "eltype", got.dtype)
        e = relerr(got, ref)
        if not e < (TOL32 if f32 else TOL64):
            self.fail(case, cfg, mode, "relerr", e)
        if not f32 and e > self.err64[0]:
            self.err64 = (e, (case, cfg.name, mode))

    def ulps(self, case, cfg, mode, got, ref, axis=None):
        """Float32 types: the element-wise bound, 8 log2(nfft) ulp of the largest bin (along `axis`)"""
        if case.dtype not in (ct.F32, ct.C32) or np.asarray(got).shape != ref.shape:
            return
        u = ulps_of_max(got, ref, axis=axis)
        if not u < _ulp_bound(case.nfft):
            self.fail(case, cfg, mode, f"ulps_of_max (bound {_ulp_bound(case.nfft):.1f})", u)
        if u / _ulp_bound(case.nfft) > self.ulp_ratio[0]:
            self.ulp_ratio = (u / _ulp_bound(case.nfft), (case, cfg.name, mode))

    def exact(self, case, cfg, mode, what, got, ref):
        if not np.array_equal(np.asarray(got), np.asarray(ref)):
            self.fail(case, cfg, mode, what, "differs")


def _channels(a, cfg):
    """the channels of a (..., channels) result or signal, or the array itself where the configuration has one"""
    a = np.asarray(a)
    return [a] if cfg.channels == 1 else [a[..., c] for c in range(cfg.channels)]


def _check_route(lib, case, cfg, rep):
    """The query is asked again; it is not the plan that ran that answers.  That pins the kernel because plan creation decides through the same function as the query,
    and because every array here stays below the size from which host arrays take the chunked host pipeline (_dev.HOST_PIPELINE_MIN_BYTES), so the calls run the plan
    on the device path."""
    from dsp_jl_amd import _lib
    eng, route, r0 = C.c_int(), C.c_int(), C.c_int()
    for engine in (ct.AUTO, ct.FUSED):      # the calls below leave the engine to the library
        _lib.check(lib.mdsp_spectral_route_for(case.kind, case.dtype, case.nfft, engine, C.byref(eng), C.byref(route), C.byref(r0)))
        if (eng.value, route.value, r0.value) != (ct.FUSED, case.route, case.r0):
            rep.fail(case, cfg, f"engine {engine}", "(engine, route, r0)", (eng.value, route.value, r0.value))


def _check_welch(d, case, cfg, s, rep):
    from oracle import periodograms as opg
    dt = ct.NP_DTYPES[case.dtype]
    for onesided in ((False,) if dt.kind == "c" else (True, False)):
        mode = "welch one-sided" if onesided else "welch two-sided"
        wc = d.WelchConfig(cfg.length, dt, n=cfg.n, noverlap=cfg.noverlap, nfft=case.nfft, window=cfg.window, onesided=onesided, fs=2.5)
        if wc.engine != d.ENGINE_FUSED:
            rep.fail(case, cfg, mode, "engine", wc.engine)
        got = d.welch_pgram(s, wc)
        power = np.asarray(got.power)
        for c, (p, sc) in enumerate(zip(_channels(power, cfg), _channels(s, cfg))):
            ref = opg.welch_pgram(sc, cfg.n, cfg.noverlap, nfft=case.nfft, window=cfg.window, onesided=onesided, fs=2.5, dtype=np.float64)
            assert ref.power.shape == ((case.nfft // 2 + 1) if onesided else case.nfft,)
            rep.norm(case, cfg, f"{mode} ch {c}", p, ref.power)
            rep.ulps(case, cfg, f"{mode} ch {c}", p, ref.power)
            rep.exact(case, cfg, mode, "freq", got.freq, ref.freq)
        # deterministic: a re-used config is bit-identical call after call
        rep.exact(case, cfg, mode, "second call", d.welch_pgram(s, wc).power, power)


def _check_columns(d, case, cfg, s, rep):
    from oracle import periodograms as opg
    dt = ct.NP_DTYPES[case.dtype]
    nfft, K = case.nfft, cfg.frames
    for onesided in ((False,) if dt.kind == "c" else (True, False)):
        side = "one-sided" if onesided else "two-sided"
        nout = (nfft // 2 + 1) if onesided else nfft
        got = np.asarray(d.stft(s, cfg.n, cfg.noverlap, nfft=nfft, window=cfg.window, onesided=onesided))
        if got.shape != ((nout, K) if cfg.channels == 1 else (nout, K, cfg.channels)):
            rep.fail(case, cfg, f"stft {side}", "shape", got.shape)
            continue
        sp = d.spectrogram(s, cfg.n, cfg.noverlap, nfft=nfft, window=cfg.window, onesided=onesided, fs=3.0)
        for c, (g, p, sc) in enumerate(zip(_channels(got, cfg), _channels(sp.power, cfg), _channels(s, cfg))):
            ref = opg.stft(sc, cfg.n, cfg.noverlap, nfft=nfft, window=cfg.window, onesided=onesided, dtype=np.float64)
            assert ref.shape == (nout, K)
            rep.norm(case, cfg, f"stft {side} ch {c}", g, ref)
            rep.ulps(case, cfg, f"stft {side} ch {c}", g, ref, axis=0)
            rs = opg.spectrogram(sc, cfg.n, cfg.noverlap, nfft=nfft, window=cfg.window, onesided=onesided, fs=3.0, dtype=np.float64)
            rep.norm(case, cfg, f"spectrogram {side} ch {c}", p, rs.power)
            rep.exact(case, cfg, f"spectrogram {side}", "time", sp.time, rs.time)
            rep.exact(case, cfg, f"spectrogram {side}", "freq", sp.freq, rs.freq)
    x = np.ascontiguousarray(_channels(s, cfg)[0][:cfg.n])
    pg = d.periodogram(x, nfft=nfft, window=cfg.window, fs=2.0)
    rp = opg.periodogram(x, nfft=nfft, window=cfg.window, fs=2.0, dtype=np.float64)
    rep.norm(case, cfg, "periodogram", pg.power, rp.power)
    rep.exact(case, cfg, "periodogram", "freq", pg.freq, rp.freq)


def _comparisons(case):
    """norm-wise comparisons of one case over both configurations: per mode (one-sided and two-sided, or two-sided alone for complex signals) one per channel
    (1 + 2) for Welch sums; for columns two per channel (stft, spectrogram) and one periodogram per configuration"""
    modes = 1 if ct.NP_DTYPES[case.dtype].kind == "c" else 2
    return 3 * modes if case.kind == ct.WELCH else 6 * modes + 2


def _name(case, cfg):
    return f"({ct.NP_DTYPES[case.dtype].name}, nfft {case.nfft}, route {case.route}, r0 {case.r0}, {cfg.name})"


def run_cases(d, cases, rep):
    """A call the library REFUSES (bad argument, unsupported size) is a failure of its case, and the others still run.  Anything else -- a device error above all, a
    library-side assertion, an unknown exception -- ends the item at once with the running case named: nothing more is started on a device that may have faulted."""
    from dsp_jl_amd import _lib
    lib = _lib.lib()
    refused = (_lib.ArgumentError, _lib.DomainError, _lib.DimensionMismatch, _lib.UnsupportedError)
    for case in cases:
        for cfg in ct.configs(case.nfft):
            try:
                _check_route(lib, case, cfg, rep)
                s = ct.case_signal(case, cfg)
                (_check_welch if case.kind == ct.WELCH else _check_columns)(d, case, cfg, s, rep)
            except refused as exc:
                rep.fail(case, cfg, "call", type(exc).__name__, exc)
            except Exception as exc:
                raise RuntimeError(f"{type(exc).__name__} while running {_name(case, cfg)}, the item ends here: {exc}") from exc


@pytest.mark.parametrize("family,dtype", ITEMS)
def test_ct_schedules_vs_oracle(d, family, dtype):
    cases = ct.family_cases(family, dtype)
    assert cases
    rep = _Report()
    run_cases(d, cases, rep)
    print(f"\n{family} {ct.NP_DTYPES[dtype].name}: {len(cases)} cases x 2 configurations, {rep.checks} comparisons; "
          f"largest ulps_of_max / (8 log2 nfft) = {rep.ulp_ratio[0]:.3f} at {rep.ulp_ratio[1]}; largest Float64 relerr = {rep.err64[0]:.3e} at {rep.err64[1]}")
    assert not rep.bad, f"{len(rep.bad)} failures (dtype, nfft, route, r0, configuration, mode, measured):\n" + "\n".join(rep.bad)
    assert rep.checks == sum(_comparisons(c) for c in cases)      # no mode, channel or configuration dropped out of a loop
