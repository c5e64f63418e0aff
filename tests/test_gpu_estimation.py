"""jacobsen / quinn on the device: the two reductions and the quinn pass equal their host emulations bit for bit (lengths where the tiling takes another
path, forced cuts, four types, device pointers 0 - 3 elements off), the functions against the reference's own tests (test/estimation.jl:23-80) and the
numpy restatement with the bounds of tests/test_estimation_cpu.py, repeat calls, and every argument error."""
import numpy as np
import pytest

import estimation_cases as ec
import estimation_ref as ref
from estimation_cases import AGREE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _offset_copy(x, off):
    """x on the device, `off` elements behind the start of an allocation: (tensor kept alive, device address)."""
    import torch
    buf = np.zeros(len(x) + 4, dtype=x.dtype)
    buf[off:off + len(x)] = x
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + off * x.dtype.itemsize


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_quinn_pass_equals_its_emulation_bit_for_bit(d, dt):
    import torch
    dt = np.dtype(dt)
    nrec = 3 if dt.kind == "c" else 4
    cases = [(n, S) for n in ec.PASS_LENGTHS for S in ec.PASS_CUTS] + [ec.CARRY_CASE]
    for i, (n, S) in enumerate(cases):
        f = ec.PASS_TONES[i % 3]
        x = ec.tone(n, f, dt, seed=1776 + i)
        mean, param = ec.mean_of(x), ec.pass_param(f, dt)
        want = ec.pass_emulate(x, mean, param, S)
        plan = d.QuinnPlan(dt, n, S)
        assert (plan.segments, plan.seglen) == d.quinn_geometry(dt, n, S)[:2]
        for off in ({0, i % 4} if n > 64 else range(4)):
            keep, ptr = _offset_copy(x, off)
            out = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
            plan.pass_exec(ptr, mean, param, out.data_ptr())
            got = out.cpu().numpy()
            assert np.array_equal(got[:nrec].view(np.uint64), want.view(np.uint64)), (n, S, off, got, want)
            assert nrec == 4 or np.isnan(got[3])                          # a complex record is three doubles


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_est_reductions_equal_their_emulation_bit_for_bit(d, dt):
    import torch
    from dsp_jl_amd import _lib, estimation as est
    dt = np.dtype(dt)
    V = 16 // dt.itemsize
    rng = np.random.default_rng(8)
    ops = (_lib.EST_SUM, _lib.EST_ABS2ARGMAX) if dt.kind == "c" else (_lib.EST_SUM,)
    for n in ec.REDUCE_LENGTHS:
        x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if dt.kind == "c" else 0)).astype(dt)
        if n > 3:
            x[n // 3] = x[2 * n // 3] = x[np.argmax(np.abs(x))]          # a tie for the arg-max
        for op in ops:
            for S in ec.REDUCE_CUTS:
                plan = est.EstReducePlan(1, n, 1, op, dt, S)
                for off in range(4):
                    keep, ptr = _offset_copy(x, off)
                    out = torch.zeros(2, dtype=torch.int64, device="cuda")
                    plan.exec(ptr, out.data_ptr())
                    want = ec.est_reduce_emulate(x, op, S, off % V)[0]
                    got = out.cpu().numpy()[:len(want)]
                    assert np.array_equal(got, want.view(np.int64)), (n, op, S, off)
    # the strided route, and a NaN bin
    a = (rng.standard_normal((2, 70, 3)) + (1j * rng.standard_normal((2, 70, 3)) if dt.kind == "c" else 0)).astype(dt)
    if dt.kind == "c":
        a[1, 5, 2] = complex(np.nan, 0.0)
    for op in ops:
        plan = est.EstReducePlan(3, 70, 2, op, dt, 2)
        want = ec.est_reduce_emulate(a, op, 2)
        out = torch.zeros(want.size, dtype=torch.int64, device="cuda")
        plan.exec(torch.from_numpy(a).cuda().data_ptr(), out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), want.reshape(-1).view(np.int64)), op


def test_jacobsen_reference_cases(d):
    """test/estimation.jl:23-52, numpy and device input, Float64 and (at its own precision) Float32."""
    import torch
    for x, fc in ec.jacobsen_cases():
        got = d.jacobsen(x, ec.FS)
        assert isinstance(got, float) and abs(got - fc) <= 1e-5, (fc, got)
        assert d.jacobsen(torch.from_numpy(x).cuda(), ec.FS) == got
        assert abs(got - ref.jacobsen(x, ec.FS)) <= 1e-9
        x32 = x.astype(np.complex64 if x.dtype.kind == "c" else np.float32)
        assert abs(d.jacobsen(x32, ec.FS) - fc) <= 1e-3, fc              # delta from Float32 bins: 1e-5 is the Float64 figure
    assert abs(d.jacobsen(ec.jacobsen_cases()[1][0]) - 0.143) <= 1e-7     # Fs = 1.0


def test_jacobsen_other_lengths_and_the_nyquist_bin(d):
    t1 = np.arange(1018) / ec.FS                                         # 1018 = 2 x 509: not 7-smooth (501 = 3 x 167 is not either)
    for x, fc in ((np.cos(2 * np.pi * 17.3 * t1 + 0.3), 17.3), (np.exp(2j * np.pi * (-31.7 * t1 + 0.1)), -31.7)):
        assert abs(d.jacobsen(x, ec.FS) - fc) <= 1e-3 and abs(d.jacobsen(x, ec.FS) - ref.jacobsen(x, ec.FS)) <= 1e-9
    x = np.cos(np.pi * np.arange(512))                                   # the peak is the Nyquist bin of an even length: X[k+1] = conj(X[k-1])
    assert abs(d.jacobsen(x, ec.FS) - ec.FS / 2) <= 1e-9
    x = 2.0 + 1e-3 * np.cos(0.3 * np.arange(64))                         # the peak is DC: X[-1] = conj(X[1])
    assert d.jacobsen(x, ec.FS) <= 1e-2 and abs(d.jacobsen(x, ec.FS) - ref.jacobsen(x, ec.FS)) <= 1e-9
    assert abs(d.jacobsen(np.array([1.0, -1.0])) - 0.5) <= 1e-12         # N = 2
    assert np.isnan(d.jacobsen(np.array([1.0, np.nan, 0.5, 2.0])))


def test_quinn_reference_calls(d):
    """test/estimation.jl:66-79: the six calls, the reference's bounds, and agreement with the Float64 restatement within the CPU test's tolerance."""
    import torch
    sr, sc = ec.reference_signals()
    for x, truth, f0 in ((sr, 28.3, 50), (sc, -40.3, -20)):
        est, reached = d.quinn(x, f0, ec.FS)
        assert isinstance(est, float) and isinstance(reached, bool)
        want = ref.quinn(x, f0, ec.FS)
        print(f"quinn f0 {f0}: {est} against {want[0]}: differ by {abs(est - want[0]):.3g} Hz")
        assert not reached and abs(est - truth) <= 1e-3
        assert reached == want[1] and abs(est - want[0]) <= AGREE_TOL
        plan = d.QuinnPlan(x.dtype, len(x))
        assert plan.estimate(torch.from_numpy(x).cuda().data_ptr(), f0, ec.FS)[2] == want[2]      # iterations (17 from fs / 2)
        assert d.quinn(torch.from_numpy(x).cuda(), f0, ec.FS) == (est, reached)
        for fs in (ec.FS, None):                                         # the guess from jacobsen; then fs = 1.0 too
            args, scale = ((fs,), 1.0) if fs else ((), ec.FS)
            est, reached = d.quinn(x, *args)
            want = ref.quinn(x, d.jacobsen(x, *args), fs or 1.0)
            assert not reached and abs(est - truth / scale) <= 1e-3
            assert reached == want[1] and abs(est - want[0]) <= AGREE_TOL / scale
    est32, reached = d.quinn(sr.astype(np.float32), 50, ec.FS)
    assert not reached and abs(est32 - 28.3) <= 1e-3
    est32, reached = d.quinn(sc.astype(np.complex64), -20, ec.FS)
    assert not reached and abs(est32 + 40.3) <= 1e-3
    assert abs(d.quinn((1000 * sr).astype(np.int32), ec.FS)[0] - 28.3) <= 1e-3    # integers go through Float64


def test_repeat_calls_give_equal_results_and_reuse_plans(d):
    from dsp_jl_amd import _plancache
    sr, sc = ec.reference_signals()
    for x in (sr, sc, sr.astype(np.float32)):
        first = (d.jacobsen(x, ec.FS), d.quinn(x, ec.FS), d.quinn(x, 30.0, ec.FS, tol=1e-9, maxiters=3))
        hits = _plancache.plans.hits
        assert (d.jacobsen(x, ec.FS), d.quinn(x, ec.FS), d.quinn(x, 30.0, ec.FS, tol=1e-9, maxiters=3)) == first
        assert _plancache.plans.hits >= hits + 3


def test_iteration_limits_and_nan(d):
    sr, _ = ec.reference_signals()
    est, reached = d.quinn(sr, 50, ec.FS, maxiters=3)
    want = ref.quinn(sr, 50, ec.FS, maxiters=3)
    assert reached and want[1] and abs(est - want[0]) <= 1e-9
    x = sr.copy()
    x[100] = np.nan
    est, reached = d.quinn(x, 28.0, ec.FS)                               # a NaN runs to maxiters
    assert np.isnan(est) and reached
    est, reached = d.quinn(sr, float("nan"), ec.FS)
    assert np.isnan(est) and reached
    with pytest.raises(d.DomainError):                                   # beta = 100 (alpha - 1) = -100: the reference's acos throws
        d.quinn(np.array([0.0, 0.2]), 0.25, 1.0, maxiters=1)


def test_argument_errors(d):
    import torch
    from dsp_jl_amd import _lib
    for fn in (d.jacobsen, d.quinn):
        with pytest.raises(TypeError):
            fn(np.ones((4, 4)))
        with pytest.raises(TypeError):
            fn(torch.ones(4, 4, device="cuda"))
        with pytest.raises(d.ArgumentError):
            fn(np.ones(1))
        with pytest.raises(d.ArgumentError):
            fn(torch.ones(1, device="cuda"))
        with pytest.raises(d.UnsupportedError):
            fn(np.ones(8, dtype=np.float16))
        with pytest.raises(TypeError):
            fn(np.ones(8), "fast")
    with pytest.raises(TypeError):
        d.quinn(np.ones(8), 1.0, 2.0, 3.0)
    with pytest.raises(TypeError):
        d.quinn(np.ones(8), maxiters=2.5)
    plan = d.QuinnPlan(np.float64, 64)
    x = torch.ones(70, dtype=torch.float64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(d.ArgumentError):
        plan.pass_exec(0, 0.0, 1.0, out.data_ptr())
    with pytest.raises(d.ArgumentError):
        plan.pass_exec(x.data_ptr(), 0.0, 1.0, 0)
    with pytest.raises(d.ArgumentError):
        plan.pass_exec(x.data_ptr() + 4, 0.0, 1.0, out.data_ptr())        # not aligned to the element
    with pytest.raises(d.ArgumentError):
        plan.pass_exec(x.data_ptr(), 0.0, 1.0, out.data_ptr() + 4)
    with pytest.raises(d.UnsupportedError):
        d.QuinnPlan(np.float64, 70000).pass_exec(torch.ones(70000, dtype=torch.float64, device="cuda").data_ptr(), 0.0, 3.0, out.data_ptr())
    bins = torch.ones(9, dtype=torch.complex128, device="cuda")
    rec = torch.zeros(10, dtype=torch.int64, device="cuda")
    gather = _lib.lib().mdsp_est_peak_gather
    for args in ((bins.data_ptr(), 8, 16, 1, _lib.C64, rec.data_ptr(), rec.data_ptr() + 16, None), (bins.data_ptr(), 9, 16, 1, _lib.F64, rec.data_ptr(), rec.data_ptr() + 16, None),
                 (bins.data_ptr(), 1, 1, 0, _lib.C64, rec.data_ptr(), rec.data_ptr() + 16, None), (None, 9, 16, 1, _lib.C64, rec.data_ptr(), rec.data_ptr() + 16, None),
                 (bins.data_ptr(), 9, 16, 1, _lib.C64, rec.data_ptr() + 4, rec.data_ptr() + 16, None)):
        with pytest.raises(d.ArgumentError):
            _lib.check(gather(*args))
    torch.cuda.synchronize()
