"""Guard-band tests of mdsp_quinn_pass_exec, mdsp_est_reduce_exec and mdsp_est_peak_gather (INTEGRATION.md "What a call touches"; the layouts and
checks of tests/guard_bands.py as they are): the signal sits inside a larger allocation, 0 - 3 ELEMENTS off a 128-byte line, with a quiet-NaN poison all
around it, and the record goes into a buffer that holds another NaN pattern everywhere.  A pass or a reduction that read one sample outside the signal
would carry a NaN into its sums (or raise the NaN flag of ABS2ARGMAX) and differ from the host emulation; every word of the result buffer outside the
record must keep its pattern, every word inside must be written.  The workspace of a cut belongs to the plan; what the launches write into it is covered
by the bit equality of the record."""
import numpy as np
import pytest

import estimation_cases as ec
import guard_bands as gb

pytestmark = pytest.mark.gpu

GUARD = gb.MIN_GUARD
OFFSETS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_quinn_pass_stays_inside_the_signal_and_the_record(d, dt):
    import torch
    dt = np.dtype(dt)
    nrec = 3 if dt.kind == "c" else 4
    for n, S in ((2, 1), (3, 3), (ec.RUN + 1, 1), (ec.TILE - 1, 3), (ec.TILE + 1, 1), (2 * ec.TILE + 3, 3), ec.CARRY_CASE):
        x = ec.tone(n, 28.3, dt, seed=n)
        mean, param = ec.mean_of(x), ec.pass_param(28.3, dt)
        want = ec.pass_emulate(x, mean, param, S)
        plan = d.QuinnPlan(dt, n, S)
        for off in OFFSETS:
            what = f"quinn pass {dt.name} n {n} segments {S} offset {off}"
            lx = gb.layout(n, 1, n, GUARD, GUARD, off, dt)
            ly = gb.layout(nrec, 1, nrec, GUARD, GUARD, off % 2, np.float64)
            before = gb.new_input(lx, x.reshape(1, n))
            xd, yd = gb.to_device(before), gb.to_device(gb.new_output(ly))
            plan.pass_exec(gb.ptr(xd, lx), mean, param, gb.ptr(yd, ly))
            after = gb.from_device(yd)
            gb.check_output(after, ly, nrec, what)
            assert np.array_equal(gb.columns(after, ly).reshape(-1).view(np.uint64), want.view(np.uint64)), what
            assert np.array_equal(gb.from_device(xd), before), what + ": the signal's buffer changed"
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_est_reductions_stay_inside_their_arrays(d, dt):
    import torch
    from dsp_jl_amd import _lib, estimation as est
    dt = np.dtype(dt)
    V = 16 // dt.itemsize
    rng = np.random.default_rng(11)
    ops = (_lib.EST_SUM, _lib.EST_ABS2ARGMAX) if dt.kind == "c" else (_lib.EST_SUM,)
    for n in (1, 65, 257, ec.TILE + 1):
        x = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if dt.kind == "c" else 0)).astype(dt)
        for op in ops:
            words = 1 if (op == _lib.EST_SUM and dt.kind != "c") else 2
            for S in (1, 3):
                plan = est.EstReducePlan(1, n, 1, op, dt, S)
                for off in OFFSETS:
                    what = f"est_reduce op {op} {dt.name} n {n} segments {S} offset {off}"
                    lx = gb.layout(n, 1, n, GUARD, GUARD, off, dt)
                    ly = gb.layout(words, 1, words, GUARD, GUARD, off % 2, np.float64)
                    before = gb.new_input(lx, x.reshape(1, n))
                    xd, yd = gb.to_device(before), gb.to_device(gb.new_output(ly))
                    plan.exec(gb.ptr(xd, lx), gb.ptr(yd, ly))
                    after = gb.from_device(yd)
                    gb.check_output(after, ly, words, what)
                    want = ec.est_reduce_emulate(x, op, S, off % V)[0]
                    assert np.array_equal(gb.columns(after, ly).reshape(-1).view(np.int64), want.view(np.int64)), what
                    assert np.array_equal(gb.from_device(xd), before), what + ": the array's buffer changed"
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", [np.complex64, np.complex128], ids=lambda t: np.dtype(t).name)
def test_peak_gather_stays_inside_the_bins_and_the_record(d, dt):
    """Every bin index of a full and of a one-sided spectrum, the ends included: the neighbours come from inside the bins (poison outside would show as
    NaN in the record) and the 64 bytes of the record are all that is written."""
    import torch
    from dsp_jl_amd import _lib
    dt = np.dtype(dt)
    rng = np.random.default_rng(12)
    for n in (2, 9, 16):
        for onesided in (0, 1):
            nb = n // 2 + 1 if onesided else n
            bins = (rng.standard_normal(nb) + 1j * rng.standard_normal(nb)).astype(dt)
            for k in range(nb):
                what = f"peak gather {dt.name} n {n} onesided {onesided} k {k}"
                off = k % 4
                lx = gb.layout(nb, 1, nb, GUARD, GUARD, off, dt)
                ly = gb.layout(8, 1, 8, GUARD, GUARD, off % 2, np.float64)
                xd, yd = gb.to_device(gb.new_input(lx, bins.reshape(1, nb))), gb.to_device(gb.new_output(ly))
                arg = torch.tensor([k, 0], dtype=torch.int64, device="cuda")
                _lib.check(_lib.lib().mdsp_est_peak_gather(gb.ptr(xd, lx), nb, n, onesided, _lib.C32 if dt == np.complex64 else _lib.C64, arg.data_ptr(),
                                                           gb.ptr(yd, ly), torch.cuda.current_stream().cuda_stream))
                after = gb.from_device(yd)
                gb.check_output(after, ly, 8, what)
                assert np.array_equal(gb.columns(after, ly).reshape(-1).view(np.int64), ec.peak_emulate(bins, n, onesided, [k, 0])), what
    torch.cuda.synchronize()
