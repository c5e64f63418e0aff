"""GPU tests of the folded overlap-save kernel (real Float32, nfft 2048: ols_fused_kernel with FOLD -- twiddle and spectrum products that only feed
an add / subtract pair ride in the pair, fft_lds.h).  256 random unit-variance taps, block length L = 1793, fused engine, against the Float64
oracle with the overlap-save tolerance of the suite (TOL32 of tests/test_gpu_boundary.py).  A unit is two real blocks, so the signal lengths are
the smallest at which each path of the kernel can go wrong:

    1000            one block shorter than L; the unit has no second block
    1793            exactly one block
    3586            one full unit
    5 L + 3         an odd block count and a ragged end
    40 L + 17       21 units; with two columns the units cross a column boundary (41 blocks per column: the last unit of a column has one block)

The grid of a launch is min(units, CUs x workgroups per CU), so at these lengths every unit has a slot of its own.  The walk of several consecutive
units by one slot has a case of its own: MDSP_WG_PER_CU=1 and 3 CUs - 4 units (tests/run_schedule_cases.py has the arithmetic), so that every
slot walks a run of three units, the last run is partial and one slot idles; with MDSP_RUNS_PER_SLOT=2 runs of two, half of the slots a second
one.  A unit's arithmetic does not depend on who runs it, so those outputs equal the default schedule's bit for bit.

A unit impulse filters to the taps themselves: with an exact input the only roundings are the transforms' own, and every output must be within
4 ulp of the largest tap of its exact value (the taps shifted, zero elsewhere).

Measured on MI355X: relative error 1.1e-7 (nx 1000) to 1.8e-7 against the bound 5e-6, edges 1.7e-7 to 1.8e-7 against 2.5e-5, impulse 1.28 and 1.5 ulp."""
import numpy as np
import pytest

import run_schedule_cases as rs
from conftest import relerr
from test_gpu_boundary import TOL32

pytestmark = pytest.mark.gpu

NB, NFFT = 256, 2048
L = NFFT - NB + 1
LENGTHS = (1000, L, 2 * L, 5 * L + 3, 40 * L + 17)
NCOLS = 2


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def case():
    """Taps, two columns of the longest signal and their Float64 references, computed once (shorter cases are prefixes: filt is causal)."""
    from oracle import dspbase as odsp
    rng = np.random.default_rng(1776)
    b = rng.standard_normal(NB).astype(np.float32)
    x = rng.standard_normal((LENGTHS[-1], NCOLS)).astype(np.float32)
    ref = np.stack([odsp.filt_ba(b.astype(np.float64), 1.0, x[:, c].astype(np.float64)) for c in range(NCOLS)], axis=1)
    assert L == 1793
    return b, x, ref


@pytest.mark.parametrize("nx", LENGTHS)
def test_folded_kernel_against_the_oracle(d, case, nx):
    b, x, ref = case
    y = np.asarray(d.fftfilt(b, np.ascontiguousarray(x[:nx, 0]), NFFT, engine=d.ENGINE_FUSED))
    assert y.shape == (nx,) and y.dtype == np.float32
    e = relerr(y, ref[:nx, 0])
    print("nx", nx, "relerr", e)
    assert e < TOL32, (nx, e)
    if nx == LENGTHS[-1]:   # the edges carry the zero padding in front of the signal and the clamped last block
        e0, e1 = relerr(y[:3000], ref[:3000, 0]), relerr(y[-3000:], ref[-3000:, 0])
        print("first / last 3000 outputs", e0, e1)
        assert e0 < 5 * TOL32 and e1 < 5 * TOL32, (e0, e1)


def test_folded_kernel_two_columns(d, case):
    b, x, ref = case
    y = np.asarray(d.fftfilt(b, x, NFFT, engine=d.ENGINE_FUSED))
    assert y.shape == x.shape
    for c in range(NCOLS):
        e = relerr(y[:, c], ref[:, c])
        e0, e1 = relerr(y[:3000, c], ref[:3000, c]), relerr(y[-3000:, c], ref[-3000:, c])
        print("column", c, "relerr", e, "edges", e0, e1)
        assert e < TOL32, (c, e)
        assert e0 < 5 * TOL32 and e1 < 5 * TOL32, (c, e0, e1)
    # a column's arithmetic does not depend on its neighbours
    one = np.asarray(d.fftfilt(b, np.ascontiguousarray(x[:, 1]), NFFT, engine=d.ENGINE_FUSED))
    assert np.array_equal(one, y[:, 1])


def test_folded_kernel_several_units_per_slot(d):
    import torch
    from dsp_jl_amd import _lib
    from oracle import dspbase as odsp
    ns = rs.slots(torch.cuda.get_device_properties(0).multi_processor_count, 1, 1, "ols")
    units = rs.units_for(ns)
    assert rs.schedule(units, ns, 1)[0] == 3 and rs.schedule(units, ns, 2)[0] == 2
    nx = (2 * units - 2) * L + L // 2 + 3              # an odd block count: the last unit has one block, and that one ragged
    rng = np.random.default_rng(1777)
    b = rng.standard_normal(NB).astype(np.float32)
    x = rng.standard_normal(nx).astype(np.float32)
    ref = odsp.filt_ba(b.astype(np.float64), 1.0, x.astype(np.float64))
    xd = torch.from_numpy(x).cuda()
    dflt = d.fftfilt(b, xd, NFFT, engine=d.ENGINE_FUSED).cpu().numpy()
    for runs in (1, 2):
        try:
            _lib.set_tunable("MDSP_WG_PER_CU", 1)
            _lib.set_tunable("MDSP_RUNS_PER_SLOT", runs)
            y = d.fftfilt(b, xd, NFFT, engine=d.ENGINE_FUSED).cpu().numpy()
        finally:
            _lib.set_tunable("MDSP_WG_PER_CU", None)
            _lib.set_tunable("MDSP_RUNS_PER_SLOT", None)
        e = relerr(y, ref)
        e0, e1 = relerr(y[:3000], ref[:3000]), relerr(y[-3000:], ref[-3000:])
        print("runs per slot", runs, "units", units, "slots", ns, "relerr", e, "edges", e0, e1)
        assert e < TOL32, (runs, e)
        assert e0 < 5 * TOL32 and e1 < 5 * TOL32, (runs, e0, e1)
        assert np.array_equal(y, dflt), (runs, "first differing sample", int(np.flatnonzero(y != dflt)[0]))


@pytest.mark.parametrize("at", [0, L - 1])
def test_unit_impulse_gives_the_taps(d, case, at):
    b = case[0]
    nx = 2 * L
    x = np.zeros(nx, np.float32)
    x[at] = 1.0
    want = np.zeros(nx, np.float64)
    want[at:at + NB] = b
    y = np.asarray(d.fftfilt(b, x, NFFT, engine=d.ENGINE_FUSED)).astype(np.float64)
    ulp = float(np.spacing(np.float32(np.abs(b).max())))
    worst = float(np.abs(y - want).max()) / ulp
    print("impulse at", at, "largest error", worst, "ulp of the largest tap")
    assert worst <= 4.0, (at, worst)
