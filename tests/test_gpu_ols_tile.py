"""GPU tests of the tiled overlap-save plans (real Float32, nfft 2048, fused engine; DESIGN.md 4.2, dsp.jl_amd/csrc/ols_plan.h): the whole-column call
runs windows of TILE = 1792 outputs that start LEAD = 256 samples early instead of blocks of L = 1793 with 255 samples of history, ols_fused_kernel
with TILED.  A unit is two windows; block b's first two elements per thread are block a's last two, and the first two of the next consecutive unit of
a slot are carried in registers.  256 random unit-variance taps against the Float64 oracle with the overlap-save tolerance of the suite (TOL32 of
tests/test_gpu_boundary.py, 5 x at the first and last 3000 outputs).  Lengths: the smallest at which each path can go wrong --

    1000            shorter than a tile; the unit has no second block (its lead elements are zeros, not copies)
    1792            exactly one tile
    1793            the second block holds one sample
    3584            one full unit
    5 TILE + 3      an odd tile count and a ragged end
    40 TILE + 17    two columns, the second one not on a cache line (ldx = 71697); 41 tiles per column: the last unit of a column has one block

The grid of a launch is min(units, CUs x workgroups per CU): at these lengths every unit has a slot of its own and nothing is carried.  The carry has
cases of its own: MDSP_WG_PER_CU=1 and 3 slots - 4 units (tests/run_schedule_cases.py), every slot a run of three units, then MDSP_RUNS_PER_SLOT=2;
both must equal the default schedule bit for bit (carried registers against loaded ones) -- also with two columns sized so that a run crosses the
column boundary, where nothing may be carried.

Tolerances: TOL32 is the suite's; the impulse bound (4 ulp of the largest tap) is the folded kernel's (tests/test_gpu_ols_fold.py): an exact input
leaves the transforms' own roundings only.  Bit-for-bit comparisons need none.

Measured on MI355X: relative error 1.1e-7 (nx 1000) to 1.8e-7 against the bound 5e-6, edges 1.5e-7 to 1.8e-7 against 2.5e-5, impulse 1, 2 and 1 ulp."""
import ctypes as C

import numpy as np
import pytest

import run_schedule_cases as rs
from conftest import relerr
from test_gpu_boundary import TOL32

pytestmark = pytest.mark.gpu

NB, NFFT, TILE, LEAD = 256, 2048, 1792, 256
L = NFFT - NB + 1
P_MAX = 8                                    # DESIGN.md 4.2 (tests/test_ols_tile_rule_cpu.py holds the rule to it)
LENGTHS = (1000, TILE, TILE + 1, 2 * TILE, 5 * TILE + 3, 40 * TILE + 17)
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
    rng = np.random.default_rng(1792)
    b = rng.standard_normal(NB).astype(np.float32)
    x = rng.standard_normal((LENGTHS[-1], NCOLS)).astype(np.float32)
    ref = np.stack([odsp.filt_ba(b.astype(np.float64), 1.0, x[:, c].astype(np.float64)) for c in range(NCOLS)], axis=1)
    return b, x, ref


def _plan(taps, nx, mode=None, tile=None):
    """An owned plan of the fused engine (never the library's plan cache: the knob is read when a plan is made).  tile: MDSP_OLS_TILE for its creation."""
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    try:
        if tile is not None:
            _lib.set_tunable("MDSP_OLS_TILE", tile)
        return OlsPlan(np.ascontiguousarray(taps), NFFT, nx, _lib.OLS_FILT if mode is None else mode, _lib.ENGINE_FUSED)
    finally:
        if tile is not None:
            _lib.set_tunable("MDSP_OLS_TILE", None)


def _tile_of(plan):
    from dsp_jl_amd import _lib
    t, l = C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_ols_plan_tile(plan._h, C.byref(t), C.byref(l)))
    return t.value, l.value


def _run(plan, cols, nout=None):
    """cols: (ncols, nx) numpy -> (ncols, nout) numpy through the whole-column call."""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(cols)).cuda()
    return plan.exec(xd, cols.shape[1] if nout is None else nout).cpu().numpy()


def _check(y, ref, what):
    e = relerr(y, ref)
    e0, e1 = relerr(y[:3000], ref[:3000]), relerr(y[-3000:], ref[-3000:])
    print(what, "relerr", e, "first / last 3000 outputs", e0, e1)
    assert e < TOL32, (what, e)
    assert e0 < 5 * TOL32 and e1 < 5 * TOL32, (what, e0, e1)


@pytest.mark.parametrize("nx", LENGTHS[:-1])
def test_tiled_kernel_against_the_oracle(d, case, nx):
    b, x, ref = case
    plan = _plan(b, nx)
    assert _tile_of(plan) == (TILE, LEAD) and plan.block_len == L
    y = _run(plan, x[:nx, 0][None, :])[0]
    assert y.shape == (nx,) and y.dtype == np.float32
    _check(y, ref[:nx, 0], f"nx {nx}")


def test_tiled_kernel_two_columns(d, case):
    b, x, ref = case
    nx = LENGTHS[-1]
    assert nx % 32 != 0 and -(-nx // TILE) % 2 == 1      # the second column starts off a cache line; the last unit of a column has one block
    plan = _plan(b, nx)
    y = _run(plan, x.T)
    for c in range(NCOLS):
        _check(y[c], ref[:, c], f"column {c}")
    for c in range(NCOLS):                               # a column's arithmetic depends neither on its neighbours nor on its alignment
        one = _run(plan, x[:, c][None, :])[0]
        assert np.array_equal(one, y[c]), c


def _scheduled(plan, cols, runs):
    from dsp_jl_amd import _lib
    try:
        _lib.set_tunable("MDSP_WG_PER_CU", 1)
        _lib.set_tunable("MDSP_RUNS_PER_SLOT", runs)
        return _run(plan, cols)
    finally:
        _lib.set_tunable("MDSP_WG_PER_CU", None)
        _lib.set_tunable("MDSP_RUNS_PER_SLOT", None)


def test_carried_registers_equal_loaded_ones(d):
    import torch
    from oracle import dspbase as odsp
    ns = rs.slots(torch.cuda.get_device_properties(0).multi_processor_count, 1, 1, "ols")
    units = rs.units_for(ns)
    assert rs.schedule(units, ns, 1)[0] == 3 and rs.schedule(units, ns, 2)[0] == 2
    nx = (2 * units - 2) * TILE + TILE // 2 + 3          # an odd tile count: the last unit has one block, and that one ragged
    rng = np.random.default_rng(1793)
    b = rng.standard_normal(NB).astype(np.float32)
    x = rng.standard_normal((1, nx)).astype(np.float32)
    plan = _plan(b, nx)
    assert _tile_of(plan) == (TILE, LEAD)
    dflt = _run(plan, x)
    _check(dflt[0], odsp.filt_ba(b.astype(np.float64), 1.0, x[0].astype(np.float64)), "default schedule")
    for runs in (1, 2):
        y = _scheduled(plan, x, runs)
        assert np.array_equal(y, dflt), (runs, "first differing sample", int(np.flatnonzero(y[0] != dflt[0])[0]))


def test_no_carry_across_a_column_boundary(d):
    import torch
    ns = rs.slots(torch.cuda.get_device_properties(0).multi_processor_count, NCOLS, 1, "ols")
    upc = rs.ols_units_per_col(ns, NCOLS)
    while True:                                          # units per column that neither run length divides: a run of either schedule crosses the boundary
        r1, r2 = rs.schedule(NCOLS * upc, ns, 1)[0], rs.schedule(NCOLS * upc, ns, 2)[0]
        if r1 >= 3 and upc % r1 and r2 >= 2 and upc % r2:
            break
        upc += 1
    nx = (2 * upc - 2) * TILE + TILE // 2 + 3            # 2 upc - 1 tiles per column
    rng = np.random.default_rng(1794)
    b = rng.standard_normal(NB).astype(np.float32)
    x = rng.standard_normal((NCOLS, nx)).astype(np.float32)
    plan = _plan(b, nx)
    dflt = _run(plan, x)
    for c in range(NCOLS):
        assert np.array_equal(_run(plan, x[c][None, :])[0], dflt[c]), c
    for runs in (1, 2):
        y = _scheduled(plan, x, runs)
        for c in range(NCOLS):
            assert np.array_equal(y[c], dflt[c]), (runs, c, "first differing sample", int(np.flatnonzero(y[c] != dflt[c])[0]))


@pytest.mark.parametrize("nb,tiled", [(257, True), (NB - P_MAX + 1, True), (NB - P_MAX, False)], ids=["p0", "pmax", "pmax+1"])
def test_other_tap_counts(d, nb, tiled):
    from oracle import dspbase as odsp
    nx = 5 * TILE + 3
    rng = np.random.default_rng(1795 + nb)
    b = rng.standard_normal(nb).astype(np.float32)
    x = rng.standard_normal((1, nx)).astype(np.float32)
    plan = _plan(b, nx)
    assert _tile_of(plan) == ((TILE, LEAD) if tiled else (NFFT - nb + 1, nb - 1))
    _check(_run(plan, x)[0], odsp.filt_ba(b.astype(np.float64), 1.0, x[0].astype(np.float64)), f"{nb} taps")


def test_conv_mode(d, case):
    from dsp_jl_amd import _lib
    b, x, _ = case
    nx = 5 * TILE + 3
    plan = _plan(b, nx, mode=_lib.OLS_CONV)
    assert _tile_of(plan) == (TILE, LEAD)
    y = _run(plan, x[:nx, 0][None, :], nx + NB - 1)[0]
    assert y.shape == (nx + NB - 1,)
    _check(y, np.convolve(x[:nx, 0].astype(np.float64), b.astype(np.float64)), "conv")


@pytest.mark.parametrize("at", [0, TILE - 1, TILE])
def test_unit_impulse_gives_the_taps(d, case, at):
    b = case[0]
    nx = 2 * TILE + NB
    x = np.zeros((1, nx), np.float32)
    x[0, at] = 1.0
    want = np.zeros(nx, np.float64)
    want[at:at + NB] = b
    y = _run(_plan(b, nx), x)[0].astype(np.float64)
    ulp = float(np.spacing(np.float32(np.abs(b).max())))
    worst = float(np.abs(y - want).max()) / ulp
    print("impulse at", at, "largest error", worst, "ulp of the largest tap")
    assert worst <= 4.0, (at, worst)


def test_knob_and_block_ranges(d, case):
    """MDSP_OLS_TILE=0: the plan runs the public blocks, as every plan did before the rule; both forms pass the oracle check.  mdsp_ols_exec_range keeps the
    public block grid on a tiled plan (the untiled kernel, nothing read in front of the slice): its outputs are the untiled plan's, bit for bit."""
    import torch
    from dsp_jl_amd import _lib, _dev
    b, x, ref = case
    nx = 9 * L + 5
    col = x[:nx, 0][None, :]
    tiled, plain = _plan(b, nx), _plan(b, nx, tile=0)
    assert _tile_of(tiled) == (TILE, LEAD) and _tile_of(plain) == (L, NB - 1)
    assert _tile_of(_plan(b, nx)) == (TILE, LEAD)                   # the knob is back
    yt, yp = _run(tiled, col)[0], _run(plain, col)[0]
    _check(yt, ref[:nx, 0], "tiled")
    _check(yp, ref[:nx, 0], "MDSP_OLS_TILE=0")
    xd = torch.from_numpy(np.ascontiguousarray(col[0])).cuda()
    got = torch.full((nx,), float("nan"), dtype=torch.float32, device="cuda")
    nblocks = -(-nx // L)
    for g0, cnt in ((0, 2), (2, 4), (6, nblocks)):                  # even starts; the last range is clipped to the grid
        g1 = min(nblocks, g0 + cnt)
        lo, hi = max(0, g0 * L - (NB - 1)), min(nx, g1 * L)
        o0, o1 = g0 * L, min(nx, g1 * L)
        xs = xd[lo:hi].clone()                                       # a slice that holds nothing but what the blocks read
        ys = torch.empty(o1 - o0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().mdsp_ols_exec_range(tiled._h, _dev.ptr(xs), lo, hi - lo, nx, _dev.ptr(ys), g0, cnt, nx, _dev.stream_ptr()))
        got[o0:o1] = ys
    assert np.array_equal(got.cpu().numpy(), yp)
