"""GPU tests of the run schedule of the streaming tiled overlap-save kernel (DESIGN.md 4.2 *Run schedule*; dsp.jl_amd/csrc/ols_plan.h ols_run_rule): the
slots of a streaming launch walk short runs of consecutive units, run r of slot s at unit (r slots + s) run_len, instead of one run per slot ("whole").
A unit's arithmetic does not depend on who runs it, and the two lead elements a run start loads are the bits the unit in front would have handed
over in registers: every schedule must give the same outputs BIT FOR BIT.

The streaming instantiation is forced (MDSP_OLS_STREAM=2) and the grid is one workgroup per CU (MDSP_WG_PER_CU=1), as tests/test_gpu_run_schedules.py
sizes its grids; the columns hold just under 7 units per slot, so whole is a run of 7, runs of 2 and 3 leave a partial last run per slot and dead iterations
(niter 8 and 9), and the last round has idle slots.  Compared against whole (MDSP_OLS_RUN_LEN clamped to one run per slot): the forced lengths 1 --
where nothing is ever carried in registers --, 2 and 3, and the rule's own choice (knob unset; at these sizes one run per slot: the rule's line is
held by tests/test_ols_run_rule_cpu.py).  Whole itself is held, bit for bit, to the plain
instantiation on the default grid, which the rest of the suite checks against the oracle.

Shapes, the smallest that reach each path: one column with an odd tile count and a ragged end; three columns of a unit count that no run length
divides, so runs cross the column boundaries (where nothing may be carried), columns 1 and 2 off the cache line; nx one sample short of and one past
whole tiles; 249 and 257 taps; CONV.  One guard-band case per run length (tests/guard_bands.py): three columns inside a larger allocation, x shifted by
3 elements and y by 1, nothing outside [0, nout) of a column written, no poisoned sample used.  No tolerances: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import guard_bands as gb

pytestmark = pytest.mark.gpu

NB, NFFT, TILE, LEAD = 256, 2048, 1792, 256
WHOLE = 1 << 20                    # MDSP_OLS_RUN_LEN: clamped to one run per slot
LENGTHS = (1, 2, 3, None)          # None: the knob unset, the rule's choice
PER_SLOT = 7
NCOLS = 3


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def slots(d):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count      # one transform per workgroup, one workgroup per CU


@pytest.fixture(scope="module")
def data(slots):
    """Taps and three columns of the longest signal, made once (shorter cases are prefixes)."""
    rng = np.random.default_rng(1796)
    nmax = 2 * (PER_SLOT * slots - 4) * TILE + 1
    return {nb: rng.standard_normal(nb).astype(np.float32) for nb in (249, NB, 257)}, rng.standard_normal((NCOLS, nmax)).astype(np.float32)


class _Knobs:
    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        from dsp_jl_amd import _lib
        for k, v in self.knobs.items():
            _lib.set_tunable(k, v)

    def __exit__(self, *exc):
        from dsp_jl_amd import _lib
        for k in self.knobs:
            _lib.set_tunable(k, None)


def _small_streaming(run_len):
    return _Knobs(MDSP_OLS_STREAM=2, MDSP_WG_PER_CU=1, MDSP_OLS_RUN_LEN=run_len)


def _plan(taps, nx, conv=False):
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    plan = OlsPlan(np.ascontiguousarray(taps), NFFT, nx, _lib.OLS_CONV if conv else _lib.OLS_FILT, _lib.ENGINE_FUSED)
    t, l = C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_ols_plan_tile(plan._h, C.byref(t), C.byref(l)))
    assert (t.value, l.value) == (TILE, LEAD)
    return plan


def _run(plan, cols, nout=None):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(cols)).cuda()
    return plan.exec(xd, cols.shape[1] if nout is None else nout).cpu().numpy()


def _units(nout, ncols):
    return (-(-nout // TILE) + 1) // 2 * ncols


def _schedule(units, slots):
    """(run_len, niter) of a streaming launch under the knobs as they stand."""
    from dsp_jl_amd import _lib
    rl, ni = C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_ols_run_for(units, min(units, slots), 1, C.byref(rl), C.byref(ni)))
    return rl.value, ni.value


def _compare(plan, cols, nout, slots, what, expect_whole=PER_SLOT):
    """Every run length against whole, whole against the plain kernel on the default grid."""
    units = _units(nout, cols.shape[0])
    plain = _run(plan, cols, nout)
    with _small_streaming(WHOLE):
        assert _schedule(units, slots) == (expect_whole, expect_whole), what
        whole = _run(plan, cols, nout)
    assert np.array_equal(whole, plain), (what, "whole against the plain kernel")
    for run_len in LENGTHS:
        with _small_streaming(run_len):
            rl, niter = _schedule(units, slots)
            if run_len is not None:
                assert rl == run_len and niter == -(-expect_whole // rl) * rl, (what, run_len, rl, niter)
            y = _run(plan, cols, nout)
        for c in range(cols.shape[0]):
            same = y[c] == whole[c]
            assert same.all(), (what, "run length", run_len, "column", c, "first differing sample", int(np.flatnonzero(~same)[0]), "of", int((~same).sum()))


def _one_column_nx(slots):
    units = PER_SLOT * slots - 4
    while units % 2 == 0 or units % 3 == 0:                       # no forced run length divides the units: the last run of all is partial too
        units -= 1
    return units, (2 * units - 2) * TILE + TILE // 2 + 3          # an odd tile count: the last unit has one block, and that one ragged


@pytest.mark.parametrize("nb", [249, NB, 257])
def test_one_column_partial_last_run(d, slots, data, nb):
    taps, x = data
    units, nx = _one_column_nx(slots)
    assert _units(nx, 1) == units and -(-units // slots) == PER_SLOT and units % 2 and units % 3
    _compare(_plan(taps[nb], nx), x[:1, :nx], nx, slots, f"{nb} taps, one column")


def test_conv(d, slots, data):
    taps, x = data
    units, nx = _one_column_nx(slots)
    nout = nx + NB - 1
    assert _units(nout, 1) == units
    _compare(_plan(taps[NB], nx, conv=True), x[:1, :nx], nout, slots, "conv")


@pytest.mark.parametrize("edge", [-1, +1], ids=["one-short", "one-past"])
def test_whole_tiles_less_and_plus_one_sample(d, slots, data, edge):
    taps, x = data
    units = PER_SLOT * slots - 4
    nx = 2 * units * TILE + edge                                      # one past: a last unit of one block of one sample
    assert _units(nx, 1) == units + (edge > 0) and -(-_units(nx, 1) // slots) == PER_SLOT
    _compare(_plan(taps[NB], nx), x[:1, :nx], nx, slots, f"nx = whole tiles {edge:+d}")


def _three_column_shape(slots):
    upc = -(-(PER_SLOT * slots - 4) // NCOLS)
    while not (upc % 2 and upc % 3 and upc % PER_SLOT and -(-NCOLS * upc // slots) == PER_SLOT and (NCOLS * upc) % PER_SLOT):
        upc -= 1
    return upc, (2 * upc - 2) * TILE + TILE // 2 + 3


def test_three_columns_boundary_inside_a_run(d, slots, data):
    taps, x = data
    upc, nx = _three_column_shape(slots)
    assert _units(nx, NCOLS) == NCOLS * upc and nx % 32 != 0          # columns 1 and 2 start off a cache line
    _compare(_plan(taps[NB], nx), x[:, :nx], nx, slots, "three columns")


@pytest.mark.parametrize("run_len", LENGTHS, ids=lambda v: "rule" if v is None else str(v))
def test_guard_bands(d, slots, data, run_len):
    from dsp_jl_amd import _lib, _dev
    taps, x = data
    upc, nx = _three_column_shape(slots)
    plan = _plan(taps[NB], nx)
    guard = max(gb.MIN_GUARD, NFFT)
    with _small_streaming(WHOLE):
        whole = _run(plan, x[:, :nx])
    lx = gb.layout(nx, NCOLS, nx + 5, guard, guard, 3, np.float32)
    ly = gb.layout(nx, NCOLS, nx + 7, guard, guard, 1, np.float32)
    xd, yd = gb.to_device(gb.new_input(lx, x[:, :nx])), gb.to_device(gb.new_output(ly))
    with _small_streaming(run_len):
        _lib.check(_lib.lib().mdsp_ols_exec(plan._h, gb.ptr(xd, lx), nx, NCOLS, lx.ld, gb.ptr(yd, ly), nx, ly.ld, _dev.stream_ptr()))
    after = gb.from_device(yd)
    gb.check_output(after, ly, nx, f"run length {run_len}")
    y = gb.columns(after, ly)
    for c in range(NCOLS):
        assert np.array_equal(y[c], whole[c]), (run_len, c)
