"""GPU tests of the streaming instantiation of the tiled overlap-save kernel (dsp.jl_amd/csrc/ols.hip: AUXL / AUXS of ols_fused_kernel;
the footprint rule: csrc/ols_plan.h).  A cache policy changes no arithmetic: with MDSP_OLS_STREAM = 2 (every launch of a tiled plan streams) the
outputs must equal those of MDSP_OLS_STREAM = 0 (never) BIT FOR BIT, and pass the Float64-oracle bar of tests/test_gpu_ols_tile.py.  256 taps, nfft
2048, Float32, owned plans of the fused engine.  The knob is read at launch, so one plan runs both forms.

Shapes: the smallest at which each path of the tiled kernel runs (tests/test_gpu_ols_tile.py has the reasons) --
    3 slots - 4 units under MDSP_WG_PER_CU=1   runs of three units (the register carry next to streamed loads), a partial last run, an idle slot;
                                               then MDSP_RUNS_PER_SLOT=2
    two columns of 40 TILE + 17 samples        the second column sits off a 128-byte line (ldx = nx, not a multiple of 32 samples): streamed stores of
                                               partial lines
    conv mode, nx = k TILE -+ 1, 249 / 257 taps
Visibility: a streaming store must be seen by whatever follows the kernel in stream order -- a reduction on the same stream, a second stream behind an
event, a device-to-host copy -- without any synchronisation of the test's own in between.
mdsp_ols_exec_range (the untiled kernel: never streams) and mdsp_ols_exec_host (chunks of the tile grid) return what they return under the plain policy.

Tolerances: none of its own.  Bit-for-bit comparisons, an exact integer reduction, and _check of tests/test_gpu_ols_tile.py (TOL32, 5 x at the edges)."""
import ctypes as C

import numpy as np
import pytest

import run_schedule_cases as rs
from test_gpu_ols_tile import LEAD, NB, NFFT, TILE, L, _check, _plan, _run, _tile_of

pytestmark = pytest.mark.gpu

NX2 = 40 * TILE + 17                         # the two-column case
NXS = 5 * TILE + 3                           # the small cases


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


@pytest.fixture(scope="module")
def sched(d):
    """(slots, units, nx) of the run-of-three case on this device."""
    import torch
    ns = rs.slots(torch.cuda.get_device_properties(0).multi_processor_count, 1, 1, "ols")
    units = rs.units_for(ns)
    assert rs.schedule(units, ns, 1)[0] == 3 and rs.schedule(units, ns, 2)[0] == 2
    return ns, units, (2 * units - 2) * TILE + TILE // 2 + 3      # an odd tile count: the last unit has one block, and that one ragged


@pytest.fixture(scope="module")
def case(sched):
    """Taps, one long column and a second shorter one with their Float64 references, computed once (shorter cases are prefixes: filt is causal)."""
    from oracle import dspbase as odsp
    nx = sched[2]
    rng = np.random.default_rng(2818)
    b = rng.standard_normal(NB).astype(np.float32)
    x0 = rng.standard_normal(nx).astype(np.float32)
    x1 = rng.standard_normal(NX2).astype(np.float32)
    ref0 = odsp.filt_ba(b.astype(np.float64), 1.0, x0.astype(np.float64))
    ref1 = odsp.filt_ba(b.astype(np.float64), 1.0, x1.astype(np.float64))
    for a in (b, x0, x1, ref0, ref1):
        a.setflags(write=False)
    return b, x0, x1, ref0, ref1


class _knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from dsp_jl_amd import _lib
        for k, v in self.kv.items():
            _lib.set_tunable(k, v)

    def __exit__(self, *exc):
        from dsp_jl_amd import _lib
        for k in self.kv:
            _lib.set_tunable(k, None)


def _both(plan, cols, nout=None, **knobs):
    """The whole-column call under MDSP_OLS_STREAM = 0 and = 2 (and `knobs`); asserts that the two agree bit for bit and returns the outputs."""
    assert _tile_of(plan) == (TILE, LEAD)
    with _knobs(MDSP_OLS_STREAM=0, **knobs):
        plain = _run(plan, cols, nout)
    with _knobs(MDSP_OLS_STREAM=2, **knobs):
        streamed = _run(plan, cols, nout)
    for c in range(cols.shape[0]):
        same = np.array_equal(streamed[c], plain[c])
        assert same, (c, "first differing sample", int(np.flatnonzero(streamed[c] != plain[c])[0]))
    return streamed


@pytest.mark.parametrize("runs", [1, 2])
def test_runs_of_several_units(d, case, sched, runs):
    b, x0, _, ref0, _ = case
    nx = sched[2]
    y = _both(_plan(b, nx), x0[None, :], MDSP_WG_PER_CU=1, MDSP_RUNS_PER_SLOT=runs)
    _check(y[0], ref0, f"runs per slot {runs}")


def test_two_columns_off_a_line_boundary(d, case):
    b, x0, x1, ref0, ref1 = case
    assert NX2 % 32 != 0
    cols = np.stack([x0[:NX2], x1])
    y = _both(_plan(b, NX2), cols)
    _check(y[0], ref0[:NX2], "column 0")
    _check(y[1], ref1, "column 1")


def test_conv_mode(d, case):
    from dsp_jl_amd import _lib
    b, x0 = case[0], case[1]
    y = _both(_plan(b, NXS, mode=_lib.OLS_CONV), x0[None, :NXS], NXS + NB - 1)
    assert y.shape == (1, NXS + NB - 1)
    _check(y[0], np.convolve(x0[:NXS].astype(np.float64), b.astype(np.float64)), "conv")


@pytest.mark.parametrize("nx", [6 * TILE - 1, 6 * TILE + 1], ids=["short", "past"])
def test_one_sample_off_whole_tiles(d, case, nx):
    b, x0, _, ref0, _ = case
    y = _both(_plan(b, nx), x0[None, :nx])
    _check(y[0], ref0[:nx], f"nx {nx}")


@pytest.mark.parametrize("nb", [249, 257])
def test_ends_of_the_tile_rule(d, case, nb):
    from oracle import dspbase as odsp
    x0 = case[1]
    bb = np.random.default_rng(2818 + nb).standard_normal(nb).astype(np.float32)
    y = _both(_plan(bb, NXS), x0[None, :NXS])
    _check(y[0], odsp.filt_ba(bb.astype(np.float64), 1.0, x0[:NXS].astype(np.float64)), f"{nb} taps")


def _bits_sum(t):
    """An exact, order-independent reduction over a Float32 tensor: the sum of its bit patterns as 64-bit integers."""
    import torch
    return t.view(torch.int32).to(torch.int64).sum()


def test_streamed_outputs_are_visible_in_stream_order(d, case):
    import torch
    b, x0 = case[0], case[1]
    nx = NX2
    plan = _plan(b, nx)
    xd = torch.from_numpy(np.ascontiguousarray(x0[None, :nx])).cuda()
    with _knobs(MDSP_OLS_STREAM=0):
        plain = plan.exec(xd, nx)
        torch.cuda.synchronize()
        want_sum, want = int(_bits_sum(plain).item()), plain.cpu().numpy()
    with _knobs(MDSP_OLS_STREAM=2):
        # the same stream, nothing in between
        y = plan.exec(xd, nx)
        s_same = _bits_sum(y)
        # a second stream behind an event
        y2 = plan.exec(xd, nx)
        ev = torch.cuda.Event()
        ev.record()
        other = torch.cuda.Stream()
        other.wait_event(ev)
        with torch.cuda.stream(other):
            s_other = _bits_sum(y2)
        y2.record_stream(other)
        # a device-to-host copy in stream order
        y3 = plan.exec(xd, nx)
        host = y3.cpu().numpy()
        other.synchronize()
        assert int(s_same.item()) == want_sum
        assert int(s_other.item()) == want_sum
        assert np.array_equal(host, want)


def test_block_ranges_and_host_chunks_keep_their_results(d, case):
    import torch
    from dsp_jl_amd import _lib, _dev
    b, x0 = case[0], case[1]
    nx = 9 * L + 5
    plan = _plan(b, nx)
    assert _tile_of(plan) == (TILE, LEAD)
    xd = torch.from_numpy(np.ascontiguousarray(x0[:nx])).cuda()
    nblocks = -(-nx // L)

    def ranges():
        got = torch.full((nx,), float("nan"), dtype=torch.float32, device="cuda")
        for g0, cnt in ((0, 2), (2, 4), (6, nblocks)):
            g1 = min(nblocks, g0 + cnt)
            lo, hi = max(0, g0 * L - (NB - 1)), min(nx, g1 * L)
            o0, o1 = g0 * L, min(nx, g1 * L)
            xs = xd[lo:hi].clone()
            ys = torch.empty(o1 - o0, dtype=torch.float32, device="cuda")
            _lib.check(_lib.lib().mdsp_ols_exec_range(plan._h, _dev.ptr(xs), lo, hi - lo, nx, _dev.ptr(ys), g0, cnt, nx, _dev.stream_ptr()))
            got[o0:o1] = ys
        return got.cpu().numpy()

    nh = 300 * TILE + 11                                            # three chunks of 144 tiles at 1 MiB per chunk
    assert nh <= len(x0)
    xh = np.ascontiguousarray(x0[None, :nh])
    hplan = _plan(b, nh)
    out = {}
    for knob in (0, 2):
        with _knobs(MDSP_OLS_STREAM=knob, MDSP_HOST_CHUNK_MIB=1):   # 1 MiB chunks: several launches over the tile grid
            out[knob] = (ranges(), hplan.exec_host(xh, nh), _run(hplan, xh))
    assert not np.isnan(out[0][0]).any()
    assert np.array_equal(out[2][0], out[0][0])
    assert np.array_equal(out[2][1], out[0][1])
    assert np.array_equal(out[0][1], out[0][2]) and np.array_equal(out[2][1], out[2][2])   # host chunks == the whole-column call, under either policy
