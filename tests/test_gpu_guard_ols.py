"""Guard-band tests of mdsp_ols_exec and mdsp_ols_exec_range (INTEGRATION.md "What a call touches"; tests/guard_bands.py): every overlap-save kernel form
of tests/guard_cases.py called through the C ABI with pointers INTO larger allocations -- columns ldx = nx + 5 and ldy = nout + 7 apart (both odd: columns
1 and 2 sit off cache lines), once on a 128-byte line and once with x shifted by 3 elements and y by 1, a quiet-NaN poison in front of, between and behind
the input columns, another NaN pattern all over the output buffer, guards of max(4096, exec_nfft) elements on both sides.  Per case:

  1. nothing outside [0, nout) of any output column changed and every output was written, none NaN (one sample read outside a column would poison a
     whole transform block);
  2. every column meets the bar the suite holds that form to (TOL32 of tests/test_gpu_boundary.py / 1e-12 norm-wise against the Float64 oracle, 5 x at
     the first and last 3000 outputs): np.convolve in Float64, the Float64 transform-domain product for 20001 taps and more;
  3. every column equals, bit for bit, the same column run compactly (one column, ldx = nx, ldy = nout, straight from the allocator, same plan): there
     are no atomics, so placement must not change the arithmetic.  The rocFFT engine is held to this too: its kernels are chosen per plan, not per call.

Lengths (L: the executed tile, == the block except on tiled plans): L // 2, L, L + 1, 2 L, 3 L + 3 (the rows forms L // 2, L + 1, 2 L + 17; the two
largest plans L // 2 and L + 1).  FILT plans: nout = nx and nout = nx - 1 - L // 2, which truncates inside a block (0 outputs at nx = L // 2: the call
must then write nothing); CONV plans: nout = nx + nb - 1 and nout = nx + 1.  Taps randn / sqrt(nb).

mdsp_ols_exec_range: the tiled plan and the 3-partition plan, ranges (0, 2), (2, 2) and a clipped last one, the slice inside a poisoned buffer, the outputs
inside a filled one; the assembled column against the oracle, each range bit-identical to the same call on compact arrays.

Measured on MI355X, worst over the cases of a family:

    form                                   norm-wise            first / last 3000     bar (norm-wise; 5 x at the edges)
    Float32 single block, tiled, untiled   1.6e-7 .. 1.8e-7     1.6e-7 .. 1.8e-7      5e-6
    Float32 re-blocked, 3 / 4 partitions   1.9e-7 .. 2.2e-7     2.1e-7 .. 2.6e-7      5e-6
    Float32 rows 64 / rows 256 / 3 passes  2.2e-7 .. 2.4e-7     8.0e-7 .. 1.6e-6      5e-6
    ComplexF32 single block / multi-pass   1.7e-7 / 2.5e-7      1.7e-7 / 7.6e-7       5e-6
    rocFFT engine (also 100 taps at 1000)  1.8e-7 .. 2.0e-7     the same              5e-6
    Float64, ComplexF64 (every form)       4.2e-16 .. 7.5e-16   up to 2.5e-15         1e-12
    block ranges (tiled, 3 partitions)     1.7e-7, 1.8e-7       1.8e-7, 2.1e-7        5e-6

Every column was bit-identical to its compact run in every form, the rocFFT engine at a shifted base included.  With the output descriptors of ols_store
sized by ldy instead of nout (a scratch build), this file fails at "column 0, element nout (outside the written range by 1); 21 such element(s)" -- 7
elements of padding in each of 3 columns -- while tests/test_gpu_ols_tile.py, whose arrays are compact, passes all 16 tests.

The table's "Float32 mixed-radix, 100 taps, nfft 1000" is no fused form: the fused overlap-save engine takes powers of two (fused_supported), and engine
AUTO runs that plan on the rocFFT engine at 1000 points; the case is kept as such."""
import numpy as np
import pytest

import guard_bands as gb
import guard_cases as gc
from conftest import relerr
from test_gpu_boundary import TOL32

pytestmark = pytest.mark.gpu

TOL64 = 1e-12                      # the Float64 bar of the overlap-save tests (tests/test_gpu_boundary.py)
PAD_X, PAD_Y = 5, 7
SHIFTS = ((0, 0), (3, 1))          # (x, y) base offsets in elements
FFT_REF_FROM = 20001               # taps from which the oracle is the Float64 transform-domain product (as the long-filter tests of the suite)


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


_DATA = {}


def _data(form):
    """Taps and columns of the longest signal of a form (shorter cases are prefixes), and a cache of Float64 full convolutions per (nx, column): computed
    once, shared by the FILT and the CONV test of the form."""
    if form.id not in _DATA:
        dt = np.dtype(gc.NP_DTYPE[form.dtype])
        rdt = np.float32 if dt.itemsize // (2 if dt.kind == "c" else 1) == 4 else np.float64
        rng = np.random.default_rng(form.nb * 31 + form.dtype)
        nmax = max(gc.ols_lengths(form))
        b = (rng.standard_normal(form.nb) / np.sqrt(form.nb)).astype(rdt)
        x = rng.standard_normal((form.ncols, nmax)).astype(rdt)
        if dt.kind == "c":
            b = (b + 1j * (rng.standard_normal(form.nb) / np.sqrt(form.nb))).astype(dt)
            x = (x + 1j * rng.standard_normal((form.ncols, nmax))).astype(dt)
        _DATA[form.id] = (b, x, {})
    return _DATA[form.id]


def _full_conv(form, nx, c):
    b, x, cache = _data(form)
    if (nx, c) not in cache:
        wide = np.complex128 if b.dtype.kind == "c" else np.float64
        xc, bw = x[c, :nx].astype(wide), b.astype(wide)
        if form.nb < FFT_REF_FROM:
            cache[(nx, c)] = np.convolve(xc, bw)
        else:
            nf = 1 << int(np.ceil(np.log2(nx + form.nb - 1)))
            if wide is np.float64:
                cache[(nx, c)] = np.fft.irfft(np.fft.rfft(xc, nf) * np.fft.rfft(bw, nf), nf)[:nx + form.nb - 1]
            else:
                cache[(nx, c)] = np.fft.ifft(np.fft.fft(xc, nf) * np.fft.fft(bw, nf))[:nx + form.nb - 1]
    return cache[(nx, c)]


def _plan(form, conv):
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    import ctypes as C
    b = _data(form)[0]
    with _Knobs(form.create):
        plan = OlsPlan(b, form.nfft, 0, _lib.OLS_CONV if conv else _lib.OLS_FILT, form.engine)
    en, el, ep, t, l = C.c_int64(), C.c_int64(), C.c_int(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_ols_plan_geometry(plan._h, C.byref(en), C.byref(el), C.byref(ep)))
    _lib.check(_lib.lib().mdsp_ols_plan_tile(plan._h, C.byref(t), C.byref(l)))
    assert (en.value, ep.value, plan.engine, t.value, l.value) == form.expect[:2] + form.expect[3:], form.id      # the form the table names
    return plan, el.value


def _oracle_check(y, ref, tol, what, worst):
    if len(ref) == 0:
        return
    e, e0, e1 = relerr(y, ref), relerr(y[:3000], ref[:3000]), relerr(y[-3000:], ref[-3000:])
    worst[0], worst[1] = max(worst[0], e), max(worst[1], e0, e1)
    assert e < tol, (what, e)
    assert e0 < 5 * tol and e1 < 5 * tol, (what, e0, e1)


def _compact(plan, xcol, nout):
    """One column straight from the allocator: ldx = nx, ldy = nout."""
    import torch
    from dsp_jl_amd import _lib, _dev
    xd = torch.from_numpy(np.ascontiguousarray(xcol)).cuda()
    yd = torch.empty(max(nout, 1), dtype=xd.dtype, device="cuda")
    _lib.check(_lib.lib().mdsp_ols_exec(plan._h, xd.data_ptr(), len(xcol), 1, len(xcol), yd.data_ptr(), nout, max(nout, 1), _dev.stream_ptr()))
    torch.cuda.synchronize()
    return yd[:nout].cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


@pytest.mark.parametrize("conv", [False, True], ids=["filt", "conv"])
@pytest.mark.parametrize("fid", [f.id for f in gc.OLS_FORMS])
def test_whole_column_call_stays_inside_its_columns(d, fid, conv):
    from dsp_jl_amd import _lib, _dev
    form = gc.OLS_BY_ID[fid]
    b, x, _ = _data(form)
    dt = x.dtype
    tol = TOL32 if _bits(x).dtype == np.uint32 else TOL64
    plan, _ = _plan(form, conv)
    guard = max(gb.MIN_GUARD, form.expect[0])
    worst = [0.0, 0.0]
    with _Knobs(form.launch):
        for nx in gc.ols_lengths(form):
            for nout in gc.ols_nouts(form, nx, conv):
                assert 0 <= nout <= nx + form.nb - 1
                refs = [_full_conv(form, nx, c)[:nout] for c in range(form.ncols)]
                alone = [_compact(plan, x[c, :nx], nout) for c in range(form.ncols)]
                for sx, sy in SHIFTS:
                    what = f"{fid} {'conv' if conv else 'filt'} nx {nx} nout {nout} shift ({sx}, {sy})"
                    lx = gb.layout(nx, form.ncols, nx + PAD_X, guard, guard, sx, dt)
                    ly = gb.layout(nout, form.ncols, nout + PAD_Y, guard, guard, sy, dt)
                    xd, yd = gb.to_device(gb.new_input(lx, x[:, :nx])), gb.to_device(gb.new_output(ly))
                    _lib.check(_lib.lib().mdsp_ols_exec(plan._h, gb.ptr(xd, lx), nx, form.ncols, lx.ld, gb.ptr(yd, ly), nout, ly.ld, _dev.stream_ptr()))
                    after = gb.from_device(yd)
                    gb.check_output(after, ly, nout, what)
                    y = gb.columns(after, ly)
                    for c in range(form.ncols):
                        _oracle_check(y[c], refs[c], tol, (what, c), worst)
                        same = _bits(y[c]) == _bits(alone[c])
                        assert same.all(), (what, "column", c, "first word that differs from the compact run", int(np.flatnonzero(~same)[0]))
    print(f"MEASURED ols {fid} {'conv' if conv else 'filt'} relerr {worst[0]:.2e} edges {worst[1]:.2e} bar {tol:.0e}")


@pytest.mark.parametrize("fid", gc.OLS_RANGE_FORMS)
def test_block_ranges_stay_inside_their_slices(d, fid):
    import torch
    from dsp_jl_amd import _lib, _dev
    form = gc.OLS_BY_ID[fid]
    b = _data(form)[0]
    plan, L = _plan(form, False)                       # L: the public block grid the ranges run on (1793 on the tiled plan)
    guard = max(gb.MIN_GUARD, form.expect[0])
    nx = 5 * L + 3
    rng = np.random.default_rng(form.nb + 5)
    x = rng.standard_normal((1, nx)).astype(b.dtype)
    dt = x.dtype
    ref = np.convolve(x[0].astype(np.float64), b.astype(np.float64))[:nx]
    nblocks = -(-nx // L)
    assert nblocks == 6
    ranges = ((0, 2), (2, 2), (4, 9))                  # the last one is clipped to the grid
    worst = [0.0, 0.0]
    with _Knobs(form.launch):
        for sx, sy in SHIFTS:
            got = np.full(nx, np.nan, dt)
            for g0, cnt in ranges:
                g1 = min(nblocks, g0 + cnt)
                lo, hi = max(0, g0 * L - (form.nb - 1)), min(nx, g1 * L)
                o0, o1 = g0 * L, min(nx, g1 * L)
                what = f"{fid} blocks [{g0}, {g1}) shift ({sx}, {sy})"
                lx = gb.layout(hi - lo, 1, hi - lo + PAD_X, guard, guard, sx, dt)
                ly = gb.layout(o1 - o0, 1, o1 - o0 + PAD_Y, guard, guard, sy, dt)
                xd, yd = gb.to_device(gb.new_input(lx, x[0, lo:hi])), gb.to_device(gb.new_output(ly))
                _lib.check(_lib.lib().mdsp_ols_exec_range(plan._h, gb.ptr(xd, lx), lo, hi - lo, nx, gb.ptr(yd, ly), g0, cnt, nx, _dev.stream_ptr()))
                after = gb.from_device(yd)
                gb.check_output(after, ly, o1 - o0, what)
                got[o0:o1] = gb.columns(after, ly)[0]
                xs = torch.from_numpy(np.ascontiguousarray(x[0, lo:hi])).cuda()          # the same range on compact arrays
                ys = torch.empty(o1 - o0, dtype=xs.dtype, device="cuda")
                _lib.check(_lib.lib().mdsp_ols_exec_range(plan._h, xs.data_ptr(), lo, hi - lo, nx, ys.data_ptr(), g0, cnt, nx, _dev.stream_ptr()))
                torch.cuda.synchronize()
                same = _bits(got[o0:o1]) == _bits(ys.cpu().numpy())
                assert same.all(), (what, "first word that differs from the compact run", int(np.flatnonzero(~same)[0]))
            _oracle_check(got, ref, TOL32, (fid, "ranges", sx, sy), worst)
    print(f"MEASURED ols-range {fid} relerr {worst[0]:.2e} edges {worst[1]:.2e} bar {TOL32:.0e}")
