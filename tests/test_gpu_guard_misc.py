"""Guard-band tests of the small device entry points (INTEGRATION.md "What a call touches"; tests/guard_bands.py): mdsp_tdfir_exec / _exec_t,
mdsp_tdfir_state_exec, mdsp_hilbert, mdsp_extrapolate, mdsp_firarb_exec, mdsp_channel_sum, mdsp_frames and mdsp_ols_segment through the C ABI with
pointers INTO larger allocations: three columns, ldx = n + 5 and ldy = nout + 7 (both odd), once on a 128-byte line and once with the input shifted by 3
elements and the output by 1, a quiet-NaN poison in front of, between and behind the input columns, another NaN pattern all over the output buffer, guards
of 4096 elements.  Per call: nothing outside the outputs changed, every output written and none NaN (so the samples in front of every column read as
zeros, not as the poison that sits there); the bar of the function's existing test against the Float64 oracle; every column bit-identical to the same
column run compactly (one column, ld = n, straight from the allocator; the stateful filter with a compact (nb - 1, 1) state from the same initial state).
Exceptions, each said where it is tested: frames and overlap-save segments are bit-exact against the oracle itself; the polyphase FIR compares the shifted
placement with the aligned one, both guarded, since a single-channel filter need not take the same kernel path.

Bars: time-domain FIR and hilbert TOL32 (tests/test_gpu_parity.py) / 1e-12 (tests/test_gpu_boundary.py, test_hilbert); the arbitrary-rate resampler 3e-6 /
1e-12 (test_firarbitrary_vs_oracle_and_streaming_state); frames and overlap-save segments bit-exact (test_frames_bit_exact, test_ols_segmenter_bit_exact).
mdsp_extrapolate and mdsp_channel_sum have no test of their own to take a bar from; theirs follow from the number formats: 2 x[0] - x[k] is one rounding
of an exact doubling (bit-exact against the same expression in numpy), and a sum of nch positive terms is within (nch - 1) u of the exact one, u = 2^-24 / 2^-53.

The polyphase FIR (input side only: tests/test_gpu_polyphase_paths.py covers the output tail) takes one row of tests/fir_cases.py per kernel path 0 .. 3
with that file's extended-precision reference and bound; mdsp_periodogram2_exec (input side only) the shape and bounds of
tests/test_gpu_periodogram2.py::test_output_stride_keeps_the_tail.

Measured on MI355X, worst norm-wise error against the bar: tdfir 2.0e-7 (Float32), 2.9e-7 (ComplexF32) / 5e-6 and 2.4e-16, 5.6e-16 / 1e-12; stateful tdfir
2.1e-7 (state 1.8e-7) / 5e-6 and 2.3e-16 (state 2.2e-16) / 1e-12, real and complex signals; hilbert 1.9e-7 / 5e-6 and 6.2e-16 / 1e-12; arbitrary-rate resampler 1.4e-7 / 3e-6 and 3.0e-16 / 1e-12;
polyphase paths 0 .. 3: 3.8, 3.7, 1.0 and 1.5 u absdot against bounds of 34, 76, 4 and 10002 u absdot.  Bit-identical to the compact run wherever that is compared (see above)."""
import ctypes as C

import numpy as np
import pytest

import guard_bands as gb
import guard_cases as gc
from conftest import relerr
from test_gpu_parity import TOL32, TOL64

pytestmark = pytest.mark.gpu

NCOLS, PAD_X, PAD_Y = 3, 5, 7
SHIFTS = ((0, 0), (3, 1))
GUARD = gb.MIN_GUARD
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
CODE = {np.dtype(v): k for k, v in gc.NP_DTYPE.items()}


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _rand(rng, shape, dt):
    dt = np.dtype(dt)
    x = rng.standard_normal(shape)
    if dt.kind == "c":
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dt)


def _real(dt):
    return np.dtype(dt).type(0).real.dtype


def _tol(dt):
    return TOL32 if _real(dt) == np.float32 else TOL64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1)])


def _same(a, b, what):
    same = _bits(a) == _bits(b)
    assert same.all(), (what, "first word that differs from the compact run", int(np.flatnonzero(~same.ravel())[0]))


def _stream():
    from dsp_jl_amd import _dev
    return _dev.stream_ptr()


def _guarded(fn, x, nout, odt, sx, sy, what, n_written=None):
    """x (ncols, n) through fn(x_ptr, n, ncols, ldx, y_ptr, ldy) between guards -> (ncols, nout) outputs after check_output."""
    ncols, n = x.shape
    lx = gb.layout(n, ncols, n + PAD_X, GUARD, GUARD, sx, x.dtype)
    ly = gb.layout(nout, ncols, nout + PAD_Y, GUARD, GUARD, sy, odt)
    xd, yd = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(ly))
    fn(gb.ptr(xd, lx), n, ncols, lx.ld, gb.ptr(yd, ly), ly.ld)
    after = gb.from_device(yd)
    gb.check_output(after, ly, nout if n_written is None else n_written(), what)
    return gb.columns(after, ly)


def _compact(fn, xcol, nout, odt):
    import torch
    from dsp_jl_amd import _dev
    xd = torch.from_numpy(np.ascontiguousarray(xcol)).cuda()
    yd = torch.empty(max(nout, 1), dtype=_dev.torch_dtype(np.dtype(odt)), device="cuda")
    fn(xd.data_ptr(), len(xcol), 1, len(xcol), yd.data_ptr(), max(nout, 1))
    torch.cuda.synchronize()
    return yd[:nout].cpu().numpy()


def _all_placements(fn, x, nout, odt, what, refs, tol, worst):
    alone = [_compact(fn, x[c], nout, odt) for c in range(x.shape[0])]
    for sx, sy in SHIFTS:
        y = _guarded(fn, x, nout, odt, sx, sy, f"{what} shift ({sx}, {sy})")
        for c in range(x.shape[0]):
            if tol is None:
                assert np.array_equal(_bits(y[c]), _bits(refs[c])), (what, c, "differs from the oracle")
            else:
                e = relerr(y[c], refs[c])
                worst[0] = max(worst[0], e)
                assert e < tol, (what, sx, sy, c, e)
            _same(y[c], alone[c], (what, sx, sy, "column", c))


# ---- time-domain FIR -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("nb", [1, 66, 127])
def test_tdfir_reads_zeros_in_front_of_every_column(d, nb, dt):
    from dsp_jl_amd import _lib
    from oracle import dspbase as odsp
    lib = _lib.lib()
    dt = np.dtype(dt)
    rng = np.random.default_rng(nb * 4 + CODE[dt])
    b = (rng.standard_normal(nb) / np.sqrt(nb)).astype(_real(dt))
    wide = np.complex128 if dt.kind == "c" else np.float64
    worst = [0.0]
    for nx in sorted({1, max(nb - 1, 1), nb, 1000}):
        x = _rand(rng, (NCOLS, nx), dt)
        refs = [odsp.filt_ba(b.astype(np.float64), 1.0, x[c].astype(wide)) for c in range(NCOLS)]

        def fn(xp, n, ncols, ldx, yp, ldy):
            _lib.check(lib.mdsp_tdfir_exec(b.ctypes.data_as(C.c_void_p), nb, CODE[dt], xp, n, ncols, ldx, yp, ldy, _stream()))

        _all_placements(fn, x, nx, dt, f"tdfir {dt.name} nb {nb} nx {nx}", refs, _tol(dt), worst)
        if dt.kind == "c":                              # complex taps through the explicit-dtype entry point
            bc = _rand(rng, nb, dt) / np.sqrt(nb).astype(_real(dt))
            bc = bc.astype(dt)
            refs = [np.convolve(x[c].astype(wide), bc.astype(wide))[:nx] for c in range(NCOLS)]

            def fnt(xp, n, ncols, ldx, yp, ldy):
                _lib.check(lib.mdsp_tdfir_exec_t(bc.ctypes.data_as(C.c_void_p), nb, CODE[dt], CODE[dt], xp, n, ncols, ldx, yp, ldy, _stream()))

            _all_placements(fnt, x, nx, dt, f"tdfir_t {dt.name} nb {nb} nx {nx}", refs, _tol(dt), worst)
    print(f"MEASURED tdfir {dt.name} nb {nb} relerr {worst[0]:.2e} bar {_tol(dt):.0e}")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("nb", [2, 66, 127])
def test_tdfir_state_stays_inside_its_arrays(d, nb, dt):
    """The state (nb - 1, ncols) sits between guards too: read as the initial state, overwritten with the final one, nothing around it touched.  nb = 2 is the
    shortest filter that has a state.  Outputs and final state against the oracle's DF2TFilterFIR, and bit-identical to each column run alone on compact
    arrays (x, y and an (nb - 1, 1) state straight from the allocator) from the same initial state."""
    import torch
    from dsp_jl_amd import _lib
    from oracle import filt as ofilt
    lib = _lib.lib()
    dt = np.dtype(dt)
    wide = np.complex128 if dt.kind == "c" else np.float64
    rng = np.random.default_rng(nb * 8 + CODE[dt])
    b = (rng.standard_normal(nb) / np.sqrt(nb)).astype(_real(dt))             # real taps in the signal's precision, as mdsp_tdfir_exec takes them
    bp = b.ctypes.data_as(C.c_void_p)
    worst = [0.0, 0.0]
    for nx in sorted({1, nb - 1, nb, 1000}):
        x = _rand(rng, (NCOLS, nx), dt)
        si0 = _rand(rng, (NCOLS, nb - 1), dt)
        o = ofilt.DF2TFilterFIR(b.astype(np.float64), wide, (NCOLS,))
        o.state[...] = si0.T
        ref = o.filt(x.T.astype(wide)).T
        alone = []
        for c in range(NCOLS):
            sc = torch.from_numpy(np.ascontiguousarray(si0[c])).cuda()

            def fn1(xp, n, ncols, ldx, yp, ldy):
                _lib.check(lib.mdsp_tdfir_state_exec(bp, nb, CODE[dt], xp, n, ncols, ldx, yp, ldy, sc.data_ptr(), _stream()))

            yc = _compact(fn1, x[c], nx, dt)
            alone.append((yc, sc.cpu().numpy()))
        for sx, sy in SHIFTS:
            what = f"tdfir_state {dt.name} nb {nb} nx {nx} shift ({sx}, {sy})"
            lsi = gb.layout(nb - 1, NCOLS, nb - 1, GUARD, GUARD, sy, dt)        # compact by the ABI: no leading dimension of its own
            sbuf = gb.new_output(lsi)
            for c in range(NCOLS):
                sbuf.view(dt)[lsi.starts[c]:lsi.starts[c] + nb - 1] = si0[c]
            sd = gb.to_device(sbuf)

            def fn(xp, n, ncols, ldx, yp, ldy):
                _lib.check(lib.mdsp_tdfir_state_exec(bp, nb, CODE[dt], xp, n, ncols, ldx, yp, ldy, gb.ptr(sd, lsi), _stream()))

            y = _guarded(fn, x, nx, dt, sx, sy, what)
            safter = gb.from_device(sd)
            gb.check_output(safter, lsi, nb - 1, what + " state")
            state = gb.columns(safter, lsi)
            e, es = relerr(y, ref), relerr(state, o.state.T)
            worst[0], worst[1] = max(worst[0], e), max(worst[1], es)
            assert e < _tol(dt) and es < _tol(dt), (what, e, es)
            for c in range(NCOLS):
                _same(y[c], alone[c][0], (what, "column", c))
                _same(state[c], alone[c][1], (what, "state of column", c))
    print(f"MEASURED tdfir_state {dt.name} nb {nb} relerr {worst[0]:.2e} state {worst[1]:.2e} bar {_tol(dt):.0e}")


# ---- hilbert, extrapolate ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n", [2, 255, 256, 1001])
def test_hilbert_stays_inside_its_arrays(d, n, dt):
    from dsp_jl_amd import _lib
    from oracle import util as ou
    lib = _lib.lib()
    dt = np.dtype(dt)
    odt = np.dtype(np.complex64 if dt == np.float32 else np.complex128)
    x = _rand(np.random.default_rng(n), (NCOLS, n), dt)
    refs = [ou.hilbert(x[c].astype(np.float64)) for c in range(NCOLS)]
    worst = [0.0]

    def fn(xp, nn, ncols, ldx, yp, ldy):
        _lib.check(lib.mdsp_hilbert(xp, nn, ncols, ldx, CODE[dt], yp, ldy, _stream()))

    _all_placements(fn, x, n, odt, f"hilbert {dt.name} n {n}", refs, _tol(dt), worst)
    print(f"MEASURED hilbert {dt.name} n {n} relerr {worst[0]:.2e} bar {_tol(dt):.0e}")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda t: np.dtype(t).name)
def test_extrapolate_stays_inside_its_arrays(d, dt):
    from dsp_jl_amd import _lib
    from oracle import filt as ofilt
    lib = _lib.lib()
    dt = np.dtype(dt)
    n = 301
    x = _rand(np.random.default_rng(7), (NCOLS, n), dt)
    for pad in (0, 1, n - 1):
        refs = [ofilt.extrapolate_signal(x[c], pad).astype(dt) for c in range(NCOLS)]

        def fn(xp, nn, ncols, ldx, yp, ldy):
            _lib.check(lib.mdsp_extrapolate(xp, nn, ncols, ldx, CODE[dt], pad, yp, ldy, _stream()))

        _all_placements(fn, x, n + 2 * pad, dt, f"extrapolate {dt.name} pad {pad}", refs, None, None)


# ---- arbitrary-rate resampler --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("rate", [1.1, 0.7364])
def test_firarb_writes_nothing_beyond_nwritten(d, rate, dt):
    from dsp_jl_amd import _lib
    from oracle import design as odes, stream_filt as osf
    lib = _lib.lib()
    dt = np.dtype(dt)
    nphi, xlen = 32, 3001
    rng = np.random.default_rng(int(rate * 1000) + CODE[dt])
    h = odes.resample_filter(float(rate), nphi).astype(_real(dt))
    x = _rand(rng, (NCOLS, xlen), dt)
    wide = np.complex128 if dt.kind == "c" else np.float64
    o64 = osf.FIRFilter(h, rate, nphi)                  # as test_firarbitrary_vs_oracle_and_streaming_state: only the dot products in Float64
    o64.h, o64.pfb, o64.dpfb = h.astype(np.float64), o64.pfb.astype(np.float64), o64.dpfb.astype(np.float64)
    ol_ref = o64.outputlength(xlen)                     # from the fresh state
    refs = []
    for c in range(NCOLS):
        o64.reset()
        refs.append(o64.filt(x[c].astype(wide)))
    tol = 3e-6 if _real(dt) == np.float32 else 1e-12
    written, worst = [], [0.0]

    def make(nch):
        f = C.c_void_p()
        _lib.check(lib.mdsp_firarb_create(C.byref(f), h.ctypes.data_as(C.c_void_p), len(h), float(rate), nphi, CODE[np.dtype(_real(dt))], CODE[dt], nch))
        ol = C.c_int64()
        _lib.check(lib.mdsp_firarb_outputlength(f, xlen, C.byref(ol)))
        return f, ol.value + 1                            # outputlength + 1 holds every sample the loop writes (allocate_output, stream_filt.jl:639-655)

    def run(nch):
        def fn(xp, n, ncols, ldx, yp, ldy):
            f, ycap = make(nch)
            nw = C.c_int64(-1)
            try:
                _lib.check(lib.mdsp_firarb_exec(f, xp, n, ldx, yp, ycap, ldy, C.byref(nw), _stream()))
            finally:
                _lib.check(lib.mdsp_firarb_destroy(f))
            written.append(nw.value)
        return fn

    f0, ycap = make(NCOLS)
    _lib.check(lib.mdsp_firarb_destroy(f0))
    assert ycap - 1 == ol_ref                           # the library's outputlength is the reference's formula
    nout = len(refs[0])                                 # samplesWritten: one trajectory for all channels, and never more than the capacity above
    assert all(len(r) == nout for r in refs) and nout <= ycap, ([len(r) for r in refs], ycap)
    alone = [_compact(run(1), x[c], ycap, dt)[:nout] for c in range(NCOLS)]
    for sx, sy in SHIFTS:
        what = f"firarb {dt.name} rate {rate} shift ({sx}, {sy})"
        lx = gb.layout(xlen, NCOLS, xlen + PAD_X, GUARD, GUARD, sx, dt)
        ly = gb.layout(ycap, NCOLS, ycap + 3, GUARD, GUARD, sy, dt)
        xd, yd = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(ly))
        run(NCOLS)(gb.ptr(xd, lx), xlen, NCOLS, lx.ld, gb.ptr(yd, ly), ly.ld)
        assert written[-1] == nout, (what, written[-1], nout)            # samplesWritten is bit-exact
        after = gb.from_device(yd)
        gb.check_output(after, ly, nout, what)                           # nothing beyond nwritten in any column
        y = gb.columns(after, ly, nout)
        for c in range(NCOLS):
            e = relerr(y[c], refs[c])
            worst[0] = max(worst[0], e)
            assert e < tol, (what, c, e)
            _same(y[c], alone[c], (what, "column", c))
    print(f"MEASURED firarb {dt.name} rate {rate} relerr {worst[0]:.2e} bar {tol:.0e}")


# ---- channel sum, frames, overlap-save segments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_channel_sum_reads_only_its_rows(d, dt):
    import torch
    from dsp_jl_amd import _lib, _dev
    lib = _lib.lib()
    dt = np.dtype(dt)
    u = 2.0 ** -24 if dt == np.float32 else 2.0 ** -53
    for nout, nch in ((1, 3), (129, 3), (2049, 5)):
        p = np.abs(_rand(np.random.default_rng(nout), (nch, nout), dt)) + dt.type(0.5)       # positive, like the PSDs it sums
        ref = p.astype(np.float64).sum(axis=0)
        one = torch.empty(nout, dtype=_dev.torch_dtype(dt), device="cuda")
        pc = torch.from_numpy(p).cuda()
        _lib.check(lib.mdsp_channel_sum(pc.data_ptr(), nout, nch, nout, CODE[dt], one.data_ptr(), _stream()))
        torch.cuda.synchronize()
        for sx, sy in SHIFTS:
            what = f"channel_sum {dt.name} nout {nout} nch {nch} shift ({sx}, {sy})"
            lp = gb.layout(nout, nch, nout + PAD_X, GUARD, GUARD, sx, dt)                       # poison in the padding of the input rows
            ls = gb.layout(nout, 1, nout + PAD_Y, GUARD, GUARD, sy, dt)
            pd, sd = gb.to_device(gb.new_input(lp, p)), gb.to_device(gb.new_output(ls))
            _lib.check(lib.mdsp_channel_sum(gb.ptr(pd, lp), nout, nch, lp.ld, CODE[dt], gb.ptr(sd, ls), _stream()))
            after = gb.from_device(sd)
            gb.check_output(after, ls, nout, what)
            got = gb.columns(after, ls)[0]
            assert np.all(np.abs(got.astype(np.float64) - ref) <= (nch - 1) * u * ref), what
            _same(got, one.cpu().numpy(), what)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda t: np.dtype(t).name)
def test_frames_stay_inside_their_arrays(d, dt):
    from dsp_jl_amd import _lib
    from oracle import periodograms as opg, windows as ow
    lib = _lib.lib()
    dt = np.dtype(dt)
    length = 2000
    s = _rand(np.random.default_rng(31), (1, length), dt)
    for n, nov, nfft, win in ((256, 128, 256, ow.hanning(256)), (100, 10, 128, None), (7, 6, 7, ow.bartlett(7))):
        ref = opg.arraysplit(s[0], n, nov, nfft, win)                                          # (K, nfft)
        K = ref.shape[0]
        wp = None if win is None else np.ascontiguousarray(win, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        for sx, sy in SHIFTS:
            what = f"frames {dt.name} n {n} nfft {nfft} shift ({sx}, {sy})"
            lx = gb.layout(length, 1, length, GUARD, GUARD, sx, dt)
            lf = gb.layout(nfft, K, nfft, GUARD, GUARD, sy, dt)                                # (nfft, count): compact by the ABI
            xd, fd = gb.to_device(gb.new_input(lx, s)), gb.to_device(gb.new_output(lf))
            _lib.check(lib.mdsp_frames(gb.ptr(xd, lx), length, CODE[dt], n, nov, nfft, wp, 0, K, gb.ptr(fd, lf), _stream()))
            after = gb.from_device(fd)
            gb.check_output(after, lf, nfft, what)
            assert np.array_equal(gb.columns(after, lf), ref.astype(dt)), what


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_ols_segments_stay_inside_their_arrays(d, dt):
    from dsp_jl_amd import _lib
    from dsp_jl_amd.dspbase import OlsPlan
    from oracle import filt as ofilt
    lib = _lib.lib()
    dt = np.dtype(dt)
    rng = np.random.default_rng(3)
    for nb, nx, nfft in ((127, 5000, 1024), (200, 700, 256)):
        x = _rand(rng, (1, nx), dt)
        plan = OlsPlan(rng.standard_normal(nb).astype(dt), nfft, nx, 0, gc.FUSED)
        L, rows = ofilt.fftfilt_block_table(nb, nx, nfft)
        for sx, sy in SHIFTS:
            what = f"ols_segment {dt.name} nb {nb} nx {nx} shift ({sx}, {sy})"
            lx = gb.layout(nx, 1, nx, GUARD, GUARD, sx, dt)
            lg = gb.layout(nfft, len(rows), nfft, GUARD, GUARD, sy, dt)
            xd, gd = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(lg))
            _lib.check(lib.mdsp_ols_segment(plan._h, gb.ptr(xd, lx), nx, 0, len(rows), gb.ptr(gd, lg), _stream()))
            after = gb.from_device(gd)
            gb.check_output(after, lg, nfft, what)
            seg = gb.columns(after, lg)
            for ib, (off, npad, xstart, n, nout) in enumerate(rows):
                ref = np.zeros(nfft, dtype=dt)
                ref[npad:npad + n] = x[0, xstart - 1:xstart - 1 + n]
                assert np.array_equal(seg[ib], ref), (what, ib)


# ---- polyphase FIR and the 2-D periodogram: the input side ---------------------------------------------------------------------------------------------
def _fir_rows():
    """One row of tests/fir_cases.py per kernel path 0 .. 3: the first without knobs (Float32 taps where the table has one)."""
    from fir_cases import CASES
    rows = {}
    for row in sorted(CASES, key=lambda r: (r[3] != "f32", r[4] != "f32")):
        if not row[5] and row[6] == "rand":
            rows.setdefault(row[7], row)
    assert sorted(rows) == [0, 1, 2, 3]
    return [rows[p] for p in range(4)]


@pytest.mark.parametrize("row", _fir_rows(), ids=lambda r: f"path{r[7]}-{r[0]}_{r[1]}_h{r[2]}_{r[3]}_{r[4]}")
def test_polyphase_fir_reads_only_its_channels(d, row):
    """The tail of mdsp_fir_exec's outputs is covered by tests/test_gpu_polyphase_paths.py; here the input sits between poisoned guards with ldx = xlen + 5
    and the output has a filled guard in FRONT of it as well.  One chunk from the zero state, the reference and bound of that file."""
    from dsp_jl_amd import _lib
    from polyphase_ref import accumulation_unit, excess, outputlength, polyphase_ref
    from test_gpu_polyphase_paths import BUDGET, stream_length
    lib = _lib.lib()
    L, M, hlen, td, xd, knobs, taps, expect = row
    xnp = np.dtype({"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}[xd])
    hnp = np.float32 if td == "f32" else np.float64
    dbl = td == "f64" or xd in ("f64", "c64")
    ynp = np.dtype((np.complex128 if dbl else np.complex64) if xnp.kind == "c" else (np.float64 if dbl else np.float32))
    rng = np.random.default_rng(L * 7919 + M * 104729 + hlen)
    h = (rng.standard_normal(hlen) / np.sqrt(max(1.0, hlen / L))).astype(hnp)
    tp = -(-hlen // L)
    n = stream_length(tp, L, M, NCOLS, xnp.kind == "c", BUDGET / 8)     # that file's rule (the kernel path depends on n), an eighth of its reference budget
    x = _rand(rng, (NCOLS, n), xnp)
    nout = outputlength(n, L, M, 1, 1)
    ref, ad, _ = polyphase_ref(h, L, M, x, 1, 1, None)
    u, umin = accumulation_unit(h.dtype, xnp)
    outs = []
    for sx, sy in SHIFTS:
        what = f"fir path {expect} {L}//{M} shift ({sx}, {sy})"
        fh, path, nw = C.c_void_p(), C.c_int(-1), C.c_int64(-1)
        _lib.check(lib.mdsp_fir_create(C.byref(fh), h.ctypes.data_as(C.c_void_p), hlen, L, M, CODE[np.dtype(hnp)], CODE[xnp], NCOLS))
        try:
            _lib.check(lib.mdsp_fir_kernel_path(fh, n, C.byref(path)))
            assert path.value == expect, f"kernel path {path.value}, the table says {expect}"
            lx = gb.layout(n, NCOLS, n + PAD_X, GUARD, GUARD, sx, xnp)
            ly = gb.layout(nout, NCOLS, nout + PAD_X, GUARD, GUARD, sy, ynp)
            xd_, yd = gb.to_device(gb.new_input(lx, x)), gb.to_device(gb.new_output(ly))
            _lib.check(lib.mdsp_fir_exec(fh, gb.ptr(xd_, lx), n, lx.ld, gb.ptr(yd, ly), nout, ly.ld, C.byref(nw), _stream()))
            after = gb.from_device(yd)
        finally:
            _lib.check(lib.mdsp_fir_destroy(fh))
        assert nw.value == nout
        gb.check_output(after, ly, nout, what)
        y = gb.columns(after, ly)
        worst, ratio = excess(y, ref, ad, tp, u, umin)
        assert worst <= 1.0, (what, worst)
        outs.append(y)
    # placement against placement, not against a compact single-channel filter: the kernel path is a property of the filter AND its channel count
    _same(outs[1], outs[0], "shifted against aligned")
    print(f"MEASURED fir path {expect} max|y-ref|/(u absdot) {ratio:.3f} bound/(u absdot) {2 * (tp + 1)}")


def test_periodogram2_reads_only_its_columns(d):
    """The output stride of mdsp_periodogram2_exec has tests/test_gpu_periodogram2.py::test_output_stride_keeps_the_tail; at that shape the INPUT columns
    lds = n1 + 5 apart with poison between them, in front and behind."""
    import torch
    from dsp_jl_amd import _lib
    from dsp_jl_amd.periodograms import _P2Plan
    from periodogram2_ref import periodogram2_ref
    from test_gpu_periodogram2 import check_bounds
    lib = _lib.lib()
    n1, n2, N1, N2, ldo = 30, 20, 36, 21, 41
    x = np.random.default_rng(30).standard_normal((n1, n2))
    plan = _P2Plan(n1, n2, N1, N2, 1.0, 0, np.float64, gc.AUTO)
    ref = periodogram2_ref(x, (N1, N2))
    s = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    out = torch.empty((N2, N1), dtype=torch.float64, device="cuda")
    _lib.check(lib.mdsp_periodogram2_exec(plan._h, s.data_ptr(), n1, out.data_ptr(), N1, _stream()))
    torch.cuda.synchronize()
    for sx, sy in SHIFTS:
        what = f"periodogram2 shift ({sx}, {sy})"
        lx = gb.layout(n1, n2, n1 + PAD_X, GUARD, GUARD, sx, np.float64)
        lo = gb.layout(N1, N2, ldo, GUARD, GUARD, sy, np.float64)
        xd, od = gb.to_device(gb.new_input(lx, x.T)), gb.to_device(gb.new_output(lo))
        _lib.check(lib.mdsp_periodogram2_exec(plan._h, gb.ptr(xd, lx), lx.ld, gb.ptr(od, lo), ldo, _stream()))
        after = gb.from_device(od)
        gb.check_output(after, lo, N1, what)
        got = gb.columns(after, lo)                              # (N2, N1)
        check_bounds(got.T.copy(), ref, N1, N2, np.float64)
        _same(got, out.cpu().numpy(), what)
