"""rms, rmsfft, meanfreq, finddelay, shiftsignal and alignsignals on the device (dsp.jl_amd/util.py; mdsp_reduce_* and mdsp_shift_*).

The reductions are compared bit for bit with the host emulation of the device code (mdsp_reduce_emulate: same geometry, operators and order of additions),
ABSARGMAX with the numpy restatement of the reference's rule, the public calls with extended-precision references within bounds derived from the
arithmetic (stated at each test).  The shifts are compared bit for bit with numpy.  Arrays sit 0 - 3 elements off a 128-byte line."""
import numpy as np
import pytest

import util_cases as uc
import util_ref as ur

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 5e-6, 1e-12            # the project's FFT tolerances (tests/test_gpu_parity.py)
_op_ids = dict(ids=uc.op_id)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def offset_rows(x_flat, offsets=uc.OFFSETS, fill=0):
    """A host buffer of len(offsets) rows, each a whole number of 128-byte lines, row k holding x_flat from element offsets[k] on -> (buffer, row stride)."""
    per_line = 128 // x_flat.dtype.itemsize
    stride = -(-(x_flat.size + max(offsets) + 1) // per_line) * per_line
    buf = np.full(len(offsets) * stride, fill, x_flat.dtype)
    for k, off in enumerate(offsets):
        buf[k * stride + off:k * stride + off + x_flat.size] = x_flat
    return buf, stride


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run_reduce(d, x, op, dt, segments, step=0.0, centre=0, twice=False):
    """Every offset of uc.OFFSETS through one plan -> ([result per offset], plan)."""
    import torch
    from dsp_jl_amd import _lib
    outer, n, inner = x.shape
    buf, stride = offset_rows(x.reshape(-1))
    xd = torch.from_numpy(buf).cuda()
    assert xd.data_ptr() % 128 == 0
    words = uc.OUT_WORDS[op]
    out = torch.full((2, len(uc.OFFSETS), outer * inner * words), -7, dtype=torch.int64 if op == _lib.REDUCE_ABSARGMAX else torch.float64, device="cuda")
    plan = d.ReducePlan(inner, n, outer, op, dt, step=step, centre=centre, segments=segments)
    for rep in range(2 if twice else 1):
        for k, off in enumerate(uc.OFFSETS):
            plan.exec(xd.data_ptr() + (k * stride + off) * dt.itemsize, out[rep, k].data_ptr())
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if twice:
        assert np.array_equal(bits(res[0]), bits(res[1])), "two runs of one plan differ"
    shape = (outer, inner) if words == 1 else (outer, inner, words)
    return [res[0, k].reshape(shape) for k in range(len(uc.OFFSETS))], plan


@pytest.mark.parametrize("op_dt", uc.OPS, **_op_ids)
def test_reductions_equal_the_host_emulation_bit_for_bit(d, op_dt):
    """Every length, inner and outer size, forced cut and base offset: the device result equals mdsp_reduce_emulate bit for bit (the emulation is told the
    array's phase, the only thing of the address the order of additions depends on), two runs give the same bits, and ABSARGMAX equals the numpy rule on
    arrays with ties planted across every boundary."""
    from dsp_jl_amd import _lib
    op, dt = op_dt
    V = 16 // dt.itemsize
    for n in uc.LENS:
        centre = n // 2
        for inner in uc.INNERS:
            for outer in uc.OUTERS:
                where = set()
                for seg in uc.SEGMENTS:
                    _, S, seglen, _, _ = uc.geometry(inner, n, outer, op, dt, seg)
                    for ph in range(V if inner == 1 else 1):
                        where.update(uc.boundaries(n, S, seglen, dt.itemsize, ph))
                x = uc.reduce_input(op, dt, 1000 * n + 10 * inner + outer, outer, n, inner, centre, sorted(where))
                rule = ur.absargmax_lines(x, centre) if op == _lib.REDUCE_ABSARGMAX else None
                for seg in uc.SEGMENTS:
                    got, plan = run_reduce(d, x, op, dt, seg, uc.STEP, centre, twice=seg in (0, 3))
                    assert plan.route == (_lib.REDUCE_CONTIGUOUS if inner == 1 else _lib.REDUCE_STRIDED) and (seg == 0 or plan.segments <= seg)
                    want = {}
                    for k, off in enumerate(uc.OFFSETS):
                        ph = off % V if inner == 1 else 0
                        if ph not in want:
                            want[ph] = uc.emulate(x, op, uc.STEP, centre, seg, ph)[0]
                        what = (uc.op_id(op_dt), n, inner, outer, seg, off, plan.segments, plan.seglen)
                        assert np.array_equal(bits(got[k]), bits(want[ph])), what
                        if rule is not None:
                            assert np.array_equal(got[k], rule), what


@pytest.mark.parametrize("op_dt", [uc.OPS[0], uc.OPS[4], uc.OPS[6]], **_op_ids)
def test_one_long_line_crosses_many_segments(d, op_dt):
    """2^24 + 3 elements, the library's own cut (thousands of segments, then the finish), three elements off a line: bit for bit the emulation."""
    import torch
    from dsp_jl_amd import _lib
    op, dt = op_dt
    n, off, centre = uc.BIG, 3, uc.BIG // 3
    x = uc.gaussian(5, (1, n, 1), dt)
    if op == _lib.REDUCE_ABSARGMAX:
        x[0, [7, centre - 1000, centre + 1000, n - 2], 0] = [9.0, -9.0, 9.0, -9.0]        # equal distance on both sides: the smaller index
    buf = torch.zeros(n + 32, dtype=torch.from_numpy(x).dtype, device="cuda")
    buf[off:off + n] = torch.from_numpy(x.reshape(-1)).cuda()
    out = torch.full((2,), -7, dtype=torch.int64 if op == _lib.REDUCE_ABSARGMAX else torch.float64, device="cuda")
    plan = d.ReducePlan(1, n, 1, op, dt, step=uc.STEP, centre=centre)
    assert plan.segments > 1000
    plan.exec(buf.data_ptr() + off * dt.itemsize, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:uc.OUT_WORDS[op]]
    want = uc.emulate(x, op, uc.STEP, centre, 0, off % (16 // dt.itemsize))[0].reshape(-1)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    if op == _lib.REDUCE_ABSARGMAX:
        assert tuple(got) == (centre - 1000, 0)


def test_absargmax_nan_and_infinities(d):
    from dsp_jl_amd import _lib
    for dt in (uc.F32, uc.F64):
        x = uc.gaussian(3, (2, 300, 1), dt)
        x[0, [5, 100, 250], 0] = [np.inf, -np.inf, np.nan]
        x[1, [64, 65, 200], 0] = [-np.inf, np.nan, np.inf]
        for centre in (0, 60, 150, 299):
            rule = ur.absargmax_lines(x, centre)
            assert rule[:, 0, 1].tolist() == [1, 1]
            for seg in uc.SEGMENTS:
                for got in run_reduce(d, x, _lib.REDUCE_ABSARGMAX, dt, seg, centre=centre)[0]:
                    assert np.array_equal(got, rule), (dt, centre, seg)
        allnan = np.full((1, 70, 1), np.nan, dt)
        assert run_reduce(d, allnan, _lib.REDUCE_ABSARGMAX, dt, 2)[0][0].tolist() == [[[-1, 1]]]


# ---- the public calls against the extended-precision references --------------------------------------------------------------------------------------
def relerr(got, ref):
    got, ref = np.asarray(got).astype(ur.LD), np.asarray(ref)
    return float(np.max(np.abs(got - ref) / ref))


RMS_SHAPES = [(n,) for n in uc.LENS] + [(5, 257), (257, 3), (2, 65, 64), (3, 1023, 2), (65, 63)]


@pytest.mark.parametrize("dt", [uc.F32, uc.C32, uc.F64, uc.C64], ids=lambda t: t.name)
def test_rms_and_rmsfft_within_the_derived_bounds(d, dt):
    """Float32 / ComplexF32: the sum is accumulated in Float64 from exact products (error below 2^-40 at these depths) and rounded once to Float32:
    relative error <= 2^-23.  Float64 / ComplexF64: (depth + 3) 2^-52 with the plan's depth -- every addition and the roundings of the products, the
    division and the square root at 2^-53 each, halved by the square root; the bound has room to spare and was not fitted to the results."""
    import torch
    from dsp_jl_amd import _lib
    single = dt in (uc.F32, uc.C32)
    for shape in RMS_SHAPES:
        x = uc.gaussian(sum(shape), shape, dt)
        for axis in (None,) + tuple(range(len(shape))):
            if axis is None:
                inner, n, outer = 1, x.size, 1
            else:
                n, outer, inner = shape[axis], int(np.prod(shape[:axis])), int(np.prod(shape[axis + 1:]))
            bound = 2.0 ** -23 if single else (d.reduce_geometry(inner, n, outer, _lib.REDUCE_SUMABS2, dt)[3] + 3) * 2.0 ** -52
            ref = ur.rms(x, axis)
            got = d.rms(x, dims=axis)
            assert got.dtype == (np.float32 if single else np.float64) and np.shape(got) == np.shape(ref), (shape, axis)
            assert relerr(got, ref) <= bound, (dt, shape, axis, relerr(got, ref), bound)
            got_dev = d.rms(torch.from_numpy(x).cuda(), dims=axis)
            assert got_dev.is_cuda and tuple(got_dev.shape) == np.shape(ref) and np.array_equal(got_dev.cpu().numpy(), got), (shape, axis)
        if dt.kind == "c":
            bound = 2.0 ** -23 if single else (d.reduce_geometry(1, x.size, 1, _lib.REDUCE_SUMABS2, dt)[3] + 3) * 2.0 ** -52
            got = d.rmsfft(x)
            assert got.dtype == (np.float32 if single else np.float64) and relerr(got, ur.rmsfft(x)) <= bound, (shape, relerr(got, ur.rmsfft(x)), bound)


def test_rms_containers_types_and_empties(d):
    import torch
    x = uc.gaussian(1, (40, 6), np.float64)
    xd = torch.from_numpy(x).cuda()
    r = d.rms(xd)
    assert r.is_cuda and r.dim() == 0 and r.dtype == torch.float64 and relerr(r.item(), ur.rms(x)) < 1e-14
    view = xd.t()[:, ::2]                                              # non-contiguous: made contiguous first
    assert relerr(d.rms(view, dims=0).cpu().numpy(), ur.rms(x.T[:, ::2], 0)) < 1e-14
    col = xd.t()                                                       # column-major: handed over as it lies
    assert relerr(d.rms(col, dims=1).cpu().numpy(), ur.rms(x.T, 1)) < 1e-14 and relerr(d.rms(col, dims=-2).cpu().numpy(), ur.rms(x.T, 0)) < 1e-14
    ints = np.arange(-5, 20, dtype=np.int32)
    assert d.rms(ints).dtype == np.float64 and relerr(d.rms(ints), ur.rms(ints)) < 1e-15 and relerr(d.rms([3, 4]), ur.rms([3.0, 4.0])) < 1e-15
    assert np.isnan(d.rms(np.zeros(0, np.float32))) and d.rms(np.zeros(0, np.float32)).dtype == np.float32
    e = d.rms(torch.zeros((0, 3), device="cuda"), dims=0)
    assert e.is_cuda and tuple(e.shape) == (1, 3) and bool(torch.isnan(e).all())
    assert np.isnan(d.rmsfft(np.zeros(0, np.complex64)))
    f = np.fft.fft(x[:, 0])
    assert abs(d.rmsfft(f) - d.rms(x[:, 0])) < 1e-14                    # rmsfft(fft(s)) == rms(s)


@pytest.mark.parametrize("dt", [uc.F32, uc.F64], ids=lambda t: t.name)
def test_meanfreq_within_four_fft_tolerances(d, dt):
    """|meanfreq - reference| <= 4 TOL |reference|, TOL the project's FFT tolerance for the element type: squaring doubles the relative error of a bin,
    and the ratio takes it from two sums."""
    import torch
    tol = 4 * (TOL32 if dt == uc.F32 else TOL64)
    for n in (1, 2, 255, 256, 1000, 4099):
        x = (uc.gaussian(n, (n,), np.float64) + np.sin(0.3 * np.arange(n)) + 0.25).astype(dt)
        for fs in (2 * np.pi, 1000.0):
            ref = float(ur.meanfreq(x, fs))
            got = d.meanfreq(x, fs) if fs != 2 * np.pi else d.meanfreq(x)
            assert isinstance(got, np.float64) and abs(got - ref) <= tol * abs(ref), (dt, n, fs, got, ref)
        got_dev = d.meanfreq(torch.from_numpy(x).cuda())
        assert got_dev.is_cuda and got_dev.dim() == 0 and got_dev.dtype == torch.float64 and got_dev.item() == d.meanfreq(x)
    x32 = uc.gaussian(9, (256,), np.float32)
    assert isinstance(d.meanfreq(x32, np.float32(8000)), np.float32)     # Float32 signal and Float32 fs: Float32 (util.jl:216-218)
    assert abs(d.meanfreq(np.arange(1, 65)) - float(ur.meanfreq(np.arange(1, 65)))) < 1e-11   # integers go through Float64


@pytest.mark.parametrize("dt", [uc.F32, uc.F64], ids=lambda t: t.name)
@pytest.mark.parametrize("n,delay", [(257, 5), (4099, -37), (70001, 1234)])
def test_finddelay_finds_the_planted_delay_exactly(d, n, delay, dt):
    import torch
    x, y = uc.delayed_pair(n, delay, dt)
    got = d.finddelay(x, y)
    assert type(got) is int and got == delay
    assert d.finddelay(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) == delay and d.finddelay(y, x) == -delay


def test_finddelay_doctests_ties_and_nan(d):
    assert d.finddelay([0, 0, 1, 2, 3], [1, 2, 3]) == 2 and d.finddelay([1, 2, 3], [0, 0, 1, 2, 3]) == -2            # util.jl:329-333
    assert d.finddelay([0, 1, 0], [1, 0, 1]) == 1 and d.finddelay([1, 0, 1], [1]) == 0                               # the tie rules
    assert d.finddelay(np.array([0, 0, 1.0, 2, 3], np.float32), np.array([1.0, 2, 3])) == 2
    x, y = uc.delayed_pair(300, 4, np.float64)
    x[17] = np.nan
    with pytest.raises(d.ArgumentError):
        d.finddelay(x, y)


# ---- shiftsignal -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("esize", [4, 8, 16])
@pytest.mark.parametrize("tile", uc.TILES)
def test_shift_every_route_is_bit_exact(d, tile, esize):
    """The issue's (l, s) grid for a forced tile, every route forced and the library's own choice, 0 - 3 elements off a 128-byte line, in place and out of
    place: bit for bit numpy's result, and nothing next to the line changes."""
    import torch
    dt = np.dtype(uc.SHIFT_DTYPES[esize])
    word = {4: np.int32, 8: np.int64, 16: np.int64}[esize]
    for l, s in uc.shift_grid(tile):
        x = uc.gaussian(l + abs(s), (l,), dt)
        want = ur.shiftsignal(x, s)
        buf, stride = offset_rows(x, fill=55)                 # nonzero all around the lines: a stray zero shows
        expect_in = buf.copy()
        for k, off in enumerate(uc.OFFSETS):
            expect_in[k * stride + off:k * stride + off + l] = want
        for route in uc.ROUTES:
            for in_place in (True, False):
                if not uc.route_allowed(l, s, in_place, route):
                    continue
                plan = d.ShiftPlan(l, s, esize, in_place, tile, route)
                assert route == 0 or plan.route == route
                src = torch.from_numpy(buf).cuda()
                dst = src if in_place else torch.from_numpy(buf).cuda()
                for k, off in enumerate(uc.OFFSETS):
                    at = (k * stride + off) * esize
                    plan.exec(src.data_ptr() + at, dst.data_ptr() + at)
                torch.cuda.synchronize()
                what = (esize, tile, l, s, uc.ROUTE_NAME[route], uc.ROUTE_NAME[plan.route], in_place)
                assert np.array_equal(dst.cpu().numpy().view(word), expect_in.view(word)), what
                if not in_place:
                    assert np.array_equal(src.cpu().numpy().view(word), buf.view(word)), what + ("input modified",)


def test_shiftsignal_calls_and_containers(d):
    import torch
    from dsp_jl_amd import _lib
    assert d.shiftsignal(np.array([1, 2, 3]), 2).tolist() == [0, 0, 1] and d.shiftsignal(np.array([1, 2, 3]), -2).tolist() == [3, 0, 0]   # util.jl:380-391
    for dt in (np.float32, np.int32, np.float64, np.int64, np.complex64, np.complex128):
        x = (np.arange(1, 5001) * (1 + 1j if np.dtype(dt).kind == "c" else 1)).astype(dt)
        for s in (0, 1, -1, 17, -2499, 2500, 2501, -4999, 5000, -5000):
            want = ur.shiftsignal(x, s)
            got = d.shiftsignal(x, s)
            assert got.dtype == x.dtype and np.array_equal(got, want), (dt, s)
            xd = torch.from_numpy(x).cuda()
            yd = d.shiftsignal(xd, s)
            assert yd.is_cuda and yd.data_ptr() != xd.data_ptr() and np.array_equal(yd.cpu().numpy(), want) and np.array_equal(xd.cpu().numpy(), x), (dt, s)
            assert d.shiftsignal_(xd, s) is xd and np.array_equal(xd.cpu().numpy(), want), (dt, s)
            xh = x.copy()
            assert d.shiftsignal_(xh, s) is xh and np.array_equal(xh, want), (dt, s)
        for s in (5001, -5001):
            for fn in (d.shiftsignal, d.shiftsignal_):
                with pytest.raises(d.DomainError):
                    fn(torch.from_numpy(x).cuda(), s)
    # the library's own routes on a line long enough for all three (2^21 + 5 Float64: 64 tiles ... forced down to 4096-element tiles: 513 of them)
    n = 2 ** 21 + 5
    x = uc.gaussian(2, (n,), np.float64)
    for s, tile, route in ((100, 4096, _lib.SHIFT_HALO), (-4097, 4096, _lib.SHIFT_HALO), (100, 0, _lib.SHIFT_STAGED), (2 ** 20 + 3, 0, _lib.SHIFT_DISJOINT)):
        assert d.shift_geometry(n, s, 8, True, tile)[0] == route
        xd = torch.from_numpy(x).cuda()
        assert d.shiftsignal_(xd, s, tile=tile) is xd and np.array_equal(xd.cpu().numpy(), ur.shiftsignal(x, s)), (s, tile)
    # a non-contiguous view is shifted through a contiguous copy, and written back
    base = torch.from_numpy(x[:2000].copy()).cuda()
    view = base[::2]
    assert d.shiftsignal_(view, 3) is view and np.array_equal(view.cpu().numpy(), ur.shiftsignal(x[:2000:2], 3)) and np.array_equal(base.cpu().numpy()[1::2], x[1:2000:2])


def test_alignsignals(d):
    import torch
    a, dl = d.alignsignals(np.array([0, 0, 1, 2, 3]), np.array([1, 2, 3]))
    assert (a.tolist(), dl) == ([1, 2, 3, 0, 0], 2)                                                                 # util.jl:418-419
    a, dl = d.alignsignals(np.array([1, 2, 3]), np.array([0, 0, 1, 2, 3]))
    assert (a.tolist(), dl) == ([0, 0, 1], -2)                                                                      # util.jl:421-422
    x, y = uc.delayed_pair(4099, 37, np.float32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    out, dl = d.alignsignals(xd, yd)
    assert dl == 37 and out.is_cuda and out.data_ptr() != xd.data_ptr() and np.array_equal(out.cpu().numpy(), ur.shiftsignal(x, -37))
    same, dl = d.alignsignals_(xd, yd)
    assert same is xd and dl == 37 and np.array_equal(xd.cpu().numpy(), ur.shiftsignal(x, -37))
    xh = x.copy()
    same, dl = d.alignsignals_(xh, y)
    assert same is xh and dl == 37 and np.array_equal(xh, ur.shiftsignal(x, -37))
