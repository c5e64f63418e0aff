"""unwrap along one dimension on the device against the serial recurrence (tests/unwrap_ref.py unwrap_serial; src/unwrap.jl:25,34).  Equal means
bit for bit (signed zeros compare equal, NaN equals NaN); every input satisfies the exactness condition of tests/unwrap_cases.py by construction.  The
shapes are the smallest that reach each piece of code: line lengths around the 64-lane and tile boundaries of the contiguous route, forced cuts with a
ragged last segment on both routes, strided lines with different data in every lane, 10^5-sample ramps for large counts."""
import numpy as np
import pytest

import unwrap_cases as uc
import unwrap_ref as ur

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
_ids = dict(ids=lambda t: np.dtype(t).name)


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


_serial = {}


def serial(case):
    """unwrap_serial of a case, computed once and shared."""
    if case.name not in _serial:
        _serial[case.name] = ur.unwrap_serial(case.m, 1, case.range)
    return _serial[case.name]


def plan_for(d, m, range=None, segments=0):
    outer, n, inner = m.shape
    r = float(ur.default_range(m.dtype) if range is None else m.dtype.type(range))
    return d.UnwrapPlan(inner, n, outer, m.dtype, r, segments)


def run(d, case, segments=0, in_place=False, plan=None):
    """The case through mdsp_unwrap_exec -> (result, plan)."""
    import torch
    plan = plan or plan_for(d, case.m, case.range, segments)
    src = torch.from_numpy(case.m).cuda()
    dst = src if in_place else torch.full_like(src, 777.0)
    plan.exec(src.data_ptr(), dst.data_ptr())
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), case.m, equal_nan=True), (case.name, "input modified")
    return dst.cpu().numpy(), plan


def check(d, case, segments=0, in_place=False):
    got, plan = run(d, case, segments, in_place)
    assert ur.equal(got, serial(case)), (case.name, segments, in_place, plan.route, plan.segments, plan.seglen,
                                         "first difference at", np.argwhere(~((got == serial(case)) | (np.isnan(got) & np.isnan(serial(case)))))[:3].tolist())
    return plan


def boundaries(plan, n, itemsize):
    """Where the contiguous route changes hands in line 0 of a 16-byte-aligned array: segment starts (from the plan), and inside each segment the first
    sample of every 16-byte lane vector group of 64 (the tile) -- lane 63 | lane 0 of the next tile -- counted from the 16-byte boundary at or below the
    segment start."""
    V = 16 // itemsize
    pos = set()
    for s in range(plan.segments):
        j0 = s * plan.seglen
        pos.add(j0)
        pos.update(range(j0 - j0 % V, min(n, j0 + plan.seglen), 64 * V))
        pos.update(range(j0 - j0 % V + V, min(n, j0 + plan.seglen), 16 * V))        # and some lane | lane boundaries
    return sorted(p for p in pos if 0 < p < n)


# ---- contiguous route ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, **_ids)
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4 * 64 * 4 + 3, 10_007])
def test_contiguous_lines(d, n, dt):
    from dsp_jl_amd import _lib
    for outer in (1, 5):
        plan = check(d, uc.make(f"c_walk_{n}_{outer}_{np.dtype(dt).name}", uc.walk(n * 7 + outer, outer, n, 1, dt)))
        assert plan.route == _lib.UNWRAP_CONTIGUOUS
        if n == 10_007 and outer == 1:
            assert plan.segments == 2                         # the automatic cut of one line of this length (tests/test_unwrap_cpu.py)
        for seg in (0, 3):
            p = plan_for(d, np.zeros((outer, n, 1), dt), None, seg)
            where = boundaries(p, n, np.dtype(dt).itemsize)   # a period jump planted exactly across each of them
            check(d, uc.make(f"c_planted_{n}_{outer}_{seg}_{np.dtype(dt).name}", uc.planted(n + outer, outer, n, 1, dt, where)), seg)


# ---- strided route -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, **_ids)
@pytest.mark.parametrize("inner", [2, 3, 64, 65, 257])
def test_strided_lines_each_with_its_own_data(d, inner, dt):
    from dsp_jl_amd import _lib
    for n in (2, 17, 1000):
        for outer in (1, 3):
            plan = check(d, uc.make(f"s_walk_{inner}_{n}_{outer}_{np.dtype(dt).name}", uc.walk(inner * 1000 + n + outer, outer, n, inner, dt)))
            assert plan.route == _lib.UNWRAP_STRIDED


# ---- forced segmentation, in place and out of place ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, **_ids)
@pytest.mark.parametrize("inner", [1, 3], ids=["contiguous", "strided"])
def test_forced_segments_with_a_ragged_tail(d, inner, dt):
    for n in (7, 1000, 10_007):
        case = uc.make(f"f_walk_{inner}_{n}_{np.dtype(dt).name}", uc.walk(inner + n, 2, n, inner, dt))
        for seg in (2, 3, 7, n + 5):
            for in_place in (False, True):
                plan = check(d, case, seg, in_place)
                assert plan.segments == min(seg, n), (n, seg, plan.segments)          # honoured; clamped to len
                assert (plan.segments - 1) * plan.seglen < n <= plan.segments * plan.seglen
                if seg in (3, 7) and n > 7:
                    assert n % plan.seglen != 0                                       # the last segment is ragged
                assert plan.workspace_bytes == 2 * inner * plan.segments * 24


# ---- large counts --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, **_ids)
def test_ramps_of_1e5_samples(d, dt):
    n = 100_000
    m = np.concatenate([uc.ramp(11, n, dt, 2.0), uc.ramp(12, n, dt, -2.0)], axis=0)   # rising and falling, 2.0 +- 0.2 rad per step
    case = uc.make(f"ramps_{np.dtype(dt).name}", m)
    assert ur.max_count(m, 1) > 30_000
    check(d, case)
    check(d, case, 7, True)


@pytest.mark.parametrize("dt", DTYPES, **_ids)
@pytest.mark.parametrize("r", [10.0, 2.0, float(np.float32(2) * np.float32(np.pi))], ids=["range10", "range2", "range2pi32"])
def test_other_ranges_with_large_counts(d, r, dt):
    n = 100_000
    rng = np.random.default_rng(int(r * 100))
    step = (2.0 + rng.uniform(-0.2, 0.2, (2, n, 1))) * np.array([1.0, -1.0])[:, None, None] * (r / uc.TWO_PI)   # the ramps above, in units of this range
    case = uc.make(f"ranges_{r}_{np.dtype(dt).name}", uc.wrap(np.cumsum(step, axis=1), r).astype(dt), r)
    assert ur.max_count(case.m, 1, r) > 30_000
    check(d, case)


# ---- in place through the Python layer ------------------------------------------------------------------------------------------------------------------
def test_unwrap_in_place_returns_its_argument(d):
    import torch
    case = uc.make("inplace_api", uc.walk(3, 1, 1000, 1, np.float64))
    ref = serial(case).ravel()
    t = torch.from_numpy(case.m.ravel().copy()).cuda()
    ptr = t.data_ptr()
    assert d.unwrap_(t) is t and t.data_ptr() == ptr and ur.equal(t.cpu().numpy(), ref)
    a = case.m.ravel().copy()
    assert d.unwrap_(a) is a and ur.equal(a, ref)
    y = np.zeros_like(a)
    src = case.m.ravel().copy()
    assert d.unwrap_(y, src) is y and ur.equal(y, ref) and np.array_equal(src, case.m.ravel())      # unwrap!(y, m): m untouched
    ty = torch.zeros(1000, dtype=torch.float64, device="cuda")
    tm = torch.from_numpy(src).cuda()
    assert d.unwrap_(ty, tm) is ty and ur.equal(ty.cpu().numpy(), ref) and np.array_equal(tm.cpu().numpy(), src)


def test_partial_overlap_is_an_argument_error(d):
    import torch
    from dsp_jl_amd import _lib
    t = torch.zeros(200, dtype=torch.float32, device="cuda")
    plan = d.UnwrapPlan(1, 100, 1, np.float32, 1.0)
    assert _lib.lib().mdsp_unwrap_exec(plan._h, t.data_ptr(), t.data_ptr() + 4 * 50, None) == _lib.ERR_ARGUMENT
    assert _lib.lib().mdsp_unwrap_exec(plan._h, t.data_ptr() + 4 * 50, t.data_ptr(), None) == _lib.ERR_ARGUMENT
    assert _lib.lib().mdsp_unwrap_exec(plan._h, t.data_ptr(), t.data_ptr() + 4 * 100, None) == _lib.OK       # adjacent, not overlapping
    torch.cuda.synchronize()


# ---- non-finite samples --------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_samples_follow_the_recurrence(d):
    for case in uc.nonfinite_cases():
        n = case.m.shape[1]
        for seg in (0, 1, 3):
            got, plan = run(d, case, seg)
            assert ur.equal(got, serial(case)), (case.name, seg)
            got, _ = run(d, case, seg, in_place=True)
            assert ur.equal(got, serial(case)), (case.name, seg, "in place")
        if "line1" in case.name:                              # the second of three segments of line 1 of 3: the rest of THAT line is NaN
            assert plan.segments == 3 and plan.seglen == 10 and n == 30
            lines = got[:, :, 0] if case.m.shape[2] == 1 else got[0].T
            assert np.isfinite(lines[0]).all() and np.isfinite(lines[2]).all()
            assert np.isfinite(lines[1, :14]).all() and np.isnan(lines[1, 14:]).all()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [1, 3], ids=["contiguous", "strided"])
def test_bit_identical_exec_after_exec_and_cut_after_cut(d, inner):
    case = uc.make(f"det_{inner}", uc.walk(21, 1, 10_007, inner, np.float32))
    auto = plan_for(d, case.m)
    a, _ = run(d, case, plan=auto)
    b, _ = run(d, case, plan=auto)
    one, p1 = run(d, case, 1)
    many, p7 = run(d, case, 7)
    assert p1.segments == 1 and p7.segments == 7 and (inner != 1 or auto.segments == 2)
    for other in (b, one, many):
        assert np.array_equal(a.view(np.uint32), other.view(np.uint32))


# ---- containers and axes -------------------------------------------------------------------------------------------------------------------------------
def test_numpy_array_along_each_axis(d):
    for dt in DTYPES:
        m = uc.lattice(40, (40, 33, 5), dt)
        for axis in (0, 1, 2, -1):
            uc.require_exact(m, axis)
            got = d.unwrap(m, dims=axis)
            assert isinstance(got, np.ndarray) and ur.equal(got, ur.unwrap_serial(m, axis)), (np.dtype(dt).name, axis)
        m7 = np.asfortranarray(uc.lattice(41, (40, 33, 5), dt, period=7.0))          # any other memory order is made contiguous first
        uc.require_exact(m7, 0, 7.0)
        assert ur.equal(d.unwrap(m7, dims=0, range=7.0), ur.unwrap_serial(m7, 0, 7.0))


def test_device_tensor_in_device_tensor_out(d):
    import torch
    m = uc.lattice(8, (6, 50, 4), np.float32)
    t = torch.from_numpy(m).cuda()
    for axis in (0, 1, 2):
        uc.require_exact(m, axis)
        got = d.unwrap(t, dims=axis)
        assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == t.dtype and got.shape == t.shape
        assert ur.equal(got.cpu().numpy(), ur.unwrap_serial(m, axis))
    assert np.array_equal(t.cpu().numpy(), m)
    tt = t.permute(2, 1, 0)                                    # column-major view: no copy needed, same answer
    got = d.unwrap(tt, dims=1)
    assert got.shape == tt.shape and ur.equal(got.cpu().numpy(), ur.unwrap_serial(np.ascontiguousarray(m.transpose(2, 1, 0)), 1))


def test_phases_of_the_librarys_own_stft_across_frames(d):
    """unwrap(angle.(stft(x, 64, 48)); dims = frames): a complex tone whose phase advances by 2.0 rad per hop of 16 samples in every bin -- increments of
    2.0 or 2.0 - 2 pi, far from a tie (the condition is asserted on the phases the device produced)."""
    import torch
    hop, frames = 16, 60
    f = (2.0 + 2 * np.pi * 3) / (2 * np.pi * hop)              # cycles per sample, between bins 13 and 14 of 64
    x = np.exp(2j * np.pi * f * np.arange(64 + hop * (frames - 1))).astype(np.complex64)
    S = d.stft(torch.from_numpy(x).cuda(), 64, 48)             # (64, frames) device tensor, bins contiguous
    assert S.shape == (64, frames)
    ph = torch.angle(S)
    got = d.unwrap(ph, dims=1)
    assert isinstance(got, torch.Tensor) and got.device == ph.device
    phn = ph.cpu().numpy()
    uc.require_exact(phn, 1)
    ref = ur.unwrap_serial(phn, 1)
    assert ur.equal(got.cpu().numpy(), ref)
    assert np.all(np.abs(np.diff(ref, axis=1) - 2.0) < 0.05)   # ... and the unwrapped phase is the tone's: 2.0 rad per frame in every bin


def test_empty_arrays_give_empty_results(d):
    import torch
    for shape, axis in (((0,), 0), ((0, 4), 0), ((4, 0), 0), ((3, 0, 2), 2)):
        got = d.unwrap(np.zeros(shape, np.float32), dims=axis)
        assert isinstance(got, np.ndarray) and got.shape == shape and got.dtype == np.float32
        t = torch.zeros(shape, dtype=torch.float64, device="cuda")
        assert d.unwrap(t, dims=axis).shape == shape
    plan = d.UnwrapPlan(3, 0, 2, np.float32, 1.0)
    assert plan.segments == 1 and plan.workspace_bytes == 0
    from dsp_jl_amd import _lib
    assert _lib.lib().mdsp_unwrap_exec(plan._h, None, None, None) == _lib.OK            # no launch, no pointer needed
