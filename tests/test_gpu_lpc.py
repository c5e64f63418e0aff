"""lpc / arburg on the device: the record equals the host emulation bit for bit over the whole table of tests/lpc_cases.py (four types, the lengths at which
the tiling takes another path, forced cuts, 65 segments), numpy and device input agree, lpc defaults to Burg (test/lpc.jl:21-23), the reference's statistical
test (test/lpc.jl:3-15) through both methods, the Levinson route as the composition it is, and x unchanged after every call."""
import numpy as np
import pytest

import lpc_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def d():
    import dsp_jl_amd as dd
    from dsp_jl_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("GPU tests need a HIP device")
    _lib.check(_lib.lib().mdsp_init(0))
    return dd


def _same_bits(u, v):
    u, v = np.asarray(u), np.asarray(v)
    return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_record_equals_the_emulation_bit_for_bit(d, dt):
    import torch
    dt = np.dtype(dt)
    plans = {}
    for fam, n, p, S in lc.table(dt):
        x = lc.references(fam, n, p, dt.name)[0]
        want = lc.emulate_record(x, p, S)
        if (n, S) not in plans:
            plans[(n, S)] = d.BurgPlan(dt, n, S)
            assert (plans[(n, S)].segments, plans[(n, S)].seglen, plans[(n, S)].tile, plans[(n, S)].workspace_bytes) == d.burg_geometry(dt, n, S)
        xd = torch.from_numpy(x.copy()).cuda()
        rec = torch.full((2 * p + 3,), float("nan"), dtype=xd.dtype, device="cuda")
        plans[(n, S)].exec(xd.data_ptr(), p, rec.data_ptr())
        got = rec.cpu().numpy()
        assert _same_bits(got[:2 * p + 2], want), (fam, n, p, S, got, want)
        assert np.isnan(got[2 * p + 2])                                   # nothing behind the record
        assert _same_bits(xd.cpu().numpy(), x), (fam, n, p, S, "x changed")


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_automatic_cut_and_repeat_calls(d, dt):
    """A length at which the automatic rule cuts (several segments of whole tiles), an order at which trailing segments shrink, twice through one plan."""
    import torch
    dt = np.dtype(dt)
    n = 40 * 16 * lc.tile_of(dt) + 77
    S, seglen, tile, _ = d.burg_geometry(dt, n)
    assert S > 1 and seglen % tile == 0
    x = lc.signal("ar3", n, dt, seed=5)
    xd = torch.from_numpy(x).cuda()
    for p in (4, 0, 9):
        want = lc.emulate(x, p)
        got = d.arburg(xd, p)
        assert all(_same_bits(u, v) for u, v in zip(got, want)), p
        assert all(_same_bits(u, v) for u, v in zip(d.arburg(xd, p), want)), p
    assert _same_bits(xd.cpu().numpy(), x)


def test_numpy_and_device_input_agree_and_lpc_defaults_to_burg(d):
    import torch
    rng = np.random.default_rng(20)
    v = rng.random(1000)                                                  # test/lpc.jl:21-23
    a, e = d.lpc(v, 20)
    b, f = d.lpc(v, 20, d.LPCBurg())
    assert _same_bits(a, b) and e == f and a.shape == (20,) and a.dtype == np.float64 and np.asarray(e).dtype == np.float64
    vd = torch.from_numpy(v).cuda()
    for method in (d.LPCBurg(), d.LPCLevinson()):
        got_np, got_dev = d.lpc(v, 20, method), d.lpc(vd, 20, method)
        assert _same_bits(got_np[0], got_dev[0]) and got_np[1] == got_dev[1], method
    full = d.arburg(v, 20)
    assert _same_bits(full[0][1:], a) and full[0][0] == 1 and full[1] == e and full[2].shape == (20,) and full[2][-1] == a[-1]
    assert all(_same_bits(u, w) for u, w in zip(full, lc.emulate(v, 20)))
    assert _same_bits(vd.cpu().numpy(), v)
    # the type rules: Float32 stays, integers go through Float64
    a32, e32 = d.lpc(v.astype(np.float32), 5)
    assert a32.dtype == np.float32 and np.asarray(e32).dtype == np.float32
    vi = (1000 * v).astype(np.int32)
    ai, ei = d.lpc(vi, 5)
    assert ai.dtype == np.float64 and all(_same_bits(u, w) for u, w in zip((ai, ei), d.lpc(vi.astype(np.float64), 5)))
    c, ec = d.lpc(torch.from_numpy(vi).cuda(), 5)
    assert _same_bits(c, ai) and ec == ei


@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_reference_statistical_test_on_the_device(d, cplx):
    """test/lpc.jl:3-15 with the seeded input of tests/test_lpc_cpu.py, both methods."""
    import torch
    x, coeffs, var = lc.stat_cached(cplx)
    xd = torch.from_numpy(x.copy()).cuda()
    for method in (d.LPCBurg(), d.LPCLevinson()):
        ar, e = d.lpc(xd, len(coeffs) - 1, method)
        worst = float(np.max(np.abs(ar - coeffs[1:])))
        print(f"{type(method).__name__}: |ar - coeffs| {worst:.4f}, e {float(e):.5f} against var(s) {var:.5f}")
        assert ar.dtype == x.dtype and worst < 0.01
        assert abs(float(e) - var) <= 0.01 * max(abs(float(e)), var)
    assert _same_bits(xd.cpu().numpy(), x)


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_levinson_route_is_xcorr_then_levinson(d, dt):
    import torch
    dt = np.dtype(dt)
    x = lc.signal("ar3", 777, dt, seed=9)
    n = len(x)
    xd = torch.from_numpy(x.copy()).cuda()
    for p in (1, 3, 12):
        a, e = d.lpc(xd, p, d.LPCLevinson())
        want = d.levinson(d.xcorr(xd, scaling="biased")[n - 1:n + p], p)
        assert _same_bits(a, want[0]) and _same_bits(e, want[1]) and a.dtype == dt, p
        from_numpy = d.lpc(x, p, d.LPCLevinson())                         # a numpy signal goes to the device first
        assert _same_bits(from_numpy[0], a) and _same_bits(from_numpy[1], e), p
        assert _same_bits(xd.cpu().numpy(), x), (p, "x changed")


def test_argument_errors(d):
    import torch
    x = torch.ones(8, dtype=torch.float64, device="cuda")
    for fn in (d.arburg, d.lpc, lambda v, p: d.lpc(v, p, d.LPCLevinson())):
        with pytest.raises(TypeError):
            fn(torch.ones(4, 4, device="cuda"), 2)
        with pytest.raises(d.ArgumentError):
            fn(x, 8)
        with pytest.raises(d.ArgumentError):
            fn(x, -1)
        with pytest.raises(d.UnsupportedError):
            fn(torch.ones(8, dtype=torch.float16, device="cuda"), 2)
    plan = d.BurgPlan(np.float64, 8)
    rec = torch.zeros(32, dtype=torch.float64, device="cuda")
    for args in ((0, 2, rec.data_ptr()), (x.data_ptr(), 2, 0), (x.data_ptr(), 8, rec.data_ptr()), (x.data_ptr(), -1, rec.data_ptr()),
                 (x.data_ptr() + 4, 2, rec.data_ptr()), (x.data_ptr(), 2, rec.data_ptr() + 4)):
        with pytest.raises(d.ArgumentError):
            plan.exec(*args)
    a, e, k = d.arburg(torch.zeros(8, dtype=torch.float64, device="cuda"), 2)          # a zero signal: NaN as in the reference
    assert np.isnan(k).all() and np.isnan(e)
    assert d.levinson(torch.tensor([4.0, 2.0, 1.0, 7.0], device="cuda"), 2)[0].dtype == np.float32
    torch.cuda.synchronize()
