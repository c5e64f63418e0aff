"""esprit on the device: the Gram matrix equals the host emulation bit for bit over the whole grid of tests/esprit_cases.py (four types, the M and n at
which the lag groups and the tiling take another path, forced cuts and the automatic one), numpy and device input agree and the caller's tensor is
unchanged, the public call is the host finish on those bits, stays inside the recorded route bound of the SVD restatement (estimation.jl:67-75) and passes
the reference's own test (test/estimation.jl:19-20); input forms and refusals."""
import numpy as np
import pytest

import esprit_cases as ec
import esprit_ref as ref

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


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_gram_matrix_equals_the_emulation_bit_for_bit(d, dt):
    import torch
    dt = np.dtype(dt)
    for n, M, S in ec.grid(dt):
        x = ec.references(n, M, dt.name)[0]
        want = ec.emulate(x, M, S)
        plan = d.GramPlan(dt, n, M, S)
        assert (plan.segments, plan.seglen, plan.tile, plan.lag_group, plan.workspace_bytes) == d.hankel_gram_geometry(dt, n, M, S)
        xd = torch.from_numpy(x.copy()).cuda()
        r = torch.full((M + 1, M), float("nan"), dtype=d._dev.torch_dtype(plan.out_dtype), device="cuda")
        plan.exec(xd.data_ptr(), r.data_ptr())
        got = r.cpu().numpy()
        assert _same_bits(got[:M].T.copy(), want), (n, M, S)
        assert np.isnan(got[M]).all()                                      # nothing behind the matrix
        assert _same_bits(xd.cpu().numpy(), x), (n, M, S, "x changed")


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_several_lag_groups_per_wavefront_and_repeat_calls(d, dt):
    """M large enough that a wavefront walks more than one lag group over a staged tile, a ragged last group, the automatic cut into several segments;
    twice through the cached plan."""
    import torch
    T, G = ec.tile_and_group()
    n, M = 9 * T + 11, 4 * 2 * G + 3
    assert d.hankel_gram_geometry(dt, n, M)[0] > 1
    x = ec.signal(n, dt, seed=7)
    want = ec.emulate(x, M)
    xd = torch.from_numpy(x.copy()).cuda()
    for _ in range(2):
        got = d.hankel_gram(xd, M)
        assert got.is_cuda and _same_bits(got.cpu().numpy().copy(), want)
    assert _same_bits(d.hankel_gram(x, M).copy(), want)
    assert _same_bits(xd.cpu().numpy(), x)


@pytest.mark.parametrize("dt", (np.float32, np.complex128), ids=lambda t: np.dtype(t).name)
def test_more_lags_than_one_workgroup_takes(d, dt):
    """M above LAG_BLOCK = 1024 (csrc/gram_op.h): a second workgroup per segment stages the tile shifted by 1024 lags.  esprit stops at ESPRIT_MAX_M; the
    plan does not."""
    import torch
    M, S = 1024 + 2 * ec.tile_and_group()[1] + 3, 2
    n = 2 * M - 1 + 70
    x = ec.signal(n, dt, seed=5)
    want = ec.emulate(x, M, S)
    plan = d.GramPlan(dt, n, M, S)
    assert plan.segments == 2
    xd = torch.from_numpy(x.copy()).cuda()
    r = torch.full((M, M), float("nan"), dtype=d._dev.torch_dtype(plan.out_dtype), device="cuda")
    plan.exec(xd.data_ptr(), r.data_ptr())
    assert _same_bits(r.cpu().numpy().T.copy(), want)
    assert _same_bits(xd.cpu().numpy(), x)


def test_numpy_and_device_input_give_the_same_bits(d):
    import torch
    for dt in ec.DTYPES:
        x = ec.signal(700, dt, seed=3)
        xd = torch.from_numpy(x.copy()).cuda()
        a, b = d.hankel_gram(x, 11), d.hankel_gram(xd, 11)
        assert isinstance(a, np.ndarray) and b.is_cuda and a.dtype == ec.out_dtype(dt) and a.shape == (11, 11)
        assert _same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b.cpu().numpy())) and _same_bits(np.ascontiguousarray(a), ec.emulate(x, 11))
        assert _same_bits(d.esprit(x, 11, 2, 50.0), d.esprit(xd, 11, 2, 50.0))
        assert _same_bits(xd.cpu().numpy(), x), "the caller's tensor changed"


def test_public_call_is_the_host_finish_on_the_emulated_bits(d):
    import torch
    for name, x, M, p, Fs, truth, f_svd, sv_ratio in ec.route_cases():
        xd = torch.from_numpy(x.copy()).cuda()
        got = d.esprit(xd, M, p, Fs)
        assert got.dtype == np.float64 and got.shape == (p,)
        assert _same_bits(got, ref.finish(ec.emulate(x, M), p, Fs)), name               # the same host code on the same bits
        e = float(np.max(np.abs(np.sort(got) - f_svd)) / Fs)
        print(f"{name}: |f_device - f_svd| / Fs {e:.3g} of {ec.ROUTE_BOUND:.3g}")
        assert sv_ratio >= ec.ROUTE_MIN_SV_RATIO and e <= ec.ROUTE_BOUND, (name, e)
        if truth is not None:                                                             # test/estimation.jl:19-20
            assert np.max(np.abs(np.sort(got) - np.array(truth))) <= 1e-2, (name, got)
        assert _same_bits(xd.cpu().numpy(), x), name


def test_input_forms(d):
    import torch
    x = ec.signal(300, np.complex128, seed=11)
    want = d.esprit(x, 20, 2, 8.0)
    assert _same_bits(d.esprit(x.reshape(-1, 1), 20, 2, 8.0), want) and _same_bits(d.esprit(x.reshape(1, -1), 20, 2, 8.0), want)
    assert _same_bits(d.esprit(torch.from_numpy(x.copy()).cuda().reshape(1, -1, 1), 20, 2, 8.0), want)
    assert _same_bits(d.esprit(x, 20, 2), d.esprit(x, 20, 2, 1.0))                       # Fs defaults to 1.0
    xi = np.round(100 * ec.signal(300, np.float64, seed=12)).astype(np.int32)            # integers go through Float64
    assert _same_bits(d.esprit(xi, 20, 4), d.esprit(xi.astype(np.float64), 20, 4))
    assert _same_bits(d.esprit(torch.from_numpy(xi).cuda(), 20, 4), d.esprit(xi.astype(np.float64), 20, 4))
    assert d.hankel_gram(xi, 3).dtype == np.float64


def test_refusals(d):
    import torch
    x = torch.ones(64, dtype=torch.float64, device="cuda")
    y = np.ones(64)
    y[40] = np.nan
    for bad in (y, torch.from_numpy(y).cuda(), np.where(np.isnan(y), np.inf, y)):
        with pytest.raises(d.ArgumentError):
            d.esprit(bad, 8, 2)
    for bad in ((x, 8, 0), (x, 65, 2), (x, 0, 1), (torch.ones(4, 4, device="cuda"), 2, 1)):
        with pytest.raises(d.ArgumentError):
            d.esprit(*bad)
    for bad in ((x, 8, 8), (x, 33, 2), (torch.ones(4000, device="cuda"), d.ESPRIT_MAX_M + 1, 2), (x.to(torch.float16), 8, 2)):
        with pytest.raises(d.UnsupportedError):
            d.esprit(*bad)
    plan = d.GramPlan(np.float64, 64, 8)
    r = torch.zeros(64, dtype=torch.float64, device="cuda")
    for args in ((0, r.data_ptr()), (x.data_ptr(), 0), (x.data_ptr(), r.data_ptr(), 7), (x.data_ptr() + 4, r.data_ptr()), (x.data_ptr(), r.data_ptr() + 4)):
        with pytest.raises(d.ArgumentError):
            plan.exec(*args)
    torch.cuda.synchronize()
