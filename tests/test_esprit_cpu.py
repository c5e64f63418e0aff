"""esprit without a device: the geometry of the Hankel Gram plan, the argument and unsupported errors of the C ABI and of the Python host, the structure
and the accuracy of the library's host emulation (the text the kernels compile, csrc/gram_op.h) against the long-double Gram matrix with the bound of
tests/esprit_cases.py, the agreement of the Gram route with the SVD restatement of estimation.jl:67-75, and the reference's own test."""
import ctypes as C

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _dev, _lib

import esprit_cases as ec
import esprit_ref as ref

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_geometry_equals_the_plan_info_and_cuts_the_body_range(dt):
    T, G = ec.tile_and_group()
    per = 16 if np.dtype(dt).kind == "c" else 8
    for n, M, S in ec.grid(dt):
        geo = d.hankel_gram_geometry(dt, n, M, S)
        plan = d.GramPlan(dt, n, M, S)
        assert (plan.segments, plan.seglen, plan.tile, plan.lag_group, plan.workspace_bytes) == geo, (n, M, S)
        segs, seglen, tile, group, ws = geo
        body = n - 2 * M + 2
        assert (tile, group) == (T, G) and seglen >= 1 and ws == segs * M * per                # a partial per (segment, lag)
        assert (segs - 1) * seglen < body <= segs * seglen                                      # [M - 1, L) exactly, no segment empty
        if S > 0:                                                                               # a forced cut is honoured, clamped to the body
            assert seglen == -(-body // min(S, body)) and segs == -(-body // seglen) and segs <= S
    assert d.hankel_gram_geometry(dt, 7, 2, 100)[:2] == (5, 1)                                  # clamped: one sample per segment at most
    for n, M in ((1 << 20, 5), ((1 << 22) + 77, 300)):                                         # the automatic cut falls on tile boundaries
        segs, seglen, tile, _, _ = d.hankel_gram_geometry(dt, n, M)
        assert segs > 1 and seglen % tile == 0 and (segs - 1) * seglen < n - 2 * M + 2 <= segs * seglen
    assert d.hankel_gram_geometry(dt, 1000, 5)[0] == 1


def test_c_abi_argument_and_unsupported_errors():
    lib = _lib.lib()
    out = [C.c_int64() for _ in range(5)]
    refs = [C.byref(v) for v in out]
    f64 = _dev.md_dtype(np.float64)
    for args in ((99, 10, 2, 0), (f64, -1, 1, 0), (f64, 10, 0, 0), (f64, 10, -3, 0), (f64, 10, 2, -1)):
        with pytest.raises(d.ArgumentError):
            _lib.check(lib.mdsp_hankel_gram_geometry_for(*args, *refs))
        with pytest.raises(d.ArgumentError):
            d.GramPlan(np.float64, *args[1:]) if args[0] == f64 else _lib.check(lib.mdsp_hankel_gram_plan_create(C.byref(C.c_void_p()), *args))
    for n, M in ((10, 6), (0, 1), (2, 2)):                                                     # 2 M - 1 > n
        with pytest.raises(d.UnsupportedError):
            d.hankel_gram_geometry(np.float64, n, M)
        with pytest.raises(d.UnsupportedError):
            d.GramPlan(np.complex64, n, M)
    with pytest.raises(d.ArgumentError):
        _lib.check(lib.mdsp_hankel_gram_plan_create(None, f64, 10, 2, 0))
    with pytest.raises(d.ArgumentError):
        _lib.check(lib.mdsp_hankel_gram_plan_info(None, *refs))
    assert lib.mdsp_hankel_gram_geometry_for(f64, 10, 2, 0, None, None, None, None, None) == 0   # any output pointer may be NULL
    # exec and the emulation: ldr < M, NULL buffers -- refused before any device work, so without a device too
    plan = d.GramPlan(np.float64, 10, 3)
    x, r = np.ones(10), np.zeros((3, 3))
    for xp, rp, ldr in ((x.ctypes.data, r.ctypes.data, 2), (0, r.ctypes.data, 3), (x.ctypes.data, 0, 3), (x.ctypes.data + 4, r.ctypes.data, 3)):
        with pytest.raises(d.ArgumentError):
            plan.exec(xp, rp, ldr, stream=0)
    for xp, rp, ldr in ((x.ctypes.data, r.ctypes.data, 2), (0, r.ctypes.data, 3), (x.ctypes.data, 0, 3)):
        with pytest.raises(d.ArgumentError):
            _lib.check(lib.mdsp_hankel_gram_emulate_host(xp, f64, 10, 3, 0, rp, ldr))
    with pytest.raises(d.UnsupportedError):
        ec.emulate(np.ones(4), 3)


def test_python_refusals_come_before_device_work():
    x = np.ones(64)
    for bad in ((x, 8, 0), (x, 8, -1), (x, 65, 2), (x, 0, 1), (np.ones((4, 4)), 2, 1), (np.ones((2, 1, 3)), 2, 1)):
        with pytest.raises(d.ArgumentError):
            d.esprit(*bad)
    with pytest.raises(d.ArgumentError, match="`x` must be a 1D signal"):
        d.esprit(np.ones((4, 4)), 2, 1)
    for bad in ((x, 8, 8), (x, 8, 9), (x, 33, 2), (np.ones(4000), d.ESPRIT_MAX_M + 1, 2), (x.astype(np.float16), 8, 2)):
        with pytest.raises(d.UnsupportedError):
            d.esprit(*bad)
    for bad in ((x, 8.0, 2), (x, 8, True), (x, 8, 2, "1"), (np.array(["a", "b", "c"]), 1, 1)):
        with pytest.raises(TypeError):
            d.esprit(*bad)
    assert d.ESPRIT_MAX_M == 1024
    with pytest.raises(d.ArgumentError):
        d.hankel_gram(x, 0)
    with pytest.raises(d.UnsupportedError):
        d.hankel_gram(x, 33)
    with pytest.raises(TypeError):
        d.hankel_gram(np.ones((8, 8)), 2)
    R = ec.emulate(x, 4)
    R[1, 2] = np.nan
    with pytest.raises(d.ArgumentError):
        d.esprit_from_gram(R, 2)


def test_no_cpu_fallback():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    x = ec.signal(64, np.complex128)
    for call in (lambda: d.esprit(x, 8, 2), lambda: d.esprit(x.real.astype(np.float32), 8, 2, 100.0), lambda: d.hankel_gram(x, 8)):
        with pytest.raises(d.DeviceError):
            call()


@pytest.mark.parametrize("dt", ec.DTYPES, ids=lambda t: np.dtype(t).name)
def test_emulated_gram_matrix_structure_and_accuracy(dt):
    name = np.dtype(dt).name
    worst = (0.0, None)
    for n, M, S in ec.grid(dt):
        x, ld, e_serial = ec.references(n, M, name)
        R = ec.emulate(x, M, S)
        assert R.dtype == ec.out_dtype(dt) and R.shape == (M, M)
        assert np.array_equal(R, R.conj().T), (n, M, S, "not exactly Hermitian")
        if R.dtype.kind == "c":
            d_im = np.diagonal(R).imag
            assert not d_im.any() and not np.signbit(d_im).any(), (n, M, S, "the diagonal's imaginary part is not +0.0")
        e_emul = ref.gram_error(R, ld)
        ratio = e_emul / max(e_serial, EPS)
        if ratio > worst[0]:
            worst = (ratio, (n, M, S, e_emul, e_serial))
        assert e_emul <= ec.GRAM_C * max(e_serial, EPS), (n, M, S, e_emul, e_serial)
    print(f"{name}: worst e_emul / max(e_serial, eps) {worst[0]:.3g} at (n, M, segments, e_emul, e_serial) = {worst[1]}")


def test_emulation_respects_ldr_and_flows_nan_through():
    x = ec.signal(40, np.complex64)
    buf = ec.emulate(x, 5, 1, ldr=8)
    assert np.array_equal(buf[:, :5].T, ec.emulate(x, 5, 1)) and np.isnan(buf[:, 5:]).all()    # rows M .. ldr - 1 of every column are not touched
    y = x.copy()
    y[17] = np.nan
    assert np.isnan(ec.emulate(y, 5, 3)).any()


def test_gram_route_agrees_with_the_svd_route():
    worst = 0.0
    for name, x, M, p, Fs, truth, f_svd, sv_ratio in ec.route_cases():
        assert sv_ratio >= ec.ROUTE_MIN_SV_RATIO, (name, sv_ratio)
        f = np.sort(ref.finish(ec.emulate(x, M), p, Fs))
        assert f.dtype == np.float64 and f.shape == (p,)
        assert f.tobytes() == np.sort(d.esprit_from_gram(ec.emulate(x, M), p, Fs)).tobytes(), name   # the package's finish is these calls
        e = float(np.max(np.abs(f - f_svd)) / Fs)
        worst = max(worst, e)
        print(f"{name}: N {len(x)}, M {M}, p {p}: sigma_p / sigma_1 {sv_ratio:.3g}, |f_gram - f_svd| / Fs {e:.3g}")
        assert e <= ec.ROUTE_BOUND, (name, e)
    print(f"worst {worst:.3g} of {ec.ROUTE_BOUND:.3g}")


def test_reference_test_case_on_the_emulation():
    """test/estimation.jl:19-20: the sorted estimates within atol = 1e-2 Hz of 1000 and 1250."""
    name, x, M, p, Fs, truth, f_svd, _ = ec.route_cases()[0]
    f = np.sort(d.esprit_from_gram(ec.emulate(x, M), p, Fs))
    print(f"{name}: {f} against {truth}")
    assert np.max(np.abs(f - np.array(truth))) <= 1e-2
    assert np.max(np.abs(f_svd - np.array(truth))) <= 1e-2
