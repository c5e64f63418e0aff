"""lpc / arburg / levinson without a device: the index form of Burg's recursion against the reference's push/pop form, the library's host emulation
(the text the kernels compile, csrc/burg_op.h) against the long-double restatement with the bound of tests/lpc_cases.py, the geometry, levinson on the host,
the argument errors, and the reference's own statistical test (test/lpc.jl:3-15) on the restatement."""
import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
from conftest import isapprox

import lpc_cases as lc
import lpc_ref as ref


def _same_bits(u, v):
    u, v = np.asarray(u), np.asarray(v)
    return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_index_form_equals_the_push_pop_form_bit_for_bit(dt):
    for fam in lc.FAMILIES:
        for n, p in ((2, 1), (3, 2), (41, 3), (41, 40), (300, 17)):
            x = lc.signal(fam, n, dt)
            for got, want in zip(ref.arburg_index(x, p), ref.arburg_pushpop(x, p)):
                assert _same_bits(got, want), (fam, n, p)


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_emulation_against_long_double(dt):
    name = np.dtype(dt).name
    rows = lc.table(dt)
    assert any(S == 65 and lc.geometry(dt, n, S)[0] == 65 for _, n, _, S in rows)
    worst = {}
    for fam, n, p, S in rows:
        x, ld, _ = lc.references(fam, n, p, name)
        e_serial = lc.serial_error_of_family(fam, name)
        a, err, refl = lc.emulate(x, p, S)
        assert a.dtype == np.dtype(dt) and refl.dtype == np.dtype(dt) and len(a) == p + 1 and len(refl) == p and a[0] == 1
        assert np.asarray(err).dtype == ref.real_dtype(dt)
        e_emul = lc.burg_error((a, err, refl), ld)
        if fam not in worst or e_emul > worst[fam][0]:
            worst[fam] = (e_emul, n, p, S, e_serial)
        assert e_emul <= lc.BURG_C * e_serial, (fam, n, p, S, e_emul, e_serial)
        if lc.is_long(n, dt):                                                                 # the rows where the problem is posed well, against their own maximum
            e_long = lc.serial_error_of_long_rows(fam, name)
            assert e_emul <= lc.BURG_C_LONG * e_long, (fam, n, p, S, e_emul, e_long)
    for fam, (e_emul, n, p, S, e_serial) in worst.items():
        print(f"{name} {fam}: worst e_emul {e_emul:.3g} (n {n}, p {p}, segments {S}) against e_serial {e_serial:.3g}: ratio {e_emul / e_serial:.3g}")


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_well_conditioned_rows_agree_with_the_restatement_to_rounding(dt):
    """The bound above is carried by the ill-conditioned rows (p = N - 1).  The AR(3) family at p = 3 with many samples per coefficient is well conditioned
    (every |k| is below 0.8, so no 1 - |k|^2 cancels): there the emulation and the working-precision restatement differ only in the order and the
    precision of their sums, and N terms added in two orders differ by N units of roundoff at most."""
    eps = np.finfo(ref.real_dtype(dt)).eps
    n = 2 * lc.tile_of(dt) + 3
    x = lc.signal("ar3", n, dt)
    want = ref.arburg_pushpop(x, 3)
    assert np.max(np.abs(want[2])) < 0.8
    for S in (1, 3, 65):
        e = lc.burg_error(lc.emulate(x, 3, S), want)
        print(f"{np.dtype(dt).name} segments {S}: {e / eps:.3g} eps of {n} allowed")
        assert e <= n * eps, S


@pytest.mark.parametrize("dt", lc.DTYPES, ids=lambda t: np.dtype(t).name)
def test_geometry_tiles_the_pair_range(dt):
    tile = lc.tile_of(dt)
    seen = set()
    for _, n, _, S in lc.table(dt):
        if (n, S) in seen:
            continue
        seen.add((n, S))
        segs, seglen, t, ws = lc.geometry(dt, n, S)
        assert t == tile and 1 <= segs <= S and seglen >= 1
        bounds = [(s * seglen, min((s + 1) * seglen, n - 1)) for s in range(segs)]
        assert bounds[0][0] == 0 and bounds[-1][1] == n - 1                                   # [0, N - 1) exactly ...
        assert all(lo < hi for lo, hi in bounds) and all(bounds[i][1] == bounds[i + 1][0] for i in range(segs - 1))   # ... no gap, none empty
        assert ws >= 2 * n * np.dtype(dt).itemsize + 24 * segs
    for n in (1 << 20, (1 << 24) + 5, 1 << 26):                                               # the automatic cut falls on tile boundaries
        segs, seglen, t, ws = lc.geometry(dt, n)
        assert seglen % tile == 0 and (segs - 1) * seglen < n - 1 <= segs * seglen and segs <= 256 * 16
    assert lc.geometry(dt, 1000)[0] == 1
    with pytest.raises(d.ArgumentError):
        lc.geometry(dt, 0)
    with pytest.raises(d.ArgumentError):
        lc.geometry(dt, 10, -1)


def test_emulation_rejects_bad_orders_and_flows_nan_through():
    x = lc.signal("ar3", 10, np.float64)
    for p in (-1, 10, 11):
        with pytest.raises(d.ArgumentError):
            lc.emulate(x, p)
    a, err, refl = lc.emulate(np.zeros(8), 2)                                                 # a zero signal: 0 / 0 as in the reference
    assert np.isnan(refl).all() and np.isnan(a[1:]).all() and np.isnan(err)
    want = ref.arburg_pushpop(np.zeros(8), 2)
    assert np.isnan(want[2]).all()
    y = x.copy()
    y[4] = np.inf
    assert np.isnan(lc.emulate(y, 2)[2]).all()
    a, err, refl = lc.emulate(x, 0)
    assert a.tolist() == [1.0] and len(refl) == 0 and abs(err - np.mean(x * x)) <= 4 * np.finfo(float).eps * err


def test_levinson_reference_case_and_toeplitz_solution():
    a, err, refl = d.levinson(np.arange(1, 11).astype(np.complex128), 3)                      # test/lpc.jl:18
    assert isapprox(a.real, -np.array([1.25, 0.0, 0.25]))
    a_int, _, _ = d.levinson(np.arange(1, 11), 3)                                             # integers: Float64
    assert a_int.dtype == np.float64 and isapprox(a_int, -np.array([1.25, 0.0, 0.25]))
    rng = np.random.default_rng(3)
    for dt in lc.DTYPES:
        for p in (1, 2, 5, 12):
            x = lc.signal("ar3", 400, dt, seed=int(rng.integers(1 << 30)))
            r = ref.xcorr_biased_lags(x, p)
            a, err, refl = d.levinson(r, p)
            assert a.dtype == np.dtype(dt) and refl.dtype == np.dtype(dt) and np.asarray(err).dtype == ref.real_dtype(dt)
            r64 = r.astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
            T = np.array([[r64[i - j] if i >= j else np.conj(r64[j - i]) for j in range(p)] for i in range(p)])
            assert isapprox(a, np.linalg.solve(T, -r64[1:p + 1]).astype(dt)), (dt, p)         # T (-a) = r[1:]; the default rtol of the working type, as Julia's
            assert a[-1] == refl[-1]
            want = ref.levinson(r, p)
            assert all(_same_bits(u, v) for u, v in zip((a, err, refl), want)), (dt, p)


def test_levinson_type_rules_and_errors():
    assert d.levinson(np.array([4, 2, 1], dtype=np.int32), 2)[0].dtype == np.float64
    assert d.levinson(np.array([True, False, True]), 1)[0].dtype == np.float64
    assert d.levinson(np.array([4, 2, 1], dtype=np.float32), 2)[0].dtype == np.float32
    assert d.levinson(np.array([4, 2j, 1], dtype=np.complex64), 2)[0].dtype == np.complex64
    assert d.levinson([4.0, 2.0, 1.0, 0.5], 2)[0].shape == (2,)                               # only the first p + 1 numbers are used
    for bad_p in (0, -1, 3):
        with pytest.raises(d.ArgumentError):
            d.levinson(np.ones(3), bad_p)
    with pytest.raises(TypeError):
        d.levinson(np.ones((3, 3)), 1)
    with pytest.raises(TypeError):
        d.levinson(np.ones(3), 1.5)
    with pytest.raises(d.UnsupportedError):
        d.levinson(np.ones(3, dtype=np.float16), 1)


def test_argument_errors_come_before_device_work():
    x = np.ones(8)
    for fn in (d.arburg, d.lpc, lambda v, p: d.lpc(v, p, d.LPCLevinson())):
        with pytest.raises(TypeError):
            fn(np.ones((4, 4)), 2)
        with pytest.raises(TypeError):
            fn(np.array(["a", "b", "c"]), 1)
        with pytest.raises(TypeError):
            fn(x, 2.5)
        with pytest.raises(TypeError):
            fn(x, True)
        with pytest.raises(d.ArgumentError):
            fn(x, -1)
        with pytest.raises(d.ArgumentError):
            fn(x, 8)                                                                          # p = N: 0 / 0 in the reference
        with pytest.raises(d.ArgumentError):
            fn(x, 9)
        with pytest.raises(d.UnsupportedError):
            fn(np.ones(8, dtype=np.float16), 2)
    with pytest.raises(d.ArgumentError):
        d.lpc(x, 0, d.LPCLevinson())
    with pytest.raises(TypeError):
        d.lpc(x, 2, "burg")
    assert d.LPCBurg() == d.LPCBurg() and d.LPCBurg() != d.LPCLevinson()


def test_no_cpu_fallback():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    x = lc.signal("ar3", 64, np.float64)
    for call in (lambda: d.arburg(x, 3), lambda: d.arburg(x, 0), lambda: d.lpc(x, 3), lambda: d.lpc(x, 3, d.LPCBurg()), lambda: d.lpc(x, 3, d.LPCLevinson()),
                 lambda: d.lpc(x.astype(np.int64), 3)):
        with pytest.raises(d.DeviceError):
            call()


@pytest.mark.parametrize("cplx", [False, True], ids=["Float64", "ComplexF64"])
def test_reference_statistical_test_on_the_restatement(cplx):
    """test/lpc.jl:3-15 for both methods, and the seed's margin: the restatement sits below half of each bound, so that the device tests (which run the same
    input through the library) do not stand on a lucky draw."""
    x, coeffs, var = lc.stat_cached(cplx)
    assert len(x) == lc.STAT_N - lc.STAT_SKIP
    a, e, _ = ref.arburg_pushpop(x, 3)
    for ar, err in ((a[1:], e), ref.lpc_levinson(x, 3)):
        worst = float(np.max(np.abs(ar - coeffs[1:])))
        rel = abs(float(err) - var) / max(abs(float(err)), var)
        print(f"|ar - coeffs| {worst:.4f}, e {float(err):.5f} against var(s) {var:.5f}: {rel:.4f}")
        assert worst < 0.01 and rel <= 0.01                                                   # the reference's bounds
        assert worst < 0.005 and rel <= 0.005                                                 # the margin of the seed
    ae, ee, _ = lc.emulate(x, 3)                                                              # and the emulation, through the automatic cut
    assert float(np.max(np.abs(ae[1:] - coeffs[1:]))) < 0.01 and abs(float(ee) - var) <= 0.01 * max(abs(float(ee)), var)
