"""The guard-band checker (tests/guard_bands.py) catches what it claims, and the case tables of the guard tests (tests/guard_cases.py) reach every kernel
form they name.  No device.

A numpy stand-in "kernel" -- direct convolution per column, reading and writing through flat indices into the guard buffers as a device kernel would --
passes the checks when it is right and fails them, at the right column and offset, with each planted defect: a store one element past nout in the last
column, a store `lead` elements in front of column 0, a store into the ld padding, an output never written, a read of x[-1], a read of x[nx].

The coverage half is host arithmetic against the built library (mdsp_ols_geometry_for / _tile_for / _stream_for and mdsp_spectral_route_for need no
device), like tests/test_ols_tile_rule_cpu.py and tests/test_spectral_route_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import guard_bands as gb
import guard_cases as gc
import spectral_route_cases as src

NX, NB, NCOLS, LEAD = 300, 17, 3, 63
NOUT = NX + NB - 1


def _standin(xbuf, lx, ybuf, ly, b, defect=None):
    """y[c][k] = sum_j b[j] x[c][k - j], samples outside [0, nx) read as zeros -- unless a defect says otherwise.  Works on the flat buffers only."""
    x, y = xbuf.view(lx.dtype), ybuf.view(ly.dtype)
    for c in range(lx.ncols):
        x0, y0 = lx.col0 + c * lx.ld, ly.col0 + c * ly.ld

        def sample(i, c=c, x0=x0):
            if 0 <= i < lx.n or (defect == "read x[-1]" and c == 1 and i == -1) or (defect == "read x[nx]" and c == 1 and i == lx.n):
                return x[x0 + i]
            return lx.dtype.type(0)

        for k in range(ly.n):
            if defect == "unwritten" and c == 2 and k == 100:
                continue
            # (the taps one past either end of the column take part, as a kernel's window would hold them)
            y[y0 + k] = sum(b[j] * sample(k - j) for j in range(len(b)) if -1 <= k - j <= lx.n)
    last = ly.col0 + (ly.ncols - 1) * ly.ld
    if defect == "past nout":
        y[last + ly.n] = 1.0
    if defect == "before column 0":
        y[ly.col0 - LEAD] = 1.0
    if defect == "into padding":
        y[ly.col0 + ly.ld + ly.n + 2] = 1.0


def _run(dtype, defect, base_x=3, base_y=1):
    rng = np.random.default_rng(5)
    cols = rng.standard_normal((NCOLS, NX)).astype(dtype)
    b = rng.standard_normal(NB).astype(dtype)
    if np.dtype(dtype).kind == "c":
        cols = (cols + 1j * rng.standard_normal((NCOLS, NX))).astype(dtype)
    lx = gb.layout(NX, NCOLS, NX + 5, gb.MIN_GUARD, gb.MIN_GUARD, base_x, dtype)
    ly = gb.layout(NOUT, NCOLS, NOUT + 7, gb.MIN_GUARD, gb.MIN_GUARD, base_y, dtype)
    xbuf, ybuf = gb.new_input(lx, cols), gb.new_output(ly)
    with np.errstate(invalid="ignore"):
        _standin(xbuf, lx, ybuf, ly, b, defect)
    return cols, b, ly, ybuf


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_correct_standin_passes(dtype):
    cols, b, ly, ybuf = _run(dtype, None)
    gb.check_output(ybuf, ly, NOUT)
    got = gb.columns(ybuf, ly)
    for c in range(NCOLS):
        ref = np.convolve(cols[c].astype(np.complex128), b.astype(np.complex128))
        assert np.linalg.norm(got[c] - ref) <= 1e-5 * np.linalg.norm(ref)
    cols0, _, ly0, ybuf0 = _run(dtype, None, 0, 0)                       # placement does not change the stand-in's bits either
    assert np.array_equal(gb.columns(ybuf0, ly0).view(np.uint8), got.view(np.uint8))


# defect -> (kind, column, element index relative to the column, distance)
DEFECTS = {
    "past nout": ("stray", NCOLS - 1, NOUT, 1),
    "before column 0": ("stray", 0, -LEAD, LEAD),
    "into padding": ("stray", 1, NOUT + 2, 3),
    "unwritten": ("unwritten", 2, 100, 100),
    "read x[-1]": ("nan", 1, 0, 0),                 # x[-1] sits under tap k + 1 of output k: outputs 0 .. nb - 2 of the column are NaN, the first is reported
    "read x[nx]": ("nan", 1, NX, NB - 2),           # x[nx] reaches outputs nx .. nx + nb - 1
}


@pytest.mark.parametrize("dtype", [np.float32, np.complex128])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_is_reported_where_it_is(defect, dtype):
    _, _, ly, ybuf = _run(dtype, defect)
    with pytest.raises(gb.GuardError) as err:
        gb.check_output(ybuf, ly, NOUT, defect)
    e = err.value
    assert (e.kind, e.column, e.index, e.distance) == DEFECTS[defect], str(e)
    assert f"column {e.column}, element {e.index}" in str(e) and defect in str(e)


def test_fill_and_poison_are_distinct_quiet_nans():
    for dt in (np.float32, np.float64, np.complex64, np.complex128):
        k, w = gb.words(gb.layout(1, 1, 1, gb.MIN_GUARD, gb.MIN_GUARD, 0, dt))
        p, f = gb.poison_word(dt), gb.fill_word(dt)
        assert p != f and np.isnan(np.array([p, f], dtype=w).view({4: np.float32, 8: np.float64}[np.dtype(w).itemsize])).all()
    lay = gb.layout(10, 2, 13, 5000, 4096, 3, np.complex64)
    assert lay.front % gb.LINE_ELEMS == 0 and lay.col0 == lay.front + 3 and lay.total == lay.col0 + 26 + 4096
    buf = gb.new_input(lay, np.ones((2, 10), np.complex64))
    el = buf.view(np.complex64)
    assert np.isnan(el[:lay.col0].real).all() and np.isnan(el[:lay.col0].imag).all() and np.isnan(el[lay.col0 + 10:lay.col0 + 13].imag).all()
    assert (gb.columns(buf, lay) == 1).all()
    with pytest.raises(ValueError):
        gb.layout(10, 1, 10, 100, 4096, 0)           # a guard below the minimum


def test_per_column_written_counts():
    """n_written per column (a resampler reports how many outputs each column got): elements beyond a column's own count must keep the fill."""
    ly = gb.layout(20, 2, 23, gb.MIN_GUARD, gb.MIN_GUARD, 1, np.float32)
    buf = gb.new_output(ly)
    y = buf.view(np.float32)
    y[ly.col0:ly.col0 + 20] = 1.0
    y[ly.col0 + 23:ly.col0 + 23 + 15] = 1.0
    gb.check_output(buf, ly, [20, 15])
    with pytest.raises(gb.GuardError) as err:
        gb.check_output(buf, ly, [19, 15])
    assert (err.value.kind, err.value.column, err.value.index, err.value.distance) == ("stray", 0, 19, 1)


# ---- coverage: overlap-save --------------------------------------------------------------------------------------------------------------------------
def _lib():
    from dsp_jl_amd import _lib as L
    return L


@pytest.mark.parametrize("fid", [f.id for f in gc.OLS_FORMS])
def test_ols_case_runs_the_form_it_names(fid):
    L = _lib()
    lib = L.lib()
    f = gc.OLS_BY_ID[fid]
    try:
        for k, v in {**f.create, **f.launch}.items():
            L.set_tunable(k, v)
        for mode in (L.OLS_FILT, L.OLS_CONV):
            en, el, ep, eg, er, t, l = C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
            L.check(lib.mdsp_ols_geometry_for(f.nb, f.nfft, 0, f.dtype, mode, f.engine, C.byref(en), C.byref(el), C.byref(ep), C.byref(eg), C.byref(er)))
            L.check(lib.mdsp_ols_tile_for(f.nb, f.nfft, 0, f.dtype, mode, f.engine, C.byref(t), C.byref(l)))
            assert (en.value, ep.value, er.value, eg.value, t.value, l.value) == f.expect, (fid, mode)
            assert el.value == (en.value // 2 if ep.value > 1 else en.value - (f.nb - 1))
            for nx in gc.ols_lengths(f):
                for nout in gc.ols_nouts(f, nx, mode == L.OLS_CONV):
                    assert 0 <= nout <= nx + f.nb - 1
                    s = C.c_int(-1)
                    L.check(lib.mdsp_ols_stream_for(nx, nout, f.ncols, f.dtype, C.byref(s)))
                    assert s.value == f.streaming and (f.streaming == 0 or (t.value, l.value) == (1792, 256)), (fid, nx, nout)
    finally:
        for k in {**f.create, **f.launch}:
            L.set_tunable(k, None)


def test_ols_table_names_every_form():
    """The forms the overlap-save engine has, by what the host queries report: each must be in the table.  The classification reads
    the table's own `expect` tuples, which means something only because test_ols_case_runs_the_form_it_names holds every one of them to the library."""
    seen = set()
    for f in gc.OLS_FORMS:
        en, parts, rows, eng, tile, lead = f.expect
        kind = ("rocfft" if eng == gc.ROCFFT else "partitioned" if parts > 1 else "rows%d" % rows if rows else "three-pass" if en > 8192 else
                "tiled-stream%d" % f.streaming if (tile, lead) == (1792, 256) else "reblocked" if en != f.nfft else "single")
        seen.add((f.dtype, kind))
    F32, F64, C32, C64 = gc.F32, gc.F64, gc.C32, gc.C64
    want = {(F32, "single"), (F32, "tiled-stream0"), (F32, "tiled-stream1"), (F32, "reblocked"), (F32, "partitioned"), (F32, "rows64"), (F32, "rows256"),
            (F32, "three-pass"), (F32, "rocfft"), (F64, "single"), (F64, "partitioned"), (F64, "rows64"), (C32, "single"), (C64, "single"), (C32, "rows64"),
            (C32, "rocfft")}
    assert seen == want, (seen ^ want)
    assert {gc.OLS_BY_ID[i].expect[1] for i in gc.OLS_RANGE_FORMS} == {1, 3} and gc.OLS_BY_ID[gc.OLS_RANGE_FORMS[0]].expect[4:] == (1792, 256)
    assert sorted(f.expect[1] for f in gc.OLS_FORMS if f.dtype == F32 and f.expect[1] > 1) == [3, 4]
    assert sorted(f.nb for f in gc.OLS_FORMS if f.expect[4:] == (1792, 256) and f.streaming == 0) == [249, 256, 257]


# ---- coverage: Welch / STFT --------------------------------------------------------------------------------------------------------------------------
def _route(lib, kind, dtype, nfft, engine):
    """Route character as tests/spectral_route_cases.py writes it ('-': plan creation would fail with MDSP_ERR_UNSUPPORTED)."""
    return src.encode(lib, kind, dtype, engine, [nfft])[0]


@pytest.mark.parametrize("dtype", src.DTYPES)
@pytest.mark.parametrize("kind", src.KINDS)
def test_spectral_cases_cover_every_route_of_the_table(kind, dtype):
    lib = _lib().lib()
    cases = gc.spectral_cases(kind, dtype)
    assert len(set(cases)) == len(cases)
    for engine, nfft, c in cases:                      # every case runs the route it names
        assert nfft >= 8 and _route(lib, kind, dtype, nfft, engine) == c, (kind, dtype, engine, nfft, c)
    table = src.expected_default()
    for engine in (gc.AUTO, gc.FUSED):
        want = set(table[(kind, dtype, engine)][0]) - {"-"}
        # a case of engine AUTO stands for FUSED too where FUSED takes the same route at that size: the same kernel
        covered = {c for e, n, c in cases if e == engine or (e == gc.AUTO and _route(lib, kind, dtype, n, engine) == c)}
        assert covered == want, (kind, dtype, engine, sorted(covered ^ want))
    assert [c for e, n, c in cases if e == gc.ROCFFT] == ["0"] and set(table[(kind, dtype, gc.ROCFFT)][0]) == {"0"}
    # the register-resident power-of-two route: every size it covers is a kernel of its own, and each is a case
    pow2 = [n for n, c in zip(src.SIZES, table[(kind, dtype, gc.AUTO)][0]) if c == gc.POW2_ROUTE]
    assert pow2 == [256 << i for i in range(6 if dtype in (gc.F32, gc.C32) else 5)]
    assert [n for e, n, c in cases if e == gc.AUTO and c == gc.POW2_ROUTE] == pow2
    for n in {n for _, n, _ in cases}:
        for nn, nov, hop, length in gc.spectral_shapes(n):
            assert 0 < nov < nn <= n and (length - nn) // hop + 1 == 3 and (length - nn) % hop == hop - 1


@pytest.mark.parametrize("dtype", src.DTYPES)
def test_multitaper_sizes(dtype):
    lib = _lib().lib()
    sizes = gc.mt_sizes(dtype)
    assert [c for _, c in sizes] == ["1", "3", "a"]
    for n, c in sizes:
        assert _route(lib, gc.KIND_STFT, dtype, n, gc.AUTO) == c
