"""The case table of the chunk-seam tests (tests/chunk_cases.py) against the library's own host arithmetic -- no device: mdsp_chunk_units_for under each
case's knobs gives the chunk schedule of its loop, mdsp_spectral_route_for and mdsp_ols_geometry_for the kernel family that runs.  Per case: the number of
chunks, the size of the last one, "a chunk spans channels", "the last unit holds one frame", and one chunk (or as many as the table says) under the budget
the GPU test compares against.  A budget or a route that changes fails here; the GPU tests do not quietly go back to one chunk.

Also mdsp_chunk_units_for itself: the values of the loops' own expressions under the default tunables, its bounds and its argument checks."""
import ctypes as C

import pytest

import chunk_cases as cc
from dsp_jl_amd import _lib


class _Knobs:
    def __init__(self, *knobs):
        self.knobs = {}
        for k in knobs:
            self.knobs.update(k)

    def __enter__(self):
        for k, v in self.knobs.items():
            _lib.set_tunable(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            _lib.set_tunable(k, None)


def _per_chunk(kind, dtype, n, units):
    c = C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_chunk_units_for(kind, dtype, n, units, C.byref(c)))
    return c.value


def _route(kind, dtype, nfft, engine):
    e, r, r0 = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().mdsp_spectral_route_for(kind, dtype, nfft, engine, C.byref(e), C.byref(r), C.byref(r0)))
    return e.value, r.value


def _check_schedule(what, sched, expect, group=None, one_frame=None):
    """sched: [(first unit, count)].  group: units per channel (column) when the loop's units run across channels."""
    assert len(sched) == expect["chunks"], (what, "chunks", len(sched), sched[:4])
    assert sched[-1][1] == expect["last"], (what, "last chunk", sched[-1])
    if len(sched) > 1:
        assert all(cnt == sched[0][1] for _, cnt in sched[:-1]) and sched[-1][1] <= sched[0][1], (what, sched[:4])
    if group is not None:
        spans = any(u0 // group != (u0 + cnt - 1) // group for u0, cnt in sched)
        assert spans == expect["spans"], (what, "a chunk spans channels", spans)
    else:
        assert not expect["spans"], what
    if one_frame is not None:
        assert one_frame == expect["one_frame"], (what, "the last unit holds one frame", one_frame)


@pytest.mark.parametrize("cid", [c.id for c in cc.SPECTRAL])
def test_spectral_case_crosses_its_budget(cid):
    case = cc.BY_ID[cid]
    sh, dt = case.shape, case.dtype
    lib = _lib.lib()
    kind = cc.LOOP_KIND[case.loop]
    rocfft = case.loop.startswith("rocfft")
    with _Knobs(case.create):
        eng, route = _route(0 if case.op in ("welch", "stream") else 1, dt, sh["nfft"], cc.ROCFFT if rocfft else cc.FUSED)
    assert (eng, route) == ((cc.ROCFFT, cc.ROUTE_ROCFFT) if rocfft else (cc.FUSED, cc.ROUTE_BIG)), (cid, eng, route)
    # the frame count the table names is the one the library frames the signal into
    assert lib.mdsp_frame_count(cc.spectral_length(sh), sh["n"], sh["noverlap"]) == sh["K"], cid
    if case.op == "stream":
        assert sum(sh["slices"]) == sh["K"]
        assert cc.is_complex(dt) or all(k % 2 == 0 for k in sh["slices"][:-1])      # even slices keep the one-shot call's pairs of real frames
    if case.loop in ("big_welch", "big_welch_rows"):
        rows_knob = case.launch.get("MDSP_BIG_WELCH_ROWS", 1)
        r0 = cc.welch_rows_r0(dt, sh["nfft"]) if rows_knob else 0
        assert (r0 > 0) == (case.loop == "big_welch_rows"), (cid, r0)
        if r0 >= 128 and not cc.is_double(dt):       # (bigfft.hip welch: the 128- and 256-row forms keep three passes below 32 transforms)
            assert cc.spectral_units(case)[0] >= 32
    units = cc.spectral_units(case)
    expects = [dict(case.expect, chunks=c, last=l) for c, l in case.expect["slices"]] if case.op == "stream" else [case.expect] * len(units)
    frames = list(sh["slices"]) if case.op == "stream" else [sh["K"]] * len(units)
    for u, exp, k in zip(units, expects, frames):
        with _Knobs(case.launch):
            per = _per_chunk(kind, dt, sh["nfft"], u)
        one = None if cc.is_complex(dt) or rocfft else (k % 2 == 1)
        if case.op == "stream":
            one = None
        _check_schedule(cid, cc.schedule(u, per), exp, group=sh["K"] if rocfft else None, one_frame=one)
        ref = _per_chunk(kind, dt, sh["nfft"], u)                       # the default budget
        assert len(cc.schedule(u, ref)) == case.expect["ref_chunks"], (cid, "default budget", ref)
    assert case.expect["chunks"] >= 3 or case.op == "stream"


@pytest.mark.parametrize("cid", [c.id for c in cc.OLS])
def test_overlap_save_case_crosses_its_budget(cid):
    case = cc.BY_ID[cid]
    sh, dt = case.shape, case.dtype
    lib = _lib.lib()
    en, el, ep, eg, er = C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    with _Knobs(case.create):
        _lib.check(lib.mdsp_ols_geometry_for(sh["nb"], sh["nfft"], sh["nx_hint"], dt, sh["mode"], sh["engine"], C.byref(en), C.byref(el), C.byref(ep), C.byref(eg),
                                             C.byref(er)))
    assert (en.value, el.value, ep.value, eg.value, er.value) == case.expect["geometry"], cid
    assert (er.value > 0) == (case.loop == "big_ols_rows") and (eg.value == cc.ROCFFT) == (case.loop == "rocfft_ols")
    L = el.value
    nx, nout = cc.ols_sizes(case)
    assert -(-nout // L) == sh["nblocks"] and 0 < nx and nout <= nx + sh["nb"] - 1
    kind = cc.LOOP_KIND[case.loop]
    real = not cc.is_complex(dt)
    for g0, exp in ((0, case.expect), (sh["range_from"], case.expect["range"])):
        if g0 is None:
            continue
        assert exp is not None and (g0 == 0 or case.loop != "rocfft_ols")
        if real:
            assert g0 % 2 == 0                                          # two real blocks share a transform
        walk, cap = cc.ols_units(case, g0)
        with _Knobs(case.launch):
            per = _per_chunk(kind, dt, en.value, cap)
        first = g0 if not real or case.loop == "rocfft_ols" else g0 // 2
        one = (sh["nblocks"] % 2 == 1) if real and case.loop != "rocfft_ols" else None
        if not real:
            assert not exp["one_frame"]
        _check_schedule((cid, g0), cc.schedule(walk, per, first), exp, group=sh["nblocks"] if case.loop == "rocfft_ols" else None,
                        one_frame=one if real and case.loop != "rocfft_ols" else None)
        if g0 == 0:
            assert len(cc.schedule(walk, _per_chunk(kind, dt, en.value, cap))) == exp["ref_chunks"], (cid, "default budget")
        else:
            # the range starts inside the whole call's second chunk, and its own seams are where the table says
            whole = cc.schedule(cc.ols_units(case)[0], per)
            assert whole[1][0] <= first < whole[1][0] + whole[1][1], (cid, first, whole)
    assert case.expect["chunks"] >= 3


@pytest.mark.parametrize("cid", [c.id for c in cc.HILBERT])
def test_hilbert_case_crosses_its_budget(cid):
    case = cc.BY_ID[cid]
    sh = case.shape
    per = _per_chunk(cc.CHUNK_HILBERT, case.dtype, sh["n"], sh["ncols"])
    _check_schedule(cid, cc.schedule(sh["ncols"], per), case.expect)
    assert sh["ncols"] <= 65535                                       # mdsp_hilbert's limit per call
    if cid.endswith("long-columns"):
        assert -(-sh["n"] // 256) > 4096 and sh["n"] > cc.HILBERT_GRID_CAP      # the kernels' grids are capped and every thread strides
    else:
        assert sh["n"] < cc.HILBERT_GRID_CAP and case.expect["chunks"] >= 3


def test_every_loop_has_a_case_of_three_chunks_or_more():
    for loop in cc.LOOPS:
        assert any(c.loop == loop and c.expect["chunks"] >= 3 for c in cc.CASES), loop
    for loop in ("rocfft_welch", "rocfft_stft"):                                     # all four dtypes, both sides of a real signal
        have = {(c.dtype, c.shape["onesided"]) for c in cc.CASES if c.loop == loop}
        assert have >= {(cc.F32, True), (cc.F32, False), (cc.F64, True), (cc.F64, False), (cc.C32, False), (cc.C64, False)}, loop
    for cid, short in cc.REUSE:
        assert cid in cc.BY_ID and short >= 1


def test_reuse_cases_change_the_cached_batch():
    """The short call of a re-used plan takes fewer units per chunk than the long one: the plan's batch changes both ways."""
    for cid, short in cc.REUSE:
        case = cc.BY_ID[cid]
        kind = cc.LOOP_KIND[case.loop]
        with _Knobs(case.launch):
            if case.op == "ols":
                n, u_long, u_short = case.expect["geometry"][0], cc.ols_units(case)[1], short * case.shape["ncols"]
            elif case.op == "hilbert":
                n, u_long, u_short = case.shape["n"], case.shape["ncols"], short
            else:
                n, u_long, u_short = case.shape["nfft"], cc.spectral_units(case)[0], cc.spectral_units(case, short)[0]
            assert _per_chunk(kind, case.dtype, n, u_short) == u_short < _per_chunk(kind, case.dtype, n, u_long), cid


def test_chunk_units_for_is_the_loops_arithmetic():
    """Under the default tunables: 192 MiB (rocFFT Welch / STFT), 64 MiB (rocFFT overlap-save), 256 MiB (hilbert), 1024 MiB (multi-pass engine; two buffers for
    overlap-save on natural-order spectra)."""
    many = 1 << 40
    for dt, rsz, cplx in ((cc.F32, 4, False), (cc.F64, 8, False), (cc.C32, 4, True), (cc.C64, 8, True)):
        for n in (64, 1000, 4096, 8192, 16384, 125000, 1 << 19, 1 << 24):
            nspec = n if cplx else n // 2 + 1
            esz = rsz * (2 if cplx else 1)
            for kind in (cc.CHUNK_ROCFFT_WELCH, cc.CHUNK_ROCFFT_STFT):
                assert _per_chunk(kind, dt, n, many) == max(1, (192 << 20) // (esz * n + 2 * rsz * nspec)), (kind, dt, n)
            assert _per_chunk(cc.CHUNK_ROCFFT_OLS, dt, n, many) == max(1, (64 << 20) // (esz * n + (0 if cplx else 2 * rsz * nspec))), (dt, n)
            if not cplx:
                assert _per_chunk(cc.CHUNK_HILBERT, dt, n, many) == max(1, (256 << 20) // (rsz * n + 2 * rsz * (n // 2 + 1 + n))), (dt, n)
            for kind, buffers in ((cc.CHUNK_BIG_SPECTRAL, 1), (cc.CHUNK_BIG_OLS_ROWS, 1), (cc.CHUNK_BIG_OLS, 2)):
                assert _per_chunk(kind, dt, n, many) == max(1, (1024 << 20) // (buffers * 2 * rsz * n)), (kind, dt, n)
    for kind in range(7):
        assert _per_chunk(kind, cc.F32, 1000, 7) == 7          # never more than there is to do
        assert _per_chunk(kind, cc.F32, 1000, 0) == 1          # ... and never less than one unit per chunk
        assert _per_chunk(kind, cc.F64, 1 << 30, 5) == 1       # a unit beyond the budget still runs, alone
    with _Knobs({"MDSP_ROCFFT_CHUNK_MIB": 1, "MDSP_BIG_CHUNK_MIB": 1}):
        assert _per_chunk(cc.CHUNK_ROCFFT_WELCH, cc.F32, 1000, many) == 130 and _per_chunk(cc.CHUNK_BIG_SPECTRAL, cc.F32, 16384, many) == 8
        assert _per_chunk(cc.CHUNK_BIG_OLS, cc.F32, 65536, many) == 1
        assert _per_chunk(cc.CHUNK_ROCFFT_OLS, cc.F32, 64, many) == 129055 and _per_chunk(cc.CHUNK_HILBERT, cc.F32, 1000, many) == 16768    # fixed budgets: no knob
    assert _per_chunk(cc.CHUNK_BIG_SPECTRAL, cc.F32, 16384, many) == 8192


def test_chunk_units_for_checks_its_arguments():
    lib = _lib.lib()
    c = C.c_int64()
    assert lib.mdsp_chunk_units_for(7, cc.F32, 1000, 10, C.byref(c)) == _lib.ERR_ARGUMENT
    assert lib.mdsp_chunk_units_for(-1, cc.F32, 1000, 10, C.byref(c)) == _lib.ERR_ARGUMENT
    assert lib.mdsp_chunk_units_for(0, 4, 1000, 10, C.byref(c)) == _lib.ERR_ARGUMENT
    assert lib.mdsp_chunk_units_for(0, cc.F32, 0, 10, C.byref(c)) == _lib.ERR_ARGUMENT
    assert lib.mdsp_chunk_units_for(0, cc.F32, 1000, -1, C.byref(c)) == _lib.ERR_ARGUMENT
    assert lib.mdsp_chunk_units_for(cc.CHUNK_HILBERT, cc.C32, 1000, 10, C.byref(c)) == _lib.ERR_ARGUMENT       # hilbert takes real signals
    assert lib.mdsp_chunk_units_for(0, cc.F32, 1000, 10, None) == _lib.OK                                      # the output may be NULL
    assert (_lib.CHUNK_ROCFFT_WELCH, _lib.CHUNK_ROCFFT_STFT, _lib.CHUNK_ROCFFT_OLS, _lib.CHUNK_HILBERT, _lib.CHUNK_BIG_SPECTRAL, _lib.CHUNK_BIG_OLS,
            _lib.CHUNK_BIG_OLS_ROWS) == tuple(range(7))
