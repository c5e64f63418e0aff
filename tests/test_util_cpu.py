"""rms, rmsfft, meanfreq, finddelay, shiftsignal, alignsignals and the dB helpers without a device: the numpy restatements against the reference's doctests
and tie rules (src/util.jl:329-333, :380-391, :418-422), the geometry of the reduction plans, the host emulation of the device code (same geometry,
operators and lane walks: csrc/reduce_op.h) against the serial definitions for every forced cut, the shift planner and a host walk of its schedules
(csrc/shift_plan.h), and the argument checks of the Python layer, which come before any device work."""
import math

import numpy as np
import pytest

import dsp_jl_amd as d
from dsp_jl_amd import _lib
import util_cases as uc
import util_ref as ur

_op_ids = dict(ids=uc.op_id)


# ---- the restatements against the reference's doctests ---------------------------------------------------------------------------------------------------
def test_references_reproduce_the_doctests_and_tie_rules():
    assert ur.finddelay([0, 0, 1, 2, 3], [1, 2, 3]) == 2 and ur.finddelay([1, 2, 3], [0, 0, 1, 2, 3]) == -2           # :329-333
    assert ur.finddelay([0, 1, 0], [1, 0, 1]) == 1            # |xcorr| peaks at equal distance on both sides of the centre: the smaller index wins
    assert ur.finddelay([1, 0, 1], [1]) == 0                  # two peaks at distances 0 and 2: the nearer one wins
    assert ur.shiftsignal([1, 2, 3], 2).tolist() == [0, 0, 1] and ur.shiftsignal([1, 2, 3], -2).tolist() == [3, 0, 0]  # :380-391
    a, dl = ur.alignsignals([0, 0, 1, 2, 3], [1, 2, 3])
    assert (a.tolist(), dl) == ([1, 2, 3, 0, 0], 2)                                                                    # :418-419
    a, dl = ur.alignsignals([1, 2, 3], [0, 0, 1, 2, 3])
    assert (a.tolist(), dl) == ([0, 0, 1], -2)                                                                         # :421-422
    with pytest.raises(ValueError):
        ur.shiftsignal([1, 2, 3], 4)
    with pytest.raises(ValueError):
        ur.peak_rule(np.array([1.0, np.nan]), 0)
    assert ur.absargmax(np.array([1.0, np.nan, -np.inf, np.inf]), 3) == (3, 1) and ur.absargmax(np.array([np.nan]), 0) == (-1, 1)
    assert float(ur.rms([3.0, 4.0])) == math.sqrt(12.5) and abs(float(ur.rmsfft(np.fft.fft([3.0, 4.0]))) - math.sqrt(12.5)) < 1e-15


def test_finddelay_peaks_stand_clear_of_the_rest():
    """The GPU test asks for the exact delay: the second-largest |xcorr| is a small fraction of the peak, so transform rounding cannot move it."""
    for n, dl in ((257, 5), (4099, -37)):
        x, y = uc.delayed_pair(n, dl, np.float64)
        s = np.abs(ur.xcorr(y, x))
        assert ur.finddelay(x, y) == dl
        assert np.sort(s)[-2] / s.max() < 0.5, (n, np.sort(s)[-2] / s.max())


def test_db_helpers():
    for a in (0.5, 1, 3, 20.0, np.float32(7)):
        assert d.db2pow(a) == ur.db2pow(a) and d.db2amp(a) == ur.db2amp(a) and d.pow2db(a) == ur.pow2db(a) and d.amp2db(a) == ur.amp2db(a)
    assert d.db2pow(-3) == ur.db2pow(-3) and d.pow2db(0) == -math.inf
    assert abs(d.pow2db(d.db2pow(3)) - 3) < 1e-14 and abs(d.amp2db(d.db2amp(-6.5)) + 6.5) < 1e-14
    with pytest.raises(d.DomainError):
        d.pow2db(-1.0)
    with pytest.raises(TypeError):
        d.db2amp(1j)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op_dt", uc.OPS, **_op_ids)
def test_geometry_tiles_every_line_once(op_dt):
    op, dt = op_dt
    shapes = [(inner, n, outer) for n in uc.LENS + (uc.BIG, 2 ** 33) for inner in uc.INNERS for outer in uc.OUTERS]
    for inner, n, outer in shapes:
        for seg in uc.SEGMENTS + (64, 1000):
            route, S, seglen, depth, ws = uc.geometry(inner, n, outer, op, dt, seg)
            what = (inner, n, outer, seg, S, seglen)
            assert route == (_lib.REDUCE_CONTIGUOUS if inner == 1 else _lib.REDUCE_STRIDED), what
            assert S >= 1 and (S - 1) * seglen < n <= S * seglen, what                   # segments s * seglen .. tile [0, n) exactly once, none empty
            if seg:
                assert S <= seg and seglen == -(-n // min(seg, n)), what
            assert ws == (inner * outer * S * uc.ACC_BYTES[op] if S > 1 else 0), what
            assert depth >= 1, what
    # the automatic cut: one long line is cut, many lines are not
    assert uc.geometry(1, 2 ** 28, 1, op, dt)[1] == 8192 and uc.geometry(1, 4096, 65536, op, dt)[1] == 1 and uc.geometry(4096, 65536, 1, op, dt)[1] > 1
    assert uc.geometry(1, 4099, 1, op, dt)[1] == 1 and uc.geometry(1, uc.BIG, 1, op, dt)[1] > 1000


def test_geometry_argument_checks():
    for bad in ((-1, 4, 1, 0, uc.F32, 0), (1, 4, 1, 3, uc.F32, 0), (1, 4, 1, _lib.REDUCE_SUMABS2_W, uc.F32, 0), (1, 4, 1, _lib.REDUCE_ABSARGMAX, uc.C32, 0),
                (1, 4, 1, 0, uc.F32, -1), (2 ** 40, 2 ** 40, 1, 0, uc.F32, 0)):
        with pytest.raises(d.ArgumentError):
            uc.geometry(*bad)
    assert d.reduce_geometry(1, 100, 1, _lib.REDUCE_SUMABS2, np.float32, 2)[:3] == (_lib.REDUCE_CONTIGUOUS, 2, 50)


# ---- emulation against the serial definitions, for every forced cut -------------------------------------------------------------------------------------
SMALL = [(1, n, outer) for n in uc.LENS for outer in (1, 2)] + [(inner, n, outer) for n in (1, 2, 65, 257, 1023) for inner in (2, 3, 65) for outer in (1, 2)]


@pytest.mark.parametrize("dt", [uc.F32, uc.F64], ids=lambda t: t.name)
def test_emulated_absargmax_equals_the_rule_on_planted_ties(dt):
    op = _lib.REDUCE_ABSARGMAX
    for inner, n, outer in SMALL:
        for seg in uc.SEGMENTS + (64,):
            _, S, seglen, depth, _ = uc.geometry(inner, n, outer, op, dt, seg)
            for centre in sorted({0, n // 2, n - 1, n + 5}):
                for phase in ((0, 3) if inner == 1 else (0,)):
                    x = uc.reduce_input(op, dt, n + 7 * seg + centre, outer, n, inner, centre, uc.boundaries(n, S, seglen, dt.itemsize, phase))
                    got, reached = uc.emulate(x, op, centre=centre, segments=seg, phase=phase)
                    assert reached <= depth, (inner, n, outer, seg, reached, depth)
                    for o in range(outer):
                        for i in range(inner):
                            assert tuple(got[o, i]) == ur.absargmax(x[o, :, i], centre), (inner, n, outer, seg, centre, phase, o, i)
    # NaN and +-Inf: a NaN raises the flag and does not compete; infinities tie like any other magnitude
    x = np.array([1.0, np.nan, -np.inf, 2.0, np.inf, np.nan, -np.inf], dt).reshape(1, 7, 1)
    for seg in (1, 2, 3, 7):
        for centre in (0, 3, 6):
            assert tuple(uc.emulate(x, op, centre=centre, segments=seg)[0][0, 0]) == ur.absargmax(x[0, :, 0], centre)
    assert tuple(uc.emulate(np.full((1, 5, 1), np.nan, dt), op, segments=2)[0][0, 0]) == (-1, 1)
    assert tuple(uc.emulate(np.zeros((1, 0, 1), dt), op)[0][0, 0]) == (-1, 0)


@pytest.mark.parametrize("op_dt", uc.OPS[:6], **_op_ids)
def test_emulated_sums_stay_within_the_depth_bound(op_dt):
    """Sums of non-negative terms, every addition one Float64 rounding: a result is within depth x 2^-53 of the exact sum of its terms (first order; the
    bound is taken with 1.01 for the higher orders).  SUMABS2 of Float64 / ComplexF64 adds the roundings inside a term: one (product) / three (two
    products and their sum, each 2^-53) -- counted as 3 more.  The SUMABS2_W reference rounds its terms as the library does, so only the additions differ."""
    op, dt = op_dt
    for inner, n, outer in SMALL:
        x = uc.reduce_input(op, dt, 11 + n + inner, outer, n, inner)
        for seg in uc.SEGMENTS + (64,):
            _, S, seglen, depth, _ = uc.geometry(inner, n, outer, op, dt, seg)
            for phase in ((0, 1) if inner == 1 else (0,)):
                got, reached = uc.emulate(x, op, step=uc.STEP, segments=seg, phase=phase)
                assert reached <= depth, (inner, n, outer, seg, reached, depth)
                bound = 1.01 * (depth + (3 if dt in (uc.F64, uc.C64) and op == _lib.REDUCE_SUMABS2 else 0)) * 2.0 ** -53
                for o in range(outer):
                    for i in range(inner):
                        if op == _lib.REDUCE_SUMABS2:
                            ref = [ur.sumabs2(x[o, :, i])]
                            mine = [got[o, i]]
                        else:
                            ref, mine = ur.weighted_sums(x[o, :, i], uc.STEP), got[o, i]
                        for g, r in zip(mine, ref):
                            assert abs(ur.LD(g) - r) <= bound * r, (inner, n, outer, seg, phase, o, i, float(g), float(r), depth)


def test_emulation_does_not_depend_on_the_cut_for_exact_data():
    """Integers: every product and partial sum is exact, so every cut and phase gives the same bits as the plain sum."""
    x = np.arange(1, 5001, dtype=np.float32).reshape(1, 5000, 1) % 97
    want = float(np.sum(x.astype(np.float64) ** 2))
    for seg in (0, 1, 2, 3, 7, 500):
        for phase in range(4):
            assert uc.emulate(x, _lib.REDUCE_SUMABS2, segments=seg, phase=phase)[0][0, 0] == want


# ---- the shift planner and a host walk of its schedules -----------------------------------------------------------------------------------------------
def test_shift_planner_routes_and_workspace():
    D, H, S = _lib.SHIFT_DISJOINT, _lib.SHIFT_HALO, _lib.SHIFT_STAGED
    for esize in (4, 8, 16):
        for tile in uc.TILES:
            for l, s in uc.shift_grid(tile):
                a = abs(s)
                for in_place in (False, True):
                    route, t, chunk, ntiles, ws = uc.shift_geometry(l, s, esize, in_place, tile)
                    what = (esize, tile, l, s, in_place, route, t, chunk, ntiles, ws)
                    overlap = in_place and 0 < 2 * a < l
                    assert t == max(tile, a) and chunk == max(16, t // 4) and ntiles == -(-l // t), what
                    assert route == ((S if ntiles < 256 else H) if overlap else D), what
                    assert ws == esize * {D: 0, H: ntiles * a, S: l - a}[route], what
                    for forced in (D, H, S):
                        if uc.route_allowed(l, s, in_place, forced):
                            r2, _, _, n2, ws2 = uc.shift_geometry(l, s, esize, in_place, tile, forced)
                            assert r2 == forced and ws2 == esize * {D: 0, H: n2 * a, S: l - a}[forced], what
                        else:
                            with pytest.raises(d.ArgumentError):
                                uc.shift_geometry(l, s, esize, in_place, tile, forced)
    # the library's own tile: 256 KiB of elements; HALO from 256 tiles on, STAGED below, DISJOINT when nothing overlaps
    assert uc.shift_geometry(2 ** 28, 100, 4, True) == (H, 65536, 1024, 4096, 4 * 4096 * 100)
    assert uc.shift_geometry(2 ** 28, 2 ** 26, 4, True)[:4] == (S, 2 ** 26, 1024, 4) and uc.shift_geometry(2 ** 28, 2 ** 27 + 1, 4, True)[0] == D
    assert uc.shift_geometry(2 ** 28, -100, 16, True)[:2] == (H, 16384) and uc.shift_geometry(2 ** 28, 100, 4, False)[0] == D
    assert uc.shift_geometry(1000, 3, 4, True)[0] == S and uc.shift_geometry(2 ** 33, 5, 8, True)[:2] == (H, 32768)
    with pytest.raises(d.DomainError):
        uc.shift_geometry(10, 11, 4, True)
    with pytest.raises(d.DomainError):
        uc.shift_geometry(10, -11, 4, False)
    for bad in ((10, 1, 3, True, 0, 0), (-1, 0, 4, True, 0, 0), (10, 1, 4, True, -1, 0), (10, 1, 4, True, 0, 4)):
        with pytest.raises(d.ArgumentError):
            uc.shift_geometry(*bad)


@pytest.mark.parametrize("esize", [4, 8, 16])
@pytest.mark.parametrize("tile", uc.TILES)
def test_shift_schedules_walked_on_the_host(tile, esize):
    """Every route over the issue's grid, the units of each launch in three orders: the result equals numpy's, and no word of the line is read after it was
    written, nor (HALO) by a workgroup that does not own it."""
    dt = uc.SHIFT_DTYPES[esize]
    for l, s in uc.shift_grid(tile):
        x = (np.arange(1, l + 1) * (1 + 2j if esize == 16 else 1)).astype(dt)
        want = ur.shiftsignal(x, s)
        for in_place in (True, False):
            for route in uc.ROUTES:
                if not uc.route_allowed(l, s, in_place, route):
                    continue
                for order in (0, 1, 2):
                    got, bad = uc.shift_emulate(x, s, tile, route, order, in_place)
                    assert bad == 0 and np.array_equal(got, want), (esize, tile, l, s, in_place, uc.ROUTE_NAME[route], order, bad)


# ---- argument and exception checks, before any device work ------------------------------------------------------------------------------------------
def test_argument_errors_come_before_device_work():
    x = np.ones(8, np.float32)
    with pytest.raises(d.UnsupportedError):
        d.rms(np.ones((2, 3)), dims=(0, 1))
    with pytest.raises(d.ArgumentError):
        d.rms(np.ones((2, 3)), dims=2)
    with pytest.raises(TypeError):
        d.rmsfft(x)                                                # real input: no method in the reference
    with pytest.raises(TypeError):
        d.meanfreq(np.ones((4, 2)))
    with pytest.raises(TypeError):
        d.meanfreq(np.ones(4, np.complex64))
    with pytest.raises(d.ArgumentError):
        d.meanfreq(np.ones(0))
    with pytest.raises(TypeError):
        d.finddelay(np.ones((2, 2)), x)
    with pytest.raises(TypeError):
        d.finddelay(x, np.ones(3, np.complex128))
    for a, b in ((np.ones(0), x), (x, np.ones(0))):
        with pytest.raises(d.ArgumentError):
            d.finddelay(a, b)
    for fn in (d.shiftsignal, d.shiftsignal_):
        with pytest.raises(d.DomainError):
            fn(x.copy(), 9)
        with pytest.raises(d.DomainError):
            fn(x.copy(), -9)
        with pytest.raises(TypeError):
            fn(x.copy(), 1.5)
        with pytest.raises(TypeError):
            fn(np.ones((2, 2)), 1)
        with pytest.raises(d.UnsupportedError):
            fn(np.ones(4, np.int16), 1)
    # s == 0 needs no device at all
    y = x.copy()
    assert d.shiftsignal_(y, 0) is y and np.array_equal(d.shiftsignal(x, 0), x) and d.shiftsignal(x, 0) is not x
    if _lib.device_count() == 0:
        for call in (lambda: d.rms(x), lambda: d.rmsfft(x.astype(np.complex64)), lambda: d.meanfreq(x), lambda: d.finddelay(x, x),
                     lambda: d.shiftsignal(x, 1), lambda: d.shiftsignal_(x.copy(), 1), lambda: d.alignsignals(x, x), lambda: d.alignsignals_(x.copy(), x)):
            with pytest.raises(d.DeviceError):
                call()


def test_product_does_not_import_the_test_references():
    import os
    import re
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert not re.search(r"^\s*(from|import)\s+(util_ref|util_cases)", open(os.path.join(pkg, f)).read(), re.M), f
