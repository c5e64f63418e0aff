"""Inputs and thin ctypes helpers of the util tests (rms, rmsfft, meanfreq, finddelay, shiftsignal, alignsignals; mdsp_reduce_* and mdsp_shift_*).

A reduce case is an array of shape (outer, len, inner), C-contiguous -- element (i, j, o) of the library's (inner, len, outer) description at
i + inner (j + len o) -- reduced along axis 1; line i + inner o of the result is [o, i]."""
import ctypes as C

import numpy as np

from dsp_jl_amd import _lib

LENS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4099)
BIG = 2 ** 24 + 3                       # used once per operator: many segments of the automatic cut
INNERS, OUTERS = (1, 2, 3, 64, 65), (1, 2, 5)
SEGMENTS = (0, 1, 2, 3, 7)              # 0: the library's own choice
OFFSETS = (0, 1, 2, 3)                  # elements between a 128-byte line and the array

F32, F64, C32, C64 = (np.dtype(t) for t in (np.float32, np.float64, np.complex64, np.complex128))
CODE = {F32: _lib.F32, F64: _lib.F64, C32: _lib.C32, C64: _lib.C64}
OPS = [(_lib.REDUCE_SUMABS2, F32), (_lib.REDUCE_SUMABS2, F64), (_lib.REDUCE_SUMABS2, C32), (_lib.REDUCE_SUMABS2, C64),
       (_lib.REDUCE_SUMABS2_W, C32), (_lib.REDUCE_SUMABS2_W, C64), (_lib.REDUCE_ABSARGMAX, F32), (_lib.REDUCE_ABSARGMAX, F64)]
OP_NAME = {_lib.REDUCE_SUMABS2: "sumabs2", _lib.REDUCE_SUMABS2_W: "sumabs2_w", _lib.REDUCE_ABSARGMAX: "absargmax"}
ACC_BYTES = {_lib.REDUCE_SUMABS2: 8, _lib.REDUCE_SUMABS2_W: 16, _lib.REDUCE_ABSARGMAX: 24}
OUT_WORDS = {_lib.REDUCE_SUMABS2: 1, _lib.REDUCE_SUMABS2_W: 2, _lib.REDUCE_ABSARGMAX: 2}
STEP = 2 * np.pi / 1000                 # the `step` of the SUMABS2_W cases


def op_id(p):
    return f"{OP_NAME[p[0]]}_{p[1].name}"


def gaussian(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    return rng.standard_normal(shape).astype(dtype)


def boundaries(n, S, seglen, itemsize, phase=0):
    """Where the reduction changes hands along a line: segment starts, and inside each segment the 64-lane tile and some lane boundaries of the
    contiguous route (counted from the 16-byte boundary at or below the segment start)."""
    V = 16 // itemsize
    pos = set()
    for s in range(S):
        j0 = s * seglen
        a = (phase + j0) % V
        pos.add(j0)
        pos.update(range(j0 - a, min(n, j0 + seglen), 64 * V))
        pos.update(range(j0 - a + V, min(n, j0 + seglen), 16 * V))
    return sorted(p for p in pos if 0 < p < n)


def planted_ties(seed, n, centre, where, dtype):
    """A line of small noise (|v| < 0.5) with the magnitude 3 planted, with both signs: on both sides of every position of `where`, and in pairs at equal and
    unequal distances from `centre`.  Every planted sample ties for the maximum, so the result is decided by the distance and index rules alone."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, n)
    spots = set()
    for b in where:
        spots.update((b - 1, b))
    for k in (1, 2, 5, 40, 300):
        spots.update((centre - k, centre + k, centre + k + 1))
    spots = sorted(p for p in spots if 0 <= p < n)
    drop = rng.random(len(spots)) < 0.5          # thin them out, so that the winner is not always right next to the centre
    for p, gone in zip(spots, drop):
        if not gone:
            x[p] = 3.0 if rng.random() < 0.5 else -3.0
    return x.astype(dtype)


def reduce_input(op, dtype, seed, outer, n, inner, centre=0, where=()):
    if op == _lib.REDUCE_ABSARGMAX:
        return np.stack([np.stack([planted_ties(seed + 31 * o + i, n, centre, where, dtype) for i in range(inner)], axis=1) for o in range(outer)])
    return gaussian(seed, (outer, n, inner), dtype)


def geometry(inner, n, outer, op, dtype, segments=0):
    route, S, seglen, depth, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_reduce_geometry_for(inner, n, outer, op, CODE[np.dtype(dtype)], segments, C.byref(route), C.byref(S), C.byref(seglen),
                                                   C.byref(depth), C.byref(ws)))
    return route.value, S.value, seglen.value, depth.value, ws.value


def emulate(x, op, step=0.0, centre=0, segments=0, phase=0):
    """mdsp_reduce_emulate on an (outer, len, inner) array -> (result of shape (outer, inner[, 2]), depth reached)."""
    x = np.ascontiguousarray(x)
    outer, n, inner = x.shape
    out = np.full((outer, inner, OUT_WORDS[op]), -7, dtype=np.int64 if op == _lib.REDUCE_ABSARGMAX else np.float64)
    reached = C.c_int64()
    _lib.check(_lib.lib().mdsp_reduce_emulate(x.ctypes.data, out.ctypes.data, inner, n, outer, op, CODE[x.dtype], float(step), int(centre), int(segments),
                                              int(phase), C.byref(reached)))
    return (out[..., 0] if OUT_WORDS[op] == 1 else out), reached.value


# ---- shift
ROUTES = (_lib.SHIFT_AUTO, _lib.SHIFT_DISJOINT, _lib.SHIFT_HALO, _lib.SHIFT_STAGED)
ROUTE_NAME = {_lib.SHIFT_AUTO: "auto", _lib.SHIFT_DISJOINT: "disjoint", _lib.SHIFT_HALO: "halo", _lib.SHIFT_STAGED: "staged"}
TILES = (64, 256)
SHIFT_DTYPES = {4: np.float32, 8: np.float64, 16: np.complex128}


def shift_geometry(l, s, esize, in_place, tile=0, route=_lib.SHIFT_AUTO):
    r, t, c, n, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_shift_geometry_for(l, s, esize, int(in_place), tile, route, C.byref(r), C.byref(t), C.byref(c), C.byref(n), C.byref(ws)))
    return r.value, t.value, c.value, n.value, ws.value


def shift_grid(tile):
    """(l, s) of the issue's grid for a forced tile: the chunk is what the plan reports for that tile with a small shift."""
    out = []
    for l in (1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 3):
        chunk = shift_geometry(l, 1 if l > 1 else 0, 4, True, tile)[2]
        mags = {1, chunk - 1, chunk, chunk + 1, tile - 1, tile, tile + 1, l // 2 - 1, l // 2, l // 2 + 1, l - 1, l}
        for m in sorted(m for m in mags if 1 <= m <= l):
            out += [(l, m), (l, -m)]
        out.append((l, 0))
    return out


def route_allowed(l, s, in_place, route):
    """What the planner accepts (csrc/shift_plan.h): DISJOINT in place needs 2 |s| >= l (or s == 0), HALO is in place with s != 0."""
    if route == _lib.SHIFT_DISJOINT:
        return not (in_place and s != 0 and 2 * abs(s) < l)
    if route == _lib.SHIFT_HALO:
        return in_place and s != 0
    return True


def shift_emulate(x, s, tile=0, route=_lib.SHIFT_AUTO, order=0, in_place=True):
    """mdsp_shift_emulate -> (result, violations)."""
    src = np.ascontiguousarray(x).copy()
    dst = src if in_place else np.full_like(src, 7)
    bad = C.c_int64(-1)
    _lib.check(_lib.lib().mdsp_shift_emulate(src.ctypes.data, dst.ctypes.data, len(src), s, src.dtype.itemsize, tile, route, order, C.byref(bad)))
    return dst, bad.value


def delayed_pair(n, d, dtype, seed=0):
    """A Gaussian x and y with x = y delayed by d (finddelay(x, y) == d), plus 0.1 sigma noise on the copy."""
    rng = np.random.default_rng(seed + n)
    y = rng.standard_normal(n)
    x = np.zeros(n)
    if d >= 0:
        x[d:] = y[:n - d]
    else:
        x[:n + d] = y[-d:]
    x += 0.1 * rng.standard_normal(n)
    return x.astype(dtype), y.astype(dtype)
