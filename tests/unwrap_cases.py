"""Inputs of the unwrap tests.  A case is an array of shape (outer, len, inner), C-contiguous -- element (i, j, o) of the library's (inner, len, outer)
description at i + inner (j + len o) -- unwrapped along axis 1, with its range.

The exactness condition is a condition on the INPUTS: a case used for a bit-exact comparison satisfies

    tie_margin >= 0.01 + 4 eps(T) max|K|

(no increment (m[i] - m[i-1]) / range near a rounding tie, with room for the rounding of K range), and make() asserts it.  The margins hold by construction:
wrapped random walks with steps uniform in +-2.8 rad have margin >= (pi - 2.8) / 2 pi = 0.054; wrapped ramps of 2.0 +- 0.2 rad per step 0.118 (K to 6.4e4
at 2e5 samples); i mod 10 with range 10 has 0.4; a walk of steps within +-0.5 rad with whole periods planted on it 0.42.  Steps that reach pi are not used:
a 0.9 pi +- 0.2 ramp has margin 5e-7 and the Float32 serial form itself departs by a period."""
from collections import namedtuple

import numpy as np

import unwrap_ref as ur

Case = namedtuple("Case", "name m range")          # range None: 2T(pi)
TWO_PI = 2 * np.pi


def make(name, m, range=None, exact=True):
    m = np.ascontiguousarray(m)
    assert m.ndim == 3 and m.dtype in (np.float32, np.float64), (name, m.shape, m.dtype)
    if exact:
        # non-finite samples are placed by hand; the condition is about the increments between finite samples (the others decide no rounding)
        good = np.isfinite(m)
        held = np.where(good, m, 0.0).astype(np.float64)
        r = float(ur.default_range(np.float64) if range is None else range)
        q = (np.diff(held, axis=1) / r)[good[:, 1:] & good[:, :-1]]
        margin = 0.5 if q.size == 0 else float(np.min(0.5 - np.abs(q - np.rint(q))))
        if good.all():
            assert margin == ur.tie_margin(m, 1, range)
        kmax = ur.max_count(held.astype(m.dtype), 1, range)
        need = 0.01 + 4 * float(np.finfo(m.dtype).eps) * kmax
        assert margin >= need, f"case {name}: tie margin {margin:.4g} < {need:.4g} (max|K| {kmax})"
    return Case(name, m, range)


def wrap(u, period=TWO_PI):
    return u - period * np.rint(u / period)


def walk(seed, outer, n, inner, dtype, step=2.8):
    """Wrapped random walk, a different seed (so different data) in every line."""
    rng = np.random.default_rng(seed)
    u = np.cumsum(rng.uniform(-step, step, (outer, n, inner)), axis=1)
    return wrap(u).astype(dtype)


def ramp(seed, n, dtype, slope):
    rng = np.random.default_rng(seed)
    u = np.cumsum(slope + rng.uniform(-0.2, 0.2, n))
    return wrap(u).astype(dtype).reshape(1, n, 1)


def planted(seed, outer, n, inner, dtype, positions, period=None):
    """A walk of small steps (no wrap of its own) with whole periods planted from each position on: the increment across position - 1 -> position is
    +-1 .. 3 periods, in every line (each line with its own small walk)."""
    rng = np.random.default_rng(seed)
    T = np.dtype(dtype).type
    r = float(ur.default_range(dtype) if period is None else T(period))
    u = np.cumsum(rng.uniform(-0.5, 0.5, (outer, n, inner)) * (r / TWO_PI), axis=1)
    k = np.zeros(n)
    for c, p in enumerate(sorted({int(p) for p in positions if 0 < p < n})):
        k[p:] += (1 + c % 3) * (1 if c % 2 == 0 else -1)
    k -= np.rint(np.mean(k))                                # keep |m| small: the planted periods are increments, not a drift
    return (u + r * k[None, :, None]).astype(dtype)


def lattice(seed, shape, dtype, steps=(2.0, -1.7, 0.9), period=TWO_PI):
    """Wrapped phase of a plane wave plus noise: along axis a the increments are steps[a] +- 0.2 rad (in units of period / 2 pi) plus whole periods, so
    the condition holds along EVERY axis (margin >= (pi - 2.2) / 2 pi = 0.15)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.1, 0.1, shape)
    for a, n in enumerate(shape):
        u = u + steps[a] * np.arange(n).reshape([-1 if b == a else 1 for b in range(len(shape))])
    return wrap(u * (period / TWO_PI), period).astype(dtype)


def require_exact(m, axis, range=None):
    """The exactness condition for an array unwrapped along `axis`."""
    margin, need = ur.tie_margin(m, axis, range), 0.01 + 4 * float(np.finfo(m.dtype).eps) * ur.max_count(m, axis, range)
    assert margin >= need, f"tie margin {margin:.4g} < {need:.4g} along axis {axis}"


def nonfinite_cases():
    """(case, expected) pairs the issue states, and the rules on several lines."""
    inf, nan = np.inf, np.nan
    out = []
    # exact=False: a non-finite first sample decides the whole line, no increment behind it is ever rounded into the result
    for dt in (np.float32, np.float64):
        out.append(make(f"inf_inside_{np.dtype(dt).name}", np.array([0.1, 3, -3, inf, 0.2, 0.3], dt).reshape(1, 6, 1)))
        out.append(make(f"inf_first_{np.dtype(dt).name}", np.array([inf, 3, -3, 0.2], dt).reshape(1, 4, 1), exact=False))
        out.append(make(f"ninf_first_{np.dtype(dt).name}", np.array([-inf, 3, -3, 0.2, 7.0], dt).reshape(1, 5, 1), exact=False))
        out.append(make(f"nan_first_{np.dtype(dt).name}", np.array([nan, 3, -3, 0.2], dt).reshape(1, 4, 1), exact=False))
        out.append(make(f"inf_then_inf_{np.dtype(dt).name}", np.array([inf, 3, inf, 0.2], dt).reshape(1, 4, 1), exact=False))
        for inner in (1, 3):
            for bad in (nan, inf, -inf):
                m = walk(77 + inner, 3 if inner == 1 else 1, 30, inner, dt)
                line = 1
                if inner == 1:
                    m[line, 14, 0] = bad                    # the second of three segments of ten
                else:
                    m[0, 14, line] = bad
                out.append(make(f"{bad}_line1_inner{inner}_{np.dtype(dt).name}", m))
    return out


def cpu_cases():
    out = []
    for dt in (np.float32, np.float64):
        nm = np.dtype(dt).name
        for n in (1, 2, 3, 7, 64, 65, 1000):
            out.append(make(f"walk_{n}_{nm}", walk(n, 2, n, 1, dt)))
        out.append(make(f"walk_10007_{nm}", walk(5, 1, 10007, 1, dt)))
        for inner, n, outer in ((2, 17, 1), (3, 1000, 3), (65, 17, 2), (64, 2, 1), (5, 1, 2)):
            out.append(make(f"walk_strided_{inner}_{n}_{outer}_{nm}", walk(inner * 131 + n, outer, n, inner, dt)))
        out.append(make(f"ramp_up_{nm}", ramp(1, 20000, dt, 2.0)))
        out.append(make(f"ramp_down_{nm}", ramp(2, 20000, dt, -2.0)))
        out.append(make(f"mod10_{nm}", (np.arange(1, 101) % 10).astype(dt).reshape(1, 100, 1), 10))
        out.append(make(f"planted_{nm}", planted(3, 2, 300, 1, dt, range(10, 300, 7))))
        out.append(make(f"planted_range2_{nm}", planted(4, 1, 300, 3, dt, range(5, 300, 11), 2), 2))
        out.append(make(f"signed_zero_{nm}", np.array([0.5, -0.0, 0.0, -0.0], dt).reshape(1, 4, 1)))
    return out + nonfinite_cases()
