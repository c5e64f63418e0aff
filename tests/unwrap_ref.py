"""numpy restatement of unwrap along one dimension (src/unwrap.jl:17-34, the `dims::Integer` form).

unwrap_serial is the reference's recurrence, element by element, every operation rounded in the array's element type:

    unwrap_kernel(range) = (x, y) -> y - round((y - x) / range) * range                                   (src/unwrap.jl:34)
    accumulate!(unwrap_kernel(range), y, m; dims)                                                        (src/unwrap.jl:25)

unwrap_scan is the form the library evaluates: d_i = rint((m[i] - m[i-1]) / range), K = cumsum(d) in int64, y = m - T(K) * range.  The two are
bit-identical whenever no (m[i] - m[i-1]) / range lies near a rounding tie; tie_margin measures how far the nearest one is."""
import numpy as np


def default_range(dtype):
    """2T(pi) (src/unwrap.jl:17): pi rounded to T, doubled in T."""
    T = np.dtype(dtype).type
    return T(2) * T(np.pi)


def unwrap_serial(m, axis=0, range=None):
    m = np.asarray(m)
    T = m.dtype.type
    r = default_range(m.dtype) if range is None else T(range)
    a = np.moveaxis(m, axis, 0)
    y = np.empty_like(a)
    if a.shape[0] == 0:
        return np.moveaxis(y, 0, axis)
    with np.errstate(all="ignore"):
        y[0] = a[0]
        for i in np.arange(1, a.shape[0]):
            q = ((a[i] - y[i - 1]) / r).astype(m.dtype)          # every step an array operation in T: one rounding each
            y[i] = a[i] - (np.rint(q) * r).astype(m.dtype)       # np.rint: ties to even, like Julia's round
    return np.ascontiguousarray(np.moveaxis(y, 0, axis))


def _increments(m, axis, r):
    a = np.moveaxis(np.asarray(m), axis, 0)
    with np.errstate(all="ignore"):
        return (np.diff(a, axis=0) / r).astype(a.dtype)


def unwrap_scan(m, axis=0, range=None):
    """Finite inputs only (the non-finite rules are a property of the recurrence; tests take them from unwrap_serial)."""
    m = np.asarray(m)
    T = m.dtype.type
    r = default_range(m.dtype) if range is None else T(range)
    a = np.moveaxis(m, axis, 0)
    if a.shape[0] == 0:
        return m.copy()
    K = np.zeros(a.shape, dtype=np.int64)
    K[1:] = np.cumsum(np.rint(_increments(m, axis, r)).astype(np.int64), axis=0)
    y = a - (K.astype(m.dtype) * r).astype(m.dtype)
    return np.ascontiguousarray(np.moveaxis(y, 0, axis))


def tie_margin(m, axis=0, range=None):
    """min_i (0.5 - |q_i - rint(q_i)|) with q_i = (m[i] - m[i-1]) / range in Float64; 0.5 for a line of one sample."""
    m = np.asarray(m, dtype=np.float64)
    r = float(default_range(np.float64) if range is None else range)
    q = _increments(m, axis, r)
    return 0.5 if q.size == 0 else float(np.min(0.5 - np.abs(q - np.rint(q))))


def max_count(m, axis=0, range=None):
    """max |K| of the scan form."""
    m = np.asarray(m)
    r = default_range(m.dtype) if range is None else m.dtype.type(range)
    d = np.rint(_increments(m, axis, r)).astype(np.int64)
    return 0 if d.size == 0 else int(np.max(np.abs(np.cumsum(d, axis=0))))


def equal(a, b):
    """Bit for bit, except that signed zeros compare equal and NaN equals NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
