"""Guard bands: the layout and the checks behind the contract of INTEGRATION.md ("What a call touches") -- a call reads nothing outside [0, n) of each
column it is given and writes nothing outside [0, nout) of each output column, whatever the leading dimensions and the element alignment.

One flat allocation holds  [front guard | base_off | column 0 | padding | column 1 | padding | ... | back guard]:  `ncols` columns of `n` elements `ld`
apart (the padding of the last column included), `front` elements in front -- rounded up to whole 128-element runs, so that with an allocation on a 128-byte
line `base_off` is the distance of column 0 from such a line, in ELEMENTS: all the C ABI promises -- and `back` elements behind.

Everything is written and compared as integers (one word per real part): the input poison is a quiet NaN with the payload 0xA5A5.., the output fill a quiet
NaN with the payload 0x5A5A.. -- in both parts of a complex element.  Input buffers carry the poison everywhere but in the column bodies; a kernel that uses
one sample outside a column turns a transform block or a tap window into NaN, which check_output reports (and any comparison with an oracle fails on).
Output buffers carry the fill everywhere, bodies included: check_output finds every word outside the bodies that changed and every word inside that did not.

Plain numpy; the torch part (to_device / from_device / ptr) is three thin functions the GPU tests use.  tests/test_guard_bands_cpu.py runs the checks
against planted defects."""
from collections import namedtuple

import numpy as np

MIN_GUARD = 4096            # elements; the callers pass max(MIN_GUARD, one executed transform length)
LINE_ELEMS = 128            # the front guard is a whole number of these: a multiple of the 128-byte line for every element size

_WORD = {4: np.uint32, 8: np.uint64}
POISON = {4: 0x7FC0A5A5, 8: 0x7FF80000A5A5A5A5}      # input: outside the columns
FILL = {4: 0x7FC05A5A, 8: 0x7FF800005A5A5A5A}        # output: everywhere before the call

Layout = namedtuple("Layout", "n ncols ld front back base_off dtype col0 total starts")


class GuardError(AssertionError):
    """kind: 'stray' (a word outside the written ranges changed), 'unwritten' (an output still holds the fill) or 'nan' (an output is NaN: a poisoned sample
    was used).  column / index: the nearest column and the element index relative to its first element (negative: in front of it); distance: for a stray
    write how many elements outside the nearest written range, else how far inside from the nearest end."""

    def __init__(self, kind, column, index, distance, count, what=""):
        self.kind, self.column, self.index, self.distance, self.count = kind, int(column), int(index), int(distance), int(count)
        where = {"stray": "outside the written range by", "unwritten": "inside, from the nearest edge", "nan": "inside, from the nearest edge"}[kind]
        super().__init__(f"{what + ': ' if what else ''}{kind}: column {self.column}, element {self.index} ({where} {self.distance}); {self.count} such element(s)")


def layout(n, ncols, ld, front, back, base_off, dtype=np.float32):
    """Element offsets inside one flat allocation; col0 is the offset of column 0, starts[c] = col0 + c ld that of column c."""
    dtype = np.dtype(dtype)
    if n < 0 or ncols < 1 or ld < max(n, 1) or base_off < 0 or front < MIN_GUARD or back < MIN_GUARD:
        raise ValueError(f"layout({n}, {ncols}, {ld}, {front}, {back}, {base_off}): ld >= n and guards of at least {MIN_GUARD} elements")
    front = -(-front // LINE_ELEMS) * LINE_ELEMS
    col0 = front + base_off
    return Layout(n, ncols, ld, front, back, base_off, dtype, col0, col0 + ncols * ld + back, tuple(col0 + c * ld for c in range(ncols)))


def layout_nested(n, ncols, ld, nouter, outer_stride, front, back, base_off, dtype=np.float32):
    """`nouter` matrices of `ncols` columns ld apart, the matrices outer_stride >= ncols ld apart (the STFT's channels): one Layout of nouter x ncols
    columns, matrix m's column k being column m ncols + k.  Everything between the columns -- the padding of each and the gap behind each matrix -- is guard."""
    if nouter < 1 or outer_stride < ncols * ld:
        raise ValueError(f"layout_nested: outer stride {outer_stride} < {ncols} columns of {ld}")
    one = layout(n, ncols, ld, front, back, base_off, dtype)
    starts = tuple(one.col0 + m * outer_stride + c * ld for m in range(nouter) for c in range(ncols))
    return one._replace(ncols=nouter * ncols, total=one.col0 + nouter * outer_stride + back, starts=starts)


def _parts(dtype):
    """(words per element, word type)"""
    dtype = np.dtype(dtype)
    return (2, _WORD[dtype.itemsize // 2]) if dtype.kind == "c" else (1, _WORD[dtype.itemsize])


def _pattern(table, dtype):
    k, w = _parts(dtype)
    return w(table[np.dtype(w).itemsize])


def poison_word(dtype):
    return _pattern(POISON, dtype)


def fill_word(dtype):
    return _pattern(FILL, dtype)


def words(lay):
    """(words per element, word dtype) of a layout's buffers."""
    return _parts(lay.dtype)


def new_input(lay, cols):
    """The words of an input buffer: poison everywhere, cols (ncols, n) in the bodies."""
    k, w = _parts(lay.dtype)
    buf = np.full(lay.total * k, poison_word(lay.dtype), dtype=w)
    cols = np.ascontiguousarray(cols, dtype=lay.dtype).reshape(lay.ncols, lay.n)
    el = buf.view(lay.dtype)
    for c in range(lay.ncols):
        el[lay.starts[c]:lay.starts[c] + lay.n] = cols[c]
    return buf


def new_output(lay):
    """The words of an output buffer: the fill everywhere, bodies included."""
    k, w = _parts(lay.dtype)
    return np.full(lay.total * k, fill_word(lay.dtype), dtype=w)


def columns(buf, lay, n=None):
    """(ncols, n) copy of the column bodies (the first n elements of each) as elements."""
    n = lay.n if n is None else n
    el = np.asarray(buf).view(lay.dtype)
    return np.stack([el[lay.starts[c]:lay.starts[c] + n] for c in range(lay.ncols)])


def _locate(lay, pos, nw):
    """Flat element offset -> (column, index relative to the column, elements outside the nearest written range [0, nw[c]) )."""
    c = max(int(np.searchsorted(lay.starts, pos, side="right")) - 1, 0)
    i = pos - lay.starts[c]
    best = (c, i, -i if i < 0 else i - nw[c] + 1)
    if i >= nw[c] and c + 1 < lay.ncols and lay.starts[c + 1] - pos < best[2]:      # nearer to the start of the next column than to the end of this one
        best = (c + 1, pos - lay.starts[c + 1], lay.starts[c + 1] - pos)
    return best


def check_output(buf_after, lay, n_written, what=""):
    """buf_after: the words of a buffer made by new_output after the call.  n_written: elements the call had to write at the start of every column (one
    number, or one per column).  Raises GuardError at the first offending element: every word outside [0, n_written) of every column equals the fill, every
    element inside no longer does and is not NaN (in either part)."""
    k, w = _parts(lay.dtype)
    buf = np.asarray(buf_after)
    assert buf.dtype == np.dtype(w) and buf.shape == (lay.total * k,), (buf.dtype, buf.shape)
    nw = [int(n_written)] * lay.ncols if np.ndim(n_written) == 0 else [int(v) for v in n_written]
    assert len(nw) == lay.ncols and all(0 <= v <= lay.n for v in nw), nw
    inside = np.zeros(lay.total, dtype=bool)
    for c in range(lay.ncols):
        inside[lay.starts[c]:lay.starts[c] + nw[c]] = True
    is_fill = (buf.reshape(lay.total, k) == fill_word(lay.dtype))
    stray = np.flatnonzero(~inside & ~is_fill.all(axis=1))
    if stray.size:
        # report the stray element nearest to a written range: the most telling one when a whole run was overwritten
        c, i, dist = min((_locate(lay, int(p), nw) for p in (stray if stray.size <= 4096 else np.concatenate([stray[:2048], stray[-2048:]]))), key=lambda t: t[2])
        raise GuardError("stray", c, i, dist, stray.size, what)
    unwritten = np.flatnonzero(inside & is_fill.any(axis=1))
    vals = buf.view(np.dtype(lay.dtype).type(0).real.dtype).reshape(lay.total, k)
    nan = np.flatnonzero(inside & np.isnan(vals).any(axis=1))
    for kind, bad in (("unwritten", unwritten), ("nan", nan)):
        if bad.size:
            c, i, _ = _locate(lay, int(bad[0]), nw)
            raise GuardError(kind, c, i, min(i, nw[c] - 1 - i), bad.size, what)


# ---- the thin torch part ------------------------------------------------------------------------------------------------------------------------------
def to_device(buf):
    """The words on the device, as an integer tensor (bit patterns travel untouched)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(buf).view({4: np.int32, 8: np.int64}[buf.dtype.itemsize])).cuda()


def from_device(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ptr(t, lay, column=0, index=0):
    """Device address of element `index` of `column`.  The allocation must start on a 128-byte line (the allocator's do), so that base_off means what it says."""
    assert t.data_ptr() % 128 == 0, "allocation not on a 128-byte line"
    return t.data_ptr() + (lay.starts[column] + index) * np.dtype(lay.dtype).itemsize
