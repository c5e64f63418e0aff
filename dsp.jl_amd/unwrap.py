"""``unwrap`` / ``unwrap!`` along one dimension (src/unwrap.jl:17-34, the ``dims::Integer`` form) on the device (``mdsp_unwrap_*``).

``unwrap(m; dims, range)`` -> ``unwrap(m, dims=..., range=...)``, ``unwrap!(y, m)`` / ``unwrap!(m)`` -> ``unwrap_(y, m)`` / ``unwrap_(m)``.  ``dims`` is a
Python axis (0-based, negative from the end), as in ``resample(...; dims)``.  numpy in, numpy out; a device tensor in, a device tensor out with no copy
through the host.  The array is handed to the library as it lies in memory -- ``(inner, len, outer)`` with ``inner`` the product of the axes after
``dims`` of a C-contiguous array, before it of a column-major one -- so no axis needs a transpose; any other layout is made contiguous first.  There is no CPU fallback.
"""
from __future__ import annotations

import builtins
import ctypes as C
import numbers

import numpy as np

from . import _dev, _lib, _plancache
from ._lib import ArgumentError, UnsupportedError

_REAL = (np.dtype(np.float32), np.dtype(np.float64))


class UnwrapPlan:
    """``mdsp_unwrap_plan``: ``route`` (``_lib.UNWRAP_CONTIGUOUS`` / ``_STRIDED``), ``segments``, ``seglen``, ``workspace_bytes``.  ``segments`` = 0 lets
    the library cut the lines; a positive value forces the cut (tests, tools/unwrap_bench.py)."""

    def __init__(self, inner, length, outer, dtype, range, segments=0):
        self._h = C.c_void_p()
        self.inner, self.len, self.outer, self.dtype = int(inner), int(length), int(outer), np.dtype(dtype)
        _lib.check(_lib.lib().mdsp_unwrap_plan_create(C.byref(self._h), self.inner, self.len, self.outer, _dev.md_dtype(self.dtype), float(range), int(segments)))
        route, S, seglen, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mdsp_unwrap_plan_info(self._h, C.byref(route), C.byref(S), C.byref(seglen), C.byref(ws)))
        self.route, self.segments, self.seglen, self.workspace_bytes = route.value, S.value, seglen.value, ws.value

    def exec(self, in_ptr: int, out_ptr: int, stream: int | None = None):
        _lib.check(_lib.lib().mdsp_unwrap_exec(self._h, in_ptr, out_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_unwrap_plan_destroy(self._h)
        except Exception:
            pass


def unwrap_geometry(inner: int, length: int, outer: int, dtype, segments: int = 0):
    """(route, segments, seglen, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    route, S, seglen, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_unwrap_geometry_for(int(inner), int(length), int(outer), _dev.md_dtype(dtype), int(segments),
                                                   C.byref(route), C.byref(S), C.byref(seglen), C.byref(ws)))
    return route.value, S.value, seglen.value, ws.value


def _axis(nd: int, dims):
    """The reference's dispatch on ``dims`` (src/unwrap.jl:18-30)."""
    if dims is None:
        if nd != 1:
            raise ArgumentError("`unwrap!`: required keyword parameter dims missing")            # :19-21
        return 0
    if isinstance(dims, numbers.Integral) and not isinstance(dims, bool):
        if not -nd <= dims < nd:
            raise ArgumentError(f"`unwrap!`: Invalid dims specified: {dims}")
        return int(dims) % nd
    if isinstance(dims, (range, tuple, list)) and all(isinstance(k, numbers.Integral) and not isinstance(k, bool) for k in dims) \
            and list(dims) == list(range(nd)):
        raise UnsupportedError("unwrap over all dimensions (dims = 1:N, the N-d algorithm of Herraez et al., src/unwrap.jl:70-) is not accelerated: "
                               "use DSP.jl's CPU path")                                            # :26-27
    raise ArgumentError(f"`unwrap!`: Invalid dims specified: {dims}")                           # :28-29


def _checked(x, what):
    dt = _dev.np_dtype_of(x)
    if dt not in _REAL:
        raise TypeError(f"unwrap: {what} must be a Float32 or Float64 array, got {dt}")
    return dt


def unwrap_(y, m=None, dims=None, range=None):
    """``unwrap!(y, m; dims, range)``; ``unwrap!(m; ...)`` with one array.  Returns ``y`` itself."""
    if m is None:
        m = y
    if not hasattr(y, "shape") or not hasattr(m, "shape"):
        raise TypeError("unwrap!: arrays expected")
    dt = _checked(m, "m")
    if m is not y:
        if _checked(y, "y") != dt or tuple(y.shape) != tuple(m.shape):
            raise ArgumentError("unwrap!: y and m must have the same shape and element type")
    shape = tuple(int(k) for k in m.shape)
    axis = _axis(len(shape), dims)
    r = float(dt.type(2) * dt.type(np.pi)) if range is None else float(dt.type(range))          # 2T(pi), evaluated in T (:17)
    if not np.isfinite(r) or r == 0.0:
        raise ArgumentError(f"unwrap: range must be finite and nonzero, got {range}")
    _lib.require_device()
    if 0 in shape:
        return y                                         # nothing to do, and no launch
    nd = len(shape)
    src = _dev.as_device(m, dt)
    # a column-major tensor (what stft returns: a permuted view of channel-major memory) is a C-ordered array of the reversed shape: no copy either
    rev = nd > 1 and not src.is_contiguous() and src.permute(*reversed(builtins.range(nd))).is_contiguous()

    def view(t):
        return t.permute(*reversed(builtins.range(nd))) if rev else t

    srcv = view(src).contiguous()                        # a copy only for layouts that are neither
    vshape, vaxis = tuple(srcv.shape), (nd - 1 - axis if rev else axis)
    length = vshape[vaxis]
    outer = int(np.prod(vshape[:vaxis], dtype=np.int64))
    inner = int(np.prod(vshape[vaxis + 1:], dtype=np.int64))
    ours = not (_dev.is_device_array(m) and srcv.data_ptr() == m.data_ptr())
    if _dev.is_device_array(y) and y.device == srcv.device and view(y).is_contiguous():
        dst = view(y)                                    # unwrap!(m) on a device tensor: dst is src, in place
    elif ours:
        dst = srcv                                       # a device copy of our own: unwrap it in place
    else:
        dst = _dev.torch.empty_like(srcv)
    plan = _plancache.plans.get(("unwrap", _plancache.ctx_key(), inner, length, outer, dt.str, r),
                                lambda: UnwrapPlan(inner, length, outer, dt, r))
    plan.exec(_dev.ptr(srcv), _dev.ptr(dst))
    if _dev.is_device_array(y) and dst.data_ptr() == y.data_ptr():
        return y
    if isinstance(y, np.ndarray):
        y[...] = view(dst).cpu().numpy()
    else:
        y.copy_(view(dst))
    return y


def unwrap(m, dims=None, range=None):
    """``unwrap(m; dims, range)`` = ``unwrap!(similar(m), m; dims, range)`` (src/unwrap.jl:68)."""
    if not hasattr(m, "shape"):
        m = np.asarray(m)
    dt = _checked(m, "m")
    axis = _axis(len(m.shape), dims)                     # the argument checks come before anything touches a device
    if _dev.is_device_array(m):
        _lib.require_device()
        y = _dev.torch.empty_like(m)                     # keeps a dense layout (column-major stays column-major)
    else:
        y = np.empty(tuple(m.shape), dtype=dt)
    return unwrap_(y, m, dims=axis, range=range)
