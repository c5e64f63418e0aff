"""DSP.jl ``src/util.jl`` on this path: element-type rules and FFT-size selection (host side), and the COMMON DSP TOOLS and DELAY FINDING
UTILITIES -- ``rms``, ``rmsfft``, ``meanfreq``, ``finddelay``, ``shiftsignal(!)``, ``alignsignals(!)`` -- on the device (``mdsp_reduce_*``, ``mdsp_shift_*``).

Index arithmetic is delegated to the C ABI (``mdsp_nextfastfft`` etc.) so that Julia and Python hosts share one
bit-exact implementation.  Mutating forms ``f!`` are spelled ``f_``; numpy in, numpy out; a device tensor in, a device tensor out; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _dev, _lib, _plancache
from ._lib import ArgumentError, DomainError, UnsupportedError

_F32, _F64, _C32, _C64 = (np.dtype(t) for t in (np.float32, np.float64, np.complex64, np.complex128))


def nextfastfft(n):
    """``nextfastfft(n)`` / ``nextfastfft.(ns)`` (util.jl:134-135)."""
    if isinstance(n, (tuple, list)):
        return tuple(int(_lib.lib().mdsp_nextfastfft(int(k))) for k in n)
    return int(_lib.lib().mdsp_nextfastfft(int(n)))


def fftintype(dt) -> np.dtype:
    """util.jl:93-95."""
    dt = np.dtype(dt)
    if dt in (_F32, _F64, _C32, _C64):
        return dt
    return _C64 if dt.kind == "c" else _F64


def fftouttype(dt) -> np.dtype:
    """util.jl:98-100."""
    dt = np.dtype(dt)
    if dt in (_C32, _C64):
        return dt
    return _C32 if dt == _F32 else _C64


def fftabs2type(dt) -> np.dtype:
    """util.jl:103-105."""
    dt = np.dtype(dt)
    return _F32 if dt in (_F32, _C32) else _F64


def rfftfreq(n: int, fs=1.0) -> np.ndarray:
    """AbstractFFTs.rfftfreq."""
    return np.arange(n // 2 + 1) * (fs / n)


def fftfreq(n: int, fs=1.0) -> np.ndarray:
    """AbstractFFTs.fftfreq."""
    k = np.arange(n)
    k[k > (n - 1) // 2] -= n
    return k * (fs / n)


def promote_type(*dts) -> np.dtype:
    """Julia's ``promote_type`` for the element types of this path (Bool, Int*, UInt*, Float16/32/64 and their Complex forms).

    It is NOT ``np.result_type``: an integer never widens a float (``promote_type(Float32, Int64) == Float32``, numpy says float64), so
    ``filt(b::Vector{Float32}, 1, x::Vector{Float32})`` stays Float32 as in the reference (dspbase.jl:26-31, 775-777).  Mixed signedness
    follows Julia: the unsigned type wins at equal size, the larger type otherwise."""
    dts = [np.dtype(d) for d in dts]
    if not dts:
        raise TypeError("promote_type needs at least one type")
    cplx = any(d.kind == "c" for d in dts)
    reals = [np.dtype(np.float32) if d == _C32 else np.dtype(np.float64) if d == _C64 else d for d in dts]
    floats = [d for d in reals if d.kind == "f"]
    if floats:
        r = max(floats, key=lambda d: d.itemsize)
    else:
        ints = [d for d in reals if d.kind in "iu"]
        if not ints:
            r = np.dtype(np.bool_)
        else:
            size = max(d.itemsize for d in ints)
            unsigned_wins = any(d.kind == "u" and d.itemsize == size for d in ints)
            r = np.dtype(("u" if unsigned_wins else "i") + str(size))
    if not cplx:
        return r
    if r == np.dtype(np.float32) or r == np.dtype(np.float16):
        return _C32
    return _C64            # Complex{Int} has no numpy twin: the device computes those in ComplexF64 and rounds (dspbase._cast_result)


# ---------------------------------------------------------------------------------------------------------
# COMMON DSP TOOLS (util.jl:138-220) and DELAY FINDING UTILITIES (util.jl:316-430) on the device: mdsp_reduce_* and mdsp_shift_*
# ---------------------------------------------------------------------------------------------------------

def _real(a, what):
    if isinstance(a, bool) or not isinstance(a, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f"{what}: a real number expected, got {type(a).__name__}")
    return a


def _log10(a, what):
    if a < 0:
        raise DomainError(f"{what}: log10 of a negative number ({a})")
    return -math.inf if a == 0 else math.log10(a)


def db2pow(a):
    """``db2pow(a) = exp10(a/10)`` (util.jl:154)."""
    return 10.0 ** (_real(a, "db2pow") / 10)


def db2amp(a):
    """``db2amp(a) = exp10(a/20)`` (util.jl:162)."""
    return 10.0 ** (_real(a, "db2amp") / 20)


def pow2db(a):
    """``pow2db(a) = 10 log10(a)`` (util.jl:170)."""
    return 10 * _log10(_real(a, "pow2db"), "pow2db")


def amp2db(a):
    """``amp2db(a) = 20 log10(a)`` (util.jl:178)."""
    return 20 * _log10(_real(a, "amp2db"), "amp2db")


class ReducePlan:
    """``mdsp_reduce_plan``: ``route`` (``_lib.REDUCE_CONTIGUOUS`` / ``_STRIDED``), ``segments``, ``seglen``, ``depth`` (the longest chain of additions a term
    passes through), ``workspace_bytes``.  ``segments`` = 0 lets the library cut the lines; a positive value forces the cut (tests, tools/util_bench.py)."""

    def __init__(self, inner, length, outer, op, dtype, step=0.0, centre=0, segments=0):
        self._h = C.c_void_p()
        self.inner, self.len, self.outer, self.op, self.dtype = int(inner), int(length), int(outer), int(op), np.dtype(dtype)
        _lib.check(_lib.lib().mdsp_reduce_plan_create(C.byref(self._h), self.inner, self.len, self.outer, self.op, _dev.md_dtype(self.dtype), float(step),
                                                      int(centre), int(segments)))
        route, S, seglen, depth, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mdsp_reduce_plan_info(self._h, C.byref(route), C.byref(S), C.byref(seglen), C.byref(depth), C.byref(ws)))
        self.route, self.segments, self.seglen, self.depth, self.workspace_bytes = route.value, S.value, seglen.value, depth.value, ws.value

    def exec(self, in_ptr: int, out_ptr: int, stream: int | None = None):
        _lib.check(_lib.lib().mdsp_reduce_exec(self._h, in_ptr, out_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_reduce_plan_destroy(self._h)
        except Exception:
            pass


def reduce_geometry(inner: int, length: int, outer: int, op: int, dtype, segments: int = 0):
    """(route, segments, seglen, depth, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    route, S, seglen, depth, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_reduce_geometry_for(int(inner), int(length), int(outer), int(op), _dev.md_dtype(dtype), int(segments),
                                                   C.byref(route), C.byref(S), C.byref(seglen), C.byref(depth), C.byref(ws)))
    return route.value, S.value, seglen.value, depth.value, ws.value


class ShiftPlan:
    """``mdsp_shift_plan``: ``route`` (``_lib.SHIFT_DISJOINT`` / ``_HALO`` / ``_STAGED``), ``tile``, ``chunk``, ``ntiles``, ``workspace_bytes``.  ``tile`` = 0 and
    ``route`` = ``_lib.SHIFT_AUTO`` let the library choose; other values force them (tests, tools/util_bench.py)."""

    def __init__(self, length, s, elem_bytes, in_place, tile=0, route=_lib.SHIFT_AUTO):
        self._h = C.c_void_p()
        self.len, self.s, self.elem_bytes, self.in_place = int(length), int(s), int(elem_bytes), bool(in_place)
        _lib.check(_lib.lib().mdsp_shift_plan_create(C.byref(self._h), self.len, self.s, self.elem_bytes, int(self.in_place), int(tile), int(route)))
        r, t, c, n, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mdsp_shift_plan_info(self._h, C.byref(r), C.byref(t), C.byref(c), C.byref(n), C.byref(ws)))
        self.route, self.tile, self.chunk, self.ntiles, self.workspace_bytes = r.value, t.value, c.value, n.value, ws.value

    def exec(self, in_ptr: int, out_ptr: int, stream: int | None = None):
        _lib.check(_lib.lib().mdsp_shift_exec(self._h, in_ptr, out_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_shift_plan_destroy(self._h)
        except Exception:
            pass


def shift_geometry(length: int, s: int, elem_bytes: int, in_place: bool, tile: int = 0, route: int = _lib.SHIFT_AUTO):
    """(route, tile, chunk, ntiles, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    r, t, c, n, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_shift_geometry_for(int(length), int(s), int(elem_bytes), int(bool(in_place)), int(tile), int(route),
                                                  C.byref(r), C.byref(t), C.byref(c), C.byref(n), C.byref(ws)))
    return r.value, t.value, c.value, n.value, ws.value


def _work_dtype(dt: np.dtype, what: str) -> np.dtype:
    """The element type the device reduces: the four FFT types as they are, integers and Bool through Float64 (Complex{Int} through ComplexF64)."""
    if dt in (_F32, _F64, _C32, _C64):
        return dt
    if dt.kind in "iub":
        return _F64
    raise UnsupportedError(f"{what}: element type {dt} is not accelerated")


def _axis_of(nd: int, dims, what: str):
    if dims is None:
        return None
    if isinstance(dims, numbers.Integral) and not isinstance(dims, bool):
        if not -nd <= dims < nd:
            raise ArgumentError(f"{what}: Invalid dims specified: {dims}")
        return int(dims) % nd
    raise UnsupportedError(f"{what}: dims must be None or one axis (got {dims!r}); use DSP.jl's CPU path for several dimensions")


def _sumabs2(src, axis):
    """Float64 device tensor of sum |x|^2: 0-d over everything (axis None), else the shape of ``src`` with ``axis`` of size 1.  ``src``: a device tensor of
    one of the four FFT types, handed to the library as it lies in memory (C-contiguous, or column-major = C-contiguous of the reversed shape)."""
    tt = _dev.torch
    dt = _dev.np_dtype_of(src)
    nd = src.dim()
    rev = nd > 1 and not src.is_contiguous() and src.permute(*reversed(range(nd))).is_contiguous()
    srcv = (src.permute(*reversed(range(nd))) if rev else src).contiguous()
    if axis is None:
        inner, length, outer, oshape = 1, srcv.numel(), 1, ()
    else:
        vaxis = nd - 1 - axis if rev else axis
        vshape = tuple(srcv.shape)
        length = vshape[vaxis]
        outer = int(np.prod(vshape[:vaxis], dtype=np.int64))
        inner = int(np.prod(vshape[vaxis + 1:], dtype=np.int64))
        oshape = vshape[:vaxis] + (1,) + vshape[vaxis + 1:]
    out = tt.empty(oshape, dtype=tt.float64, device=srcv.device)
    plan = _plancache.plans.get(("reduce", _plancache.ctx_key(), inner, length, outer, _lib.REDUCE_SUMABS2, dt.str),
                                lambda: ReducePlan(inner, length, outer, _lib.REDUCE_SUMABS2, dt))
    plan.exec(_dev.ptr(srcv), _dev.ptr(out))
    return out.permute(*reversed(range(nd))) if (rev and axis is not None) else out


def _rms_like(s, dims, what, fft_form):
    if not hasattr(s, "shape"):
        s = np.asarray(s)
    dt = _dev.np_dtype_of(s)
    if fft_form and dt.kind != "c":
        raise TypeError("rmsfft: a complex array expected (f = fft(s))")           # MethodError in the reference (:200)
    W = _work_dtype(dt, what)
    R = fftabs2type(W)
    shape = tuple(int(k) for k in s.shape)
    axis = _axis_of(len(shape), dims, what)
    n = int(np.prod(shape, dtype=np.int64)) if axis is None else shape[axis]
    _lib.require_device()
    on_device = _dev.is_device_array(s)
    tt = _dev.torch
    oshape = () if axis is None else shape[:axis] + (1,) + shape[axis + 1:]
    if 0 in shape:                                         # mean of nothing: NaN (0/0), and no launch
        res = tt.full(oshape, float("nan"), dtype=_dev.torch_dtype(R), device=_dev.device())
    else:
        ssum = _sumabs2(_dev.as_device(s, W), axis)
        res = (ssum.sqrt() / n if fft_form else (ssum / n).sqrt()).to(_dev.torch_dtype(R))   # Float64 throughout, one rounding to the result type
    if on_device:
        return res
    return R.type(res.item()) if axis is None else res.cpu().numpy()


def rms(s, dims=None):
    """``rms(s; dims)`` = ``sqrt(mean(abs2, s; dims))`` (util.jl:186-192).  ``dims=None`` reduces everything; an integer axis (0-based, negative from the
    end) keeps that axis with size 1.  The result has the real type of the input (integers go through Float64); an empty input gives NaN without a
    launch.  A device tensor in gives a device tensor out (0-d for ``dims=None``) with no synchronisation; numpy in gives a numpy scalar / array.
    The sum is a deterministic Float64 reduction on the device (``mdsp_reduce_*``, SUMABS2): Float32 terms are exact products in Float64."""
    return _rms_like(s, dims, "rms", False)


def rmsfft(f):
    """``rmsfft(f)`` = ``sqrt(sum(abs2, f)) / length(f)`` (util.jl:200): the rms of ``ifft(f)``.  Complex input only."""
    return _rms_like(f, None, "rmsfft", True)


def _real_vector(x, what):
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    dt = _dev.np_dtype_of(x)
    if len(x.shape) != 1 or dt.kind not in "fiub":
        raise TypeError(f"{what}: a real vector expected")                           # MethodError in the reference
    return x, dt


def meanfreq(x, fs=2 * np.pi):
    """``meanfreq(x, fs=2pi)`` (util.jl:211-220): ``sum(pxx .* freqrg) / sum(pxx)`` with ``pxx = abs2.(rfft(x))`` and ``freqrg = fs/len .* (0:fld(len,2))``.
    The spectrum is one frame of the existing transform path (no window, any length); one pass over the bins forms both Float64 sums (SUMABS2_W), no
    ``|X|^2`` array is written.  Float64 unless ``x`` and ``fs`` are both Float32.  Device in, 0-d device tensor out; numpy in, numpy scalar out."""
    x, dt = _real_vector(x, "meanfreq")
    _real(fs, "meanfreq")
    n = int(x.shape[0])
    if n == 0:
        raise ArgumentError("meanfreq: empty signal")
    W = _F32 if dt == _F32 else _work_dtype(dt, "meanfreq")
    R = _F32 if (W == _F32 and isinstance(fs, np.float32)) else _F64
    _lib.require_device()
    from . import periodograms
    bins = periodograms.stft(_dev.as_device(x, W), n, 0, nfft=n, window=None, onesided=True).reshape(-1).contiguous()
    nb, cdt = int(bins.shape[0]), fftouttype(W)
    step = float(R.type(fs) / R.type(n)) if R == _F32 else float(fs) / n
    plan = _plancache.plans.get(("reduce", _plancache.ctx_key(), 1, nb, 1, _lib.REDUCE_SUMABS2_W, cdt.str, step),
                                lambda: ReducePlan(1, nb, 1, _lib.REDUCE_SUMABS2_W, cdt, step=step))
    out = _dev.torch.empty(2, dtype=_dev.torch.float64, device=bins.device)
    plan.exec(_dev.ptr(bins), _dev.ptr(out))
    res = (out[0] / out[1]).to(_dev.torch_dtype(R))
    return res if _dev.is_device_array(x) else R.type(res.item())


def finddelay(x, y) -> int:
    """``finddelay(x, y)`` (util.jl:336-347): the delay of ``x`` with respect to ``y``, from the peak of ``xcorr(y, x)``; ties go to the peak nearest to the
    centre, then to the smaller index.  The correlation and the arg-max (ABSARGMAX, ``centre = length(x)``) run on the device; the result is a Python
    ``int``, which costs one 16-byte copy to the host and a synchronisation.  A NaN in the correlation, or an empty operand, raises ``ArgumentError``
    (the reference's reduction over an empty collection throws)."""
    x, xdt = _real_vector(x, "finddelay")
    y, ydt = _real_vector(y, "finddelay")
    nx, ny = int(x.shape[0]), int(y.shape[0])
    if nx == 0 or ny == 0:
        raise ArgumentError("finddelay: reducing over an empty collection is not allowed")
    T = promote_type(xdt, ydt)
    if T.kind not in "iuf" or T == np.dtype(np.float16):
        T = _F64
    _lib.require_device()
    from . import dspbase
    s = dspbase.xcorr(_dev.as_device(y, T), _dev.as_device(x, T))                    # padmode = :none
    if _dev.np_dtype_of(s) not in (_F32, _F64):
        s = s.to(_dev.torch.float64)
    s = s.contiguous()
    n, sdt, centre = int(s.shape[0]), _dev.np_dtype_of(s), nx - 1                    # center_idx = length(x), 1-based
    plan = _plancache.plans.get(("reduce", _plancache.ctx_key(), 1, n, 1, _lib.REDUCE_ABSARGMAX, sdt.str, centre),
                                lambda: ReducePlan(1, n, 1, _lib.REDUCE_ABSARGMAX, sdt, centre=centre))
    rec = _dev.torch.empty(2, dtype=_dev.torch.int64, device=s.device)
    plan.exec(_dev.ptr(s), _dev.ptr(rec))
    idx, flag = rec.tolist()
    if flag or idx < 0:
        raise ArgumentError("finddelay: the cross-correlation holds NaN: no peak to locate")
    return centre - idx


def _shift_args(x, s, what):
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    if len(x.shape) != 1:
        raise TypeError(f"{what}: a vector expected")
    if isinstance(s, bool) or not isinstance(s, numbers.Integral):
        raise TypeError(f"{what}: s must be an integer")
    n, s = int(x.shape[0]), int(s)
    if abs(s) > n:
        raise DomainError(f"{what}: The absolute value of s must not be greater than the length of x (s = {s}, length {n})")   # :359-361
    esize = _dev.np_dtype_of(x).itemsize
    if esize not in (4, 8, 16):
        raise UnsupportedError(f"{what}: elements of {esize} bytes are not accelerated (4, 8 or 16)")
    return x, s, n, esize


def _shift_exec(src, dst, s, n, esize, tile=0, route=_lib.SHIFT_AUTO):
    in_place = src.data_ptr() == dst.data_ptr()
    plan = _plancache.plans.get(("shift", _plancache.ctx_key(), n, s, esize, in_place, tile, route), lambda: ShiftPlan(n, s, esize, in_place, tile, route))
    plan.exec(_dev.ptr(src), _dev.ptr(dst))
    return plan


def shiftsignal_(x, s, tile: int = 0, route: int = _lib.SHIFT_AUTO):
    """``shiftsignal!(x, s)`` (util.jl:357-370): shift ``x`` by ``s`` samples in place, zeros shifted in; returns ``x`` itself.  A contiguous device tensor is
    shifted where it lies (``mdsp_shift_*``: no full temporary unless the plan says STAGED); any other container goes through a device copy.
    ``abs(s) > length(x)`` raises ``DomainError``; ``s == 0`` returns without a launch.  ``tile`` / ``route``: forced plan arguments (tests, tools)."""
    x, s, n, esize = _shift_args(x, s, "shiftsignal!")
    if s == 0 or n == 0:
        return x
    _lib.require_device()
    if _dev.is_device_array(x) and x.is_contiguous():
        _shift_exec(x, x, s, n, esize, tile, route)
        return x
    t = (x if _dev.is_device_array(x) else _dev.torch.from_numpy(np.ascontiguousarray(x)).to(_dev.device())).contiguous()
    t = t.clone() if _dev.is_device_array(x) and t.data_ptr() == x.data_ptr() else t
    _shift_exec(t, t, s, n, esize, tile, route)
    if isinstance(x, np.ndarray):
        x[...] = t.cpu().numpy()
    else:
        x.copy_(t)
    return x


def shiftsignal(x, s, tile: int = 0, route: int = _lib.SHIFT_AUTO):
    """``shiftsignal(x, s)`` = ``shiftsignal!(copy(x), s)`` (util.jl:395), out of place in one launch: ``y[i] = x[i - s]`` where that exists, else 0."""
    x, s, n, esize = _shift_args(x, s, "shiftsignal")
    if s == 0 or n == 0:
        return x.clone() if _dev.is_device_array(x) else np.array(x, copy=True)
    _lib.require_device()
    on_device = _dev.is_device_array(x)
    src = (x if on_device else _dev.torch.from_numpy(np.ascontiguousarray(x)).to(_dev.device())).contiguous()
    dst = _dev.torch.empty_like(src)
    _shift_exec(src, dst, s, n, esize, tile, route)
    return dst if on_device else dst.cpu().numpy()


def alignsignals_(x, y):
    """``alignsignals!(x, y)`` (util.jl:404-408): ``(shiftsignal!(x, -d), d)`` with ``d = finddelay(x, y)``."""
    d = finddelay(x, y)
    return shiftsignal_(x, -d), d


def alignsignals(x, y):
    """``alignsignals(x, y)`` (util.jl:427): ``(x shifted by -d, d)``."""
    d = finddelay(x, y)
    return shiftsignal(x, -d), d
