"""Filter responses of DSP.jl ``src/Filters/response.jl`` on the device (``mdsp_resp_*``): ``freqresp``, ``phaseresp``, ``grpdelay``, ``impresp``, ``stepresp``
for filters with real coefficients; ``freqresp``, ``phaseresp`` and ``grpdelay`` also of analog (``"s"``) filters, at the points ``i w`` (response.jl:35, :113-120).

Every coefficient type runs through its own form -- a ``PolynomialRatio`` through POLY, a ``Biquad`` / ``SecondOrderSections`` through SECTIONS, a
``ZeroPoleGain`` through ZPK (response.jl:42-52) --, never through a conversion.  The working type is ComplexF32 when the coefficients and ``w`` are both
Float32, ComplexF64 otherwise.  ``w`` decides where the result lives: a numpy array or a Python sequence gives numpy, a device tensor a device tensor; the
result has the shape of ``w``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _dev, _lib, _plancache
from ._lib import ArgumentError, UnsupportedError
from .coefficients import Biquad, FilterCoefficients, PolynomialRatio, SecondOrderSections, ZeroPoleGain, coefa, coefb, require_z
from .unwrap import unwrap

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


class RespPlan:
    """``mdsp_resp_plan``: ``chunks``, ``chunk_len``, ``workspace_bytes``.  ``num`` / ``den``: the coefficient vectors of POLY, the K x 5 table of SECTIONS
    (``den`` None), complex zeros and poles of ZPK.  ``dtype`` is the real type of the working type.  ``chunks`` = 0 lets the library cut a long
    polynomial; a positive value forces the cut (tests, tools/response_bench.py).  Creating a plan needs no device."""

    def __init__(self, form, dtype, num, den=None, gain=1.0, nw=0, flags=0, out_mode=_lib.RESP_COMPLEX, in_mode=_lib.RESP_W, cminus=0.0, chunks=0):
        self._h = C.c_void_p()
        self.form, self.dtype, self.nw, self.out_mode, self.in_mode = int(form), np.dtype(dtype), int(nw), int(out_mode), int(in_mode)

        def flat(v):
            if v is None:
                return None, 0
            a = np.asarray(v)
            if form == _lib.RESP_ZPK:
                a = np.ascontiguousarray(a.astype(np.complex128).reshape(-1))
                return a.view(np.float64), a.size
            if a.dtype.kind == "c":
                raise UnsupportedError("complex filter coefficients are not accelerated: use DSP.jl's CPU path")
            a = np.ascontiguousarray(a, dtype=np.float64)
            return (a.reshape(-1), a.size // 5) if form == _lib.RESP_SECTIONS else (a.reshape(-1), a.size)

        nv, nn = flat(num)
        dv, nd = (nv, nn) if den is num and den is not None else flat(den)
        self._keep = (nv, dv)
        _lib.check(_lib.lib().mdsp_resp_plan_create(C.byref(self._h), self.form, int(flags), self.out_mode, self.in_mode, _dev.md_dtype(self.dtype),
                                                    None if nv is None else nv.ctypes.data_as(_lib.pdbl), nn,
                                                    None if dv is None or nd == 0 else dv.ctypes.data_as(_lib.pdbl), nd, float(gain), float(cminus),
                                                    self.nw, int(chunks)))
        c, ln, ws = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mdsp_resp_plan_info(self._h, C.byref(c), C.byref(ln), C.byref(ws)))
        self.chunks, self.chunk_len, self.workspace_bytes = c.value, ln.value, ws.value

    def exec(self, in_ptr: int, out_ptr: int, stream: int | None = None):
        _lib.check(_lib.lib().mdsp_resp_exec(self._h, in_ptr, out_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_resp_plan_destroy(self._h)
        except Exception:
            pass


def resp_geometry(form: int, dtype, ncoef: int, has_den: bool, nw: int, chunks: int = 0):
    """(chunks, chunk_len, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    c, ln, ws = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_resp_geometry_for(int(form), _dev.md_dtype(dtype), int(ncoef), 1 if has_den else 0, int(nw), int(chunks),
                                                 C.byref(c), C.byref(ln), C.byref(ws)))
    return c.value, ln.value, ws.value


def _freqrange(f=None):
    if f is None or f.domain == "z":
        return np.linspace(0.0, np.pi, 257)                              # response.jl:158
    f = ZeroPoleGain(f)                                                  # :159-175, on the host
    w_interesting = np.sort(np.abs(np.concatenate([f.p, f.z])).astype(np.float64))
    include_zero = w_interesting.size > 0 and w_interesting[0] == 0
    nonzero = np.flatnonzero(w_interesting)
    if nonzero.size == 0:                                                # no non-zero poles or zeros
        with np.errstate(divide="ignore"):
            inv_k = np.float64(1.0) / np.float64(f.k)
        if not include_zero or not np.isfinite(inv_k):
            w = 10.0 ** np.arange(-1, 7)                                 # fallback
            w[0] = 0.0
            return w
        return np.linspace(0.0, 10 * float(max(np.float64(f.k), inv_k)), 200)   # the point where |H| = 1 (if any), and further by a factor 10
    w_min, w_max = w_interesting[nonzero[0]], w_interesting[-1]          # from the smallest to the largest pole / zero, extended by a factor 10
    w = 10.0 ** np.linspace(np.log10(w_min) - 1, np.log10(w_max) + 1, 200)
    return np.concatenate([[0.0], w]) if include_zero else w


def _check_filter(f):
    if not isinstance(f, FilterCoefficients):
        raise TypeError("a filter coefficient object (PolynomialRatio, Biquad, ZeroPoleGain, SecondOrderSections) is expected")


def _w_type(w):
    """(w as it is: a device tensor or a numpy array, its float type).  Complex frequencies are not accelerated."""
    if not _dev.is_device_array(w) and not isinstance(w, _dev.torch.Tensor):
        w = np.asarray(w)
    dt = _dev.np_dtype_of(w)
    if dt.kind == "c":
        raise UnsupportedError("complex frequencies are not accelerated: use DSP.jl's CPU path")
    if dt.kind not in "fiub":
        raise TypeError("w must be real numbers")
    return w, (_F32 if dt == _F32 else _F64)


def _real_type(wdt, *coef_types):
    """Float32 when w and every coefficient type are (integers promote to anything), Float64 otherwise."""
    single = wdt == _F32 and all(np.dtype(t) == _F32 or np.dtype(t).kind in "iub" for t in coef_types)
    return _F32 if single else _F64


def _in_mode(f):
    """The plan's input: ``w`` for a digital filter (the kernel forms e^{iw}), the points ``i w`` for an analog one (response.jl:27, :35)."""
    return _lib.RESP_POINTS if f.domain == "s" else _lib.RESP_W


def _form_of(f, wdt):
    """(form, real type, num, den, gain, flags) of a filter's own form.  The section and zero-pole-gain forms are written in the point itself, so they
    serve both domains; an ``"s"`` ``PolynomialRatio`` hands its coefficients over lowest power first, to be evaluated at the point as it is."""
    if isinstance(f, PolynomialRatio) and f.domain == "s":
        den = None if len(f.a) == 1 and f.a[0] == 1 else f.a[::-1].copy()
        return _lib.RESP_POLY, _real_type(wdt, f.dtype), f.b[::-1].copy(), den, 1.0, 0
    if isinstance(f, PolynomialRatio):
        return _lib.RESP_POLY, _real_type(wdt, f.dtype), f.b, (f.a if len(f.a) > 1 else None), 1.0, _lib.RESP_NEG
    if isinstance(f, Biquad):
        return _lib.RESP_SECTIONS, _real_type(wdt, f.dtype), np.array([[float(v) for v in f.coefficients()]]), None, 1.0, 0
    if isinstance(f, SecondOrderSections):
        return _lib.RESP_SECTIONS, _real_type(wdt, f.dtype, f.gdtype), f.table(), None, float(f.g), 0
    if isinstance(f, ZeroPoleGain):
        return _lib.RESP_ZPK, _real_type(wdt, f.dtype, f.kdtype), f.z, f.p, float(f.k), 0
    raise TypeError("not a filter coefficient object")


def _run(w, R, form, num, den, gain, flags, out_mode, cminus=0.0, in_mode=_lib.RESP_W):
    """One plan over the points of ``w`` (already checked); the result has w's shape and lives where w lives.  ``in_mode`` RESP_POINTS: the plan is given
    the points ``i w`` of the imaginary axis, formed on the device, instead of ``w``."""
    _lib.require_device()
    shape = tuple(int(k) for k in w.shape)
    nw = int(np.prod(shape, dtype=np.int64))
    odt = np.dtype(np.complex64 if R == _F32 else np.complex128) if out_mode == _lib.RESP_COMPLEX else R
    on_device = _dev.is_device_array(w)
    if nw == 0:                                                          # nothing to do, and no launch
        return _dev.torch.empty(shape, dtype=_dev.torch_dtype(odt), device=w.device) if on_device else np.empty(shape, dtype=odt)
    wd = _dev.as_device(w, R).contiguous().reshape(-1)
    if in_mode == _lib.RESP_POINTS:                                      # im .* w (response.jl:35, :118)
        wd = _dev.torch.complex(_dev.torch.zeros_like(wd), wd)
    out = _dev.torch.empty(nw, dtype=_dev.torch_dtype(odt), device=wd.device)
    numa, dena = np.asarray(num), (None if den is None else np.asarray(den))
    key = ("resp", _plancache.ctx_key(), form, R.str, numa.tobytes(), numa.dtype.str, None if dena is None else dena.tobytes(), float(gain), flags, out_mode,
           float(cminus), nw, in_mode)
    plan = _plancache.plans.get(key, lambda: RespPlan(form, R, numa, numa if den is num and den is not None else dena, gain, nw, flags, out_mode,
                                                      in_mode, cminus))
    plan.exec(_dev.ptr(wd), _dev.ptr(out))
    out = out.reshape(shape)
    return out if on_device else out.cpu().numpy()


def freqresp(f, w=None):
    """``freqresp(f)`` -> ``(H, w)`` with ``w = range(0, π, 257)``; ``freqresp(f, w)`` -> ``H`` (response.jl:16-27)."""
    _check_filter(f)
    if w is None:
        w = _freqrange(f)
        return freqresp(f, w), w
    w, wdt = _w_type(w)
    form, R, num, den, gain, flags = _form_of(f, wdt)
    return _run(w, R, form, num, den, gain, flags, _lib.RESP_COMPLEX, in_mode=_in_mode(f))


def phaseresp(f, w=None):
    """``phaseresp(f[, w])`` (response.jl:62-76): ``unwrap(angle.(freqresp(f, w)); dims=ndims)``, the angle taken in the response kernel."""
    _check_filter(f)
    if w is None:
        w = _freqrange(f)
        return phaseresp(f, w), w
    w, wdt = _w_type(w)
    form, R, num, den, gain, flags = _form_of(f, wdt)
    phi = _run(w, R, form, num, den, gain, flags, _lib.RESP_ANGLE, in_mode=_in_mode(f))
    if len(phi.shape) == 0 or 0 in tuple(phi.shape):
        return phi
    return unwrap(phi, dims=-1)


def _is_sym(x):                                                          # response.jl:148-151
    n = len(x) // 2
    return all(x[i] == x[len(x) - 1 - i] for i in range(n))


def _is_anti_sym(x):                                                     # response.jl:153-156 (the range is 0:n)
    n = len(x) // 2
    return all(x[i] == -x[len(x) - 1 - i] for i in range(n + 1))


def _analog_grpdelay_polys(b, a):
    """``b' a - a' b`` and ``a b`` (response.jl:115-119) of ``coefb`` / ``coefa`` of an ``"s"`` filter, as plain Float64 polynomial products, lowest
    power first: what the POLY plan takes."""
    b, a = np.asarray(b, np.float64)[::-1], np.asarray(a, np.float64)[::-1]
    bd, ad = b[1:] * np.arange(1, len(b)), a[1:] * np.arange(1, len(a))
    num = np.zeros(max(len(b) + len(a) - 2, 1))
    for d, c, sign in ((bd, a, 1.0), (ad, b, -1.0)):
        if len(d):
            num[:len(d) + len(c) - 1] += sign * np.convolve(d, c)
    return num, np.convolve(a, b)


def grpdelay(f, w=None):
    """``grpdelay(f[, w])`` (response.jl:85-111): a constant for a linear-phase FIR filter, else ``c = xcorr(b, a)`` on the device and
    ``real(sum k c[k] y^k / sum c[k] y^k) - (length(a) - 1)`` at ``y = exp(-iw)`` in one plan over the one vector ``c``.

    An analog filter (:113-120): ``real((b' a - a' b)(s) / (a b)(s))`` at ``s = iw``, the two products formed on the host in Float64, one plan."""
    _check_filter(f)
    if w is None:
        w = _freqrange(f)
        return grpdelay(f, w), w
    w, wdt = _w_type(w)
    b, a = coefb(f), coefa(f)
    R = _real_type(wdt, b.dtype, a.dtype)
    if f.domain == "s":
        num, den = _analog_grpdelay_polys(b, a)
        return _run(w, R, _lib.RESP_POLY, num, den, 1.0, 0, _lib.RESP_REAL_MINUS, cminus=0.0, in_mode=_lib.RESP_POINTS)
    if len(a) == 1 and (_is_sym(b) or _is_anti_sym(b)):                  # linear-phase FIR
        _lib.require_device()
        shape = tuple(int(k) for k in w.shape)
        val = (len(b) - 1) / 2
        if _dev.is_device_array(w):
            return _dev.torch.full(shape, val, dtype=_dev.torch.float64, device=w.device)
        return np.full(shape, val, dtype=np.float64)
    _lib.require_device()
    from .dspbase import xcorr
    c = xcorr(_dev.as_device(b.astype(R), R), _dev.as_device(a.astype(R), R), padmode="none").cpu().numpy()   # the coefficients of a plan are host arrays
    return _run(w, R, _lib.RESP_POLY, c, c, 1.0, _lib.RESP_NEG | _lib.RESP_DERIV, _lib.RESP_REAL_MINUS, cminus=len(a) - 1)


def _time_response(f, n, step, device):
    _check_filter(f)
    require_z(f, "stepresp" if step else "impresp")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError("n must be an integer")
    if n < 0:
        raise ArgumentError(f"the number of points must not be negative, got {n}")
    if isinstance(f, PolynomialRatio) and len(f.a) > 1:
        f = SecondOrderSections(f)                                       # the reference runs direct form here; this library has the cascade only
    _lib.require_device()
    tt = _dev.torch
    x = tt.ones(int(n), dtype=tt.float64, device=_dev.device()) if step else tt.zeros(int(n), dtype=tt.float64, device=_dev.device())
    if not step and n > 0:
        x[0] = 1.0
    from . import filt
    y = filt(f, x) if n > 0 else x
    return y if device else y.cpu().numpy()


def impresp(f, n=100, device: bool = False):
    """``impresp(f, n=100)`` (response.jl:127-130): ``filt(f, [1, 0, 0, ...])``, the Float64 impulse made on the device.  A ``PolynomialRatio`` with a
    vector ``a`` is converted with ``SecondOrderSections(f)`` first (the reference runs direct form).  ``device=True`` leaves the result on the device."""
    return _time_response(f, n, False, device)


def stepresp(f, n=100, device: bool = False):
    """``stepresp(f, n=100)`` (response.jl:137-140): ``filt(f, ones(n))``; see ``impresp``."""
    return _time_response(f, n, True, device)
