"""DSP.jl ``src/lpc.jl`` : ``arburg`` and ``lpc(x, p, LPCBurg())`` on the device (``mdsp_burg_*``), ``levinson`` on the host,
``lpc(x, p, LPCLevinson())`` as the device ``xcorr`` followed by ``levinson``.

Vectors only; numpy or a device tensor in, small numpy arrays of the working type ``F`` and a scalar of its real type ``R`` out (every call ends in one
small copy to the host).  Float32 stays Float32, integers and Bool go through Float64 (lpc.jl:57-58).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import numbers

import numpy as np

from . import _dev, _lib, _plancache
from ._lib import ArgumentError, UnsupportedError
from .util import _work_dtype


class LPCBurg:
    """Dispatch type of ``lpc`` (lpc.jl:11): Burg's method."""

    def __eq__(self, other):
        return isinstance(other, LPCBurg)

    def __hash__(self):
        return hash(LPCBurg)


class LPCLevinson:
    """Dispatch type of ``lpc`` (lpc.jl:12): the autocorrelation method."""

    def __eq__(self, other):
        return isinstance(other, LPCLevinson)

    def __hash__(self):
        return hash(LPCLevinson)


class BurgPlan:
    """``mdsp_burg_plan`` for vectors of ``n`` samples of ``dtype``: ``segments``, ``seglen``, ``tile``, ``workspace_bytes``.  ``segments`` = 0 lets the library cut
    the pair range; a positive value forces the cut (tests, tools/lpc_bench.py)."""

    def __init__(self, dtype, n, segments=0):
        self._h = C.c_void_p()
        self.dtype, self.n = np.dtype(dtype), int(n)
        _lib.check(_lib.lib().mdsp_burg_plan_create(C.byref(self._h), _dev.md_dtype(self.dtype), self.n, int(segments)))
        S, seglen, tile, ws = (C.c_int64() for _ in range(4))
        _lib.check(_lib.lib().mdsp_burg_plan_info(self._h, C.byref(S), C.byref(seglen), C.byref(tile), C.byref(ws)))
        self.segments, self.seglen, self.tile, self.workspace_bytes = S.value, seglen.value, tile.value, ws.value

    def exec(self, x_ptr: int, p: int, rec_ptr: int, stream: int | None = None):
        """The whole recursion of order ``p``: the record -- ``2 p + 2`` elements of ``dtype``: ``a``, the reflection coefficients, ``prediction_err`` in the real
        part of the last -- goes to ``rec_ptr``."""
        _lib.check(_lib.lib().mdsp_burg_exec(self._h, x_ptr, int(p), rec_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_burg_plan_destroy(self._h)
        except Exception:
            pass


def burg_geometry(dtype, n: int, segments: int = 0):
    """(segments, seglen, tile, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    S, seglen, tile, ws = (C.c_int64() for _ in range(4))
    _lib.check(_lib.lib().mdsp_burg_geometry_for(_dev.md_dtype(dtype), int(n), int(segments), C.byref(S), C.byref(seglen), C.byref(tile), C.byref(ws)))
    return S.value, seglen.value, tile.value, ws.value


def split_record(rec: np.ndarray, p: int):
    """(a, prediction_err, reflection_coeffs) of a record of ``2 p + 2`` elements."""
    rec = np.asarray(rec)
    return rec[:p + 1].copy(), rec[2 * p + 1].real, rec[p + 1:2 * p + 1].copy()


def _order(p, what):
    if isinstance(p, bool) or not isinstance(p, numbers.Integral):
        raise TypeError(f"{what}: the order must be an integer, got {type(p).__name__}")
    return int(p)


def _vector(x, what):
    """(x, working dtype, n) after the checks that come before any device work."""
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    dt = _dev.np_dtype_of(x)
    if len(x.shape) != 1 or dt.kind not in "fciub":
        raise TypeError(f"{what}: a vector of numbers expected")                       # MethodError in the reference
    if dt == np.dtype(np.float16):
        raise UnsupportedError(f"{what}: element type {dt} is not accelerated")
    return x, _work_dtype(dt, what), int(x.shape[0])


def arburg(x, p):
    """``arburg(x, p)`` (lpc.jl:53-92): ``(a, prediction_err, reflection_coeffs)`` by Burg's method -- ``a`` with its leading 1, ``p + 1`` numbers.  ``2 p`` launches
    on the current stream and one copy of the record; the two work arrays belong to the cached plan and ``x`` is not written.  ``0 <= p <= N - 1``: the
    reference throws for ``p > N`` only and divides zero by zero at ``p = N``, here both are ``ArgumentError``.  A zero signal or a sample that is not finite
    gives NaN coefficients as in the reference."""
    x, W, n = _vector(x, "arburg")
    p = _order(p, "arburg")
    if not 0 <= p <= n - 1:
        raise ArgumentError(f"arburg: the order must be in [0, N - 1] = [0, {n - 1}], got {p}")
    _lib.require_device()
    xd = _dev.as_device(x, W).contiguous()
    plan = _plancache.plans.get(("burg", _plancache.ctx_key(), W.str, n), lambda: BurgPlan(W, n))
    rec = _dev.torch.empty(2 * p + 2, dtype=_dev.torch_dtype(W), device=xd.device)
    plan.exec(_dev.ptr(xd), p, _dev.ptr(rec))
    return split_record(rec.cpu().numpy(), p)


def _abs2(z):
    return z.real * z.real + z.imag * z.imag


def levinson(R_xx, p):
    """``levinson(R_xx, p)`` (lpc.jl:122-145): ``(a, prediction_err, reflection_coeffs)`` of the Hermitian Toeplitz system with first column ``R_xx[:p]``, without
    the leading 1.  Host code, ``O(p^2)`` on ``p + 1`` numbers in the working type, in the reference's order with a sequential ``dotu``; a device tensor is
    read by copying ``p + 1`` elements.  ``p >= 1`` and ``len(R_xx) >= p + 1``."""
    p = _order(p, "levinson")
    R_xx, W, n = _vector(R_xx, "levinson")
    if p < 1 or n < p + 1:
        raise ArgumentError(f"levinson: p >= 1 and length(R_xx) >= p + 1 are needed (p = {p}, length {n})")   # the reference indexes out of bounds
    head = R_xx[:p + 1]
    r = (head.cpu().numpy() if _dev.is_device_array(head) else np.asarray(head)).astype(W)
    Rt = np.dtype(np.float32) if W in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)
    one = Rt.type(1)
    with np.errstate(all="ignore"):
        k = -r[1] / r[0]                                                                # :124
        err = (r[0] * (one - _abs2(k))).real                                            # :126
        a = np.zeros(p, dtype=W)
        refl = np.zeros(p, dtype=W)
        a[0] = refl[0] = k
        for m in range(2, p + 1):                                                       # :135-141
            rev = a[m - 2::-1].copy()
            dotu = W.type(0)
            for i in range(m - 1):
                dotu = r[1 + i] * rev[i] + dotu
            k = -(r[m] + dotu) / err
            a[:m - 1] = k * np.conj(rev) + a[:m - 1]
            a[m - 1] = refl[m - 1] = k
            err = err * (one - _abs2(k))
    return a, Rt.type(err), refl


def lpc(x, p, method=None):
    """``lpc(x, p, [LPCBurg()])`` / ``lpc(x, p, LPCLevinson())`` (lpc.jl:28-32, :94-98, :159): ``(a, prediction_err)`` without the leading 1.  Burg is ``arburg``;
    Levinson is the device ``xcorr(x, scaling="biased")``, its lags ``0 .. p`` and ``levinson`` on the host."""
    method = LPCBurg() if method is None else method
    if isinstance(method, LPCBurg):
        a, err, _ = arburg(x, p)
        return a[1:], err
    if not isinstance(method, LPCLevinson):
        raise TypeError(f"lpc: LPCBurg() or LPCLevinson() expected, got {type(method).__name__}")
    x, W, n = _vector(x, "lpc")
    p = _order(p, "lpc")
    if not 1 <= p <= n - 1:
        raise ArgumentError(f"lpc: the order of the Levinson method must be in [1, N - 1] = [1, {n - 1}], got {p}")
    _lib.require_device()
    from .dspbase import xcorr
    r = xcorr(_dev.as_device(x, W).contiguous(), scaling="biased")
    a, err, _ = levinson(r[n - 1:n + p], p)
    return a, err
