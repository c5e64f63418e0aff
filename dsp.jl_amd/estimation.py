"""DSP.jl ``src/estimation.jl`` on the device: ``jacobsen`` and ``quinn`` (``mdsp_est_*``, ``mdsp_quinn_*``) and ``esprit`` (the Gram matrix
of its Hankel matrix by ``mdsp_hankel_gram_*``, the ``M x M`` eigenproblem on the host).  ``esprit`` refuses ``p >= M``, ``2 M - 1 > N`` and
``M > ESPRIT_MAX_M``.

Vectors only; numpy or a device tensor in, Python numbers out (every call ends in one small copy to the host).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import numbers

import numpy as np

from . import _dev, _lib, _plancache
from ._lib import ArgumentError, UnsupportedError
from .util import _work_dtype, fftouttype

PEAK_WORDS = 8


class EstReducePlan:
    """``mdsp_est_reduce_plan`` (``_lib.EST_SUM`` / ``EST_ABS2ARGMAX``): ``route``, ``segments``, ``seglen``, ``depth``, ``workspace_bytes`` as ``util.ReducePlan``."""

    def __init__(self, inner, length, outer, op, dtype, segments=0):
        self._h = C.c_void_p()
        self.inner, self.len, self.outer, self.op, self.dtype = int(inner), int(length), int(outer), int(op), np.dtype(dtype)
        _lib.check(_lib.lib().mdsp_est_reduce_plan_create(C.byref(self._h), self.inner, self.len, self.outer, self.op, _dev.md_dtype(self.dtype), int(segments)))
        route, S, seglen, depth, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().mdsp_est_reduce_plan_info(self._h, C.byref(route), C.byref(S), C.byref(seglen), C.byref(depth), C.byref(ws)))
        self.route, self.segments, self.seglen, self.depth, self.workspace_bytes = route.value, S.value, seglen.value, depth.value, ws.value

    def exec(self, in_ptr: int, out_ptr: int, stream: int | None = None):
        _lib.check(_lib.lib().mdsp_est_reduce_exec(self._h, in_ptr, out_ptr, _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_est_reduce_plan_destroy(self._h)
        except Exception:
            pass


def est_reduce_geometry(inner: int, length: int, outer: int, op: int, dtype, segments: int = 0):
    """(route, segments, seglen, depth, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    route, S, seglen, depth, ws = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().mdsp_est_reduce_geometry_for(int(inner), int(length), int(outer), int(op), _dev.md_dtype(dtype), int(segments),
                                                       C.byref(route), C.byref(S), C.byref(seglen), C.byref(depth), C.byref(ws)))
    return route.value, S.value, seglen.value, depth.value, ws.value


class QuinnPlan:
    """``mdsp_quinn_plan`` for vectors of ``n`` samples of ``dtype``: ``segments``, ``seglen``, ``tile``, ``run``, ``workspace_bytes``.  ``segments`` = 0 lets the
    library cut the signal; a positive value forces the cut (tests, tools/est_bench.py)."""

    def __init__(self, dtype, n, segments=0):
        self._h = C.c_void_p()
        self.dtype, self.n = np.dtype(dtype), int(n)
        _lib.check(_lib.lib().mdsp_quinn_plan_create(C.byref(self._h), _dev.md_dtype(self.dtype), self.n, int(segments)))
        S, seglen, tile, run, ws = (C.c_int64() for _ in range(5))
        _lib.check(_lib.lib().mdsp_quinn_plan_info(self._h, C.byref(S), C.byref(seglen), C.byref(tile), C.byref(run), C.byref(ws)))
        self.segments, self.seglen, self.tile, self.run, self.workspace_bytes = S.value, seglen.value, tile.value, run.value, ws.value

    def pass_exec(self, x_ptr: int, mean, param: float, out_ptr: int, stream: int | None = None):
        """One pass: ``param`` is alpha (real ``dtype``) or omega (complex); the record (4 or 3 doubles) goes to ``out_ptr``."""
        mu = (C.c_double * 2)(float(np.real(mean)), float(np.imag(mean)))
        _lib.check(_lib.lib().mdsp_quinn_pass_exec(self._h, x_ptr, mu, float(param), out_ptr, _dev.stream_ptr() if stream is None else stream))

    def estimate(self, x_ptr: int, f0: float, fs: float, tol: float = 1e-6, maxiters: int = 20, stream: int | None = None):
        """(estimate, reached_maxiters, iterations) of ``mdsp_quinn_estimate``."""
        est, reached, iters = C.c_double(), C.c_int(), C.c_int64()
        _lib.check(_lib.lib().mdsp_quinn_estimate(self._h, x_ptr, float(f0), float(fs), float(tol), int(maxiters), C.byref(est), C.byref(reached), C.byref(iters),
                                                  _dev.stream_ptr() if stream is None else stream))
        return est.value, bool(reached.value), iters.value

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_quinn_plan_destroy(self._h)
        except Exception:
            pass


def quinn_geometry(dtype, n: int, segments: int = 0):
    """(segments, seglen, tile, run, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    S, seglen, tile, run, ws = (C.c_int64() for _ in range(5))
    _lib.check(_lib.lib().mdsp_quinn_geometry_for(_dev.md_dtype(dtype), int(n), int(segments), C.byref(S), C.byref(seglen), C.byref(tile), C.byref(run), C.byref(ws)))
    return S.value, seglen.value, tile.value, run.value, ws.value


def _vector(x, what):
    """(x, working dtype, n) after the checks that come before any device work."""
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    dt = _dev.np_dtype_of(x)
    if len(x.shape) != 1 or dt.kind not in "fciub":
        raise TypeError(f"{what}: a vector of numbers expected")                       # MethodError in the reference
    if dt == np.dtype(np.float16):
        raise UnsupportedError(f"{what}: element type {dt} is not accelerated")
    W = _work_dtype(dt, what)
    n = int(x.shape[0])
    if n < 2:
        raise ArgumentError(f"{what}: at least two samples are needed (got {n})")     # the reference indexes out of bounds at N = 1
    return x, W, n


def _fs(fs, what):
    if isinstance(fs, bool) or not isinstance(fs, (numbers.Real, np.floating, np.integer)):
        raise TypeError(f"{what}: a real number expected, got {type(fs).__name__}")
    return float(fs)


def jacobsen_from_record(rec, n: int, fs: float, real: bool) -> float:
    """estimation.jl:97, :108-114 in Float64 from a peak record (``mdsp_est_peak_gather``): eight 8-byte words {index, flag, X[k-1], X[k], X[k+1]}."""
    rec = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)
    k, flag = (int(v) for v in rec[:16].view(np.int64))
    if flag or k < 0:
        return float("nan")
    xm, x0, xp = rec[16:].view(np.complex128)
    fpeak = (k if k < (n + 1) // 2 else k - n) * (fs / n)                             # fftfreq(N, Fs)[k]
    den = 2 * x0 - xm - xp
    delta = -((xp - xm) / den).real if den != 0 else float("nan")
    est = fpeak + delta * fs / n
    return abs(est) if real else est


def jacobsen(x, Fs=1.0) -> float:
    """``jacobsen(x, Fs=1.0)`` (estimation.jl:93-115): the frequency of the largest sinusoid in ``x`` from the peak bin of one transform of the whole signal and
    its two neighbours.  The spectrum is one frame of the existing transform path (no window, any length; one-sided for a real signal: the mirrored half
    gives the same value after ``abs``), ABS2ARGMAX finds the peak, one lane gathers the three bins, and 64 bytes come to the host, where ``delta`` is formed
    in Float64.  A NaN in the spectrum gives NaN."""
    x, W, n = _vector(x, "jacobsen")
    fs = _fs(Fs, "jacobsen")
    _lib.require_device()
    from . import periodograms
    real = W.kind != "c"
    bins = periodograms.stft(_dev.as_device(x, W), n, 0, nfft=n, window=None, onesided=real).reshape(-1).contiguous()
    nb, cdt = int(bins.shape[0]), fftouttype(W)
    plan = _plancache.plans.get(("est_reduce", _plancache.ctx_key(), 1, nb, 1, _lib.EST_ABS2ARGMAX, cdt.str),
                                lambda: EstReducePlan(1, nb, 1, _lib.EST_ABS2ARGMAX, cdt))
    rec = _dev.torch.empty(2 + PEAK_WORDS, dtype=_dev.torch.int64, device=bins.device)
    plan.exec(_dev.ptr(bins), _dev.ptr(rec))
    _lib.check(_lib.lib().mdsp_est_peak_gather(_dev.ptr(bins), nb, n, int(real), _dev.md_dtype(cdt), _dev.ptr(rec), _dev.ptr(rec) + 16, _dev.stream_ptr()))
    return jacobsen_from_record(rec[2:].cpu().numpy(), n, fs, real)


def quinn(x, *args, tol=1e-6, maxiters=20):
    """``quinn(x)``, ``quinn(x, Fs)``, ``quinn(x, f0, Fs)`` (estimation.jl:153-220), told apart by the argument count as the reference's methods are: the
    frequency of the largest sinusoid in ``x`` by Quinn & Fernandes' iteration (real ``x``) or Quinn's (complex ``x``), from the guess ``f0`` -- ``jacobsen(x, Fs)``
    where none is given; ``Fs`` defaults to 1.0.  Returns ``(estimate, reachedmaxiters)``.  Every iteration is one pass over the signal on the device that
    leaves a record of a few Float64 sums (``mdsp_quinn_estimate``); the filtered signal is never stored.  A final ``|beta| > 2`` raises ``DomainError`` as the
    reference's ``acos`` does; a NaN runs to ``maxiters`` and gives ``(nan, True)``."""
    if len(args) > 2:
        raise TypeError(f"quinn: at most three positional arguments (x, f0, Fs), got {1 + len(args)}")
    x, W, n = _vector(x, "quinn")
    fs = _fs(args[-1], "quinn") if args else 1.0
    f0 = _fs(args[0], "quinn") if len(args) == 2 else None
    if isinstance(maxiters, bool) or not isinstance(maxiters, numbers.Integral):
        raise TypeError("quinn: maxiters must be an integer")
    tol = _fs(tol, "quinn")
    _lib.require_device()
    xd = _dev.as_device(x, W).contiguous()
    if f0 is None:
        f0 = jacobsen(xd, fs)
    plan = _plancache.plans.get(("quinn", _plancache.ctx_key(), W.str, n), lambda: QuinnPlan(W, n))
    est, reached, _ = plan.estimate(_dev.ptr(xd), f0, fs, tol, int(maxiters))
    return est, reached


ESPRIT_MAX_M = 1024      # the largest correlation matrix esprit takes: a cap on the host eigenproblem and on the 16 MiB of R, not on the kernels


class GramPlan:
    """``mdsp_hankel_gram_plan`` for vectors of ``n`` samples of ``dtype`` and ``M`` rows: ``segments``, ``seglen``, ``tile``, ``lag_group``, ``workspace_bytes``.
    ``segments`` = 0 lets the library cut the body range; a positive value forces the cut (tests, tools/esprit_bench.py)."""

    def __init__(self, dtype, n, M, segments=0):
        self._h = C.c_void_p()
        self.dtype, self.n, self.M = np.dtype(dtype), int(n), int(M)
        self.out_dtype = np.dtype(np.complex128 if self.dtype.kind == "c" else np.float64)
        _lib.check(_lib.lib().mdsp_hankel_gram_plan_create(C.byref(self._h), _dev.md_dtype(self.dtype), self.n, self.M, int(segments)))
        S, seglen, tile, group, ws = (C.c_int64() for _ in range(5))
        _lib.check(_lib.lib().mdsp_hankel_gram_plan_info(self._h, C.byref(S), C.byref(seglen), C.byref(tile), C.byref(group), C.byref(ws)))
        self.segments, self.seglen, self.tile, self.lag_group, self.workspace_bytes = S.value, seglen.value, tile.value, group.value, ws.value

    def exec(self, x_ptr: int, r_ptr: int, ldr: int | None = None, stream: int | None = None):
        """``R`` (``M x M``, column-major, leading dimension ``ldr`` -- ``M`` where none is given --, elements of ``out_dtype``) goes to ``r_ptr``."""
        _lib.check(_lib.lib().mdsp_hankel_gram_exec(self._h, x_ptr, r_ptr, self.M if ldr is None else int(ldr), _dev.stream_ptr() if stream is None else stream))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().mdsp_hankel_gram_plan_destroy(self._h)
        except Exception:
            pass


def hankel_gram_geometry(dtype, n: int, M: int, segments: int = 0):
    """(segments, seglen, tile, lag_group, workspace_bytes) a plan for these arguments has: host arithmetic of the library, no device needed."""
    S, seglen, tile, group, ws = (C.c_int64() for _ in range(5))
    _lib.check(_lib.lib().mdsp_hankel_gram_geometry_for(_dev.md_dtype(dtype), int(n), int(M), int(segments), C.byref(S), C.byref(seglen), C.byref(tile),
                                                        C.byref(group), C.byref(ws)))
    return S.value, seglen.value, tile.value, group.value, ws.value


def _integer(v, what, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError(f"{what}: {name} must be an integer, got {type(v).__name__}")
    return int(v)


def _signal(x, what):
    """(x, working dtype) of an array of numbers, before any device work."""
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    dt = _dev.np_dtype_of(x)
    if dt.kind not in "fciub":
        raise TypeError(f"{what}: an array of numbers expected")
    if dt == np.dtype(np.float16):
        raise UnsupportedError(f"{what}: element type {dt} is not accelerated")
    return x, _work_dtype(dt, what)


def hankel_gram(x, M):
    """``R = X X^H`` of the Hankel matrix ``X[i, k] = x[i + k]`` with ``M`` rows and ``N - M + 1`` columns (estimation.jl:70) of a vector ``x``: ``M x M``, Float64
    for a real signal and ComplexF64 for a complex one, exactly Hermitian.  Numpy in gives numpy out, a device tensor in gives a device tensor out (a
    column-major view).  ``1 <= M`` and ``2 M - 1 <= N``."""
    x, W = _signal(x, "hankel_gram")
    if len(x.shape) != 1:
        raise TypeError("hankel_gram: a vector of numbers expected")
    M, n = _integer(M, "hankel_gram", "M"), int(x.shape[0])
    if M < 1:
        raise ArgumentError(f"hankel_gram: M >= 1 is needed (got {M})")
    if 2 * M - 1 > n:
        raise UnsupportedError(f"hankel_gram: 2 M - 1 <= N is needed (M = {M}, N = {n})")
    _lib.require_device()
    xd = _dev.as_device(x, W).contiguous()
    plan = _plancache.plans.get(("hankel_gram", _plancache.ctx_key(), W.str, n, M), lambda: GramPlan(W, n, M))
    r = _dev.torch.empty((M, M), dtype=_dev.torch_dtype(plan.out_dtype), device=xd.device)
    plan.exec(_dev.ptr(xd), _dev.ptr(r))
    r = r.t()                                                                          # the library wrote columns
    return r if _dev.is_device_array(x) else r.cpu().numpy()


def esprit_from_gram(R, p: int, fs: float = 1.0) -> np.ndarray:
    """The host finish of ``esprit`` (estimation.jl:71-74) from the Gram matrix: the ``p`` eigenvectors of the largest eigenvalues of ``R`` span what the first
    ``p`` left singular vectors of the Hankel matrix span, and the eigenvalues of ``U[:-1] \\ U[1:]`` do not depend on the basis.  Float64 vector of length ``p``."""
    R = np.asarray(R)
    if not np.isfinite(R).all():
        raise ArgumentError("esprit: the signal holds Infs or NaNs")                  # the reference's svd refuses them before LAPACK
    _, V = np.linalg.eigh(R)                                                           # eigenvalues ascending
    U = V[:, ::-1][:, :p]
    psi = np.linalg.lstsq(U[:-1], U[1:], rcond=None)[0]
    return np.asarray(np.angle(np.linalg.eigvals(psi)) * (fs / (2 * np.pi)), dtype=np.float64)


def esprit(x, M, p, Fs=1.0) -> np.ndarray:
    """``esprit(x, M, p, Fs=1.0)`` (estimation.jl:67-75): the frequencies of ``p`` cisoids in ``x`` from the signal subspace of the ``M x (N - M + 1)`` Hankel matrix
    of ``x``.  The reference takes the subspace from an SVD of that matrix; here the device forms its ``M x M`` Gram matrix in Float64 (``hankel_gram``), and the
    host takes ``eigh`` of it, the ``p`` leading eigenvectors, ``lstsq`` and ``eigvals``.  Squaring the singular values loses a component whose singular value is
    below about ``sqrt(eps)`` of the largest.  The order of the frequencies is unspecified, as in the reference.

    ``x`` has at most one non-singleton dimension.  ``p < 1`` or ``M > N``: ``ArgumentError`` (a ``BoundsError`` in the reference).  ``p >= M`` (the reference solves an
    under-determined system), ``2 M - 1 > N`` and ``M > ESPRIT_MAX_M``: ``UnsupportedError``.  Infs and NaNs: ``ArgumentError``."""
    x, W = _signal(x, "esprit")
    if sum(int(s) != 1 for s in x.shape) > 1:
        raise ArgumentError("`x` must be a 1D signal")
    M, p, fs = _integer(M, "esprit", "M"), _integer(p, "esprit", "p"), _fs(Fs, "esprit")
    n = 1
    for s in x.shape:
        n *= int(s)
    if p < 1 or M < 1 or M > n:
        raise ArgumentError(f"esprit: p >= 1 and 1 <= M <= N are needed (M = {M}, p = {p}, N = {n})")
    if p >= M:
        raise UnsupportedError(f"esprit: p < M is needed (M = {M}, p = {p})")
    if 2 * M - 1 > n:
        raise UnsupportedError(f"esprit: 2 M - 1 <= N is needed (M = {M}, N = {n})")
    if M > ESPRIT_MAX_M:
        raise UnsupportedError(f"esprit: M <= {ESPRIT_MAX_M} is needed (got {M})")
    _lib.require_device()
    R = hankel_gram(_dev.as_device(x, W).reshape(-1), M)
    return esprit_from_gram(R.cpu().numpy(), p, fs)
