"""Restatements for the esprit tests, plain numpy, no device and no library:

  esprit_svd       the reference's algorithm (src/estimation.jl:67-75) with numpy.linalg.svd
  gram_longdouble  the Gram matrix R = X X^H of the Hankel matrix X[i, k] = x[i + k] by its definition, in numpy.longdouble
  gram_serial      the same by a serial Float64 loop in index order: the yardstick the library's order of additions is measured against
  finish           the host finish from a Gram matrix (eigh, the p leading eigenvectors, lstsq, eigvals): the calls of dsp_jl_amd.esprit_from_gram
"""
import numpy as np


def hankel(x, M):
    """X[i, k] = x[i + k], M x (N - M + 1) (estimation.jl:70)."""
    x = np.asarray(x).reshape(-1)
    return np.lib.stride_tricks.sliding_window_view(x, len(x) - M + 1)[:M]


def esprit_svd(x, M, p, Fs=1.0):
    """(frequencies, singular values of the Hankel matrix): estimation.jl:68-74."""
    x = np.asarray(x)
    if sum(s != 1 for s in x.shape) > 1:                                               # :68
        raise ValueError("`x` must be a 1D signal")
    X = hankel(x.reshape(-1).astype(np.complex128 if x.dtype.kind == "c" else np.float64), M)   # :69-70
    U, sv, _ = np.linalg.svd(X, full_matrices=False)                                   # :71
    D = np.linalg.eigvals(np.linalg.lstsq(U[:-1, :p], U[1:, :p], rcond=None)[0])       # :72
    return np.angle(D) * (Fs / (2 * np.pi)), sv                                        # :74


def _wide(x):
    x = np.asarray(x).reshape(-1)
    return x.astype(np.clongdouble if x.dtype.kind == "c" else np.longdouble)


def gram_longdouble(x, M):
    """R[i, j] = sum over k of x[i + k] conj(x[j + k]), k = 0 .. N - M, in long double."""
    X = hankel(_wide(x), M)
    return np.array([[np.sum(X[i] * np.conj(X[j])) for j in range(M)] for i in range(M)])


def gram_serial(x, M):
    """The same in Float64, each entry one running sum over k in ascending order (cumsum adds one term after the other)."""
    x = np.asarray(x).reshape(-1)
    X = hankel(x.astype(np.complex128 if x.dtype.kind == "c" else np.float64), M)
    return np.array([[np.cumsum(X[i] * np.conj(X[j]))[-1] for j in range(M)] for i in range(M)])


def gram_error(R, want):
    """max |R - want| / max |want|, the difference taken in long double."""
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(R).astype(want.dtype) - want)) / np.max(np.abs(want)))


def finish(R, p, Fs=1.0):
    R = np.asarray(R)
    _, V = np.linalg.eigh(R)
    U = V[:, ::-1][:, :p]
    psi = np.linalg.lstsq(U[:-1], U[1:], rcond=None)[0]
    return np.asarray(np.angle(np.linalg.eigvals(psi)) * (Fs / (2 * np.pi)), dtype=np.float64)
