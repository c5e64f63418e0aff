"""numpy restatement of the reference's src/estimation.jl (jacobsen :93-115, quinn :157-220), line by line, for the estimation tests.

Two forms: Float64 (``np.float64`` -- what the reference computes for a Float64 signal, without fused multiply-adds) and ``np.longdouble``, the
yardstick the error figures are measured against.  ``quinn_pass_*`` is ONE iteration's loop over the signal with the sums the device's record holds;
``quinn`` is the whole method.  The mean is an argument of the passes so that both forms and the device remove the same one."""
import numpy as np


def fftfreq(n, fs, k):
    """AbstractFFTs.fftfreq(n, fs)[k], k 0-based."""
    return (k if k < (n + 1) // 2 else k - n) * (fs / n)


def jacobsen(x, fs=1.0):
    """estimation.jl:93-115."""
    x = np.asarray(x)
    n = len(x)                                                   # :94
    X = np.fft.fft(x.astype(np.complex128))                      # :95
    k = int(np.argmax(np.abs(X)))                                # :96 findmax: the first maximum
    fpeak = fftfreq(n, fs, k)                                    # :97
    if k == n - 1:                                               # :98-100
        xm, xp = X[n - 2], X[0]
    elif k == 0:                                                 # :101-103
        xp, xm = X[1], X[n - 1]
    else:                                                        # :104-106
        xp, xm = X[k + 1], X[k - 1]
    delta = -((xp - xm) / (2 * X[k] - xm - xp)).real             # :108
    est = fpeak + delta * fs / n                                 # :109
    return abs(est) if x.dtype.kind != "c" else est              # :111-114


def quinn_pass_real(x, mean, alpha, ftype=np.float64):
    """estimation.jl:176-182 for one alpha: (num, den, xi_1, xi_2) with beta = (xi_2 / xi_1 + num) / den; num = sum_{t=3..N} (xi_t + xi_(t-2)) xi_(t-1),
    den = sum_{t=1..N-1} xi_t^2 (serial sums, in ``ftype``)."""
    F = ftype
    d = np.asarray(x).astype(F) - F(mean)                        # :164
    a = F(alpha)
    n = len(d)
    xi = np.zeros(n, dtype=F)
    xi[0] = d[0]                                                 # :171
    xi[1] = a * xi[0] + d[1]                                     # :176
    num = F(0)
    for t in range(2, n):                                        # :178-181
        xi[t] = d[t] + (a * xi[t - 1] - xi[t - 2])
        num = (xi[t] + xi[t - 2]) * xi[t - 1] + num
    den = F(0)
    for t in range(n - 1):                                       # :182 sum(abs2, xi[1:end-1])
        den = den + xi[t] * xi[t]
    return num, den, xi[0], xi[1]


def quinn_pass_complex(x, mean, omega, ftype=np.float64):
    """estimation.jl:205-212 for one omega: (S, den), S = sum_{t=2..N} x_t conj(xi_(t-1)), den = sum_{t=1..N-1} |xi_t|^2."""
    F = ftype
    C = np.clongdouble if F is np.longdouble else np.complex128
    d = np.asarray(x).astype(C) - C(mean)                        # :196
    c = C(np.cos(F(omega)) + 1j * np.sin(F(omega)))              # :206
    n = len(d)
    xi = np.zeros(n, dtype=C)
    xi[0] = d[0]                                                 # :200
    S = C(0)
    for t in range(1, n):                                        # :207-210
        xi[t] = d[t] + c * xi[t - 1]
        S = S + d[t] * np.conj(xi[t - 1])
    den = F(0)
    for t in range(n - 1):                                       # :212
        den = den + (xi[t].real * xi[t].real + xi[t].imag * xi[t].imag)
    return S, den


def quinn(x, f0, fs, tol=1e-6, maxiters=20, ftype=np.float64):
    """estimation.jl:157-220: (estimate, reachedmaxiters, iterations)."""
    F = ftype
    x = np.asarray(x)
    cplx = x.dtype.kind == "c"
    fn = F(fs) / 2                                               # :158 / :191
    w = F(np.pi) * F(f0) / fn                                    # :161 / :193
    mean = x.astype(np.clongdouble if cplx else np.longdouble).sum() / len(x)
    mean = complex(mean) if cplx else float(mean)
    it = 0
    if not cplx:
        alpha = 2 * np.cos(w)                                    # :168
        beta = F(0)
        for it in range(1, maxiters + 1):                        # :175
            num, den, xi1, xi2 = quinn_pass_real(x, mean, alpha, F)
            beta = (xi2 / xi1 + num) / den                       # :177, :180, :182
            if abs(alpha - beta) < tol:                          # :183
                break
            alpha = 2 * beta - alpha                             # :184
        return float(fn * np.arccos(0.5 * beta) / F(np.pi)), it == maxiters, it      # :187
    for it in range(1, maxiters + 1):                            # :204
        S, den = quinn_pass_complex(x, mean, w, F)
        num = (S * np.conj(np.cos(w) + 1j * np.sin(w))).imag     # :211
        w = w + 2 * num / den                                    # :213
        if abs(2 * num / den) < tol:                             # :216
            break
    return float(fn * w / F(np.pi)), it == maxiters, it          # :219
