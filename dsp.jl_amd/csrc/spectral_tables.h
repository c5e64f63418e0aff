// The two tables every Welch / STFT kernel family reads: the n forward roots of unity and the window in the working precision.  A plan's tables are built
// ONCE, at plan creation, from host data (upload_roots, upload_window: synchronous copies, no kernel and no stream); convert_window is for the launches whose
// window is a device pointer that changes from launch to launch (complex-signal columns, the tapers of a multitaper plan).
#pragma once

#include <cstdint>
#include <vector>

#include "hostfft.h"

namespace mdsp {
// ---- host only (tests/cpu_harness/spectral_tables.cpp compiles this part with g++) ----------------------------------------------------------------
template <typename R> struct RootPair { R x, y; };   // the layout of fft::cx<R>

// W_n^k = exp(-2 pi i k / n), k < n, rounded from Float64 to R
template <typename R> std::vector<RootPair<R>> root_table(int64_t n) {
    std::vector<RootPair<R>> w((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const zd r = unit_root(k, n, -1);
        w[(size_t)k] = {(R)r.real(), (R)r.imag()};
    }
    return w;
}

// nfft values: the window rounded to R (ones without a window) on i < n, zeros behind
template <typename R> std::vector<R> working_window(const double* win, int n, int64_t nfft) {
    std::vector<R> w((size_t)nfft);
    for (int64_t i = 0; i < nfft; ++i) w[(size_t)i] = i < n ? (win ? (R)win[i] : (R)1) : (R)0;
    return w;
}
}  // namespace mdsp

#ifdef __HIPCC__
#include "common.h"

namespace mdsp {
// buf <- root_table<float | double>(n)
int upload_roots(DevBuf& buf, bool dbl, int64_t n);
// buf <- working_window<float | double>(win_host, n, nfft)
int upload_window(DevBuf& buf, bool dbl, const double* win_host, int n, int64_t nfft);
// the same values from a window on the device, on `st`
int convert_window(DevBuf& buf, bool dbl, const double* win_dev, int n, int64_t nfft, hipStream_t st);
}  // namespace mdsp
#endif
