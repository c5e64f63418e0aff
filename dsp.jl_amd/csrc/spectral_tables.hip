// Root and window tables of the spectral plans (spectral_tables.h).
#include "spectral_tables.h"

using namespace mdsp;

namespace {
template <typename T> int upload(DevBuf& buf, const std::vector<T>& v) {
    MDSP_TRY(buf.reserve(sizeof(T) * v.size()));
    MDSP_HIP(hipMemcpy(buf.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return MDSP_OK;
}

template <typename R> __global__ __launch_bounds__(256) void window_kernel(const double* __restrict__ win, R* __restrict__ out, int n, int nfft) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < nfft) out[i] = i < n ? (win ? (R)win[i] : (R)1) : (R)0;
}
}  // namespace

namespace mdsp {
int upload_roots(DevBuf& buf, bool dbl, int64_t n) { return dbl ? upload(buf, root_table<double>(n)) : upload(buf, root_table<float>(n)); }

int upload_window(DevBuf& buf, bool dbl, const double* win_host, int n, int64_t nfft) {
    return dbl ? upload(buf, working_window<double>(win_host, n, nfft)) : upload(buf, working_window<float>(win_host, n, nfft));
}

int convert_window(DevBuf& buf, bool dbl, const double* win_dev, int n, int64_t nfft, hipStream_t st) {
    MDSP_TRY(buf.reserve((dbl ? sizeof(double) : sizeof(float)) * (size_t)nfft));
    const dim3 grid((unsigned)cdiv(nfft, 256));
    if (dbl) hipLaunchKernelGGL(window_kernel<double>, grid, dim3(256), 0, st, win_dev, buf.as<double>(), n, (int)nfft);
    else hipLaunchKernelGGL(window_kernel<float>, grid, dim3(256), 0, st, win_dev, buf.as<float>(), n, (int)nfft);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}
}  // namespace mdsp
