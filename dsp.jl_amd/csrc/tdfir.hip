// Time-domain FIR: the stateful DF2TFilter form (mdsp_tdfir_state_exec*), filtfilt's odd extension (mdsp_extrapolate) and the stateless filt(b, 1, x) /
// tdfilt (mdsp_tdfir_exec*), which runs a cached FIRFilter of fir.hip from a zero state.
//
// Stateful time-domain FIR: DF2TFilter{PolynomialRatio} with a = [1] (Filters/filt.jl:153-181) advanced by
// _filt_fir! (dspbase.jl:95-105).  The state si[0..nb-2] is the TDF-II register file, NOT an input history:
//     y[n]   = fma(x[n], b0, fma(x[n-1], b1, ... start))            start = si0[n]                (n <  nb-1)
//                                                                       = b[nb-1] * x[n-nb+1]      (n >= nb-1)
//     si'[j] = fma(x[N-1], b[j+1], fma(x[N-2], b[j+2], ... start))  start = si0[j+N]              (N <= nb-2-j)
//                                                                       = b[nb-1] * x[N-1-(nb-2-j)] otherwise
// -- the same innermost-first accumulation order the serial recursion produces, so outputs and state agree with
// the reference to the last fused-multiply-add.
#include <algorithm>
#include <string>

#include "fir_plan.h"
#include "fir_op.h"

using namespace mdsp;
using namespace mdsp::firop;
using mdsp::fft::cx;

namespace {

template <typename A, typename R>
MDSP_NO_LSO __global__ __launch_bounds__(256) void tdfir_state_out_kernel(const A* __restrict__ x, const A* __restrict__ si0, A* __restrict__ y, const R* __restrict__ b,
                                                              int64_t nx, int64_t ldx, int64_t ldy, int nb) {
    const int64_t col = blockIdx.y;
    const A* xc = x + col * ldx;
    const A* sc = si0 + col * (int64_t)(nb - 1);
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < nx; n += (int64_t)gridDim.x * blockDim.x) {
        A acc;
        int k;
        if (n < nb - 1) {
            acc = sc[n];
            k = (int)n;
        } else {
            acc = mul_first(b[nb - 1], xc[n - (nb - 1)]);
            k = nb - 2;
        }
        for (; k >= 0; --k) fma_acc(acc, b[k], xc[n - k]);
        y[col * ldy + n] = acc;
    }
}

// one workgroup per column; every thread first computes its new registers (reading the OLD state), then all write
template <typename A, typename R>
MDSP_NO_LSO __global__ __launch_bounds__(256) void tdfir_state_next_kernel(const A* __restrict__ x, A* __restrict__ si, const R* __restrict__ b, int64_t N, int64_t ldx,
                                                               int nb) {
    constexpr int MAXPER = 16;   // nb - 1 <= 256 * MAXPER
    const int64_t col = blockIdx.x;
    const A* xc = x + col * ldx;
    A* sc = si + col * (int64_t)(nb - 1);
    A res[MAXPER];
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int j = threadIdx.x + 256 * q;
        if (j >= nb - 1) break;
        const int span = nb - 2 - j;             // largest m with b[j+1+m] defined
        A acc;
        int64_t m;
        if (N <= span) {
            acc = sc[j + N];
            m = N - 1;
        } else {
            acc = mul_first(b[nb - 1], xc[N - 1 - span]);
            m = span - 1;
        }
        for (; m >= 0; --m) fma_acc(acc, b[j + 1 + m], xc[N - 1 - m]);
        res[q] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < MAXPER; ++q) {
        const int j = threadIdx.x + 256 * q;
        if (j >= nb - 1) break;
        sc[j] = res[q];
    }
}

// extrapolate_signal! (Filters/filt.jl:243-257): out = [2 x[1] .- x[pad+1:-1:2]; x; 2 x[end] .- x[end-1:-1:end-pad]]
template <typename A>
MDSP_NO_LSO __global__ __launch_bounds__(256) void extrapolate_kernel(const A* __restrict__ x, A* __restrict__ out, int64_t n, int64_t ldx, int64_t ldo, int64_t pad) {
    const int64_t col = blockIdx.y;
    const A* xc = x + col * ldx;
    A* oc = out + col * ldo;
    const int64_t total = n + 2 * pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        A v;
        if (i < pad) v = sub2(xc[0], xc[pad - i]);                     // 1-based: out[i] = 2 sig[1] - sig[2 + pad - i]
        else if (i < pad + n) v = xc[i - pad];
        else v = sub2(xc[n - 1], xc[n - 1 - (i - pad - n + 1)]);     // out[n + pad + i'] = 2 sig[n] - sig[n - i']
        oc[i] = v;
    }
}

// Device copies of the taps of the recently used stateful filters: a streaming caller passes the same coefficients chunk after chunk
// (often one sample at a time), so the upload -- and any allocation -- happens once per filter, not once per call.  Entries live in the
// library's LRU (plancache.hip), keyed by (device, thread, stream, tap bytes): filters with different taps that alternate each keep
// their buffer, nothing synchronises the device, and no lock is held across a launch.
template <typename A, typename R>
int tdfir_state_run(const void* taps_host, int64_t nb, const void* x, int64_t nx, int64_t ncols, int64_t ldx, void* y, int64_t ldy, void* si, hipStream_t st) {
    const size_t bytes = sizeof(R) * (size_t)nb;
    std::string key = plan_cache_key('t', st);
    key.append(static_cast<const char*>(taps_host), bytes);
    void* h = nullptr;
    MDSP_TRY(plan_cache_get(key, &h,
                            [&](void** out) -> int {
                                auto buf = new DevBuf();
                                int rc = buf->reserve(bytes);
                                if (rc == MDSP_OK && hipMemcpyAsync(buf->p, taps_host, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
                                    rc = set_error(MDSP_ERR_DEVICE, "tap upload failed");
                                if (rc == MDSP_OK && hipStreamSynchronize(st) != hipSuccess) rc = set_error(MDSP_ERR_DEVICE, "tap upload failed");   // taps_host may be freed on return
                                if (rc != MDSP_OK) { delete buf; return rc; }
                                *out = buf;
                                return MDSP_OK;
                            },
                            [](void* p) { delete static_cast<DevBuf*>(p); }));
    const R* taps = static_cast<DevBuf*>(h)->as<R>();
    if (nx > 0) {
        const dim3 g((unsigned)std::min<int64_t>(cdiv(nx, 256), 4096), (unsigned)ncols);
        hipLaunchKernelGGL((tdfir_state_out_kernel<A, R>), g, dim3(256), 0, st, (const A*)x, (const A*)si, (A*)y, taps, nx, ldx, ldy, (int)nb);
        MDSP_LAUNCH_CHECK();
        hipLaunchKernelGGL((tdfir_state_next_kernel<A, R>), dim3((unsigned)ncols), dim3(256), 0, st, (const A*)x, (A*)si, taps, nx, ldx, (int)nb);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

template <typename A> int extrapolate_run(const void* x, int64_t n, int64_t ncols, int64_t ldx, void* out, int64_t ldo, int64_t pad, hipStream_t st) {
    const dim3 g((unsigned)std::min<int64_t>(cdiv(n + 2 * pad, 256), 65535), (unsigned)ncols);
    hipLaunchKernelGGL(extrapolate_kernel<A>, g, dim3(256), 0, st, (const A*)x, (A*)out, n, ldx, ldo, pad);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

extern "C" {

// The promotion of a tap dtype and a signal dtype (promote_type): complex if either is, double if either is.
static int tdfir_promote(int taps_dtype, int x_dtype) {
    const bool dbl = dtype_is_double(taps_dtype) || dtype_is_double(x_dtype), c = dtype_is_complex(taps_dtype) || dtype_is_complex(x_dtype);
    return c ? (dbl ? MDSP_C64 : MDSP_C32) : (dbl ? MDSP_F64 : MDSP_F32);
}

int mdsp_tdfir_state_exec_t(const void* taps_host, int64_t nb, int taps_dtype, int x_dtype, const void* x_dev, int64_t nx, int64_t ncols, int64_t ldx,
                            void* y_dev, int64_t ldy, void* si_dev, void* stream) {
    if (!taps_host || nb < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter vector b must be non-empty");
    if (!dtype_valid(taps_dtype) || !dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    // x, y and the state are all of the promoted dtype, which the signal must already have (the state IS of the output's type, filt.jl:149-151)
    if (tdfir_promote(taps_dtype, x_dtype) != x_dtype) MDSP_FAIL(MDSP_ERR_ARGUMENT, "x_dtype must be the promotion of the tap and signal dtypes");
    if (!dtype_is_complex(taps_dtype)) {
        if (taps_dtype != dtype_real_of(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "real taps must be in the precision of x_dtype");
        return mdsp_tdfir_state_exec(taps_host, nb, x_dtype, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, stream);
    }
    if (taps_dtype != x_dtype) MDSP_FAIL(MDSP_ERR_ARGUMENT, "complex taps must be in the precision of x_dtype");
    if (nx < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (nb < 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "a one-tap filter has no state; scale the signal instead");
    if (nb - 1 > 256 * 16) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "stateful time-domain FIR supports at most 4097 taps");
    if (nx == 0 || ncols == 0) return MDSP_OK;
    if (ncols > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 columns per call");
    if (!x_dev || !y_dev || !si_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    hipStream_t st = as_stream(stream);
    if (x_dtype == MDSP_C32) return tdfir_state_run<cx<float>, cx<float>>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
    return tdfir_state_run<cx<double>, cx<double>>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
}

int mdsp_tdfir_state_exec(const void* taps_host, int64_t nb, int dtype, const void* x_dev, int64_t nx, int64_t ncols, int64_t ldx, void* y_dev,
                          int64_t ldy, void* si_dev, void* stream) {
    if (!taps_host || nb < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter vector b must be non-empty");
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    if (nx < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (nb < 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "a one-tap filter has no state; scale the signal instead");   // mul!(out, x, b[1]), filt.jl:163
    if (nb - 1 > 256 * 16) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "stateful time-domain FIR supports at most 4097 taps");
    if (nx == 0 || ncols == 0) return MDSP_OK;
    if (ncols > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 columns per call");
    if (!x_dev || !y_dev || !si_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    hipStream_t st = as_stream(stream);
    switch (dtype) {
        case MDSP_F32: return tdfir_state_run<float, float>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
        case MDSP_F64: return tdfir_state_run<double, double>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
        case MDSP_C32: return tdfir_state_run<cx<float>, float>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
        default: return tdfir_state_run<cx<double>, double>(taps_host, nb, x_dev, nx, ncols, ldx, y_dev, ldy, si_dev, st);
    }
}

int mdsp_extrapolate(const void* x_dev, int64_t n, int64_t ncols, int64_t ldx, int dtype, int64_t pad, void* out_dev, int64_t ldo, void* stream) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    if (n < 1 || pad < 0 || pad > n - 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "pad_length must be in [0, length(x) - 1]");     // sig[2 + pad - i] must exist
    if (ldo < n + 2 * pad) MDSP_FAIL(MDSP_ERR_ARGUMENT, "output is incorrectly sized");                               // filt.jl:245
    if (ncols <= 0) return MDSP_OK;
    if (ncols > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 columns per call");
    if (!x_dev || !out_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    hipStream_t st = as_stream(stream);
    switch (dtype) {
        case MDSP_F32: return extrapolate_run<float>(x_dev, n, ncols, ldx, out_dev, ldo, pad, st);
        case MDSP_F64: return extrapolate_run<double>(x_dev, n, ncols, ldx, out_dev, ldo, pad, st);
        case MDSP_C32: return extrapolate_run<cx<float>>(x_dev, n, ncols, ldx, out_dev, ldo, pad, st);
        default: return extrapolate_run<cx<double>>(x_dev, n, ncols, ldx, out_dev, ldo, pad, st);
    }
}

// ---- time-domain FIR: filt(b, a::Number, x) / tdfilt (dspbase.jl:95-105) -------------------------------------
// taps_host: nb REAL taps in the precision of `dtype`; x / y of `dtype`.  Same accumulation order as the TDF-II
// recursion: oldest sample first, one multiply then a chain of fused multiply-adds.
int mdsp_tdfir_exec(const void* taps_host, int64_t nb, int dtype, const void* x_dev, int64_t nx, int64_t ncols, int64_t ldx, void* y_dev,
                    int64_t ldy, void* stream) {
    if (!taps_host || nb < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter vector b must be non-empty");
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    if (nx < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (nx == 0 || ncols == 0) return MDSP_OK;
    if (ncols > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 columns per call");
    // The filter object (device taps, history) comes from the library's LRU, keyed by (device, thread, stream, taps, dtype, columns):
    // repeated filt(b, 1, x) / tdfilt / direct-conv calls allocate and upload nothing, and nothing synchronises the caller's stream.
    std::string key = plan_cache_key('f', stream);
    key.append(reinterpret_cast<const char*>(&dtype), sizeof(dtype));
    key.append(reinterpret_cast<const char*>(&ncols), sizeof(ncols));
    key.append(static_cast<const char*>(taps_host), (size_t)nb * dtype_size(dtype_real_of(dtype)));
    void* h = nullptr;
    MDSP_TRY(plan_cache_get(key, &h, [&](void** out) { return mdsp_fir_create(reinterpret_cast<mdsp_fir*>(out), taps_host, nb, 1, 1, dtype_real_of(dtype), dtype, ncols); },
                            [](void* p) { (void)mdsp_fir_destroy(static_cast<mdsp_fir>(p)); }));
    mdsp_fir f = static_cast<mdsp_fir>(h);
    MDSP_TRY(fir_reset_on(f, as_stream(stream), true));   // zero initial state: every call is a fresh filt(b, a, x)
    int64_t nw = 0;
    return mdsp_fir_exec(f, x_dev, nx, ldx, y_dev, nx, ldy, &nw, stream);
}

// The same with an explicit tap dtype (real or complex) next to the signal's: x of x_dtype, y of promote_type(taps_dtype, x_dtype).  Complex taps take the
// plain complex product (no conjugate), oldest sample first.
int mdsp_tdfir_exec_t(const void* taps_host, int64_t nb, int taps_dtype, int x_dtype, const void* x_dev, int64_t nx, int64_t ncols, int64_t ldx,
                      void* y_dev, int64_t ldy, void* stream) {
    if (!taps_host || nb < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter vector b must be non-empty");
    if (!dtype_valid(taps_dtype) || !dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype");
    if (nx < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (nx == 0 || ncols == 0) return MDSP_OK;
    if (ncols > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 columns per call");
    std::string key = plan_cache_key('g', stream);   // (its own key class: the tap dtype is part of the key)
    key.append(reinterpret_cast<const char*>(&taps_dtype), sizeof(taps_dtype));
    key.append(reinterpret_cast<const char*>(&x_dtype), sizeof(x_dtype));
    key.append(reinterpret_cast<const char*>(&ncols), sizeof(ncols));
    key.append(static_cast<const char*>(taps_host), (size_t)nb * dtype_size(taps_dtype));
    void* h = nullptr;
    MDSP_TRY(plan_cache_get(key, &h, [&](void** out) { return mdsp_fir_create(reinterpret_cast<mdsp_fir*>(out), taps_host, nb, 1, 1, taps_dtype, x_dtype, ncols); },
                            [](void* p) { (void)mdsp_fir_destroy(static_cast<mdsp_fir>(p)); }));
    mdsp_fir f = static_cast<mdsp_fir>(h);
    MDSP_TRY(fir_reset_on(f, as_stream(stream), true));   // zero initial state: every call is a fresh filt(b, a, x)
    int64_t nw = 0;
    return mdsp_fir_exec(f, x_dev, nx, ldx, y_dev, nx, ldy, &nw, stream);
}

}  // extern "C"
