// What more than one spectral unit compiles into device code or launch templates: the window product, the framing kernel K4 of the rocFFT engine
// (spectral.hip mdsp_frames, welch.hip, stft.hip), and the argument block, geometry, unit schedule and grid of the register-resident power-of-two kernels
// (welch.hip, stft.hip).  Everything here has internal linkage, as the kernels that take SpecArgs have: each including unit compiles its own copy.
// Internal to the library.
#pragma once

#include <algorithm>

#include "common.h"
#include "fft_lds.h"

namespace {

using mdsp::fft::cx;

template <typename T> struct real_of { using type = T; };
template <typename R> struct real_of<cx<R>> { using type = R; };

// Float64 window product, rounded once (periodograms.jl:66 `x.buf[i] = x.s[offset+i] * window[i]`)
__device__ __forceinline__ float win_mul(float s, double w) { return (float)((double)s * w); }
__device__ __forceinline__ double win_mul(double s, double w) { return s * w; }
__device__ __forceinline__ cx<float> win_mul(cx<float> s, double w) { return {(float)((double)s.x * w), (float)((double)s.y * w)}; }
__device__ __forceinline__ cx<double> win_mul(cx<double> s, double w) { return {s.x * w, s.y * w}; }

// K4: frames [f0, f0+count) of channel `ch` (unit u = ch*K + f) -> fr[(u-u0)*nfft + i]
template <typename T>
__global__ __launch_bounds__(256) void frame_window_kernel(const T* __restrict__ s, T* __restrict__ fr, const double* __restrict__ win,
                                                           int64_t lds_, int64_t K, int64_t hop, int n, int nfft, int64_t u0, int64_t nunits) {
    const int64_t u = u0 + blockIdx.x;
    if (u >= nunits) return;
    const int64_t ch = u / K, f = u - ch * K;
    const T* src = s + ch * lds_ + f * hop;
    T* dst = fr + (int64_t)blockIdx.x * nfft;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < nfft; i += gridDim.y * blockDim.x) {
        T v{};
        if (i < n) v = win ? win_mul(src[i], win[i]) : src[i];
        dst[i] = v;
    }
}

// LDS padding of the workgroup FFT: one element per 2^shift.  4 everywhere except the two headline geometries, where 5 measured
// faster (Welch nfft = 4096 E = 16: +5 %; overlap-save nfft = 2048: +3 %; the STFT nfft = 1024 kernel loses 7 % with 5).
template <typename R> constexpr int pad_default() { return 4; }

struct SpecArgs {
    const void* s;
    void* out;             // Welch: double partials [slot][ch][N];  STFT: output matrix
    const void* table;     // N forward roots
    const double* win;     // n doubles or nullptr
    int64_t len, lds_, K, hop;
    int64_t units_per_ch;  // frame pairs (real Welch) or frames
    int64_t nch;
    int64_t ldo, chs;      // STFT output strides
    int n, nout, onesided;
    int64_t run_len, niter;  // unit schedule: runs of run_len consecutive units per slot, niter iterations per slot
    int ablate;              // profiling aid (MDSP_ABLATE): 1 skip HBM loads, 2 skip transforms, 4 skip accumulate/stores
    int memprio;             // MDSP_SPEC_PRIO: bit 0 a Welch unit's loads, bit 1 the STFT column stores are issued at raised wave priority
    int accumulate;          // STFT PSD mode: add to the output column instead of overwriting it (multitaper)
    int ntapers;             // > 0: multitaper PSD in one launch (stft_pair_kernel<MT>): win holds ntapers windows of n doubles, rinv their 1/r
    const double* rinv;
    double r;
};

// Load E window values for the thread (zero past n so that the zero tail needs no branch later)
template <int E, int T> __device__ __forceinline__ void load_window_regs(double (&w)[E], const double* win, int n, int t) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = t + T * e;
        w[e] = i < n ? (win ? win[i] : 1.0) : 0.0;
    }
}

// geometry shared by the fused launchers
template <typename R, int N> struct Geo {
    static constexpr bool DBL = sizeof(R) == 8;
    // 8 elements per thread in general; nfft = 1024 in Float32 takes 16 so that a transform is ONE wavefront (no s_barrier)
#ifndef MDSP_GEO_E1024
#define MDSP_GEO_E1024 16
#endif
    static constexpr int EMAX = (N == 1024 && !DBL) ? MDSP_GEO_E1024 : 8;
    static constexpr int E = (N / 64 < EMAX) ? N / 64 : EMAX;
    static constexpr int T = N / E;
    static constexpr int G = mdsp::slots_per_workgroup(T);
    static constexpr int NBUF = T <= 64 ? 1 : 2;
#ifndef MDSP_TW_F64
#define MDSP_TW_F64 1
#endif
    static constexpr int TWREG = DBL ? MDSP_TW_F64 : 1;   // Float64 twiddles: 1 = registers, 0 = global table
};

// runs of consecutive units per slot (default: one run = fully contiguous), identical trip count for every slot
void set_schedule(SpecArgs& a, int64_t nunits, int64_t nslots) {
    a.ablate = MDSP_DBG(ablate);
    a.memprio = mdsp::tunables().spec_prio;
    const int64_t runs = mdsp::tunables().runs_per_slot;
    a.run_len = std::max<int64_t>(1, mdsp::cdiv(nunits, nslots * runs));
    a.niter = mdsp::cdiv(mdsp::cdiv(nunits, a.run_len), nslots) * a.run_len;
}

template <typename K> int grid_for(K kern, int threads, int64_t work_wgs, int64_t nch, int* grid) {
    int per_cu = 0;
    MDSP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0));
    if (per_cu < 1) per_cu = 1;
    if (mdsp::tunables().wg_per_cu > 0) per_cu = mdsp::tunables().wg_per_cu;
    const int64_t resident = (int64_t)mdsp::device_cu_count() * per_cu;
    const int64_t per_ch = std::max<int64_t>(1, resident / std::max<int64_t>(1, nch));
    *grid = (int)std::max<int64_t>(1, std::min<int64_t>(work_wgs, per_ch));
    return MDSP_OK;
}

}  // namespace
