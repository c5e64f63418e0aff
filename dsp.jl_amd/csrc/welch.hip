// Welch PSD (mdsp_welch_*), the rows form the multi-pass engine calls (mdsp::welch_rows_accumulate) and the cross-channel sum (mdsp_channel_sum).
//
// Reference loops being replaced (src/periodograms.jl; framing and K4: spectral.hip):
//   F3  mul!(outbuf, plan, sig) :754, :888        rfft (real) / fft (complex), out of place
//   K5  fft2pow! :142-172              out[i] = muladd(abs2(X[i]), m, out[i]),  m = 1/r or 2/r
//
// Engines:
//   FUSED  (power-of-two nfft in [256, 8192]): persistent kernel; a transform slot packs TWO real frames into one complex FFT (z = w*(a + i b)),
//             and accumulates |Z[k]|^2 per bin in double in registers.  Since |A[k]|^2 + |B[k]|^2 =
//             (|Z[k]|^2 + |Z[N-k]|^2)/2, no untangling is needed: the fold happens once in the tiny finalize
//             kernel.  HBM traffic = the signal, read once (+ overlap re-reads served by L2).
//          Other sizes: the Welch sums (MODE 0) of spectral_gen.hip, spectral_gx.h, spectral_ct*.hip and bigfft.hip.
//   ROCFFT : K4 kernel -> batched rocFFT -> K5 kernel over cache-sized chunks; any nfft.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "devio.h"
#include "fft_lds.h"
#include "fft_wg.h"
#include "hostfft.h"
#include "rocfft_wrap.h"
#include "spectral_tables.h"
#include "welch_plan.h"
#include "spectral_op.h"
#include "spectral_plan.h"
#include "gx_kernels.h"   // (namespace mdsp::gx and the kernel template: ahead of the anonymous namespace that includes spectral_gx.h)

using namespace mdsp;
using mdsp::fft::cx;

namespace {

// ======================================================================================================
// rocFFT-engine kernels
// ======================================================================================================
// K5 (Welch): partial[slice][ch][k] += sum over this chunk's frames of channel ch of |X[k]|^2   (double)
// grid: (bins/256, nslices, nch).  Frame u of the chunk belongs to slice (u % nslices); deterministic order.
template <typename R>
__global__ __launch_bounds__(256) void abs2_accum_kernel(const cx<R>* __restrict__ spec, double* __restrict__ partial, int nspec, int64_t K,
                                                         int64_t u0, int64_t cnt, int64_t nch) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nspec) return;
    const int64_t ch = blockIdx.z;
    // units of this chunk that belong to channel ch: [max(u0, ch*K), min(u0+cnt, (ch+1)*K))
    const int64_t lo = std::max<int64_t>(u0, ch * K), hi = std::min<int64_t>(u0 + cnt, (ch + 1) * K);
    double acc = 0;
    for (int64_t u = lo + blockIdx.y; u < hi; u += gridDim.y) {
        const cx<R> z = spec[(u - u0) * nspec + k];
        acc += (double)z.x * (double)z.x + (double)z.y * (double)z.y;
    }
    if (lo + (int64_t)blockIdx.y < hi) partial[((int64_t)blockIdx.y * nch + ch) * nspec + k] += acc;
}

// Slice reduction: reduced[ch][k] = sum_s partial[s][ch][k], fixed order (deterministic).  32 bins x 8 slice lanes per
// workgroup so the nslices-long sum is spread over threads instead of being one latency-bound loop per bin.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ partial, double* __restrict__ reduced, int nslices,
                                                              int64_t nch, int nacc, int accumulate) {
    __shared__ double sm[8][33];
    const int bx = threadIdx.x & 31, sy = threadIdx.x >> 5;
    const int k = blockIdx.x * 32 + bx;
    const int64_t ch = blockIdx.y;
    double a = 0;
    if (k < nacc)
        for (int s = sy; s < nslices; s += 8) a += partial[((int64_t)s * nch + ch) * nacc + k];
    sm[sy][bx] = a;
    __syncthreads();
    if (sy == 0 && k < nacc) {
        double t = sm[0][bx];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += sm[i][bx];
        reduced[ch * nacc + k] = accumulate ? reduced[ch * nacc + k] + t : t;   // accumulate: a further slice of the same stream
    }
}

// With hundreds of slices (a persistent grid writes one row per workgroup: 1024 rows of nfft doubles are 24-32 MiB) the single kernel above is
// ~100 workgroups walking 128 rows each with 256-byte reads -- 60-120 us behind a 0.3-1.4 ms kernel.  Two steps instead: groups of rows summed by
// (bins / 256) x groups workgroups with 2 KiB reads per wave, then the kernel above over the groups.  Fixed order either way.
constexpr int REDUCE_GROUPS = 64;
__global__ __launch_bounds__(256) void reduce_partials_groups_kernel(const double* __restrict__ partial, double* __restrict__ tmp, int nslices, int64_t nch, int nacc,
                                                                     int per_group) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int g = blockIdx.y;
    const int64_t ch = blockIdx.z;
    if (k >= nacc) return;
    const int s0 = g * per_group, s1 = min(nslices, s0 + per_group);
    double a = 0;
#pragma unroll 4
    for (int s = s0; s < s1; ++s) a += partial[((int64_t)s * nch + ch) * nacc + k];
    tmp[((int64_t)g * nch + ch) * nacc + k] = a;
}
inline int reduce_partials(mdsp_welch_plan_s* pl, const double* partial, double* reduced, int nslices, int64_t nch, int nacc, int accumulate, hipStream_t st) {
    if (nslices > 2 * REDUCE_GROUPS) {
        const int per_group = (int)cdiv(nslices, REDUCE_GROUPS), ng = (int)cdiv(nslices, per_group);
        MDSP_TRY(pl->redtmp.reserve(sizeof(double) * (size_t)ng * (size_t)nch * (size_t)nacc));
        hipLaunchKernelGGL(reduce_partials_groups_kernel, dim3((unsigned)cdiv(nacc, 256), (unsigned)ng, (unsigned)nch), dim3(256), 0, st, partial, pl->redtmp.as<double>(),
                           nslices, nch, nacc, per_group);
        MDSP_LAUNCH_CHECK();
        partial = pl->redtmp.as<double>();
        nslices = ng;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv(nacc, 32), (unsigned)nch), dim3(256), 0, st, partial, reduced, nslices, nch, nacc, accumulate);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

// Welch finalize: psd[ch][j] = T( m_j * fold(sum over slices) )
//   MODE 0: one-sided from half spectrum  (acc has nspec = nfft/2+1 bins)       m = 1/r (DC, Nyquist if even) else 2/r
//   MODE 1: two-sided from full spectrum  (acc has nfft bins)                   m = 1/r
//   MODE 2: two-sided from half spectrum  (mirror, periodograms.jl:158-168)     m = 1/r
//   MODE 3: one-sided from PAIR-PACKED full spectrum: (A[k] + A[N-k])/2
//   MODE 4: two-sided from PAIR-PACKED full spectrum
template <typename R, int MODE>
__global__ __launch_bounds__(256) void welch_finalize_kernel(const double* __restrict__ partial, R* __restrict__ psd, int64_t ldp, int nslices,
                                                             int64_t nch, int nacc, int nfft, int nout, double r_total, const double* __restrict__ kdev,
                                                             double r_unit) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ch = blockIdx.y;
    if (j >= nout) return;
    if (kdev) {   // frame count summed over ranks on the device (mdsp_welch_allreduce): r = K fs sum(w^2) is formed here
        const double k = *kdev;
        if (!(k > 0)) {   // no frames anywhere: fill!(out, 0)
            psd[ch * ldp + j] = (R)0;
            return;
        }
        r_total = k * r_unit;
    }
    auto sum_bin = [&](int k) {
        double a = 0;
        for (int s = 0; s < nslices; ++s) a += partial[((int64_t)s * nch + ch) * nacc + k];
        return a;
    };
    double v;
    const double m1 = 1.0 / r_total, m2 = 2.0 / r_total;
    if (MODE == 0) {
        v = sum_bin(j) * ((j == 0 || (j == nout - 1 && (nfft % 2 == 0))) ? m1 : m2);
    } else if (MODE == 1) {
        v = sum_bin(j) * m1;
    } else if (MODE == 2) {
        const int k = j <= nfft / 2 ? j : nfft - j;
        v = sum_bin(k) * m1;
    } else {
        const int k2 = (nfft - j) % nfft;
        const double a = 0.5 * (sum_bin(j) + sum_bin(k2));
        if (MODE == 3) v = a * ((j == 0 || (j == nout - 1 && (nfft % 2 == 0))) ? m1 : m2);
        else v = a * m1;
    }
    psd[ch * ldp + j] = (R)v;
}

// ======================================================================================================
// Fused kernels
// ======================================================================================================
// SHIFT > 0 (complex signals; host guarantees n == N and hop == SHIFT * T): the samples a frame shares with its predecessor stay
// in registers, shifted by SHIFT elements per frame -- see stft_fused_kernel (stft.hip).
template <typename R, int N, int E, int G, int TWMODE, int PADSHIFT, bool CPLX, int NBUF, bool WIN64, int SHIFT = 0>
__global__ __launch_bounds__((N / E) * G, 2) void welch_fused_kernel(SpecArgs a) {
    using C = fft::Cfg<N, E>;
    using TT = std::conditional_t<CPLX, cx<R>, R>;
    constexpr int T = C::T;
    static_assert(T % 64 == 0, "a transform must own whole wavefronts");
    constexpr int NTWA = C::NTW > 0 ? C::NTW : 1;
    constexpr int REGION = fft::wg_lds_elems<C, PADSHIFT, NBUF>();
    constexpr int64_t SZ = (int64_t)sizeof(TT);
    __shared__ __attribute__((aligned(16))) cx<R> lds_all[G * REGION];
    const int t = threadIdx.x % T;
    const int slot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / T));  // wave-uniform (T % 64 == 0)
    cx<R>* lds = lds_all + slot * REGION;
    const cx<R>* table = static_cast<const cx<R>*>(a.table);
    const int64_t ch = blockIdx.y;

    cx<R> tw[NTWA];
    __shared__ __attribute__((aligned(16))) cx<R> twl[(TWMODE == fft::TW_LDS || TWMODE == fft::TW_HYB) ? fft::tw_lds_entries<C, TWMODE>() : 1];
    const cx<R>* twsrc = fft::wg_twiddle_setup<C, TWMODE>(tw, twl, t, slot, table);
    std::conditional_t<WIN64, double, R> w[E];
    {
        double wd[E];
        load_window_regs<E, T>(wd, a.win, a.n, t);
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = (std::conditional_t<WIN64, double, R>)wd[e];
    }
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;

    const TT* sc = static_cast<const TT*>(a.s) + ch * a.lds_;
    // Unit schedule (wave-uniform): slot s of S walks runs of run_len consecutive units; run g of slot s starts at unit
    // (g*S + s)*run_len.  Consecutive frames share their n-hop overlap through L1/L2.
    const int64_t nslots = (int64_t)gridDim.x * G;
    int64_t wbase = ((int64_t)blockIdx.x * G + slot) * a.run_len, wj = 0;
    auto unit_cur = [&](bool more) { return (more && wbase + wj < a.units_per_ch) ? wbase + wj : a.units_per_ch; };  // else dead
    auto walk = [&]() {
        if (++wj == a.run_len) {
            wj = 0;
            wbase += nslots * a.run_len;
        }
    };
    const int64_t niter = a.niter;

    TT ra[E];
    TT rb[CPLX ? 1 : E];
    int64_t held = -2;   // SHIFT: frame whose raw samples ra[] holds
    auto issue = [&](int64_t u) {
        const bool live = u < a.units_per_ch;
        const int64_t f0 = CPLX ? u : 2 * u;
        const int64_t start = f0 * a.hop;
        // a frame never reads past start+n: the descriptor ends there (zero tail) or at the end of the signal
        const __amdgpu_buffer_rsrc_t r0 = io::make_rsrc(sc + start, live ? std::min<int64_t>(a.n, a.len - start) * SZ : 0);
        if constexpr (SHIFT > 0) {
            static_assert(CPLX && SHIFT < E, "frame-overlap reuse is wired for complex signals");
            if (live && u == held + 1) {   // wave-uniform: the next frame of the same run
#pragma unroll
                for (int e = 0; e < E - SHIFT; ++e) ra[e] = ra[e + SHIFT];
                io::load_window_tail<TT, E, T, E - SHIFT>(ra, r0, t);
                held = u;
                return;
            }
            held = live ? u : -2;
        }
        io::load_window<TT, E, T>(ra, r0, 0, t);
        if constexpr (!CPLX) {
            const bool haveB = live && (f0 + 1) < a.K;
            const int64_t startB = start + a.hop;
            const __amdgpu_buffer_rsrc_t r1 = io::make_rsrc(sc + startB, haveB ? std::min<int64_t>(a.n, a.len - startB) * SZ : 0);
            io::load_window<TT, E, T>(rb, r1, 0, t);
        }
    };
    int64_t u = unit_cur(niter > 0);
    issue(u);
    for (int64_t it = 0; it < niter; ++it) {
        walk();
        const int64_t unext = unit_cur(it + 1 < niter);
        cx<R> v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if constexpr (CPLX) {
                if constexpr (WIN64) v[e] = win_mul(ra[e], (double)w[e]);
                else v[e] = {ra[e].x * w[e], ra[e].y * w[e]};
            } else {
                if constexpr (WIN64) v[e] = {win_mul(ra[e], (double)w[e]), win_mul(rb[e], (double)w[e])};
                else v[e] = {ra[e] * w[e], rb[e] * w[e]};
            }
        }
        if (!MDSP_ABLATED(a, 1)) issue(unext);   // the next unit's samples stream in while this one is transformed
        u = unext;
        if (!MDSP_ABLATED(a, 2))
        fft::wg_fft<C, -1, TWMODE, PADSHIFT, NBUF, 0>(v, t, tw, twsrc, lds);
        // an odd number of exchanges per iteration would re-enter on the buffer that was used last: fence it
        if constexpr (C::P > 1 && NBUF > 1 && ((C::P - 1) % NBUF) != 0) fft::wg_sync<T>();  // NBUF == 1: wg_fft already ends every exchange with a barrier
        // K5: |Z|^2 in the working precision (one rounding per term), accumulated over frames in double
        if (!MDSP_ABLATED(a, 4)) {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += (double)(v[e].x * v[e].x + v[e].y * v[e].y);
        }
    }
    // partial[(blockIdx.x*G + slot)][ch][k]
    double* part = static_cast<double*>(a.out) + (((int64_t)blockIdx.x * G + slot) * a.nch + ch) * N;
#pragma unroll
    for (int e = 0; e < E; ++e) part[t + T * e] = acc[e];
}

#include "spectral_gx.h"

template <typename R, bool CPLX>
int welch_accumulate_rocfft(mdsp_welch_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, hipStream_t st) {
    using TT = std::conditional_t<CPLX, cx<R>, R>;
    const int64_t nfft = pl->nfft, n = pl->n, hop = pl->n - pl->noverlap;
    const int64_t K = mdsp_frame_count(len, n, pl->noverlap);
    const int nspec = (int)(CPLX ? nfft : nfft / 2 + 1);
    const int64_t nunits = K * nch;
    const int nslices = 32;
    pl->acc_nslices = nslices;
    pl->acc_nacc = nspec;
    pl->acc_mode = CPLX ? 1 : (pl->onesided ? 0 : 2);
    if (pl->acc_fresh) {
        MDSP_TRY(pl->partial.reserve(sizeof(double) * (size_t)nslices * (size_t)nch * (size_t)nspec));
        MDSP_HIP(hipMemsetAsync(pl->partial.p, 0, sizeof(double) * (size_t)nslices * (size_t)nch * (size_t)nspec, st));
        pl->acc_fresh = false;
    }
    if (nunits > 0) {
        const int64_t batch = chunk_units_rocfft_spectral(CPLX, (int64_t)sizeof(R), nfft, nunits, rocfft_chunk_bytes());
        if (pl->batch != batch) {
            MDSP_TRY(pl->fr.reserve((size_t)(sizeof(TT) * nfft * batch)));
            MDSP_TRY(pl->spec.reserve((size_t)(sizeof(cx<R>) * nspec * batch)));
            MDSP_TRY(pl->fwd.create(CPLX ? FftKind::C2C_FWD : FftKind::R2C, sizeof(R) == 8, nfft, batch, false));
            pl->batch = batch;
        }
        const int gx = (int)std::min<int64_t>(cdiv(nfft, 256), 8);
        for (int64_t u0 = 0; u0 < nunits; u0 += batch) {
            const int64_t cnt = std::min<int64_t>(batch, nunits - u0);
            hipLaunchKernelGGL(frame_window_kernel<TT>, dim3((unsigned)cnt, gx), dim3(256), 0, st, (const TT*)s, pl->fr.as<TT>(),
                               pl->have_win ? pl->win.as<double>() : nullptr, lds_, K, hop, (int)n, (int)nfft, u0, nunits);
            MDSP_LAUNCH_CHECK();
            MDSP_TRY(pl->fwd.exec(pl->fr.p, pl->spec.p, st));
            hipLaunchKernelGGL(abs2_accum_kernel<R>, dim3((unsigned)cdiv(nspec, 256), nslices, (unsigned)nch), dim3(256), 0, st,
                               pl->spec.as<cx<R>>(), pl->partial.as<double>(), nspec, K, u0, cnt, nch);
            MDSP_LAUNCH_CHECK();
        }
    }
    return MDSP_OK;
}

// psd[ch][j] = T( m_j * fold(accumulated |X|^2 sums) ), m from r_total = K_total * fs * sum(w^2)  (periodograms.jl:751, :142-172)
template <typename R> int welch_finalize(mdsp_welch_plan_s* pl, int64_t K_total, int64_t nch, void* psd, int64_t ldp, hipStream_t st) {
    const int nout = (int)pl->nout;
    const double* kdev = (K_total == 0 && pl->frames_on_device) ? pl->kdev.as<double>() : nullptr;
    if (K_total <= 0 && !kdev) {  // fill!(out, 0); no frames (0 * r would be a division by zero in m)
        for (int64_t c = 0; c < nch; ++c) MDSP_HIP(hipMemsetAsync((R*)psd + c * ldp, 0, sizeof(R) * (size_t)nout, st));
        return MDSP_OK;
    }
    const double r_total = (double)K_total * pl->r;
    const dim3 grid((unsigned)cdiv(nout, 256), (unsigned)nch);
    const double* acc = pl->acc_ptr();
    const int ns = pl->acc_nslices, na = pl->acc_nacc, nfft = (int)pl->nfft;
#define MDSP_FIN(MODE) hipLaunchKernelGGL((welch_finalize_kernel<R, MODE>), grid, dim3(256), 0, st, acc, (R*)psd, ldp, ns, nch, na, nfft, nout, r_total, kdev, pl->r)
    switch (pl->acc_mode) {
        case 0: MDSP_FIN(0); break;
        case 1: MDSP_FIN(1); break;
        case 2: MDSP_FIN(2); break;
        case 3: MDSP_FIN(3); break;
        default: MDSP_FIN(4); break;
    }
#undef MDSP_FIN
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

// ---- Welch, real input, n == nfft, 50 % overlap (the default `noverlap = n >> 1` and BASELINE config 3) -----------
// With hop = N/2 the second half of frame a IS the first half of frame b, and the second half of frame b IS the first
// half of the next unit's frame a.  A slot that walks consecutive units therefore loads every sample exactly ONCE:
// E loads per thread per unit instead of 2E, and 3E/2 instead of 2E prefetch registers.
template <typename R, int N, int E, int G, int TWMODE, int PADSHIFT, int NBUF>
__global__ __launch_bounds__((N / E) * G, 2) void welch_half_kernel(SpecArgs a) {
    using C = fft::Cfg<N, E>;
    constexpr int T = C::T;
    constexpr int H = E / 2;
    static_assert(T % 64 == 0 && E % 2 == 0, "geometry");
    constexpr int NTWA = C::NTW > 0 ? C::NTW : 1;
    constexpr int REGION = fft::wg_lds_elems<C, PADSHIFT, NBUF>();
    constexpr int64_t SZ = (int64_t)sizeof(R);
    __shared__ __attribute__((aligned(16))) cx<R> lds_all[G * REGION];
    const int t = threadIdx.x % T;   // sample / window ownership before the transform, bin ownership after it: t + T*e
    const int slot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / T));
    cx<R>* lds = lds_all + slot * REGION;
    const cx<R>* table = static_cast<const cx<R>*>(a.table);
    const int64_t ch = blockIdx.y;

    cx<R> tw[NTWA];
    __shared__ __attribute__((aligned(16))) cx<R> twl[(TWMODE == fft::TW_LDS || TWMODE == fft::TW_HYB) ? fft::tw_lds_entries<C, TWMODE>() : 1];
    const cx<R>* twsrc = fft::wg_twiddle_setup<C, TWMODE>(tw, twl, t, slot, table);
    R w[E];
    {
        double wd[E];
        load_window_regs<E, T>(wd, a.win, a.n, t);
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = (R)wd[e];
    }
    // Power accumulators.  Float32: (re^2, im^2) pairs fed by one packed FMA per bin, folded into the slot's Float64
    // partial row every FLUSH units (the reference accumulates in Float32 over ALL frames, periodograms.jl:757; a
    // run of <= 2 FLUSH same-sign terms per lane keeps this far tighter).  Float64: plain double accumulators.
    constexpr bool PAIR = sizeof(R) == 4;
    constexpr int FLUSH = 128;
    cx<R> accp[PAIR ? E : 1];
    double acc[PAIR ? 1 : E];
    if constexpr (PAIR) {
#pragma unroll
        for (int e = 0; e < E; ++e) accp[e] = {(R)0, (R)0};
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.0;
    }
    double* part = static_cast<double*>(a.out) + (((int64_t)blockIdx.x * G + slot) * a.nch + ch) * N;
    const __amdgpu_buffer_rsrc_t prs = io::make_rsrc(part, (int64_t)N * 8);
    int since = 0;
    bool first = true;
    auto flush = [&, t]() {   // wave-uniform control flow; per-lane state is one laundered byte offset
        int off = t * 8;
        asm volatile("" : "+v"(off));
        if (first) {
#pragma unroll
            for (int e = 0; e < E; ++e) io::Ld<double>::store((double)accp[e].x + (double)accp[e].y, prs, off + T * e * 8);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double s = io::Ld<double>::load(prs, off + T * e * 8) + ((double)accp[e].x + (double)accp[e].y);
                io::Ld<double>::store(s, prs, off + T * e * 8);
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) accp[e] = {(R)0, (R)0};
        first = false;
        since = 0;
    };

    const R* sc = static_cast<const R*>(a.s) + ch * a.lds_;
    const int64_t nslots = (int64_t)gridDim.x * G;
    int64_t wbase = ((int64_t)blockIdx.x * G + slot) * a.run_len, wj = 0;
    auto unit_cur = [&](bool more) { return (more && wbase + wj < a.units_per_ch) ? wbase + wj : a.units_per_ch; };
    auto walk = [&]() {
        if (++wj == a.run_len) {
            wj = 0;
            wbase += nslots * a.run_len;
        }
    };
    const int64_t niter = a.niter;
    // half-frame h of unit u starts at sample u*N + h*(N/2), h = 0 (a lo), 1 (a hi = b lo), 2 (b hi)
    // (both lambdas take t by value: captured by reference it stays in memory until they are inlined, and the transform's address arithmetic is
    // selected and scheduled differently)
    auto load_half = [&, t](R (&dst)[H], int64_t u, int h, bool on) {
        const int64_t pos = u * N + (int64_t)h * (N / 2);
        const __amdgpu_buffer_rsrc_t r = io::make_rsrc(sc + pos, on ? std::min<int64_t>(N / 2, a.len - pos) * SZ : 0);
        io::load_window<R, H, T>(dst, r, 0, t);
    };
    R lo[H], ahi[H], bhi[H];
    int64_t u = unit_cur(niter > 0);
    const bool live = u < a.units_per_ch;
    load_half(lo, u, 0, live);
    load_half(ahi, u, 1, live);
    load_half(bhi, u, 2, live && (2 * u + 1) < a.K);
    for (int64_t it = 0; it < niter; ++it) {
        walk();
        const int64_t unext = unit_cur(it + 1 < niter);
        const bool haveB = (2 * u + 1) < a.K;   // u live implied (K >= 1) -- a dead unit has all-zero halves anyway
        cx<R> v[E];
        if (haveB) {
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (PAIR) {   // one packed multiply per bin: (lo, ahi) w_e and (ahi, bhi) w_{e+H}, the window half picked by op_sel
#pragma unroll
                for (int e = 0; e < H; ++e) {
                    const cx<R> wp = {w[e], w[e + H]};
                    v[e] = fft::pk_mul_blo(cx<R>{lo[e], ahi[e]}, wp);
                    v[e + H] = fft::pk_mul_bhi(cx<R>{ahi[e], bhi[e]}, wp);
                }
            } else
#endif
            {
#pragma unroll
                for (int e = 0; e < H; ++e) {
                    v[e] = {lo[e] * w[e], ahi[e] * w[e]};
                    v[e + H] = {ahi[e] * w[e + H], bhi[e] * w[e + H]};
                }
            }
        } else {  // odd frame count: the last unit has no second frame
#pragma unroll
            for (int e = 0; e < H; ++e) {
                v[e] = {lo[e] * w[e], (R)0};
                v[e + H] = {ahi[e] * w[e + H], (R)0};
            }
        }
        // next unit: reuse this unit's last half when it is the next frame's first half
        const bool nlive = unext < a.units_per_ch;
        if (unext == u + 1 && nlive) {
#pragma unroll
            for (int e = 0; e < H; ++e) lo[e] = bhi[e];
        } else {
            load_half(lo, unext, 0, nlive);
        }
        load_half(ahi, unext, 1, nlive);
        load_half(bhi, unext, 2, nlive && (2 * unext + 1) < a.K);
        u = unext;
        if (!MDSP_ABLATED(a, 2)) {
            fft::wg_fft<C, -1, TWMODE, PADSHIFT, NBUF, 0>(v, t, tw, twsrc, lds);
            if constexpr (C::P > 1 && NBUF > 1 && ((C::P - 1) % NBUF) != 0) fft::wg_sync<T>();  // NBUF == 1: wg_fft already ends every exchange with a barrier
        }
        if constexpr (PAIR) {
#pragma unroll
            for (int e = 0; e < E; ++e) accp[e] = fft::lanefma(v[e], v[e], accp[e]);
            if (++since == FLUSH) flush();
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += (double)(v[e].x * v[e].x + v[e].y * v[e].y);
        }
    }
    if constexpr (PAIR) {
        flush();
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) part[t + T * e] = acc[e];
    }
}

// ---- the same path, Float32, 16 elements per thread, with the instruction diet of round 3 ---------------------------------------------
// The round-2 loop issued ~420 VALU instructions per thread and unit for 335 of arithmetic.  What went:
//   * the samples of a unit live in PAIRS: Q[e] = (frame a, frame b)[t + T e] for the first half-frame, F[e] for the second -- exactly the
//     (re, im) operands of the packed first stage, so no v_mov builds them.  Frame b's first half IS frame a's second half: it is loaded a
//     second time (an L1/L2 hit, a VMEM slot instead of VALU work), predicated on the unit HAVING a frame b -- the odd last frame needs no
//     branch and no zeroing in the loop;
//   * the half-frame a unit hands to its successor (b's second half = the next a's first half) is not copied: the pair that holds it BECOMES
//     the successor's Q, and the successor packs z = b + i a instead of a + i b (|Z[k]|^2 + |Z[N-k]|^2 is symmetric in a <-> b, and k <-> N-k is
//     folded by the finalize kernel anyway), so the roles of the two pair arrays and of their halves alternate from unit to unit (loop unrolled x2);
//   * the window rides in the first butterfly stage (fft::bfly16_win: 8 packed operations less), and the butterflies' constant roots come
//     from SGPR pairs (fft_lds.h, MDSP_FFT_SGPR_CONST).
template <int N>
__global__ __launch_bounds__(N / 16, 2) void welch_half3_kernel(SpecArgs a) {
    using R = float;
    constexpr int E = 16, H = 8, PADSHIFT = 5;   // one LDS buffer, one element of padding per 32
    using C = fft::Cfg<N, E>;
    constexpr int T = C::T;
    static_assert(T % 64 == 0 && T >= 128, "one transform per workgroup");
    constexpr int NTWA = C::NTW > 0 ? C::NTW : 1;
    constexpr int REGION = fft::wg_lds_elems<C, PADSHIFT, 1>();
    __shared__ __attribute__((aligned(16))) cx<R> lds[REGION];
    const int t = threadIdx.x;
    const cx<R>* table = static_cast<const cx<R>*>(a.table);
    const int64_t ch = blockIdx.y;

    cx<R> tw[NTWA];
    fft::load_twiddles<C, R, 1, fft::TW_REG>(tw, t, table);
    cx<R> wp[H];   // {w[t + T e], w[t + T (e + 8)]}
    {
        double wd[E];
        load_window_regs<E, T>(wd, a.win, a.n, t);
#pragma unroll
        for (int e = 0; e < H; ++e) wp[e] = {(R)wd[e], (R)wd[e + H]};
    }
    constexpr int FLUSH = 128;
    cx<R> accp[E];
#pragma unroll
    for (int e = 0; e < E; ++e) accp[e] = {(R)0, (R)0};
    double* part = static_cast<double*>(a.out) + ((int64_t)blockIdx.x * a.nch + ch) * N;
    const __amdgpu_buffer_rsrc_t prs = io::make_rsrc(part, (int64_t)N * 8);
    int since = 0;
    bool first = true;
    auto flush = [&]() {
        int off = t * 8;
        asm volatile("" : "+v"(off));
        if (first) {
#pragma unroll
            for (int e = 0; e < E; ++e) io::Ld<double>::store((double)accp[e].x + (double)accp[e].y, prs, off + T * e * 8);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double s = io::Ld<double>::load(prs, off + T * e * 8) + ((double)accp[e].x + (double)accp[e].y);
                io::Ld<double>::store(s, prs, off + T * e * 8);
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) accp[e] = {(R)0, (R)0};
        first = false;
        since = 0;
    };

    const R* sc = static_cast<const R*>(a.s) + ch * a.lds_;
    const int64_t nslots = (int64_t)gridDim.x;
    int64_t wbase = (int64_t)blockIdx.x * a.run_len, wj = 0;
    auto unit_cur = [&](bool more) { return (more && wbase + wj < a.units_per_ch) ? wbase + wj : a.units_per_ch; };
    auto walk = [&]() {
        if (++wj == a.run_len) {
            wj = 0;
            wbase += nslots * a.run_len;
        }
    };
    // half-frame h of unit u starts at sample u N + h N/2: h = 0 (a lo), 1 (a hi = b lo), 2 (b hi); `on` false -> all zeros
    auto half_rsrc = [&](int64_t u, int h, bool on) {
        const int64_t pos = u * N + (int64_t)h * (N / 2);
        return io::make_rsrc(sc + pos, on ? std::min<int64_t>(N / 2, a.len - pos) * 4 : 0);
    };
    // component selectors: XA = true -> frame a rides in .x (z = a + i b), false -> in .y (z = b + i a)
    auto ld8 = [&](cx<R> (&dst)[H], bool to_x, const __amdgpu_buffer_rsrc_t r) {
        int off = t * 4;
        asm volatile("" : "+v"(off));
#pragma unroll
        for (int e = 0; e < H; ++e) {
            const R s = io::Ld<R>::load(r, off + T * e * 4);
            if (to_x) dst[e].x = s;
            else dst[e].y = s;
        }
    };
    // all four half-frame streams of unit u: Q = (a lo | b lo), F = (a hi | b hi); `carry`: a lo is already in Q (handed over by the predecessor)
    auto load_unit = [&](cx<R> (&Q)[H], cx<R> (&F)[H], bool xa, int64_t u, bool carry) {
        const bool live = u < a.units_per_ch, haveB = live && (2 * u + 1) < a.K;
        if (a.memprio) __builtin_amdgcn_s_setprio(3);
        if (!carry) ld8(Q, xa, half_rsrc(u, 0, live));
        ld8(Q, !xa, half_rsrc(u, 1, haveB));
        ld8(F, xa, half_rsrc(u, 1, live));
        ld8(F, !xa, half_rsrc(u, 2, haveB));
        if (a.memprio) __builtin_amdgcn_s_setprio(0);
    };
    cx<R> P1[H], P2[H];
    int64_t u = unit_cur(a.niter > 0);
    load_unit(P1, P2, true, u, false);
#ifdef MDSP_WELCH_PROF
    unsigned long long prof_sum[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prof_last = 0, prof_units = 0, prof_t0 = 0;
#define MDSP_STAMP(k)                                                                   \
    do {                                                                                \
        unsigned long long now_;                                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_) : : "memory"); \
        prof_sum[k] += now_ - prof_last;                                                \
        prof_last = now_;                                                               \
    } while (0)
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_last) : : "memory");
    prof_t0 = prof_last;
#endif
    // everything of a unit after its first pass (whose results are on their way to LDS) and after the prefetch has been issued
    auto tail = [&]() {
        cx<R> v[E];
#ifdef MDSP_WELCH_PROF
        // phase timeline of one unit (debug builds: build.py --tag prof --cflags -DMDSP_WELCH_PROF): shader-clock stamps at the phase boundaries,
        // summed per wave; s_memtime needs lgkmcnt(0), which every boundary here waits for anyway (barriers, first use of the reloaded operands)
        static_assert(C::P == 3, "the phase profile is wired for three passes");
        MDSP_STAMP(1);   // pass 0: butterflies + LDS writes done, next unit's loads issued
        fft::wg_sync<T>();
        MDSP_STAMP(2);   // barrier 1
        fft::pass_reload<C, PADSHIFT>(v, t, lds);
        MDSP_STAMP(3);   // operands of pass 1 back from LDS
        fft::wg_sync<T>();
        MDSP_STAMP(4);   // barrier 2
        fft::pass_compute<C, -1, 1, fft::TW_REG, PADSHIFT>(v, t, tw, table, lds);
        MDSP_STAMP(5);   // pass 1 + LDS writes
        fft::wg_sync<T>();
        MDSP_STAMP(6);   // barrier 3
        fft::pass_reload<C, PADSHIFT>(v, t, lds);
        MDSP_STAMP(7);   // operands of pass 2
        fft::wg_sync<T>();
        MDSP_STAMP(8);   // barrier 4
        fft::pass_compute<C, -1, 2, fft::TW_REG, PADSHIFT>(v, t, tw, table, lds);
#pragma unroll
        for (int e = 0; e < E; ++e) accp[e] = fft::lanefma(v[e], v[e], accp[e]);
        asm volatile("" :: "v"(accp[0].x), "v"(accp[E - 1].y));
        MDSP_STAMP(9);   // pass 2 + |Z|^2
        if (++since == FLUSH) flush();
        MDSP_STAMP(0);   // (flush); also the start of the next unit
        ++prof_units;
#else
        fft::wg_sync<T>();
        fft::pass_reload<C, PADSHIFT>(v, t, lds);
        fft::wg_sync<T>();
        fft::wg_fft<C, -1, fft::TW_REG, PADSHIFT, 1, 0, 1>(v, t, tw, table, lds);
#pragma unroll
        for (int e = 0; e < E; ++e) accp[e] = fft::lanefma(v[e], v[e], accp[e]);
        if (++since == FLUSH) flush();
#endif
    };
    auto unit = [&](cx<R> (&Q)[H], cx<R> (&F)[H], bool xa, bool more) {
        walk();
        const int64_t unext = unit_cur(more);
#ifdef MDSP_WELCH_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        MDSP_STAMP(10);   // this unit's samples have arrived
        {
            cx<R> v0[16];
            fft::bfly16_win<-1>(Q, F, wp, v0);
            asm volatile("" :: "v"(v0[0].x), "v"(v0[15].y));
            MDSP_STAMP(11);   // first pass: arithmetic
            fft::pass0_scatter<C, PADSHIFT>(v0, t, lds);
            MDSP_STAMP(12);   // first pass: LDS writes retired
        }
#else
        fft::pass0_windowed<C, PADSHIFT>(Q, F, wp, t, lds);   // consumes Q and F
#endif
        // the successor: F's frame-b-second-half component is its frame a's first half when it follows directly (roles and halves swap)
        const bool carry = unext == u + 1 && unext < a.units_per_ch;   // wave-uniform
        load_unit(F, Q, !xa, unext, carry);
        u = unext;
        tail();
    };
    for (int64_t it = 0; it < a.niter; it += 2) {   // same trip count for every slot (barriers inside)
        unit(P1, P2, true, it + 1 < a.niter);
        if (it + 1 < a.niter) unit(P2, P1, false, it + 2 < a.niter);
    }
    flush();
#ifdef MDSP_WELCH_PROF
    if (a.rinv && (threadIdx.x & 63) == 0) {   // one record per wave: 10 phase sums, units, total clocks  (a.rinv: the profile buffer in these builds)
        unsigned long long* rec = (unsigned long long*)a.rinv + ((size_t)blockIdx.x * (T / 64) + threadIdx.x / 64) * 16;
        for (int k = 0; k < 13; ++k) rec[k] = prof_sum[k];
        rec[13] = prof_units;
        rec[14] = prof_last - prof_t0;
    }
#undef MDSP_STAMP
#endif
}

// One persistent launch of a power-of-two Welch kernel with G transform slots per workgroup of `threads`: the grid the device holds, one Float64 partial
// row of nfft bins per slot and channel in pl->partial, the unit schedule.  *nslices = rows written.
template <typename K> int welch_run(K kern, int threads, int G, mdsp_welch_plan_s* pl, SpecArgs& a, hipStream_t st, int* nslices) {
    int grid = 1;
    MDSP_TRY(grid_for(kern, threads, cdiv(a.units_per_ch, G), a.nch, &grid));
    MDSP_TRY(pl->partial.reserve(sizeof(double) * (size_t)grid * G * (size_t)a.nch * (size_t)pl->nfft));
    a.out = pl->partial.p;
    set_schedule(a, a.units_per_ch, (int64_t)grid * G);
    hipLaunchKernelGGL(kern, dim3(grid, (unsigned)a.nch), dim3(threads), 0, st, a);
    MDSP_LAUNCH_CHECK();
    *nslices = grid * G;
    return MDSP_OK;
}

template <int N> int welch_run_half3(mdsp_welch_plan_s* pl, SpecArgs& a, hipStream_t st, int* nslices) {
    auto kern = welch_half3_kernel<N>;
    constexpr int threads = N / 16;
#ifdef MDSP_WELCH_PROF
    int grid = 1;   // (the grid welch_run is about to choose: the profile buffer has a record per wave)
    MDSP_TRY(grid_for(kern, threads, a.units_per_ch, a.nch, &grid));
    static DevBuf profbuf;
    const size_t nrec = (size_t)grid * (threads / 64);
    MDSP_TRY(profbuf.reserve(nrec * 16 * 8));
    a.rinv = a.nch == 1 ? static_cast<const double*>(profbuf.p) : nullptr;
    hipEvent_t e0, e1;
    MDSP_HIP(hipEventCreate(&e0)); MDSP_HIP(hipEventCreate(&e1));
    MDSP_HIP(hipEventRecord(e0, st));
#endif
    MDSP_TRY(welch_run(kern, threads, 1, pl, a, st, nslices));
#ifdef MDSP_WELCH_PROF
    MDSP_HIP(hipEventRecord(e1, st));
    MDSP_HIP(hipStreamSynchronize(st));
    float ms = 0;
    MDSP_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (a.rinv) {   // debug build only: one line per launch
        std::vector<unsigned long long> h(nrec * 16);
        MDSP_HIP(hipMemcpy(h.data(), profbuf.p, nrec * 16 * 8, hipMemcpyDeviceToHost));
        double sum[13] = {0}, units = 0, tot = 0, totmax = 0;
        for (size_t r = 0; r < nrec; ++r) {
            for (int k = 0; k < 13; ++k) sum[k] += (double)h[r * 16 + k];
            units += (double)h[r * 16 + 13];
            tot += (double)h[r * 16 + 14];
            totmax = std::max(totmax, (double)h[r * 16 + 14]);
        }
        static const char* nm[13] = {"flush+loop", "load-issue", "barrier1", "reload1", "barrier2", "pass1+ldsW", "barrier3", "reload2", "barrier4", "pass2+acc",
                                     "memwait", "pass0-valu", "pass0-ldsW"};
        fprintf(stderr, "WELCHPROF grid %d x %d waves, %.4f ms, %.0f units/wave, clocks/unit %.0f (max-wave total %.0f clocks -> %.3f GHz):", grid, threads / 64, ms,
                units / nrec, tot / units, totmax, totmax / (ms * 1e6));
        for (int k : {10, 11, 12, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0}) fprintf(stderr, " %s %.0f", nm[k], sum[k] / units);
        fprintf(stderr, "\n");
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
#endif
    return MDSP_OK;
}

#include "welch_w64.h"   // one wavefront per transform: the hand-allocated kernels and welch_run_w64asm

// the accumulator now holds the fused engine's sums: Float64, nfft bins per channel (pair-packed full spectrum for real signals)
void set_fused_sums(mdsp_welch_plan_s* pl) {
    pl->acc_fresh = false;
    pl->acc_nslices = 1;
    pl->acc_nacc = (int)pl->nfft;
    pl->acc_mode = dtype_is_complex(pl->dtype) ? 1 : (pl->onesided ? 3 : 4);
}

template <typename R, int N, bool CPLX>
int welch_launch_n(mdsp_welch_plan_s* pl, SpecArgs& a, hipStream_t st) {
    using Gm = Geo<R, N>;
    int nslices = 0, rc = MDSP_OK;
    const bool half_ok = !CPLX && a.n == N && 2 * a.hop == N && !MDSP_DBG(welch_nohalf);
    if constexpr (!CPLX && N >= 256) {
        if (half_ok) {
            if constexpr (N == 4096 && sizeof(R) == 4) {
                // The headline shape has five kernels, selectable with MDSP_WELCH_VARIANT when the plan is made:
                //   45 csrc/welch_w64e_asm.s: variant 44 with counted load waits (no full wait at the top of a unit).  The same arithmetic and the
                //      same bits as 44; 1.21 against 1.28 ms (profiles/welch_w64e_ab.json).  The default where 44 was.
                //   44 csrc/welch_w64d_asm.s: hand-allocated, one wavefront per transform, the half-frame two units share carried in registers, folded
                //      twiddles.  It reduces into pl->reduced itself.  These kernels are the default where the stream is long enough to give every wave
                //      of the chip a unit and the schedule is one run per slot (MDSP_RUNS_PER_SLOT); 30 is the default otherwise.
                //   43 csrc/welch_w64c_asm.s: the same kernel before the twiddles were folded (13 % more vector instructions; 1.356 against 1.275 ms,
                //      profiles/r07_welch_w64d_ab.json).  The tests compare 44 against it.
                //   30 welch_half3_kernel: the HIP kernel for every other stream length and schedule (1.17 against 1.00 ms for 43 on an all-zero
                //      stream, profiles/r04_welch_carry_power.json).
                //   18 welch_half_kernel with pad shift 5: the generic half-frame kernel, the reference the tests hold 30 and 43 against.
                // Any other number selects the default rule.
                if (pl->variant == 18) rc = welch_run(welch_half_kernel<R, N, 16, 1, 1, 5, 1>, N / 16, 1, pl, a, st, &nslices);
                else {
                    const bool long_enough = a.K / 2 >= (int64_t)device_cu_count() * 8 && tunables().runs_per_slot == 1;
                    const bool forced = pl->variant == 43 || pl->variant == 44 || pl->variant == 45;
                    if (forced || (pl->variant != 30 && long_enough)) {
                        bool handled = false;
                        rc = w64::welch_run_w64asm(pl, a, st, &handled, forced ? pl->variant : 45);
                        if (rc == MDSP_OK && handled) goto reduced_done;
                        if (rc != MDSP_OK) return rc;
                    }
                    rc = welch_run_half3<N>(pl, a, st, &nslices);
                }
            } else {
                constexpr int EH = (N >= 2048 && sizeof(R) == 4) ? 16 : Gm::E;   // Float32, nfft >= 1024: 16 elements per thread (Geo does 1024)
                constexpr int GH = slots_per_workgroup(N / EH);
                constexpr int NBH = (EH == 16 || N / EH <= 64) ? 1 : 2;
                rc = welch_run(welch_half_kernel<R, N, EH, GH, Gm::TWREG, pad_default<R>(), NBH>, (N / EH) * GH, GH, pl, a, st, &nslices);
            }
            goto finalize;
        }
    }
    if constexpr (N == 4096 && !CPLX && sizeof(R) == 4) {   // the headline shape off the half-frame path: 16 elements per thread, one LDS buffer
        rc = welch_run(welch_fused_kernel<R, N, 16, 1, 1, 4, CPLX, 1, false>, N / 16, 1, pl, a, st, &nslices);
    } else {
        bool done = false;
        if constexpr (CPLX && sizeof(R) == 4 && Gm::E > 4) {   // complex Float32 frames advancing by whole elements: overlap stays in registers
            constexpr int T = N / Gm::E;
            const int shift = (!MDSP_DBG(stft_noshift) && a.n == N && a.hop % T == 0 && a.hop / T < Gm::E) ? (int)(a.hop / T) : 0;
            done = shift == 1 || shift == 2 || shift == 4;
            if (shift == 1) rc = welch_run(welch_fused_kernel<R, N, Gm::E, Gm::G, Gm::TWREG, pad_default<R>(), CPLX, Gm::NBUF, false, 1>, (N / Gm::E) * Gm::G, Gm::G, pl, a, st, &nslices);
            else if (shift == 2) rc = welch_run(welch_fused_kernel<R, N, Gm::E, Gm::G, Gm::TWREG, pad_default<R>(), CPLX, Gm::NBUF, false, 2>, (N / Gm::E) * Gm::G, Gm::G, pl, a, st, &nslices);
            else if (shift == 4) rc = welch_run(welch_fused_kernel<R, N, Gm::E, Gm::G, Gm::TWREG, pad_default<R>(), CPLX, Gm::NBUF, false, 4>, (N / Gm::E) * Gm::G, Gm::G, pl, a, st, &nslices);
        }
        if (!done) rc = welch_run(welch_fused_kernel<R, N, Gm::E, Gm::G, Gm::TWREG, pad_default<R>(), CPLX, Gm::NBUF, sizeof(R) == 8>, (N / Gm::E) * Gm::G, Gm::G, pl, a, st, &nslices);
    }
finalize:
    if (rc != MDSP_OK) return rc;
    // fold the slots' partial rows into the plan's Float64 accumulator (added to what earlier slices of the stream left there)
    MDSP_TRY(pl->reduced.reserve(sizeof(double) * (size_t)a.nch * N));
    MDSP_TRY(reduce_partials(pl, pl->partial.as<double>(), pl->reduced.as<double>(), nslices, a.nch, N, pl->acc_fresh ? 0 : 1, st));
reduced_done:
    if (rc != MDSP_OK) return rc;
    set_fused_sums(pl);
    return MDSP_OK;
}

template <typename R, bool CPLX>
int welch_accumulate_fused(mdsp_welch_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, hipStream_t st) {
    const int64_t K = mdsp_frame_count(len, pl->n, pl->noverlap), hop = pl->n - pl->noverlap, N = pl->nfft;
    const double* win = pl->have_win ? pl->win.as<double>() : nullptr;
    if (pl->route != MDSP_ROUTE_POW2 || K == 0) MDSP_TRY(pl->reduced.reserve(sizeof(double) * (size_t)nch * (size_t)N));
    if (K == 0) {
        if (pl->acc_fresh) {   // nothing to add; make the accumulator exist (zeros) so that a later finalize / all-reduce is defined
            MDSP_HIP(hipMemsetAsync(pl->reduced.p, 0, sizeof(double) * (size_t)nch * (size_t)N, st));
            set_fused_sums(pl);
        }
        return MDSP_OK;
    }
    // the single-workgroup kernels leave partial rows per group of workgroups in pl->partial (same Float64 accumulator protocol), reduced below
    int64_t ngroups = 0;
    switch (pl->route) {
        case MDSP_ROUTE_POW2: {
            SpecArgs a{};
            a.s = s; a.table = pl->table.p; a.win = win; a.len = len; a.lds_ = lds_; a.K = K; a.hop = hop; a.units_per_ch = CPLX ? K : cdiv(K, 2); a.nch = nch;
            a.n = (int)pl->n; a.nout = (int)pl->nout; a.onesided = pl->onesided; a.r = pl->r;
            switch (N) {
                case 256: return welch_launch_n<R, 256, CPLX>(pl, a, st);
                case 512: return welch_launch_n<R, 512, CPLX>(pl, a, st);
                case 1024: return welch_launch_n<R, 1024, CPLX>(pl, a, st);
                case 2048: return welch_launch_n<R, 2048, CPLX>(pl, a, st);
                case 4096: return welch_launch_n<R, 4096, CPLX>(pl, a, st);
                case 8192:
                    if constexpr (sizeof(R) == 4) return welch_launch_n<R, 8192, CPLX>(pl, a, st);
                default: break;
            }
            MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "fused Welch does not support nfft=%lld", (long long)N);
        }
        case MDSP_ROUTE_GEN:   // mixed-radix sizes: everything through LDS (spectral_gen.hip)
            MDSP_TRY(gen_welch(pl, s, len, nch, lds_, K, hop, win, st, &ngroups));
            break;
        case MDSP_ROUTE_GX: {   // run-time-schedule kernel (spectral_gx.h)
            GxArgs g{};
            g.s = s; g.lds_ = lds_; g.K = K; g.hop = hop; g.nch = nch;
            g.n = (int)pl->n; g.nfft = (int)N; g.nout = (int)pl->nout; g.onesided = pl->onesided; g.r = pl->r;
            MDSP_TRY((gx_launch<R, CPLX, 0>(pl->gx, g, win, pl->dtype, st, &ngroups, &pl->partial)));
            break;
        }
        case MDSP_ROUTE_CTBIG:   // one workgroup, compile-time schedule (spectral_ctbig.hip): 8400 .. 12500 points
            MDSP_TRY(ctbig_welch(pl->ctcols, pl->dtype, s, lds_, K, hop, nch, (int)pl->n, N, win, st, &ngroups, &pl->partial));
            break;
        case MDSP_ROUTE_CTCOLS_BIG:   // R0 x a row size with a compile-time schedule (spectral_ctcols*.hip)
            MDSP_TRY(ctcols_big_welch(pl->ctcols, pl->dtype, s, lds_, K, hop, nch, (int)pl->n, N, pl->r0, st, &ngroups, &pl->partial));
            break;
        case MDSP_ROUTE_CTCOLS_F64:
            MDSP_TRY(ctcols64_welch(pl->ctcols, CPLX, s, lds_, K, hop, nch, (int)pl->n, N, pl->r0, st, &ngroups, &pl->partial));
            break;
        case MDSP_ROUTE_CTCOLS:
            MDSP_TRY(ctcols_welch(pl->ctcols, pl->dtype, s, lds_, K, hop, nch, (int)pl->n, N, pl->r0, st, &ngroups, &pl->partial));
            break;
        case MDSP_ROUTE_CTROWS:   // nfft = R0 x S in two kernels (spectral_ctrows.hip): straight into the accumulator
            MDSP_TRY(ctrows_welch(pl->ctrows, pl->dtype, pl->r0, s, lds_, K, hop, nch, (int)pl->n, N, pl->reduced.as<double>(), pl->acc_fresh, st));
            set_fused_sums(pl);
            return MDSP_OK;
        case MDSP_ROUTE_BIG: {   // nfft above the one-workgroup sizes: channel by channel through the multi-pass engine, straight into the accumulator
            using TT = std::conditional_t<CPLX, cx<R>, R>;
            for (int64_t c = 0; c < nch; ++c)
                MDSP_TRY(big::welch(pl->big, pl->dtype, pl->n, N, static_cast<const TT*>(s) + c * lds_, K, hop, win, pl->reduced.as<double>() + c * N, pl->acc_fresh, st));
            set_fused_sums(pl);
            return MDSP_OK;
        }
        default: MDSP_FAIL(MDSP_ERR_ASSERTION, "Welch plan with route %d on the fused engine", pl->route);
    }
    MDSP_TRY(reduce_partials(pl, pl->partial.as<double>(), pl->reduced.as<double>(), (int)ngroups, nch, (int)N, pl->acc_fresh ? 0 : 1, st));
    set_fused_sums(pl);
    return MDSP_OK;
}

// Every table the plan's route reads, built once at plan creation from host data (synchronous copies: complete before the plan exists, whatever stream the
// first exec runs on).  The exec functions above upload nothing; one that finds a table missing fails.
int prepare_welch_tables(mdsp_welch_plan_s* pl, const double* window_host) {
    const bool dbl = dtype_is_double(pl->dtype);
    const int n = (int)pl->n;
    const int64_t N = pl->nfft, S = pl->r0 > 0 ? N / pl->r0 : N;
    switch (pl->route) {
        case MDSP_ROUTE_POW2:
            MDSP_TRY(upload_roots(pl->table, dbl, N));
            if (N == w64::N && pl->dtype == MDSP_F32) MDSP_TRY(w64::w64asm_prepare(pl->w64prep, window_host, n));
            return MDSP_OK;
        case MDSP_ROUTE_GEN:
            MDSP_TRY(upload_roots(pl->table, dbl, N));
            if (lean_window_needed(N, dbl)) MDSP_TRY(upload_window(pl->winr, dbl, window_host, n, N));
            return MDSP_OK;
        case MDSP_ROUTE_GX:
            MDSP_TRY(dbl ? gx_prepare<double>(pl->gx, pl->dtype, N, true) : gx_prepare<float>(pl->gx, pl->dtype, N, true));
            return upload_window(pl->gx.win, dbl, window_host, n, N);
        case MDSP_ROUTE_CTBIG:
            MDSP_TRY(upload_roots(pl->ctcols.roots, dbl, N));
            return upload_window(pl->ctcols.win, dbl, window_host, n, N);
        case MDSP_ROUTE_CTCOLS:
        case MDSP_ROUTE_CTCOLS_BIG:
        case MDSP_ROUTE_CTCOLS_F64:
            MDSP_TRY(upload_roots(pl->ctcols.roots, dbl, S));
            MDSP_TRY(upload_roots(pl->ctcols.rootsN, dbl, N));
            return upload_window(pl->ctcols.win, dbl, window_host, n, N);
        case MDSP_ROUTE_CTROWS:   // the column kernel's tables, and the row kernel's: S-point transforms of whole rows, no window
            MDSP_TRY(upload_roots(pl->ctrows.rootsN, dbl, N));
            MDSP_TRY(upload_window(pl->ctrows.win, dbl, window_host, n, N));
            MDSP_TRY(upload_roots(pl->ctrows.rows.roots, dbl, S));
            return upload_window(pl->ctrows.rows.win, dbl, nullptr, (int)S, S);
        default: return MDSP_OK;   // the multi-pass engine builds its own at first use (bigfft.hip); rocFFT has none
    }
}

}  // namespace

namespace mdsp {
// Welch in the rows form of the multi-pass engine (bigfft.hip run_welch_rows): `nch` rows of S = pl->nfft complex points, K frames `hop` elements apart
// (the rows of K transforms of nch x S points, column pass done) -> pl->reduced[row][bin] (+)= |FFT_S(frame)|^2 on the single-workgroup kernels.
// pl: a complex, two-sided, window-free FUSED plan of S points (n = nfft = S).
int welch_rows_accumulate(mdsp_welch_plan_s* pl, const void* work, int64_t K, int64_t hop, int64_t nch, hipStream_t st) {
    if (pl->route != MDSP_ROUTE_POW2) MDSP_FAIL(MDSP_ERR_ASSERTION, "rows of %lld points on route %d, not the power-of-two kernel", (long long)pl->nfft, pl->route);
    if (K <= 0 || nch <= 0) return MDSP_OK;
    SpecArgs a{};
    a.s = work;
    a.table = pl->table.p;
    a.win = nullptr;
    a.len = (K - 1) * hop + pl->n;
    a.lds_ = pl->n;
    a.K = K;
    a.hop = hop;
    a.units_per_ch = K;
    a.nch = nch;
    a.n = (int)pl->n;
    a.nout = (int)pl->nout;
    a.onesided = 0;
    a.r = 1.0;
    if (pl->dtype == MDSP_C32 && pl->nfft == 8192) return welch_launch_n<float, 8192, true>(pl, a, st);
    if (pl->dtype == MDSP_C64 && pl->nfft == 4096) return welch_launch_n<double, 4096, true>(pl, a, st);
    MDSP_FAIL(MDSP_ERR_ASSERTION, "rows of %lld points of dtype %d", (long long)pl->nfft, pl->dtype);
}
}  // namespace mdsp

extern "C" {

int mdsp_welch_plan_create(mdsp_welch_plan* plan, int64_t n, int64_t noverlap, int64_t nfft, const double* window_host, double r, int onesided,
                           int dtype, int engine) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype %d", dtype);
    if (onesided && dtype_is_complex(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "cannot compute one-sided FFT of a complex signal");
    if (!(nfft >= n)) MDSP_FAIL(MDSP_ERR_DOMAIN, "nfft must be >= n (nfft=%lld, n=%lld)", (long long)nfft, (long long)n);
    MDSP_TRY(check_split(n, noverlap, nfft));
    if (!(r > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "normalisation r must be positive");
    SpecRoute rt;
    MDSP_TRY(choose_spectral_route(engine, dtype, nfft, 0, &rt));
    auto pl = new mdsp_welch_plan_s();
    pl->dtype = dtype;
    pl->engine = rt.engine;
    pl->route = rt.route;
    pl->r0 = rt.r0;
    pl->onesided = onesided ? 1 : 0;
    pl->n = n;
    pl->noverlap = noverlap;
    pl->nfft = nfft;
    pl->nout = onesided ? nfft / 2 + 1 : nfft;
    pl->r = r;
    pl->variant = tunables().welch_variant;
    int st = MDSP_OK;
    if (window_host) {
        pl->have_win = true;
        st = pl->win.reserve(sizeof(double) * (size_t)n);
        if (st == MDSP_OK && hipMemcpy(pl->win.p, window_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
            st = set_error(MDSP_ERR_DEVICE, "window upload failed");
    }
    if (st == MDSP_OK) st = prepare_welch_tables(pl, window_host);
    if (st != MDSP_OK) {
        delete pl;
        return st;
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_welch_plan_destroy(mdsp_welch_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_welch_plan_info(mdsp_welch_plan plan, int64_t* nout, int* engine_used) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nout) *nout = plan->nout;
    if (engine_used) *engine_used = plan->engine;
    return MDSP_OK;
}

static int welch_check_args(mdsp_welch_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (len < 0 || nch < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (!s_dev && len > 0 && nch > 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "s is NULL");
    if (nch > 1 && lds_ < len) MDSP_FAIL(MDSP_ERR_DIMENSION, "leading dimension smaller than the column length");
    if (nch > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 channels per call");
    return MDSP_OK;
}

int mdsp_welch_reset(mdsp_welch_plan plan) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    plan->acc_fresh = true;
    plan->acc_frames = 0;
    plan->acc_nch = 0;
    plan->frames_on_device = false;
    plan->sums_global = false;
    return MDSP_OK;
}

int mdsp_welch_accumulate(mdsp_welch_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_, void* stream) {
    MDSP_TRY(welch_check_args(plan, s_dev, len, nch, lds_));
    if (nch == 0) return MDSP_OK;
    if (!plan->acc_fresh && plan->acc_nch != nch)
        MDSP_FAIL(MDSP_ERR_DIMENSION, "accumulating %lld channels into sums of %lld channels (mdsp_welch_reset first)", (long long)nch, (long long)plan->acc_nch);
    if (plan->sums_global)   // a later all-reduce would add the earlier global totals once per rank
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "these sums are totals over ranks (mdsp_welch_allreduce ran): mdsp_welch_reset before accumulating again");
    hipStream_t st = as_stream(stream);
    const bool cplx = dtype_is_complex(plan->dtype), dbl = dtype_is_double(plan->dtype);
    int rc;
    if (plan->engine == MDSP_ENGINE_ROCFFT) {
        if (cplx) rc = dbl ? welch_accumulate_rocfft<double, true>(plan, s_dev, len, nch, lds_, st) : welch_accumulate_rocfft<float, true>(plan, s_dev, len, nch, lds_, st);
        else rc = dbl ? welch_accumulate_rocfft<double, false>(plan, s_dev, len, nch, lds_, st) : welch_accumulate_rocfft<float, false>(plan, s_dev, len, nch, lds_, st);
    } else {
        if (cplx) rc = dbl ? welch_accumulate_fused<double, true>(plan, s_dev, len, nch, lds_, st) : welch_accumulate_fused<float, true>(plan, s_dev, len, nch, lds_, st);
        else rc = dbl ? welch_accumulate_fused<double, false>(plan, s_dev, len, nch, lds_, st) : welch_accumulate_fused<float, false>(plan, s_dev, len, nch, lds_, st);
    }
    if (rc != MDSP_OK) return rc;
    plan->acc_nch = nch;
    plan->acc_frames += mdsp_frame_count(len, plan->n, plan->noverlap);
    plan->frames_on_device = false;   // an all-reduced count (mdsp_welch_allreduce) does not know about these frames: finalize takes frames_total from its caller then
    return MDSP_OK;
}

int mdsp_welch_frames_accumulated(mdsp_welch_plan plan, int64_t* frames_per_channel) {
    if (!plan || !frames_per_channel) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    *frames_per_channel = plan->acc_frames;
    if (plan->frames_on_device) {   // after mdsp_welch_allreduce: the total over ranks, read back (this query, unlike the collective, synchronises)
        double k = 0;
        MDSP_HIP(hipStreamSynchronize(plan->count_stream));   // the set / all-reduce of the count were queued there (possibly a non-blocking stream)
        MDSP_HIP(hipMemcpy(&k, plan->kdev.p, sizeof(double), hipMemcpyDeviceToHost));
        *frames_per_channel = (int64_t)k;
    }
    return MDSP_OK;
}

int mdsp_welch_accumulator(mdsp_welch_plan plan, void** acc_dev, int64_t* count) {
    if (!plan || !acc_dev || !count) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    if (plan->acc_fresh) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nothing accumulated since the last mdsp_welch_reset");
    *acc_dev = plan->acc_ptr();
    *count = (int64_t)plan->acc_nslices * plan->acc_nch * plan->acc_nacc;
    return MDSP_OK;
}

int mdsp_welch_finalize(mdsp_welch_plan plan, int64_t frames_total, void* psd_dev, int64_t ldp, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (!psd_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "out is NULL");
    if (plan->acc_fresh) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nothing accumulated since the last mdsp_welch_reset");
    if (plan->acc_nch > 1 && ldp < plan->nout) MDSP_FAIL(MDSP_ERR_DIMENSION, "leading dimension smaller than the column length");
    const int64_t K = frames_total > 0 ? frames_total : (plan->frames_on_device ? 0 : plan->acc_frames);   // 0 with frames_on_device: the kernel reads the all-reduced count
    return dtype_is_double(plan->dtype) ? welch_finalize<double>(plan, K, plan->acc_nch, psd_dev, ldp, as_stream(stream))
                                        : welch_finalize<float>(plan, K, plan->acc_nch, psd_dev, ldp, as_stream(stream));
}

int mdsp_welch_exec(mdsp_welch_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_, void* psd_dev, int64_t ldp, void* stream) {
    MDSP_TRY(welch_check_args(plan, s_dev, len, nch, lds_));
    if (nch == 0) return MDSP_OK;
    if (!psd_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "out is NULL");
    if (nch > 1 && ldp < plan->nout) MDSP_FAIL(MDSP_ERR_DIMENSION, "leading dimension smaller than the column length");
    MDSP_TRY(mdsp_welch_reset(plan));
    MDSP_TRY(mdsp_welch_accumulate(plan, s_dev, len, nch, lds_, stream));
    return mdsp_welch_finalize(plan, 0, psd_dev, ldp, stream);
}

}  // extern "C"

// channel sum (local part of the cross-channel Welch mean); `scale` != 1: the mean in the same launch, rounded exactly as sum-then-scale would be
template <typename R>
__global__ __launch_bounds__(256) void channel_sum_kernel(const R* __restrict__ psd, R* __restrict__ out, int64_t nout, int64_t nch, int64_t ldp, double scale) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nout) return;
    double a = 0;
    for (int64_t c = 0; c < nch; ++c) a += (double)psd[c * ldp + j];
    const R sum = (R)a;
    out[j] = scale == 1.0 ? sum : (R)((double)sum * scale);
}

namespace mdsp {
int channel_sum_scaled(const void* psd_dev, int64_t nout, int64_t nch, int64_t ldp, int real_dtype, void* sum_dev, double scale, void* stream) {
    if (real_dtype != MDSP_F32 && real_dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_ARGUMENT, "real dtype expected");
    if (nout <= 0) return MDSP_OK;
    const dim3 g((unsigned)cdiv(nout, 256));
    if (real_dtype == MDSP_F32)
        hipLaunchKernelGGL(channel_sum_kernel<float>, g, dim3(256), 0, as_stream(stream), (const float*)psd_dev, (float*)sum_dev, nout, nch, ldp, scale);
    else
        hipLaunchKernelGGL(channel_sum_kernel<double>, g, dim3(256), 0, as_stream(stream), (const double*)psd_dev, (double*)sum_dev, nout, nch, ldp, scale);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}
}  // namespace mdsp

extern "C" int mdsp_channel_sum(const void* psd_dev, int64_t nout, int64_t nch, int64_t ldp, int real_dtype, void* sum_dev, void* stream) {
    return mdsp::channel_sum_scaled(psd_dev, nout, nch, ldp, real_dtype, sum_dev, 1.0, stream);
}
