// STFT / spectrogram / periodogram columns (mdsp_stft_*); multitaper.hip runs its tapers through the same plans (stft_dispatch).
//
// Reference loops being replaced (src/periodograms.jl; framing and K4: spectral.hip):
//   F3  mul!(outbuf, plan, sig) :754, :888        rfft (real) / fft (complex), out of place
//   K5  fft2pow! :142-172              out[i] = muladd(abs2(X[i]), m, out[i]),  m = 1/r or 2/r
//   K6  fft2oneortwosided! :234-244    raw STFT column, conjugate mirror for real -> two-sided
//
// Engines:
//   FUSED  (power-of-two nfft in [256, 8192]): window -> FFT -> (|X|^2 * m | X) -> coalesced column store, one kernel.
//          Other sizes: the columns (MODE 1) of spectral_gen.hip, spectral_gx.h, spectral_ctbig_cols.hip and bigfft.hip.
//   ROCFFT : K4 kernel -> batched rocFFT -> K5/K6 kernel over cache-sized chunks; any nfft.
#include <algorithm>
#include <vector>

#include "common.h"
#include "devio.h"
#include "fft_lds.h"
#include "fft_wg.h"
#include "rocfft_wrap.h"
#include "spectral_tables.h"
#include "spectral_op.h"
#include "spectral_plan.h"
#include "hostpipe.h"
#include "gx_kernels.h"   // (namespace mdsp::gx and the kernel template: ahead of the anonymous namespace that includes spectral_gx.h)

using namespace mdsp;
using mdsp::fft::cx;

namespace {

// ======================================================================================================
// rocFFT-engine kernel
// ======================================================================================================
// K5/K6 (STFT): column store from a batched spectrum.  PSD: out real; else complex.
//   HALF: spectrum has nfft/2+1 bins (real input); two-sided output mirrors (conjugate for raw STFT).
template <typename R, bool PSD, bool HALF>
__global__ __launch_bounds__(256) void stft_store_kernel(const cx<R>* __restrict__ spec, void* __restrict__ out, int nspec, int nfft, int nout,
                                                         int64_t K, int64_t ldo, int64_t chs, int64_t u0, int64_t nunits, double r, int onesided,
                                                         int accumulate) {
    const int64_t u = u0 + blockIdx.x;
    if (u >= nunits) return;
    const int64_t ch = u / K, f = u - ch * K;
    const cx<R>* z = spec + (int64_t)blockIdx.x * nspec;
    const R m1 = (R)(1.0 / r), m2 = (R)(2.0 / r);
    for (int j = blockIdx.y * blockDim.x + threadIdx.x; j < nout; j += gridDim.y * blockDim.x) {
        int k = j;
        bool conj = false;
        if (HALF && j > nfft / 2) {
            k = nfft - j;
            conj = true;
        }
        const cx<R> v = z[k];
        if (PSD) {
            const R p = v.x * v.x + v.y * v.y;
            R m = m1;
            if (onesided && !(j == 0 || (j == nout - 1 && nfft % 2 == 0))) m = m2;
            R* o = static_cast<R*>(out) + ch * chs + f * ldo + j;
            *o = accumulate ? fma(p, m, *o) : p * m;                 // fft2pow!: out = muladd(abs2, m, out)
        } else {
            static_cast<cx<R>*>(out)[ch * chs + f * ldo + j] = conj ? cx<R>{v.x, -v.y} : v;
        }
    }
}

// ======================================================================================================
// Fused kernels
// ======================================================================================================
// One frame per transform slot (real frames ride with a zero imaginary part).
// SHIFT > 0 (host guarantees n == N and hop == SHIFT * T): consecutive frames of a slot's run overlap by N - hop samples, and a
// thread's element e of frame f+1 is its element e + SHIFT of frame f -- the raw samples stay in registers, shift by SHIFT
// elements per frame, and only the SHIFT new ones are loaded: every sample is read from memory once per run instead of
// N / hop times (config 4, 75 % overlap: the L2 absorbed only part of the re-reads, PMC fetch 2.3x the input).
template <typename R, int N, int E, int G, int TWMODE, int PADSHIFT, bool CPLX, bool PSD, int NBUF, int SHIFT = 0>
__global__ __launch_bounds__((N / E) * G, 2) void stft_fused_kernel(SpecArgs a) {
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
    // window in the working precision: Float32 frames are multiplied by the Float32-rounded window (one rounding more than the
    // reference's Float64 product rounded once, periodograms.jl:62 -- 6e-8 relative, far inside the Float32 FFT's own error),
    // which halves the window registers and drops four conversions per sample from the VALU stream
    R w[E];
    {
        double wd[E];
        load_window_regs<E, T>(wd, a.win, a.n, t);
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = (R)wd[e];
    }
    const bool havewin = a.win != nullptr;

    const TT* sc = static_cast<const TT*>(a.s) + ch * a.lds_;
    const int64_t nslots = (int64_t)gridDim.x * G;
    int64_t wbase = ((int64_t)blockIdx.x * G + slot) * a.run_len, wj = 0;
    auto unit_cur = [&](bool more) { return (more && wbase + wj < a.K) ? wbase + wj : a.K; };
    auto walk = [&]() {
        if (++wj == a.run_len) {
            wj = 0;
            wbase += nslots * a.run_len;
        }
    };
    const int64_t niter = a.niter;
    const R m1 = (R)(1.0 / a.r), m2 = (R)(2.0 / a.r);

    TT ra[E];
    int64_t held = -2;   // frame whose raw samples ra[] holds
    auto issue = [&](int64_t f) {
        const bool live = f < a.K;
        const int64_t start = f * a.hop;
        const __amdgpu_buffer_rsrc_t r0 = io::make_rsrc(sc + start, live ? std::min<int64_t>(a.n, a.len - start) * SZ : 0);
        if constexpr (SHIFT > 0) {
            static_assert(SHIFT < E, "a frame shift leaves samples to reuse");
            if (live && f == held + 1) {   // wave-uniform: the next frame of the same run
#pragma unroll
                for (int e = 0; e < E - SHIFT; ++e) ra[e] = ra[e + SHIFT];
                io::load_window_tail<TT, E, T, E - SHIFT>(ra, r0, t);
                held = f;
                return;
            }
            held = live ? f : -2;
        }
        io::load_window<TT, E, T>(ra, r0, 0, t);
    };
    int64_t fcur = unit_cur(niter > 0);
    issue(fcur);
    for (int64_t it = 0; it < niter; ++it) {
        const int64_t f = fcur;
        walk();
        fcur = unit_cur(it + 1 < niter);
        cx<R> v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if constexpr (CPLX) v[e] = havewin ? cx<R>{ra[e].x * w[e], ra[e].y * w[e]} : ra[e];
            else v[e] = {havewin ? ra[e] * w[e] : ra[e], (R)0};
        }
        issue(fcur);   // the next frame's samples stream in while this one is transformed
        fft::wg_fft<C, -1, TWMODE, PADSHIFT, NBUF, 0>(v, t, tw, twsrc, lds);
        if constexpr (C::P > 1 && NBUF > 1 && ((C::P - 1) % NBUF) != 0) fft::wg_sync<T>();  // NBUF == 1: wg_fft already ends every exchange with a barrier
        // column store: bins k = t + T*e < nout, contiguous across lanes
        const bool live = f < a.K;
        if (a.memprio & 2) __builtin_amdgcn_s_setprio(3);
        if constexpr (PSD) {
            R* col = static_cast<R*>(a.out) + ch * a.chs + f * a.ldo;
            const __amdgpu_buffer_rsrc_t wr = io::make_rsrc(col, live ? (int64_t)a.nout * (int64_t)sizeof(R) : 0);
            R old[E];
            if (a.accumulate) io::load_window<R, E, T>(old, wr, 0, t);   // wave-uniform branch; the column is this slot's alone
            io::store_window<R, E, T>(
                [&](int e) {
                    const int k = t + T * e;
                    R m = m1;
                    if (a.onesided && !(k == 0 || (k == a.nout - 1 && N % 2 == 0))) m = m2;
                    const R p = (v[e].x * v[e].x + v[e].y * v[e].y) * m;
                    return a.accumulate ? p + old[e] : p;
                },
                wr, 0, t);
        } else {
            cx<R>* col = static_cast<cx<R>*>(a.out) + ch * a.chs + f * a.ldo;
            const __amdgpu_buffer_rsrc_t wr = io::make_rsrc(col, live ? (int64_t)a.nout * (int64_t)sizeof(cx<R>) : 0);
            io::store_window<cx<R>, E, T>([&](int e) { return v[e]; }, wr, 0, t);
        }
        if (a.memprio & 2) __builtin_amdgcn_s_setprio(0);
    }
}

// ---- STFT / spectrogram of REAL signals: two frames per complex transform ----------------------------------------------
// z = w (a + i b) with a, b two consecutive frames; after the forward transform the two spectra are untangled with the
// mirror bin,  A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2i),  for the nfft/2+1 non-redundant
// bins.  Z[N-k] lives in another thread (bin N-k = (T-t) + T (E-1-e)), so the spectrum takes one more trip through LDS
// -- one exchange instead of a second transform's P-1 exchanges and all of its butterflies.
template <typename R, int N, int E, int G, int TWMODE, int PADSHIFT, bool PSD, int MINW, int NBUF, bool MT = false>
__global__ __launch_bounds__((N / E) * G, MINW) void stft_pair_kernel(SpecArgs a) {
    using C = fft::Cfg<N, E>;
    constexpr int T = C::T, H = E / 2;
    static_assert(T % 64 == 0 && E % 2 == 0, "a transform must own whole wavefronts");
    constexpr int NTWA = C::NTW > 0 ? C::NTW : 1;
    constexpr int REGION = fft::wg_lds_elems<C, PADSHIFT, NBUF>();
    constexpr int64_t SZ = (int64_t)sizeof(R);
    __shared__ __attribute__((aligned(16))) cx<R> lds_all[G * REGION];
    const int t = threadIdx.x % T;
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
    const R m1 = (R)(1.0 / a.r), m2 = (R)(2.0 / a.r);
    using OT = std::conditional_t<PSD, R, cx<R>>;

    R ra[E], rb[E];
    auto issue = [&](int64_t u) {   // frames 2u and 2u+1 (the second one may not exist)
        const int64_t fa = 2 * u, fb = 2 * u + 1;
        const int64_t sa = fa * a.hop, sb = fb * a.hop;
        const __amdgpu_buffer_rsrc_t r0 = io::make_rsrc(sc + sa, fa < a.K ? std::min<int64_t>(a.n, a.len - sa) * SZ : 0);
        const __amdgpu_buffer_rsrc_t r1 = io::make_rsrc(sc + sb, fb < a.K ? std::min<int64_t>(a.n, a.len - sb) * SZ : 0);
        io::load_window<R, E, T>(ra, r0, 0, t);
        io::load_window<R, E, T>(rb, r1, 0, t);
    };
    int64_t ucur = unit_cur(niter > 0);
    issue(ucur);
    for (int64_t it = 0; it < niter; ++it) {
        const int64_t u = ucur;
        walk();
        ucur = unit_cur(it + 1 < niter);
        if constexpr (MT && PSD) {
            // multitaper PSD (mt_pgram!, multitaper.jl:239-243): the frame pair stays in registers while every taper is applied,
            // transformed, untangled and accumulated; one store per bin at the end
            static_assert(PSD, "multitaper accumulates powers");
            R pa[H], pb[H], pna = (R)0, pnb = (R)0;
#pragma unroll
            for (int e = 0; e < H; ++e) pa[e] = pb[e] = (R)0;
            const int mbase = fft::lds_pad<PADSHIFT>((N - t) & (N - 1));
            for (int k = 0; k < a.ntapers; ++k) {
                const double* wk = a.win + (int64_t)k * a.n;
                cx<R> v[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = t + T * e;
                    const R wv = i < a.n ? (R)wk[i] : (R)0;
                    v[e] = {ra[e] * wv, rb[e] * wv};
                }
                fft::wg_fft<C, -1, TWMODE, PADSHIFT, NBUF, 0>(v, t, tw, twsrc, lds);
                if constexpr (C::P > 1 && NBUF > 1) fft::wg_sync<T>();
                {
                    const int base = fft::lds_pad<PADSHIFT>(t);
#pragma unroll
                    for (int e = 0; e < E; ++e) lds[base + fft::lds_padc<PADSHIFT>(T * e)] = v[e];
                }
                fft::wg_sync<T>();
                const double rk = a.rinv[k];
                const R k1 = (R)rk, k2 = (R)(2.0 * rk);
                auto power = [&](cx<R> z, cx<R> p, R m, R& qa, R& qb) {
                    const cx<R> A = {(z.x + p.x) * (R)0.5, (z.y - p.y) * (R)0.5};
                    const cx<R> B = {(z.y + p.y) * (R)0.5, (p.x - z.x) * (R)0.5};
                    qa += (A.x * A.x + A.y * A.y) * m;
                    qb += (B.x * B.x + B.y * B.y) * m;
                };
#pragma unroll
                for (int e = 0; e < H; ++e) {
                    const cx<R> p = e == 0 ? lds[mbase] : lds[fft::lds_pad<PADSHIFT>(N - t - T * e)];
                    const bool dc = (t + T * e) == 0;
                    power(v[e], p, (a.onesided && !dc) ? k2 : k1, pa[e], pb[e]);
                }
                if (t == 0) power(v[H], v[H], k1, pna, pnb);       // Nyquist (nfft even): weight 1/r in both layouts
                if constexpr (C::P > 1) fft::wg_sync<T>();
            }
            issue(ucur);
            const int64_t fa = 2 * u, fb = 2 * u + 1;
            R* colA = static_cast<R*>(a.out) + ch * a.chs + fa * a.ldo;
            R* colB = static_cast<R*>(a.out) + ch * a.chs + fb * a.ldo;
            const __amdgpu_buffer_rsrc_t wa = io::make_rsrc(colA, fa < a.K ? (int64_t)a.nout * (int64_t)sizeof(R) : 0);
            const __amdgpu_buffer_rsrc_t wb = io::make_rsrc(colB, fb < a.K ? (int64_t)a.nout * (int64_t)sizeof(R) : 0);
#pragma unroll
            for (int e = 0; e < H; ++e) {
                const int kb = t + T * e;
                io::Ld<R>::store(pa[e], wa, kb * (int)sizeof(R));
                io::Ld<R>::store(pb[e], wb, kb * (int)sizeof(R));
                if (!a.onesided && kb != 0) {
                    io::Ld<R>::store(pa[e], wa, (N - kb) * (int)sizeof(R));
                    io::Ld<R>::store(pb[e], wb, (N - kb) * (int)sizeof(R));
                }
            }
            if (t == 0) {
                io::Ld<R>::store(pna, wa, (N / 2) * (int)sizeof(R));
                io::Ld<R>::store(pnb, wb, (N / 2) * (int)sizeof(R));
            }
            continue;
        }
        cx<R> v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = {ra[e] * w[e], rb[e] * w[e]};   // w == 1 beyond... load_window_regs gives 1 without a window, 0 past n
        issue(ucur);
        fft::wg_fft<C, -1, TWMODE, PADSHIFT, NBUF, 0>(v, t, tw, twsrc, lds);
        // mirror exchange through the (now idle) first LDS buffer: natural order, so both the writes and the descending reads
        // are contiguous across lanes
        if constexpr (C::P > 1 && NBUF > 1) fft::wg_sync<T>();   // the last gather of the transform may still be reading buffer (P-2) % NBUF
        {
            const int base = fft::lds_pad<PADSHIFT>(t);
#pragma unroll
            for (int e = 0; e < E; ++e) lds[base + fft::lds_padc<PADSHIFT>(T * e)] = v[e];
        }
        fft::wg_sync<T>();
        const int64_t fa = 2 * u, fb = 2 * u + 1;
        const bool liveA = fa < a.K, liveB = fb < a.K;
        OT* colA = static_cast<OT*>(a.out) + ch * a.chs + fa * a.ldo;
        OT* colB = static_cast<OT*>(a.out) + ch * a.chs + fb * a.ldo;
        const __amdgpu_buffer_rsrc_t wa = io::make_rsrc(colA, liveA ? (int64_t)a.nout * (int64_t)sizeof(OT) : 0);
        const __amdgpu_buffer_rsrc_t wb = io::make_rsrc(colB, liveB ? (int64_t)a.nout * (int64_t)sizeof(OT) : 0);
        auto emit = [&](int k, cx<R> z, cx<R> p) {   // bin k <= N/2 of both frames from Z[k] = z and Z[N-k] = p
            const cx<R> A = {(z.x + p.x) * (R)0.5, (z.y - p.y) * (R)0.5};
            const cx<R> B = {(z.y + p.y) * (R)0.5, (p.x - z.x) * (R)0.5};
            const int off = k * (int)sizeof(OT);
            if constexpr (PSD) {
                R m = m1;
                if (a.onesided && !(k == 0 || (k == N / 2 && N % 2 == 0))) m = m2;
                R pa = (A.x * A.x + A.y * A.y) * m, pb = (B.x * B.x + B.y * B.y) * m;
                if (a.accumulate) {   // multitaper: fft2pow! adds this taper's power to the column (wave-uniform branch)
                    pa += io::Ld<R>::load(wa, off);
                    pb += io::Ld<R>::load(wb, off);
                }
                io::Ld<R>::store(pa, wa, off);
                io::Ld<R>::store(pb, wb, off);
                if (!a.onesided && k != 0 && k != N / 2) {   // real signal, two-sided output: the mirrored bin carries the same power
                    const int offm = (N - k) * (int)sizeof(OT);
                    io::Ld<R>::store(pa, wa, offm);
                    io::Ld<R>::store(pb, wb, offm);
                }
            } else {
                io::Ld<cx<R>>::store(A, wa, off);
                io::Ld<cx<R>>::store(B, wb, off);
                if (!a.onesided && k != 0 && k != N / 2) {   // fft2oneortwosided!: out[N-k] = conj(out[k])
                    const int offm = (N - k) * (int)sizeof(OT);
                    io::Ld<cx<R>>::store(cx<R>{A.x, -A.y}, wa, offm);
                    io::Ld<cx<R>>::store(cx<R>{B.x, -B.y}, wb, offm);
                }
            }
        };
        // bins k = t + T e, e < E/2, are <= N/2 - 1 + ... (k < N/2); their mirrors N - k sit at index (N - t) - T e
        {
            const int mbase = fft::lds_pad<PADSHIFT>((N - t) & (N - 1));   // t == 0: bin 0 mirrors itself (index 0)
#pragma unroll
            for (int e = 0; e < H; ++e) {
                cx<R> p;
                if (e == 0) p = lds[mbase];
                else p = lds[fft::lds_pad<PADSHIFT>(N - t - T * e)];
                emit(t + T * e, v[e], p);
            }
            if (t == 0) emit(N / 2, v[H], v[H]);   // the Nyquist bin is thread 0's element E/2 and its own mirror
        }
        if constexpr (C::P > 1) fft::wg_sync<T>();   // the next transform's first scatter reuses this buffer
    }
}

#include "spectral_gx.h"

template <typename R, bool CPLX>
int stft_exec_rocfft(mdsp_stft_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, void* out, int64_t ldo, int64_t chs, hipStream_t st) {
    using TT = std::conditional_t<CPLX, cx<R>, R>;
    const int64_t nfft = pl->nfft, n = pl->n, hop = pl->n - pl->noverlap;
    const int64_t K = mdsp_frame_count(len, n, pl->noverlap);
    const int nspec = (int)(CPLX ? nfft : nfft / 2 + 1);
    const int64_t nunits = K * nch;
    if (nunits == 0) return MDSP_OK;
    const int64_t batch = chunk_units_rocfft_spectral(CPLX, (int64_t)sizeof(R), nfft, nunits, rocfft_chunk_bytes());
    if (pl->batch != batch) {
        MDSP_TRY(pl->fr.reserve((size_t)(sizeof(TT) * nfft * batch)));
        MDSP_TRY(pl->spec.reserve((size_t)(sizeof(cx<R>) * nspec * batch)));
        MDSP_TRY(pl->fwd.create(CPLX ? FftKind::C2C_FWD : FftKind::R2C, sizeof(R) == 8, nfft, batch, false));
        pl->batch = batch;
    }
    const int gx = (int)std::min<int64_t>(cdiv(nfft, 256), 8);
    const int nout = (int)pl->nout;
    const bool direct = !pl->psd_only && nout == nspec && ldo == nout && (nch == 1 || chs == K * (int64_t)nout) && !MDSP_DBG(stft_nodirect);
    for (int64_t u0 = 0; u0 < nunits; u0 += batch) {
        const int64_t cnt = std::min<int64_t>(batch, nunits - u0);
        hipLaunchKernelGGL(frame_window_kernel<TT>, dim3((unsigned)cnt, gx), dim3(256), 0, st, (const TT*)s, pl->fr.as<TT>(),
                           pl->have_win ? pl->win_ptr : nullptr, lds_, K, hop, (int)n, (int)nfft, u0, nunits);
        MDSP_LAUNCH_CHECK();
        // raw STFT whose output matrix has exactly the batched transform's layout (contiguous columns of nspec bins, channels
        // back to back): full batches are transformed straight into it, one pass over the spectra less
        if (direct && cnt == batch) {
            MDSP_TRY(pl->fwd.exec(pl->fr.p, static_cast<cx<R>*>(out) + u0 * nout, st));
            continue;
        }
        MDSP_TRY(pl->fwd.exec(pl->fr.p, pl->spec.p, st));
        const dim3 g((unsigned)cnt, gx);
        if (pl->psd_only)
            hipLaunchKernelGGL((stft_store_kernel<R, true, !CPLX>), g, dim3(256), 0, st, pl->spec.as<cx<R>>(), out, nspec, (int)nfft, nout, K, ldo, chs, u0,
                               nunits, pl->r, pl->onesided, pl->accumulate);
        else
            hipLaunchKernelGGL((stft_store_kernel<R, false, !CPLX>), g, dim3(256), 0, st, pl->spec.as<cx<R>>(), out, nspec, (int)nfft, nout, K, ldo, chs, u0,
                               nunits, pl->r, pl->onesided, 0);
        MDSP_LAUNCH_CHECK();
    }
    return MDSP_OK;
}

template <typename R, int N, bool CPLX> int stft_launch_n(mdsp_stft_plan_s* pl, SpecArgs& a, hipStream_t st) {
    using Gm = Geo<R, N>;
    constexpr int E = Gm::E, G = Gm::G, NBUF = Gm::NBUF;
    constexpr bool TWREG = Gm::TWREG;
    constexpr int threads = (N / E) * G;
    const int64_t work = cdiv(a.K, G);
    int grid = 1;
    auto run = [&](auto kern) -> int {
        MDSP_TRY(grid_for(kern, threads, work, a.nch, &grid));
        set_schedule(a, a.K, (int64_t)grid * G);
        hipLaunchKernelGGL(kern, dim3(grid, (unsigned)a.nch), dim3(threads), 0, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    };
    if constexpr (!CPLX) {
        // real signals: two frames per transform (stft_pair_kernel); MDSP_STFT_NOPAIR=1 keeps the one-frame-per-transform kernel
        const bool nopair = MDSP_DBG(stft_nopair);
        if (!nopair && a.n <= N) {
            const int64_t units = cdiv(a.K, 2);
            a.units_per_ch = units;
            auto runp = [&](auto kern) -> int {
                MDSP_TRY(grid_for(kern, threads, cdiv(units, G), a.nch, &grid));
                set_schedule(a, units, (int64_t)grid * G);
                hipLaunchKernelGGL(kern, dim3(grid, (unsigned)a.nch), dim3(threads), 0, st, a);
                MDSP_LAUNCH_CHECK();
                return MDSP_OK;
            };
            if (pl->psd_only && a.ntapers > 0) return runp(stft_pair_kernel<R, N, E, G, TWREG, pad_default<R>(), true, 2, NBUF, true>);
            if (pl->psd_only) return runp(stft_pair_kernel<R, N, E, G, TWREG, pad_default<R>(), true, 2, NBUF>);
            return runp(stft_pair_kernel<R, N, E, G, TWREG, pad_default<R>(), false, 2, NBUF>);
        }
    }
    if constexpr (CPLX && sizeof(R) == 4) {   // complex Float32 frames that advance by whole elements: overlap stays in registers
        constexpr int T = N / E;
        const int shift = (!MDSP_DBG(stft_noshift) && a.n == N && a.hop % T == 0 && a.hop / T < E) ? (int)(a.hop / T) : 0;
#define MDSP_STFT_GEN(S) \
    (pl->psd_only ? run(stft_fused_kernel<R, N, E, G, TWREG, pad_default<R>(), CPLX, true, NBUF, S>) \
                  : run(stft_fused_kernel<R, N, E, G, TWREG, pad_default<R>(), CPLX, false, NBUF, S>))
        if constexpr (E > 4) {
            if (shift == 1) return MDSP_STFT_GEN(1);
            if (shift == 2) return MDSP_STFT_GEN(2);
            if (shift == 4) return MDSP_STFT_GEN(4);
        }
        if constexpr (E > 8) {   // nfft 1024: one wavefront per transform (Geo), 16 elements per thread
            if (shift == 8) return MDSP_STFT_GEN(8);
        }
#undef MDSP_STFT_GEN
    }
    if (pl->psd_only) return run(stft_fused_kernel<R, N, E, G, TWREG, pad_default<R>(), CPLX, true, NBUF>);
    return run(stft_fused_kernel<R, N, E, G, TWREG, pad_default<R>(), CPLX, false, NBUF>);
}

template <typename R, bool CPLX>
int stft_exec_fused(mdsp_stft_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, void* out, int64_t ldo, int64_t chs, hipStream_t st) {
    const int64_t K = mdsp_frame_count(len, pl->n, pl->noverlap), hop = pl->n - pl->noverlap;
    if (K == 0) return MDSP_OK;
    const double* win = pl->have_win ? pl->win_ptr : nullptr;
    // multitaper plans come here once per taper (accumulate) on every route but the power-of-two kernels of real signals
    switch (pl->route) {
        case MDSP_ROUTE_POW2: {
            SpecArgs a{};
            a.s = s; a.out = out; a.table = pl->table.p; a.win = win; a.accumulate = pl->accumulate; a.ntapers = pl->mt_ntapers; a.rinv = pl->mt_rinv;
            a.len = len; a.lds_ = lds_; a.K = K; a.hop = hop; a.units_per_ch = K; a.nch = nch; a.ldo = ldo; a.chs = chs;
            a.n = (int)pl->n; a.nout = (int)pl->nout; a.onesided = pl->onesided; a.r = pl->r;
            switch (pl->nfft) {
                case 256: return stft_launch_n<R, 256, CPLX>(pl, a, st);
                case 512: return stft_launch_n<R, 512, CPLX>(pl, a, st);
                case 1024: return stft_launch_n<R, 1024, CPLX>(pl, a, st);
                case 2048: return stft_launch_n<R, 2048, CPLX>(pl, a, st);
                case 4096: return stft_launch_n<R, 4096, CPLX>(pl, a, st);
                case 8192:
                    if constexpr (sizeof(R) == 4) return stft_launch_n<R, 8192, CPLX>(pl, a, st);
                default: break;
            }
            MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "fused STFT does not support nfft=%lld", (long long)pl->nfft);
        }
        case MDSP_ROUTE_GEN:   // mixed-radix sizes (spectral_gen.hip)
            return gen_stft(pl, s, len, nch, lds_, out, ldo, chs, K, hop, win, st);
        case MDSP_ROUTE_GX: {   // run-time-schedule kernel (spectral_gx.h)
            GxArgs g{};
            g.s = s; g.out = out; g.lds_ = lds_; g.K = K; g.hop = hop; g.nch = nch; g.ldo = ldo; g.chs = chs;
            g.n = (int)pl->n; g.nfft = (int)pl->nfft; g.nout = (int)pl->nout; g.onesided = pl->onesided; g.psd = pl->psd_only; g.accumulate = pl->accumulate; g.r = pl->r;
            int64_t ngroups = 0;
            return gx_launch<R, CPLX, 1>(pl->gx, g, win, pl->dtype, st, &ngroups, nullptr);
        }
        case MDSP_ROUTE_CTBIG_COLS: {   // a single-workgroup compile-time schedule (spectral_ctbig_cols.hip)
            CtBigColsArgs c{};
            c.s = s; c.out = out; c.win = win; c.len = len; c.lds_ = lds_; c.K = K; c.hop = hop; c.nch = nch; c.ldo = ldo; c.chs = chs;
            c.n = (int)pl->n; c.nfft = pl->nfft; c.nout = (int)pl->nout; c.onesided = pl->onesided; c.psd = pl->psd_only; c.accumulate = pl->accumulate; c.r = pl->r;
            return ctbig_stft(pl->ctbig, pl->dtype, c, st);
        }
        case MDSP_ROUTE_BIG: {   // nfft above the one-workgroup sizes (bigfft.hip)
            using TT = std::conditional_t<CPLX, cx<R>, R>;
            const size_t osz = pl->psd_only ? sizeof(R) : sizeof(cx<R>);
            for (int64_t c = 0; c < nch; ++c)
                MDSP_TRY(big::stft(pl->big, pl->dtype, pl->n, pl->nfft, static_cast<const TT*>(s) + c * lds_, K, hop, win,
                                   static_cast<char*>(out) + (size_t)(c * chs) * osz, ldo, pl->nout, pl->onesided, pl->psd_only, pl->accumulate, pl->r, st));
            return MDSP_OK;
        }
        default: MDSP_FAIL(MDSP_ERR_ASSERTION, "STFT plan with route %d on the fused engine", pl->route);
    }
}

}  // namespace

namespace mdsp {

int stft_dispatch(mdsp_stft_plan_s* plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_, void* out_dev, int64_t ldo, int64_t chs, hipStream_t st) {
    const bool cplx = dtype_is_complex(plan->dtype), dbl = dtype_is_double(plan->dtype);
    if (plan->engine == MDSP_ENGINE_ROCFFT) {
        if (cplx) return dbl ? stft_exec_rocfft<double, true>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st)
                             : stft_exec_rocfft<float, true>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st);
        return dbl ? stft_exec_rocfft<double, false>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st)
                   : stft_exec_rocfft<float, false>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st);
    }
    if (cplx) return dbl ? stft_exec_fused<double, true>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st)
                         : stft_exec_fused<float, true>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st);
    return dbl ? stft_exec_fused<double, false>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st)
               : stft_exec_fused<float, false>(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, st);
}

// The root tables of the plan's route, at plan creation (multitaper plans: of their STFT plan).  The working-precision window of the column kernels stays
// per launch: a multitaper plan points win_ptr at another taper for each pass (convert_window at those sites).
int prepare_stft_tables(mdsp_stft_plan_s* pl) {
    const bool dbl = dtype_is_double(pl->dtype);
    switch (pl->route) {
        case MDSP_ROUTE_POW2:
        case MDSP_ROUTE_GEN: return upload_roots(pl->table, dbl, pl->nfft);
        case MDSP_ROUTE_GX: return dbl ? gx_prepare<double>(pl->gx, pl->dtype, pl->nfft, false) : gx_prepare<float>(pl->gx, pl->dtype, pl->nfft, false);
        case MDSP_ROUTE_CTBIG_COLS: return upload_roots(pl->ctbig.roots, dbl, pl->nfft);
        default: return MDSP_OK;
    }
}

}  // namespace mdsp

extern "C" {

int mdsp_stft_plan_create(mdsp_stft_plan* plan, int64_t n, int64_t noverlap, int64_t nfft, const double* window_host, double r, int onesided,
                          int psd_only, int dtype, int engine) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype %d", dtype);
    if (onesided && dtype_is_complex(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "cannot compute one-sided FFT of a complex signal");
    MDSP_TRY(check_split(n, noverlap, nfft));
    if (psd_only && !(r > 0)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "normalisation r must be positive");
    SpecRoute rt;
    MDSP_TRY(choose_spectral_route(engine, dtype, nfft, 1, &rt));
    auto pl = new mdsp_stft_plan_s();
    pl->dtype = dtype;
    pl->engine = rt.engine;
    pl->route = rt.route;
    pl->r0 = rt.r0;
    pl->onesided = onesided ? 1 : 0;
    pl->psd_only = psd_only ? 1 : 0;
    pl->n = n;
    pl->noverlap = noverlap;
    pl->nfft = nfft;
    pl->nout = onesided ? nfft / 2 + 1 : nfft;
    pl->r = r;
    int st = MDSP_OK;
    if (window_host) {
        pl->have_win = true;
        st = pl->win.reserve(sizeof(double) * (size_t)n);
        if (st == MDSP_OK && hipMemcpy(pl->win.p, window_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
            st = set_error(MDSP_ERR_DEVICE, "window upload failed");
        pl->win_ptr = pl->win.as<double>();
    }
    if (st == MDSP_OK) st = prepare_stft_tables(pl);
    if (st != MDSP_OK) {
        delete pl;
        return st;
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_stft_plan_destroy(mdsp_stft_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_stft_plan_info(mdsp_stft_plan plan, int64_t* nout, int* engine_used) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nout) *nout = plan->nout;
    if (engine_used) *engine_used = plan->engine;
    return MDSP_OK;
}

int mdsp_stft_exec(mdsp_stft_plan plan, const void* s_dev, int64_t len, int64_t nch, int64_t lds_, void* out_dev, int64_t ldo, int64_t chs,
                   void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (len < 0 || nch < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    const int64_t K = mdsp_frame_count(len, plan->n, plan->noverlap);
    if (nch == 0 || K == 0) return MDSP_OK;
    if (!out_dev || !s_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (ldo < plan->nout) MDSP_FAIL(MDSP_ERR_DIMENSION, "column stride smaller than the column length");
    if (nch > 1 && (lds_ < len || chs < ldo * (K - 1) + plan->nout)) MDSP_FAIL(MDSP_ERR_DIMENSION, "channel stride too small");
    if (nch > 65535) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "more than 65535 channels per call");
    return stft_dispatch(plan, s_dev, len, nch, lds_, out_dev, ldo, chs, as_stream(stream));
}

// stft / spectrogram of host arrays (periodograms.jl:872-897 takes a host vector and returns a host matrix): channel by channel, runs of whole
// frames.  Chunk c of a channel holds frames [k0, k1): their samples [k0 hop, (k1-1) hop + n) go up, their columns come down -- every frame is the
// same frame the device-resident call transforms, so the two agree bit for bit.  The output is 2-8x the input (40 B per sample at config 4), which is
// why the chunk is sized by its OUTPUT and why the pipeline keeps the D2H stream busy while the next chunk uploads (hostpipe.h).
int mdsp_stft_exec_host(mdsp_stft_plan plan, const void* s_host, int64_t len, int64_t nch, int64_t lds_, void* out_host, int64_t ldo, int64_t chs,
                        int flags) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (len < 0 || nch < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    if (plan->accumulate || plan->mt_ntapers > 0) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "multitaper plans have no host-array entry");
    const int64_t n = plan->n, hop = plan->n - plan->noverlap, nout = plan->nout;
    const int64_t K = mdsp_frame_count(len, n, plan->noverlap);
    if (nch == 0 || K == 0) return MDSP_OK;
    if (!out_host || !s_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (ldo < nout) MDSP_FAIL(MDSP_ERR_DIMENSION, "column stride smaller than the column length");
    if (nch > 1 && (lds_ < len || chs < ldo * (K - 1) + nout)) MDSP_FAIL(MDSP_ERR_DIMENSION, "channel stride too small");
    const bool pinned = (flags & MDSP_HOST_PINNED) != 0;
    const size_t esz = dtype_size(plan->dtype);
    const size_t osz = plan->psd_only ? dtype_size(dtype_real_of(plan->dtype)) : dtype_size(dtype_complex_of(plan->dtype));
    // frames per chunk: EVEN -- real signals ride two consecutive frames (2j, 2j+1) per transform, and a chunk that started at an odd frame would
    // pair them differently from the device-resident call (same values up to rounding, not bit for bit)
    int64_t fpc = std::max<int64_t>(2, ((int64_t)tunables().host_chunk_mib << 20) / (int64_t)(nout * (int64_t)osz));
    fpc &= ~int64_t(1);
    const size_t in_cap = (size_t)((fpc - 1) * hop + n) * esz, out_cap = (size_t)fpc * (size_t)nout * osz;
    hostpipe::Session ss(in_cap, out_cap, pinned);
    int rc = ss.status();
    for (int64_t c = 0; c < nch && rc == MDSP_OK; ++c) {
        const char* sc = static_cast<const char*>(s_host) + (size_t)(c * lds_) * esz;
        char* oc = static_cast<char*>(out_host) + (size_t)(c * chs) * osz;
        for (int64_t k0 = 0; k0 < K && rc == MDSP_OK; k0 += fpc) {
            hostpipe::Lane* ln = nullptr;
            if ((rc = ss.acquire(&ln)) != MDSP_OK) break;
            const int64_t k1 = std::min(K, k0 + fpc), cl = (k1 - k0 - 1) * hop + n;
            if ((rc = ss.upload(ln, sc + (size_t)(k0 * hop) * esz, (size_t)cl * esz, (size_t)cl * esz, 1)) != MDSP_OK) break;
            if ((rc = mdsp_stft_exec(plan, ln->din.p, cl, 1, cl, ln->dout.p, nout, nout * (k1 - k0), ss.kstream())) != MDSP_OK) break;
            rc = ss.download(ln, oc + (size_t)(k0 * ldo) * osz, (size_t)ldo * osz, (size_t)nout * osz, (size_t)(k1 - k0), 0, (size_t)nout * osz);
        }
    }
    return ss.finish(rc);
}

}  // extern "C"
