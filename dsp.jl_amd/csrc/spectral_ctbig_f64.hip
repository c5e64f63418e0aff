// Float64 / ComplexF64 on the single-workgroup compile-time schedules of ctbig_sizes.h (round 6): Welch sums and the column modes for every table size whose
// ONE buffer of 16-byte elements and twiddle tables fit 160 KiB (up to 9600 points) -- DSP.jl's default element type at the 7-smooth sizes that have no schedule in
// ct_sched.h's tables, which ran the run-time schedule (0.5 - 0.9 TB/s).  The lean form throughout: window loaded beside the samples (register-consumed modes),
// table twiddles derived from ~2 sqrt(R) values, no group padding (the Float64 rule of spectral_gen.h), real-signal columns on the one buffer.
// Reference loops: periodograms.jl:746-759 (welch_pgram_helper!), :872-897 (stft), :57-69 (ArraySplit), :142-172 / :234-244 (fft2pow!, fft2oneortwosided!).
#include <algorithm>

#include "common.h"
#include "devio.h"
#include "fft_lds.h"
#include "hostfft.h"
#include "spectral_ctcols.h"
#include "spectral_tables.h"

using namespace mdsp;
using mdsp::fft::cx;

namespace {
#include "spectral_gen.h"

#include "ctbig_sizes.h"

constexpr int f64_flags(int f) { return ((f) & ~(512 | 1024 | 8192 | 32768 | 65536)) | 16 | 2048 | 4096 | 16384; }
constexpr int f64_flags_real_cols(int f) { return (f64_flags(f) & ~4096) | 65536; }
template <typename S> constexpr bool f64_fits() { return sizeof(cx<double>) * ((size_t)S::NP + S::TWS + S::NTWHI) <= (size_t)160 * 1024; }

// MODE 0: Welch sums; 1: columns
template <bool CPLX, int MODE> int dispatch64(GenArgs& a, int64_t nch, hipStream_t st, int64_t* nslots, DevBuf* partial) {
    switch (a.N) {
#define MDSP_X(N, T, F, ...)                                                                                              \
    case N: {                                                                                                             \
        using S = CtSched<N, T, (MODE == 1 && !CPLX) ? f64_flags_real_cols(F) : f64_flags(F), __VA_ARGS__>;               \
        if constexpr (f64_fits<S>()) return gen_ct_launch<double, CPLX, MODE, S>(a, nch, st, nslots, partial);            \
        break;                                                                                                            \
    }
        MDSP_CTBIG_SIZES(MDSP_X)
        MDSP_CTBIG_LEAN_SIZES(MDSP_X)
        MDSP_CTBIG_SMALL_SIZES(MDSP_X)
#undef MDSP_X
        default: break;
    }
    MDSP_FAIL(MDSP_ERR_ASSERTION, "no Float64 single-workgroup compile-time schedule of %d points", a.N);
}

}  // namespace

namespace mdsp {
bool ctbig64_ok(int64_t nfft) {
    switch (nfft) {
#define MDSP_X(N, T, F, ...) \
    case N: return f64_fits<CtSched<N, T, f64_flags(F), __VA_ARGS__>>();
        MDSP_CTBIG_SIZES(MDSP_X)
        MDSP_CTBIG_LEAN_SIZES(MDSP_X)
        MDSP_CTBIG_SMALL_SIZES(MDSP_X)
#undef MDSP_X
        default: return false;
    }
}

int ctbig64_welch(CtColsPlan& cp, bool cplx, const void* s, int64_t lds_, int64_t K, int64_t hop, int64_t nch, int n, int64_t nfft, const double* win_dev, hipStream_t st,
                  int64_t* nslots, DevBuf* partial, int accumulate) {
    if (!ctbig64_ok(nfft)) MDSP_FAIL(MDSP_ERR_ASSERTION, "nfft=%lld has no Float64 single-workgroup compile-time schedule", (long long)nfft);
    if (!cp.roots.p || !cp.win.p) MDSP_FAIL(MDSP_ERR_ASSERTION, "the tables of nfft=%lld were not built at plan creation", (long long)nfft);
    GenArgs g{};
    g.s = s; g.roots = cp.roots.p; g.win = win_dev; g.winr = cp.win.p;
    g.lds_ = lds_; g.K = K; g.hop = hop; g.nch = nch; g.units_per_ch = cplx ? K : cdiv(K, 2);
    g.n = n; g.N = (int)nfft; g.accumulate = accumulate;
    return cplx ? dispatch64<true, 0>(g, nch, st, nslots, partial) : dispatch64<false, 0>(g, nch, st, nslots, partial);
}

int ctbig64_stft(CtColsPlan& cp, bool cplx, const CtBigColsArgs& c, hipStream_t st) {
    if (!ctbig64_ok(c.nfft)) MDSP_FAIL(MDSP_ERR_ASSERTION, "nfft=%lld has no Float64 single-workgroup column schedule", (long long)c.nfft);
    if (!cp.roots.p) MDSP_FAIL(MDSP_ERR_ASSERTION, "the roots of nfft=%lld were not built at plan creation", (long long)c.nfft);
    if (cplx) MDSP_TRY(convert_window(cp.win, true, c.win, c.n, c.nfft, st));   // (per launch: the window of a multitaper plan changes between tapers)
    GenArgs g{};
    g.s = c.s; g.out = c.out; g.roots = cp.roots.p; g.win = c.win; g.winr = cp.win.p;
    g.len = c.len; g.lds_ = c.lds_; g.K = c.K; g.hop = c.hop; g.nch = c.nch; g.ldo = c.ldo; g.chs = c.chs;
    g.units_per_ch = cplx ? c.K : cdiv(c.K, 2);
    g.n = c.n; g.N = (int)c.nfft; g.nout = c.nout; g.onesided = c.onesided; g.psd = c.psd; g.accumulate = c.accumulate; g.r = c.r;
    int64_t nslots = 0;
    return cplx ? dispatch64<true, 1>(g, c.nch, st, &nslots, nullptr) : dispatch64<false, 1>(g, c.nch, st, &nslots, nullptr);
}
}  // namespace mdsp
