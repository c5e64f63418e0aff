// The mixed-radix kernels of spectral_gen.h, Welch sums (MODE 0) and STFT columns (MODE 1) in ONE unit: a size's two modes mostly share their schedule
// type CtSched<...>, whose members have internal linkage, and a kernel compiles differently when the other mode's kernel of the same schedule is not
// beside it.  welch.hip and stft.hip reach them through gen_welch / gen_stft (spectral_plan.h), as they reach spectral_ct*.hip.
#include <algorithm>

#include "common.h"
#include "devio.h"
#include "fft_lds.h"
#include "spectral_tables.h"
#include "welch_plan.h"
#include "spectral_plan.h"

using namespace mdsp;
using mdsp::fft::cx;

namespace {

#include "spectral_gen.h"

// partial rows per slot in pl->partial (the Float64 accumulator protocol of welch.hip); *ngroups = rows written
template <typename R, bool CPLX>
int gen_welch_t(mdsp_welch_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, int64_t K, int64_t hop, const double* win, hipStream_t st, int64_t* ngroups) {
    const int64_t N = pl->nfft;
    GenArgs g{};
    g.s = s; g.roots = pl->table.p; g.win = win;
    g.len = len; g.lds_ = lds_; g.K = K; g.hop = hop; g.nch = nch; g.units_per_ch = CPLX ? K : cdiv(K, 2);
    g.n = (int)pl->n; g.N = (int)N; g.nout = (int)pl->nout; g.onesided = pl->onesided; g.r = pl->r;
    if (lean_window_needed(N, sizeof(R) == 8)) {
        if (!pl->winr.p) MDSP_FAIL(MDSP_ERR_ASSERTION, "the working-precision window of nfft=%lld was not built at plan creation", (long long)N);
        g.winr = pl->winr.p;
    }
    return gen_launch<R, CPLX, 0>(g, nch, st, ngroups, &pl->partial);
}

template <typename R, bool CPLX>
int gen_stft_t(mdsp_stft_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, void* out, int64_t ldo, int64_t chs, int64_t K, int64_t hop, const double* win,
               hipStream_t st) {
    GenArgs g{};
    g.s = s; g.out = out; g.roots = pl->table.p; g.win = win;
    g.len = len; g.lds_ = lds_; g.K = K; g.hop = hop; g.nch = nch; g.ldo = ldo; g.chs = chs;
    g.units_per_ch = CPLX ? K : cdiv(K, 2);
    g.n = (int)pl->n; g.N = (int)pl->nfft; g.nout = (int)pl->nout; g.onesided = pl->onesided; g.psd = pl->psd_only; g.accumulate = pl->accumulate; g.r = pl->r;
    if (CPLX && lean_window_needed(pl->nfft, sizeof(R) == 8)) {   // (per launch: the window pointer of a multitaper plan changes between tapers)
        MDSP_TRY(convert_window(pl->winr, true, win, g.n, pl->nfft, st));
        g.winr = pl->winr.p;
    }
    int64_t nslots = 0;
    return gen_launch<R, CPLX, 1>(g, nch, st, &nslots, nullptr);
}

}  // namespace

namespace mdsp {

int gen_welch(mdsp_welch_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, int64_t K, int64_t hop, const double* win, hipStream_t st, int64_t* ngroups) {
    const bool cplx = dtype_is_complex(pl->dtype), dbl = dtype_is_double(pl->dtype);
    if (cplx) return dbl ? gen_welch_t<double, true>(pl, s, len, nch, lds_, K, hop, win, st, ngroups) : gen_welch_t<float, true>(pl, s, len, nch, lds_, K, hop, win, st, ngroups);
    return dbl ? gen_welch_t<double, false>(pl, s, len, nch, lds_, K, hop, win, st, ngroups) : gen_welch_t<float, false>(pl, s, len, nch, lds_, K, hop, win, st, ngroups);
}

int gen_stft(mdsp_stft_plan_s* pl, const void* s, int64_t len, int64_t nch, int64_t lds_, void* out, int64_t ldo, int64_t chs, int64_t K, int64_t hop, const double* win,
             hipStream_t st) {
    const bool cplx = dtype_is_complex(pl->dtype), dbl = dtype_is_double(pl->dtype);
    if (cplx) return dbl ? gen_stft_t<double, true>(pl, s, len, nch, lds_, out, ldo, chs, K, hop, win, st) : gen_stft_t<float, true>(pl, s, len, nch, lds_, out, ldo, chs, K, hop, win, st);
    return dbl ? gen_stft_t<double, false>(pl, s, len, nch, lds_, out, ldo, chs, K, hop, win, st) : gen_stft_t<float, false>(pl, s, len, nch, lds_, out, ldo, chs, K, hop, win, st);
}

}  // namespace mdsp
