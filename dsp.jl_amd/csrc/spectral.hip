// What the spectral products share on the host: the route of a Welch / STFT / spectrogram / periodogram / multitaper plan (choose_spectral_route,
// mdsp_spectral_route_for), the argument checks, framing alone (mdsp_frames) and the dispatch to the run-time-schedule kernels (mdsp::gx_run).
// The products themselves: welch.hip, stft.hip, multitaper.hip, hilbert.hip.
//
// Reference loop being replaced here (src/periodograms.jl):
//   K4  ArraySplit getindex :57-69     buf[i] = s[offset+i] * window[i], zero tail up to nfft
//
// Frame k (0-based) of a channel covers s[k*hop .. k*hop+n), hop = n - noverlap; K = (len-n) div hop + 1 frames
// (the trailing partial frame is dropped, :49-50).  The window is ALWAYS Float64 in the reference (:250): the
// product is formed in double and rounded once to the buffer eltype -- done the same way here.
//
// Engines (a plan's route names the kernel family within one):
//   FUSED  : window, transform and consumer in one kernel, from power-of-two nfft in [256, 8192] (welch.hip, stft.hip) through the mixed-radix and
//            run-time schedules (spectral_gen.h, spectral_gx.h, spectral_ct*.hip) to the multi-pass engine (bigfft.hip).
//   ROCFFT : K4 kernel -> batched rocFFT -> K5/K6 kernel over cache-sized chunks; any nfft.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "devio.h"
#include "fft_lds.h"
#include "hostfft.h"
#include "spectral_tables.h"
#include "spectral_ctrows.h"
#include "spectral_op.h"
#include "spectral_plan.h"
#include "gx_kernels.h"   // (namespace mdsp::gx and the kernel template: ahead of the anonymous namespace that includes spectral_gx.h)

using namespace mdsp;
using mdsp::fft::cx;

namespace {

#include "spectral_gen.h"   // gen_size_ok, gen_ct_size: no kernel is instantiated here
#include "spectral_gx.h"    // gx_choose

bool fused_size_ok(int dtype, int64_t nfft) {
    const bool dbl = dtype_is_double(dtype);
    switch (nfft) {
        case 256: case 512: case 1024: case 2048: case 4096: return true;
        case 8192: return !dbl;
        default: return false;
    }
}

// the column factor of the run-time-schedule kernel's split (1: one workgroup per transform; 0: no schedule), memoised per size and precision: the
// schedule search behind it (spectral_gx.h gx_choose) plans every candidate split, and every plan creation asks.  The process's one memo.
int gx_split_r0(int dtype, int64_t nfft) {
    static std::mutex mu;
    static std::map<int64_t, int> memo;   // (nfft << 1 | double) -> R0
    const int64_t key = (nfft << 1) | (dtype_is_double(dtype) ? 1 : 0);
    {
        std::lock_guard<std::mutex> lk(mu);
        if (auto it = memo.find(key); it != memo.end()) return it->second;
    }
    int R0 = 0;
    if (!gx_choose(dtype, nfft, true, &R0, nullptr)) R0 = 0;
    std::lock_guard<std::mutex> lk(mu);
    memo.emplace(key, R0);
    return R0;
}
bool gx_size_ok(int dtype, int64_t nfft) { return gx_split_r0(dtype, nfft) > 0; }

}  // namespace

namespace mdsp {

// The kernel family (MDSP_ROUTE_*) and engine of a Welch (kind 0: sums of |X|^2) or STFT / spectrogram / periodogram / multitaper (kind 1: columns)
// plan: decided here, once, when the plan is created, from the tunables of that moment -- the plan records it and its exec dispatches on the record.
// The only reader of the knobs that steer the choice (MDSP_GX, MDSP_BIGFFT, MDSP_ENGINE, MDSP_GEN_CT_F64_MAX) apart from the predicates it calls.
//
// round 6: the run-time-schedule kernel (spectral_gx.h) takes every 7-smooth size it plans that has neither a register-resident power-of-two kernel
// nor a compile-time schedule -- in front of the round-2 LDS kernel, the multi-pass engine and the rocFFT pipeline.
// Measured against both (profiles/r06_gx_vs_r5.json: Float32 / Float64 / ComplexF32 / ComplexF64, 1125 .. 65536 points):
//   Welch          : 2 - 7 x either at every size but the powers of two from 32768 (the multi-pass engine's two register stages: a tie)
//   real columns   : 1.1 - 6 x, a tie with rocFFT at R0 >= 5 (12500, 40000); 16384 = 2 x 8192 loses 8 % to the multi-pass engine
//   complex columns: wins from 4097 points while one workgroup holds the transform and up to R0 = 4 (8400, 20000); rocFFT is faster below 4097
//                    (1.4 - 1.7 against 0.9 - 1.3 TB/s) and at R0 >= 5 (40000: 0.75 / 0.91 against 0.67 / 0.59)
// nfft = R0 x S in two kernels (spectral_ctrows.hip), R0 up to 32: from R0 = 6.  Measured (profiles/r06_ctrows.json, TB/s): 98304 = 6 x 16384 0.70 against 0.61
// on the fused column step, 100000 = 8 x 12500 0.66 / 0.49, 131072 0.74 / 0.54; a tie at R0 = 5 (81920: 0.69 / 0.69); the fused step wins below (65536 = 4 x 16384
// 0.74 / 0.81, 32768 0.76 / 1.01).  Beyond eight rows there is no fused step: 150000 .. 500000 points 0.50 - 0.67 against the multi-pass engine's 0.08 - 0.18, 2^19 =
// 32 x 16384 0.73 against 0.52 on the engine's rows form.  MDSP_GX=8: wherever a split exists (A/B), MDSP_GX=-1: never.
int choose_spectral_route(int engine, int dtype, int64_t nfft, int kind, SpecRoute* out) {
    const int m = tunables().gx;
    const bool dbl = dtype_is_double(dtype), cplx = dtype_is_complex(dtype);
    const bool direct = kind == 0 || cplx;   // the last pass is consumed from registers (spectral_gen.h)
    const bool pow2 = (nfft & (nfft - 1)) == 0;
    const bool reg = fused_size_ok(dtype, nfft), gen = !reg && gen_size_ok(dtype, nfft), ct = gen_ct_size(dtype, nfft, direct);
    const bool ctbig = !(m == 3 && dbl) && ctbig_ok(dtype, nfft);            // (MDSP_GX=3: Float64 stays on the run-time schedule, A/B)
    const bool ctbig_cols = !(m == 3 && dbl) && ctbig_cols_ok(dtype, nfft);
    const int cols = kind == 0 ? ctcols_split(dtype, nfft) : 0;
    const int rows = [&] {
        if (kind != 0 || reg || m == 0 || m == -1 || m == 4 || m == 5 || m == 6 || ctbig || (m == 3 && dbl)) return 0;   // (rows above 4096 / 8192 points)
        const int any = ctrows_split(dtype, nfft, 2);
        if (any == 0 || m == 8) return any;
        return (cols == 0 || cols >= (dbl ? 5 : 6)) ? any : 0;   // (Float64, r06s71 / r06s72: 48000 = 5 x 9600 0.60 against 0.51 fused, 57600 0.62 / 0.45; a tie at R0 = 4)
    }();
    const bool gx = [&] {   // a single-workgroup kernel of spectral_gx.h / spectral_ct*.hip
        if (m == 0) return false;
        if (kind == 0 && m != 4 && m != 5 && ctbig_preferred(dtype, nfft)) return true;
        if (kind == 0 && m != 4 && !reg && !ct && ((m != 5 && ctbig) || cols > 0 || rows > 0))
            return true;   // Welch sums on a compile-time schedule (one workgroup, or R0 x S rows): whatever the run-time-schedule kernel plans
        if (kind == 1 && m != 4 && m != 5 && !reg && !ct && ctbig_cols)
            return true;   // columns on a single-workgroup compile-time schedule (spectral_ctbig_cols.hip), 16384 points included
        if (!gx_size_ok(dtype, nfft)) return false;
        if (m >= 2) return true;
        if (pow2 && nfft >= (kind == 0 ? 32768 : 16384) && big::size_ok(dtype, nfft) && cols == 0) return false;   // (Welch, Float32: 4 x / 8 x 8192 on the compile-time rows)
        return !reg && !ct;
    }();
    const bool big = !gx && !reg && !gen && !ct && big::size_ok(dtype, nfft);   // round 5: the multi-pass engine (bigfft.hip) takes what no single-workgroup kernel does
    int eng = engine == MDSP_ENGINE_AUTO ? tunables().engine : engine;
    if (eng == MDSP_ENGINE_AUTO) {
        // AUTO takes the mixed-radix kernel where it measured faster than the rocFFT pipeline (profiles/r02g_mixed.json, 2^27 samples): Welch and
        // real-signal columns up to 4096 points (1.4-3x), complex columns above (1.6x); elsewhere the two are within 20 % and rocFFT is kept.
        // Round 3: the sizes with a compile-time schedule (spectral_gen.h, Float32 / ComplexF32) beat the rocFFT pipeline 2-9x in every mode
        // (profiles/r03d_mixed_ct.json) and are always taken.
        // ... the multi-pass engine where it measured faster than the rocFFT pipeline (profiles/r05_big_vs_rocfft.json, 2^26 samples): powers of two from 16384 on
        // (two-stage register passes: Welch 1.5 - 2.2x, columns 1.1 - 1.4x; the 8192-point Float64 split loses 0.7 - 0.8x), other 7-smooth sizes from
        // 50000 points on for Welch and real-signal columns (1.1 - 1.7x at 50000 / 100000 / 125000 / 200000; complex columns lose 0.7 - 0.9x there, and
        // below 50000 the generic passes' small tiles lose to rocFFT at most sizes: 8400 .. 10000 0.7x, 20000 0.5x, 40000 1.0x)
        // ... and the run-time-schedule kernel everywhere but complex columns, which rocFFT serves faster below 4097 points and from R0 = 5 on --
        // except on a single-workgroup compile-time schedule: 1.6 - 2.9 TB/s against rocFFT's 0.3 - 1.4 (r06s58)
        const auto gx_wins = [&] { return kind == 0 || !cplx || (m != 4 && m != 5 && ctbig_cols) || (nfft > 4096 && gx_split_r0(dtype, nfft) <= 4); };
        const bool big_wins = big && (pow2 ? nfft >= 16384 : (nfft >= 50000 && !(kind == 1 && cplx)));
        const bool fused_wins = (gx && gx_wins()) || big_wins || reg || ct || (gen && ((nfft <= 4096) == (kind == 0 || !cplx)));
        eng = fused_wins ? MDSP_ENGINE_FUSED : MDSP_ENGINE_ROCFFT;
    }
    if (eng == MDSP_ENGINE_FUSED && !(gx || reg || gen || ct || big))
        MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "fused engine supports nfft = 2^a 3^b 5^c 7^d (up to %d, or splitting into 2..4 factors of at most 512); got %lld",
                  dbl ? 4096 : 8192, (long long)nfft);
    if (eng != MDSP_ENGINE_FUSED && eng != MDSP_ENGINE_ROCFFT) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid engine %d", engine);
    SpecRoute r;
    r.engine = eng;
    if (eng == MDSP_ENGINE_ROCFFT) r.route = MDSP_ROUTE_ROCFFT;
    else if (!gx) r.route = big ? MDSP_ROUTE_BIG : reg ? MDSP_ROUTE_POW2 : MDSP_ROUTE_GEN;
    else if (kind == 1) r.route = (m != 4 && m != 5 && ctbig_cols) ? MDSP_ROUTE_CTBIG_COLS : MDSP_ROUTE_GX;
    // R0 x a row size with a COMPILE-TIME schedule (16384 = 2 x 8192, 12500 = 5 x 2500, 20000 = 4 x 5000 ...): the same decomposition on the kernels of
    // spectral_gen.h (spectral_ctcols.hip) -- about half the vector instructions per point of the run-time schedule
    else if (m != 4 && m != 5 && ctbig) r.route = MDSP_ROUTE_CTBIG;   // one workgroup, compile-time schedule (spectral_ctbig.hip): 8400 .. 12500 points
    else if (rows > 0) {
        r.route = MDSP_ROUTE_CTROWS;
        r.r0 = rows;
    } else if (m != 4 && cols > 0) {   // rows of 8193 .. 16384 points first (MDSP_GX=6: without them), then Float64 rows of 4097 .. 9600 points
        const int64_t S = nfft / cols;
        r.r0 = cols;
        if (m != 6 && ctcols_big_row_ok(dtype, S)) r.route = MDSP_ROUTE_CTCOLS_BIG;
        else if (dbl && m != 6 && m != 3 && ctcols64_row_ok(S)) r.route = MDSP_ROUTE_CTCOLS_F64;
        else r.route = MDSP_ROUTE_CTCOLS;
    } else r.route = MDSP_ROUTE_GX;
    *out = r;
    return MDSP_OK;
}

// the lean compile-time schedules (spectral_gen.h ct_pass0_lean) read the window in the working precision: nfft values, ones without a window, zero tail
bool lean_window_needed(int64_t nfft, bool dbl) { return dbl && MDSP_F64_LEAN && nfft >= 4800; }   // (wherever gen_ct_f64_tw2l may set flag 4096)

int check_split(int64_t n, int64_t noverlap, int64_t nfft) {
    if (n < 1) MDSP_FAIL(MDSP_ERR_DOMAIN, "n (%lld) must be positive", (long long)n);
    if (!(0 <= noverlap && noverlap < n))
        MDSP_FAIL(MDSP_ERR_DOMAIN, "noverlap must be between zero and n (noverlap=%lld, n=%lld)", (long long)noverlap, (long long)n);
    if (!(nfft >= n)) MDSP_FAIL(MDSP_ERR_DOMAIN, "nfft must be >= n (nfft=%lld, n=%lld)", (long long)nfft, (long long)n);
    return MDSP_OK;
}

}  // namespace mdsp

// ======================================================================================================
// mdsp_frames (K4 only)
// ======================================================================================================
extern "C" int mdsp_frames(const void* s_dev, int64_t len, int dtype, int64_t n, int64_t noverlap, int64_t nfft, const double* window_host,
                           int64_t first, int64_t count, void* frames_dev, void* stream) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype %d", dtype);
    MDSP_TRY(check_split(n, noverlap, nfft));
    const int64_t K = mdsp_frame_count(len, n, noverlap);
    if (first < 0 || count < 0 || first + count > K) MDSP_FAIL(MDSP_ERR_ARGUMENT, "frame range [%lld,%lld) outside [0,%lld)", (long long)first, (long long)(first + count), (long long)K);
    if (count == 0) return MDSP_OK;
    hipStream_t st = as_stream(stream);
    DevBuf win;
    if (window_host) {
        MDSP_TRY(win.reserve(sizeof(double) * (size_t)n));
        MDSP_HIP(hipMemcpyAsync(win.p, window_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    }
    const int64_t hop = n - noverlap;
    const int gx = (int)std::min<int64_t>(cdiv(nfft, 256), 8);
    for (int64_t c0 = 0; c0 < count; c0 += 32768) {
        const int64_t cnt = std::min<int64_t>(32768, count - c0);
#define FR(TT)                                                                                                                          \
    hipLaunchKernelGGL(frame_window_kernel<TT>, dim3((unsigned)cnt, gx), dim3(256), 0, st, (const TT*)s_dev, (TT*)frames_dev + c0 * nfft, \
                       window_host ? win.as<double>() : nullptr, (int64_t)0, K, hop, (int)n, (int)nfft, first + c0, first + count)
        switch (dtype) {
            case MDSP_F32: FR(float); break;
            case MDSP_F64: FR(double); break;
            case MDSP_C32: FR(cx<float>); break;
            default: FR(cx<double>); break;
        }
#undef FR
        MDSP_LAUNCH_CHECK();
    }
    if (window_host) MDSP_HIP(hipStreamSynchronize(st));  // `win` is freed on return
    return MDSP_OK;
}

namespace mdsp {
int gx_run(int id, const GxArgs& a, unsigned grid_x, unsigned grid_y, int threads, size_t lds_bytes, hipStream_t st) {
    switch (id) {
#define MDSP_GX_CASE(ID) case ID: return gx_run_##ID(a, grid_x, grid_y, threads, lds_bytes, st);
        MDSP_GX_CASE(0) MDSP_GX_CASE(1) MDSP_GX_CASE(2) MDSP_GX_CASE(3) MDSP_GX_CASE(5) MDSP_GX_CASE(6) MDSP_GX_CASE(7) MDSP_GX_CASE(8)
        MDSP_GX_CASE(10) MDSP_GX_CASE(11) MDSP_GX_CASE(12) MDSP_GX_CASE(14) MDSP_GX_CASE(15) MDSP_GX_CASE(16) MDSP_GX_CASE(17) MDSP_GX_CASE(19)
#undef MDSP_GX_CASE
        default: MDSP_FAIL(MDSP_ERR_ASSERTION, "gx kernel id %d", id);
    }
}
}  // namespace mdsp

extern "C" int mdsp_spectral_route_for(int kind, int dtype, int64_t nfft, int engine, int* engine_used, int* route, int* r0) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid dtype %d", dtype);
    if (kind != 0 && kind != 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid kind %d (0: Welch sums, 1: STFT columns)", kind);
    SpecRoute r;
    MDSP_TRY(choose_spectral_route(engine, dtype, nfft, kind, &r));
    if (engine_used) *engine_used = r.engine;
    if (route) *route = r.route;
    if (r0) *r0 = r.r0;
    return MDSP_OK;
}
