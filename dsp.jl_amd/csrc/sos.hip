// filt / filt! for Biquad and SecondOrderSections (Filters/filt.jl:35-92) on the device.  The arithmetic, the geometry and the carry matrices are
// sos_scan.h (shared with the host emulation); here are the thread mapping and the C ABI.
//
// A wavefront per (line, segment), four per workgroup, nothing shared between them.  A line is a real column, or the real or the imaginary parts of a
// complex one (element stride 2): the coefficients are real, so the recurrence never mixes the two.  A tile of 64 x RUN samples is loaded with
// consecutive lanes on consecutive samples and handed to the lanes run by run through LDS (rows of RUN + 1 words: lane l reading run l meets no
// bank twice); the outputs go back the same way.  A tile is read completely before any of it is written and a segment touches only its own samples,
// so y may be x itself.  The filter travels in the kernel arguments, the carry matrices are read from global memory at wave-uniform addresses, the
// state lives in registers.  S == 1 is one launch; S > 1 is three on the caller's stream -- reduce, carries, apply -- every dependence between
// workgroups a kernel boundary: no flags, no atomics, nothing waits, and a result depends on the call's arguments only.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "sos_scan.h"

using namespace mdsp;
using namespace mdsp::sosscan;

namespace {

enum : int { MODE_WHOLE = 0, MODE_REDUCE = 1, MODE_APPLY = 2 };

template <typename W, int KP> struct Args {
    Coef<W, KP> f;
    const W* x;
    W* y;
    int64_t n, colx, coly;      // samples per line; elements of W between columns of x, of y
    int64_t S, seglen, nunits;
    const W* tilemats;          // A^(RUN 2^d), d = 0 .. 5
    W* ws;                      // S > 1: 2 K values per (line, segment)
    W* state;                   // (2, K, ncols) of the working type, or nullptr
    int cs, reverse, mode;
};

// element i of the state of line q inside the caller's (2, K, ncols) array
__device__ __forceinline__ int64_t state_index(int64_t q, int i, int K, int cs) { return ((q / cs) * 2 * K + i) * cs + q % cs; }

template <typename W, int KP> __device__ __forceinline__ void wave_scan(const W* mats, int K, int lane, W* v, W* u) {
#pragma unroll
    for (int d = 0; d < LEVELS; ++d) {
#pragma unroll
        for (int i = 0; i < 2 * KP; ++i)
            if (i < 2 * K) u[i] = __shfl_up(v[i], 1 << d, 64);
        if (lane >= (1 << d)) affine_add<W, KP>(mats + d * 4 * KP * KP, K, u, v);
    }
}

template <typename W, int KP> __global__ __launch_bounds__(256) void sos_kernel(const Args<W, KP> a) {
    __shared__ W lds_all[4][64 * (RUN + 1)];
    const int lane = threadIdx.x & 63, K = a.f.K;
    W* lds = lds_all[threadIdx.x >> 6];
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); unit < a.nunits; unit += nwaves) {   // wave-uniform
        const int64_t q = unit / a.S, s = unit - q * a.S;
        const int64_t j0 = s * a.seglen, j1 = j0 + a.seglen < a.n ? j0 + a.seglen : a.n;
        const W* x = a.x + (q / a.cs) * a.colx + q % a.cs;
        W* y = a.y + (q / a.cs) * a.coly + q % a.cs;
        W z[2 * KP], v[2 * KP], u[2 * KP], xs[RUN];
#pragma unroll
        for (int i = 0; i < 2 * KP; ++i) {
            z[i] = (W)0;
            if (i < 2 * K) {
                if (a.mode == MODE_APPLY) z[i] = a.ws[unit * 2 * K + i];
                else if (a.mode == MODE_WHOLE && a.state) z[i] = a.state[state_index(q, i, K, a.cs)];
            }
        }
        for (int64_t t0 = j0; t0 < j1; t0 += TILE) {
            const int cnt = (int)(j1 - t0 < TILE ? j1 - t0 : TILE);
            __builtin_amdgcn_wave_barrier();   // the reads of the tile before are done (the DS operations of a wavefront execute in order)
#pragma unroll
            for (int t = 0; t < RUN; ++t) {
                const int i = t * 64 + lane;
                if (i < cnt) lds[i + i / RUN] = x[(a.reverse ? a.n - 1 - (t0 + i) : t0 + i) * a.cs];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            int mine = cnt - lane * RUN;
            mine = mine < 0 ? 0 : mine > RUN ? RUN : mine;
#pragma unroll
            for (int t = 0; t < RUN; ++t) xs[t] = t < mine ? lds[lane * (RUN + 1) + t] : (W)0;
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i) v[i] = lane == 0 ? z[i] : (W)0;
            walk_run<W, KP, false>(a.f, xs, mine, v);
            wave_scan<W, KP>(a.tilemats, K, lane, v, u);
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i) {
                u[i] = (W)0;
                if (i < 2 * K) {
                    u[i] = __shfl_up(v[i], 1, 64);
                    if (lane == 0) u[i] = z[i];
                }
            }
            // (the reduce step walks again too: taking a full tile's end state from the scan instead was tried and costs accuracy)
            walk_run<W, KP, true>(a.f, xs, mine, u);   // from its true start state every run is the serial recurrence
            const int last = (cnt - 1) / RUN;
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i)
                if (i < 2 * K) z[i] = __shfl(u[i], last, 64);
            if (a.mode != MODE_REDUCE) {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < RUN; ++t)
                    if (t < mine) lds[lane * (RUN + 1) + t] = xs[t];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int t = 0; t < RUN; ++t) {
                    const int i = t * 64 + lane;
                    if (i < cnt) y[(a.reverse ? a.n - 1 - (t0 + i) : t0 + i) * a.cs] = lds[i + i / RUN];
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i) {
                if (i < 2 * K) {
                    if (a.mode == MODE_REDUCE) a.ws[unit * 2 * K + i] = z[i];
                    else if (a.state && s == a.S - 1) a.state[state_index(q, i, K, a.cs)] = z[i];
                }
            }
        }
    }
}

// step 2: a wavefront per line, 64 records at a time; the records become the states at the segments' first samples
template <typename W, int KP>
__global__ __launch_bounds__(256) void sos_carry_kernel(const W* segmats, W* ws, const W* state, int64_t lines, int64_t S, int K, int cs) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < lines; q += nwaves) {   // wave-uniform
        W r[2 * KP], v[2 * KP], u[2 * KP];
#pragma unroll
        for (int i = 0; i < 2 * KP; ++i) r[i] = i < 2 * K && state ? state[state_index(q, i, K, cs)] : (W)0;
        W* rec = ws + q * S * 2 * K;
        for (int64_t s0 = 0; s0 < S; s0 += 64) {
            const int64_t s = s0 + lane;
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i) v[i] = s < S && i < 2 * K ? rec[s * 2 * K + i] : (W)0;
            if (lane == 0) affine_add<W, KP>(segmats, K, r, v);
            wave_scan<W, KP>(segmats, K, lane, v, u);
#pragma unroll
            for (int i = 0; i < 2 * KP; ++i) {
                if (i < 2 * K) {
                    W c = __shfl_up(v[i], 1, 64);
                    if (lane == 0) c = r[i];
                    if (s < S) rec[s * 2 * K + i] = c;
                    r[i] = __shfl(v[i], 63, 64);
                }
            }
        }
    }
}

constexpr int64_t MAX_GRID = 1 << 20;   // workgroups per launch; the kernels stride over what is left

struct Filter {
    int K = 1, KP = 1, has_gain = 0;
    double c[5 * MAXK];
    double g = 1.0;
};

// the checks every entry shares; *empty: a size is 0, nothing to do
int check_args(const double* coef, int64_t K, double gain, int has_gain, int dtype, int64_t n, int64_t ncols, int64_t segments, Filter* f, bool* empty) {
    if (n < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: negative size (%lld, %lld)", (long long)n, (long long)ncols);
    if (K < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: at least one section is needed (got %lld)", (long long)K);
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: bad dtype %d", dtype);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    if (!coef) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: coef is NULL");
    const bool dbl = dtype_is_double(dtype);
    for (int64_t i = 0; i < 5 * K; ++i)
        if (!std::isfinite(dbl ? coef[i] : (double)(float)coef[i])) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: coefficient %lld of section %lld is not finite", (long long)(i % 5), (long long)(i / 5));
    if (has_gain && !std::isfinite(dbl ? gain : (double)(float)gain)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: the gain is not finite");
    *empty = n == 0 || ncols == 0;
    int64_t total = 0;
    if (!*empty && (__builtin_mul_overflow(n, ncols, &total) || total > (INT64_MAX >> 6))) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: array too large");
    if (K > MAXK) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "sos: cascades of more than %d sections are not accelerated (got %lld): use DSP.jl's CPU path", MAXK, (long long)K);
    f->K = (int)K;
    f->KP = padded_sections(K);
    f->has_gain = has_gain ? 1 : 0;
    f->g = has_gain ? (dbl ? gain : (double)(float)gain) : 1.0;
    for (int64_t k = 0; k < K; ++k) {
        for (int i = 0; i < 5; ++i) f->c[5 * k + i] = dbl ? coef[5 * k + i] : (double)(float)coef[5 * k + i];   // as the kernels use them
        const double a1 = f->c[5 * k + 3], a2 = f->c[5 * k + 4];
        // the poles are the roots of z^2 + a1 z + a2; beyond the unit circle the carry matrices grow without bound.  The margin covers the
        // rounding of this formula only (a double pole at 1 runs).
        const double disc = a1 * a1 - 4.0 * a2;
        const double r = disc < 0.0 ? std::sqrt(a2) : 0.5 * (std::fabs(a1) + std::sqrt(disc));
        if (r > 1.0 + 1e-12)
            MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "sos: section %lld has a pole of modulus %.17g > 1 (unstable): use DSP.jl's CPU path", (long long)k, r);
    }
    return MDSP_OK;
}

Geom geometry(const Filter& f, int dtype, int64_t n, int64_t ncols, int64_t segments) {
    return make_geometry(f.K, dtype_is_complex(dtype), dtype_is_double(dtype), n, ncols, segments);
}

// the two ladders of matrices in W: [0] for the tiles, [LEVELS ..] for the segments (S > 1 only)
template <typename W> int make_matrices(const Filter& f, const Geom& g, std::vector<unsigned char>* out) {
    long double c[5 * MAXK];
    for (int i = 0; i < 5 * f.K; ++i) c[i] = (long double)f.c[i];
    const LMat A = state_matrix(c, f.K);
    const size_t per = (size_t)LEVELS * 4 * f.KP * f.KP;
    out->assign((g.S > 1 ? 2 : 1) * per * sizeof(W), 0);
    W* m = reinterpret_cast<W*>(out->data());
    if (!power_ladder<W>(A, RUN, f.KP, m) || (g.S > 1 && !power_ladder<W>(A, g.seglen, f.KP, m + per)))
        MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "sos: the carry matrices of this cascade overflow the working type: use DSP.jl's CPU path");
    return MDSP_OK;
}

template <typename W, int KP> Coef<W, KP> make_coef(const Filter& f) {
    Coef<W, KP> c{};
    for (int i = 0; i < 5 * KP; ++i) c.c[i] = i < 5 * f.K ? (W)f.c[i] : (W)0;
    c.g = (W)f.g;
    c.K = f.K;
    c.has_gain = f.has_gain;
    return c;
}

template <typename W, int KP>
void emulate(const Filter& f, const Geom& g, const W* mats, const W* x, int64_t ldx, W* y, int64_t ldy, W* state, int reverse) {
    const Coef<W, KP> cf = make_coef<W, KP>(f);
    const int K = f.K;
    const W* segmats = g.S > 1 ? mats + (size_t)LEVELS * 4 * KP * KP : mats;
    std::vector<W> ws((size_t)(g.S > 1 ? g.lines * g.S * 2 * K : 0));
    W z[2 * KP];
    auto sidx = [&](int64_t q, int i) { return ((q / g.cs) * 2 * K + i) * g.cs + q % g.cs; };
    for (int pass = 0; pass < (g.S > 1 ? 3 : 1); ++pass) {
        for (int64_t q = 0; q < g.lines; ++q) {
            const W* xl = x + (q / g.cs) * ldx * g.cs + q % g.cs;
            W* yl = y + (q / g.cs) * ldy * g.cs + q % g.cs;
            if (g.S > 1 && pass == 1) {
                for (int i = 0; i < 2 * K; ++i) z[i] = state ? state[sidx(q, i)] : (W)0;
                carries_host<W, KP>(segmats, K, &ws[(size_t)(q * g.S * 2 * K)], g.S, z);
                continue;
            }
            for (int64_t s = 0; s < g.S; ++s) {
                W* rec = g.S > 1 ? &ws[(size_t)((q * g.S + s) * 2 * K)] : nullptr;
                for (int i = 0; i < 2 * K; ++i) z[i] = g.S > 1 ? (pass == 2 ? rec[i] : (W)0) : (state ? state[sidx(q, i)] : (W)0);
                unit_host<W, KP>(cf, mats, xl, g.S > 1 && pass == 0 ? nullptr : yl, g.cs, g.cs, g.n, reverse, s * g.seglen, std::min(g.n, (s + 1) * g.seglen), z);
                for (int i = 0; i < 2 * K; ++i) {
                    if (g.S > 1 && pass == 0) rec[i] = z[i];
                    else if (state && s == g.S - 1) state[sidx(q, i)] = z[i];
                }
            }
        }
    }
}

}  // namespace

struct mdsp_sos_plan_s {
    Filter f;
    Geom g;
    int dtype = MDSP_F32;
    bool empty = false;
    std::vector<unsigned char> mats;   // host copy of the carry matrices in W
    std::mutex mu;
    bool on_device = false;            // the plan touches the device at its first exec, not before
    DevBuf dmats, ws;
};

namespace {

int ensure_device(mdsp_sos_plan pl) {
    std::lock_guard<std::mutex> lock(pl->mu);
    if (pl->on_device) return MDSP_OK;
    MDSP_TRY(pl->dmats.reserve(pl->mats.size()));
    MDSP_HIP(hipMemcpy(pl->dmats.p, pl->mats.data(), pl->mats.size(), hipMemcpyHostToDevice));
    if (pl->g.workspace > 0) MDSP_TRY(pl->ws.reserve((size_t)pl->g.workspace));
    pl->on_device = true;
    return MDSP_OK;
}

template <typename W, int KP> int sos_exec(mdsp_sos_plan pl, const void* x_dev, int64_t ldx, void* y_dev, int64_t ldy, void* state_dev, int reverse, hipStream_t st) {
    const Geom& g = pl->g;
    Args<W, KP> a{};
    a.f = make_coef<W, KP>(pl->f);
    a.x = static_cast<const W*>(x_dev);
    a.y = static_cast<W*>(y_dev);
    a.n = g.n;
    a.colx = ldx * g.cs;
    a.coly = ldy * g.cs;
    a.S = g.S;
    a.seglen = g.seglen;
    a.nunits = g.lines * g.S;
    a.tilemats = pl->dmats.as<W>();
    a.ws = pl->ws.as<W>();
    a.state = static_cast<W*>(state_dev);
    a.cs = g.cs;
    a.reverse = reverse ? 1 : 0;
    const dim3 grid((unsigned)std::min(cdiv(a.nunits, 4), MAX_GRID)), block(256);
    if (g.S == 1) {
        a.mode = MODE_WHOLE;
        hipLaunchKernelGGL((sos_kernel<W, KP>), grid, block, 0, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    a.mode = MODE_REDUCE;
    hipLaunchKernelGGL((sos_kernel<W, KP>), grid, block, 0, st, a);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((sos_carry_kernel<W, KP>), dim3((unsigned)std::min(cdiv(g.lines, 4), MAX_GRID)), block, 0, st,
                       pl->dmats.as<W>() + (size_t)LEVELS * 4 * KP * KP, a.ws, static_cast<const W*>(state_dev), g.lines, g.S, pl->f.K, g.cs);
    MDSP_LAUNCH_CHECK();
    a.mode = MODE_APPLY;
    hipLaunchKernelGGL((sos_kernel<W, KP>), grid, block, 0, st, a);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

// FN<W, KP>(args...) for the working type's real type and the compiled section count
#define SOS_DISPATCH(dbl, KP, CALL)                          \
    switch ((KP) * 2 + ((dbl) ? 1 : 0)) {                    \
        case 2: { using W = float; constexpr int P = 1; CALL; } break;    \
        case 3: { using W = double; constexpr int P = 1; CALL; } break;   \
        case 4: { using W = float; constexpr int P = 2; CALL; } break;    \
        case 5: { using W = double; constexpr int P = 2; CALL; } break;   \
        case 8: { using W = float; constexpr int P = 4; CALL; } break;    \
        case 9: { using W = double; constexpr int P = 4; CALL; } break;   \
        case 16: { using W = float; constexpr int P = 8; CALL; } break;   \
        case 17: { using W = double; constexpr int P = 8; CALL; } break;  \
        case 32: { using W = float; constexpr int P = 16; CALL; } break;  \
        default: { using W = double; constexpr int P = 16; CALL; } break; \
    }

int check_exec(const Geom& g, int dtype, const void* x, int64_t ldx, const void* y, int64_t ldy, bool host) {
    if (!x || !y) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: NULL buffer");
    if (ldx < g.n || ldy < g.n) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: leading dimensions (%lld, %lld) below the length %lld", (long long)ldx, (long long)ldy, (long long)g.n);
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y), es = dtype_size(dtype);
    const uintptr_t xb = (uintptr_t)((g.ncols - 1) * ldx + g.n) * es, yb = (uintptr_t)((g.ncols - 1) * ldy + g.n) * es;
    if (!(a == b && ldx == ldy) && a < b + yb && b < a + xb) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: y must be x itself (with the same leading dimension) or not overlap it");
    if (!host && (a % (uintptr_t)g.real_size || b % (uintptr_t)g.real_size)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: arrays must be aligned to their element size");
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_sos_geometry_for(int64_t nsections, int dtype, int64_t n, int64_t ncols, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile,
                          int64_t* run, int64_t* workspace_bytes) {
    if (n < 0 || ncols < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: negative size (%lld, %lld)", (long long)n, (long long)ncols);
    if (nsections < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: at least one section is needed (got %lld)", (long long)nsections);
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: bad dtype %d", dtype);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "sos: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    if (nsections > MAXK) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "sos: cascades of more than %d sections are not accelerated (got %lld)", MAXK, (long long)nsections);
    const Geom g = make_geometry(nsections, dtype_is_complex(dtype), dtype_is_double(dtype), n, ncols, segments);
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (tile) *tile = TILE;
    if (run) *run = RUN;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_sos_plan_create(mdsp_sos_plan* plan, const double* coef, int64_t nsections, double gain, int has_gain, int dtype, int64_t n, int64_t ncols,
                         int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    Filter f;
    bool empty = false;
    MDSP_TRY(check_args(coef, nsections, gain, has_gain, dtype, n, ncols, segments, &f, &empty));
    auto pl = new mdsp_sos_plan_s();
    pl->f = f;
    pl->g = geometry(f, dtype, n, ncols, segments);
    pl->dtype = dtype;
    pl->empty = empty;
    const int st = dtype_is_double(dtype) ? make_matrices<double>(f, pl->g, &pl->mats) : make_matrices<float>(f, pl->g, &pl->mats);
    if (st != MDSP_OK) {
        delete pl;
        return st;
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_sos_plan_destroy(mdsp_sos_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_sos_plan_info(mdsp_sos_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* run, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (tile) *tile = TILE;
    if (run) *run = RUN;
    if (workspace_bytes) *workspace_bytes = plan->g.workspace;
    return MDSP_OK;
}

int mdsp_sos_exec(mdsp_sos_plan plan, const void* x_dev, int64_t ldx, void* y_dev, int64_t ldy, void* state_dev, int reverse, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (plan->empty) return MDSP_OK;
    MDSP_TRY(check_exec(plan->g, plan->dtype, x_dev, ldx, y_dev, ldy, false));
    MDSP_TRY(ensure_device(plan));
    hipStream_t st = as_stream(stream);
    int status = MDSP_OK;
    SOS_DISPATCH(dtype_is_double(plan->dtype), plan->f.KP, (status = sos_exec<W, P>(plan, x_dev, ldx, y_dev, ldy, state_dev, reverse, st)));
    return status;
}

int mdsp_sos_emulate_host(const void* x_host, int64_t ldx, void* y_host, int64_t ldy, void* state_host, const double* coef, int64_t nsections, double gain,
                          int has_gain, int dtype, int64_t n, int64_t ncols, int64_t segments, int reverse) {
    Filter f;
    bool empty = false;
    MDSP_TRY(check_args(coef, nsections, gain, has_gain, dtype, n, ncols, segments, &f, &empty));
    if (empty) return MDSP_OK;
    const Geom g = geometry(f, dtype, n, ncols, segments);
    MDSP_TRY(check_exec(g, dtype, x_host, ldx, y_host, ldy, true));
    std::vector<unsigned char> mats;
    MDSP_TRY(dtype_is_double(dtype) ? make_matrices<double>(f, g, &mats) : make_matrices<float>(f, g, &mats));
    SOS_DISPATCH(dtype_is_double(dtype), f.KP,
                 (emulate<W, P>(f, g, reinterpret_cast<const W*>(mats.data()), static_cast<const W*>(x_host), ldx, static_cast<W*>(y_host), ldy,
                                static_cast<W*>(state_host), reverse)));
    return MDSP_OK;
}

}  // extern "C"
