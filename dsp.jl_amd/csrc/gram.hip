// The Hankel Gram matrix behind esprit (src/estimation.jl:69-71) on the device.  The decomposition, the arithmetic, the geometry, the order of every
// addition and the host emulation are gram_op.h; here are the thread mapping of the body launch, the assembly launch and the C ABI.
//
// Body: a workgroup of 4 wavefronts per (segment, block of LAG_BLOCK lags).  Per tile the workgroup stages the samples [t0 + D0, t0 + D0 + cnt + nl - 1)
// -- the tile shifted by the block's first lag D0, plus the halo of its nl lags -- into LDS in the element type; every index is below n because
// k <= L - 1 and d <= M - 1 give k + d <= n - 1.  A lane keeps its E samples x[k] (k = t0 + 64 e + l) in registers as Float64 and reads x[k + d] from
// LDS: consecutive lanes read consecutive elements.  A wavefront walks the lag groups g, g + 4, .. of the block over the staged tile: G accumulators
// per lane, a fold by lane exchanges, and lane 0 adds the tile's sums to the running sums of its lags in LDS -- a lag belongs to one wavefront, so the
// only barriers are the two around the staging.  At the segment's end the running sums are stored: one partial per (segment, lag).
// Assembly: one lane per diagonal (gram_op.h: assemble_diagonal).
#include <algorithm>
#include <mutex>

#include "common.h"
#include "gram_op.h"

using namespace mdsp;
using namespace mdsp::gram;

namespace {

template <typename F> struct BodyArgs {
    int64_t M, L, seglen;
    const F* x;
    double* part;
};

template <typename F> struct AsmArgs {
    int64_t M, L, S, ldr;
    const F* x;
    const double* part;
    double* r;
};

template <bool CP> __device__ __forceinline__ Acc wave_fold(Acc a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.re = add_rn(a.re, __shfl_down(a.re, off, 64));
        if constexpr (CP) a.im = add_rn(a.im, __shfl_down(a.im, off, 64));
    }
    return a;
}

template <typename F> __global__ __launch_bounds__(64 * WAVES) void gram_body_kernel(const BodyArgs<F> a) {
    constexpr bool CP = Elem<F>::CPLX;
    constexpr int NC = CP ? 2 : 1;
    constexpr int NT = 64 * WAVES;
    __shared__ F tile[TILE + LAG_BLOCK - 1];
    __shared__ double run[LAG_BLOCK * NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x, D0 = (int64_t)blockIdx.y * LAG_BLOCK;
    const int nl = (int)(a.M - D0 < LAG_BLOCK ? a.M - D0 : LAG_BLOCK);
    const int ngroups = (nl + G - 1) / G;
    int64_t k0, k1;
    segment_range(a.M, a.L, a.seglen, s, &k0, &k1);
    for (int i = tid; i < nl * NC; i += NT) run[i] = 0.0;
    for (int64_t t0 = k0; t0 < k1; t0 += TILE) {
        __syncthreads();   // the tile before is read out (first tile: the running sums are zeroed)
        const int cnt = (int)(k1 - t0 < TILE ? k1 - t0 : TILE);
        const int need = cnt + nl - 1;
        const F* src = a.x + t0 + D0;
        for (int i = tid; i < need; i += NT) tile[i] = src[i];
        double cre[E], cim[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = 64 * e + lane;
            F c{};
            if (i < cnt) c = a.x[t0 + i];
            cre[e] = re_of(c);
            cim[e] = im_of(c);
        }
        __syncthreads();
        for (int g = wave; g < ngroups; g += WAVES) {   // wave-uniform
            const int base = g * G;
            Acc acc[G];
#pragma unroll
            for (int i = 0; i < G; ++i) acc[i] = Acc{0.0, 0.0};
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int at = 64 * e + lane;
                if (at < cnt) {
#pragma unroll
                    for (int i = 0; i < G; ++i) {
                        if (base + i < nl) {   // wave-uniform
                            const F v = tile[at + base + i];
                            add_term<CP>(re_of(v), im_of(v), cre[e], cim[e], acc[i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const Acc t = wave_fold<CP>(acc[i]);
                if (lane == 0 && base + i < nl) {
                    double* q = run + (base + i) * NC;
                    q[0] = add_rn(q[0], t.re);
                    if constexpr (CP) q[1] = add_rn(q[1], t.im);
                }
            }
        }
    }
    __syncthreads();
    double* out = a.part + (s * a.M + D0) * NC;
    for (int i = tid; i < nl * NC; i += NT) out[i] = run[i];
}

template <typename F> __global__ __launch_bounds__(64) void gram_assemble_kernel(const AsmArgs<F> a) {
    const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (d < a.M) assemble_diagonal<F>(a.x, a.M, a.L, a.S, a.part, d, a.r, a.ldr);
}

constexpr int64_t MAX_M = 1 << 20;

int gram_check(int dtype, int64_t n, int64_t M, int64_t segments) {
    if (!dtype_valid(dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: bad dtype %d", dtype);
    if (n < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: n must be >= 0, got %lld", (long long)n);
    if (n > (INT64_MAX >> 6)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: signal too long");
    if (M < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: M must be >= 1, got %lld", (long long)M);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    if (M > MAX_M || 2 * M - 1 > n)
        MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "hankel_gram: 2 M - 1 <= n and M <= %lld are needed (M = %lld, n = %lld)", (long long)MAX_M, (long long)M, (long long)n);
    return MDSP_OK;
}

bool is_complex(int dtype) { return dtype == MDSP_C32 || dtype == MDSP_C64; }

template <typename F> int gram_launch(const Geom& g, const void* x_dev, void* ws, void* r_dev, int64_t ldr, hipStream_t st) {
    const F* x = static_cast<const F*>(x_dev);
    double* part = static_cast<double*>(ws);
    BodyArgs<F> ba{g.M, g.L, g.seglen, x, part};
    hipLaunchKernelGGL((gram_body_kernel<F>), dim3((unsigned)g.S, (unsigned)cdiv(g.M, LAG_BLOCK)), dim3(64 * WAVES), 0, st, ba);
    MDSP_LAUNCH_CHECK();
    AsmArgs<F> aa{g.M, g.L, g.S, ldr, x, part, static_cast<double*>(r_dev)};
    hipLaunchKernelGGL((gram_assemble_kernel<F>), dim3((unsigned)cdiv(g.M, 64)), dim3(64), 0, st, aa);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

struct mdsp_hankel_gram_plan_s {
    Geom g;
    int dtype = MDSP_F32;
    std::mutex mu;
    DevBuf ws;   // the plan touches the device at its first exec, not before
};

extern "C" {

int mdsp_hankel_gram_geometry_for(int dtype, int64_t n, int64_t M, int64_t segments, int64_t* nsegments, int64_t* seglen, int64_t* tile,
                                  int64_t* lag_group, int64_t* workspace_bytes) {
    MDSP_TRY(gram_check(dtype, n, M, segments));
    const Geom g = make_geometry(is_complex(dtype), n, M, segments);
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (tile) *tile = TILE;
    if (lag_group) *lag_group = G;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_hankel_gram_plan_create(mdsp_hankel_gram_plan* plan, int dtype, int64_t n, int64_t M, int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    MDSP_TRY(gram_check(dtype, n, M, segments));
    auto pl = new mdsp_hankel_gram_plan_s();
    pl->g = make_geometry(is_complex(dtype), n, M, segments);
    pl->dtype = dtype;
    *plan = pl;
    return MDSP_OK;
}

int mdsp_hankel_gram_plan_destroy(mdsp_hankel_gram_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_hankel_gram_plan_info(mdsp_hankel_gram_plan plan, int64_t* nsegments, int64_t* seglen, int64_t* tile, int64_t* lag_group,
                               int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (tile) *tile = TILE;
    if (lag_group) *lag_group = G;
    if (workspace_bytes) *workspace_bytes = plan->g.workspace;
    return MDSP_OK;
}

int mdsp_hankel_gram_exec(mdsp_hankel_gram_plan plan, const void* x_dev, void* r_dev, int64_t ldr, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (ldr < plan->g.M) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: ldr = %lld is below M = %lld", (long long)ldr, (long long)plan->g.M);
    if (!x_dev || !r_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: NULL buffer");
    if (reinterpret_cast<uintptr_t>(x_dev) % dtype_size(plan->dtype) || reinterpret_cast<uintptr_t>(r_dev) % 8)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: the signal must be aligned to its element size and R to 8 bytes");
    {
        std::lock_guard<std::mutex> lock(plan->mu);
        MDSP_TRY(plan->ws.reserve((size_t)plan->g.workspace));
    }
    hipStream_t st = as_stream(stream);
    switch (plan->dtype) {
        case MDSP_F32: return gram_launch<float>(plan->g, x_dev, plan->ws.p, r_dev, ldr, st);
        case MDSP_F64: return gram_launch<double>(plan->g, x_dev, plan->ws.p, r_dev, ldr, st);
        case MDSP_C32: return gram_launch<c32>(plan->g, x_dev, plan->ws.p, r_dev, ldr, st);
        default: return gram_launch<c64>(plan->g, x_dev, plan->ws.p, r_dev, ldr, st);
    }
}

int mdsp_hankel_gram_emulate_host(const void* x_host, int dtype, int64_t n, int64_t M, int64_t segments, void* r_host, int64_t ldr) {
    MDSP_TRY(gram_check(dtype, n, M, segments));
    if (ldr < M) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: ldr = %lld is below M = %lld", (long long)ldr, (long long)M);
    if (!x_host || !r_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "hankel_gram: NULL buffer");
    const Geom g = make_geometry(is_complex(dtype), n, M, segments);
    double* r = static_cast<double*>(r_host);
    switch (dtype) {
        case MDSP_F32: emulate<float>(g, static_cast<const float*>(x_host), r, ldr); break;
        case MDSP_F64: emulate<double>(g, static_cast<const double*>(x_host), r, ldr); break;
        case MDSP_C32: emulate<c32>(g, static_cast<const c32*>(x_host), r, ldr); break;
        default: emulate<c64>(g, static_cast<const c64*>(x_host), r, ldr); break;
    }
    return MDSP_OK;
}

}  // extern "C"
