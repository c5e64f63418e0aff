// unwrap / unwrap! along one dimension (src/unwrap.jl:17-34, the `dims::Integer` form) on the device.  The operator, the geometry and the
// per-segment walk are unwrap_scan.h (shared with the host emulation); here are the two thread mappings and the C ABI.
//
// The array is (inner, len, outer), element (i, j, o) at i + inner (j + len o), the scan along j.
//   contiguous route (inner == 1): a wavefront per (line, segment), four per workgroup, nothing shared between them.  A tile is 64 lanes x 16
//       bytes; the tiles sit on 16-byte boundaries of the INPUT address whatever the alignment of the array (the ragged first and last vectors
//       are loaded element by element, nothing outside [j0, j1) is touched), the in-wave scan is __shfl_up, the carry from tile to tile and
//       the left neighbour of a tile's first sample stay in registers.
//   strided route (inner > 1): a lane per (i, o, segment) walking j with K in a register; neighbouring lanes hold neighbouring i, so every
//       access of a wavefront is one contiguous run.
// S == 1 is one launch (8 bytes per Float32 sample).  S > 1 is three launches on the caller's stream -- reduce, carries, apply -- and 12 bytes
// per sample: every dependence between workgroups is a kernel boundary; there are no flags, tickets or atomics, so nothing ever waits for
// another workgroup and results are bit-identical exec after exec.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "unwrap_scan.h"

using namespace mdsp;
using namespace mdsp::unwrapscan;

namespace {

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

__device__ __forceinline__ Acc shfl_up_acc(Acc a, int off) {
    return Acc{(uint64_t)__shfl_up((unsigned long long)a.K, off, 64), __shfl_up(a.st, off, 64)};
}
__device__ __forceinline__ Acc shfl_acc(Acc a, int src) {
    return Acc{(uint64_t)__shfl((unsigned long long)a.K, src, 64), __shfl(a.st, src, 64)};
}
// inclusive scan over the 64 lanes; every lane of the wavefront must be here
__device__ __forceinline__ Acc wave_scan(Acc a, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Acc o = shfl_up_acc(a, off);
        if (lane >= off) a = combine(o, a);
    }
    return a;
}

// ---------------------------------------------------------------- contiguous route.  MODE as walk_segment: 0 one pass, 1 reduce, 2 apply.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void unwrap_contiguous_kernel(const T* in, T* out, int64_t len, int64_t S, int64_t seglen, int64_t nunits, T range,
                                                                Rec* rec) {
    using VT = typename Vec16<T>::type;
    constexpr int V = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < nunits; u += nwaves) {   // wave-uniform
        const int64_t line = u / S, s = u - line * S;
        const int64_t j0 = s * seglen, j1 = j0 + seglen < len ? j0 + seglen : len;
        const T* m = in + line * len;
        T* y = out + line * len;
        const int64_t a = (int64_t)((reinterpret_cast<uintptr_t>(m + j0) / sizeof(T)) % V);   // samples between the 16-byte boundary below m + j0 and m + j0
        const bool yvec = (reinterpret_cast<uintptr_t>(y) + (uintptr_t)((j0 - a) * (int64_t)sizeof(T))) % 16 == 0;
        Acc run{0, ST_FIN}, bnd{0, ST_FIN};
        if (MODE == 2) run = Acc{rec[u].K, rec[u].st};
        T last = (T)0;   // the last sample of the tile before, as it was read: in place, memory may hold its result by now
        for (int64_t p0 = j0 - a; p0 < j1; p0 += 64 * V) {
            const int64_t p = p0 + (int64_t)lane * V;
            const bool full = p >= j0 && p + V <= j1;
            T v[V];
            if (full) {
                const VT w = *reinterpret_cast<const VT*>(m + p);
                __builtin_memcpy(v, &w, 16);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) v[k] = (p + k >= j0 && p + k < j1) ? m[p + k] : (T)0;
            }
            T left = __shfl_up(v[V - 1], 1, 64);
            if (lane == 0) left = last;
            Acc ev[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int64_t e = p + k;
                if (e < j0 || e >= j1) ev[k] = Acc{0, ST_FIN};
                else if (e == j0) {
                    // the segment's first sample.  MODE 2: the carry already stands AT it.  MODE 1 reads the last sample of the segment before
                    // (nothing has been written yet: step 3 comes after a kernel boundary).  Sample 0 of a line has no left neighbour.
                    if (MODE == 2) ev[k] = Acc{0, ST_FIN};
                    else if (j0 == 0) ev[k] = bnd = start_event(v[k]);
                    else ev[k] = bnd = step_event(m[j0 - 1], v[k], range);
                } else ev[k] = step_event(k ? v[k - 1] : left, v[k], range);
                if (k) ev[k] = combine(ev[k - 1], ev[k]);
            }
            const Acc incl = wave_scan(ev[V - 1], lane);
            Acc base = shfl_up_acc(incl, 1);
            if (lane == 0) base = Acc{0, ST_FIN};
            base = combine(run, base);
            if (MODE != 1) {
                T r[V];
#pragma unroll
                for (int k = 0; k < V; ++k) r[k] = finish(v[k], combine(base, ev[k]), range);
                if (full && yvec) {
                    VT w;
                    __builtin_memcpy(&w, r, 16);
                    *reinterpret_cast<VT*>(y + p) = w;
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k)
                        if (p + k >= j0 && p + k < j1) y[p + k] = r[k];
                }
            }
            run = combine(run, shfl_acc(incl, 63));
            last = __shfl(v[V - 1], 63, 64);
        }
        if (MODE == 1 && lane == 0) rec[u] = Rec{run.K, bnd.K, run.st, bnd.st};   // sample j0 is in lane 0 of the first tile (a < V)
    }
}

// ---------------------------------------------------------------- strided route
template <typename T, int MODE>
__global__ __launch_bounds__(256) void unwrap_strided_kernel(const T* in, T* out, int64_t inner, int64_t len, int64_t outer, int64_t S, int64_t seglen,
                                                             int64_t nthreads, T range, Rec* rec) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nthreads; g += step) {
        const int64_t i = g % inner, r = g / inner, o = r % outer, s = r / outer;
        const int64_t j0 = s * seglen, j1 = j0 + seglen < len ? j0 + seglen : len;
        const int64_t base = i + inner * len * o;
        walk_segment<MODE, T>(in + base, out + base, inner, j0, j1, range, rec + ((i + inner * o) * S + s));
    }
}

// ---------------------------------------------------------------- step 2: a wavefront per line, 64 records at a time
__global__ __launch_bounds__(256) void unwrap_carry_kernel(Rec* rec, int64_t lines, int64_t S) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); line < lines; line += nwaves) {   // wave-uniform
        Rec* r = rec + line * S;
        Acc run{0, ST_FIN};
        for (int64_t s0 = 0; s0 < S; s0 += 64) {
            const int64_t s = s0 + lane;
            Acc tot{0, ST_FIN}, b{0, ST_FIN};
            if (s < S) {
                tot = Acc{r[s].K, r[s].st};
                b = Acc{r[s].bK, r[s].bst};
            }
            const Acc incl = wave_scan(tot, lane);
            Acc ex = shfl_up_acc(incl, 1);
            if (lane == 0) ex = Acc{0, ST_FIN};
            const Acc carry = combine(combine(run, ex), b);
            if (s < S) {
                r[s].K = carry.K;
                r[s].st = carry.st;
            }
            run = combine(run, shfl_acc(incl, 63));
        }
    }
}

constexpr int64_t MAX_GRID = 1 << 20;   // workgroups per launch; the kernels stride over what is left

bool valid_range(double range, int dtype) {
    if (!std::isfinite(range) || range == 0.0) return false;
    if (dtype == MDSP_F32) {
        const float r = (float)range;
        return std::isfinite(r) && r != 0.0f;
    }
    return true;
}

// the checks every entry shares; *empty: a size is 0, nothing to do
int check_shape(int64_t inner, int64_t len, int64_t outer, int dtype, int64_t segments, bool* empty) {
    if (inner < 0 || len < 0 || outer < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: negative size (%lld, %lld, %lld)", (long long)inner, (long long)len, (long long)outer);
    if (dtype != MDSP_F32 && dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap takes Float32 or Float64 (dtype %d)", dtype);
    if (segments < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: segments must be >= 0 (0 = auto), got %lld", (long long)segments);
    *empty = inner == 0 || len == 0 || outer == 0;
    int64_t n = 0;
    if (!*empty && (__builtin_mul_overflow(inner, len, &n) || __builtin_mul_overflow(n, outer, &n) || n > (INT64_MAX >> 5)))
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: array too large");
    return MDSP_OK;
}

template <typename T> void emulate(const T* in, T* out, const Geom& g, T range) {
    std::vector<Rec> rec((size_t)(g.S > 1 ? g.lines * g.S : 1));
    auto each = [&](auto&& fn) {
        for (int64_t o = 0; o < g.outer; ++o)
            for (int64_t i = 0; i < g.inner; ++i)
                for (int64_t s = 0; s < g.S; ++s) fn(i + g.inner * g.len * o, (i + g.inner * o) * g.S + s, s * g.seglen, std::min(g.len, (s + 1) * g.seglen));
    };
    if (g.S == 1) {
        each([&](int64_t base, int64_t r, int64_t j0, int64_t j1) { walk_segment<0, T>(in + base, out + base, g.inner, j0, j1, range, &rec[0]); });
        return;
    }
    each([&](int64_t base, int64_t r, int64_t j0, int64_t j1) { walk_segment<1, T>(in + base, out + base, g.inner, j0, j1, range, &rec[r]); });
    for (int64_t line = 0; line < g.lines; ++line) scan_carries(&rec[line * g.S], g.S);
    each([&](int64_t base, int64_t r, int64_t j0, int64_t j1) { walk_segment<2, T>(in + base, out + base, g.inner, j0, j1, range, &rec[r]); });
}

}  // namespace

struct mdsp_unwrap_plan_s {
    Geom g;
    int dtype = MDSP_F32;
    double range = 0.0;
    bool empty = false;
    DevBuf ws;   // S > 1: lines x S records
};

namespace {

template <typename T> int unwrap_exec(mdsp_unwrap_plan pl, const void* in_dev, void* out_dev, hipStream_t st) {
    const Geom& g = pl->g;
    const T* in = static_cast<const T*>(in_dev);
    T* out = static_cast<T*>(out_dev);
    const T range = (T)pl->range;
    Rec* rec = pl->ws.as<Rec>();
    const int64_t units = g.lines * g.S;
    const unsigned carry_grid = (unsigned)std::min(cdiv(g.lines, 4), MAX_GRID);
    if (g.route == ROUTE_CONTIGUOUS) {
        const dim3 grid((unsigned)std::min(cdiv(units, 4), MAX_GRID)), block(256);
        if (g.S == 1) {
            hipLaunchKernelGGL((unwrap_contiguous_kernel<T, 0>), grid, block, 0, st, in, out, g.len, g.S, g.seglen, units, range, rec);
            MDSP_LAUNCH_CHECK();
            return MDSP_OK;
        }
        hipLaunchKernelGGL((unwrap_contiguous_kernel<T, 1>), grid, block, 0, st, in, out, g.len, g.S, g.seglen, units, range, rec);
        MDSP_LAUNCH_CHECK();
        hipLaunchKernelGGL(unwrap_carry_kernel, dim3(carry_grid), block, 0, st, rec, g.lines, g.S);
        MDSP_LAUNCH_CHECK();
        hipLaunchKernelGGL((unwrap_contiguous_kernel<T, 2>), grid, block, 0, st, in, out, g.len, g.S, g.seglen, units, range, rec);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    const dim3 grid((unsigned)std::min(cdiv(units, 256), MAX_GRID)), block(256);
    if (g.S == 1) {
        hipLaunchKernelGGL((unwrap_strided_kernel<T, 0>), grid, block, 0, st, in, out, g.inner, g.len, g.outer, g.S, g.seglen, units, range, rec);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    hipLaunchKernelGGL((unwrap_strided_kernel<T, 1>), grid, block, 0, st, in, out, g.inner, g.len, g.outer, g.S, g.seglen, units, range, rec);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(unwrap_carry_kernel, dim3(carry_grid), block, 0, st, rec, g.lines, g.S);
    MDSP_LAUNCH_CHECK();
    hipLaunchKernelGGL((unwrap_strided_kernel<T, 2>), grid, block, 0, st, in, out, g.inner, g.len, g.outer, g.S, g.seglen, units, range, rec);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_unwrap_geometry_for(int64_t inner, int64_t len, int64_t outer, int dtype, int64_t segments, int* route, int64_t* nsegments, int64_t* seglen,
                             int64_t* workspace_bytes) {
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, dtype, segments, &empty));
    const Geom g = make_geometry(inner, len, outer, segments);
    if (route) *route = g.route;
    if (nsegments) *nsegments = g.S;
    if (seglen) *seglen = g.seglen;
    if (workspace_bytes) *workspace_bytes = g.workspace;
    return MDSP_OK;
}

int mdsp_unwrap_plan_create(mdsp_unwrap_plan* plan, int64_t inner, int64_t len, int64_t outer, int dtype, double range, int64_t segments) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, dtype, segments, &empty));
    if (!valid_range(range, dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: range must be finite and nonzero in the element type (got %g)", range);
    auto pl = new mdsp_unwrap_plan_s();
    pl->g = make_geometry(inner, len, outer, segments);
    pl->dtype = dtype;
    pl->range = range;
    pl->empty = empty;
    if (pl->g.workspace > 0) {
        const int st = pl->ws.reserve((size_t)pl->g.workspace);
        if (st != MDSP_OK) {
            delete pl;
            return st;
        }
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_unwrap_plan_destroy(mdsp_unwrap_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_unwrap_plan_info(mdsp_unwrap_plan plan, int* route, int64_t* nsegments, int64_t* seglen, int64_t* workspace_bytes) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (route) *route = plan->g.route;
    if (nsegments) *nsegments = plan->g.S;
    if (seglen) *seglen = plan->g.seglen;
    if (workspace_bytes) *workspace_bytes = (int64_t)plan->ws.bytes;
    return MDSP_OK;
}

int mdsp_unwrap_exec(mdsp_unwrap_plan plan, const void* in_dev, void* out_dev, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (plan->empty) return MDSP_OK;
    if (!in_dev || !out_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(in_dev), b = reinterpret_cast<uintptr_t>(out_dev);
    const uintptr_t bytes = (uintptr_t)(plan->g.lines * plan->g.len) * dtype_size(plan->dtype);
    if (a != b && a < b + bytes && b < a + bytes) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: out must be the input array itself or not overlap it");
    if (a % dtype_size(plan->dtype) || b % dtype_size(plan->dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: arrays must be aligned to their element size");
    hipStream_t st = as_stream(stream);
    return plan->dtype == MDSP_F64 ? unwrap_exec<double>(plan, in_dev, out_dev, st) : unwrap_exec<float>(plan, in_dev, out_dev, st);
}

int mdsp_unwrap_emulate_host(const void* in_host, void* out_host, int64_t inner, int64_t len, int64_t outer, int dtype, double range, int64_t segments) {
    bool empty = false;
    MDSP_TRY(check_shape(inner, len, outer, dtype, segments, &empty));
    if (!valid_range(range, dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "unwrap: range must be finite and nonzero in the element type (got %g)", range);
    if (empty) return MDSP_OK;
    if (!in_host || !out_host) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    const Geom g = make_geometry(inner, len, outer, segments);
    if (dtype == MDSP_F64) emulate<double>(static_cast<const double*>(in_host), static_cast<double*>(out_host), g, range);
    else emulate<float>(static_cast<const float*>(in_host), static_cast<float*>(out_host), g, (float)range);
    return MDSP_OK;
}

}  // extern "C"
