// Decimator kernel (fir_dec.h; round 5): L = 1, any M <= 64, any filter length.  FIRDecimator (stream_filt.jl:43-56, :522-558) is the commonest multirate
// call and was the matrix-core kernel's worst shape: its product has 15 M structural-zero rows, the taps do not fit registers and the row stride M
// is bank-hostile (1//16 Float32 at 0.08 of the HBM roof, 87 % of the LDS cycles bank conflicts: profiles/r04_fir_decim16_pmc.json).
//
//     y[m] = sum_i h'[i] z[c + m M + i]     (h' = pfbT, the taps oldest sample first; z = [history ; x]; c = d0 - 1 + phi0 - 1)
//          = sum_{r < M}  sum_q h'[M q + r] z[c + M (m + q) + r]
//
// A lane owns ONE PHASE r of the M-decimated input: its inner sum is a short correlation (ceil(tp / M) taps) over every M-th sample, and the M
// lanes of a group read M CONSECUTIVE samples per step -- conflict-free whatever M is.  Per block of P = 16 outputs and chunk of QC = 8 taps a
// lane reads P + QC - 1 samples and QC taps from LDS for P QC multiply-adds; the M partial sums of an output meet through LDS (one write per
// lane and output, M reads by the lane that stores it).  Multiply-adds are packed pairs: a complex sample is one (real taps), and a real signal
// pairs the two halves of its tile (the staging loop writes sample k of the first half next to sample k of the second).
// Every output reads exactly its own tp-sample window, as the reference does: the zero taps that pad the last chunk are masked, not multiplied.
// The summation order differs from the reference's oldest-first chain (phases first, then across phases): results agree to rounding, state
// (history, phase, deficit) stays bit-exact -- it never was arithmetic.
#include "fir_dec.h"

#include <algorithm>
#include <type_traits>

#include "devio.h"
#include "fir_op.h"

using namespace mdsp;
using mdsp::fft::cx;

namespace {

template <typename R> struct DecV { R x, y; };
__device__ __forceinline__ DecV<float> dec_fma(DecV<float> w, float g, DecV<float> a) {
    typedef float f2v __attribute__((ext_vector_type(2)));
    const f2v d = __builtin_elementwise_fma(f2v{w.x, w.y}, f2v{g, g}, f2v{a.x, a.y});
    return {d.x, d.y};
}
__device__ __forceinline__ DecV<double> dec_fma(DecV<double> w, double g, DecV<double> a) { return {fma(w.x, g, a.x), fma(w.y, g, a.y)}; }

struct DecArgs {
    const void* x;
    const void* hist;
    void* y;
    const void* pfbT;      // tp taps, oldest sample first
    int64_t xlen, ldx, ldy, nout, zb;   // zb: index into [history ; x] of the first sample of output 0's window
    int M, Mp, logMp, tp, hl;
    int nq;                // ceil(tp / M) tap steps; the LDS tap table is padded to a multiple of QC steps
    int nbh;               // blocks of P outputs per half tile (real signals: a tile is two halves) / per tile (complex)
    int nz;                // staged samples per (half) tile
    unsigned blkmagic;     // ceil(2^32 / (P M)): k div (P M) == umulhi(k, blkmagic) for the staged indices
    int ablate;            // MDSP_FIR_DEC_ABLATE (profiling; garbage results): 1 no multiply-adds, 2 no staging, 4 no reduction / stores
};

// LDS position of staged sample k of a tile: M elements of padding behind every block of P M samples, so that the groups of a wavefront -- whose
// blocks start P M samples apart, a multiple of the 256-byte bank row for every power-of-two M -- read bank rows that interleave instead of coincide
// (first run without it: 2-way conflicts on every read at M = 16, 16-way at M = 2; profiles/r05_fir_dec_ab.json "first").
__device__ __forceinline__ int dec_pos(int k, int M, unsigned blkmagic) { return k + (int)__umulhi((unsigned)k, blkmagic) * M; }

// MC: M as a compile-time constant (0: run-time M) -- the window reads are then one address register plus immediates
// NC: the filter's chunks of QC taps per phase as a compile-time constant (0: run-time loop).  The chunk loop is then unrolled, so a lane's taps live in registers
// for the whole tile and its sample window SLIDES -- QC new samples per chunk instead of P + QC - 1: 8 LDS reads per 128 packed multiply-adds instead of 31.
// NC = 5 is every decimator resample_filter designs (36.4 taps per phase and M, stream_filt.jl / design.jl:700-720): the LDS was as busy as the vector unit
// with the run-time loop (per CU: 4 x 640 clocks of LDS reads against 2800 of multiply-adds per block).
template <typename R, bool CPLX, int P, int MC, int NC = 0>
MDSP_NO_LSO __global__ __launch_bounds__(256, (sizeof(R) == 4 ? 3 : 2)) void decimator_kernel(DecArgs a) {
    using V = DecV<R>;
    using XS = std::conditional_t<CPLX, cx<R>, R>;
    constexpr int QC = 8, PH = 4;   // taps per chunk; outputs per reduction round
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = MC ? MC : a.M, Mp = a.Mp;
    const int nqp = (a.nq + QC - 1) / QC * QC;
    const int nzp = dec_pos(a.nz - 1, M, a.blkmagic) + 1;
    V* zs = reinterpret_cast<V*>(smem);
    R* tl = reinterpret_cast<R*>(zs + nzp);
    V* red = reinterpret_cast<V*>(tl + (((size_t)nqp * M + 3) & ~(size_t)3));
    const int64_t ch = blockIdx.y;
    const int TO = (CPLX ? 1 : 2) * a.nbh * P;                  // outputs per tile
    const int64_t ntile = (a.nout + TO - 1) / TO;
    const XS* xc = static_cast<const XS*>(a.x) + ch * a.ldx;
    const XS* hc = static_cast<const XS*>(a.hist) + ch * (int64_t)a.hl;
    const int H = a.nbh * P * M;                                // samples between the two halves of a real tile
    // Float64 / ComplexF64 (PRE): a workgroup walks tiles blockIdx.x, + gridDim.x, ... with the NEXT tile's samples on their way from HBM (in registers: at
    // most 40 KiB a tile, ten 16-byte loads a thread) while this tile is multiplied; they are written to the LDS behind the barrier that ends it.  One
    // tile per workgroup -- the first form -- left staging and arithmetic to overlap across co-resident workgroups only, and they added up
    // (profiles/r05_fir_dec_ab.json "ablation").  Float64 1//4 ... 1//16 0.92 - 1.00 -> 0.82 - 0.98 ms, ComplexF64 1.93 - 2.23 -> 1.54 - 2.02.
    // Float32 / ComplexF32 keep one tile per workgroup: their 170 registers leave no room for the tile in flight at three workgroups per CU, and every
    // form that made room measured slower -- two workgroups per CU 0.51 ms at 1//8 against 0.44, eight outputs per block with three 0.64, with four
    // workgroups and 30 KiB tiles 0.88, 24 KiB tiles 0.64 (profiles/r05_fir_dec_ab.json "prefetch_forms").
    // Steady state: the tile (both halves of a real one) lies wholly inside x.  16-byte loads -- four Float32 samples, two Float64 / ComplexF32, one
    // ComplexF64; consecutive samples sit at consecutive LDS positions (a block's padding never falls inside a group: block lengths are multiples
    // of 16 samples, groups start at multiples of 4)
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    constexpr int NV = 16 / (int)sizeof(XS);
    constexpr bool PRE = sizeof(R) == 8;
    constexpr int NIT = PRE ? (CPLX ? 11 : 6) : 1;              // 256 threads x NIT x 16 (32: both halves) bytes: the 40 KiB of blocks (fir_dec_geo) plus the window tail
                                                                // (M = 16 with 40 tap steps: 43 KiB -- with ten / five loads those tiles fell out of the prefetching form)
    u4v pa[NIT], pb[CPLX ? 1 : NIT];
    const bool fits = a.nz <= 256 * NIT * NV;                   // (filters of several thousand taps per phase: the tile outgrows the registers -- staged in place)
    auto inside = [&](int64_t tile) {
        const int64_t zf = a.zb + tile * TO * M;
        return tile < ntile && !(a.ablate & 2) && zf >= a.hl && zf - a.hl + a.nz + (CPLX ? 0 : H) <= a.xlen;
    };
    auto steady = [&](int64_t tile) { return PRE && fits && inside(tile); };
    auto issue = [&](int64_t tile) __attribute__((always_inline)) {
        const int64_t zf = a.zb + tile * TO * M;
        const __amdgpu_buffer_rsrc_t rs = io::make_rsrc(xc + (zf - a.hl), (a.xlen - (zf - a.hl)) * (long long)sizeof(XS));
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int k = (threadIdx.x + u * 256) * NV;
            pa[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, k < a.nz ? k * (int)sizeof(XS) : io::OOB, 0, 0);
            if constexpr (!CPLX) pb[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, k < a.nz ? (k + H) * (int)sizeof(XS) : io::OOB, 0, 0);
        }
    };
    auto elem = [](const u4v& q, int i) -> XS {
        if constexpr (std::is_same_v<XS, float>) return __uint_as_float(q[i]);
        else if constexpr (std::is_same_v<XS, double>) return __hiloint2double((int)q[2 * i + 1], (int)q[2 * i]);
        else if constexpr (std::is_same_v<XS, cx<float>>) return XS{__uint_as_float(q[2 * i]), __uint_as_float(q[2 * i + 1])};
        else return XS{__hiloint2double((int)q[1], (int)q[0]), __hiloint2double((int)q[3], (int)q[2])};
    };
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int k = (threadIdx.x + u * 256) * NV;
            if (k < a.nz) {
                V* dst = zs + dec_pos(k, M, a.blkmagic);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    if constexpr (CPLX) {
                        const XS v = elem(pa[u], i);
                        dst[i] = {v.x, v.y};
                    } else dst[i] = {elem(pa[u], i), elem(pb[u], i)};
                }
            }
        }
    };
    auto stage_slow = [&](int64_t tile) {   // tiles that straddle the history or the end of x
        const int64_t zf = a.zb + tile * TO * M;
        if (inside(tile)) {                 // Float32: the whole tile in ONE round of 16-byte loads (ten a thread: the registers of the multiply-adds are not live
                                            // yet; four at a time were three HBM latencies per tile); Float64 tiles beyond the registers: four in flight
            constexpr int U = PRE ? 4 : (CPLX ? 10 : 5);
            const __amdgpu_buffer_rsrc_t rs = io::make_rsrc(xc + (zf - a.hl), (a.xlen - (zf - a.hl)) * (long long)sizeof(XS));
            for (int k0 = threadIdx.x * NV; k0 < a.nz; k0 += U * 256 * NV) {
                u4v va[U], vb[CPLX ? 1 : U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * 256 * NV;
                    va[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, k < a.nz ? k * (int)sizeof(XS) : io::OOB, 0, 0);
                    if constexpr (!CPLX) vb[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, k < a.nz ? (k + H) * (int)sizeof(XS) : io::OOB, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * 256 * NV;
                    if (k < a.nz) {
                        V* dst = zs + dec_pos(k, M, a.blkmagic);
#pragma unroll
                        for (int i = 0; i < NV; ++i) {
                            if constexpr (CPLX) {
                                const XS v = elem(va[u], i);
                                dst[i] = {v.x, v.y};
                            } else dst[i] = {elem(va[u], i), elem(vb[u], i)};
                        }
                    }
                }
            }
            return;
        }
        auto sample = [&](int64_t zi) -> XS {
            if (zi < a.hl) return hc[zi];
            if (zi - a.hl < a.xlen) return xc[zi - a.hl];
            return XS{};
        };
        for (int k = threadIdx.x; k < a.nz; k += 256) {
            if constexpr (CPLX) {
                const XS v = sample(zf + k);
                zs[dec_pos(k, M, a.blkmagic)] = {v.x, v.y};
            } else zs[dec_pos(k, M, a.blkmagic)] = {sample(zf + k), sample(zf + k + H)};
        }
    };
    int64_t tile = blockIdx.x;
    bool pre = steady(tile);                                    // workgroup-uniform
    if (pre) issue(tile);
    {
        const R* pf = static_cast<const R*>(a.pfbT);
        for (int k = threadIdx.x; k < nqp * M; k += 256) tl[k] = k < a.tp ? pf[k] : (R)0;
    }
    const int r = threadIdx.x & (Mp - 1), gq = threadIdx.x >> a.logMp, ng = 256 >> a.logMp;
    const bool lane_on = r < M;
    const int rr = lane_on ? r : 0;
    V* myred = red + (size_t)gq * PH * (Mp + 1);
    using Y = std::conditional_t<CPLX, cx<R>, R>;
    Y* yc = static_cast<Y*>(a.y) + ch * a.ldy;
    for (; tile < ntile; tile += gridDim.x) {
        const int64_t m0 = tile * TO;
        if (PRE && pre) commit();
        else if (!(a.ablate & 2)) stage_slow(tile);
        __syncthreads();
        if constexpr (PRE) {
            pre = steady(tile + gridDim.x);
            if (pre) issue(tile + gridDim.x);
        }
        for (int bl = gq; bl < a.nbh; bl += ng) {
            V acc[P];
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = {(R)0, (R)0};
            // sample (bl P + t) M + r of the tile sits at  bl (P + 1) M + (t + t div P) M + r : t = q0 + j walks the window
            const V* zb = zs + (size_t)bl * (P + 1) * M + rr;
            if constexpr (NC > 0) {
                if (!(a.ablate & 1)) {
                    constexpr bool GREG = sizeof(R) == 4;   // Float64: the taps of a chunk from LDS as it starts (80 registers of taps next to the tile in flight spilt)
                    R g[GREG ? NC * QC : QC];
                    if constexpr (GREG) {
#pragma unroll
                        for (int u = 0; u < NC * QC; ++u) g[u] = tl[u * M + rr];
                    }
                    V w[P + QC - 1];
#pragma unroll
                    for (int j = 0; j < P + QC - 1; ++j) w[j] = zb[(j + j / P) * M];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int q0 = c * QC, g0 = GREG ? q0 : 0;
                        if constexpr (!GREG) {
#pragma unroll
                            for (int u = 0; u < QC; ++u) g[u] = tl[(q0 + u) * M + rr];
                        }
                        if (c > 0) {
#pragma unroll
                            for (int j = 0; j < P - 1; ++j) w[j] = w[j + QC];
#pragma unroll
                            for (int j = P - 1; j < P + QC - 1; ++j) {
                                const int t = q0 + j;
                                w[j] = zb[(t + t / P) * M];
                            }
                        }
                        if (c < NC - 1 || (q0 + QC) * M <= a.tp) {
#pragma unroll
                            for (int u = 0; u < QC; ++u)
#pragma unroll
                                for (int p = 0; p < P; ++p) acc[p] = dec_fma(w[p + u], g[g0 + u], acc[p]);
                        } else {   // the last chunk, masked as below
#pragma unroll
                            for (int u = 0; u < QC; ++u) {
                                if ((q0 + u) * M + rr < a.tp) {
#pragma unroll
                                    for (int p = 0; p < P; ++p) acc[p] = dec_fma(w[p + u], g[g0 + u], acc[p]);
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                }
            } else
            for (int q0 = 0; q0 < ((a.ablate & 1) ? 0 : a.nq); q0 += QC) {
                R g[QC];
                V w[P + QC - 1];
#pragma unroll
                for (int u = 0; u < QC; ++u) g[u] = tl[(q0 + u) * M + rr];
#pragma unroll
                for (int j = 0; j < P + QC - 1; ++j) {
                    const int t = q0 + j;
                    w[j] = zb[(t + t / P) * M];
                }
                if ((q0 + QC) * M <= a.tp) {   // every tap of the chunk exists (uniform)
#pragma unroll
                    for (int u = 0; u < QC; ++u)
#pragma unroll
                        for (int p = 0; p < P; ++p) acc[p] = dec_fma(w[p + u], g[u], acc[p]);
                } else {                       // the last chunk: positions past the filter's end are not read (a NaN there must not reach the output).  A lane
                                               // whose tap does not exist sits the step out under the execution mask (first form: a select per multiply-add --
                                               // 256 v_cndmask next to 128 packed FMAs, the chunk cost as much as three others: profiles/r05_fir_dec_ab.json)
#pragma unroll
                    for (int u = 0; u < QC; ++u) {
                        if ((q0 + u) * M + rr < a.tp) {
#pragma unroll
                            for (int p = 0; p < P; ++p) acc[p] = dec_fma(w[p + u], g[u], acc[p]);
                        }
                        __builtin_amdgcn_sched_barrier(0);   // keeps the eight guarded groups apart (if-conversion would bring the selects back)
                    }
                }
            }
            // the M partial sums of every output meet in LDS (the lanes of a group sit in one wavefront: its DS operations execute in order)
#pragma unroll
            for (int p0 = 0; p0 < ((a.ablate & 4) ? 0 : P); p0 += PH) {
                __builtin_amdgcn_wave_barrier();
                if (lane_on) {
#pragma unroll
                    for (int p = 0; p < PH; ++p) myred[p * (Mp + 1) + r] = acc[p0 + p];
                }
                __builtin_amdgcn_wave_barrier();
                for (int pp = r; pp < PH; pp += Mp) {
                    V s = myred[pp * (Mp + 1)];
                    for (int k = 1; k < M; ++k) {
                        const V t = myred[pp * (Mp + 1) + k];
                        s.x += t.x;
                        s.y += t.y;
                    }
                    const int64_t m = m0 + (int64_t)bl * P + p0 + pp;
                    if constexpr (CPLX) {
                        if (m < a.nout) yc[m] = Y{s.x, s.y};
                    } else {
                        if (m < a.nout) yc[m] = s.x;
                        if (m + (int64_t)a.nbh * P < a.nout) yc[m + (int64_t)a.nbh * P] = s.y;
                    }
                }
            }
        }
        if constexpr (!PRE) break;   // (one tile per workgroup: straight-line code -- as a loop the Float32 form spilt 27 registers and ran 1.5x slower)
        __syncthreads();   // every group has read its last window before the next tile's samples overwrite them
    }
}

}  // namespace

// ---- decimator kernel: geometry (DecGeo: fir_dec.h) and launch -----------------------------------------------------------------------------------
DecGeo mdsp::fir_dec_geo(const mdsp_fir_s* f) {
    DecGeo g;
    if (f->ctaps || f->L != 1 || f->M < 2 || f->M > 64 || tunables().fir_dec == 0 || tunables().fir_exact || f->exact || MDSP_DBG(fir_generic)) return g;
    if (f->acc_double != dtype_is_double(f->x_dtype)) return g;   // Float32 samples under Float64 taps: the generic kernel converts as it stages
    // Where it wins (profiles/r05_fir_dec_ab.json, 4 channels x 2^26 samples, resample_filter taps): Float64 / ComplexF64 from M = 4 on (1.1 - 4.1x),
    // Float32 / ComplexF32 at M = 4 (1.17 - 1.19x) and from M = 8 on (1.1 - 3.9x); at M = 2, 3 and the Float32 M = 5, 6, 7 the matrix-core kernel's
    // short products stay ahead (0.31 - 0.54 of the roof against 0.24 - 0.38).  MDSP_FIR_DEC=3 takes it for every M <= 64 (tests).
    // (re-measured with the unrolled chunk loop, profiles/r05_fir_dec_ab.json "rule_recheck": unchanged but for real Float32 at M = 3 -- 0.52 against 0.61 ms)
    if (tunables().fir_dec == 1 && !(f->acc_double ? f->M >= 4 : (f->M == 4 || f->M >= 8 || (f->M == 3 && !dtype_is_complex(f->x_dtype))))) return g;
    const bool dbl = f->acc_double, cplx = dtype_is_complex(f->x_dtype);
    const int M = (int)f->M;
    g.P = dbl ? 8 : 16;
    g.Mp = 2;
    g.logMp = 1;
    while (g.Mp < M) g.Mp *= 2, ++g.logMp;
    if (f->tp > (int64_t)1 << 20) return g;
    g.nq = (int)cdiv(f->tp, M);
    const int nqp = (g.nq + 7) / 8 * 8, ng = 256 / g.Mp;
    const size_t vsz = dbl ? 16 : 8, rsz = dbl ? 8 : 4;
    // blocks per (half) tile: a multiple of the groups of a workgroup (every group the same number of blocks), as many as ~40 KiB of samples hold
    int kb = 1;
    while (((size_t)ng * (kb + 1) * g.P * M + (size_t)nqp * M) * vsz <= 40 * 1024) ++kb;
    g.nbh = ng * kb;
    g.nz = g.nbh * g.P * M + nqp * M;
    const size_t nzp = (size_t)g.nz + (size_t)((g.nz - 1) / (g.P * M)) * M;   // with M elements of padding behind every block (dec_pos)
    g.lds = nzp * vsz + (((size_t)nqp * M + 3) & ~(size_t)3) * rsz + (size_t)ng * 4 * (g.Mp + 1) * vsz;
    (void)cplx;
    g.ok = g.lds <= 150 * 1024;
    return g;
}

namespace {
template <typename R, bool CPLX, int P> int fir_dec_launch(mdsp_fir_s* f, const FirArgs& a, const DecGeo& g, hipStream_t st) {
    DecArgs d{};
    d.x = a.x;
    d.hist = a.hist;
    d.y = a.y;
    d.pfbT = a.pfbT;
    d.xlen = a.xlen;
    d.ldx = a.ldx;
    d.ldy = a.ldy;
    d.nout = a.nout;
    d.zb = a.d0 - 1 + a.phi0m1;
    d.M = a.M;
    d.Mp = g.Mp;
    d.logMp = g.logMp;
    d.tp = a.tp;
    d.hl = a.hl;
    d.nq = g.nq;
    d.nbh = g.nbh;
    d.nz = g.nz;
    d.ablate = tunables().fir_dec_ablate;
    d.blkmagic = (unsigned)((((uint64_t)1 << 32) + (uint64_t)(P * a.M) - 1) / (uint64_t)(P * a.M));
    void (*kern)(DecArgs) = decimator_kernel<R, CPLX, P, 0>;
    // chunks of taps per phase: five is what resample_filter designs for every decimator; two .. six unrolled for M = 4, 8, 16 (the run-time loop otherwise)
    const int nc = tunables().fir_dec_nc != 0 ? (g.nq + 7) / 8 : 0;
#define MDSP_DEC_NC(MCV)                                                                      \
    switch (nc) {                                                                             \
        case 2: kern = decimator_kernel<R, CPLX, P, MCV, 2>; break;                           \
        case 3: kern = decimator_kernel<R, CPLX, P, MCV, 3>; break;                           \
        case 4: kern = decimator_kernel<R, CPLX, P, MCV, 4>; break;                           \
        case 5: kern = decimator_kernel<R, CPLX, P, MCV, 5>; break;                           \
        case 6: kern = decimator_kernel<R, CPLX, P, MCV, 6>; break;                           \
        default: kern = decimator_kernel<R, CPLX, P, MCV>; break;                             \
    }
    switch (a.M) {
        case 2: kern = decimator_kernel<R, CPLX, P, 2>; break;
        case 4: MDSP_DEC_NC(4) break;
        case 8: MDSP_DEC_NC(8) break;
        case 16: MDSP_DEC_NC(16) break;
        default:
            if (nc == 5) kern = decimator_kernel<R, CPLX, P, 0, 5>;
            break;
    }
#undef MDSP_DEC_NC
    if (tunables().fir_dec == 2) kern = decimator_kernel<R, CPLX, P, 0>;   // MDSP_FIR_DEC=2: the run-time M form for every M
    if (g.lds > 48 * 1024) MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    const int64_t TO = (int64_t)(CPLX ? 1 : 2) * g.nbh * P;
    // Float64: the workgroups that stay resident (two a CU), each walking its share of the tiles with the next one's samples in flight; Float32: one tile each
    const int64_t ntile = cdiv(a.nout, TO);
    const int wgs = tunables().fir_dec_wgs > 0 ? tunables().fir_dec_wgs : 2;
    const int64_t per = sizeof(R) == 8 ? std::max<int64_t>(1, (int64_t)device_cu_count() * wgs / std::max<int64_t>(1, f->nch)) : ntile;
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(ntile, per), (unsigned)f->nch), dim3(256), g.lds, st, d);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}
}  // namespace

int mdsp::fir_dec_dispatch(mdsp_fir_s* f, const FirArgs& a, const DecGeo& g, hipStream_t st) {
    switch (f->x_dtype) {
        case MDSP_F32: return fir_dec_launch<float, false, 16>(f, a, g, st);
        case MDSP_F64: return fir_dec_launch<double, false, 8>(f, a, g, st);
        case MDSP_C32: return fir_dec_launch<float, true, 16>(f, a, g, st);
        default: return fir_dec_launch<double, true, 8>(f, a, g, st);
    }
}
