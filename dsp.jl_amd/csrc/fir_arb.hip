// FIRArbitrary (floating-point rate; mdsp_firarb_*, mdsp_arb_*): polyphase bank + derivative bank with linear interpolation between
// neighbouring phases (stream_filt.jl:80-134, filt! :579-625).
//
// The reference advances a Float64 phase accumulator serially (update! :567-577): phiAcc += Delta; on overflow
// (dx, phiAcc) = divrem(phiAcc, Nphi), xIdx += dx; alpha = frac(phiAcc), phiIdx = 1 + trunc(phiAcc).  Every step
// rounds, so the index sequence depends on the accumulated roundings.  To stay bit-exact with it, anchors -- the exact
// (xIdx, phiAcc) of every ARB_BLK-th output -- are produced either by the same IEEE operations run serially on the host
// (arb_trajectory, short streams) or by the parallel integer evaluation of arb_scan.h on the device (long streams), cached
// per (state, length) and shared by all channels.  Wave 0 of a workgroup replays ARB_BLK updates per lane from those anchors
// (v_add_f64 / v_floor_f64 are IEEE-exact; ArbStep::fast) into an LDS record per output, then all threads evaluate
//   y = muladd(yUpper, alpha, yLower)   (:616) with yLower/yUpper the two tapsPerPhase-term
// chains (oldest sample first) over the input span staged in LDS.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "fir_plan.h"
#include "fir_op.h"
#include "arb_scan.h"

using namespace mdsp;
using namespace mdsp::firop;
using mdsp::fft::cx;

namespace {

constexpr int ARB_BLK = 16;   // outputs per anchor (16 bytes each: 1 B of extra traffic per output); one lane of wave 0 replays one block

struct ArbStep {              // one update! (stream_filt.jl:567-577), shared by host and device
    double delta, nphi, inv_nphi;
    double c1, c2;            // qd nphi and (qd + 1) nphi, qd = floor(delta / nphi): the only two quotients an update can produce
    int64_t qd;
    static ArbStep make(double delta, double nphi) {
        ArbStep s{};
        s.delta = delta;
        s.nphi = nphi;
        s.inv_nphi = 1.0 / nphi;
        const double rd = std::fmod(delta, nphi);   // exact
        s.qd = (int64_t)((delta - rd) / nphi);       // exact: delta - rd is a multiple of nphi
        s.c1 = (double)s.qd * nphi;
        s.c2 = (double)(s.qd + 1) * nphi;
        return s;
    }
    // The reference's form, operation by operation.
    __host__ __device__ inline void operator()(double& acc, int64_t& xidx) const {
        acc = acc + delta;
        if (acc >= nphi) {
            if (acc < 2.0 * nphi) {
                // q = 1, the common overflow: nphi <= acc < 2 nphi makes acc - nphi exact (Sterbenz), which is what divrem
                // returns -- and keeps floor / multiply / compare-and-fix off the loop-carried chain
                acc -= nphi;
                xidx += 1;
                return;
            }
            // divrem(acc, nphi): q = floor(acc/nphi) up to one unit, r = acc - q nphi (exact), then fix q
            double q = floor(acc * inv_nphi);
            double r = acc - q * nphi;   // q nphi is an exact integer and |r| <= acc is a multiple of ulp(acc): exact with or without FMA
            if (r < 0.0) {
                q -= 1.0;
                r += nphi;
            } else if (r >= nphi) {
                q += 1.0;
                r -= nphi;
            }
            xidx += (int64_t)q;
            acc = r;
        }
    }
    // Branch-free equivalent for the device replay.  s = fl(acc + delta) lies in [delta, nphi + delta], so the quotient of
    // divrem(s, nphi) is qd or qd + 1 (none when qd = 0 and s < nphi); for a quotient q >= 1, q nphi <= s < (q + 1) nphi <= 2 q nphi
    // makes s - q nphi exact (Sterbenz) -- the exact remainder divrem returns.  Valid while qd nphi < 2^53.
    __host__ __device__ inline void fast(double& acc, int64_t& xidx) const {
        const double s = acc + delta;
        const double r1 = s - c1, r2 = s - c2;   // both candidates next to the compare: three dependent operations per update instead of four
        const bool big = s >= c2;
        acc = big ? r2 : r1;
        xidx += qd + (big ? 1 : 0);
    }
};

struct ArbArgs {
    const void* x;
    const void* hist;
    void* y;
    const void* taps2;    // tp * Nphi pairs (pfb, dpfb), taps2[i*Nphi + phi]
    const int64_t* tab_x; // 1-based xIdx of output ARB_BLK b
    const double* tab_acc;
    int64_t xlen, ldx, ldy, nout, nch;
    ArbStep step;
    int nphi, tp, hl;
    int tile;             // outputs per workgroup (multiple of ARB_BLK)
    int span;             // staged samples per tile (0: read [history ; x] straight from global/L2)
    int taps_in_lds;
    long long* prof;      // profiling only (MDSP_ARB_PROF): 8 clock64() stamps per workgroup
    int ablate;           // profiling only (MDSP_ABLATE): 1 no phase-A replay, 2 one tap instead of tp, 4 no staging loads, 8 no tap copy
    int prio;             // MDSP_ARB_PRIO: 1 = the prologue (replay, tap copy, staging) runs at raised wave priority
};

// Per-output trajectory records of a tile, written by phase A: the phase accumulator (phi = floor(acc), alpha = acc - phi: both exact, taken
// at the point of use) and xIdx relative to the tile's first output.  Two arrays (8 + 4 bytes per output instead of one 16-byte record):
// with 1185 taps x 32 phases and four interleaved channels the workgroup needs 38 KiB of LDS instead of 43 -- FOUR workgroups per CU instead
// of three, which is what this kernel's prologue / compute overlap lives on.
struct ArbRecs {
    double* acc;
    int* xrel;
};

// both arrays are written by phase A with a lane stride of ARB_BLK records: one pad record per ARB_BLK keeps those stores off a single
// bank group
__host__ __device__ constexpr int arb_rec_slot(int j) { return j + j / ARB_BLK; }
__host__ __device__ constexpr size_t arb_rec_bytes(int tile) { return ((size_t)arb_rec_slot(tile) * 12 + 15) & ~size_t(15); }

template <typename R> struct alignas(2 * sizeof(R)) Tap2 {   // (pfb, dpfb) of one (tap, phase): one 8 / 16-byte LDS read feeds both chains
    R p, d;
};

// One tile of outputs for one group of NCH channels.  `pf` is either the LDS copy of the tap pairs or the global
// table (the caller branches, so each copy of this body sees one address space and the LDS copy compiles to
// ds_read_b64); the samples of the NCH channels are interleaved in LDS, zs[k * NCH + c], so one tap-pair read and one
// NCH-wide sample read feed 2 NCH FMAs: 4 + 8 / NCH bytes of LDS traffic per tap and output instead of 12.
// ds_read_b128 is serviced in four groups of 16 NON-contiguous lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and the same
// +32; MI355X_MICROARCH.md, LDS): lane l of a wave takes output ARB_B128_ORDER[l & 31] + (l & 32) of the wave's 64, so each
// group reads the windows of 16 CONSECUTIVE outputs -- consecutive 16-byte slots, no bank conflicts for rates >= 1
// (measured before: half of the kernel's LDS cycles were conflicts on this read).
__device__ const unsigned char ARB_B128_ORDER[32] = {0,  1,  2,  3,  16, 17, 18, 19, 20, 21, 22, 23, 4,  5,  6,  7,
                                                     24, 25, 26, 27, 8,  9,  10, 11, 12, 13, 14, 15, 28, 29, 30, 31};

// NPHI: the number of phases when it is known at compile time (32, the reference's default: the tap reads of an unrolled batch
// then differ by immediate offsets from one address register instead of one register and one v_add each), 0: run-time nphi
template <typename A, typename R, int NCH, int NPHI>
__device__ __forceinline__ void arb_tile_staged_n(const ArbRecs rec, const Tap2<R>* __restrict__ pf, const A* zs, A* const (&yc)[NCH], int nc, int cnt,
                                                  int tp, int nphi_rt) {
    const int nphi = NPHI ? NPHI : nphi_rt;
    struct alignas(sizeof(A) * NCH <= 16 ? sizeof(A) * NCH : 16) ZV {
        A v[NCH];
    };
    const ZV* zv = reinterpret_cast<const ZV*>(zs);
    int j0 = threadIdx.x;
    if constexpr (sizeof(ZV) == 16) j0 = (j0 & ~31) + ARB_B128_ORDER[j0 & 31];
    for (int j = j0; j < cnt; j += blockDim.x) {
        const double racc = rec.acc[arb_rec_slot(j)];
        const double rfl = floor(racc);
        const double ralpha = racc - rfl;
        const Tap2<R>* hq = pf + (int)rfl;
        const ZV* zp = zv + rec.xrel[arb_rec_slot(j)];
        A lo[NCH], up[NCH];
        {
            const Tap2<R> t = *hq;
            const ZV z = zp[0];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                lo[c] = mul_first(t.p, z.v[c]);
                up[c] = mul_first(t.d, z.v[c]);
            }
        }
        // taps 1 .. tp-1 in batches of 8 (sixteen LDS reads in flight, then their FMAs in tap order), the remainder as one batch of 4, 2 and 1
        // (wave-uniform branches) instead of single taps that each wait for their own two reads
        auto batch = [&](auto n, int i0) __attribute__((always_inline)) {
            constexpr int N = decltype(n)::value;
            Tap2<R> t[N];
            ZV z[N];
#pragma unroll
            for (int r = 0; r < N; ++r) {
                t[r] = hq[(i0 + r) * nphi];
                z[r] = zp[i0 + r];
            }
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    fma_acc(lo[c], t[r].p, z[r].v[c]);
                    fma_acc(up[c], t[r].d, z[r].v[c]);
                }
            }
        };
        int i = 1;
        for (; i + 8 <= tp; i += 8) batch(std::integral_constant<int, 8>{}, i);
        if ((tp - i) & 4) {
            batch(std::integral_constant<int, 4>{}, i);
            i += 4;
        }
        if ((tp - i) & 2) {
            batch(std::integral_constant<int, 2>{}, i);
            i += 2;
        }
        if ((tp - i) & 1) batch(std::integral_constant<int, 1>{}, i);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (c < nc) yc[c][j] = arb_combine(up[c], ralpha, lo[c]);
    }
}
template <typename A, typename R, int NCH>
__device__ __forceinline__ void arb_tile_staged(const ArbRecs rec, const Tap2<R>* __restrict__ pf, const A* zs, A* const (&yc)[NCH], int nc, int cnt,
                                                int tp, int nphi) {
    if (nphi == 32) arb_tile_staged_n<A, R, NCH, 32>(rec, pf, zs, yc, nc, cnt, tp, nphi);
    else arb_tile_staged_n<A, R, NCH, 0>(rec, pf, zs, yc, nc, cnt, tp, nphi);
}

// (the second launch bound: four workgroups per CU -- what the 38 KiB of LDS of the Float32 four-channel form admit -- need <= 128 VGPRs)
template <typename XS, typename A, typename R, int NCH>
MDSP_NO_LSO __global__ __launch_bounds__(256, (sizeof(A) * NCH <= 16 ? 4 : 1)) void arbitrary_fir_kernel(ArbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ArbRecs rec{reinterpret_cast<double*>(smem), reinterpret_cast<int*>(smem + (size_t)arb_rec_slot(a.tile) * sizeof(double))};
    A* zs = reinterpret_cast<A*>(smem + arb_rec_bytes(a.tile));
    Tap2<R>* ps = reinterpret_cast<Tap2<R>*>(smem + arb_rec_bytes(a.tile) + (size_t)a.span * NCH * sizeof(A));
    const int64_t m0 = (int64_t)blockIdx.x * a.tile;
    if (m0 >= a.nout) return;
    const int cnt = (int)std::min<int64_t>(a.tile, a.nout - m0);
    const int64_t b0 = m0 / ARB_BLK;
    const int tid = threadIdx.x;
    auto stamp = [&](int k) {
        if (a.prof && tid == 0) a.prof[(int64_t)blockIdx.x * 8 + k] = clock64();
    };
    if ((a.prio & 1) || ((a.prio & 2) && tid < 64)) __builtin_amdgcn_s_setprio(3);   // a workgroup in its latency-bound prologue (1), or only its replaying wave (2), goes first among the co-resident ones
    stamp(0);
    const int64_t x_first = a.tab_x[b0];
    const int64_t z_first = x_first - 1;                                    // z = [history ; x], output n reads z[n-1 .. n-1+tp)
    if (a.prof && tid == 0) a.prof[(int64_t)blockIdx.x * 8 + 1] = clock64() + (x_first & 0);
    auto zload = [&](int64_t ch, int64_t zi) -> A {   // branch-free: the loads of a staging batch all issue before the first wait
        const XS* xc = static_cast<const XS*>(a.x) + ch * a.ldx;
        const XS* hc = static_cast<const XS*>(a.hist) + ch * (int64_t)a.hl;
        const int64_t xi = zi - a.hl;
        const bool in_hist = zi < a.hl, ok = in_hist || xi < a.xlen;
        const XS* p = in_hist ? hc + zi : xc + (xi < a.xlen ? xi : 0);
        const A v = to_acc(*p, (A*)nullptr);
        return ok ? v : A{};
    };
    // stage z[z_first .. z_first + count) of the channel group at c0 into zs, interleaved; `lanes` threads starting at `first`.  Loads and
    // stores of a round are separate steps so that the prologue can put the tap copy's loads in front of the same wait.
    constexpr int RB = sizeof(A) * NCH <= 16 ? 6 : 4;   // RB * NCH independent loads in flight per thread (six rounds of 192 threads cover a 1024-output tile's span at rates >= 1)
    // a tile whose whole span lies inside x (every tile but the first and the last few of a call) loads through one uniform base pointer per
    // channel: the history / end-of-input selects of zload cost a dozen vector instructions per load, which is most of what the staging
    // waves issue -- and they issue in competition with three computing workgroups
    const bool interior = z_first >= a.hl && z_first + a.span <= (int64_t)a.hl + a.xlen;
    auto stage_loads = [&](A(&v)[RB][NCH], int64_t c0, int nc, int k0, int lanes, int count) __attribute__((always_inline)) {
        if (interior) {
            const XS* xb[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) xb[c] = static_cast<const XS*>(a.x) + (c0 + (c < nc ? c : 0)) * a.ldx + (z_first - a.hl);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int k = min(k0 + r * lanes, count - 1);
#pragma unroll
                for (int c = 0; c < NCH; ++c) v[r][c] = to_acc(xb[c][k], (A*)nullptr);
            }
        } else {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int k = k0 + r * lanes;
                const int64_t zi = z_first + (k < count ? k : count - 1);
#pragma unroll
                for (int c = 0; c < NCH; ++c) v[r][c] = zload(c0 + (c < nc ? c : 0), zi);
            }
        }
    };
    auto stage_stores = [&](const A(&v)[RB][NCH], int nc, int k0, int lanes, int count) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int k = k0 + r * lanes;
            if (k < count) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) zs[k * NCH + c] = c < nc ? v[r][c] : A{};
            }
        }
    };
    auto stage = [&](int64_t c0, int nc, int first, int lanes, int count) __attribute__((always_inline)) {
        for (int k0 = first; k0 < count; k0 += RB * lanes) {
            A v[RB][NCH];
            stage_loads(v, c0, nc, k0, lanes, count);
            stage_stores(v, nc, k0, lanes, count);
        }
    };
    const Tap2<R>* pg = static_cast<const Tap2<R>*>(a.taps2);
    const int64_t c_first = (int64_t)blockIdx.y * NCH;
    // Prologue, wave-specialised so that its two latency chains overlap: wave 0 replays the recurrence from the anchors (phase A,
    // once per tile, shared by every channel; one lane per ARB_BLK outputs), waves 1..3 meanwhile copy the tap pairs and stage the
    // first channel group's samples (the whole span: its exact extent is only known after phase A).
    if (tid < 64) {
        if (tid * ARB_BLK < cnt) {
            int64_t xi = a.tab_x[b0 + tid];
            double acc = a.tab_acc[b0 + tid];
            const int base = tid * ARB_BLK;
            const int n = min(ARB_BLK, cnt - base);
            for (int k = 0; k < n; ++k) {
                rec.acc[arb_rec_slot(base + k)] = acc;
                rec.xrel[arb_rec_slot(base + k)] = (int)(xi - x_first);
                if (!MDSP_ABLATED(a, 1)) a.step.fast(acc, xi);
            }
        }
        stamp(2);
    } else {
        const int lanes = (int)blockDim.x - 64, u = tid - 64;
        // the tap pairs travel as 16-byte units (two Float32 pairs, one Float64 pair); round 0 of the tap copy and round 0 of the staging
        // issue ALL their loads before the first wait -- one memory latency for the tap table and the whole span of a 1024-output tile
        constexpr int RT = 4;
        const bool do_taps = a.taps_in_lds && !MDSP_ABLATED(a, 8);
        const bool do_stage = a.span > 0 && c_first < a.nch && !MDSP_ABLATED(a, 4);
        const int np = a.tp * a.nphi;
        const int nu = do_taps ? (int)((size_t)np * sizeof(Tap2<R>) / 16) : 0;
        const int nc0 = (int)std::min<int64_t>(NCH, a.nch - c_first);
        const uint4* pg16 = reinterpret_cast<const uint4*>(pg);
        uint4* ps16 = reinterpret_cast<uint4*>(ps);
        uint4 tv[RT];
        A sv[RB][NCH];
#pragma unroll
        for (int r = 0; r < RT; ++r) tv[r] = pg16[min(u + r * lanes, max(nu, 1) - 1)];   // unconditional (the table always exists): no private copy of tv
        stage_loads(sv, do_stage ? c_first : 0, do_stage ? nc0 : 1, u, lanes, max(a.span, 1));
        if (do_taps) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (u + r * lanes < nu) ps16[u + r * lanes] = tv[r];
        }
        if (do_stage) stage_stores(sv, nc0, u, lanes, a.span);
        if (do_taps) {
            for (int k0 = u + RT * lanes; k0 < nu; k0 += RT * lanes) {
#pragma unroll
                for (int r = 0; r < RT; ++r) tv[r] = pg16[min(k0 + r * lanes, nu - 1)];
#pragma unroll
                for (int r = 0; r < RT; ++r)
                    if (k0 + r * lanes < nu) ps16[k0 + r * lanes] = tv[r];
            }
            if constexpr (sizeof(Tap2<R>) == 8) {
                if ((np & 1) && u == 0) ps[np - 1] = pg[np - 1];   // an odd number of 8-byte pairs: the last one is not part of a 16-byte unit
            }
        }
        if (do_stage) stage(c_first, nc0, u + RB * lanes, lanes, a.span);
    }
    __syncthreads();
    if (a.prio) __builtin_amdgcn_s_setprio(0);
    stamp(3);
    const int64_t nz = (int64_t)rec.xrel[arb_rec_slot(cnt - 1)] + a.tp;
    const bool staged = nz <= a.span;                                       // workgroup-uniform
    for (int64_t c0 = c_first; c0 < a.nch; c0 += (int64_t)gridDim.y * NCH) {
        const int nc = (int)std::min<int64_t>(NCH, a.nch - c0);
        if (staged) {
            if (c0 != c_first) {
                __syncthreads();   // the previous channel group's readers are done with zs
                stage(c0, nc, tid, (int)blockDim.x, (int)nz);
                __syncthreads();
            }
            A* yc[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) yc[c] = static_cast<A*>(a.y) + (c0 + (c < nc ? c : 0)) * a.ldy + m0;
            const int tpe = MDSP_ABLATED(a, 2) ? 1 : a.tp;
            if (a.taps_in_lds) arb_tile_staged<A, R, NCH>(rec, ps, zs, yc, nc, cnt, tpe, a.nphi);
            else arb_tile_staged<A, R, NCH>(rec, pg, zs, yc, nc, cnt, tpe, a.nphi);
            stamp(4);
        } else {
            const Tap2<R>* pf = a.taps_in_lds ? ps : pg;
            for (int c = 0; c < nc; ++c) {
                A* yc = static_cast<A*>(a.y) + (c0 + c) * a.ldy;
                for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
                    const double racc = rec.acc[arb_rec_slot(j)];
                    const double rfl = floor(racc);                                 // alpha = modf(acc)[1] is exact
                    const Tap2<R>* hp = pf + (int)rfl;
                    const int64_t z0 = z_first + rec.xrel[arb_rec_slot(j)];
                    A z = zload(c0 + c, z0);
                    Tap2<R> t = hp[0];
                    A lo = mul_first(t.p, z);
                    A up = mul_first(t.d, z);
                    for (int i = 1; i < a.tp; ++i) {
                        z = zload(c0 + c, z0 + i);
                        t = hp[(int64_t)i * a.nphi];
                        fma_acc(lo, t.p, z);
                        fma_acc(up, t.d, z);
                    }
                    yc[m0 + j] = arb_combine(up, racc - rfl, lo);
                }
            }
        }
    }
    __syncthreads();
    stamp(5);
}

// ---- FIRArbitrary host side ---------------------------------------------------------------------------------
// The loop of filt!(buffer, ::FIRFilter{FIRArbitrary}, x) (stream_filt.jl:593-622) without the dot products.
// Anchors (xIdx, phiAcc) of outputs 0, blk, 2 blk, ... go to ax / aa when given.  Same IEEE operations as the
// reference, so the trajectory -- and with it the output count and the final state -- is bit-exact.
// kstop: stop after that many outputs (a multiple of blk) with the state of output kstop -- the pilot of the parallel scan.
void arb_trajectory(double acc, int64_t deficit, const ArbStep& st, int64_t xlen, int64_t blk, std::vector<int64_t>* ax, std::vector<double>* aa,
                    int64_t* nout, double* acc_end, int64_t* xidx_end, int64_t kstop = INT64_MAX) {
    int64_t n = 0, xi = deficit;
    const double nphi = st.nphi, nphi2 = 2.0 * st.nphi, nphi3 = 3.0 * st.nphi, nphi4 = 4.0 * st.nphi, delta = st.delta;
    while (xi <= xlen && n < kstop) {
        if (ax) {
            ax->push_back(xi);
            aa->push_back(acc);
        }
        // one anchor block: the loop-carried chain is add -> compare -> (subtract); q = 1 is the common overflow and
        // acc - nphi is exact there (Sterbenz), which is what divrem returns
        const int64_t stop = n + blk;
        while (n < stop && xi <= xlen) {
            ++n;
            const double prev = acc;
            acc = prev + delta;
            if (acc >= nphi) {
                if (acc < nphi2) {
                    acc -= nphi;
                    xi += 1;
                } else if (acc < nphi3) {   // q = 2, 3: same argument (q nphi <= acc < 2 q nphi)
                    acc -= nphi2;
                    xi += 2;
                } else if (acc < nphi4) {
                    acc -= nphi3;
                    xi += 3;
                } else {               // many input samples skipped at once (rate < 1/4): the general divrem
                    acc = prev;
                    st(acc, xi);
                }
            }
        }
    }
    *nout = n;
    *acc_end = acc;
    *xidx_end = xi;
}

// ---- parallel trajectory scan (arb_scan.h): kernels and drivers ------------------------------------------------
static_assert(arbscan::ANCH == ARB_BLK && arbscan::BLK == 2 * ARB_BLK, "two anchors per scan block");

template <int RC> __global__ __launch_bounds__(256) void arb_scan_tables_kernel(arbscan::ScanArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < a.nb) arbscan::scan_tables_body<RC>(a, b);
}
template <int RC, typename TIn> __global__ __launch_bounds__(256) void arb_scan_compose_kernel(arbscan::Grid G, const TIn* in, int64_t n, int64_t* out, int64_t ng) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < ng) arbscan::scan_compose_body<RC>(G, in, n, out, g);
}
template <typename TIn> void launch_compose(const arbscan::Grid& G, const TIn* in, int64_t n, int64_t* out, int64_t ng, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(ng, (int64_t)256));
    switch (G.R) {
        case 2: hipLaunchKernelGGL((arb_scan_compose_kernel<2, TIn>), grid, dim3(256), 0, st, G, in, n, out, ng); break;
        case 4: hipLaunchKernelGGL((arb_scan_compose_kernel<4, TIn>), grid, dim3(256), 0, st, G, in, n, out, ng); break;
        case 8: hipLaunchKernelGGL((arb_scan_compose_kernel<8, TIn>), grid, dim3(256), 0, st, G, in, n, out, ng); break;
        default: hipLaunchKernelGGL((arb_scan_compose_kernel<16, TIn>), grid, dim3(256), 0, st, G, in, n, out, ng); break;
    }
}
__global__ void arb_scan_top_kernel(arbscan::Grid G, const int64_t* in, int64_t n, int64_t* Eout) {
    if (blockIdx.x == 0 && threadIdx.x == 0) arbscan::scan_top_body(G, in, n, Eout);
}
template <typename TIn>
__global__ __launch_bounds__(256) void arb_scan_expand_kernel(arbscan::Grid G, const TIn* in, int64_t n, const int64_t* Ecoarse, int64_t* Efine, int64_t ng) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < ng) arbscan::scan_expand_body(G, in, n, Ecoarse, Efine, g);
}
__global__ __launch_bounds__(256) void arb_scan_finalize_kernel(arbscan::ScanArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < a.nb) arbscan::scan_finalize_body(a, b);
}

struct ScanLayout {
    std::vector<int64_t> n;      // elements per level: n[0] blocks, n[l+1] = ceil(n[l] / FAN); the last level is scanned serially
    std::vector<int64_t> woff;   // wide tables of level l >= 1 start at woff[l] (int64 elements)
    std::vector<int64_t> eoff;   // E of level l starts at eoff[l]
    int64_t wide_total = 0, e_total = 0;
};
ScanLayout scan_layout(int64_t nb, int R) {
    ScanLayout L;
    L.n.push_back(nb);
    do L.n.push_back(cdiv(L.n.back(), (int64_t)arbscan::FAN));
    while (L.n.back() > 1024);
    L.woff.assign(L.n.size(), 0);
    L.eoff.assign(L.n.size(), 0);
    for (size_t l = 0; l < L.n.size(); ++l) {
        L.eoff[l] = L.e_total;
        L.e_total += L.n[l];
        if (l >= 1) {
            L.woff[l] = L.wide_total;
            L.wide_total += L.n[l] * R;
        }
    }
    return L;
}

// One pass of the scan: tables -> up-sweep -> serial top -> down-sweep -> finalize.  device = false runs the same bodies in
// host loops (CPU tests of the arithmetic; the product path always passes true).
int scan_pass(const arbscan::ScanArgs& a, const ScanLayout& L, int64_t* wide, int64_t* Eall, bool device, hipStream_t st) {
    using namespace arbscan;
    const int nl = (int)L.n.size() - 1;   // top level
    const auto blocks = [](int64_t n) { return dim3((unsigned)cdiv(n, (int64_t)256)); };
    if (device) {
        switch (a.G.R) {   // table size 2^(J+1) as a template argument: the candidates stay in registers
            case 2: hipLaunchKernelGGL(arb_scan_tables_kernel<2>, blocks(a.nb), dim3(256), 0, st, a); break;
            case 4: hipLaunchKernelGGL(arb_scan_tables_kernel<4>, blocks(a.nb), dim3(256), 0, st, a); break;
            case 8: hipLaunchKernelGGL(arb_scan_tables_kernel<8>, blocks(a.nb), dim3(256), 0, st, a); break;
            default: hipLaunchKernelGGL(arb_scan_tables_kernel<16>, blocks(a.nb), dim3(256), 0, st, a); break;
        }
        launch_compose<int32_t>(a.G, (const int32_t*)a.t0, L.n[0], wide + L.woff[1], L.n[1], st);
        for (int l = 2; l <= nl; ++l)
            launch_compose<int64_t>(a.G, (const int64_t*)(wide + L.woff[l - 1]), L.n[l - 1], wide + L.woff[l], L.n[l], st);
        hipLaunchKernelGGL(arb_scan_top_kernel, dim3(1), dim3(64), 0, st, a.G, (const int64_t*)(wide + L.woff[nl]), L.n[nl], Eall + L.eoff[nl]);
        for (int l = nl; l >= 2; --l)
            hipLaunchKernelGGL(arb_scan_expand_kernel<int64_t>, blocks(L.n[l]), dim3(256), 0, st, a.G, (const int64_t*)(wide + L.woff[l - 1]), L.n[l - 1],
                               (const int64_t*)(Eall + L.eoff[l]), Eall + L.eoff[l - 1], L.n[l]);
        hipLaunchKernelGGL(arb_scan_expand_kernel<int32_t>, blocks(L.n[1]), dim3(256), 0, st, a.G, (const int32_t*)a.t0, L.n[0], (const int64_t*)(Eall + L.eoff[1]),
                           Eall + L.eoff[0], L.n[1]);
        hipLaunchKernelGGL(arb_scan_finalize_kernel, blocks(a.nb), dim3(256), 0, st, a);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    for (int64_t b = 0; b < a.nb; ++b) scan_tables_body<0>(a, b);
    for (int64_t g = 0; g < L.n[1]; ++g) scan_compose_body<0>(a.G, (const int32_t*)a.t0, L.n[0], wide + L.woff[1], g);
    for (int l = 2; l <= nl; ++l)
        for (int64_t g = 0; g < L.n[l]; ++g) scan_compose_body<0>(a.G, (const int64_t*)(wide + L.woff[l - 1]), L.n[l - 1], wide + L.woff[l], g);
    scan_top_body(a.G, wide + L.woff[nl], L.n[nl], Eall + L.eoff[nl]);
    for (int l = nl; l >= 2; --l)
        for (int64_t g = 0; g < L.n[l]; ++g) scan_expand_body(a.G, (const int64_t*)(wide + L.woff[l - 1]), L.n[l - 1], Eall + L.eoff[l], Eall + L.eoff[l - 1], g);
    for (int64_t g = 0; g < L.n[1]; ++g) scan_expand_body(a.G, (const int32_t*)a.t0, L.n[0], Eall + L.eoff[1], Eall + L.eoff[0], g);
    for (int64_t b = 0; b < a.nb; ++b) scan_finalize_body(a, b);
    return MDSP_OK;
}

// What the scan needs from the serial pilot: anchors of the first `pilot` outputs, the exact state of output `pilot`
// on the grid, the slope of the rounding drift, and how many blocks can still follow.
struct ScanSetup {
    arbscan::Grid G;
    std::vector<int64_t> ax;
    std::vector<double> aa;
    uint64_t As = 0;
    int64_t xs = 0, k0 = 0, nb = 0;
    double sigma = 0.0;
};
// false: not applicable (short stream, recurrence outside the integer model) -- the caller runs the serial loop
bool scan_setup(double acc, int64_t deficit, const ArbStep& st, int64_t nphi, int64_t xlen, int64_t pilot, ScanSetup& S) {
    using namespace arbscan;
    if (pilot < 2 * BLK || pilot % BLK) return false;
    if (!make_grid(st.delta, nphi, S.G)) return false;
    int64_t n = 0, xe = 0;
    double ae = 0.0;
    arb_trajectory(acc, deficit, st, xlen, ANCH, &S.ax, &S.aa, &n, &ae, &xe, pilot);
    if (n < pilot || xe > xlen) return false;   // the stream ends inside the pilot
    if (!to_grid(S.G, ae, S.As)) return false;
    S.xs = xe;
    S.k0 = pilot;
    // drift slope over outputs BLK .. pilot (both on the grid):  E = U(pilot) - U(BLK) - (pilot - BLK) D
    uint64_t A1 = 0;
    if (!to_grid(S.G, S.aa[BLK / ANCH], A1)) return false;
    const __int128 U1 = (__int128)A1 + (__int128)S.G.N * S.ax[BLK / ANCH], U0 = (__int128)S.As + (__int128)S.G.N * xe;
    const __int128 E = U0 - U1 - (__int128)(pilot - BLK) * (__int128)S.G.D;
    S.sigma = (double)E / (double)(pilot - BLK);
    // outputs that can follow output k0: xIdx first exceeds xlen after about ((xlen + 1 - xs) N - As) / D updates; two spare blocks
    const __int128 room = (__int128)(xlen + 1 - xe) * (__int128)S.G.N;
    const __int128 kmax = room / (__int128)S.G.D + 2;
    if (kmax > ((__int128)1 << 33)) return false;   // scan work space is ~40 B per 32 outputs: keep it within a few GiB, longer streams go serial
    S.nb = (int64_t)kmax / BLK + 2;
    return true;
}

// Host emulation of the whole scan (same integer bodies as the kernels), for the CPU tests.  Returns false when the caller
// has to fall back to the serial loop.
bool arb_scan_host(double acc, int64_t deficit, const ArbStep& st, int64_t nphi, int64_t xlen, int64_t pilot, std::vector<int64_t>& ax,
                   std::vector<double>& aa, int64_t* nout, double* acc_end, int64_t* xidx_end, int* passes) {
    using namespace arbscan;
    ScanSetup S;
    if (!scan_setup(acc, deficit, st, nphi, xlen, pilot, S)) return false;
    const ScanLayout L = scan_layout(S.nb, S.G.R);
    const int64_t nanch = S.k0 / ANCH + 2 * S.nb;
    ax = S.ax;
    aa = S.aa;
    ax.resize((size_t)nanch);
    aa.resize((size_t)nanch);
    std::vector<int32_t> t0((size_t)S.nb * S.G.R);
    std::vector<uint32_t> mind((size_t)S.nb);
    std::vector<int64_t> cb((size_t)S.nb), wide((size_t)L.wide_total), Eall((size_t)L.e_total), res(4, 0);
    ScanArgs a{};
    a.G = S.G;
    a.As = S.As;
    a.xs = S.xs;
    a.k0 = S.k0;
    a.xlen = xlen;
    a.nb = S.nb;
    a.sigma = S.sigma;
    a.t0 = t0.data();
    a.mind = mind.data();
    a.cb = cb.data();
    a.E = Eall.data() + L.eoff[0];
    a.baseA = reinterpret_cast<uint64_t*>(aa.data() + S.k0 / ANCH);
    a.baseW = ax.data() + S.k0 / ANCH;
    a.tab_x = ax.data();
    a.tab_acc = aa.data();
    a.result = res.data();
    for (int pass = 0; pass < 2; ++pass) {
        a.pass = pass;
        std::fill(res.begin(), res.end(), 0);
        scan_pass(a, L, wide.data(), Eall.data(), false, nullptr);
        if (passes) *passes = pass + 1;
        if (!(res[0] & 1)) break;
    }
    if ((res[0] & 1) || !(res[0] & 2)) return false;
    *nout = res[1];
    *xidx_end = res[2];
    std::memcpy(acc_end, &res[3], 8);
    ax.resize((size_t)cdiv(*nout, (int64_t)ANCH));
    aa.resize(ax.size());
    return true;
}

// Device scan for one call: pilot on the host, everything else on the stream; the anchors are written straight into the
// filter's device tables.  false: fall back to the serial loop (nothing the caller relies on has been modified).
int arb_scan_device(mdsp_firarb_s* f, const ArbStep& step, int64_t xlen, int64_t pilot, hipStream_t st, bool* used, int64_t* nout, double* acc_end,
                    int64_t* xidx_end) {
    using namespace arbscan;
    *used = false;
    ScanSetup S;
    if (!scan_setup(f->phi_acc, f->input_deficit, step, f->nphi, xlen, pilot, S)) return MDSP_OK;
    const ScanLayout L = scan_layout(S.nb, S.G.R);
    const int64_t nanch = S.k0 / ANCH + 2 * S.nb;
    MDSP_TRY(f->tab_x.reserve(sizeof(int64_t) * (size_t)nanch));
    MDSP_TRY(f->tab_acc.reserve(sizeof(double) * (size_t)nanch));
    MDSP_TRY(f->scan_t0.reserve(sizeof(int32_t) * (size_t)S.nb * S.G.R));
    MDSP_TRY(f->scan_mind.reserve(sizeof(uint32_t) * (size_t)S.nb));
    MDSP_TRY(f->scan_cb.reserve(sizeof(int64_t) * (size_t)S.nb));
    MDSP_TRY(f->scan_wide.reserve(sizeof(int64_t) * (size_t)L.wide_total));
    MDSP_TRY(f->scan_E.reserve(sizeof(int64_t) * (size_t)L.e_total));
    MDSP_TRY(f->scan_res.reserve(sizeof(int64_t) * 4));
    MDSP_HIP(hipStreamSynchronize(st));   // a previous launch on this stream may still read the anchor tables
    MDSP_HIP(hipMemcpy(f->tab_x.p, S.ax.data(), sizeof(int64_t) * S.ax.size(), hipMemcpyHostToDevice));
    MDSP_HIP(hipMemcpy(f->tab_acc.p, S.aa.data(), sizeof(double) * S.aa.size(), hipMemcpyHostToDevice));
    ScanArgs a{};
    a.G = S.G;
    a.As = S.As;
    a.xs = S.xs;
    a.k0 = S.k0;
    a.xlen = xlen;
    a.nb = S.nb;
    a.sigma = S.sigma;
    a.t0 = f->scan_t0.as<int32_t>();
    a.mind = f->scan_mind.as<uint32_t>();
    a.cb = f->scan_cb.as<int64_t>();
    a.E = f->scan_E.as<int64_t>() + L.eoff[0];
    a.baseA = reinterpret_cast<uint64_t*>(f->tab_acc.as<double>() + S.k0 / ANCH);
    a.baseW = f->tab_x.as<int64_t>() + S.k0 / ANCH;
    a.tab_x = f->tab_x.as<int64_t>();
    a.tab_acc = f->tab_acc.as<double>();
    a.result = f->scan_res.as<int64_t>();
    int64_t res[4] = {0, 0, 0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        a.pass = pass;
        MDSP_HIP(hipMemsetAsync(f->scan_res.p, 0, sizeof(res), st));
        MDSP_TRY(scan_pass(a, L, f->scan_wide.as<int64_t>(), f->scan_E.as<int64_t>(), true, st));
        MDSP_HIP(hipMemcpyAsync(res, f->scan_res.p, sizeof(res), hipMemcpyDeviceToHost, st));
        MDSP_HIP(hipStreamSynchronize(st));
        if (!(res[0] & 1)) break;
    }
    if ((res[0] & 1) || !(res[0] & 2)) return MDSP_OK;   // ambiguous twice, or no end found: serial loop
    *nout = res[1];
    *xidx_end = res[2];
    std::memcpy(acc_end, &res[3], 8);
    *used = true;
    return MDSP_OK;
}

// Every launch decision of the arbitrary-rate kernel, as pure host arithmetic: mdsp_firarb_exec launches with exactly what this returns,
// and mdsp_arb_kernel_geometry reports it (the tests assert on it which path a case runs).  real_bytes = sizeof(R) of the arithmetic,
// acc_bytes = sizeof(A) of one sample in it.
struct ArbGeometry {
    int tile;         // outputs per workgroup
    int64_t span;     // staged samples per tile and channel (0: the windows are read straight from global memory)
    int nchg;         // channels per group (the NCH instantiation: 4, 2 or 1)
    int64_t groups, tiles;
    unsigned gy;      // grid rows; gy < groups: a workgroup loops over several channel groups
    bool taps_in_lds;
    size_t lds_bytes;
};
ArbGeometry arb_geometry(int64_t tp, int64_t nphi, double delta, int64_t real_bytes, int64_t acc_bytes, int64_t nch, int64_t nout, int cu_count) {
    ArbGeometry g{};
    const int64_t taps_bytes = 2 * tp * nphi * real_bytes;
    g.taps_in_lds = taps_bytes <= 32 * 1024;
    const int nch_max = tunables().arb_nch;   // tuning knob
    // channels per group: the most whose workgroup (trajectory records + interleaved input span of tile * Delta / Nphi + tp
    // samples per channel + tap pairs) stays within 44 KiB of LDS, i.e. leaves >= 3 workgroups per CU; measured on MI355X,
    // larger footprints lose more to occupancy than the shared tap reads save
    int nchg = nch >= 3 ? 4 : (int)std::max<int64_t>(1, nch);
    nchg = std::min(nchg, nch_max >= 4 ? 4 : nch_max >= 2 ? 2 : 1);
    int tile = 1024;
    if (tunables().arb_tile > 0) tile = std::min(64 * ARB_BLK, std::max(ARB_BLK, tunables().arb_tile / ARB_BLK * ARB_BLK));   // tuning knob (one wave replays the tile)
    const int tile0 = tile;
    int64_t span = 0;
    const auto span_of = [&](int t) { return ((int64_t)std::ceil((double)t * delta / (double)nphi) + tp + 4 + 3) & ~int64_t(3); };   // multiple of 4: the tap pairs that follow stay 16-byte aligned
    const int64_t fixed = (int64_t)arb_rec_bytes(tile0) + (g.taps_in_lds ? taps_bytes : 0);
    span = span_of(tile);
    while (nchg > 1 && fixed + span * nchg * acc_bytes > 44 * 1024) nchg /= 2;
    if (nchg == 1) {   // one channel at a time: shrink the tile until its span fits 48 KiB
        while ((span = span_of(tile)) * acc_bytes > 48 * 1024 && tile > ARB_BLK) tile /= 2;
        if (span * acc_bytes > 48 * 1024) span = 0;   // very low rates: outputs are far apart, read through L2 instead
    }
    g.tile = tile;
    g.span = span;
    g.nchg = nchg;
    g.lds_bytes = arb_rec_bytes(tile) + (size_t)span * nchg * (size_t)acc_bytes + (g.taps_in_lds ? (size_t)taps_bytes : 0);
    // channels share a tile's replayed trajectory (and, NCH at a time, its tap reads): loop over the channel groups inside the
    // workgroup unless there are too few tiles to fill the GPU
    g.tiles = cdiv(nout, tile);
    g.groups = cdiv(nch, nchg);
    g.gy = (unsigned)std::min<int64_t>(g.groups, std::max<int64_t>(1, cdiv((int64_t)cu_count * 8, std::max<int64_t>(1, g.tiles))));
    return g;
}

template <typename XS, typename A, typename R, int NCH> int arb_launch_n(mdsp_firarb_s* f, ArbArgs& a, const ArbGeometry& g, hipStream_t st) {
    a.tile = g.tile;
    a.span = (int)g.span;
    const size_t lds_bytes = g.lds_bytes;
    auto kern = arbitrary_fir_kernel<XS, A, R, NCH>;
    if (lds_bytes > 48 * 1024) MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    const int64_t tiles = g.tiles;
    const unsigned gy = g.gy;
    const dim3 grid((unsigned)tiles, gy);
    const bool prof = MDSP_DBG(arb_prof) && gy == 1;
    if (prof) {
        MDSP_TRY(f->prof.reserve(sizeof(long long) * 8 * (size_t)tiles));
        MDSP_HIP(hipMemsetAsync(f->prof.p, 0, sizeof(long long) * 8 * (size_t)tiles, st));
        a.prof = f->prof.as<long long>();
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, st, a);
    MDSP_LAUNCH_CHECK();
    if (prof) {   // phase durations (shader clocks) averaged over the workgroups of the middle half of the launch
        std::vector<long long> h((size_t)tiles * 8);
        MDSP_HIP(hipStreamSynchronize(st));
        MDSP_HIP(hipMemcpy(h.data(), f->prof.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        double sum[5] = {0, 0, 0, 0, 0};
        int64_t n = 0;
        long long tmin = LLONG_MAX, tmax = 0;
        for (int64_t t = 0; t < tiles; ++t) {
            tmin = std::min(tmin, h[t * 8]);
            tmax = std::max(tmax, h[t * 8 + 5]);
        }
        for (int64_t t = tiles / 4; t < tiles * 3 / 4; ++t, ++n)
            for (int k = 0; k < 5; ++k) sum[k] += (double)(h[t * 8 + k + 1] - h[t * 8 + (k == 2 ? 1 : k)]);
        fprintf(stderr, "[MDSP_ARB_PROF] tiles %lld, kernel span %lld clk; per workgroup (clk): x_first load %.0f, replay(wave0) %.0f, prologue->barrier %.0f, compute %.0f, drain %.0f\n",
                (long long)tiles, tmax - tmin, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n);
    }
    return MDSP_OK;
}

template <typename XS, typename A, typename R> int arb_launch(mdsp_firarb_s* f, ArbArgs& a, hipStream_t st) {
    const ArbGeometry g = arb_geometry(f->base.tp, f->nphi, f->delta, (int64_t)sizeof(R), (int64_t)sizeof(A), f->base.nch, a.nout, device_cu_count());
    a.taps_in_lds = g.taps_in_lds;
    a.ablate = MDSP_DBG(ablate);
    a.prio = tunables().arb_prio;
    switch (g.nchg) {
        case 4: return arb_launch_n<XS, A, R, 4>(f, a, g, st);
        case 2: return arb_launch_n<XS, A, R, 2>(f, a, g, st);
        default: return arb_launch_n<XS, A, R, 1>(f, a, g, st);
    }
}

int arb_dispatch(mdsp_firarb_s* f, ArbArgs& a, hipStream_t st) {
    const bool d = f->base.acc_double;
    switch (f->base.x_dtype) {
        case MDSP_F32: return d ? arb_launch<float, double, double>(f, a, st) : arb_launch<float, float, float>(f, a, st);
        case MDSP_F64: return arb_launch<double, double, double>(f, a, st);
        case MDSP_C32: return d ? arb_launch<cx<float>, cx<double>, double>(f, a, st) : arb_launch<cx<float>, cx<float>, float>(f, a, st);
        default: return arb_launch<cx<double>, cx<double>, double>(f, a, st);
    }
}

// (at least 16 bytes, zeroed: the arbitrary-rate kernel's tap copy loads the table in 16-byte units, and one Float32 pair is 8)
int upload_bank(DevBuf& buf, const std::vector<double>& pd, bool as_double) {
    const size_t bytes = (as_double ? sizeof(double) : sizeof(float)) * pd.size();
    MDSP_TRY(buf.reserve(std::max<size_t>(16, bytes)));
    if (bytes < 16) MDSP_HIP(hipMemset(buf.p, 0, 16));
    if (as_double) {
        MDSP_HIP(hipMemcpy(buf.p, pd.data(), bytes, hipMemcpyHostToDevice));
    } else {
        std::vector<float> pf(pd.size());
        for (size_t i = 0; i < pd.size(); ++i) pf[i] = (float)pd[i];
        MDSP_HIP(hipMemcpy(buf.p, pf.data(), bytes, hipMemcpyHostToDevice));
    }
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_arb_trajectory(double phi_acc, int64_t input_deficit, double rate, int64_t nphi, int64_t xlen, int64_t block, int64_t* anchors_x,
                        double* anchors_acc, int64_t anchors_cap, int64_t* nout, double* phi_acc_end, int64_t* input_deficit_end) {
    if (!(rate > 0.0) || nphi < 1 || xlen < 0 || input_deficit < 1 || block < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid trajectory arguments");
    if (!nout || !phi_acc_end || !input_deficit_end) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL result pointer");
    if (xlen < input_deficit) {   // stream_filt.jl:586-590
        *nout = 0;
        *phi_acc_end = phi_acc;
        *input_deficit_end = input_deficit - xlen;
        return MDSP_OK;
    }
    const double delta = (double)nphi / rate;
    const ArbStep st = ArbStep::make(delta, (double)nphi);
    std::vector<int64_t> ax;
    std::vector<double> aa;
    int64_t xe = 0;
    arb_trajectory(phi_acc, input_deficit, st, xlen, block, anchors_x ? &ax : nullptr, anchors_x ? &aa : nullptr, nout, phi_acc_end, &xe);
    *input_deficit_end = xe - xlen;
    if (anchors_x) {
        if ((int64_t)ax.size() > anchors_cap || !anchors_acc) MDSP_FAIL(MDSP_ERR_ARGUMENT, "anchor buffers too small: need %lld", (long long)ax.size());
        std::copy(ax.begin(), ax.end(), anchors_x);
        std::copy(aa.begin(), aa.end(), anchors_acc);
    }
    return MDSP_OK;
}

// Host emulation of the device's parallel trajectory scan (same integer code, arb_scan.h): for the CPU tests.  *used = 0
// when the scan does not apply (short stream, recurrence outside the integer model, ambiguous twice) -- the product then
// runs the serial loop, and so should the caller.
int mdsp_arb_trajectory_scan(double phi_acc, int64_t input_deficit, double rate, int64_t nphi, int64_t xlen, int64_t pilot, int64_t* anchors_x,
                             double* anchors_acc, int64_t anchors_cap, int64_t* nout, double* phi_acc_end, int64_t* input_deficit_end, int* used,
                             int* passes) {
    if (!(rate > 0.0) || nphi < 1 || xlen < 0 || input_deficit < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid trajectory arguments");
    if (!nout || !phi_acc_end || !input_deficit_end || !used) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL result pointer");
    *used = 0;
    if (xlen < input_deficit) return MDSP_OK;
    const double delta = (double)nphi / rate;
    const ArbStep st = ArbStep::make(delta, (double)nphi);
    std::vector<int64_t> ax;
    std::vector<double> aa;
    int64_t xe = 0;
    if (!arb_scan_host(phi_acc, input_deficit, st, nphi, xlen, pilot, ax, aa, nout, phi_acc_end, &xe, passes)) return MDSP_OK;
    *input_deficit_end = xe - xlen;
    if (anchors_x) {
        if ((int64_t)ax.size() > anchors_cap || !anchors_acc) MDSP_FAIL(MDSP_ERR_ARGUMENT, "anchor buffers too small: need %lld", (long long)ax.size());
        std::copy(ax.begin(), ax.end(), anchors_x);
        std::copy(aa.begin(), aa.end(), anchors_acc);
    }
    *used = 1;
    return MDSP_OK;
}

// Test helper: number of updates (out of nsteps from phi_acc) at which the branch-free update of the device replay
// (ArbStep::fast) differs from the reference-form update (ArbStep::operator()) in phase or in index increment.
int mdsp_arb_replay_check(double phi_acc, double rate, int64_t nphi, int64_t nsteps, int64_t* mismatches) {
    if (!(rate > 0.0) || nphi < 1 || nsteps < 0 || !mismatches) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid arguments");
    const ArbStep st = ArbStep::make((double)nphi / rate, (double)nphi);
    double a1 = phi_acc, a2 = phi_acc;
    int64_t x1 = 0, x2 = 0, bad = 0;
    for (int64_t k = 0; k < nsteps; ++k) {
        st(a1, x1);
        st.fast(a2, x2);
        if (a1 != a2 || x1 != x2) {
            ++bad;
            a2 = a1;
            x2 = x1;
        }
    }
    *mismatches = bad;
    return MDSP_OK;
}

int mdsp_arb_kernel_geometry(int64_t taps_per_phase, int64_t nphi, double rate, int taps_dtype, int x_dtype, int64_t nch, int64_t nout, int cu_count,
                             int64_t out8[8]) {
    if (taps_per_phase < 1 || taps_per_phase > (int64_t(1) << 30) || nphi < 1 || nphi > (int64_t(1) << 20) || !(rate > 0.0) || nch < 1 || nch > 65535 || nout < 0)
        MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid geometry arguments");
    if (taps_dtype != MDSP_F32 && taps_dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "FIRArbitrary takes real Float32/Float64 taps only");
    if (!dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid x dtype");
    if (!out8) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL result pointer");
    const bool dbl = (taps_dtype == MDSP_F64) || dtype_is_double(x_dtype);   // the arithmetic mdsp_firarb_create chooses
    const int64_t rb = dbl ? 8 : 4, ab = dtype_is_complex(x_dtype) ? 2 * rb : rb;
    const ArbGeometry g = arb_geometry(taps_per_phase, nphi, (double)nphi / rate, rb, ab, nch, nout, cu_count > 0 ? cu_count : device_cu_count());
    const int64_t o[8] = {g.tile, g.span, g.nchg, g.groups, g.tiles, (int64_t)g.gy, g.taps_in_lds ? 1 : 0, (int64_t)g.lds_bytes};
    std::copy(o, o + 8, out8);
    return MDSP_OK;
}

int mdsp_firarb_scan_stats(mdsp_firarb f, int64_t* scanned, int64_t* serial) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (scanned) *scanned = f->n_scanned;
    if (serial) *serial = f->n_serial;
    return MDSP_OK;
}

int mdsp_firarb_create(mdsp_firarb* fo, const void* taps_host, int64_t hlen, double rate, int64_t nphi, int taps_dtype, int x_dtype, int64_t nch) {
    if (!fo) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle pointer is NULL");
    *fo = nullptr;
    if (!(rate > 0.0)) MDSP_FAIL(MDSP_ERR_DOMAIN, "rate must be greater than 0");          // stream_filt.jl:151
    if (!taps_host || hlen < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "filter taps must be non-empty");
    if (nphi < 1 || nphi > (int64_t(1) << 20)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "Nphi must be in [1, 2^20]");
    if (taps_dtype != MDSP_F32 && taps_dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "FIRArbitrary takes real Float32/Float64 taps only (complex taps: integer and rational ratios)");
    if (!dtype_valid(x_dtype)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid x dtype");
    if (nch < 1 || nch > 65535) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nch must be in [1, 65535]");
    std::unique_ptr<mdsp_firarb_s> f(new mdsp_firarb_s());
    mdsp_fir_s& b = f->base;
    b.kind = 4;
    b.L = nphi;
    b.M = 1;
    b.hlen = hlen;
    b.nch = nch;
    b.taps_dtype = taps_dtype;
    b.x_dtype = x_dtype;
    b.tp = cdiv(hlen, nphi);
    b.hl = b.tp - 1;
    b.acc_double = (taps_dtype == MDSP_F64) || dtype_is_double(x_dtype);
    b.out_dtype = dtype_is_complex(x_dtype) ? (b.acc_double ? MDSP_C64 : MDSP_C32) : (b.acc_double ? MDSP_F64 : MDSP_F32);
    f->rate = rate;
    f->nphi = nphi;
    f->delta = (double)nphi / rate;                                                         // :114
    // dh = [diff(h); 0] in the taps' own precision (:107), both banks through taps2pfb (:108-109, :294-307)
    const size_t np = (size_t)(b.tp * nphi);
    std::vector<double> pd(np, 0.0), dd(np, 0.0);
    auto tap = [&](int64_t i) -> double { return taps_dtype == MDSP_F32 ? (double)((const float*)taps_host)[i] : ((const double*)taps_host)[i]; };
    auto dtap = [&](int64_t i) -> double {
        if (i + 1 >= hlen) return 0.0;
        if (taps_dtype == MDSP_F32) return (double)(((const float*)taps_host)[i + 1] - ((const float*)taps_host)[i]);
        return ((const double*)taps_host)[i + 1] - ((const double*)taps_host)[i];
    };
    for (int64_t row = 0; row < b.tp; ++row)
        for (int64_t col = 0; col < nphi; ++col) {
            const int64_t hidx = (b.tp - 1 - row) * nphi + col;
            if (hidx < hlen) {
                pd[(size_t)(row * nphi + col)] = tap(hidx);
                dd[(size_t)(row * nphi + col)] = dtap(hidx);
            }
        }
    std::vector<double> both(2 * np);
    for (size_t i = 0; i < np; ++i) {
        both[2 * i] = pd[i];
        both[2 * i + 1] = dd[i];
    }
    MDSP_TRY(upload_bank(b.pfbT, both, b.acc_double));   // interleaved (pfb, dpfb) pairs
    const size_t hbytes = dtype_size(x_dtype) * (size_t)std::max<int64_t>(1, b.hl) * (size_t)nch;
    for (int k = 0; k < 2; ++k) {
        MDSP_TRY(b.hist[k].reserve(hbytes));
        MDSP_HIP(hipMemset(b.hist[k].p, 0, hbytes));
    }
    *fo = f.release();
    return MDSP_OK;
}

int mdsp_firarb_destroy(mdsp_firarb f) {
    delete f;
    return MDSP_OK;
}

int mdsp_firarb_reset(mdsp_firarb f) {   // reset! stream_filt.jl:260-276
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    const mdsp_fir_s& b = f->base;
    MDSP_HIP(hipMemset(b.hist[b.cur].p, 0, dtype_size(b.x_dtype) * (size_t)std::max<int64_t>(1, b.hl) * (size_t)b.nch));
    f->phi_acc = 0.0;
    f->input_deficit = 1;
    f->x_idx = 1;
    return MDSP_OK;
}

int mdsp_firarb_setphase(mdsp_firarb f, double phi) {   // setphase! :231-239
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (!(phi >= 0)) MDSP_FAIL(MDSP_ERR_DOMAIN, "phi must be >= 0");
    double whole = 0.0;
    const double frac = std::modf(phi, &whole);
    f->input_deficit += round_half_even(whole);
    f->phi_acc = frac * (double)f->nphi;
    return MDSP_OK;
}

int mdsp_firarb_timedelay(mdsp_firarb f, double* tau) {   // :400-401
    if (!f || !tau) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    *tau = (double)(f->base.hlen - 1) / (double)(2 * f->nphi);
    return MDSP_OK;
}

int mdsp_firarb_outputlength(mdsp_firarb f, int64_t inputlength, int64_t* outlen) {   // :340-342
    if (!f || !outlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    const double a = (double)(inputlength - f->input_deficit + 1) * f->rate;   // separate statements: no contraction
    const double b = f->phi_acc / f->delta;
    const double c = a - b;
    *outlen = (int64_t)std::ceil(c);
    return MDSP_OK;
}

int mdsp_firarb_inputlength(mdsp_firarb f, int64_t outputlength, int round_up, int64_t* inlen) {   // :385-389
    if (!f || !inlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL argument");
    const int64_t d = round_up ? 1 : 0;
    const double b = f->phi_acc / f->delta;
    const double s = (double)(outputlength - d) + b;
    const double q = s / f->rate;
    *inlen = (int64_t)std::floor(q) + d + f->input_deficit - 1;
    return MDSP_OK;
}

int mdsp_firarb_info(mdsp_firarb f, int64_t* nphi, int64_t* taps_per_phase, int64_t* history_len, int* out_dtype, double* delta) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (nphi) *nphi = f->nphi;
    if (taps_per_phase) *taps_per_phase = f->base.tp;
    if (history_len) *history_len = f->base.hl;
    if (out_dtype) *out_dtype = f->base.out_dtype;
    if (delta) *delta = f->delta;
    return MDSP_OK;
}

int mdsp_firarb_get_state(mdsp_firarb f, double* phi_acc, double* alpha, int64_t* phi_idx, int64_t* input_deficit, int64_t* x_idx,
                          void* history_host) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    const double fl = std::floor(f->phi_acc);
    if (phi_acc) *phi_acc = f->phi_acc;
    if (alpha) *alpha = f->phi_acc - fl;               // modf(phiAcc)[1]  (:576, :238)
    if (phi_idx) *phi_idx = 1 + (int64_t)fl;           // 1 + Int(foffset) (:577, :237)
    if (input_deficit) *input_deficit = f->input_deficit;
    if (x_idx) *x_idx = f->x_idx;
    const mdsp_fir_s& b = f->base;
    if (history_host && b.hl > 0) {
        MDSP_HIP(hipDeviceSynchronize());
        MDSP_HIP(hipMemcpy(history_host, b.hist[b.cur].p, dtype_size(b.x_dtype) * (size_t)b.hl * (size_t)b.nch, hipMemcpyDeviceToHost));
    }
    return MDSP_OK;
}

int mdsp_firarb_set_state(mdsp_firarb f, double phi_acc, int64_t input_deficit, const void* history_host) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (!(phi_acc >= 0.0) || !(phi_acc < (double)f->nphi) || input_deficit < 1) MDSP_FAIL(MDSP_ERR_ARGUMENT, "state out of range");
    f->phi_acc = phi_acc;
    f->input_deficit = input_deficit;
    const mdsp_fir_s& b = f->base;
    if (history_host && b.hl > 0) {
        MDSP_HIP(hipDeviceSynchronize());
        MDSP_HIP(hipMemcpy(b.hist[b.cur].p, history_host, dtype_size(b.x_dtype) * (size_t)b.hl * (size_t)b.nch, hipMemcpyHostToDevice));
    }
    return MDSP_OK;
}

int mdsp_firarb_exec(mdsp_firarb f, const void* x_dev, int64_t xlen, int64_t ldx, void* y_dev, int64_t ycap, int64_t ldy, int64_t* nwritten,
                     void* stream) {
    if (!f) MDSP_FAIL(MDSP_ERR_ARGUMENT, "handle is NULL");
    if (xlen < 0 || ycap < 0) MDSP_FAIL(MDSP_ERR_ARGUMENT, "negative size");
    mdsp_fir_s& b = f->base;
    if (b.nch > 1 && ldx < xlen) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldx smaller than xlen");
    hipStream_t st = as_stream(stream);
    if (nwritten) *nwritten = 0;
    if (xlen < f->input_deficit) {   // stream_filt.jl:586-590
        MDSP_TRY(shiftin_dispatch(&b, x_dev, xlen, ldx, st));
        f->input_deficit -= xlen;
        return MDSP_OK;
    }
    const ArbStep step = ArbStep::make(f->delta, (double)f->nphi);
    const bool hit = f->cache_valid && f->c_acc0 == f->phi_acc && f->c_def0 == f->input_deficit && f->c_xlen == xlen;
    if (!hit) {
        int64_t nout = 0, xe = 0;
        double ae = 0.0;
        bool scanned = false;
        f->cache_valid = false;
        // long streams: the recurrence is evaluated in parallel on the device, bit for bit (arb_scan.h); MDSP_ARB_SCAN=0 and
        // MDSP_ARB_SCAN_MIN (outputs) are test / tuning knobs
        const int64_t scan_min = tunables().arb_scan_min;
        const int64_t pilot = std::min<int64_t>(65536, std::max<int64_t>(2 * arbscan::BLK, (scan_min / 4) & ~int64_t(arbscan::BLK - 1)));
        if (tunables().arb_scan != 0 && (double)xlen * f->rate >= (double)scan_min)
            MDSP_TRY(arb_scan_device(f, step, xlen, pilot, st, &scanned, &nout, &ae, &xe));
        if (scanned) {
            ++f->n_scanned;
        } else {
            std::vector<int64_t> ax;
            std::vector<double> aa;
            ax.reserve((size_t)((double)xlen * f->rate / ARB_BLK) + 16);
            aa.reserve(ax.capacity());
            arb_trajectory(f->phi_acc, f->input_deficit, step, xlen, ARB_BLK, &ax, &aa, &nout, &ae, &xe);
            MDSP_TRY(f->tab_x.reserve(sizeof(int64_t) * std::max<size_t>(1, ax.size())));
            MDSP_TRY(f->tab_acc.reserve(sizeof(double) * std::max<size_t>(1, aa.size())));
            MDSP_HIP(hipStreamSynchronize(st));   // a previous launch on this stream may still read the anchor tables
            if (!ax.empty()) {
                MDSP_HIP(hipMemcpy(f->tab_x.p, ax.data(), sizeof(int64_t) * ax.size(), hipMemcpyHostToDevice));
                MDSP_HIP(hipMemcpy(f->tab_acc.p, aa.data(), sizeof(double) * aa.size(), hipMemcpyHostToDevice));
            }
            ++f->n_serial;
        }
        f->c_acc0 = f->phi_acc;
        f->c_def0 = f->input_deficit;
        f->c_xlen = xlen;
        f->c_nout = nout;
        f->c_acc_end = ae;
        f->c_xidx_end = xe;
        f->c_def_end = xe - xlen;
        f->cache_valid = true;
    }
    const int64_t nout = f->c_nout;
    // the reference indexes buffer[bufIdx] unchecked beyond allocate_output's outputlength + 1 (:639-655): a short
    // buffer is a BoundsError there, an ArgumentError here -- raised before anything is written
    if (ycap < nout) MDSP_FAIL(MDSP_ERR_ARGUMENT, "buffer is too small: need %lld, have %lld", (long long)nout, (long long)ycap);
    if (b.nch > 1 && ldy < nout) MDSP_FAIL(MDSP_ERR_ARGUMENT, "ldy smaller than the output length");
    if (nout > 0) {
        if (!x_dev || !y_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
        ArbArgs a{};
        a.x = x_dev;
        a.hist = b.hist[b.cur].p;
        a.y = y_dev;
        a.taps2 = b.pfbT.p;
        a.nch = b.nch;
        a.tab_x = f->tab_x.as<int64_t>();
        a.tab_acc = f->tab_acc.as<double>();
        a.xlen = xlen;
        a.ldx = ldx;
        a.ldy = ldy;
        a.nout = nout;
        a.step = step;
        a.nphi = (int)f->nphi;
        a.tp = (int)b.tp;
        a.hl = (int)b.hl;
        MDSP_TRY(arb_dispatch(f, a, st));
    }
    f->phi_acc = f->c_acc_end;
    f->x_idx = f->c_xidx_end;
    f->input_deficit = f->c_def_end;                                       // :619
    MDSP_TRY(shiftin_dispatch(&b, x_dev, xlen, ldx, st));                  // :620
    if (nwritten) *nwritten = nout;
    return MDSP_OK;
}

}  // extern "C"
