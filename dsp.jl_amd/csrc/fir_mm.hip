// Matrix-core polyphase kernel (fir_mm.h): the polyphase bank as the B operand of v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (Float32 taps on Float32 /
// ComplexF32 signals, Float64 arithmetic on Float64 / ComplexF64 signals; any ratio with L <= 1024 and filters of any length).
//
// The Float32 register-tap kernel (fir.hip, polyphase_fast_kernel) is bound by the LDS and the vector ALU: P = 2 residues share one window (16.5 ds_read_b32 and
// 16.5 v_pk_fma_f32 per output; 68 % LDS-array busy, the packed FMAs at 8 - 10 clocks each between their LDS reads against 4.4 in
// isolation), more residues per thread cost VGPRs and occupancy (P = 4: 228 VGPRs, slower) -- 2.5 ms on BASELINE config 5 against an
// HBM floor of 1.6 - 1.9.
// Outputs of the same residue s in different rounds q share their taps, and neighbouring residues read windows that start delta_j =
// c_{s0+j} - c_{s0} <= j samples apart: for 16 rounds x 16 residues,
//      Y[q][j] = sum_k  X[q][k] * H[k][j],    X[q][k] = z[q M + c_{s0} + k],    H[k][j] = pfb[phase_j][k - delta_j]  (0 outside the bank)
// is a (16 x K)(K x 16) product with K = tp + delta_15 -- what the f32 matrix instruction computes, four k per issue: 1024 multiply-adds
// per operand read from LDS, at the vector unit's peak FMA rate, and with the VALU left free.  Its arithmetic is bit for bit a k-ordered
// fmaf chain (one rounding per product, no wider accumulator: verified bit for bit against the register-tap kernel, tests/test_gpu_boundary.py), i.e. exactly the oldest-sample-first chain of the
// register-tap kernel: the zero taps add exact zeros and the two kernels agree bit for bit (tests/test_gpu_boundary.py).
// This is not a GEMM reshaping of the problem: no operand is materialised or reordered in memory, X is the staged signal tile
// itself (lane l reads z[(q0 + l%16) M + c + 4 t + l/16], one ds_read_b32 per MFMA), H lives in T VGPRs per wave for the whole
// kernel (lane l: tap k = 4 t + l/16 of residue j = l%16), and the roofline that bounds the kernel stays HBM.
//   tile   = 64 rounds = 64 M input samples + the window tail, staged in LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no VGPRs, no
//            ds_write pass); its 64 L outputs go through an LDS output buffer (row pitch 16 NB + 4) and leave as one contiguous
//            run of 16-byte stores
//   waves  = NB multiplying waves (one block of 16 residues each, the 64 rounds as four independent accumulators), then nd waves
//            that only issue the DMA of the next tile and ns waves that only store the previous tile's outputs: the memory
//            waves work through the whole tile period beside the MFMAs, one s_barrier per tile
//   LDS    = two sample buffers + two output buffers (config 5: 2 x 38 KiB + 2 x 41 KiB = 158 KiB, one workgroup of 16 waves per CU)
// Variations, all chosen by fir_mm_geo(): for L < 16 a row of the product is RB whole rounds (RB L <= 16 consecutive outputs, RB M
// samples) and several groups of rows share a tile; 2 or 1 chunks of 16 rows per wave when the tile would not fit; rows staged one by
// one (padded pitch) when their sample stride is bank-hostile; taps fetched from L2 per tile when they do not fit registers (long
// filters, or several column blocks per wave for L > 192).
// Measured on BASELINE config 5 (4 ch x 2^28, 160//147, 5120 taps): 1.86 ms = 4.8 TB/s of algorithmic traffic, the device-copy
// rate of this GPU, against 2.4 - 2.5 ms for the register-tap kernel (profiles/r02q_*); other ratios and types: DESIGN.md section 4.6.
#include "fir_mm.h"

#include <algorithm>
#include <atomic>
#include <numeric>

#include "fir_op.h"

using namespace mdsp;

namespace {

struct FirMArgs {
    const void* x;               // (xlen, nch) samples: R or (R, R) pairs
    const void* hist;
    void* y;
    const void* pfbT;            // tp * L taps of type R
    int64_t xlen, ldx, ldy, nout;
    int64_t nrows;               // rows of Lr outputs in this call: ceil(nout / Lr)
    int64_t d0;
    int L, M, hl, tp;            // the filter's ratio L // M
    int Lr, Mr;                  // a ROW = RB rounds = Lr = RB L consecutive outputs, Mr = RB M input samples (RB = 1 when L >= 16)
    int NB, NG;                  // blocks of 16 columns (outputs of a row); groups of 16 CH rows per tile
    int NBW;                     // multiplying waves per row group: wave w takes the column blocks w % NBW, w % NBW + NBW, .. (more than one only with T = 0)
    int Lp;                      // row pitch of the output buffer in LDS (R elements): Lr CS when NB = 1 (contiguous outputs), else 16 NB CS + 16 bytes
    int bufsz;                   // dwords per LDS sample buffer (two of them, then two output buffers)
    int steps;                   // k-steps of four taps when they do not fit registers (template T = 0): the taps are then fetched per tile
    int pitch;                   // 0: the samples of a tile are staged as one run (row r starts at r Mr); else every row is staged on its own, pitch dwords apart
    int rowpad;                  // > 0 (with pitch == 0): one run per tile, staged in the same 256-dword DMA granules as the plain run, with rowpad dwords of
                                 // padding behind every granule (dword d of the tile sits at d + (d / 256) rowpad): rows whose stride is bank-hostile spread
                                 // over the banks without the duplicated window tails of the row-staged form
    int memprio;                 // 1: the DMA and store waves run at raised priority (s_setprio)
    int vstore;                  // 1: output rows that are not whole vectors leave as gathered wide stores (0: element by element, round 2)
    int ablate;                  // MDSP_DEBUG_KNOBS builds (MDSP_ABLATE): 1 no tile DMA after the first, 2 no matrix products, 4 no output stores
    int nd, ns;                  // waves that issue the LDS-DMA / that store, after the multiplying waves
    unsigned lmagic, rmagic;     // ceil(2^32 / L), ceil(2^32 / (Lr CS)): quotients of small numbers by multiply-high
    int phi0m1;                  // phi0 - 1: output j of a row has phase (phi0-1 + j M) mod L and window start (phi0-1 + j M) div L
};

#ifndef MDSP_FIR_TAP_CARRY
#define MDSP_FIR_TAP_CARRY 1   // long-filter mode, ComplexF64: fetched taps carried raw into the next group of k-steps (0: masked next to the fetch)
#endif
typedef int mm_i4 __attribute__((ext_vector_type(4)));
// 64 consecutive dwords of a raw buffer straight into LDS (no VGPRs, no ds_write pass): lane l moves the dword at byte offset voff
// to lds_byte + 4 l.  Issued by hand: the compiler's wait-count bookkeeping makes every later ds_read wait for a DMA it knows of
// (it cannot tell the two tile buffers apart), which would serialise the next tile's loads with this tile's products.  M0 carries
// the LDS address and is the compiler's to use, so it is saved and restored inside the statement.
__device__ __forceinline__ void mm_dma64(mm_i4 rsrc, unsigned lds_byte, int voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dword %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_byte), "v"(voff), "s"(rsrc) : "memory");
}
// 256 consecutive dwords, 16 bytes per lane (lane l: byte offset voff -> lds_byte + 16 l).  A 16-byte access that crosses the end of
// the buffer is dropped whole, so the caller uses this form only for granules that lie inside the signal.
__device__ __forceinline__ void mm_dma256(mm_i4 rsrc, unsigned lds_byte, int voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_byte), "v"(voff), "s"(rsrc) : "memory");
}
__device__ __forceinline__ mm_i4 mm_rsrc(const void* base, long long bytes) {   // raw buffer: zero fill past `bytes`
    const unsigned long long p = (unsigned long long)base;
    const long long nb = bytes < 0 ? 0 : (bytes > 0x7ffffff0ll ? 0x7ffffff0ll : bytes);
    return mm_i4{(int)__builtin_amdgcn_readfirstlane((unsigned)p), (int)(__builtin_amdgcn_readfirstlane((unsigned)(p >> 32)) & 0xffffu),
                 (int)__builtin_amdgcn_readfirstlane((unsigned)nb), 0x00020000};
}
// the matrix instruction per element type: D (16 x 16) += A (16 x 4) B (4 x 16); lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16]
template <typename R> struct Mm;
template <> struct Mm<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lk, int r) { return 4 * lk + r; }   // D register r of lane l: row 4 (l / 16) + r, column l % 16
};
template <> struct Mm<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lk, int r) { return lk + 4 * r; }   // D register r of lane l: row (l / 16) + 4 r, column l % 16
};

// R: Float32 / Float64 arithmetic (signal and taps of that type); CS: 1 real signal, 2 complex signal (interleaved pairs: the two parts
// are two products against the same taps); CH: 16-row chunks per multiplying wave (independent accumulators); T: k-steps of four taps
// RP: padded runs (a separate instantiation: the two forms of the product loop in one function cost the plain form 20 - 70 VGPRs)
// NBLK > 1: a multiplying wave owns NBLK column blocks (L > 192) with the taps of ALL of them in registers (T k-steps each)
template <typename R, int CS, int CH, int T, bool RP = false, int NBLK = 1>
__device__ __forceinline__ void polyphase_mfma_body(const FirMArgs& a) {
    typedef typename Mm<R>::acc_t acc_t;
    constexpr int DW = (int)(sizeof(R) / 4) * CS;   // dwords per sample
    constexpr int VW = 16 / (int)sizeof(R);         // R elements per 16-byte store
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R* zs = reinterpret_cast<R*>(smem);            // two sample buffers of bufsz dwords, then two output buffers [Q][Lp]
    const int Q = 16 * CH * a.NG;                  // rows per tile
    const int64_t ch = blockIdx.y;
    const R* xc = static_cast<const R*>(a.x) + ch * a.ldx * CS;
    const R* hc = static_cast<const R*>(a.hist) + ch * (int64_t)a.hl * CS;
    R* yc = static_cast<R*>(a.y) + ch * a.ldy * CS;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int lj = lane & 15, lk = lane >> 4;
    // Wave roles: the first NB NG waves multiply (wave w: column block w % NB, rows 16 CH (w / NB) ..), the next nd waves issue the
    // LDS-DMA of the samples, the last ns waves store the outputs.  The memory waves work through the whole tile period beside the
    // MFMAs -- a wave that first moved data and then multiplied would hold up its SIMD's matrix pipe (measured: 2 000 - 6 000 clocks
    // of DMA issue / store issue per tile, against 4 600 of MFMA) -- and no wave waits on a vmcnt that mixes loads with younger stores.
    const int ncomp = a.NBW * a.NG;
    const bool is_comp = wave < ncomp, is_dma = wave >= ncomp && wave < ncomp + a.nd, is_store = wave >= ncomp + a.nd;
    const int wb0 = wave % a.NBW, wg = wave / a.NBW;
    if (!is_comp && a.memprio) __builtin_amdgcn_s_setprio(3);   // the memory waves' few instructions go first: a late DMA or store holds the whole tile up
    // H: this wave's taps, in registers for the whole kernel (T k-steps) -- or, for filters too long for that (T = 0), fetched from the
    // bank in L2 for every tile (a dword per lane and k-step, beside the four to eight MFMAs it feeds)
    constexpr int TR = T ? T : 1;
    const int steps = T ? T : a.steps;
    R hreg[NBLK][TR];
    int wb = wb0, c0 = 0, tap_phase = 0, tap_delta = 0;
    bool tap_valid = false;
    const R* pf = static_cast<const R*>(a.pfbT);
    const auto block_setup = [&](int b) {   // window start of column block b and this lane's column of it
        wb = b;
        const int s0 = 16 * b, sj = s0 + lj;
        const unsigned p0 = (unsigned)(a.phi0m1 + s0 * a.M), pj = (unsigned)(a.phi0m1 + sj * a.M);
        c0 = a.L == 1 ? (int)p0 : (int)__umulhi(p0, a.lmagic);   // (ceil(2^32 / 1) does not fit the magic)
        const int cj = a.L == 1 ? (int)pj : (int)__umulhi(pj, a.lmagic);
        tap_phase = (int)pj - cj * a.L;
        tap_delta = cj - c0;
        tap_valid = sj < a.Lr;
    };
    if (is_comp) block_setup(wb0);
    const auto tap = [&](int t) -> R {   // H[k = 4 t + lane / 16][j = lane % 16]
        const int i = 4 * t + lk - tap_delta;
        const bool ok = tap_valid && i >= 0 && i < a.tp;
        // branch-free: lanes without a tap read the bank's first entry and discard it -- a skipped load is an exec-masked branch per fetch,
        // and the long-filter mode's eight fetches in flight then come out one by one with a wait between them
        const R v = pf[ok ? (int64_t)i * a.L + tap_phase : (int64_t)0];
        return ok ? v : (R)0;
    };
#pragma unroll
    for (int kb = 0; kb < NBLK; ++kb) {
        if (NBLK > 1 && is_comp && wb0 + kb * a.NBW < a.NB) block_setup(wb0 + kb * a.NBW);
#pragma unroll
        for (int t = 0; t < TR; ++t) hreg[kb][t] = (T && is_comp && wb0 + kb * a.NBW < a.NB) ? tap(t) : (R)0;
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): the taps are in (their first use must not look like a pending load inside the tile loop)
    const int64_t cbase = a.d0 - 1;
    const int wtail = 4 * steps + 4;   // samples read past a window start
    const int64_t ntiles = (a.nrows + Q - 1) / Q;
    // Software pipeline over tiles with ONE barrier per tile.  LDS holds two sample buffers and two output buffers; in iteration t
    //   sample buffer t+1 receives the NEXT tile by LDS-DMA (no registers, no ds_write pass), issued right after the barrier;
    //   sample buffer t   feeds the products, and every multiplying wave writes its outputs into output buffer t as soon as its
    //                     own MFMAs are done (nobody else touches those rows and columns);
    //   output buffer t-1 leaves as coalesced stores.
    // The first tile(s), which straddle the history, are filled by ordinary loads (all waves).
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) R*)zs;
    const auto dma_ok = [&](int64_t tile) { return tile < ntiles && tile * Q * a.Mr + cbase >= a.hl; };
    // Row-staged tiles (pitch != 0): when the sample stride of a row, Mr, is a multiple of 8 the 16 rows of an A operand would sit on
    // 2 - 8 banks of a linear tile (147//160: all on one); every row is then DMA-ed on its own -- its Mr samples and the window tail
    // again -- to rows pitch = 256 g + 4 dwords apart (two-way conflicts at worst); the duplicates come from L2.  (Round 3: where a window is
    // shorter than a granule the padded run -- rowpad, below -- replaces this form.)
    const int rgran = a.pitch ? (a.pitch - 4) / 256 : 0;                    // 256-dword granules per row
    const int padE = RP ? a.rowpad / (int)(sizeof(R) / 4) : 0;                 // R elements of padding behind a granule (padded runs)
    const int zpitch = a.pitch ? a.pitch / (int)(sizeof(R) / 4) : a.Mr * CS;   // R elements between rows (padded runs: + padE from segment to segment)
    const auto dma = [&](int64_t tile, int buf) {
        if (!is_dma || !dma_ok(tile)) return;
        const int64_t q0 = tile * Q, z0 = q0 * a.Mr + cbase;
        const int nq = (int)std::min<int64_t>(Q, a.nrows - q0);
        const mm_i4 rs = mm_rsrc(xc + (z0 - a.hl) * CS, (a.xlen - (z0 - a.hl)) * 4 * DW);   // re-based at the tile start: zero fill past the signal
        const int64_t exist = (a.xlen - (z0 - a.hl)) * DW;                     // dwords of the signal from the tile start on
        if (a.pitch == 0) {
            const int nzd = (nq * a.Mr + a.Mr + wtail) * DW;   // dwords of the tile
            for (int i = wave - ncomp; 256 * i < nzd; i += a.nd) {   // granules of 256 dwords, round-robin over the DMA waves
                const unsigned dst = lds0 + (unsigned)(buf * a.bufsz + (256 + (RP ? a.rowpad : 0)) * i) * 4u;   // (padded runs: rowpad dwords between granules)
                if (256 * (int64_t)(i + 1) <= exist) mm_dma256(rs, dst, (256 * i + 4 * lane) * 4);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) mm_dma64(rs, dst + 256u * j, (256 * i + 64 * j + lane) * 4);
                }
            }
        } else {
            for (int i = wave - ncomp; i < nq * rgran; i += a.nd) {   // (row, granule) pairs
                const int row = i / rgran, gr = i - row * rgran;
                const int src = row * a.Mr * DW + 256 * gr;                     // dwords from the tile start
                const unsigned dst = lds0 + (unsigned)(buf * a.bufsz + row * a.pitch + 256 * gr) * 4u;
                if (src + 256 <= exist) mm_dma256(rs, dst, (src + 4 * lane) * 4);
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) mm_dma64(rs, dst + 256u * j, (src + 64 * j + lane) * 4);
                }
            }
        }
    };
    // the outputs of a tile, m = q0 Lr .., are contiguous in y: coalesced 16-byte stores (element-aligned; global memory takes them
    // unaligned) by the storing waves, four LDS reads in flight per thread.  Indices count R elements.
    const int st0 = (int)threadIdx.x - 64 * (ncomp + a.nd), stn = 64 * a.ns;
    const int lrc = a.Lr * CS;
    const auto copy_out = [&](int64_t tile, const R* zo) {
        if (!is_store) return;
        const int64_t q0 = tile * Q, mbase = q0 * a.Lr;
        const int total = (int)std::min<int64_t>(std::min<int64_t>(Q, a.nrows - q0) * a.Lr, a.nout - mbase) * CS;
        R* yo = yc + mbase * CS;
        typedef R vec_t __attribute__((ext_vector_type(VW)));
        const bool flat = a.Lp == lrc;   // rows without padding: the buffer IS the run of outputs
        if (flat || lrc % VW == 0) {
            const int nv = total / VW;
            for (int iv = st0; iv < nv; iv += 4 * stn) {
                vec_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int idx = VW * std::min(iv + u * stn, nv - 1), row = flat ? 0 : (int)__umulhi((unsigned)idx, a.rmagic), col = idx - row * lrc;
                    v[u] = *reinterpret_cast<const vec_t*>(zo + row * a.Lp + col);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (iv + u * stn < nv) __builtin_memcpy(yo + VW * (iv + u * stn), &v[u], sizeof(vec_t));
            }
            for (int idx = nv * VW + st0; idx < total; idx += stn) {
                const int row = flat ? 0 : (int)__umulhi((unsigned)idx, a.rmagic), col = idx - row * lrc;
                yo[idx] = zo[row * a.Lp + col];
            }
        } else if (a.vstore) {
            // rows of Lr elements that are not whole vectors (147//160: ten column blocks, 147 outputs per row): a vector's elements are
            // gathered one by one -- they may straddle a row end -- and leave as ONE wide store; the run of outputs itself is contiguous
            const int nv = total / VW;
            for (int iv = st0; iv < nv; iv += 2 * stn) {
                vec_t v[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int idx = VW * std::min(iv + u * stn, nv - 1);
                    int row = (int)__umulhi((unsigned)idx, a.rmagic), col = idx - row * lrc;
#pragma unroll
                    for (int j = 0; j < VW; ++j) {
                        v[u][j] = zo[row * a.Lp + col];
                        if (++col == lrc) { col = 0; ++row; }
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (iv + u * stn < nv) __builtin_memcpy(yo + VW * (iv + u * stn), &v[u], sizeof(vec_t));
            }
            for (int idx = nv * VW + st0; idx < total; idx += stn) {
                const int row = (int)__umulhi((unsigned)idx, a.rmagic), col = idx - row * lrc;
                yo[idx] = zo[row * a.Lp + col];
            }
        } else {
            for (int idx = st0; idx < total; idx += stn) {
                const int row = (int)__umulhi((unsigned)idx, a.rmagic), col = idx - row * lrc;
                yo[idx] = zo[row * a.Lp + col];
            }
        }
    };
    // Which row of the tile a row of the 16 x 16 product is: with odd Mr, the 16 EVEN (then the 16 odd) rows of a 32-row span put the
    // 2 x 16 A-operand reads of a lane group on 32 different banks (16 consecutive rows collide two ways).
    const bool eo = CH >= 2 && (a.Mr & 1) && a.pitch == 0;   // (a single 16-row chunk per wave keeps consecutive rows)
    const int ra = eo ? 2 : 1;
    const auto rbase = [&](int c) { return 16 * CH * wg + (eo ? 32 * (c >> 1) + (c & 1) : 16 * c); };
    R* zout = zs + 2 * (a.bufsz / (int)(sizeof(R) / 4));
    const int osz = Q * a.Lp;
    int cur = 0;
    int64_t prev_tile = -1;
    dma(blockIdx.x, 0);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, cur ^= 1) {
        const int64_t q0 = tile * Q;
        const int nq = (int)std::min<int64_t>(Q, a.nrows - q0);
        const int64_t z0 = q0 * a.Mr + cbase;
        const int nz = nq * a.Mr + a.Mr + wtail;
        const R* zt = zs + cur * (a.bufsz / (int)(sizeof(R) / 4));   // this tile's samples
        R* zo = zout + cur * osz;                                      // this tile's outputs
        if (dma_ok(tile)) {
            if (is_dma) __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's share of the tile has landed
        } else {  // the first tile(s) straddle the history
            R* zw = zs + cur * (a.bufsz / (int)(sizeof(R) / 4));
            const int rowlen = a.pitch ? (a.Mr + wtail) * CS : nz * CS, nrow = a.pitch ? nq : 1;   // R elements per staged row; rows
            for (int k2 = threadIdx.x; k2 < rowlen * nrow; k2 += blockDim.x) {
                const int row = k2 / rowlen, e = k2 - row * rowlen;
                const int64_t zi = z0 + (int64_t)row * a.Mr + e / CS;
                const int part = e % CS;
                R v = (R)0;
                if (zi < a.hl) v = hc[zi * CS + part];
                else if (zi - a.hl < a.xlen) v = xc[(zi - a.hl) * CS + part];
                zw[row * zpitch + e + (RP ? ((e * (int)(sizeof(R) / 4)) >> 8) * padE : 0)] = v;
            }
            __builtin_amdgcn_s_waitcnt(0x0f70);
        }
        __syncthreads();   // tile t is in; the outputs of t-1 are complete; the other sample buffer and the other output buffer are free
        if (!MDSP_ABLATED(a, 1)) dma(tile + gridDim.x, cur ^ 1);
        if (prev_tile >= 0 && !MDSP_ABLATED(a, 4)) copy_out(prev_tile, zout + (cur ^ 1) * osz);
        if (is_comp && !MDSP_ABLATED(a, 2)) {
            constexpr int KBU = T == 0 ? 1 : NBLK;   // blocks of the unrolled inner loop (their taps are registers hreg[kb])
            for (int b0 = wb0; b0 < a.NB; b0 += KBU * a.NBW)   // (T = 0: the run-time walk over a wave's blocks; else one trip)
#pragma unroll
            for (int kb = 0; kb < KBU; ++kb) {   // (one block per wave unless the taps are fetched, T = 0, or NBLK > 1)
                const int b = b0 + kb * a.NBW;
                if (b >= a.NB) break;
                if (a.NBW < a.NB) block_setup(b);
                acc_t acc[CS][CH];
#pragma unroll
                for (int p = 0; p < CS; ++p)
#pragma unroll
                    for (int c = 0; c < CH; ++c) acc[p][c] = acc_t{(R)0, (R)0, (R)0, (R)0};
                const R* ap[CH];   // A operand: row = lane % 16, k = lane / 16
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int row = ra * lj + rbase(c);
                    ap[c] = zt + row * zpitch + (RP ? (((row * a.Mr + c0 + lk) * DW) >> 8) * padE : 0) + (c0 + lk) * CS;
                }
                // padded runs (T != 0, a window shorter than a granule: it meets ONE pad at most): the positions behind the granule boundary sit
                // padE elements further on -- a per-lane choice between two base pointers, so that every read keeps its immediate offset (computed
                // addresses cost the read-ahead of the A operands: measured 1.08 against 0.78 ms at 147//160)
                if constexpr (T != 0 && RP) {
                    // dwords from this lane's first window position to the next granule boundary (16 rows are a whole number of granules,
                    // so the distance is the same for every chunk)
                    const int th = 256 - (((ra * lj + rbase(0)) * a.Mr + c0 + lk) * DW & 255);   // (rbase(0): single-chunk waves need not start on a granule, round 5 prep)
#pragma unroll
                    for (int t = 0; t < TR; ++t) {
                        const bool hi = 4 * t * DW >= th;
                        // (round 5 prep) windows longer than a granule -- 4 T DW dwords up to 512 -- meet a second pad: a third base pointer
                        const bool hi2 = 4 * (T - 1) * DW + DW > 256 && 4 * t * DW >= th + 256;
#pragma unroll
                        for (int c = 0; c < CH; ++c) {
                            const R* pp = hi2 ? ap[c] + 2 * padE : hi ? ap[c] + padE : ap[c];
#pragma unroll
                            for (int p = 0; p < CS; ++p) acc[p][c] = Mm<R>::mfma(pp[4 * t * CS + p], hreg[T == 0 ? 0 : kb][t], acc[p][c]);
                        }
                    }
                } else if constexpr (T != 0) {
#pragma unroll
                    for (int t = 0; t < T; ++t)
#pragma unroll
                        for (int c = 0; c < CH; ++c)
#pragma unroll
                            for (int p = 0; p < CS; ++p) acc[p][c] = Mm<R>::mfma(ap[c][4 * t * CS + p], hreg[T == 0 ? 0 : kb][t], acc[p][c]);
                } else {
                    // steps is a multiple of 8: the taps of eight k-steps are fetched while the previous eight are multiplied (a fetch is an L2 round
                    // trip; a wave that waits for it in front of every group leaves its SIMD's matrix pipe idle half of the time).  The fetched
                    // words are carried RAW into the next group and only then masked: a select next to the fetch would wait for it on the spot.
                    // Measured against masking next to the fetch, alternating processes on one box (tools/r03_session35.sh): ComplexF64 3//8 4.94 -> 4.37 ms,
                    // 1//4 2.99 -> 2.76, 1//8 5.16 -> 5.04; Float32 1//8 +3 %, but 1//16 -7 %, Float64 1//16 -4 %: the carried form for ComplexF64 only.
                    // (round 5 prep) padded runs with fetched taps: the window spans any number of granules, so the pads in front of a position are
                    // computed per k-step (one shift and one multiply-add beside a tap fetch and CH matrix instructions; the vector unit idles here)
                    const int off0 = RP ? (((ra * lj + rbase(0)) * a.Mr + c0 + lk) * DW & 255) : 0;
                    const auto padx = [&](int t) { return RP ? ((off0 + 4 * t * DW) >> 8) * padE : 0; };
                    if constexpr (MDSP_FIR_TAP_CARRY && CS == 2 && sizeof(R) == 8) {
                    R hraw[8];
                    unsigned okm = 0;
                    const auto fetch = [&](int tb) {
                        okm = 0;
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int i = 4 * (tb + u) + lk - tap_delta;
                            const bool ok = tap_valid && i >= 0 && i < a.tp;
                            hraw[u] = pf[ok ? (int64_t)i * a.L + tap_phase : (int64_t)0];
                            okm |= ok ? 1u << u : 0u;
                        }
                    };
                    fetch(0);
                    for (int t0 = 0; t0 < steps; t0 += 8) {
                        R h[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) h[u] = (okm >> u & 1u) ? hraw[u] : (R)0;
                        fetch(t0 + 8 < steps ? t0 + 8 : t0);   // (the last group re-reads its own: no branch around the loads)
#pragma unroll
                        for (int u = 0; u < 8; ++u)
#pragma unroll
                            for (int c = 0; c < CH; ++c)
#pragma unroll
                                for (int p = 0; p < CS; ++p) acc[p][c] = Mm<R>::mfma(ap[c][4 * (t0 + u) * CS + p + padx(t0 + u)], h[u], acc[p][c]);
                    }
                    } else {
                    R h[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) h[u] = tap(u);
                    for (int t0 = 0; t0 < steps; t0 += 8) {
                        R hn[8];
                        const int tn = t0 + 8 < steps ? t0 + 8 : t0;
#pragma unroll
                        for (int u = 0; u < 8; ++u) hn[u] = tap(tn + u);
#pragma unroll
                        for (int u = 0; u < 8; ++u)
#pragma unroll
                            for (int c = 0; c < CH; ++c)
#pragma unroll
                                for (int p = 0; p < CS; ++p) acc[p][c] = Mm<R>::mfma(ap[c][4 * (t0 + u) * CS + p + padx(t0 + u)], h[u], acc[p][c]);
#pragma unroll
                        for (int u = 0; u < 8; ++u) h[u] = hn[u];
                    }
                    }
                }
                if (16 * wb + lj < a.Lr) {
#pragma unroll
                    for (int c = 0; c < CH; ++c)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int p = 0; p < CS; ++p) zo[(ra * Mm<R>::row(lk, r) + rbase(c)) * a.Lp + (16 * wb + lj) * CS + p] = acc[p][c][r];
                }
            }
        }
        prev_tile = tile;
    }
    __syncthreads();
    if (prev_tile >= 0) copy_out(prev_tile, zout + (cur ^ 1) * osz);
}
// the two kernels around the body: taps in registers on a plain run -> no merged LDS reads; fetched taps (T = 0) and padded runs -> the pass stays on
template <typename R, int CS, int CH, int T, bool RP = false, int NBLK = 1>
MDSP_NO_LSO __global__ __launch_bounds__(1024) void polyphase_mfma_kernel(FirMArgs a) { polyphase_mfma_body<R, CS, CH, T, RP, NBLK>(a); }
template <typename R, int CS, int CH, int T, bool RP = false, int NBLK = 1>
__global__ __launch_bounds__(1024) void polyphase_mfma_kernel_lso(FirMArgs a) { polyphase_mfma_body<R, CS, CH, T, RP, NBLK>(a); }

// ---- host side: the geometry (FirMGeo: fir_mm.h), launch and dispatch --------------------------------------------------------------------------
int fir_mm_tsel(int64_t steps) { return steps <= 4 ? 4 : steps <= 8 ? 8 : steps <= 12 ? 12 : steps <= 16 ? 16 : steps <= 20 ? 20 : steps <= 24 ? 24 : steps <= 32 ? 32 : steps <= 48 ? 48 : 64; }
// tight (round 4, only tried where nothing else fits the LDS -- shapes that would otherwise fall to the generic kernel at 0.03 - 0.07 of the roofline):
//   rb_cap > 0: rows of at most rb_cap rounds for L < 16 (ComplexF64 1//16: 14 rounds of 16 samples fit where the conflict-best 15 miss by 1 KiB);
//   Float32 windows of 33 - 40 k-steps take the 40-step register form with single-chunk waves instead of 48 (ComplexF32 160//441: the 32 samples
//   less of window tail per buffer are what the tile misses); ComplexF64 windows of 13 - 14 k-steps take a 14-step form (round 5).
FirMGeo fir_mm_geo_compute(const mdsp_fir_s* f, bool allow_regs, int rb_cap = 0) {   // allow_regs: round 3's register-tap rules (fewer chunks / shorter rows)
    FirMGeo g;
    const bool t64 = allow_regs && tunables().fir_mm_t64 != 0;
    // element type: signal and compute type must agree (Float32 taps x Float32 samples, or Float64 arithmetic on Float64 samples)
    if (f->ctaps || f->acc_double != dtype_is_double(f->x_dtype)) return g;   // (complex taps: not a matrix-core shape)
    g.esz = f->acc_double ? 8 : 4;
    g.CS = dtype_is_complex(f->x_dtype) ? 2 : 1;
    int chmax = (g.esz == 4 && g.CS == 1) ? 4 : 2;   // 16-row chunks per multiplying wave: fewer when the tile would not fit the LDS
    if (tunables().fir_mm_ch > 0) chmax = std::min(chmax, tunables().fir_mm_ch);
    if (f->L > 1024 || f->M > 4096) return g;
    if (f->L < 16) {   // rounds per row: most outputs per LDS cycle of the A-operand reads (16 rows x 2 taps per lane group)
        double best = -1;
        for (int rb = 1; rb * f->L <= 16 && (rb_cap <= 0 || rb <= rb_cap); ++rb) {
            const int64_t mr = rb * f->M;
            int worst = 1;
            if (!(mr & 1)) {   // odd strides are conflict-free with the even / odd row order of the kernel
                int cnt[32] = {0};
                for (int i = 0; i < 16; ++i)
                    for (int k = 0; k < 2; ++k) worst = std::max(worst, ++cnt[(int)((i * mr + k) & 31)]);
            }
            double score = (double)(rb * f->L) / worst + 1e-3 * rb;
            // rows short enough for the taps to stay in registers (single-chunk waves) run up to twice as fast per k-step as rows whose taps are
            // fetched per tile (profiles/r03o_fir_register_taps.json): 1//8 with 293 taps takes 11 outputs per row (94 k-steps) instead of 15 (104)
            if (t64) {
                const int64_t st = cdiv(f->tp + ((f->L - 1) + (int64_t)(std::min<int64_t>(rb * f->L, 16) - 1) * f->M) / f->L, (int64_t)4);
                const int64_t treg = g.esz == 4 ? 96 : (g.CS == 1 ? 48 : 40);
                if (st <= treg) score *= 1.6;   // (2.0 takes 9 of 16 columns for ComplexF64 3//8: measured 14 % slower than fetching with 15)
            }
            if (score > best) { best = score; g.RB = rb; }
        }
    }
    g.Lr = g.RB * (int)f->L;
    g.Mr = g.RB * (int)f->M;
    g.NB = (int)cdiv((int64_t)g.Lr, (int64_t)16);
    const int64_t steps = cdiv(f->tp + ((f->L - 1) + (int64_t)(std::min(g.Lr, 16) - 1) * f->M) / f->L, (int64_t)4);   // tp + max delta within a block
    if (steps > 1024 || (int64_t)(f->L + (int64_t)(g.Lr + 16) * f->M) * f->L >= ((int64_t)1 << 32)) return g;   // (the multiply-high quotients stay exact)
    g.NBW = std::min(g.NB, 12);   // more than 12 column blocks (L > 192): a wave takes several, with their taps fetched per tile
    if (g.NBW < g.NB) g.NBW = (int)cdiv((int64_t)g.NB, cdiv((int64_t)g.NB, (int64_t)12));   // as even as it gets
    // Taps in registers whenever SOME chunk count admits it (round 3): a wave that carries fewer chunks of 16 rows has fewer accumulators and
    // room for more taps -- Float32: 48 k-steps with four chunks, 64 with two, 96 with one (ComplexF32 64 / 96); Float64 32 / 48 (ComplexF64
    // 24 / 40).  Fetching the taps per tile instead (T = 0) costs far more than the smaller tile: 1//4 (56 steps) 0.67 -> 0.46 ms with two
    // chunks, profiles/r03o_fir_register_taps.json.  MDSP_FIR_MM_T64=0: round 2's limits.
    const auto tmax_of = [&](int ch) {
        if (g.esz == 4) return g.CS == 1 ? (ch >= 4 ? 48 : ch == 2 ? 64 : 96) : (ch >= 2 ? 64 : 96);   // (112 steps spill 43 registers: slower than fetching)
        return g.CS == 1 ? (ch >= 2 ? 32 : 48) : (ch >= 2 ? 24 : 40);
    };
    bool regs = false;
    if (g.NBW == g.NB && t64 && steps > tmax_of(chmax)) {
        for (int ch = chmax / 2; ch >= 1 && !regs; ch /= 2)
            if (steps <= tmax_of(ch)) {
                chmax = ch;
                regs = true;
            }
    }
    // L > 192 (more than 12 column blocks): a wave walks two or three blocks.  With short windows (12 / 16 k-steps: the 32 taps per phase of the
    // default resampling filters) the taps of ALL its blocks fit registers -- single-chunk waves -- instead of being fetched per tile.
    const int nblk = (int)cdiv((int64_t)g.NB, (int64_t)g.NBW);
    if (g.NBW < g.NB && t64 && nblk <= 3 && steps <= 16 && tunables().fir_mm_nblk != 0) {
        chmax = g.esz == 4 ? std::min(chmax, 2) : 1;   // (Float32: two chunks of 16 rows per wave still leave room for three blocks' taps)
        g.NBLK = nblk;
        g.T = steps <= 12 ? 12 : 16;
        g.steps = g.T;
    } else
    if (regs) {
        g.T = (g.esz == 8 && steps > 32 && steps <= 40) ? 40 : steps <= 64 ? fir_mm_tsel(steps) : steps <= 80 ? 80 : 96;   // (Float64: 40 between 32 and 48 -- a shorter window tail)
        g.steps = g.T;
    } else
    if (steps > (g.esz == 8 ? (g.CS == 2 ? 24 : 32) : (g.CS == 2 ? 64 : 48)) || g.NBW < g.NB) {   // (beyond: too many registers -- measured: ComplexF64 at T = 32 and Float32 at T = 64 spill and lose 40 - 50 %)   // the taps do not fit registers (T, Float64 2 T, VGPRs): fetched per tile
        g.T = 0;
        g.steps = (int)cdiv(steps, (int64_t)8) * 8;
    } else
    if (rb_cap < 0 && g.esz == 4 && steps > 32 && steps <= 40) {
        g.T = 40;
        g.steps = 40;
        chmax = 1;
    } else
    if (rb_cap < 0 && g.esz == 8 && g.CS == 2 && steps > 12 && steps <= 14) {   // (round 5) ComplexF64 160//147 with resample_filter's 5921 taps (13 k-steps): the 16-step
        g.T = 14;                                                                  // form's window tail misses the LDS by 2 KiB and the cell fell to the generic kernel (0.125)
        g.steps = 14;
        chmax = 1;
    } else {
        g.T = fir_mm_tsel(steps);
        g.steps = g.T;
    }
    g.Lp = g.NB == 1 ? g.Lr * g.CS : 16 * g.NB * g.CS + 16 / g.esz;
    const int dw = g.esz / 4 * g.CS;
    // Rows (lane stride Mr samples) of a linear tile hit banks / gcd(Mr dw, banks) places.  From four-way conflicts on, staging the rows
    // one by one (pitch 256 g + 4 dwords: two-way conflicts in Float32, none in Float64) is the alternative -- unless the window tail it
    // duplicates per row (long filters) shrinks the tile too much.
    const int wtail = 4 * g.steps + 4;
    // conflict ways of the 16 rows of an A operand: 4-byte reads see 32 banks, 8-byte reads 64; rows s dwords apart land on banks / gcd(s, banks) places
    const int banks = g.esz == 8 ? 64 : 32;
    const auto ways_of = [&](int64_t s) { return (double)std::max<int64_t>(1, 16 / std::min<int64_t>(16, banks / std::gcd(s, (int64_t)banks))); };
    const int rpitch = (int)cdiv((int64_t)(g.Mr + wtail) * dw, (int64_t)256) * 256 + 4;
    const double ways_lin = ((g.Mr * dw) & 1) ? 1.0 : ways_of((int64_t)g.Mr * dw), ways_row = ways_of(rpitch);
    // cost per row of outputs ~ max(1, 0.2 ways) [the A-operand reads keep the LDS about 20 % busy when conflict-free] + 32 / rows [one
    // barrier and pipeline turn-around per tile, worth about 32 rows]: the staging mode and tile with the smallest cost
    // Two ways to pick the tile (16 CH rows per multiplying wave, NG groups of NBW waves):
    //   * ratios above one (and anything with several column blocks per wave): the largest tile that fits, scored by
    //     max(1, 0.2 ways) + 32 / rows as in round 2 -- with at most FOUR groups when there is one column block (2//1, 3//2, 4//1 ...):
    //     4 + 2 + 2 waves put one multiplying and one memory wave of a workgroup on every SIMD and three such workgroups share a CU
    //     (2//1 0.95 -> 0.91 ms, 4//1 2.03 -> 1.82, ComplexF32 2//1 1.84 -> 1.49; 3 and 6 groups leave the SIMDs unevenly loaded and lose
    //     10 - 20 %).  profiles/r03h_fir_groups.json
    //   * ratios up to one (decimators, single-rate FIR): one big workgroup per CU, so what a tile costs is the matrix work of its BUSIEST
    //     SIMD -- waves go round the four SIMDs, ceil(mw / 4) multiplying waves on the fullest -- plus the tap fetches of the long-filter
    //     mode (every multiplying wave fetches every k-step's taps: ~25 clocks each through the CU's one L1 pipe) plus ~3900 clocks of
    //     barrier and pipeline turn-around, per row:  cost = (ceil(mw/4) CH steps c_mfma max(1, 0.2 ways) + [T = 0] mw steps 25 + 3900) / rows.
    //     Fitted on 1//8 (0.98 : 0.87 : 1.22 measured for CH = 4, 2, 1 against 1 : 0.88 : 1.27) and checked on 1//2 ... 1//16, 3//8
    //     (profiles/r03h_fir_groups.json): 1//3 and 3//8 leave five groups for eight half-size ones (+25 %), 1//8 and 1//16 two / one
    //     groups of four chunks for twice as many of two (+12 %, +30 %).  Costs within 3 % of each other go to the larger tile.
    const bool by_model = f->L <= f->M && tunables().fir_mm_ng <= 0 && tunables().fir_mm_ch <= 0;
    double best_score = -1, best_cost = 0;
    int best_rows = 0, best_mw = 0;
    for (int pad = tunables().fir_mm_pad == 0 ? 0 : 1; pad >= 0 && !g.ok; --pad) {   // (a last resort: output rows without their 16 bytes of padding -- ComplexF64 at 160//147 then fits exactly)
    if (g.NB > 1) g.Lp = 16 * g.NB * g.CS + (pad ? 16 / g.esz : 0);
    else if (!pad) break;
    // round 3: a third staging form for the bank-hostile strides -- ONE run per tile, moved by the same full 256-dword DMA granules as mode 0,
    // with 4 dwords of padding behind every GRANULE (dword d of the tile at d + 4 (d / 256)).  Rows then spread over the banks (counted below),
    // no window tail is fetched twice (row-staged 147//160: 228 samples per 160 new ones in 256-dword granules, 1.6x the L2 -> LDS traffic; its
    // DMA alone took 0.53 of the kernel's 0.78 ms) and the tile is not shrunk by the duplicates.  A window shorter than a granule meets one pad
    // at most, at a lane-dependent step: the A-operand reads choose between two base pointers per lane and keep their immediate offsets.
    // What did NOT work on the way (profiles/r03k_fir_padded_runs.json): padding behind every row or every two rows -- the segments then are
    // 640 or 1280 bytes, i.e. 16-byte DMA with lanes switched off, or a 16-byte plus a 4-byte instruction: 0.87 - 1.0 ms of DMA alone against 0.36
    // for whole granules -- and computed (instead of immediate) read offsets.  147//160 0.76 -> 0.60 ms, Float64 1.41 -> 1.08, 49//48 1.64 -> 0.73.
    const int RPAD = tunables().fir_mm_rpad > 0 ? tunables().fir_mm_rpad : 4;
    double ways_pad = 1;
    {   // conflict ways of the 16 rows of an A operand, counted on the layout itself
        int cnt[64] = {0};
        for (int i = 0; i < 16; ++i) {
            const int64_t d = (int64_t)i * g.Mr * dw, ad = d + (d >> 8) * RPAD;
            ways_pad = std::max<double>(ways_pad, ++cnt[(int)((g.esz == 8 ? ad / 2 : ad) % 32)]);
        }
    }
    const int fm = tunables().fir_mm_rows;
    for (int mode = 0; mode < 3; ++mode) {   // 0: one linear run per tile, 1: row by row, 2: one run with padded rows
        if (mode >= 1 && ways_lin < 4 && fm < 0) continue;
        if (fm >= 0 && mode != fm) continue;
        // 16 rows are whole granules; taps in registers; a window (4 T dw dwords) meets one pad at most.  (round 5 prep, MDSP_FIR_MM_RPX=1: fetched taps
        // with computed pads, and register forms of single-chunk waves whose window meets two pads at most -- 4 T dw <= 512)
        const bool rpx = tunables().fir_mm_rpx != 0;
        const bool gran16 = !((g.Mr * dw) & 15);   // 16 rows are whole granules: every chunk of a wave crosses at the same step (single-chunk waves do not need it)
        const bool pad_ok = (gran16 && g.T != 0 && g.T <= 32 && g.T * dw <= 64) || (rpx && g.T == 0 && (gran16 || chmax == 1)) ||
                            (rpx && g.T != 0 && g.NBLK == 1 && g.T * dw <= 128 && chmax == 1);
        if (mode == 2 && !pad_ok) continue;
        if (mode == 1 && fm < 0 && pad_ok && ways_pad <= 2 * ways_row) continue;   // the padded run replaces the row-staged form wherever it applies and spreads the
                                                                                     // rows comparably (rows shorter than a granule share its pad: Mr dw = 16 stays 15-way)
        const double ways = mode == 1 ? ways_row : mode == 2 ? ways_pad : ways_lin;
        for (int ch = chmax; ch >= 1; ch /= 2) {   // the largest tile (16 CH NG rows) that leaves four memory waves and fits the LDS
            const int rows = 16 * ch;
            const int ngdef = (g.NBW == 1 && f->L > f->M) ? 4 : 8;
            for (int ng = std::min(tunables().fir_mm_ng > 0 ? tunables().fir_mm_ng : ngdef, 12 / g.NBW); ng >= 1; --ng) {
                const int64_t bufsz = mode == 1 ? cdiv((int64_t)rows * ng * rpitch, (int64_t)256) * 256
                                    : mode == 2 ? cdiv((cdiv(((int64_t)rows * ng * g.Mr + g.Mr + wtail) * dw, (int64_t)256) + 1) * (256 + RPAD), (int64_t)256) * 256
                                                : cdiv(((int64_t)rows * ng * g.Mr + g.Mr + wtail) * dw, (int64_t)256) * 256;
                const size_t bytes = (size_t)(2 * bufsz) * 4 + (size_t)(2 * rows * ng * g.Lp) * (size_t)g.esz;
                if (bytes > 160 * 1024) continue;
                const auto take = [&] { g.CH = ch; g.NG = ng; g.bufsz = bufsz; g.lds_bytes = bytes; g.ok = true; g.pitch = mode == 1 ? rpitch : 0; g.rowpad = mode == 2 ? RPAD : 0; };
                if (!by_model) {
                    const double score = 1.0 / (std::max(1.0, 0.2 * ways) + 32.0 / (rows * ng)) + 1e-6 * ch;
                    if (score > best_score) { best_score = score; take(); }
                    break;   // (only the largest tile of this chunk count)
                }
                const int mw = g.NBW * ng, trows = rows * ng;
                const double c_mfma = (g.esz == 8 ? 64.0 : 32.0) * g.CS;
                const double cost = (((mw + 3) / 4) * (double)ch * cdiv(g.NB, g.NBW) * g.steps * c_mfma * std::max(1.0, 0.2 * ways) + (g.T == 0 ? mw * g.steps * 25.0 : 0.0) + 3900.0) / trows;
                // (round 5 prep, MDSP_FIR_MM_TIEWAVES=1, unmeasured as a rule) equal tiles at equal cost: the one with more multiplying waves -- the k-steps of
                // a wave are a latency chain (profiles/r04_fir_decim16_pmc.json), and profiles/r04_fir_ch1_ab.json has both tie cases faster that way
                // (1//16 Float32 1.74 -> 1.46 ms, ComplexF32 1//4 1.01 -> 0.83)
                const bool tie_waves = tunables().fir_mm_tiewaves != 0 && g.ok && cost < 1.03 * best_cost && trows == best_rows && mw > best_mw;
                if (!g.ok || cost < 0.97 * best_cost || (cost < 1.03 * best_cost && trows > best_rows) || tie_waves) {
                    best_cost = g.ok ? std::min(best_cost, cost) : cost;
                    best_rows = trows;
                    best_mw = mw;
                    take();
                }
            }
        }
    }
    }
    if (!g.ok) return g;
    const int extra = 16 - g.NBW * g.NG;   // memory waves beside the multiplying ones (16 waves per workgroup at most)
    g.nd = extra >= 4 ? 2 : 1;
    g.ns = std::max(1, std::min(f->L >= f->M ? 2 : 4, extra - g.nd));   // measured: two store waves when the ratio is >= 1 (160//147 1.94 -> 1.87 ms, 2//1 1.01 -> 0.93), four below (1//2 0.48 -> 0.45)
    if (tunables().fir_mm_nd > 0 && tunables().fir_mm_ns > 0 && tunables().fir_mm_nd + tunables().fir_mm_ns <= extra) {   // tuning knobs
        g.nd = tunables().fir_mm_nd;
        g.ns = tunables().fir_mm_ns;
    }
    return g;
}

}  // namespace

// every exec asks twice (use? / dispatch): one memo per calling thread, keyed by what the geometry depends on (the search above is a few
// hundred iterations -- microseconds, but a sample-at-a-time stream pays them per call)
FirMGeo mdsp::fir_mm_geo(const mdsp_fir_s* f) {
    struct Memo {
        int64_t L = -1, M = 0, hlen = 0;
        int td = 0, xd = 0;
        uint64_t gen = 0;
        FirMGeo g;
    };
    static thread_local Memo m;
    const uint64_t gen = tunables_generation();
    if (m.L != f->L || m.M != f->M || m.hlen != f->hlen || m.td != f->taps_dtype || m.xd != f->x_dtype || m.gen != gen) {
        m.g = fir_mm_geo_compute(f, true);
        if (!m.g.ok) m.g = fir_mm_geo_compute(f, false);   // (longer register forms read a longer window tail: where that no longer fits the LDS, fetch the taps)
        if (!m.g.ok && tunables().fir_mm_tight != 0) {     // the tight forms: see fir_mm_geo_compute
            if (f->L < 16)
                for (int cap = (int)(16 / f->L) - 1; cap >= 1 && !m.g.ok; --cap) m.g = fir_mm_geo_compute(f, true, cap);
            else m.g = fir_mm_geo_compute(f, true, -1);
        }
        m.L = f->L; m.M = f->M; m.hlen = f->hlen; m.td = f->taps_dtype; m.xd = f->x_dtype; m.gen = gen;
    }
    return m.g;
}

namespace {

bool fir_mm_shape_ok(const mdsp_fir_s* f) { return fir_mm_geo(f).ok; }

template <typename R, int CS, int CH, int T, bool RP = false, int NBLK = 1> int fir_mm_launch(mdsp_fir_s* f, const FirArgs& a, const FirMGeo& g, hipStream_t st) {
    FirMArgs b{};
    b.x = a.x;
    b.hist = a.hist;
    b.y = a.y;
    b.pfbT = a.pfbT;
    b.xlen = a.xlen; b.ldx = a.ldx; b.ldy = a.ldy; b.nout = a.nout;
    b.d0 = a.d0;
    b.L = a.L; b.M = a.M; b.hl = a.hl; b.tp = a.tp;
    b.Lr = g.Lr; b.Mr = g.Mr; b.NB = g.NB; b.NBW = g.NBW; b.NG = g.NG; b.Lp = g.Lp; b.nd = g.nd; b.ns = g.ns;
    b.nrows = cdiv(a.nout, (int64_t)g.Lr);
    b.lmagic = (unsigned)((((uint64_t)1 << 32) + (uint64_t)a.L - 1) / (uint64_t)a.L);
    b.rmagic = (unsigned)((((uint64_t)1 << 32) + (uint64_t)(g.Lr * CS) - 1) / (uint64_t)(g.Lr * CS));
    b.phi0m1 = (int)a.phi0m1;
    b.bufsz = (int)g.bufsz;
    b.pitch = g.pitch;
    b.rowpad = g.rowpad;
    b.steps = g.steps;
    b.vstore = tunables().fir_mm_vstore;
    // measured on 19 ratio x type combinations (profiles/r03l_fir_memprio.json): +2 ... +16 % (config 5 1.86 -> 1.76 ms) wherever a wave owns one column
    // block; -4 % where it walks several (441//160), which keep the default priority
    b.memprio = tunables().fir_mm_prio >= 0 ? tunables().fir_mm_prio : (g.NBW == g.NB ? 1 : 0);
    b.ablate = MDSP_DBG(ablate);
    const int nw = g.NBW * g.NG + g.nd + g.ns;
    void (*kern)(FirMArgs);
    if constexpr (T == 0 || RP) kern = polyphase_mfma_kernel_lso<R, CS, CH, T, RP, NBLK>;
    else kern = polyphase_mfma_kernel<R, CS, CH, T, RP, NBLK>;
    static std::atomic<unsigned long long> lds_opt_in{0};   // once per instantiation and device (later calls may sit inside a stream capture): the whole 160 KiB
    int dev = 0;
    MDSP_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(lds_opt_in.load(std::memory_order_acquire) & bit)) {
        MDSP_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        lds_opt_in.fetch_or(bit, std::memory_order_release);
    }
    const int64_t ntiles = cdiv(b.nrows, (int64_t)16 * CH * g.NG);
    int wgs = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)(160 * 1024) / (int64_t)g.lds_bytes, 32 / nw));
    if (tunables().wg_per_cu > 0) wgs = tunables().wg_per_cu;
    const int64_t per = std::max<int64_t>(1, (int64_t)device_cu_count() * wgs / std::max<int64_t>(1, f->nch));
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, per), (unsigned)f->nch);
    hipLaunchKernelGGL(kern, grid, dim3(64 * nw), g.lds_bytes, st, b);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

template <typename R, int CS, int CH> int fir_mm_dispatch_t(mdsp_fir_s* f, const FirArgs& a, const FirMGeo& g, hipStream_t st) {
    if constexpr (CH == 1 || (CH == 2 && sizeof(R) == 4)) {
        if (g.NBLK == 2) return g.T == 12 ? fir_mm_launch<R, CS, CH, 12, false, 2>(f, a, g, st) : fir_mm_launch<R, CS, CH, 16, false, 2>(f, a, g, st);
        if (g.NBLK == 3) return g.T == 12 ? fir_mm_launch<R, CS, CH, 12, false, 3>(f, a, g, st) : fir_mm_launch<R, CS, CH, 16, false, 3>(f, a, g, st);
    }
    if (g.NBLK > 1) MDSP_FAIL(MDSP_ERR_ASSERTION, "no matrix-core instantiation for %d blocks per wave with %d chunks", g.NBLK, CH);
    switch (g.T) {
        case 0: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 0, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 0>(f, a, g, st);
        case 4: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 4, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 4>(f, a, g, st);
        case 8: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 8, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 8>(f, a, g, st);
        case 12: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 12, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 12>(f, a, g, st);
        case 14:
            if constexpr (sizeof(R) == 8 && CS == 2 && CH == 1) return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 14, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 14>(f, a, g, st);
            MDSP_FAIL(MDSP_ERR_ASSERTION, "the 14-step form exists for ComplexF64 single-chunk waves only");
        case 16: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 16, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 16>(f, a, g, st);
        case 20: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 20, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 20>(f, a, g, st);
        case 24: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 24, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 24>(f, a, g, st);
        case 32: return g.rowpad > 0 ? fir_mm_launch<R, CS, CH, 32, true>(f, a, g, st) : fir_mm_launch<R, CS, CH, 32>(f, a, g, st);
        default:
            if constexpr (CH == 1) {   // the long register forms exist for single-chunk waves only
                if constexpr (sizeof(R) == 4) {
                    if (g.rowpad > 0) {   // (round 5 prep) padded runs with two pads per window: Float32 up to 96 k-steps (ComplexF32: 64)
                        if (g.T == 40) return fir_mm_launch<R, CS, CH, 40, true>(f, a, g, st);
                        if (g.T == 48) return fir_mm_launch<R, CS, CH, 48, true>(f, a, g, st);
                        if (g.T == 64) return fir_mm_launch<R, CS, CH, 64, true>(f, a, g, st);
                        if constexpr (CS == 1) {
                            if (g.T == 80) return fir_mm_launch<R, CS, CH, 80, true>(f, a, g, st);
                            if (g.T == 96) return fir_mm_launch<R, CS, CH, 96, true>(f, a, g, st);
                        }
                        MDSP_FAIL(MDSP_ERR_ASSERTION, "no padded-run instantiation for %d k-steps", g.T);
                    }
                    if (g.T == 40) return fir_mm_launch<R, CS, CH, 40>(f, a, g, st);
                    if (g.T == 80) return fir_mm_launch<R, CS, CH, 80>(f, a, g, st);
                    if (g.T == 96) return fir_mm_launch<R, CS, CH, 96>(f, a, g, st);
                } else {
                    if (g.rowpad > 0) {   // Float64 up to 48 k-steps (ComplexF64: 32 -- one pad, above)
                        if constexpr (CS == 1) {
                            if (g.T == 40) return fir_mm_launch<R, CS, CH, 40, true>(f, a, g, st);
                            if (g.T == 48) return fir_mm_launch<R, CS, CH, 48, true>(f, a, g, st);
                        }
                        MDSP_FAIL(MDSP_ERR_ASSERTION, "no padded-run instantiation for %d k-steps", g.T);
                    }
                    if (g.T == 40) return fir_mm_launch<R, CS, CH, 40>(f, a, g, st);
                    if constexpr (CS == 1) { if (g.T == 48) return fir_mm_launch<R, CS, CH, 48>(f, a, g, st); }
                }
            }
            if (g.T > 64 || (sizeof(R) == 8 && g.T > 32)) MDSP_FAIL(MDSP_ERR_ASSERTION, "no matrix-core instantiation for %d k-steps", g.T);
            if constexpr (sizeof(R) == 4) return g.T == 48 ? fir_mm_launch<R, CS, CH, 48>(f, a, g, st) : fir_mm_launch<R, CS, CH, 64>(f, a, g, st);
            else return fir_mm_launch<R, CS, CH, 32>(f, a, g, st);
    }
}

}  // namespace

int mdsp::fir_mm_dispatch(mdsp_fir_s* f, const FirArgs& a, hipStream_t st) {
    const FirMGeo g = fir_mm_geo(f);
    if (g.esz == 4 && g.CS == 1) return g.CH == 4 ? fir_mm_dispatch_t<float, 1, 4>(f, a, g, st) : g.CH == 2 ? fir_mm_dispatch_t<float, 1, 2>(f, a, g, st) : fir_mm_dispatch_t<float, 1, 1>(f, a, g, st);
    if (g.esz == 4) return g.CH == 2 ? fir_mm_dispatch_t<float, 2, 2>(f, a, g, st) : fir_mm_dispatch_t<float, 2, 1>(f, a, g, st);
    if (g.CS == 1) return g.CH == 2 ? fir_mm_dispatch_t<double, 1, 2>(f, a, g, st) : fir_mm_dispatch_t<double, 1, 1>(f, a, g, st);
    return g.CH == 2 ? fir_mm_dispatch_t<double, 2, 2>(f, a, g, st) : fir_mm_dispatch_t<double, 2, 1>(f, a, g, st);
}

// where the matrix-core kernel is used: wherever the shape fits, whatever the chunk length -- one channel of 2^8 ... 2^16 samples takes
// 17 - 29 us against 32 - 61 us at 2//1, 18 - 23 against 21 - 31 at 160//147, 20 - 26 against 16 - 44 at 1//2 (profiles/r03h_fir_small_chunks.txt:
// no size gate pays), up to 2^28 (profiles/r02r_tune_fir); MDSP_FIR_MM=0 turns it off
bool mdsp::fir_mm_use(const mdsp_fir_s* f, const FirArgs& a) {
    (void)a;
    if (tunables().fir_mm == 0 || tunables().fir_exact || f->exact) return false;
    const FirMGeo g = fir_mm_geo(f);
    if (!g.ok) return false;
    // L > 192 (several column blocks per wave, small tiles): measured slower than the register-tap kernel where that one applies
    // (Float32, 441//160: 1.1 against 2.3 TB/s) and 4 - 5x faster than the generic kernel everything else would take (Float64: 0.26 -> 1.2)
    // (round 3: with the taps of TWO blocks per wave in registers the matrix cores win -- 320//147 1.11 against 1.32 ms, 250//249 0.70 against 0.92;
    // with three the register-tap kernel still does: 441//160 1.67 against 2.39)
    if (g.NBW < g.NB && g.NBLK != 2 && tunables().fir_mm != 1 && fir_fast_ok(f, 2)) return false;
    return true;
}
