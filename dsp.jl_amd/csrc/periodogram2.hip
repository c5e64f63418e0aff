// 2-D periodogram: periodogram(s::AbstractMatrix{<:Real}; nfft, fs, radialsum, radialavg) (periodograms.jl:473-509) with the
// kernels fft2pow2! / fft2pow2radial! (:175-232), composed from the single-column STFT plans of stft.hip and three kernels of
// its own.  An exec is four steps on the caller's stream, with no host synchronisation:
//
//   1. rows     -- internal STFT plan (n = n1, noverlap 0, nfft = N1, one-sided, raw columns) over the n2 columns of s:
//                  A = rfft along dim 1, (H, n2) complex, i contiguous  (H = N1 / 2 + 1)
//   2. transpose-- transpose_kernel: B = A^T, (n2, H) complex, j contiguous (LDS tiles, padded rows)
//   3. columns  -- internal STFT plan (n = n2, nfft = N2, two-sided, psd_only, r = fs n1 n2) over the H columns of B:
//                  P[j + N2 i] = |X[i, j]|^2 / r   (X = fft2 of the zero-padded (N1, N2) input)
//   4. epilogue -- ptype 0: full_kernel writes out[i + ldo j] for all N1 x N2 bins (rows i >= H are the Hermitian mirror of a real
//                  input's full fft); ptype 1 / 2: radial_rows_kernel (R1) + radial_bins_kernel (R2), a two-pass deterministic
//                  reduction (no atomics: bit-identical results run to run).
//
// Radial geometry.  The bin of (i, j) is the reference's round(Int, sqrt(muladd(c1 i, c1 i, (c2 kj)^2))) (+1 there: bins are 0-based
// here), kj the signed frequency index of column j.  Within row i the bin is monotone in |kj| = m, so row i touches the contiguous
// bins [lo_i, hi_i] and every bin is the image of a contiguous m range (and of its negative twins); the rows touching bin k form one
// contiguous row range too (lo_i and hi_i are non-decreasing in i).  The ragged partial buffer holds, for each row, one Float64 per bin
// of [lo_i, hi_i] (R1: the row's weighted sum over that bin, m ascending, the positive then the negative twin); R2 sums each bin's
// rows in a fixed order (a wavefront per bin, rows strided over the lanes, a fixed shuffle tree).  Row offsets, lo_i, each bin's row range and the wave counts are host arithmetic at plan creation
// (mdsp_periodogram2_geometry_for exposes kmax, wc and the partial count without a device).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

using namespace mdsp;

namespace {

// ---------------------------------------------------------------- radial geometry shared by the host tables and the kernels
struct P2Scale {
    double c1, c2;   // :191-197
};
__host__ __device__ inline P2Scale p2_scale(int64_t N1, int64_t N2) {
    return N1 <= N2 ? P2Scale{1.0, (double)N1 / (double)N2} : P2Scale{(double)N2 / (double)N1, 1.0};
}
// 0-based wave-number bin of row i, |kj| = m: round(Int, sqrt(muladd(c1 i, c1 i, (kj c2)^2))) in Float64 (rint: ties to even, as
// Julia's round).  The ONE definition of the bin: plan tables, geometry_for and the R1 kernel all call it.
__host__ __device__ inline int64_t p2_bin(P2Scale s, int64_t i, int64_t m) {
    const double a = s.c1 * (double)i, k = (double)m * s.c2;
    return (int64_t)rint(sqrt(fma(a, a, k * k)));
}
// smallest m in [0, M + 1] with p2_bin(i, m) >= b (M + 1: none).  The guess inverts the radius; the two walks make the answer exact
// whatever the guess (p2_bin is monotone in m), usually after one or two evaluations.
__host__ __device__ inline int64_t p2_first(P2Scale s, int64_t i, int64_t b, int64_t M) {
    const double a = s.c1 * (double)i, h = (double)b - 0.5, d = h * h - a * a;
    const double guess = d > 0 ? ceil(sqrt(d) / s.c2) : 0.0;
    int64_t g = guess < (double)(M + 1) ? (int64_t)guess : M + 1;
    while (g > 0 && p2_bin(s, i, g - 1) >= b) --g;
    while (g <= M && p2_bin(s, i, g) < b) ++g;
    return g;
}

struct P2Geom {
    int64_t N1 = 0, N2 = 0, H = 0, M = 0, Mneg = 0, kmax = 0, npart = 0;
    std::vector<int64_t> off, lo, r0, nr, wc;   // off: H + 1 row offsets into the partials; lo: each row's first bin; r0 / nr: each bin's rows
};
__host__ __device__ inline int64_t p2_row_weight(int64_t i, int64_t H, int64_t N1) { return i == 0 ? 1 : (i < H - 1 ? 2 : (N1 % 2 == 0 ? 1 : 2)); }   // :199-225

int p2_geometry(int64_t N1, int64_t N2, P2Geom& g) {
    if (N1 < 2 || N2 < 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nfft must be >= 2 in both dimensions (got %lld, %lld)", (long long)N1, (long long)N2);
    const P2Scale s = p2_scale(N1, N2);
    g.N1 = N1;
    g.N2 = N2;
    g.H = N1 / 2 + 1;
    g.M = N2 >> 1;          // largest |kj|
    g.Mneg = (N2 - 1) >> 1; // largest |kj| that also occurs as -|kj|
    g.kmax = std::min(N1, N2) / 2 + 1;
    g.off.assign(g.H + 1, 0);
    g.lo.assign(g.H, 0);
    g.r0.assign(g.kmax, -1);
    g.nr.assign(g.kmax, 0);
    g.wc.assign(g.kmax, 0);
    for (int64_t i = 0; i < g.H; ++i) {
        const int64_t lo = p2_bin(s, i, 0), hi = std::min(p2_bin(s, i, g.M), g.kmax - 1), w = p2_row_weight(i, g.H, N1);
        g.lo[i] = lo;
        g.off[i + 1] = g.off[i] + (lo <= hi ? hi - lo + 1 : 0);
        int64_t first = 0;   // = p2_first(s, i, lo, M)
        for (int64_t b = lo; b <= hi; ++b) {
            const int64_t next = p2_first(s, i, b + 1, g.M);
            const int64_t cnt = (next - first) + std::max<int64_t>(0, std::min(next - 1, g.Mneg) - std::max<int64_t>(first, 1) + 1);
            g.wc[b] += w * cnt;
            if (g.r0[b] < 0) g.r0[b] = i;
            ++g.nr[b];
            first = next;
        }
    }
    g.npart = g.off[g.H];
    return MDSP_OK;
}

// ---------------------------------------------------------------- step 2: B (n2, H) = A^T (H, n2), complex
// One 32 x 32 tile per workgroup of 256 threads.  V complex values per global access: 2 for ComplexF32 when H and n2 are even (16-byte
// loads and stores), else 1 (8 bytes ComplexF32, 16 bytes ComplexF64).  The LDS tile is [j][i]; bank conflicts (cdna_hip_programming
// section 2 / Guideline 4 rules):
//   V = 1: rows padded by one element.  Writes (ds_write_b64 / _b128) store contiguous bytes per lane group; the column reads are
//          ds_read_b64 at 66 dwords per row (bank 2 j mod 64: all 64 banks) or ds_read_b128 at 132 (16 distinct 16-byte slots per group).
//   V = 2: rows of 256 bytes, unpadded (ds_write_b128 needs 16-byte aligned rows), the 16-byte slot of (j, i) XOR-swizzled by j / 2: a write
//          group (8 lanes, one row) covers 8 distinct slots = 32 banks.  In the store phase lane l reads rows j, j + 1 (j / 2 = (l / 2) % 16)
//          at column i with i % 2 = l % 2; hipcc merges the two reads into one ds_read2_b64 (16-lane groups, bank mod 32): a group meets
//          8 slots with distinct low three bits, both 8-byte halves of each = 32 banks (as two ds_read_b64: 16 slots x 2 halves = 64).
constexpr int TT = 32;

template <typename R, int V> struct VecOf;
template <> struct VecOf<float, 1> { using T = float2; };
template <> struct VecOf<float, 2> { using T = float4; };
template <> struct VecOf<double, 1> { using T = double2; };

template <int V> __device__ __forceinline__ int tcol(int j, int i) { return V == 1 ? i : ((((i >> 1) ^ (j >> 1)) & 15) << 1) | (i & 1); }

template <typename R, int V>
__global__ __launch_bounds__(256) void transpose_kernel(const cplx<R>* __restrict__ A, cplx<R>* __restrict__ B, int64_t H, int64_t n2, int64_t tiles_i) {
    using VT = typename VecOf<R, V>::T;
    __shared__ __attribute__((aligned(16))) cplx<R> t[TT][TT + (V == 1 ? 1 : 0)];
    const int64_t ti = blockIdx.x % tiles_i, tj = blockIdx.x / tiles_i;
    const int64_t i0 = ti * TT, j0 = tj * TT;
    constexpr int LANES = TT / V, ROWS = 256 / LANES;   // lanes along the contiguous dimension, rows per pass
    const int lane = threadIdx.x % LANES, row = threadIdx.x / LANES;
    {
        const int64_t i = i0 + lane * V;   // V = 2: H is even and i is even, so i < H covers both values
#pragma unroll
        for (int p = 0; p < TT; p += ROWS) {
            const int64_t j = j0 + row + p;
            if (i < H && j < n2) *reinterpret_cast<VT*>(&t[row + p][tcol<V>(row + p, lane * V)]) = *reinterpret_cast<const VT*>(A + i + H * j);
        }
    }
    __syncthreads();
    {
        const int sl = V == 2 ? (threadIdx.x >> 1) & 15 : lane, sr = V == 2 ? ((threadIdx.x >> 5) << 1) | (threadIdx.x & 1) : row;
        const int64_t j = j0 + sl * V;
#pragma unroll
        for (int p = 0; p < TT; p += ROWS) {
            const int64_t i = i0 + sr + p;
            if (i < H && j < n2) {
                VT v;
                cplx<R>* e = reinterpret_cast<cplx<R>*>(&v);
#pragma unroll
                for (int k = 0; k < V; ++k) e[k] = t[sl * V + k][tcol<V>(sl * V + k, sr + p)];
                *reinterpret_cast<VT*>(B + j + n2 * i) = v;
            }
        }
    }
}

// ---------------------------------------------------------------- step 4, ptype 0: out[i + ldo j] from P (N2 x H, ld N2)
// i < H: P[j + N2 i]; i >= H: P[(N2 - j) mod N2 + N2 (N1 - i)] (fft of a real input: X[N1 - i, -j] = conj X[i, j]).  The reads run
// along j (contiguous, descending in the mirrored rows), the writes along i, through a 32 x 33 LDS tile (ds_read_b32 column reads:
// 33 j mod 32 = distinct banks; Float64: 66 dwords per row -> 2 j mod 64).
template <typename R>
__global__ __launch_bounds__(256) void full_kernel(const R* __restrict__ P, R* __restrict__ out, int64_t N1, int64_t N2, int64_t H, int64_t ldo, int64_t tiles_i) {
    __shared__ R t[TT][TT + 1];
    const int64_t ti = blockIdx.x % tiles_i, tj = blockIdx.x / tiles_i;
    const int64_t i0 = ti * TT, j0 = tj * TT;
    const int x = threadIdx.x % TT, y = threadIdx.x / TT;
#pragma unroll
    for (int p = 0; p < TT; p += 256 / TT) {
        const int64_t i = i0 + y + p, j = j0 + x;
        if (i < N1 && j < N2) {
            const bool mirror = i >= H;
            const int64_t src_row = mirror ? N1 - i : i, src_col = mirror ? (j == 0 ? 0 : N2 - j) : j;
            t[y + p][x] = P[src_col + N2 * src_row];
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < TT; p += 256 / TT) {
        const int64_t i = i0 + x, j = j0 + y + p;
        if (i < N1 && j < N2) out[i + ldo * j] = t[x][y + p];
    }
}

// ---------------------------------------------------------------- step 4, ptype 1 / 2: the radial reduction
// R1: one thread per partial e.  Its row i (binary search in off), bin b = lo_i + e - off_i, the m range [first(b), first(b + 1)) of
// that bin; the sum runs m ascending, P[i][m] then its negative twin P[i][N2 - m], in Float64, times the row weight (exact: 1 or 2).
template <typename R>
__global__ __launch_bounds__(256) void radial_rows_kernel(const R* __restrict__ P, const int64_t* __restrict__ off, const int64_t* __restrict__ lo,
                                                          double* __restrict__ part, int64_t npart, int64_t H, int64_t N1, int64_t N2, P2Scale s) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= npart) return;
    int64_t a = 0, z = H;   // last row with off[row] <= e (rows of width 0 share their offset with the next row: take the last)
    while (z - a > 1) {
        const int64_t mid = (a + z) >> 1;
        if (off[mid] <= e) a = mid;
        else z = mid;
    }
    const int64_t i = a, b = lo[i] + (e - off[i]);
    const int64_t M = N2 >> 1, Mneg = (N2 - 1) >> 1;
    const int64_t m0 = p2_first(s, i, b, M), m1 = p2_first(s, i, b + 1, M);
    const R* row = P + N2 * i;
    double acc = 0.0;
    for (int64_t m = m0; m < m1; ++m) {
        acc += (double)row[m];
        if (m >= 1 && m <= Mneg) acc += (double)row[N2 - m];
    }
    part[e] = acc * (double)p2_row_weight(i, H, N1);
}

// R2: one wavefront per bin k (four per workgroup): lane l sums rows r0 + l, r0 + l + 64, ... in order, then a fixed shuffle tree adds the
// 64 lane sums -- the same order on every run; radialavg divides by the wave count (:227-231).
template <typename R>
__global__ __launch_bounds__(256) void radial_bins_kernel(const double* __restrict__ part, const int64_t* __restrict__ off, const int64_t* __restrict__ lo,
                                                          const int64_t* __restrict__ r0, const int64_t* __restrict__ nr, const int64_t* __restrict__ wc,
                                                          R* __restrict__ out, int64_t kmax, int avg) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= kmax) return;   // wave-uniform: the whole wave has the same k
    double acc = 0.0;
    for (int64_t i = r0[k] + lane, e = r0[k] + nr[k]; i < e; i += 64) acc += part[off[i] + (k - lo[i])];
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_down(acc, sh, 64);
    if (lane == 0) out[k] = (R)(avg ? acc / (double)wc[k] : acc);
}

}  // namespace

struct mdsp_periodogram2_plan_s {
    int64_t n1 = 0, n2 = 0, N1 = 0, N2 = 0, H = 0, kmax = 0, npart = 0;
    int ptype = 0, dtype = 0, engine = MDSP_ENGINE_AUTO;
    mdsp_stft_plan rows = nullptr, cols = nullptr;   // owned here, not borrowed from the plan cache
    DevBuf ap;     // A (H x n2 complex), then P (N2 x H real): A is dead once B exists
    DevBuf bt;     // B (n2 x H complex)
    DevBuf part;   // radial: Float64 row partials
    DevBuf tab;    // radial: off (H + 1), lo (H), r0, nr, wc (kmax each), int64
    ~mdsp_periodogram2_plan_s() {
        if (rows) mdsp_stft_plan_destroy(rows);
        if (cols) mdsp_stft_plan_destroy(cols);
    }
};

namespace {

template <typename R> int p2_exec(mdsp_periodogram2_plan pl, const void* s_dev, int64_t lds_, void* out_dev, int64_t ldo, hipStream_t st) {
    using C = cplx<R>;
    const int64_t n1 = pl->n1, n2 = pl->n2, N1 = pl->N1, N2 = pl->N2, H = pl->H;
    constexpr int64_t CH = 65535;   // channels per mdsp_stft_exec call
    C* A = pl->ap.as<C>();
    R* P = pl->ap.as<R>();
    C* B = pl->bt.as<C>();
    // 1. rows: column c of s -> column c of A
    for (int64_t c0 = 0; c0 < n2; c0 += CH) {
        const int64_t nc = std::min(CH, n2 - c0);
        MDSP_TRY(mdsp_stft_exec(pl->rows, static_cast<const R*>(s_dev) + c0 * lds_, n1, nc, lds_, A + c0 * H, H, H, st));
    }
    // 2. transpose
    {
        const int64_t tiles_i = cdiv(H, TT), tiles = tiles_i * cdiv(n2, TT);
        if (tiles > INT32_MAX) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "2-D periodogram too large");
        bool vec2 = false;
        if constexpr (sizeof(R) == 4) {
            vec2 = H % 2 == 0 && n2 % 2 == 0;
            if (vec2) hipLaunchKernelGGL((transpose_kernel<R, 2>), dim3((unsigned)tiles), dim3(256), 0, st, A, B, H, n2, tiles_i);
        }
        if (!vec2) hipLaunchKernelGGL((transpose_kernel<R, 1>), dim3((unsigned)tiles), dim3(256), 0, st, A, B, H, n2, tiles_i);
        MDSP_LAUNCH_CHECK();
    }
    // 3. columns: column i of B (n2 points) -> row i of P (N2 bins)
    for (int64_t c0 = 0; c0 < H; c0 += CH) {
        const int64_t nc = std::min(CH, H - c0);
        MDSP_TRY(mdsp_stft_exec(pl->cols, B + c0 * n2, n2, nc, n2, P + c0 * N2, N2, N2, st));
    }
    // 4. epilogue
    R* out = static_cast<R*>(out_dev);
    if (pl->ptype == 0) {
        const int64_t tiles_i = cdiv(N1, TT), tiles = tiles_i * cdiv(N2, TT);
        if (tiles > INT32_MAX) MDSP_FAIL(MDSP_ERR_UNSUPPORTED, "2-D periodogram too large");
        hipLaunchKernelGGL(full_kernel<R>, dim3((unsigned)tiles), dim3(256), 0, st, P, out, N1, N2, H, ldo, tiles_i);
        MDSP_LAUNCH_CHECK();
        return MDSP_OK;
    }
    const int64_t* off = pl->tab.as<int64_t>();
    const int64_t *lo = off + (H + 1), *r0 = lo + H, *nr = r0 + pl->kmax, *wc = nr + pl->kmax;
    double* part = pl->part.as<double>();
    if (pl->npart > 0) {
        hipLaunchKernelGGL(radial_rows_kernel<R>, dim3((unsigned)cdiv(pl->npart, 256)), dim3(256), 0, st, P, off, lo, part, pl->npart, H, N1, N2, p2_scale(N1, N2));
        MDSP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(radial_bins_kernel<R>, dim3((unsigned)cdiv(pl->kmax, 4)), dim3(256), 0, st, part, off, lo, r0, nr, wc, out, pl->kmax, pl->ptype == 2 ? 1 : 0);
    MDSP_LAUNCH_CHECK();
    return MDSP_OK;
}

}  // namespace

extern "C" {

int mdsp_periodogram2_geometry_for(int64_t nfft1, int64_t nfft2, int64_t* kmax, int64_t* wc_host, int64_t* partials) {
    P2Geom g;
    MDSP_TRY(p2_geometry(nfft1, nfft2, g));
    if (kmax) *kmax = g.kmax;
    if (wc_host) std::copy(g.wc.begin(), g.wc.end(), wc_host);
    if (partials) *partials = g.npart;
    return MDSP_OK;
}

int mdsp_periodogram2_plan_create(mdsp_periodogram2_plan* plan, int64_t n1, int64_t n2, int64_t nfft1, int64_t nfft2, double fs, int ptype, int dtype,
                                  int engine) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    *plan = nullptr;
    // the reference's checks, in its order (:477-487), then what this entry adds
    if (!(n1 <= nfft1 && n2 <= nfft2)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "nfft must be >= size(s)");
    if (!(n1 > 1 && n2 > 1)) MDSP_FAIL(MDSP_ERR_ARGUMENT, "dimensions of s must be > 1");
    if (ptype < 0 || ptype > 2) MDSP_FAIL(MDSP_ERR_ARGUMENT, "invalid ptype %d (0 full, 1 radialsum, 2 radialavg)", ptype);
    if (dtype != MDSP_F32 && dtype != MDSP_F64) MDSP_FAIL(MDSP_ERR_ARGUMENT, "the 2-D periodogram takes a real matrix (dtype %d)", dtype);
    const double r = fs * (double)n1 * (double)n2;   // norm2 = length(s), not prod(nfft) (:488)
    auto pl = new mdsp_periodogram2_plan_s();
    pl->n1 = n1;
    pl->n2 = n2;
    pl->N1 = nfft1;
    pl->N2 = nfft2;
    pl->H = nfft1 / 2 + 1;
    pl->ptype = ptype;
    pl->dtype = dtype;
    const size_t rsz = dtype_size(dtype), csz = 2 * rsz;
    int st = mdsp_stft_plan_create(&pl->rows, n1, 0, nfft1, nullptr, 1.0, 1, 0, dtype, engine);
    if (st == MDSP_OK) st = mdsp_stft_plan_create(&pl->cols, n2, 0, nfft2, nullptr, r, 0, 1, dtype_complex_of(dtype), engine);
    if (st == MDSP_OK) st = pl->ap.reserve(std::max((size_t)pl->H * (size_t)n2 * csz, (size_t)pl->H * (size_t)nfft2 * rsz));
    if (st == MDSP_OK) st = pl->bt.reserve((size_t)pl->H * (size_t)n2 * csz);
    if (st == MDSP_OK) {
        int e1 = 0, e2 = 0;
        mdsp_stft_plan_info(pl->rows, nullptr, &e1);
        mdsp_stft_plan_info(pl->cols, nullptr, &e2);
        pl->engine = e1 == e2 ? e1 : MDSP_ENGINE_AUTO;
    }
    if (st == MDSP_OK && ptype != 0) {
        P2Geom g;
        st = p2_geometry(nfft1, nfft2, g);
        if (st == MDSP_OK) {
            pl->kmax = g.kmax;
            pl->npart = g.npart;
            std::vector<int64_t> t;
            t.reserve(2 * g.H + 1 + 3 * g.kmax);
            for (const auto* v : {&g.off, &g.lo, &g.r0, &g.nr, &g.wc}) t.insert(t.end(), v->begin(), v->end());
            st = pl->tab.reserve(t.size() * sizeof(int64_t));
            if (st == MDSP_OK && hipMemcpy(pl->tab.p, t.data(), t.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
                st = set_error(MDSP_ERR_DEVICE, "radial table upload failed");
            if (st == MDSP_OK) st = pl->part.reserve(std::max<int64_t>(g.npart, 1) * sizeof(double));
        }
    }
    if (st != MDSP_OK) {
        delete pl;
        return st;
    }
    *plan = pl;
    return MDSP_OK;
}

int mdsp_periodogram2_plan_destroy(mdsp_periodogram2_plan plan) {
    delete plan;
    return MDSP_OK;
}

int mdsp_periodogram2_plan_info(mdsp_periodogram2_plan plan, int64_t* nout, int64_t* workspace_bytes, int* engine_used) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (nout) *nout = plan->ptype == 0 ? plan->N1 * plan->N2 : plan->kmax;
    if (workspace_bytes) *workspace_bytes = (int64_t)(plan->ap.bytes + plan->bt.bytes + plan->part.bytes + plan->tab.bytes);
    if (engine_used) *engine_used = plan->engine;
    return MDSP_OK;
}

int mdsp_periodogram2_exec(mdsp_periodogram2_plan plan, const void* s_dev, int64_t lds_, void* out_dev, int64_t ldo, void* stream) {
    if (!plan) MDSP_FAIL(MDSP_ERR_ARGUMENT, "plan is NULL");
    if (!s_dev || !out_dev) MDSP_FAIL(MDSP_ERR_ARGUMENT, "NULL buffer");
    if (lds_ < plan->n1) MDSP_FAIL(MDSP_ERR_DIMENSION, "column stride of s (%lld) smaller than size(s, 1) (%lld)", (long long)lds_, (long long)plan->n1);
    if (plan->ptype == 0 && ldo < plan->N1)
        MDSP_FAIL(MDSP_ERR_DIMENSION, "column stride of out (%lld) smaller than nfft[1] (%lld)", (long long)ldo, (long long)plan->N1);
    hipStream_t st = as_stream(stream);
    return dtype_is_double(plan->dtype) ? p2_exec<double>(plan, s_dev, lds_, out_dev, ldo, st) : p2_exec<float>(plan, s_dev, lds_, out_dev, ldo, st);
}

}  // extern "C"
