// The overlap-save plan object (opaque behind the C ABI), shared by ols.hip (kernels) and hostpath.hip (host-pointer pipeline).
#pragma once

#include "common.h"
#include "rocfft_wrap.h"
#include "bigfft.h"

struct mdsp_ols_plan_s {
    int dtype = MDSP_F32, mode = MDSP_OLS_FILT, engine = MDSP_ENGINE_ROCFFT;
    int64_t nb = 0, nfft = 0, L = 0;      // nfft / L: the geometry that EXECUTES (== the reference's unless the fused engine re-blocked a long filter)
    int64_t ref_nfft = 0, ref_L = 0;     // what the caller / optimalfftfiltlength asked for (plan_info, mdsp_ols_segment: the reference's tmp1 blocks)
    // What the whole-column call and the host pipeline execute: windows of `tile` outputs that start tile_lead samples in front of their first
    // output.  Everywhere tile == L and tile_lead == nb - 1, except real Float32 plans of 249 .. 257 taps at nfft 2048 on the fused engine (`tiled`): 1792
    // outputs per window and 256 samples of lead, so every window starts a multiple of 1 KiB into a line-aligned column and the overlap of consecutive
    // blocks is whole per-thread elements.  The spectrum does not change (the taps past nb are zero either way); the public block grid (L) does not move.
    int64_t tile = 0, tile_lead = 0;
    bool tiled = false;
    int partitions = 1;                  // > 1: uniformly partitioned overlap-save (upols_fused_kernel): nfft = 2 B, `partitions` spectra in H
    mdsp::DevBuf H;       // rocFFT engine: nspec (real) or nfft (complex) entries; fused: nfft entries
    mdsp::DevBuf table;   // fused: nfft forward roots
    // rocFFT engine state
    mdsp::RocPlan fwd, inv;
    mdsp::DevBuf td, fd;
    int64_t batch = 0;
    int variant = 0;  // partitioned plans: kernel form (tuning knob, MDSP_OLS_VARIANT)
    // filters beyond the partitioned kernels: blocks of nfft = 8 .. 16 nb points on the multi-pass engine (bigfft.hip), H = nfft entries, natural order
    bool big = false;
    int big_rows = 0;                    // > 0: H is row-major for the rows form of that engine (R0 rows: bigfft.h ols_rows_r0)
    mdsp::big::EngineHolder bigeng;
};

namespace mdsp {
// The footprint rule of the tiled kernel's streaming cache policy (AUXL / AUXS of ols_fused_kernel).  A streaming policy is right only when
// nothing the launch touches can still be in cache for its consumer: the streaming instantiation runs when the bytes the launch reads plus the bytes it
// writes exceed 512 MiB, twice the Infinity Cache (measured: at exactly 512 MiB streaming lost one round of sixteen), the plain one up to that -- small signals, the chunks of mdsp_ols_exec_host.  `knob` is MDSP_OLS_STREAM, read
// at launch: 1 this rule, 0 always plain, 2 always streaming (tests, A/B).  Only tiled launches have a streaming instantiation.
constexpr int64_t kOlsStreamBytes = int64_t(512) << 20;
inline bool ols_stream_rule(int knob, bool tiled, int64_t nread, int64_t nwritten, int64_t columns, int64_t elem_bytes) {
    if (!tiled || knob == 0) return false;
    if (knob == 2) return true;
    return (nread + nwritten) * columns * elem_bytes > kOlsStreamBytes;
}

// The run schedule of the fused kernel's persistent grid (DESIGN 4.2 *Run schedule*; ols.hip launch_fused_geo).  Slot s of `nslots` walks runs of run_len
// consecutive units, run r of slot s at unit (r nslots + s) run_len, every slot the same niter = rounds x run_len iterations (barriers inside).  "Whole"
// is one run per slot, run_len = ceil(units / nslots): every workgroup streams one contiguous piece, the chunked pattern of a copy.  Short runs keep all
// slots inside one moving window of nslots x run_len units, the interleaved pattern.  ols_run_rule answers kOlsRunUnits for the streaming tiled launch
// (`streaming_tiled`: ols_stream_rule said yes) of at least kOlsRunFromUnits units and whole for every other one -- smaller streaming launches, plain
// tiled, untiled, block ranges, the rows form, Float64, complex --, which keep the schedule they had.  Never longer than whole, never shorter than 1.
// Measured at 2^30 samples (profiles/ols_runs_ab.json): the memory side alone 1.673 ms whole, 1.617 / 1.599 / 1.614 / 1.634 / 1.655 ms at runs of
// 1 / 2 / 4 / 8 / 16 units, each below whole in all six rounds, 32 and 73 above it; 2 below 1 and 4 in every round.  The line: runs of 2 lost no round
// against whole at 2^28 and 2^30 samples (74899 and 299594 units); at 2^27 (37450 units, 37 per slot, where the one iteration more is 2.7 %) they are
// 5 % faster once the chip is warm and 3 % slower in the first rounds of a process that starts there -- so the smallest power of two above it.
// Padding: ceil(ceil(units / run_len) / nslots) == ceil(units / (run_len nslots)), so niter is the smallest multiple of run_len that is >= whole:
// at most run_len - 1 iterations more than whole's, none at run_len == 1; a slot idles through at most one run (the last round's), as with whole.
// `forced` (knob MDSP_OLS_RUN_LEN, tests and the A/B): > 0 this length for every fused launch; `runs_per_slot` (knob MDSP_RUNS_PER_SLOT) != 1 wins over both.
constexpr int64_t kOlsRunUnits = 2, kOlsRunFromUnits = int64_t(1) << 16;
inline int64_t ols_run_whole(int64_t units, int64_t nslots) { return std::max<int64_t>(1, cdiv(units, std::max<int64_t>(1, nslots))); }
inline int64_t ols_run_rule(int64_t units, int64_t nslots, bool streaming_tiled) {
    const int64_t whole = ols_run_whole(units, nslots);
    return streaming_tiled && units >= kOlsRunFromUnits ? std::min(whole, kOlsRunUnits) : whole;
}
inline int64_t ols_run_len(int64_t units, int64_t nslots, bool streaming_tiled, int runs_per_slot, int forced) {
    if (runs_per_slot != 1) return std::max<int64_t>(1, cdiv(units, std::max<int64_t>(1, nslots) * runs_per_slot));
    if (forced > 0) return std::min<int64_t>(forced, ols_run_whole(units, nslots));
    return ols_run_rule(units, nslots, streaming_tiled);
}
inline int64_t ols_run_niter(int64_t units, int64_t nslots, int64_t run_len) { return cdiv(cdiv(units, run_len), std::max<int64_t>(1, nslots)) * run_len; }

// Tiles [first_tile, first_tile + ntiles) of the grid the whole-column call runs for one column of nx samples / nout outputs, from a slice of the signal:
// xs_dev holds x[xs_first .. xs_first + xs_len) and covers [first_tile tile - tile_lead, (first_tile + ntiles) tile) clipped to [0, nx); ys_dev[0..] receives
// the outputs from first_tile tile on.  first_tile even for real dtypes on single-block plans.  Bit-identical to the whole-column call (mdsp_ols_exec_host).
int ols_exec_tiles(mdsp_ols_plan_s* plan, const void* xs_dev, int64_t xs_first, int64_t xs_len, int64_t nx, void* ys_dev, int64_t first_tile, int64_t ntiles,
                   int64_t nout, hipStream_t stream);
}  // namespace mdsp
