// Matrix-core polyphase kernel (fir_mm.hip): the predicate, the tile geometry (mdsp_fir_mm_geometry and mdsp_fir_kernel_path report it) and the run function.
// Internal to the library.
#pragma once

#include "fir_plan.h"

namespace mdsp {
// Shapes it is built for: Float32 taps x Float32 / ComplexF32 signals, and Float64 arithmetic on Float64 / ComplexF64 signals; L <= 1024,
// a tile that fits the LDS.  Up to 12 column blocks (L <= 192) and 256 (Float64: 128) window positions per block the taps of a wave's block
// live in registers; beyond either, a wave fetches the taps of its block(s) from L2 for every tile.
// For L < 16 a row of the product is RB whole rounds (Lr = RB L <= 16 consecutive outputs, Mr = RB M samples): the columns of a
// row still repeat their phases from row to row, which is all the kernel needs; RB is chosen so that rows (lane stride Mr samples)
// spread over the LDS banks (odd Mr: conflict-free).
struct FirMGeo {
    bool ok = false;
    int esz = 4, CS = 1, CH = 4;   // bytes of R; parts per sample; 16-row chunks per multiplying wave
    int RB = 1, Lr = 0, Mr = 0, NB = 0, NBW = 0, NG = 1, T = 0, steps = 0, Lp = 0, nd = 1, ns = 1;   // T = 0: `steps` k-steps with the taps fetched per tile
    int NBLK = 1;                  // column blocks per multiplying wave whose taps ALL live in registers (L > 192 with T = 12 / 16; else 1)
    int64_t bufsz = 0;             // dwords per sample buffer
    int pitch = 0;                 // dwords between separately staged rows (0: one linear run per tile)
    int rowpad = 0;                // dwords of padding behind every 256-dword granule of a linear run (0: none)
    size_t lds_bytes = 0;
};
#pragma GCC visibility push(hidden)
FirMGeo fir_mm_geo(const mdsp_fir_s* f);
bool fir_mm_use(const mdsp_fir_s* f, const FirArgs& a);
int fir_mm_dispatch(mdsp_fir_s* f, const FirArgs& a, hipStream_t st);
#pragma GCC visibility pop
}  // namespace mdsp
