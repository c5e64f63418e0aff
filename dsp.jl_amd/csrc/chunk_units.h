// Units per chunk of every engine loop that cuts its work to a memory budget: each loop calls the function of its kind, and mdsp_chunk_units_for
// (api_core.hip) answers with the same functions under the tunables as they stand -- host arithmetic, so that a test can hold its shapes to the seams
// it means to cross.  rsz: bytes of a real of the working precision (4 / 8); `units` is what the loop walks; never less than one unit per chunk.
// Internal to the library.
#pragma once

#include <algorithm>
#include <cstdint>

namespace mdsp {

// rocFFT Welch / STFT (welch.hip welch_accumulate_rocfft, stft.hip stft_exec_rocfft): a unit is one frame of one channel -- nfft windowed samples
// and its nspec bins; budget: rocfft_chunk_bytes()
inline int64_t chunk_units_rocfft_spectral(bool cplx, int64_t rsz, int64_t nfft, int64_t units, int64_t budget) {
    const int64_t nspec = cplx ? nfft : nfft / 2 + 1;
    const int64_t per_unit = (cplx ? 2 : 1) * rsz * nfft + 2 * rsz * nspec;
    return std::max<int64_t>(1, std::min<int64_t>(units, budget / per_unit));
}

// rocFFT overlap-save (ols.hip exec_rocfft): a unit is one block of one column; td + fd stay cache resident (~64 MiB)
inline int64_t chunk_units_rocfft_ols(bool cplx, int64_t rsz, int64_t nfft, int64_t units) {
    const int64_t nspec = cplx ? nfft : nfft / 2 + 1;
    const int64_t per_unit = (cplx ? 2 : 1) * rsz * nfft + (cplx ? 0 : 2 * rsz * nspec);
    return std::max<int64_t>(1, std::min<int64_t>(units, (int64_t(64) << 20) / per_unit));
}

// hilbert (hilbert.hip hilbert_run): a unit is one column of n points; the intermediates of a batch stay within ~256 MiB
inline int64_t chunk_units_hilbert(int64_t rsz, int64_t n, int64_t units) {
    const int64_t nspec = n / 2 + 1;
    const int64_t per_col = rsz * n + 2 * rsz * (nspec + n);
    return std::max<int64_t>(1, std::min<int64_t>(units, (int64_t(256) << 20) / per_col));
}

// multi-pass engine (bigfft.hip): a unit is one transform of nfft complex points (two real frames or blocks, one complex); `buffers` work buffers
// of that size per unit share the budget (run_ols: two, everything else: one)
inline int64_t chunk_units_big(int64_t rsz, int64_t nfft, int64_t units, int64_t budget, int buffers) {
    const int64_t per = 2 * rsz * nfft;
    return std::max<int64_t>(1, std::min<int64_t>(units, budget / (buffers * per)));
}

}  // namespace mdsp
