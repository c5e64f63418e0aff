// Decimator kernel (fir_dec.hip; L = 1, M <= 64, any filter length): the geometry, whose `ok` is the predicate, and the run function.
// Internal to the library.
#pragma once

#include "fir_plan.h"

namespace mdsp {
struct DecGeo {
    bool ok = false;
    int Mp = 0, logMp = 0, nq = 0, nbh = 0, nz = 0, P = 0;
    size_t lds = 0;
};
#pragma GCC visibility push(hidden)
DecGeo fir_dec_geo(const mdsp_fir_s* f);
int fir_dec_dispatch(mdsp_fir_s* f, const FirArgs& a, const DecGeo& g, hipStream_t st);
#pragma GCC visibility pop
}  // namespace mdsp
