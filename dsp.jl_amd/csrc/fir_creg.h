// Register-tap polyphase kernel for COMPLEX taps (fir_creg.hip): the structure of fir_reg.hip with (re, im) tap pairs in registers.  The signal stays in
// its own class in LDS (a real signal is staged as reals: half the LDS per tile), converted to the arithmetic precision as it is staged.  Internal to the
// library; args are fir_reg.h's FirRegArgs with pfbT holding tp * L complex taps of the arithmetic precision.
#pragma once

#include "fir_reg.h"

namespace mdsp {
// true: a complex-tap register instantiation exists for (x_dtype, double arithmetic?, taps per phase, L, M); everything else takes the generic kernel
bool fir_creg_ok(int x_dtype, bool acc_double, int64_t tp, int64_t L, int64_t M);
int fir_creg_run(int x_dtype, bool acc_double, FirRegArgs& a, int64_t nch, hipStream_t st);
}  // namespace mdsp
