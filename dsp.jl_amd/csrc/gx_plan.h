// What a Welch / STFT plan keeps for the run-time-schedule spectral kernel (spectral_gx.h): the schedule, the split nfft = R0 x S, the root tables
// and the window in working precision.  Built at plan creation (gx_prepare); columns convert their launch's window into `win`.
#pragma once

#include "common.h"
#include "gx_sched.h"

namespace mdsp {
struct GxPlan {
    gx::Sched sc;
    int R0 = 1, nhs = 0, nhn = 0;
    size_t lds_bytes = 0;
    DevBuf tw, win;
};
}  // namespace mdsp
