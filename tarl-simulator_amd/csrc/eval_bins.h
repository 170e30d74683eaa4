// eval_bins.h — the frame-to-bin schedule of the evaluation's per-frame accumulators (link_counts.hip, occupancy.hip):
// frame f of a call starts at clock t0 + f * timestep and belongs to the stored bin h = clock / bin_seconds - first_bin.
#pragma once
#include "tarl_common.h"

// The run [f, f1) of frames in frame f's bin h -> f1: two divisions per run, uniform over the launch (scalar arithmetic).
__device__ __forceinline__ int64_t bin_run(int64_t t0, int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t f,
                                           int64_t F, int64_t& h) {
  const int64_t bin = (t0 + f * timestep) / bin_seconds;
  h = bin - first_bin;
  // timestep > 0: the first frame at or past the bin's upper edge, > f, because frame f lies below that edge; 0: all the rest
  const int64_t f1 = timestep > 0 ? ((bin + 1) * bin_seconds - t0 + timestep - 1) / timestep : F;
  return f1 < F ? f1 : F;
}

// Host: the first and the last frame's bin are in [0, H) and timestep >= 0, so every h in between is too. (A macro: it
// returns from the entry point, which TARL_REQUIRE names.)
#define TARL_REQUIRE_BINS(t0, dt, bs, fb, F, H)                                                                          \
  do {                                                                                                                   \
    const int64_t lim_ = (int64_t)1 << 40;                                                                               \
    TARL_REQUIRE((t0) >= 0 && (t0) < lim_ && (dt) >= 0 && (dt) < lim_ && (fb) >= 0, "bad clock");                        \
    TARL_REQUIRE((bs) >= 1 && (bs) < lim_, "bin_seconds must be positive");                                              \
    TARL_REQUIRE((t0) / (bs) - (fb) >= 0, "bin out of range: the first frame falls below first_bin");                    \
    TARL_REQUIRE(((t0) + ((F)-1) * (dt)) / (bs) - (fb) < (H), "bin out of range: the last frame falls in a bin >= H");   \
  } while (0)
