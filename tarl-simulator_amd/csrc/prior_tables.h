// prior_tables.h — internal: what the heads that read the shortest-path tables share (prior.hip, goal_mlp.hip): the sentinel of
// an unreachable candidate, the two table lookups and the congested travel time of a road. fp32, the reference's operation
// order (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#define PRIOR_UNREACHABLE (-1e20f)

// time_travel(v) = max(FF, FF * (MAXN + 10 - MAX_FLOW * FF / 3600) / (MAXN + 10 - NUMBER_OF_AGENT))   (of road v)
__device__ __forceinline__ float prior_time_travel(float ff, float maxn, float maxflow, float na) {
  const float crit = maxflow * ff / 3600.0f;                             // critical_number (:182)
  const float tc = ff * (maxn + 10.0f - crit) / (maxn + 10.0f - na);     // time_congestion (:183)
  const float tt = (ff != ff || tc != tc) ? NAN : fmaxf(ff, tc);         // torch.max over the stack (:184)
  return tt;
}

// dist[v][dest]: the N x N all-pairs table
struct PriorAllPairs {
  const float* __restrict__ dist;
  int64_t N;
  __device__ __forceinline__ float operator()(int64_t v, float dest_f) const {
    const long long d = (long long)dest_f;                 // agent_destination.to(torch.long) (:186)
    return (d >= 0 && d < N) ? dist[v * N + d] : INFINITY;
  }
};

// table[v][slot[dest]]: the [N][D] per-destination table; no column -> unreachable
struct PriorPerDest {
  const float* __restrict__ table;
  const int32_t* __restrict__ slot;
  int64_t N, D;
  __device__ __forceinline__ float operator()(int64_t v, float dest_f) const {
    const long long d = (long long)dest_f;
    if (d < 0 || d >= N) return INFINITY;
    const int32_t s = slot[d];
    return (s >= 0 && s < D) ? table[v * D + s] : INFINITY;
  }
};
