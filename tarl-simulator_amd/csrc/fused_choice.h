// fused_choice.h — the per-frame action draw as device code: the one piece two translation units need (k_fused_choice in
// fused_choice.hip, the choice role of k_fused_insert_choice in fused_insert.hip).
#pragma once
#include "fused_frame.h"

// ---- choice phase (env-minor: lane = environment, a workgroup walks a chunk of nodes) --------------------------------
// Consecutive nodes of one environment share Philox blocks (index = b*G + g), so a chunk costs ~nchunk/4 + 1 Philox
// evaluations per lane instead of one per node. The action AND the new SELECTED_ROAD are one byte per (node, env): the
// rank of the chosen out-edge (sel_out); a node that draws nothing (no out-edges, or u beyond the last threshold through
// rounding) carries its previous code over from sel_prev with SEL_CARRIED set.
__device__ __forceinline__ void fused_choice_body(unsigned bx, unsigned by, const int32_t* __restrict__ out_ptr,
                                                  const int32_t* __restrict__ out_eid,
                                                  const int32_t* __restrict__ group_of_node, int64_t G, int64_t B,
                                                  int64_t N, long long* __restrict__ acc_lp, int64_t acc_slots,
                                                  const float* __restrict__ thr, const long long* __restrict__ lgt,
                                                  const float* __restrict__ uniform, uint64_t pseed, uint64_t pcounter,
                                                  uint8_t* __restrict__ sel_out, const uint8_t* __restrict__ sel_prev,
                                                  int32_t* __restrict__ choice, int nchunk, int want_lp,
                                                  int64_t env_base) {
  const int64_t b = (int64_t)bx * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int32_t i0 = by * nchunk;
  const int32_t i1 = (i0 + nchunk < N) ? i0 + nchunk : (int32_t)N;
  long long lp = 0;
  bool bad = false;
  PhiloxRun rng;
  for (int32_t i = i0; i < i1; ++i) {
    const int64_t row = (int64_t)i * B + b;
    int32_t ch = -1;
    uint32_t code = SEL_RAW;
    bool found = false;
    const int32_t gi = group_of_node[i];
    if (gi >= 0) {
      const float u = uniform ? uniform[b * G + gi] : rng.uniform(pseed, pcounter, (uint64_t)((env_base + b) * G + gi));
      // first out-edge (plan order) whose threshold exceeds u. Every table operand is wave-uniform (scalar loads), the
      // per-lane part is compare + select: no dependent vector gathers
      long long lpn = 0;
      const int32_t k0 = out_ptr[i], k1 = out_ptr[i + 1];
      for (int32_t k = k0; k < k1; ++k) {
        const bool hit = !found && (u < thr[k]);
        const long long lgk = lgt[k];
        code = hit ? (uint32_t)(k - k0) : code;
        ch = hit ? out_eid[k] : ch;
        lpn = hit ? lgk : lpn;
        found = found || hit;
      }
      if (found) lp += lpn; else bad = true;
    }
    if (!found) code = (sel_prev[row] & 0x7Fu) | SEL_CARRIED;   // keeps its previous SELECTED_ROAD
    sel_out[row] = (uint8_t)code;
    if (choice) __builtin_nontemporal_store(ch, &choice[row]);  // frame API: the action as an edge id (-1: none)
  }
  // infeasible action (some node picked nothing): poison the accumulator far beyond any legitimate sum
  if (want_lp)
    atomicAdd((unsigned long long*)&acc_lp[(int64_t)(by % (unsigned)acc_slots) * B + b],
              (unsigned long long)(bad ? -(1ll << 50) : lp));  // up to 2^13 chunks cannot wrap
}
