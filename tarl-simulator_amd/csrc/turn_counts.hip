// turn_counts.hip — per-turn movement counts of the vectorised evaluation: how many vehicles crossed each route edge
// u -> v per (environment, time bin), and how many agents the reference's U-turn double pop (DESIGN quirk Q24) lost on
// which road, from what tarl_fused_frame already offers per frame: the popped mask, the SELECTED_ROAD byte and the
// NUMBER_OF_AGENT column.
//
// Reference semantics restated: DirectionMPNN.aggregate (src/direction_mpnn.py) picks per road v ONE in-edge e = (u -> v)
// by a Gumbel race over the upstream heads that selected v; where the chosen agent id is not 0 that head enters v in this
// frame: moved_t[e]. ResponseMPNN (src/response_mpnn.py) then pops every road u one of whose out-edges (u -> v) was
// accepted: v's new tail came from u. Q24: an agent that moves from v into an EMPTY road u, where the edge u -> v exists
// too, is accepted on both edges; u is popped although nothing left it, and the agent is gone. With n_pre[u] the
// NUMBER_OF_AGENT of u BEFORE the frame (the `counts` slice of the frame before; 0 after a reset), popped_t the frame's
// mask and sel8_t the packed SELECTED_ROAD byte the frame ran with:
//   moved_t[e]   <=>  popped_t[u] & 1  and  n_pre[u] > 0  and  (sel8_t[u] & 0x7F) == rank of e in u's CSR out-list
//   phantom_t[u] <=>  popped_t[u] & 1  and  not n_pre[u] > 0      (NaN counts as empty: the convention of oc_count)
//   a popped, non-empty road whose code names no out-edge (0x7F, 0x7E, rank >= out-degree) is unresolved.
// Every popped bit lands in exactly one of the three tables.
#include "eval_bins.h"

#define TC_ENVS 64                      // environments of one workgroup's tile: the lanes of a wave
#define TC_ROADS 16                     // roads of the tile: one per wave
#define TC_CHUNK 8                      // frames staged between two barriers
#define TC_MAX_FRAMES ((int64_t)1 << 23)

// One workgroup of 16 waves owns a tile of 64 environments x 16 roads for every frame and every bin; thread (wave w, lane l)
// owns the pair (environment k0 + l, road n0 + w) and is the only writer of lost[k][.][u] and of turns[k][.][e] for the
// out-edges e of its road u (an edge has one source): plain read-modify-write, no atomics, and integer sums do not depend
// on an order. The road is uniform over the wave: its CSR bounds are read once, through the scalar cache.
//   popped is the transposed input ([F][K][N], env-major). Per chunk of up to 8 frames of one bin, lane l of wave w reads
//   the byte of (environment k0 + 4 w + l / 16, road n0 + l % 16): four environments' 16 consecutive road bytes per wave
//   and frame, the 8 loads of a chunk independent and in flight together. __ballot of bit 0 is those four environments'
//   road masks, 16 bits each: one 64-bit word in LDS, s_mask[frame][w]. After the barrier lane l reads the word of its
//   environment, s_mask[c][l / 4] (ds_read_b64, 16 consecutive words, four lanes share one: conflict-free), and tests the
//   bit of its road. Byte loads, so a ring that starts at any address is read as it is.
//   sel8 and counts are env-minor ([F][N][K]): the lanes of a wave run along the environment axis, as in occupancy.hip.
//   They are read only where the popped bit is set: pops are sparse (about 2 % of the (road, frame) pairs at BASELINE
//   config 4), so the kernel's traffic is the popped bytes plus the cache lines the events touch. What bounds the kernel
//   is latency, not bytes: an event is a chain of three dependent global accesses ({count before, SELECTED_ROAD byte} ->
//   edge id -> the table's read-modify-write), and the frames of an element are in sequence in its single writer. So a
//   thread owns ONE road (as many waves as the shape allows), and the chunk's 8 frames go through the chain together:
//   all their first loads, then all their edge ids, then the read-modify-writes in frame order.
// Tiles at the K and N edges are partial: a byte outside [K][N] is not loaded and enters the ballot as 0, so no thread
// ever sees an event for an element that does not exist; every other access is reached only through such an event.
// unresolved[k] has no single owner (any road of environment k may add to it). It must be 0 on every graph the fused
// path accepts and the evaluator raises when it is not, so that one, never-taken path uses an integer atomicAdd.
__global__ __launch_bounds__(TC_ENVS* TC_ROADS) void k_turn_counts_accumulate(
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_eid, const uint8_t* __restrict__ popped,
    const uint8_t* __restrict__ sel8, const float* __restrict__ counts, const float* __restrict__ prev_counts, int64_t F,
    int64_t K, int64_t N, int64_t E, int64_t H, int64_t t0, int64_t timestep, int64_t bin_seconds, int64_t first_bin,
    int64_t k_tiles, int32_t* __restrict__ turns, int32_t* __restrict__ lost, int32_t* __restrict__ unresolved) {
  __shared__ uint64_t s_mask[TC_CHUNK][TC_ROADS];
  const int l = threadIdx.x & (TC_ENVS - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / TC_ENVS);
  const int64_t k0 = ((int64_t)blockIdx.x % k_tiles) * TC_ENVS, n0 = ((int64_t)blockIdx.x / k_tiles) * TC_ROADS;
  // staging side: this lane's byte of a frame's popped slice, if it exists
  const int64_t ks = k0 + 4 * w + (l >> 4), ns = n0 + (l & 15);
  const bool s_in = ks < K && ns < N;
  const int64_t s_off = ks * N + ns;
  // event side: this thread's (environment, road); an event exists only where both do
  const int64_t k = k0 + l, u = n0 + w;
  const int bit = ((l & 3) << 4) + w;
  const int32_t o0 = u < N ? out_ptr[u] : 0, deg = u < N ? out_ptr[u + 1] - o0 : 0;
  const int64_t i = u * K + k;      // its element of an env-minor slice
  for (int64_t f = 0; f < F;) {
    int64_t h;
    const int64_t f1 = bin_run(t0, timestep, bin_seconds, first_bin, f, F, h);      // the run [f, f1) of frames in bin h
    int32_t* const lost_e = lost + (k * H + h) * N + u;
    int32_t* const turns_k = turns + (k * H + h) * E;
    for (; f < f1; f += f1 - f < TC_CHUNK ? f1 - f : TC_CHUNK) {      // (ends at f == f1 exactly: the next run starts there)
      const int nc = (int)(f1 - f < TC_CHUNK ? f1 - f : TC_CHUNK);
      uint8_t b[TC_CHUNK];
#pragma unroll
      for (int c = 0; c < TC_CHUNK; ++c) b[c] = (c < nc && s_in) ? popped[(f + c) * K * N + s_off] : (uint8_t)0;
      __syncthreads();      // the previous chunk's reads are done
#pragma unroll
      for (int c = 0; c < TC_CHUNK; ++c) {
        const uint64_t m = __ballot(b[c] & 1);
        if (l == 0) s_mask[c][w] = m;
      }
      __syncthreads();
      // 0: no event, 1: phantom pop, 2: a movement over edge id[c], 3: unresolved
      int kind[TC_CHUNK];
      float before[TC_CHUNK];
      int32_t id[TC_CHUNK];
#pragma unroll
      for (int c = 0; c < TC_CHUNK; ++c) {
        kind[c] = (int)((s_mask[c][l >> 2] >> bit) & 1);      // (frames c >= nc were staged as zeros)
        if (kind[c]) {
          const int64_t fr = f + c;
          before[c] = fr > 0 ? counts[(fr - 1) * N * K + i] : (prev_counts ? prev_counts[i] : 0.0f);
          id[c] = sel8[fr * N * K + i] & 0x7F;
        }
      }
#pragma unroll
      for (int c = 0; c < TC_CHUNK; ++c) {
        if (kind[c] && before[c] > 0.0f) {      // not empty (0, -0.0 and NaN are): something left the road
          kind[c] = id[c] < deg ? 2 : 3;
          if (kind[c] == 2) id[c] = out_eid[o0 + id[c]];
        }
      }
#pragma unroll
      for (int c = 0; c < TC_CHUNK; ++c) {      // in frame order: two frames of a chunk may meet in one element
        if (kind[c] == 1)
          *lost_e += 1;
        else if (kind[c] == 2)
          turns_k[id[c]] += 1;
        else if (kind[c] == 3)
          atomicAdd(&unresolved[k], 1);
      }
    }
  }
}

extern "C" int tarl_turn_counts_accumulate(const tarl_plan* plan, const uint8_t* popped, const uint8_t* sel8,
                                           const float* counts, const float* prev_counts, int64_t F, int64_t K, int64_t t0,
                                           int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t H, int32_t* turns,
                                           int32_t* lost, int32_t* unresolved, tarl_stream stream) {
  TARL_REQUIRE(plan && popped && sel8 && counts && turns && lost && unresolved, "null argument");
  TARL_REQUIRE(F >= 1 && F <= TC_MAX_FRAMES, "F must be in [1, 2^23]");
  const int64_t lim = (int64_t)1 << 40, N = plan->N, E = plan->E;
  TARL_REQUIRE(N >= 1 && E >= 1, "the plan has no road or no edge");
  TARL_REQUIRE(K >= 1 && H >= 1 && K < lim && N < lim && E < lim && H < lim && K * N < lim && K * N * H < lim &&
                   K * E < lim && K * E * H < lim && K * N * F < lim,
               "bad sizes");
  TARL_REQUIRE_BINS(t0, timestep, bin_seconds, first_bin, F, H);
  const int64_t k_tiles = ceil_div(K, TC_ENVS), tiles = k_tiles * ceil_div(N, TC_ROADS);
  TARL_REQUIRE(tiles < ((int64_t)1 << 31), "bad sizes: too many tiles for one launch");
  hipLaunchKernelGGL(k_turn_counts_accumulate, dim3((unsigned)tiles), dim3(TC_ENVS * TC_ROADS), 0, (hipStream_t)stream,
                     plan->out_ptr, plan->out_eid, popped, sel8, counts, prev_counts, F, K, N, E, H, t0, timestep, bin_seconds,
                     first_bin, k_tiles, turns, lost, unresolved);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
