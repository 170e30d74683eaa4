// msa.hip — per-origin shortest-path trees for the MSA user equilibrium (src/algorithms/user_equilibrium_msa.py:65-165 of
// the reference) on graphs too large for an all-pairs next-hop table (routing.hip's k_apsp: N^2 outputs per iteration).
//
// One 256-thread workgroup per source, grid-strided over the sources. The workgroup owns a private global scratch row
// (dist fp64 [N], pred int32 [N]) and four N-bit bitmaps in LDS. Three phases:
//   1. distances: frontier -> candidates -> pull. Every set bit u of the frontier marks its out-neighbours in the
//      candidate bitmap (LDS atomic OR); after a barrier each candidate word is owned by one thread, which computes
//      min_u fl(dist[u] + w(u,v)) over the CSC in-edges of each of its nodes and, when that improves dist[v], stores it
//      (plain 8-B store) and sets v in the next frontier. Distances only decrease and a stale read of dist[u] is still a
//      real path length; a u that changed in this round is in the next frontier, so v is pulled again. Every schedule
//      reaches the same fixed point, the minimum over paths of the left-to-right fp64 sum: Dijkstra's result bit for bit.
//   2. predecessors: level-synchronous BFS from s over the TIGHT edges (fl(dist[u] + w) == dist[v], dist[v] finite).
//      pred[v] = the smallest node id u at the previous BFS level with a tight edge u -> v. Tie rule: minimise
//      (dist, hop count over tight edges) lexicographically, then the smallest predecessor id. Hops strictly increase
//      along the tree, so zero-weight cycles cannot close one; the rule does not depend on scheduling.
//   3. (assignment only) the OD pairs of the source (sorted by origin, od_ptr offsets) walk d -> o along pred and add the
//      pair's volume to every road node of path[1:] (d included, o not), fp64 atomics into aux_flow as k_msa_assign does.
//      With sptt_part / unrouted_part (tarl_msa_assign_sssp_gap) one thread also sums volume x dist[d] over the origin's
//      pairs, in pair order, while the distances are still in the scratch row: the gap costs no second pass.
// Scratch is O(workgroups x N), never O(sources x N).
#include "tarl_common.h"

#define MSA_BLOCK 256
#define MSA_MAX_WG 1024                      // resident workgroups (256 CUs x 4): bounds the scratch
#define MSA_LDS_MAX (160 * 1024)

static inline int64_t msa_row_bytes(int64_t N) { return (12 * N + 255) / 256 * 256; }

__device__ __forceinline__ bool bit_of(const uint32_t* bm, int32_t v) { return (bm[v >> 5] >> (v & 31)) & 1u; }

__global__ __launch_bounds__(MSA_BLOCK) void k_msa_trees(
    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, const double* __restrict__ w, int64_t N,
    const int64_t* __restrict__ sources, int64_t S, uint8_t* __restrict__ scratch, int64_t row_bytes,
    double* __restrict__ dist_out, int32_t* __restrict__ pred_out, const int64_t* __restrict__ od_ptr,
    const int64_t* __restrict__ od_dest, const double* __restrict__ od_vol, const uint8_t* __restrict__ is_road,
    double* __restrict__ aux_flow, double* __restrict__ sptt_part, double* __restrict__ unrouted_part) {
  extern __shared__ uint32_t msa_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  uint32_t* F = msa_lds;          // frontier
  uint32_t* C = F + W;            // candidates (all zero between rounds)
  uint32_t* NF = C + W;           // next BFS level
  uint32_t* V = NF + W;           // visited by the BFS
  double* dist = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  int32_t* pred = (int32_t*)(dist + N);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);

  for (int64_t j = blockIdx.x; j < S; j += gridDim.x) {
    const int64_t s64 = sources[j];
    if (s64 < 0 || s64 >= N) continue;      // uniform: out-of-range source writes nothing
    const int32_t s = (int32_t)s64;
    for (int64_t v = tid; v < N; v += MSA_BLOCK) dist[v] = INF;
    for (int32_t i = tid; i < W; i += MSA_BLOCK) {
      F[i] = 0u;
      C[i] = 0u;
      V[i] = 0u;
    }
    __syncthreads();
    if (tid == 0) {
      dist[s] = 0.0;
      F[s >> 5] = 1u << (s & 31);
      V[s >> 5] = 1u << (s & 31);
    }
    __syncthreads();

    // ---- 1. distances (at most N rounds: only reachable with negative weights, which the contract excludes) ----
    for (int64_t round = 0; round < N; ++round) {
      for (int32_t i = tid; i < W; i += MSA_BLOCK) {
        uint32_t m = F[i];
        while (m) {
          const int32_t u = (i << 5) + __builtin_ctz(m);
          m &= m - 1u;
          const int32_t k1 = out_ptr[u + 1];
          for (int32_t k = out_ptr[u]; k < k1; ++k) {
            const int32_t v = out_dst[k];
            atomicOr(&C[v >> 5], 1u << (v & 31));
          }
        }
      }
      __syncthreads();
      int any = 0;
      for (int32_t i = tid; i < W; i += MSA_BLOCK) {
        uint32_t c = C[i];
        uint32_t nf = 0u;
        if (c) C[i] = 0u;
        while (c) {
          const int b = __builtin_ctz(c);
          c &= c - 1u;
          const int32_t v = (i << 5) + b;
          const double old = dist[v];
          double best = old;
          const int32_t k1 = in_ptr[v + 1];
          for (int32_t k = in_ptr[v]; k < k1; ++k) {
            const double d = dist[in_src[k]] + w[in_eid[k]];
            if (d < best) best = d;
          }
          if (best < old) {
            dist[v] = best;
            nf |= 1u << b;
          }
        }
        F[i] = nf;
        any |= (nf != 0u);
      }
      if (!__syncthreads_or(any)) break;
    }

    // ---- 2. predecessors: BFS levels over the tight edges; F = {s}, V = {s} ----
    for (int32_t i = tid; i < W; i += MSA_BLOCK) F[i] = V[i];
    __syncthreads();
    uint32_t* cur = F;
    uint32_t* nxt = NF;
    for (;;) {
      for (int32_t i = tid; i < W; i += MSA_BLOCK) {
        uint32_t m = cur[i];
        while (m) {
          const int32_t u = (i << 5) + __builtin_ctz(m);
          m &= m - 1u;
          const int32_t k1 = out_ptr[u + 1];
          for (int32_t k = out_ptr[u]; k < k1; ++k) {
            const int32_t v = out_dst[k];
            if (!bit_of(V, v)) atomicOr(&C[v >> 5], 1u << (v & 31));
          }
        }
      }
      __syncthreads();
      int any = 0;
      for (int32_t i = tid; i < W; i += MSA_BLOCK) {
        uint32_t c = C[i];
        uint32_t nf = 0u;
        if (c) C[i] = 0u;
        while (c) {
          const int b = __builtin_ctz(c);
          c &= c - 1u;
          const int32_t v = (i << 5) + b;
          const double dv = dist[v];
          if (!(dv < INF)) continue;
          int32_t best = -1;
          const int32_t k1 = in_ptr[v + 1];
          for (int32_t k = in_ptr[v]; k < k1; ++k) {
            const int32_t u = in_src[k];
            if ((best < 0 || u < best) && bit_of(cur, u) && dist[u] + w[in_eid[k]] == dv) best = u;
          }
          if (best >= 0) {
            pred[v] = best;
            nf |= 1u << b;
          }
        }
        nxt[i] = nf;
        V[i] |= nf;
        any |= (nf != 0u);
      }
      const int more = __syncthreads_or(any);
      uint32_t* t = cur;
      cur = nxt;
      nxt = t;
      if (!more) break;
    }

    // ---- outputs: unreached nodes (and the source itself) have pred -1; pred is only valid where dist is finite ----
    if (dist_out || pred_out) {
      for (int64_t v = tid; v < N; v += MSA_BLOCK) {
        const double d = dist[v];
        if (dist_out) dist_out[j * N + v] = d;
        if (pred_out) pred_out[j * N + v] = (d < INF && v != s) ? pred[v] : -1;
      }
    }

    // ---- 3. fused all-or-nothing assignment of this origin's OD pairs ----
    if (od_ptr) {
      const int64_t p0 = od_ptr[j], p1 = od_ptr[j + 1], P = od_ptr[S];
      if (p0 >= 0 && p0 <= p1 && p1 <= P) {
        for (int64_t p = p0 + tid; p < p1; p += MSA_BLOCK) {
          const int64_t d = od_dest[p];
          const double vol = od_vol[p];
          if (d < 0 || d >= N || !(vol > 0.0) || !(dist[d] < INF)) continue;
          int32_t node = (int32_t)d;
          for (int64_t hops = 0; node != s && hops < N; ++hops) {
            if (is_road[node]) atomicAdd(&aux_flow[node], vol);
            node = pred[node];
            if (node < 0 || node >= N) break;
          }
        }
        // the demand's shortest-path travel time out of the same scratch row: one thread, pair order, no atomics (the
        // last thread: it has a walk of its own only when the origin has 256 pairs or more)
        if (sptt_part && tid == MSA_BLOCK - 1) {
          double sp = 0.0, un = 0.0;
          for (int64_t p = p0; p < p1; ++p) {
            const int64_t d = od_dest[p];
            const double vol = od_vol[p];
            if (d < 0 || d >= N || !(vol > 0.0)) continue;
            const double dd = dist[d];
            if (dd < INF) sp += vol * dd;
            else un += vol;
          }
          sptt_part[j] = sp;
          unrouted_part[j] = un;
        }
      }
    }
    __syncthreads();   // the next source re-initialises the row other threads may still be reading
  }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t tarl_msa_scratch_bytes(const tarl_plan* plan, int64_t num_sources) {
  if (!plan || num_sources < 0) return -1;
  const int64_t wg = num_sources < MSA_MAX_WG ? num_sources : MSA_MAX_WG;
  return wg * msa_row_bytes(plan->N);
}

static int msa_launch(const tarl_plan* plan, const double* weights, const int64_t* sources, int64_t S, void* scratch,
                      int64_t scratch_bytes, double* dist_out, int32_t* pred_out, const int64_t* od_ptr,
                      const int64_t* od_dest, const double* od_vol, const uint8_t* is_road, double* aux_flow,
                      double* sptt_part, double* unrouted_part, tarl_stream stream) {
  TARL_REQUIRE(plan && weights && sources, "null argument");
  TARL_REQUIRE(S >= 0, "bad sizes");
  const int64_t N = plan->N;
  const int64_t lds = 16 * ((N + 31) / 32);
  TARL_REQUIRE(lds <= MSA_LDS_MAX, "graph too large for the per-origin trees (N > 327680)");
  if (S == 0 || N == 0) return TARL_OK;
  const int64_t need = tarl_msa_scratch_bytes(plan, S);
  TARL_REQUIRE(scratch && scratch_bytes >= need, "scratch too small (tarl_msa_scratch_bytes)");
  const int64_t wg = S < MSA_MAX_WG ? S : MSA_MAX_WG;
  if (lds > 64 * 1024)
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_msa_trees, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_msa_trees, dim3((unsigned)wg), dim3(MSA_BLOCK), (size_t)lds, (hipStream_t)stream, plan->in_ptr,
                     plan->in_src, plan->in_eid, plan->out_ptr, plan->out_dst, weights, N, sources, S,
                     (uint8_t*)scratch, msa_row_bytes(N), dist_out, pred_out, od_ptr, od_dest, od_vol, is_road,
                     aux_flow, sptt_part, unrouted_part);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_sssp_f64(const tarl_plan* plan, const double* weights, const int64_t* sources, int64_t num_sources,
                             void* scratch, int64_t scratch_bytes, double* dist_out, int32_t* pred_out,
                             tarl_stream stream) {
  return msa_launch(plan, weights, sources, num_sources, scratch, scratch_bytes, dist_out, pred_out, nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int tarl_msa_assign_sssp(const tarl_plan* plan, const double* weights, const int64_t* origins,
                                    int64_t num_origins, const int64_t* od_ptr, const int64_t* od_dest,
                                    const double* od_volume, const uint8_t* is_road, void* scratch,
                                    int64_t scratch_bytes, double* aux_flow, tarl_stream stream) {
  TARL_REQUIRE(od_ptr && od_dest && od_volume && is_road && aux_flow, "null argument");
  return msa_launch(plan, weights, origins, num_origins, scratch, scratch_bytes, nullptr, nullptr, od_ptr, od_dest,
                    od_volume, is_road, aux_flow, nullptr, nullptr, stream);
}

// tarl_msa_assign_sssp that also returns, per origin, the shortest-path travel time of its demand and the volume no path
// serves. Entries of out-of-range origins (and of origins with an inconsistent od_ptr range) are not written.
extern "C" int tarl_msa_assign_sssp_gap(const tarl_plan* plan, const double* weights, const int64_t* origins,
                                        int64_t num_origins, const int64_t* od_ptr, const int64_t* od_dest,
                                        const double* od_volume, const uint8_t* is_road, void* scratch,
                                        int64_t scratch_bytes, double* aux_flow, double* sptt_part,
                                        double* unrouted_part, tarl_stream stream) {
  TARL_REQUIRE(od_ptr && od_dest && od_volume && is_road && aux_flow && sptt_part && unrouted_part, "null argument");
  return msa_launch(plan, weights, origins, num_origins, scratch, scratch_bytes, nullptr, nullptr, od_ptr, od_dest,
                    od_volume, is_road, aux_flow, sptt_part, unrouted_part, stream);
}
