// dest_trees.hip — per-destination next-hop tables for the classical "dijkstra" agent (DijkstraAgents.choice,
// src/agents/base.py:519-584 of the reference) on graphs too large for routing.hip's all-pairs table (N^2 outputs and
// about N^3 work per refresh). A row only needs next_hop[u][dest] for the destination of its head agent, so the agent
// keeps one REVERSE shortest-path tree per distinct destination: O(E) work and O(N) state per tree, a [D][N] table.
//
// The mirror image of msa.hip's k_msa_trees (per-origin trees). One 256-thread workgroup per destination d, grid-strided
// over the destinations. The workgroup owns a private global scratch row (dist fp64 [N], hop int32 [N]) and four N-bit
// bitmaps in LDS. Two phases:
//   1. distances: frontier -> candidates -> pull. Every set bit v of the frontier marks its IN-neighbours (CSC) in the
//      candidate bitmap (LDS atomic OR); after a barrier each candidate word is owned by one thread, which computes
//      min_v fl(w(u,v) + dist[v]) over the CSR out-edges of each of its nodes u and, when that improves dist[u], stores it
//      (plain 8-B store) and sets u in the next frontier. Distances only decrease and a stale read of dist[v] is still a
//      real path length; a v that changed in this round is in the next frontier, so u is pulled again. Every schedule
//      reaches the same fixed point: the minimum over paths u -> d of the fp64 sum w1 + (w2 + (... + wk)).
//   2. next hops: level-synchronous BFS backwards from d over the TIGHT edges (fl(w(u,v) + dist[v]) == dist[u], dist[u]
//      finite). hop[u] = the smallest node id v at the previous BFS level with a tight edge u -> v. Tie rule: the fewest
//      hops to d over tight edges, then the smallest successor id. Hops strictly decrease along the table, so zero-weight
//      cycles cannot close one; the rule does not depend on scheduling.
// Exactness against networkx (which sums left to right from u): the weights are fp32 and the sums fp64, so both orders
// are exact — and the distances equal networkx's bit for bit — whenever, on every shortest path, the exponent span of the
// weights (largest over smallest, in bits) plus ceil(log2 hops) stays at or below 28 (24-bit fp32 significands in a 53-bit
// fp64 one). Beyond that only the last bit may differ, and with it the tie choice.
// Scratch is O(workgroups x N), never O(destinations x N).
//
// k_prior_dest_table runs phase 1 alone for the shortest-path prior head (prior.hip) and writes the fp32 rounding of each
// distance straight into the destination's column of a candidate-major [N][D] table: no next hops, no fp64 [D][N] output.
// The column stores are scattered (stride 4 D bytes); they cost little next to the relaxation rounds.
#include "tarl_common.h"

#define DT_BLOCK 256
#define DT_MAX_WG 1024                      // resident workgroups (256 CUs x 4): bounds the scratch
#define DT_LDS_MAX (160 * 1024)

static inline int64_t dt_row_bytes(int64_t N) { return (12 * N + 255) / 256 * 256; }

__device__ __forceinline__ bool dt_bit(const uint32_t* bm, int32_t v) { return (bm[v >> 5] >> (v & 31)) & 1u; }

// ---- phase 1, shared by k_dest_trees and k_prior_dest_table ------------------------------------------------------------
// dist [N] (the workgroup's scratch row) <- the fp64 distances of every node to d; F and C are W-word LDS bitmaps (C is left
// all zero). With VISITED, V is cleared and gets {d}. Ends on a barrier.
template <bool VISITED>
__device__ __forceinline__ void dt_distances(const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                             const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                             const int32_t* __restrict__ out_eid, const float* __restrict__ w, int64_t N,
                                             int32_t d, double* dist, uint32_t* F, uint32_t* C, uint32_t* V) {
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  for (int64_t v = tid; v < N; v += DT_BLOCK) dist[v] = INF;
  for (int32_t i = tid; i < W; i += DT_BLOCK) {
    F[i] = 0u;
    C[i] = 0u;
    if (VISITED) V[i] = 0u;
  }
  __syncthreads();
  if (tid == 0) {
    dist[d] = 0.0;
    F[d >> 5] = 1u << (d & 31);
    if (VISITED) V[d >> 5] = 1u << (d & 31);
  }
  __syncthreads();

  // at most N rounds: only reachable with negative weights, which the contract excludes
  for (int64_t round = 0; round < N; ++round) {
    for (int32_t i = tid; i < W; i += DT_BLOCK) {
      uint32_t m = F[i];
      while (m) {
        const int32_t v = (i << 5) + __builtin_ctz(m);
        m &= m - 1u;
        const int32_t k1 = in_ptr[v + 1];
        for (int32_t k = in_ptr[v]; k < k1; ++k) {
          const int32_t u = in_src[k];
          atomicOr(&C[u >> 5], 1u << (u & 31));
        }
      }
    }
    __syncthreads();
    int any = 0;
    for (int32_t i = tid; i < W; i += DT_BLOCK) {
      uint32_t c = C[i];
      uint32_t nf = 0u;
      if (c) C[i] = 0u;
      while (c) {
        const int b = __builtin_ctz(c);
        c &= c - 1u;
        const int32_t u = (i << 5) + b;
        const double old = dist[u];
        double best = old;
        const int32_t k1 = out_ptr[u + 1];
        for (int32_t k = out_ptr[u]; k < k1; ++k) {
          const double du = (double)w[out_eid[k]] + dist[out_dst[k]];
          if (du < best) best = du;
        }
        if (best < old) {
          dist[u] = best;
          nf |= 1u << b;
        }
      }
      F[i] = nf;
      any |= (nf != 0u);
    }
    if (!__syncthreads_or(any)) break;
  }
}

__global__ __launch_bounds__(DT_BLOCK) void k_dest_trees(
    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src, const int32_t* __restrict__ out_ptr,
    const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_eid, const float* __restrict__ w, int64_t N,
    const int64_t* __restrict__ dests, int64_t D, uint8_t* __restrict__ scratch, int64_t row_bytes,
    int32_t* __restrict__ next_hop_out, double* __restrict__ dist_out) {
  extern __shared__ uint32_t dt_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  uint32_t* F = dt_lds;           // frontier
  uint32_t* C = F + W;            // candidates (all zero between rounds)
  uint32_t* NF = C + W;           // next BFS level
  uint32_t* V = NF + W;           // visited by the BFS
  double* dist = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  int32_t* hop = (int32_t*)(dist + N);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);

  for (int64_t j = blockIdx.x; j < D; j += gridDim.x) {
    const int64_t d64 = dests[j];
    if (d64 < 0 || d64 >= N) continue;      // uniform: an out-of-range destination writes nothing
    const int32_t d = (int32_t)d64;

    // ---- 1. distances ----
    dt_distances<true>(in_ptr, in_src, out_ptr, out_dst, out_eid, w, N, d, dist, F, C, V);

    // ---- 2. next hops: BFS levels backwards over the tight edges; F = {d}, V = {d} ----
    if (next_hop_out) {
      for (int32_t i = tid; i < W; i += DT_BLOCK) F[i] = V[i];
      __syncthreads();
      uint32_t* cur = F;
      uint32_t* nxt = NF;
      for (;;) {
        for (int32_t i = tid; i < W; i += DT_BLOCK) {
          uint32_t m = cur[i];
          while (m) {
            const int32_t v = (i << 5) + __builtin_ctz(m);
            m &= m - 1u;
            const int32_t k1 = in_ptr[v + 1];
            for (int32_t k = in_ptr[v]; k < k1; ++k) {
              const int32_t u = in_src[k];
              if (!dt_bit(V, u)) atomicOr(&C[u >> 5], 1u << (u & 31));
            }
          }
        }
        __syncthreads();
        int any = 0;
        for (int32_t i = tid; i < W; i += DT_BLOCK) {
          uint32_t c = C[i];
          uint32_t nf = 0u;
          if (c) C[i] = 0u;
          while (c) {
            const int b = __builtin_ctz(c);
            c &= c - 1u;
            const int32_t u = (i << 5) + b;
            const double du = dist[u];
            if (!(du < INF)) continue;
            int32_t best = -1;
            const int32_t k1 = out_ptr[u + 1];
            for (int32_t k = out_ptr[u]; k < k1; ++k) {
              const int32_t v = out_dst[k];
              if ((best < 0 || v < best) && dt_bit(cur, v) && (double)w[out_eid[k]] + dist[v] == du) best = v;
            }
            if (best >= 0) {
              hop[u] = best;
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
    }

    // ---- outputs: d on its own slot, -1 where d is unreachable; hop is only valid where the BFS visited (V) ----
    for (int64_t u = tid; u < N; u += DT_BLOCK) {
      if (dist_out) dist_out[j * N + u] = dist[u];
      if (next_hop_out) next_hop_out[j * N + u] = (u == d) ? d : (dt_bit(V, (int32_t)u) ? hop[u] : -1);
    }
    __syncthreads();   // the next destination re-initialises the row other threads may still be reading
  }
}

// ---- SELECTED_ROAD[i] = next_hop[dest_slot[DESTINATION(head agent of i)]][i] for every row --------------------------------
// routing.hip's k_select_next_hop with the [D][N] table: the same rules (an empty FIFO reads agent 0; an out-of-range head
// or destination leaves the row untouched; the road is written as float), and a destination without a tree (slot -1)
// leaves the row untouched too. One table for all B environments.
__global__ __launch_bounds__(DT_BLOCK) void k_select_next_hop_dest(float* __restrict__ x, Layout L, int64_t B, int64_t N,
                                                                   const float* __restrict__ ag, int64_t A,
                                                                   int64_t a_bstride, const int32_t* __restrict__ dest_slot,
                                                                   const int32_t* __restrict__ next_hop, int64_t D) {
  const int64_t gid = (int64_t)blockIdx.x * DT_BLOCK + threadIdx.x;
  if (gid >= B * N) return;
  const int64_t b = gid / N;
  const int64_t i = gid - b * N;
  float* xi = x + b * L.bstride + i * L.ldx;
  const long long head = (long long)xi[0];
  if (head < 0 || head >= A) return;
  const long long dest = (long long)ag[b * a_bstride + head * AG_COLS + AG_DEST];
  if (dest < 0 || dest >= N) return;
  const int32_t slot = dest_slot[dest];
  if (slot < 0 || slot >= D) return;
  xi[L.col_sel()] = (float)next_hop[(int64_t)slot * N + i];
}

// ---- the prior head's distance table: table[u][j] = (float) dist(u -> dests[j]), candidate-major ----------------------------
// One workgroup per destination as k_dest_trees, phase 1 only (two LDS bitmaps, an fp64 scratch row of N). +inf where
// unreachable, 0 at the destination; an out-of-range destination gets a column of +inf.
__global__ __launch_bounds__(DT_BLOCK) void k_prior_dest_table(
    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src, const int32_t* __restrict__ out_ptr,
    const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_eid, const float* __restrict__ w, int64_t N,
    const int64_t* __restrict__ dests, int64_t D, uint8_t* __restrict__ scratch, int64_t row_bytes,
    float* __restrict__ table) {
  extern __shared__ uint32_t dt_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  double* dist = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  for (int64_t j = blockIdx.x; j < D; j += gridDim.x) {
    const int64_t d64 = dests[j];
    if (d64 < 0 || d64 >= N) {               // uniform
      for (int64_t u = tid; u < N; u += DT_BLOCK) table[u * D + j] = __int_as_float(0x7F800000);
      continue;
    }
    dt_distances<false>(in_ptr, in_src, out_ptr, out_dst, out_eid, w, N, (int32_t)d64, dist, dt_lds, dt_lds + W, nullptr);
    for (int64_t u = tid; u < N; u += DT_BLOCK) table[u * D + j] = (float)dist[u];
    __syncthreads();   // the next destination re-initialises the row other threads may still be reading
  }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t tarl_dest_trees_scratch_bytes(const tarl_plan* plan, int64_t num_dests) {
  if (!plan || num_dests < 0) return -1;
  const int64_t wg = num_dests < DT_MAX_WG ? num_dests : DT_MAX_WG;
  return wg * dt_row_bytes(plan->N);
}

extern "C" int tarl_dest_trees(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests,
                               void* scratch, int64_t scratch_bytes, int32_t* next_hop_out, double* dist_out,
                               tarl_stream stream) {
  TARL_REQUIRE(plan && weights && dests, "null argument");
  TARL_REQUIRE(next_hop_out || dist_out, "no output requested");
  TARL_REQUIRE(num_dests >= 0, "bad sizes");
  const int64_t N = plan->N;
  const int64_t lds = 16 * ((N + 31) / 32);
  TARL_REQUIRE(lds <= DT_LDS_MAX, "graph too large for the per-destination trees (N > 327680)");
  if (num_dests == 0 || N == 0) return TARL_OK;
  const int64_t need = tarl_dest_trees_scratch_bytes(plan, num_dests);
  TARL_REQUIRE(scratch && scratch_bytes >= need, "scratch too small (tarl_dest_trees_scratch_bytes)");
  const int64_t wg = num_dests < DT_MAX_WG ? num_dests : DT_MAX_WG;
  if (lds > 64 * 1024)
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_dest_trees, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_dest_trees, dim3((unsigned)wg), dim3(DT_BLOCK), (size_t)lds, (hipStream_t)stream, plan->in_ptr,
                     plan->in_src, plan->out_ptr, plan->out_dst, plan->out_eid, weights, N, dests, num_dests,
                     (uint8_t*)scratch, dt_row_bytes(N), next_hop_out, dist_out);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_select_next_hop_dest(float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                                         int64_t num_nodes, const float* agent_features, int64_t num_agents,
                                         int64_t a_bstride, const int32_t* dest_slot, const int32_t* next_hop,
                                         int64_t num_dests, tarl_stream stream) {
  TARL_REQUIRE(x && agent_features && dest_slot && next_hop, "null argument");
  TARL_REQUIRE(B >= 1 && Nmax >= 1 && ldx >= 3 * (int64_t)Nmax + 7 && num_agents >= 1 && num_nodes >= 0 &&
                   num_dests >= 0, "bad shape");
  if (num_nodes == 0) return TARL_OK;
  Layout L{Nmax, ldx, x_bstride};
  hipLaunchKernelGGL(k_select_next_hop_dest, dim3((unsigned)ceil_div(B * num_nodes, DT_BLOCK)), dim3(DT_BLOCK), 0,
                     (hipStream_t)stream, x, L, B, num_nodes, agent_features, num_agents, a_bstride, dest_slot, next_hop,
                     num_dests);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

static inline int64_t pt_row_bytes(int64_t N) { return (8 * N + 255) / 256 * 256; }

extern "C" int64_t tarl_prior_dest_table_scratch_bytes(const tarl_plan* plan, int64_t num_dests) {
  if (!plan || num_dests < 0) return -1;
  const int64_t wg = num_dests < DT_MAX_WG ? num_dests : DT_MAX_WG;
  return wg * pt_row_bytes(plan->N);
}

extern "C" int tarl_prior_dest_table(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests,
                                     void* scratch, int64_t scratch_bytes, float* table, tarl_stream stream) {
  TARL_REQUIRE(plan && weights && dests && table, "null argument");
  TARL_REQUIRE(num_dests >= 0, "bad sizes");
  const int64_t N = plan->N;
  const int64_t lds = 8 * ((N + 31) / 32);
  TARL_REQUIRE(lds <= DT_LDS_MAX, "graph too large for the per-destination trees (N > 655360)");
  if (num_dests == 0 || N == 0) return TARL_OK;
  const int64_t need = tarl_prior_dest_table_scratch_bytes(plan, num_dests);
  TARL_REQUIRE(scratch && scratch_bytes >= need, "scratch too small (tarl_prior_dest_table_scratch_bytes)");
  const int64_t wg = num_dests < DT_MAX_WG ? num_dests : DT_MAX_WG;
  if (lds > 64 * 1024)
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_prior_dest_table, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
  hipLaunchKernelGGL(k_prior_dest_table, dim3((unsigned)wg), dim3(DT_BLOCK), (size_t)lds, (hipStream_t)stream, plan->in_ptr,
                     plan->in_src, plan->out_ptr, plan->out_dst, plan->out_eid, weights, N, dests, num_dests,
                     (uint8_t*)scratch, pt_row_bytes(N), table);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
