// dest_trees.hip — per-destination next-hop tables for the classical "dijkstra" agent (DijkstraAgents.choice,
// src/agents/base.py:519-584 of the reference) on graphs too large for routing.hip's all-pairs table (N^2 outputs and
// about N^3 work per refresh). A row only needs next_hop[u][dest] for the destination of its head agent, so the agent
// keeps one REVERSE shortest-path tree per distinct destination: O(E) work and O(N) state per tree, a [D][N] table.
//
// The trees are sp_trees.h's, from the destination backwards: candidates are marked over the CSC in-lists and pulled over
// the CSR out-lists, so dist[u] is the fp64 sum w1 + (w2 + (... + wk)) of the shortest path u -> d and the link of a node
// is its next hop (sp_trees.h states when that equals networkx's left-to-right sum bit for bit). The workgroup's scratch
// row is (dist fp64 [N], hop int32 [N]), with four N-bit bitmaps in LDS. tarl_dest_trees_batched runs the same kernel over
// B weight sets x D destinations (the vectorised baseline of tarl_hip/evaluator.py: one table per environment).
//
// k_prior_dest_table runs the distance phase alone for the shortest-path prior head (prior.hip) and writes the fp32
// rounding of each distance straight into the destination's column of a candidate-major [N][D] table: no next hops, no
// fp64 [D][N] output. The column stores are scattered (stride 4 D bytes); they cost little next to the relaxation rounds.
#include "sp_trees.h"

__global__ __launch_bounds__(SPT_BLOCK) void k_dest_trees(
    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src, const int32_t* __restrict__ out_ptr,
    const int32_t* __restrict__ out_dst, const int32_t* __restrict__ out_eid, const float* __restrict__ w, int64_t N,
    const int64_t* __restrict__ dests, int64_t D, uint8_t* __restrict__ scratch, int64_t row_bytes,
    int32_t* __restrict__ next_hop_out, double* __restrict__ dist_out, int64_t B, int64_t w_bstride) {
  extern __shared__ uint32_t dt_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  uint32_t* F = dt_lds;           // frontier
  uint32_t* C = F + W;            // candidates (all zero between rounds)
  uint32_t* NF = C + W;           // next BFS level
  uint32_t* V = NF + W;           // visited by the BFS
  double* dist = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  int32_t* hop = (int32_t*)(dist + N);

  // the workgroups stride over the B * D (weight set, destination) pairs, pair = b * D + slot: tarl_dest_trees is B = 1
  for (int64_t j = blockIdx.x; j < B * D; j += gridDim.x) {
    const int64_t wb = j / D;
    const int64_t d64 = dests[j - wb * D];
    if (d64 < 0 || d64 >= N) continue;      // uniform: an out-of-range destination writes nothing
    const int32_t d = (int32_t)d64;
    const float* wj = w + wb * w_bstride;
    spt_distances<float, true>(in_ptr, in_src, out_ptr, out_dst, out_eid, wj, N, W, tid, d, dist, F, C, V);
    if (next_hop_out) spt_links<float>(in_ptr, in_src, out_ptr, out_dst, out_eid, wj, N, W, tid, dist, hop, F, C, NF, V);

    // ---- outputs: d on its own slot, -1 where d is unreachable; hop is only valid where the BFS visited (V) ----
    for (int64_t u = tid; u < N; u += SPT_BLOCK) {
      if (dist_out) dist_out[j * N + u] = dist[u];
      if (next_hop_out) next_hop_out[j * N + u] = (u == d) ? d : (spt_bit(V, (int32_t)u) ? hop[u] : -1);
    }
    __syncthreads();   // the next destination re-initialises the row other threads may still be reading
  }
}

// ---- SELECTED_ROAD[i] = next_hop[dest_slot[DESTINATION(head agent of i)]][i] for every row --------------------------------
// routing.hip's k_select_next_hop with the [D][N] table: the same rules (an empty FIFO reads agent 0; an out-of-range head
// or destination leaves the row untouched; the road is written as float), and a destination without a tree (slot -1)
// leaves the row untouched too. One table for all B environments.
#define SEL_BLOCK 256
__global__ __launch_bounds__(SEL_BLOCK) void k_select_next_hop_dest(float* __restrict__ x, Layout L, int64_t B, int64_t N,
                                                                   const float* __restrict__ ag, int64_t A,
                                                                   int64_t a_bstride, const int32_t* __restrict__ dest_slot,
                                                                   const int32_t* __restrict__ next_hop, int64_t D) {
  const int64_t gid = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
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
__global__ __launch_bounds__(SPT_BLOCK) void k_prior_dest_table(
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
      for (int64_t u = tid; u < N; u += SPT_BLOCK) table[u * D + j] = __int_as_float(0x7F800000);
      continue;
    }
    spt_distances<float, false>(in_ptr, in_src, out_ptr, out_dst, out_eid, w, N, W, tid, (int32_t)d64, dist, dt_lds,
                                dt_lds + W, nullptr);
    for (int64_t u = tid; u < N; u += SPT_BLOCK) table[u * D + j] = (float)dist[u];
    __syncthreads();   // the next destination re-initialises the row other threads may still be reading
  }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
static const spt_query DT_QUERY = {"tarl_dest_trees", true, 4, 12,
                                   "graph too large for the per-destination trees (N > 327680)",
                                   "scratch too small (tarl_dest_trees_scratch_bytes)"};
static const spt_query PT_QUERY = {"tarl_prior_dest_table", true, 2, 8,
                                   "graph too large for the per-destination trees (N > 655360)",
                                   "scratch too small (tarl_prior_dest_table_scratch_bytes)"};

extern "C" int64_t tarl_dest_trees_scratch_bytes(const tarl_plan* plan, int64_t num_dests) {
  return spt_scratch_bytes(plan, num_dests, DT_QUERY.node_bytes);
}

extern "C" int tarl_dest_trees(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests,
                               void* scratch, int64_t scratch_bytes, int32_t* next_hop_out, double* dist_out,
                               tarl_stream stream) {
  TARL_REQUIRE(plan && weights && dests, "null argument");
  TARL_REQUIRE(next_hop_out || dist_out, "no output requested");
  return spt_launch(DT_QUERY, k_dest_trees, plan, weights, dests, num_dests, scratch, scratch_bytes, stream, next_hop_out,
                    dist_out, (int64_t)1, (int64_t)0);
}

// B weight sets at once: the same kernel over B * num_dests pairs. spt_launch sizes grid and scratch by the roots it is
// given, so this entry sizes them by the pairs itself.
extern "C" int64_t tarl_dest_trees_batched_scratch_bytes(const tarl_plan* plan, int64_t B, int64_t num_dests) {
  if (!plan || B < 1 || num_dests < 0) return -1;
  return spt_scratch_bytes(plan, B * num_dests, DT_QUERY.node_bytes);
}

extern "C" int tarl_dest_trees_batched(const tarl_plan* plan, const float* weights, int64_t B, int64_t w_bstride,
                                       const int64_t* dests, int64_t num_dests, void* scratch, int64_t scratch_bytes,
                                       int32_t* next_hop_out, tarl_stream stream) {
  static const spt_query Q = {"tarl_dest_trees_batched", true, 4, 12,
                              "graph too large for the per-destination trees (N > 327680)",
                              "scratch too small (tarl_dest_trees_batched_scratch_bytes)"};
  if (!(plan && weights && dests && next_hop_out)) return spt_invalid(Q, "null argument");
  if (B < 1 || num_dests < 0 || w_bstride < 0 || (w_bstride != 0 && w_bstride < plan->E)) return spt_invalid(Q, "bad sizes");
  const int64_t N = plan->N, pairs = B * num_dests;
  const int64_t lds = 4 * Q.bitmaps * ((N + 31) / 32);
  if (lds > SPT_LDS_MAX) return spt_invalid(Q, Q.too_large);
  if (pairs == 0 || N == 0) return TARL_OK;
  if (!scratch || scratch_bytes < spt_scratch_bytes(plan, pairs, Q.node_bytes)) return spt_invalid(Q, Q.scratch_small);
  if (lds > 64 * 1024)
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_dest_trees, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_dest_trees, dim3((unsigned)spt_workgroups(pairs)), dim3(SPT_BLOCK), (size_t)lds, (hipStream_t)stream,
                     plan->in_ptr, plan->in_src, plan->out_ptr, plan->out_dst, plan->out_eid, weights, N, dests, num_dests,
                     (uint8_t*)scratch, spt_row_bytes(N, Q.node_bytes), next_hop_out, (double*)nullptr, B, w_bstride);
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
  hipLaunchKernelGGL(k_select_next_hop_dest, dim3((unsigned)ceil_div(B * num_nodes, SEL_BLOCK)), dim3(SEL_BLOCK), 0,
                     (hipStream_t)stream, x, L, B, num_nodes, agent_features, num_agents, a_bstride, dest_slot, next_hop,
                     num_dests);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int64_t tarl_prior_dest_table_scratch_bytes(const tarl_plan* plan, int64_t num_dests) {
  return spt_scratch_bytes(plan, num_dests, PT_QUERY.node_bytes);
}

extern "C" int tarl_prior_dest_table(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests,
                                     void* scratch, int64_t scratch_bytes, float* table, tarl_stream stream) {
  TARL_REQUIRE(plan && weights && dests && table, "null argument");
  return spt_launch(PT_QUERY, k_prior_dest_table, plan, weights, dests, num_dests, scratch, scratch_bytes, stream, table);
}
