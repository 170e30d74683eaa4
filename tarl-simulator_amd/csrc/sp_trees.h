// sp_trees.h — the shared core of the shortest-path tree kernels: k_msa_trees (msa.hip, one tree per origin),
// k_dest_trees and k_prior_dest_table (dest_trees.hip, one reverse tree / one distance column per destination).
//
// One 256-thread workgroup per root, grid-strided over the roots by the kernel. The workgroup owns a private global
// scratch row (dist fp64 [N], then link int32 [N] where links are wanted) and N-bit bitmaps in LDS. Two phases, each
// written over two adjacencies: the MARK lists (mark_ptr, mark_idx) lead from a node whose value changed to the nodes that
// depend on it, the PULL lists (pull_ptr, pull_nbr, pull_eid) lead from a node to the nodes its value is computed from.
// Trees from an origin mark over the CSR out-lists and pull over the CSC in-lists; trees towards a destination do the
// opposite. The weights are fp64 or fp32 in original edge order; every sum is fp64.
//   1. spt_distances: frontier -> candidates -> pull. Every set bit of the frontier marks its dependants in the candidate
//      bitmap (LDS atomic OR); after a barrier each candidate word is owned by one thread, which computes
//      min_k fl(dist[nbr_k] + w_k) over the pull list of each of its nodes and, when that improves dist[v], stores it (plain
//      8-B store) and sets v in the next frontier. Distances only decrease and a stale read of dist[nbr] is still a real
//      path length; a neighbour that changed in this round is in the next frontier, so v is pulled again. Every schedule
//      reaches the same fixed point: the minimum over paths of the fp64 sum accumulated from the root outwards, which is
//      Dijkstra's result bit for bit (from an origin: left to right; towards a destination: w1 + (w2 + (... + wk))).
//   2. spt_links: level-synchronous BFS from the root over the TIGHT edges (fl(dist[nbr] + w) == dist[v], dist[v] finite).
//      link[v] = the smallest node id at the previous BFS level with a tight edge to v: the predecessor from an origin,
//      the next hop towards a destination. Tie rule: minimise (dist, hop count over tight edges) lexicographically, then
//      the smallest link id. Hops strictly increase away from the root, so zero-weight cycles cannot close a tree; the
//      rule does not depend on scheduling.
// Exactness against networkx (which sums left to right from the start of the path) for the reverse trees: with fp32
// weights and fp64 sums both orders are exact — and the distances equal networkx's bit for bit — whenever, on every
// shortest path, the exponent span of the weights (largest over smallest, in bits) plus ceil(log2 hops) stays at or below
// 28 (24-bit fp32 significands in a 53-bit fp64 one). Beyond that only the last bit may differ, and with it the tie choice.
// Scratch is O(workgroups x N), never O(roots x N).
//
// The graph arrays are separate __restrict__ pointer parameters, not a struct: in this code base that choice decides
// scalar against vector loads, and with them the register count.
#pragma once
#include "tarl_common.h"

#define SPT_BLOCK 256
#define SPT_MAX_WG 1024                      // resident workgroups (256 CUs x 4): bounds the scratch
#define SPT_LDS_MAX (160 * 1024)

__device__ __forceinline__ bool spt_bit(const uint32_t* bm, int32_t v) { return (bm[v >> 5] >> (v & 31)) & 1u; }

// Both phases take the kernel's own tid (threadIdx.x) and W (the words of an N-bit bitmap) instead of deriving them again:
// the compiler simplifies these functions before it inlines them, and with the two values recomputed k_msa_trees came out
// 0.5 % slower than with them passed in (profiles/sp_trees_ab.txt).
// ---- phase 1 -------------------------------------------------------------------------------------------------------------
// dist [N] (the workgroup's scratch row) <- the fp64 distances between root and every node; F and C are W-word LDS bitmaps
// (C is left all zero). With VISITED, V is cleared and gets {root}. Ends on a barrier.
template <typename WT, bool VISITED>
__device__ __forceinline__ void spt_distances(const int32_t* __restrict__ mark_ptr, const int32_t* __restrict__ mark_idx,
                                              const int32_t* __restrict__ pull_ptr, const int32_t* __restrict__ pull_nbr,
                                              const int32_t* __restrict__ pull_eid, const WT* __restrict__ w, int64_t N,
                                              int32_t W, int tid, int32_t root, double* dist, uint32_t* F, uint32_t* C, uint32_t* V) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  for (int64_t v = tid; v < N; v += SPT_BLOCK) dist[v] = INF;
  for (int32_t i = tid; i < W; i += SPT_BLOCK) {
    F[i] = 0u;
    C[i] = 0u;
    if (VISITED) V[i] = 0u;
  }
  __syncthreads();
  if (tid == 0) {
    dist[root] = 0.0;
    F[root >> 5] = 1u << (root & 31);
    if (VISITED) V[root >> 5] = 1u << (root & 31);
  }
  __syncthreads();

  // at most N rounds: only reachable with negative weights, which the contract excludes
  for (int64_t round = 0; round < N; ++round) {
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
      uint32_t m = F[i];
      while (m) {
        const int32_t u = (i << 5) + __builtin_ctz(m);
        m &= m - 1u;
        const int32_t k1 = mark_ptr[u + 1];
        for (int32_t k = mark_ptr[u]; k < k1; ++k) {
          const int32_t v = mark_idx[k];
          atomicOr(&C[v >> 5], 1u << (v & 31));
        }
      }
    }
    __syncthreads();
    int any = 0;
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
      uint32_t c = C[i];
      uint32_t nf = 0u;
      if (c) C[i] = 0u;
      while (c) {
        const int b = __builtin_ctz(c);
        c &= c - 1u;
        const int32_t v = (i << 5) + b;
        const double old = dist[v];
        double best = old;
        const int32_t k1 = pull_ptr[v + 1];
        for (int32_t k = pull_ptr[v]; k < k1; ++k) {
          const double d = dist[pull_nbr[k]] + (double)w[pull_eid[k]];
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
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------------
// After spt_distances<WT, true>: BFS levels over the tight edges, starting from V = {root}. link[v] is written for every
// node the BFS visits except the root, and V is left as the visited set: link is only valid where V is set. F, C, NF and
// V are W-word LDS bitmaps (C all zero on entry and on exit). Ends on a barrier.
template <typename WT>
__device__ __forceinline__ void spt_links(const int32_t* __restrict__ mark_ptr, const int32_t* __restrict__ mark_idx,
                                          const int32_t* __restrict__ pull_ptr, const int32_t* __restrict__ pull_nbr,
                                          const int32_t* __restrict__ pull_eid, const WT* __restrict__ w, int64_t N,
                                          int32_t W, int tid, const double* dist, int32_t* link, uint32_t* F, uint32_t* C, uint32_t* NF,
                                          uint32_t* V) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  for (int32_t i = tid; i < W; i += SPT_BLOCK) F[i] = V[i];
  __syncthreads();
  uint32_t* cur = F;
  uint32_t* nxt = NF;
  for (;;) {
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
      uint32_t m = cur[i];
      while (m) {
        const int32_t u = (i << 5) + __builtin_ctz(m);
        m &= m - 1u;
        const int32_t k1 = mark_ptr[u + 1];
        for (int32_t k = mark_ptr[u]; k < k1; ++k) {
          const int32_t v = mark_idx[k];
          if (!spt_bit(V, v)) atomicOr(&C[v >> 5], 1u << (v & 31));
        }
      }
    }
    __syncthreads();
    int any = 0;
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
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
        const int32_t k1 = pull_ptr[v + 1];
        for (int32_t k = pull_ptr[v]; k < k1; ++k) {
          const int32_t u = pull_nbr[k];
          if ((best < 0 || u < best) && spt_bit(cur, u) && dist[u] + (double)w[pull_eid[k]] == dv) best = u;
        }
        if (best >= 0) {
          link[v] = best;
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

// ---- host side -----------------------------------------------------------------------------------------------------------
// What tells the three queries apart on the host: the direction of the trees, the LDS bitmaps and scratch bytes per node of
// the kernel, and the texts of its errors.
struct spt_query {
  const char* entry;           // the name that leads the error messages
  bool towards_root;           // false: mark CSR, pull CSC (k_msa_trees); true: the opposite (the per-destination kernels)
  int bitmaps;                 // N-bit LDS bitmaps: 4 with links (F, C, NF, V), 2 for distances alone (F, C)
  int node_bytes;              // scratch row bytes per node: 12 = dist + link, 8 = dist only
  const char* too_large;
  const char* scratch_small;
};

static inline int64_t spt_workgroups(int64_t roots) { return roots < SPT_MAX_WG ? roots : SPT_MAX_WG; }

static inline int64_t spt_row_bytes(int64_t N, int64_t node_bytes) { return (node_bytes * N + 255) / 256 * 256; }

static inline int64_t spt_scratch_bytes(const tarl_plan* plan, int64_t roots, int64_t node_bytes) {
  if (!plan || roots < 0) return -1;
  return spt_workgroups(roots) * spt_row_bytes(plan->N, node_bytes);
}

static inline int spt_invalid(const spt_query& q, const char* msg) {
  tarl_set_error("%s: requirement failed: %s", q.entry, msg);
  return TARL_ERR_INVALID;
}

// Checks the arguments every query shares, sizes the launch and runs it. Every kernel takes the five graph arrays of its
// direction (pull lists with edge ids, mark lists without), weights, N, roots, count, scratch, row bytes, then `out`.
template <typename Kernel, typename WT, typename... Out>
static int spt_launch(const spt_query& q, Kernel kernel, const tarl_plan* plan, const WT* weights, const int64_t* roots,
                      int64_t count, void* scratch, int64_t scratch_bytes, tarl_stream stream, Out... out) {
  if (!(plan && weights && roots)) return spt_invalid(q, "null argument");
  if (count < 0) return spt_invalid(q, "bad sizes");
  const int64_t N = plan->N;
  const int64_t lds = 4 * q.bitmaps * ((N + 31) / 32);
  if (lds > SPT_LDS_MAX) return spt_invalid(q, q.too_large);
  if (count == 0 || N == 0) return TARL_OK;
  if (!scratch || scratch_bytes < spt_scratch_bytes(plan, count, q.node_bytes)) return spt_invalid(q, q.scratch_small);
  if (lds > 64 * 1024)   // the dynamic-LDS limit only needs raising above the 64 KB default
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)spt_workgroups(count)), block(SPT_BLOCK);
  const int64_t row_bytes = spt_row_bytes(N, q.node_bytes);
  if (q.towards_root)
    hipLaunchKernelGGL(kernel, grid, block, (size_t)lds, (hipStream_t)stream, plan->in_ptr, plan->in_src, plan->out_ptr,
                       plan->out_dst, plan->out_eid, weights, N, roots, count, (uint8_t*)scratch, row_bytes, out...);
  else
    hipLaunchKernelGGL(kernel, grid, block, (size_t)lds, (hipStream_t)stream, plan->in_ptr, plan->in_src, plan->in_eid,
                       plan->out_ptr, plan->out_dst, weights, N, roots, count, (uint8_t*)scratch, row_bytes, out...);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
