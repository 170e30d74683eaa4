// msa.hip — per-origin shortest-path trees for the MSA user equilibrium (src/algorithms/user_equilibrium_msa.py:65-165 of
// the reference) on graphs too large for an all-pairs next-hop table (routing.hip's k_apsp: N^2 outputs per iteration).
//
// The trees are sp_trees.h's, from the origin outwards: candidates are marked over the CSR out-lists and pulled over the
// CSC in-lists, so dist is Dijkstra's left-to-right fp64 sum and the link of a node is its predecessor. The workgroup's
// scratch row is (dist fp64 [N], pred int32 [N]), with four N-bit bitmaps in LDS. What this file adds per source:
//   - the outputs: dist and pred as they stand, pred -1 for the source and for unreached nodes;
//   - (assignment only) the OD pairs of the source (sorted by origin, od_ptr offsets) walk d -> o along pred and add the
//     pair's volume to every road node of path[1:] (d included, o not), fp64 atomics into aux_flow as k_msa_assign does.
//     With sptt_part / unrouted_part (tarl_msa_assign_sssp_gap) one thread also sums volume x dist[d] over the origin's
//     pairs, in pair order, while the distances are still in the scratch row: the gap costs no second pass.
#include "sp_trees.h"

__global__ __launch_bounds__(SPT_BLOCK) void k_msa_trees(
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
    spt_distances<double, true>(out_ptr, out_dst, in_ptr, in_src, in_eid, w, N, W, tid, s, dist, F, C, V);
    spt_links<double>(out_ptr, out_dst, in_ptr, in_src, in_eid, w, N, W, tid, dist, pred, F, C, NF, V);

    // ---- outputs: unreached nodes (and the source itself) have pred -1; pred is only valid where dist is finite ----
    if (dist_out || pred_out) {
      for (int64_t v = tid; v < N; v += SPT_BLOCK) {
        const double d = dist[v];
        if (dist_out) dist_out[j * N + v] = d;
        if (pred_out) pred_out[j * N + v] = (d < INF && v != s) ? pred[v] : -1;
      }
    }

    // ---- fused all-or-nothing assignment of this origin's OD pairs ----
    if (od_ptr) {
      const int64_t p0 = od_ptr[j], p1 = od_ptr[j + 1], P = od_ptr[S];
      if (p0 >= 0 && p0 <= p1 && p1 <= P) {
        for (int64_t p = p0 + tid; p < p1; p += SPT_BLOCK) {
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
        if (sptt_part && tid == SPT_BLOCK - 1) {
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
static const spt_query MSA_QUERY = {"msa_launch", false, 4, 12, "graph too large for the per-origin trees (N > 327680)",
                                    "scratch too small (tarl_msa_scratch_bytes)"};

extern "C" int64_t tarl_msa_scratch_bytes(const tarl_plan* plan, int64_t num_sources) {
  return spt_scratch_bytes(plan, num_sources, MSA_QUERY.node_bytes);
}

static int msa_launch(const tarl_plan* plan, const double* weights, const int64_t* sources, int64_t S, void* scratch,
                      int64_t scratch_bytes, double* dist_out, int32_t* pred_out, const int64_t* od_ptr,
                      const int64_t* od_dest, const double* od_vol, const uint8_t* is_road, double* aux_flow,
                      double* sptt_part, double* unrouted_part, tarl_stream stream) {
  return spt_launch(MSA_QUERY, k_msa_trees, plan, weights, sources, S, scratch, scratch_bytes, stream, dist_out, pred_out,
                    od_ptr, od_dest, od_vol, is_road, aux_flow, sptt_part, unrouted_part);
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
