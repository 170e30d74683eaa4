// path_trace.hip — per-agent path trace of the vectorised evaluation: which roads every (environment, agent) was
// seen on, what the hops between them cost at free flow and how much of that was detour, from what the packed state already
// offers after every frame: word 0 of hdp, head_id << 8 | count byte. NOT reference semantics: the reference writes no
// per-traveller output. The frame kernels are not touched; this file only READS the packed state.
//
// Two facts about the simulator carry the trace (tests/test_path_trace_host.py establishes both on the oracle):
//   1. after a frame an agent id other than 0 is the head of at most one non-empty road of an environment (an agent stands in
//      one FIFO; an agent lost to the U-turn double pop, quirk Q24, is queued nowhere), and
//   2. only heads move, and Direction reads the heads as of the start of the frame: an agent seen as head on p and next on
//      u != p crossed the edge p -> u in between.
//
// The rule, per (environment b, agent a in [1, A)), one SIGHTING PASS after every frame over every road u of environment b
// whose count bits (hdp.x & 0x7F; bit 7 is the packed state's DIRTY flag, not a count) are not 0, with a = hdp.x >> 8:
//   a == 0: nothing. a >= A: bad[b] += 1. p = last_road[b][a]; p == u: nothing. Otherwise u is a new road, h = roads[b][a]:
//     p >= 0: e = the first entry of p's CSR out-list whose target is u; none: bad[b] += 1 and no cost. With weights:
//       w = (double) weights[eid(e)], path_cost += w; s = dest_slot[a_dest[b][a]]; the destination out of range, s outside
//       [0, D) or dist[s][u] / dist[s][p] not finite: off_tree += 1; else excess += (w + dist[s][u]) - dist[s][p] in fp64, in
//       exactly this order (no multiply: nothing to contract).
//     any route[b][a][i] == u, i < min(h, L): revisits += 1 (the KEPT prefix only).  h < L: route[b][a][h] = u.
//     roads = h + 1, last_road = u.
#include <math.h>

#include "fused_common.h"

#define PT_ENVS 64                  // environments of one workgroup's tile: the lanes of a wave
#define PT_ROADS 4                  // roads of the tile: one per wave
#define PT_MAX_HOPS 4096            // = TARL_PATH_MAX_HOPS
#define PT_MAX_AGENTS ((int64_t)1 << 24)
#define PS_BLOCK 64                 // tarl_path_agent_stats: one wave of agents per workgroup

// ---- reset ---------------------------------------------------------------------------------------------------------------------
// The initial values are not all zero (last_road and route are -1): a flat grid over the largest of the arrays.
__global__ __launch_bounds__(256) void k_path_trace_reset(int64_t BA, int64_t BAL, int64_t B, int32_t* __restrict__ last_road,
                                                          int32_t* __restrict__ roads, int32_t* __restrict__ revisits,
                                                          int32_t* __restrict__ off_tree, double* __restrict__ path_cost,
                                                          double* __restrict__ excess, int32_t* __restrict__ route,
                                                          int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < BA) {
    last_road[i] = -1;
    roads[i] = 0;
    revisits[i] = 0;
    off_tree[i] = 0;
    path_cost[i] = 0.0;
    excess[i] = 0.0;
  }
  if (i < BAL) route[i] = -1;
  if (i < B) bad[i] = 0;
}

// ---- the sighting pass -----------------------------------------------------------------------------------------------------------
// One thread per (road, environment): wave w of the workgroup owns road n0 + w, its lanes the environments k0 + l, so that a
// wave's hdp loads are 64 consecutive records and the road is uniform over the wave (turn_counts.hip / occupancy.hip). A
// thread whose row is empty, or whose head stands where it was seen last, leaves after two loads (the word, last_road). Fact 1
// makes every (b, a) element single-writer within a launch: plain read-modify-write, no atomics — except bad[b], which any road
// of environment b may add to; it must stay 0 and the evaluator raises when it does not, so that never-taken path uses an
// integer atomicAdd (the precedent of `unresolved` in turn_counts.hip). The out-list search (out-degree <= 126) and the prefix
// scan (<= L <= 4096) run only on a new-road event. Tiles at the B and N edges are partial: a thread outside [N][B] returns
// before its first load, and every other access is indexed by (b, a) with a < A tested, by p in [0, N) tested, or by a CSR
// position of p's out-list.
__global__ __launch_bounds__(PT_ENVS* PT_ROADS) void k_fused_path_trace(
    const uint32_t* __restrict__ hdp, const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
    const int32_t* __restrict__ out_eid, const int32_t* __restrict__ a_dest, int64_t B, int64_t N, int64_t A, int32_t L,
    int64_t b_tiles, int32_t* __restrict__ last_road, int32_t* __restrict__ roads, int32_t* __restrict__ revisits,
    int32_t* __restrict__ off_tree, double* __restrict__ path_cost, double* __restrict__ excess, int32_t* __restrict__ route,
    int32_t* __restrict__ bad, const float* __restrict__ weights, const double* __restrict__ dist,
    const int32_t* __restrict__ dest_slot, int64_t D) {
  const int l = threadIdx.x & (PT_ENVS - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / PT_ENVS);
  const int64_t b = ((int64_t)blockIdx.x % b_tiles) * PT_ENVS + l, u = ((int64_t)blockIdx.x / b_tiles) * PT_ROADS + w;
  if (b >= B || u >= N) return;
  const uint32_t hd = hdp[2 * (u * B + b)];      // word 0 of the pair
  if ((hd & HD_CNT) == 0u) return;               // an empty row: whatever head id it still shows is stale
  const int64_t a = (int64_t)(hd >> 8);
  if (a == 0) return;
  if (a >= A) {
    atomicAdd(&bad[b], 1);
    return;
  }
  const int64_t idx = b * A + a;
  const int32_t p = last_road[idx];
  if (p == (int32_t)u) return;
  // a new road for this agent
  const int32_t h = roads[idx];
  if (p >= 0) {
    int32_t e = -1;
    if (p < N) {
      const int32_t e1 = out_ptr[p + 1];
      for (int32_t q = out_ptr[p]; q < e1; ++q)
        if (out_dst[q] == (int32_t)u) {
          e = q;
          break;
        }
    }
    if (e < 0) {
      atomicAdd(&bad[b], 1);
    } else if (weights) {
      const double wd = (double)weights[out_eid[e]];
      path_cost[idx] += wd;
      const int32_t dest = a_dest[idx];
      const int32_t s = (dest >= 0 && dest < N) ? dest_slot[dest] : -1;
      double du = INFINITY, dp = INFINITY;
      if (s >= 0 && s < D) {
        du = dist[(int64_t)s * N + u];
        dp = dist[(int64_t)s * N + p];
      }
      if (isfinite(du) && isfinite(dp))
        excess[idx] += (wd + du) - dp;
      else
        off_tree[idx] += 1;
    }
  }
  const int32_t m = h < L ? h : L;
  const int32_t* r = route + idx * (int64_t)L;      // (never dereferenced when L == 0: m == 0 and h < L is false)
  bool seen = false;
  for (int32_t i = 0; i < m && !seen; ++i) seen = r[i] == (int32_t)u;
  if (seen) revisits[idx] += 1;
  if (h >= 0 && h < L) route[idx * (int64_t)L + h] = (int32_t)u;
  roads[idx] = h + 1;
  last_road[idx] = (int32_t)u;
}

// sizes of the state arrays: every product below 2^40, the [B][A][L] one included
static int path_sizes(int64_t B, int64_t num_agents, int64_t L, const char** why) {
  const int64_t lim = (int64_t)1 << 40;
  if (!(B >= 1 && B < ((int64_t)1 << 31))) return *why = "bad sizes", 0;
  if (!(num_agents >= 1 && num_agents <= PT_MAX_AGENTS)) return *why = "num_agents must be in [1, 2^24]", 0;
  if (!(L >= 0 && L <= PT_MAX_HOPS)) return *why = "L must be in [0, 4096] (TARL_PATH_MAX_HOPS)", 0;
  if (!(B * num_agents < lim && B * num_agents * (L > 0 ? L : 1) < lim)) return *why = "bad sizes: the state arrays overflow", 0;
  return 1;
}

extern "C" int tarl_path_trace_reset(int64_t B, int64_t num_agents, int64_t L, int32_t* last_road, int32_t* roads,
                                     int32_t* revisits, int32_t* off_tree, double* path_cost, double* excess, int32_t* route,
                                     int32_t* bad, tarl_stream stream) {
  TARL_REQUIRE(last_road && roads && revisits && off_tree && path_cost && excess && bad, "null argument");
  const char* why = "";
  TARL_REQUIRE(path_sizes(B, num_agents, L, &why), why);
  TARL_REQUIRE(L == 0 || route, "null argument: route (L > 0)");
  const int64_t BA = B * num_agents, BAL = BA * L;      // BA >= B: the grid over max(BA, BAL) covers bad[] too
  const int64_t n = BAL > BA ? BAL : BA, blocks = ceil_div(n, 256);
  TARL_REQUIRE(blocks < ((int64_t)1 << 31), "bad sizes: too many elements for one launch");
  hipLaunchKernelGGL(k_path_trace_reset, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, BA, BAL, B, last_road,
                     roads, revisits, off_tree, path_cost, excess, route, bad);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_fused_path_trace(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                     int64_t L, int32_t* last_road, int32_t* roads, int32_t* revisits, int32_t* off_tree,
                                     double* path_cost, double* excess, int32_t* route, int32_t* bad, const float* weights,
                                     const double* dist, const int32_t* dest_slot, int64_t num_dests, tarl_stream stream) {
  TARL_REQUIRE(plan && f && last_road && roads && revisits && off_tree && path_cost && excess && bad, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  const char* why = "";
  TARL_REQUIRE(path_sizes(B, num_agents, L, &why), why);
  TARL_REQUIRE(L == 0 || route, "null argument: route (L > 0)");
  TARL_REQUIRE((!weights == !dist) && (!weights == !dest_slot), "weights, dist and dest_slot come together");
  TARL_REQUIRE(!weights || (num_dests >= 1 && num_dests < ((int64_t)1 << 31) && num_dests * plan->N < ((int64_t)1 << 40)),
               "bad sizes: num_dests");
  TARL_REQUIRE(!weights || f->a_dest, "fused agent buffers missing (a_dest)");
  if (plan->N == 0) return TARL_OK;
  const int64_t b_tiles = ceil_div(B, PT_ENVS), tiles = b_tiles * ceil_div(plan->N, PT_ROADS);
  TARL_REQUIRE(tiles < ((int64_t)1 << 31), "bad sizes: too many tiles for one launch");
  hipLaunchKernelGGL(k_fused_path_trace, dim3((unsigned)tiles), dim3(PT_ENVS * PT_ROADS), 0, (hipStream_t)stream,
                     (const uint32_t*)f->hdp, plan->out_ptr, plan->out_dst, plan->out_eid, (const int32_t*)f->a_dest, B, plan->N,
                     num_agents, (int32_t)L, b_tiles, last_road, roads, revisits, off_tree, path_cost, excess, route, bad,
                     weights, dist, dest_slot, num_dests);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- per agent over the environments ----------------------------------------------------------------------------------------------
// The counterpart of tarl_trip_agent_stats for the trace: one thread per agent, the lanes of a wave along the agent axis of the
// [K][A] arrays (64 consecutive elements per load; the DONE flags are 36 B apart, as in trips.hip), a loop over k = 0, 1, ...
// in order: every fp64 sum starts from +0.0 and adds the environments in ascending order, bit-identical from run to run.
//   out_i32 [8][A]:  0 n_done, 1 n_zero_excess, 2 n_loop, 3 n_trunc (over the environments in which the agent is DONE),
//                    4 n_seen, 5 n_loop_all, 6 max roads (over all environments), 7 n_both (PAIR; else left alone)
//   out_f64 [10][A]: 0/1 sum and sum of squares of moves = max(roads - 1, 0), 2/3 of path_cost, 4/5 of excess (DONE);
//                    6/7 of moves - moves_b, 8/9 of excess - excess_b over the environments DONE in both runs (PAIR)
// Entry 0 (the dummy) is written as zero.
template <bool PAIR>
__global__ __launch_bounds__(PS_BLOCK) void k_path_agent_stats(
    const int32_t* __restrict__ roads, const int32_t* __restrict__ revisits, const int32_t* __restrict__ off_tree,
    const double* __restrict__ path_cost, const double* __restrict__ excess, const float* __restrict__ ag, int64_t a_bstride,
    const int32_t* __restrict__ roads_b, const double* __restrict__ excess_b, const float* __restrict__ agb, int64_t b_bstride,
    int64_t K, int64_t A, int32_t L, int32_t* __restrict__ out_i32, double* __restrict__ out_f64) {
  const int64_t a = (int64_t)blockIdx.x * PS_BLOCK + threadIdx.x;
  if (a >= A) return;
  int32_t n_done = 0, n_zero = 0, n_loop = 0, n_trunc = 0, n_seen = 0, n_loop_all = 0, r_max = 0, n_both = 0;
  double m1 = 0.0, m2 = 0.0, c1 = 0.0, c2 = 0.0, x1 = 0.0, x2 = 0.0, dm1 = 0.0, dm2 = 0.0, dx1 = 0.0, dx2 = 0.0;
  if (a >= 1) {
    for (int64_t k = 0; k < K; ++k) {
      const int64_t i = k * A + a;
      const int32_t r = roads[i], rv = revisits[i];
      const bool done = ag[k * a_bstride + a * AG_COLS + AG_DONE] == 1.0f;
      n_seen += r > 0 ? 1 : 0;
      n_loop_all += rv > 0 ? 1 : 0;
      r_max = r > r_max ? r : r_max;
      const double mv = (double)(r > 1 ? r - 1 : 0);
      if (done) {
        const double pc = path_cost[i], ex = excess[i];
        n_done += 1;
        n_zero += (ex == 0.0 && off_tree[i] == 0) ? 1 : 0;
        n_loop += rv > 0 ? 1 : 0;
        n_trunc += r > L ? 1 : 0;
        m1 += mv;
        m2 += mv * mv;
        c1 += pc;
        c2 += pc * pc;
        x1 += ex;
        x2 += ex * ex;
        if (PAIR && agb[k * b_bstride + a * AG_COLS + AG_DONE] == 1.0f) {
          const int32_t rb = roads_b[i];
          const double dm = mv - (double)(rb > 1 ? rb - 1 : 0), dx = ex - excess_b[i];
          n_both += 1;
          dm1 += dm;
          dm2 += dm * dm;
          dx1 += dx;
          dx2 += dx * dx;
        }
      }
    }
  }
  out_i32[0 * A + a] = n_done;
  out_i32[1 * A + a] = n_zero;
  out_i32[2 * A + a] = n_loop;
  out_i32[3 * A + a] = n_trunc;
  out_i32[4 * A + a] = n_seen;
  out_i32[5 * A + a] = n_loop_all;
  out_i32[6 * A + a] = r_max;
  out_f64[0 * A + a] = m1;
  out_f64[1 * A + a] = m2;
  out_f64[2 * A + a] = c1;
  out_f64[3 * A + a] = c2;
  out_f64[4 * A + a] = x1;
  out_f64[5 * A + a] = x2;
  if (PAIR) {
    out_i32[7 * A + a] = n_both;
    out_f64[6 * A + a] = dm1;
    out_f64[7 * A + a] = dm2;
    out_f64[8 * A + a] = dx1;
    out_f64[9 * A + a] = dx2;
  }
}

extern "C" int tarl_path_agent_stats(const int32_t* roads, const int32_t* revisits, const int32_t* off_tree,
                                     const double* path_cost, const double* excess, const float* agents, int64_t a_bstride,
                                     const int32_t* roads_b, const double* excess_b, const float* agents_b, int64_t b_bstride,
                                     int64_t K, int64_t num_agents, int64_t L, int32_t* out_i32, double* out_f64,
                                     tarl_stream stream) {
  TARL_REQUIRE(roads && revisits && off_tree && path_cost && excess && agents && out_i32 && out_f64, "null argument");
  TARL_REQUIRE((!roads_b == !excess_b) && (!roads_b == !agents_b), "null argument: roads_b, excess_b and agents_b come together");
  const char* why = "";
  TARL_REQUIRE(path_sizes(K, num_agents, L, &why), why);
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TARL_REQUIRE(!agents_b || b_bstride >= num_agents * AG_COLS, "agent tables overlap (agents_b)");
  const dim3 grid((unsigned)ceil_div(num_agents, PS_BLOCK)), block(PS_BLOCK);
  if (agents_b)
    hipLaunchKernelGGL(k_path_agent_stats<true>, grid, block, 0, (hipStream_t)stream, roads, revisits, off_tree, path_cost,
                       excess, agents, a_bstride, roads_b, excess_b, agents_b, b_bstride, K, num_agents, (int32_t)L, out_i32,
                       out_f64);
  else
    hipLaunchKernelGGL(k_path_agent_stats<false>, grid, block, 0, (hipStream_t)stream, roads, revisits, off_tree, path_cost,
                       excess, agents, a_bstride, roads_b, excess_b, agents_b, b_bstride, K, num_agents, (int32_t)L, out_i32,
                       out_f64);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
