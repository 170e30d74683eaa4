// goal_mlp.hip — the goal-conditioned policy head of MPNNPolicyNet (policy_head = "goal_mlp"; NOT in the reference): a small
// per-edge MLP on destination-relative features, built from what the prior head (prior.hip) already reads. For a route edge
// e = (u -> v):
//
//     d      = (long) DESTINATION of u's head agent      (read as prior.hip reads it: an empty FIFO, or an id outside [0, A),
//                                                          reads agent 0)
//     D(e)   = tab(v, d)                                   (PriorAllPairs / PriorPerDest, prior_tables.h; +inf: unreachable,
//                                                          out of range, or no column)
//     tt(v)  = prior_time_travel(v)                        (the prior's congested travel time, same fp32 operation order)
//     c(e)   = D(e) + tt(v);   e is REACHABLE when c(e) is finite;   cmin(u) = min of c over u's reachable out-edges
//     S      = time_scale > 0 (the mean FREE_FLOW over the roads, computed by the host)
//
//     g0 = min((c - cmin) / S, 8)    (8 on an unreachable edge)      g4 = NUMBER_OF_AGENT(u) / MAXN(u), 0 where MAXN <= 0
//     g1 = v == d ? 1 : 0                                            g5 = min(D / S, 64) / 8
//     g2 = min(tt / FF(v) - 1, 8), 0 unless FF(v) > 0                g6 = NUMBER_OF_AGENT(u) == 0 ? 1 : 0
//     g3 = NUMBER_OF_AGENT(v) / MAXN(v), 0 where MAXN <= 0           g7 = min(FF(v) / S, 8)
//
//     logit = the 8 -> 16 (ReLU) -> 1 network of mlp8.h on g (its operation order, its flat layout of MLP8_NW floats:
//             goal_mlp.0.weight, .0.bias, .2.weight, .2.bias)
//
// so a numpy fp32 restatement reproduces features and logits bit for bit. An unreachable edge gets exactly PRIOR_UNREACHABLE
// (-1e20), not mlp - 1e20, and takes no part in the backward; no inf or NaN is emitted.
//
// Producers:
//   * from observations obs16 [M][N][16] (tarl_policy_goal_features, tarl_policy_goal_mlp_fwd, tarl_policy_goal_mlp_bwd): one
//     thread per (sample, edge) in original edge order, which walks u's out-list for cmin (served by L1) and then evaluates
//     its own edge. The backward recomputes the features; a workgroup owns a fixed run of (sample, edge) pairs and puts them
//     through mlp8.h's gradient scheme a tile at a time, every lane of the tile a staged row, in pair order. The partials
//     [partition][MLP8_NW] go to the caller's scratch, k_goal_bwd_sum adds them in partition order and ACCUMULATES (+=) into
//     grads, as tarl_policy_edge_mlp_bwd does. No float atomics: two runs are bit-identical.
//   * tarl_fused_goal_mlp_logits: from the packed state, k_prior_fused's shape (a workgroup owns 64 environments x 64 CSR
//     positions, lanes along the environments, u and v wave-uniform, the tile turned through LDS). Each wave takes 16
//     CONSECUTIVE positions, so the out-list of a node falls to one wave where it can: on entering a node the wave walks the
//     node's whole out-list once for cmin (wherever the list starts and ends: a list that straddles waves or tiles is walked
//     by each of them), then evaluates its own positions, the second read of the same words served by L1/L2. The weights
//     are wave-uniform reads of one const __restrict__ array (scalar loads).
//   * tarl_fused_rollout_goal: the shared loop of the state-dependent heads (tarl_rollout_head) with this head's frame.
#include <math.h>

#include "mlp8.h"
#include "prior_tables.h"
#include "rollout_heads.h"

#define GM_BLOCK MLP8_ROWS
#define GM_TE 64            // environments per fused tile (one per lane)
#define GM_TK 64            // CSR positions per fused tile
#define GM_WK (GM_TK / (GM_BLOCK / 64))     // consecutive positions per wave
#define GM_MAX_PARTS 1024   // partial-sum rows of the backward at most

struct GoalCand {
  float D, tt, ff, maxn, na;
};

__device__ __forceinline__ bool goal_finite(float c) { return fabsf(c) <= 3.4028234663852886e38f; }     // false for NaN

__device__ __forceinline__ void goal_features(const GoalCand& q, float cmin, bool reach, bool v_is_d, float maxnu, float nau,
                                              float S, float g[MLP8_NF]) {
  g[0] = reach ? fminf(((q.D + q.tt) - cmin) / S, 8.0f) : 8.0f;
  g[1] = v_is_d ? 1.0f : 0.0f;
  g[2] = (q.ff > 0.0f) ? fminf(q.tt / q.ff - 1.0f, 8.0f) : 0.0f;
  g[3] = (q.maxn > 0.0f) ? q.na / q.maxn : 0.0f;
  g[4] = (maxnu > 0.0f) ? nau / maxnu : 0.0f;
  g[5] = fminf(q.D / S, 64.0f) / 8.0f;
  g[6] = (nau == 0.0f) ? 1.0f : 0.0f;
  g[7] = fminf(q.ff / S, 8.0f);
}

static __device__ __forceinline__ bool goal_v_is_d(int64_t v, float dest_f) { return (long long)dest_f == (long long)v; }

// ---- from observations ---------------------------------------------------------------------------------------------------
template <class Tab>
__device__ __forceinline__ GoalCand goal_cand_obs(const float* __restrict__ om, int64_t v, float dest, const Tab& tab) {
  const float4 a = *reinterpret_cast<const float4*>(om + v * 16);     // {MAXN, NUMBER_OF_AGENT, FF, LENGTH}
  return GoalCand{tab(v, dest), prior_time_travel(a.z, a.x, om[v * 16 + 4], a.y), a.z, a.x, a.y};
}

// features of edge e of sample row om = obs + m * N * 16 -> g; true when the edge is reachable
template <class Tab>
__device__ __forceinline__ bool goal_edge_obs(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                              const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                              const float* __restrict__ om, int64_t e, const Tab& tab, float S,
                                              float g[MLP8_NF]) {
  const int64_t u = src[e], v = dst[e];
  const float maxnu = om[u * 16 + 0], nau = om[u * 16 + 1], dest = om[u * 16 + 8];
  float cmin = INFINITY;
  for (int32_t j = out_ptr[u], j1 = out_ptr[u + 1]; j < j1; ++j) {
    const GoalCand q = goal_cand_obs(om, out_dst[j], dest, tab);
    const float c = q.D + q.tt;
    if (goal_finite(c)) cmin = fminf(cmin, c);
  }
  const GoalCand q = goal_cand_obs(om, v, dest, tab);
  const bool reach = goal_finite(q.D + q.tt);
  goal_features(q, cmin, reach, goal_v_is_d(v, dest), maxnu, nau, S, g);
  return reach;
}

struct GoalGraph {
  const int32_t *src, *dst, *out_ptr, *out_dst;
  int64_t N, E;
};

static GoalGraph goal_graph(const tarl_plan* p) { return GoalGraph{p->src, p->dst, p->out_ptr, p->out_dst, p->N, p->E}; }

template <class Tab>
__global__ __launch_bounds__(GM_BLOCK) void k_goal_feats(GoalGraph G, const float* __restrict__ obs, int64_t M, Tab tab,
                                                         float S, float* __restrict__ feats) {
  const int64_t gid = (int64_t)blockIdx.x * GM_BLOCK + threadIdx.x;
  if (gid >= M * G.E) return;
  const int64_t m = gid / G.E, e = gid - m * G.E;
  float g[MLP8_NF];
  goal_edge_obs(G.src, G.dst, G.out_ptr, G.out_dst, obs + m * G.N * 16, e, tab, S, g);
  float4* o = reinterpret_cast<float4*>(feats + gid * MLP8_NF);
  o[0] = make_float4(g[0], g[1], g[2], g[3]);
  o[1] = make_float4(g[4], g[5], g[6], g[7]);
}

template <class Tab>
__global__ __launch_bounds__(GM_BLOCK) void k_goal_fwd(GoalGraph G, const float* __restrict__ obs, int64_t M, Tab tab, float S,
                                                       const float* __restrict__ w, float* __restrict__ logits) {
  const int64_t gid = (int64_t)blockIdx.x * GM_BLOCK + threadIdx.x;
  if (gid >= M * G.E) return;
  const int64_t m = gid / G.E, e = gid - m * G.E;
  float g[MLP8_NF];
  const bool reach = goal_edge_obs(G.src, G.dst, G.out_ptr, G.out_dst, obs + m * G.N * 16, e, tab, S, g);
  logits[gid] = reach ? mlp8_eval(w, g) : PRIOR_UNREACHABLE;
}

// Partition p owns the pairs [p * chunk, min((p + 1) * chunk, M * E)), chunk a multiple of GM_BLOCK: a function of the
// shapes alone. Every pair of a tile is a staged row, in pair order (mlp8.h); an unreachable pair is a row of exact zeros,
// whatever its grad_logits.
template <class Tab>
__global__ __launch_bounds__(GM_BLOCK) void k_goal_bwd(GoalGraph G, const float* __restrict__ obs, int64_t M, Tab tab, float S,
                                                       const float* __restrict__ w, const float* __restrict__ gl,
                                                       int64_t chunk, float* __restrict__ partial) {
  MLP8_STAGE_ARRAYS;
  const int t = threadIdx.x;
  const int64_t total = M * G.E;
  const int64_t p0 = (int64_t)blockIdx.x * chunk, p1 = (p0 + chunk < total) ? p0 + chunk : total;
  float acc = 0.0f;
  for (int64_t base = p0; base < p1; base += GM_BLOCK) {
    const int64_t gid = base + t;
    float g[MLP8_NF], a[MLP8_NH], gh[MLP8_NH], r = 0.0f;
#pragma unroll
    for (int k = 0; k < MLP8_NF; ++k) g[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < MLP8_NH; ++j) a[j] = gh[j] = 0.0f;
    if (gid < p1) {
      const int64_t m = gid / G.E, e = gid - m * G.E;
      if (goal_edge_obs(G.src, G.dst, G.out_ptr, G.out_dst, obs + m * G.N * 16, e, tab, S, g)) {
        r = gl[gid];
#pragma unroll
        for (int j = 0; j < MLP8_NH; ++j) mlp8_row_unit(w, g, r, j, &a[j], &gh[j]);
      } else {
#pragma unroll
        for (int k = 0; k < MLP8_NF; ++k) g[k] = 0.0f;     // an unreachable pair adds exact zeros, whatever its grad_logits
      }
    }
    __syncthreads();     // the previous tile has been summed
#pragma unroll
    for (int j = 0; j < MLP8_NH; ++j) {
      s_a[t][j] = a[j];
      s_h[t][j] = gh[j];
    }
#pragma unroll
    for (int k = 0; k < MLP8_NF; ++k) s_f[t][k] = g[k];
    s_r[t] = r;
    __syncthreads();
    const int n = (int)((p1 - base < GM_BLOCK) ? p1 - base : GM_BLOCK);
    MLP8_ACCUMULATE(acc, t, n)
  }
  mlp8_write_partial(partial, blockIdx.x, t, acc);
}

// One thread per element, the partitions in order. NOT k_dcr_sum's wave per element (decision_critic.hip): that one adds in
// another order, so sharing either would change the other's gradient bits (mlp8.h).
__global__ __launch_bounds__(GM_BLOCK) void k_goal_bwd_sum(const float* __restrict__ partial, int64_t parts,
                                                           float* __restrict__ grads) {
  const int t = threadIdx.x;
  if (t >= MLP8_NW) return;
  float s = 0.0f;
  for (int64_t p = 0; p < parts; ++p) s = s + partial[p * MLP8_NW + t];
  grads[t] = grads[t] + s;
}

// -> the pairs per partition (a multiple of GM_BLOCK) and the number of partitions of M * E pairs
static void goal_partition(int64_t total, int64_t* chunk, int64_t* parts) {
  const int64_t tiles = ceil_div(total, GM_BLOCK);
  const int64_t per = ceil_div(tiles, GM_MAX_PARTS);
  *chunk = per * GM_BLOCK;
  *parts = ceil_div(tiles, per);
}

static int goal_check_table(const tarl_plan* plan, const float* table, int64_t table_cols, const int32_t* dest_slot,
                            float time_scale) {
  TARL_REQUIRE(plan && table, "null argument");
  TARL_REQUIRE(time_scale > 0.0f && time_scale <= 3.0e38f, "time_scale must be finite and > 0");
  if (!dest_slot) {
    TARL_REQUIRE(table_cols == plan->N, "distance table is not N x N for this plan (dest_slot is null)");
  } else {
    TARL_REQUIRE(table_cols >= 1, "the per-destination table needs at least one column");
  }
  return TARL_OK;
}

static int goal_check_obs(const tarl_plan* plan, const float* obs16, int64_t M) {
  TARL_REQUIRE(obs16, "null argument");
  TARL_REQUIRE(M >= 1, "bad sizes");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0, "obs16 must be 16-byte aligned");
  TARL_REQUIRE(M <= ((int64_t)1 << 40) / (plan->E > 0 ? plan->E : 1) && ceil_div(M * plan->E, GM_BLOCK) < 2147483647LL,
               "too many (sample, edge) pairs for one grid dimension");
  return TARL_OK;
}

// calls fn(tab) with the lookup the arguments name
template <class F>
static int goal_with_table(const tarl_plan* plan, const float* table, int64_t table_cols, const int32_t* dest_slot, F fn) {
  if (!dest_slot) return fn(PriorAllPairs{table, plan->N});
  return fn(PriorPerDest{table, dest_slot, plan->N, table_cols});
}

extern "C" int tarl_policy_goal_features(const tarl_plan* plan, const float* obs16, int64_t M, const float* table,
                                         int64_t table_cols, const int32_t* dest_slot, float time_scale, float* feats,
                                         tarl_stream stream) {
  int rc = goal_check_table(plan, table, table_cols, dest_slot, time_scale);
  if (rc) return rc;
  TARL_REQUIRE(feats, "null argument");
  TARL_REQUIRE(((uintptr_t)feats) % 16 == 0, "feats must be 16-byte aligned");
  if ((rc = goal_check_obs(plan, obs16, M))) return rc;
  if (plan->E == 0) return TARL_OK;
  return goal_with_table(plan, table, table_cols, dest_slot, [&](auto tab) -> int {
    hipLaunchKernelGGL(k_goal_feats<decltype(tab)>, dim3((unsigned)ceil_div(M * plan->E, GM_BLOCK)), dim3(GM_BLOCK), 0,
                       (hipStream_t)stream, goal_graph(plan), obs16, M, tab, time_scale, feats);
    TARL_LAUNCH_CHECK();
    return (int)TARL_OK;
  });
}

extern "C" int tarl_policy_goal_mlp_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* table,
                                        int64_t table_cols, const int32_t* dest_slot, float time_scale, const float* weights,
                                        float* logits, tarl_stream stream) {
  int rc = goal_check_table(plan, table, table_cols, dest_slot, time_scale);
  if (rc) return rc;
  TARL_REQUIRE(weights && logits, "null argument");
  if ((rc = goal_check_obs(plan, obs16, M))) return rc;
  if (plan->E == 0) return TARL_OK;
  return goal_with_table(plan, table, table_cols, dest_slot, [&](auto tab) -> int {
    hipLaunchKernelGGL(k_goal_fwd<decltype(tab)>, dim3((unsigned)ceil_div(M * plan->E, GM_BLOCK)), dim3(GM_BLOCK), 0,
                       (hipStream_t)stream, goal_graph(plan), obs16, M, tab, time_scale, weights, logits);
    TARL_LAUNCH_CHECK();
    return (int)TARL_OK;
  });
}

extern "C" int64_t tarl_policy_goal_mlp_bwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 1) return -1;
  if (plan->E == 0) return 0;
  if (M > ((int64_t)1 << 40) / plan->E || ceil_div(M * plan->E, GM_BLOCK) >= 2147483647LL) return -1;
  int64_t chunk, parts;
  goal_partition(M * plan->E, &chunk, &parts);
  return parts * MLP8_NW;
}

extern "C" int tarl_policy_goal_mlp_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* table,
                                        int64_t table_cols, const int32_t* dest_slot, float time_scale, const float* weights,
                                        const float* grad_logits, float* grads, float* scratch, tarl_stream stream) {
  int rc = goal_check_table(plan, table, table_cols, dest_slot, time_scale);
  if (rc) return rc;
  TARL_REQUIRE(weights && grad_logits && grads && scratch, "null argument");
  TARL_REQUIRE(((uintptr_t)scratch) % 16 == 0, "scratch must be 16-byte aligned");
  if ((rc = goal_check_obs(plan, obs16, M))) return rc;
  if (plan->E == 0) return TARL_OK;
  int64_t chunk, parts;
  goal_partition(M * plan->E, &chunk, &parts);
  rc = goal_with_table(plan, table, table_cols, dest_slot, [&](auto tab) -> int {
    hipLaunchKernelGGL(k_goal_bwd<decltype(tab)>, dim3((unsigned)parts), dim3(GM_BLOCK), 0, (hipStream_t)stream,
                       goal_graph(plan), obs16, M, tab, time_scale, weights, grad_logits, chunk, scratch);
    TARL_LAUNCH_CHECK();
    return (int)TARL_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_goal_bwd_sum, dim3(1), dim3(GM_BLOCK), 0, (hipStream_t)stream, scratch, parts, grads);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- from the packed state -------------------------------------------------------------------------------------------------
struct GoalState {
  const uint2* hdp;
  const float4* st0;     // {MAXN, FF, ROAD_INDEX, congestion_constant}
  const float* x0;      // MAX_FLOW of road 0 (the static columns of environment 0), row stride ldx
  int64_t ldx;
  const float* ag;
  int64_t A, a_bstride;
};

template <class Tab>
__device__ __forceinline__ GoalCand goal_cand_fused(const GoalState& s, int64_t B, int64_t b, int32_t v, float dest,
                                                    const Tab& tab) {
  const uint32_t hv = s.hdp[(int64_t)v * B + b].x;
  const float4 st = s.st0[v];
  const float na = (float)(hv & HD_CNT);
  return GoalCand{tab(v, dest), prior_time_travel(st.y, st.x, s.x0[(int64_t)v * s.ldx], na), st.y, st.x, na};
}

template <class Tab>
__global__ __launch_bounds__(GM_BLOCK) void k_goal_fused(const int32_t* __restrict__ src, const int32_t* __restrict__ out_ptr,
                                                         const int32_t* __restrict__ out_dst,
                                                         const int32_t* __restrict__ out_eid, int32_t B, int32_t E,
                                                         GoalState s, Tab tab, float S, const float* __restrict__ w,
                                                         float* __restrict__ logits) {
  __shared__ float tile[GM_TE][GM_TK + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t b0 = (int32_t)blockIdx.x * GM_TE, k0 = (int32_t)blockIdx.y * GM_TK;     // B, E < 65536 * 64 (host check)
  const int32_t b = b0 + lane;
  int32_t u_prev = -1;
  float cmin = INFINITY, dest = 0.0f, nau = 0.0f, maxnu = 0.0f;
  for (int kk = wv * GM_WK; kk < (wv + 1) * GM_WK; ++kk) {     // consecutive CSR positions: u, v wave-uniform
    const int32_t k = k0 + kk;
    if (k >= E) break;
    const int32_t u = src[out_eid[k]], v = out_dst[k];
    float l = 0.0f;
    if (b < B) {
      if (u != u_prev) {     // entering a node: its head's destination and the minimum over its whole out-list
        const uint32_t hu = s.hdp[(int64_t)u * B + b].x;
        const long long head = (long long)(hu >> 8);
        dest = s.ag[(int64_t)b * s.a_bstride + ((head >= 0 && head < s.A) ? head : 0) * AG_COLS + AG_DEST];
        nau = (float)(hu & HD_CNT);
        maxnu = s.st0[u].x;
        cmin = INFINITY;
        for (int32_t j = out_ptr[u], j1 = out_ptr[u + 1]; j < j1; ++j) {
          const GoalCand q = goal_cand_fused(s, B, b, out_dst[j], dest, tab);
          const float c = q.D + q.tt;
          if (goal_finite(c)) cmin = fminf(cmin, c);
        }
      }
      const GoalCand q = goal_cand_fused(s, B, b, v, dest, tab);
      const bool reach = goal_finite(q.D + q.tt);
      float g[MLP8_NF];
      goal_features(q, cmin, reach, goal_v_is_d(v, dest), maxnu, nau, S, g);
      l = reach ? mlp8_eval(w, g) : PRIOR_UNREACHABLE;
    }
    u_prev = u;
    tile[lane][kk] = l;
  }
  __syncthreads();
  const int32_t k = k0 + lane;
  if (k >= E) return;
  const int32_t e = out_eid[k];
  for (int r = wv; r < GM_TE; r += GM_BLOCK / 64) {
    const int32_t bb = b0 + r;
    if (bb < B) logits[(int64_t)bb * E + e] = tile[r][lane];
  }
}

static int goal_check_state(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, const float* x,
                            const float* agent_features, int64_t A, const float* table, int64_t table_cols,
                            const int32_t* dest_slot, float time_scale, const float* weights) {
  int rc = goal_check_table(plan, table, table_cols, dest_slot, time_scale);
  if (rc) return rc;
  TARL_REQUIRE(f && x && agent_features && weights, "null argument");
  TARL_REQUIRE(B >= 1 && A >= 1, "bad sizes");
  TARL_REQUIRE(ceil_div(plan->E, GM_TK) < 65536 && ceil_div(B, GM_TE) < 65536, "too many tiles for one grid dimension");
  return tarl_check_fused_core(plan, f, B, Nmax);
}

template <class Tab>
static int launch_goal_fused(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, const float* x, int64_t ldx,
                             const float* agent_features, int64_t A, int64_t a_bstride, Tab tab, float time_scale,
                             const float* weights, float* logits, hipStream_t s) {
  const FusedBufs fb = tarl_to_bufs(f);
  const Layout L{Nmax, ldx, 0};
  const GoalState st{fb.hdp, fb.st0, x + L.col_maxflow(), ldx, agent_features, A, a_bstride};
  hipLaunchKernelGGL(k_goal_fused<Tab>, dim3((unsigned)ceil_div(B, GM_TE), (unsigned)ceil_div(plan->E, GM_TK)), dim3(GM_BLOCK),
                     0, s, plan->src, plan->out_ptr, plan->out_dst, plan->out_eid, (int32_t)B, (int32_t)plan->E, st, tab,
                     time_scale, weights, logits);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_fused_goal_mlp_logits(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B,
                                          int64_t x_bstride, int64_t ldx, int32_t Nmax, const float* agent_features,
                                          int64_t num_agents, int64_t a_bstride, const float* table, int64_t table_cols,
                                          const int32_t* dest_slot, float time_scale, const float* weights, float* logits,
                                          tarl_stream stream) {
  (void)x_bstride;    // the static columns of environment 0 speak for all
  int rc = goal_check_state(plan, f, B, Nmax, x, agent_features, num_agents, table, table_cols, dest_slot, time_scale, weights);
  if (rc) return rc;
  TARL_REQUIRE(logits, "null argument");
  if (plan->E == 0) return TARL_OK;
  return goal_with_table(plan, table, table_cols, dest_slot, [&](auto tab) -> int {
    return launch_goal_fused(plan, f, B, Nmax, x, ldx, agent_features, num_agents, a_bstride, tab, time_scale, weights, logits,
                             (hipStream_t)stream);
  });
}

// ---- the rollout head (rollout_heads.h): kept observation rows and the logits of one frame ---------------------------------
template <class Tab>
struct GoalHead {
  Tab tab;
  float time_scale;
  const float* weights;
};

template <class Tab>
static int goal_frame(const HeadRollout& a, void* ctx, int64_t, const int32_t* env, const int32_t* slot, int64_t n) {
  const GoalHead<Tab>& h = *(const GoalHead<Tab>*)ctx;
  const int rc = tarl_head_keep_rows(a, env, slot, n);
  if (rc || a.plan->E == 0) return rc;
  return launch_goal_fused(a.plan, a.f, a.B, a.Nmax, a.x, a.ldx, a.agent_features, a.A, a.a_bstride, h.tab, h.time_scale,
                           h.weights, a.logits_scratch, (hipStream_t)a.stream);
}

extern "C" int tarl_fused_rollout_goal(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                       const float* times_host, float prev_time, const float* x, int64_t x_bstride,
                                       int64_t ldx, float* agent_features, int64_t A, int64_t a_bstride,
                                       const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong,
                                       const float* table, int64_t table_cols, const int32_t* dest_slot, float time_scale,
                                       const float* weights, float temperature, uint64_t policy_seed,
                                       uint64_t policy_counter0, uint64_t seed, uint64_t counter0,
                                       const int64_t* keep_ptr_host, const int32_t* keep_env, const int32_t* keep_slot,
                                       float* obs_keep, float* logits_scratch, void* dist_scratch, int32_t* ins_scratch,
                                       uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                                       tarl_stream stream) {
  int rc = goal_check_state(plan, f, B, Nmax, x, agent_features, A, table, table_cols, dest_slot, time_scale, weights);
  if (rc) return rc;
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  const HeadRollout a{plan, f, B, Nmax, T, times_host, prev_time, x, x_bstride, ldx, agent_features, A, a_bstride, edge_attr,
                      log_edge_attr, log_eps, use_cong, temperature, policy_seed, policy_counter0, seed, counter0,
                      keep_ptr_host, keep_env, keep_slot, obs_keep, logits_scratch, dist_scratch, ins_scratch, choice8,
                      log_prob, reward, counts, 0, nullptr, nullptr, nullptr, stream};
  return goal_with_table(plan, table, table_cols, dest_slot, [&](auto tab) -> int {
    GoalHead<decltype(tab)> h{tab, time_scale, weights};
    return tarl_rollout_head(a, goal_frame<decltype(tab)>, &h);
  });
}
