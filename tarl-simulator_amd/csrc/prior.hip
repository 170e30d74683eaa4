// prior.hip — the shortest-path prior head of MPNNPolicyNet (policy_head = "embedding_dijkstra"):
//
//     logit[e] = W_emb[ROAD_INDEX(v)] + prior_weight * ((-dist[v][dest(u)]) - time_travel(v)),   u = src(e), v = dst(e)
//     time_travel(v) = max(FF, FF * (MAXN + 10 - MAX_FLOW * FF / 3600) / (MAXN + 10 - NUMBER_OF_AGENT))   (of road v)
//
// The reference computes every term (src/agents/mpnn_agent.py:180-187, compute_dijkstra_logits :81-113) and leaves the sum
// commented out (:188); this is that sum with a weight on the prior. fp32, the reference's operation order (the library is
// built with -ffp-contract=off). dest(u) = (long) DESTINATION of u's head agent, read exactly as the observation kernels read
// it (tarl_policy_obs16 / tarl_fused_obs16: an empty FIFO's head id, and an id outside [0, A), read agent 0).
// dist = the free-flow all-pairs table [N][N] of MPNNPolicyNet.dist_matrix (tarl_apsp), +inf where unreachable.
//
// Unreachable pairs. A candidate whose destination cannot be reached from v (dist = +inf, or a destination id outside
// [0, N)) gets the prior PRIOR_UNREACHABLE = -1e20 instead of prior_weight * (-inf): the segment softmax subtracts the node's
// maximum, so next to any reachable candidate its probability is exp(-1e20 + O(1e12)) = 0 exactly (the reference's value);
// when every candidate of a node is unreachable (the reference's softmax is NaN there) all of them carry W_emb + -1e20,
// which rounds to -1e20 for |W_emb| < 2^43 — the node draws uniformly among its out-edges. No inf or NaN is ever emitted
// (the logits stay finite after division by a temperature >= 1e-18), so probabilities, samples, log-probs, entropies and
// their gradients stay finite. The logit depends on W_emb with derivative 1 on every edge, reachable or not, which is what
// tarl_policy_edge_logits_bwd propagates.
//
// Two producers of the same numbers:
//   * tarl_policy_prior_logits: from observations obs16 [M][N][16] (the tarl_policy_obs16 layout) — the module forward and
//     the PPO update. One thread per (sample, edge), original edge order: coalesced logits stores.
//   * tarl_fused_prior_logits: from the fused engine's packed state (count byte + head id of hdp) and the static columns, no
//     observation written — the rollout's hot path. A workgroup owns 64 environments x 64 CSR positions: lanes run along
//     the environments, so the packed words are read as contiguous 512-byte runs, the source/target road of a position is
//     wave-uniform, and the table row dist[v] is one row for the whole wave (the table is stored [candidate][destination]:
//     the 64 lanes gather inside one row of N floats instead of touching 64 rows). The [64 env][64 edge] tile is turned
//     through LDS and leaves as 256-byte runs of each environment's logits row.
// tarl_fused_rollout_prior is the shared rollout loop of the state-dependent heads (tarl_rollout_head, rollout_heads.h) with
// this head's frame function: per frame kept observation rows -> prior logits, then the loop's tarl_graphdist_rollout_at ->
// Direction -> rows -> insert (SELECTED_ROAD set by the sampler, count bytes written by the frame kernels), in one foreign call.
//
// The *_dest entry points read the same distances from the per-destination table of tarl_prior_dest_table instead:
// table [N][D] fp32 (candidate-major like dist, one column per destination) and dest_slot int32 [N] (the column of each
// destination, -1 = none). A destination outside [0, N) or without a column is unreachable (the sentinel). The kernels are
// the same templates; only the table lookup differs (PriorAllPairs / PriorPerDest).
#include <math.h>

#include "prior_tables.h"     // PRIOR_UNREACHABLE, PriorAllPairs / PriorPerDest, prior_time_travel (shared with goal_mlp.hip)
#include "rollout_heads.h"

#define PR_BLOCK 256
#define PR_TE 64      // environments per fused tile (one per lane)
#define PR_TK 64      // CSR positions per fused tile

__device__ __forceinline__ float prior_logit(float em, float d, float ff, float maxn, float maxflow, float na, float w) {
  if (!(d <= 3.4028234663852886e38f)) return em + PRIOR_UNREACHABLE;     // +inf (unreachable) or NaN
  const float tt = prior_time_travel(ff, maxn, maxflow, na);             // :182-184
  return em + w * ((-d) - tt);                                           // logits + logits_dijkstra (:113, :188)
}

__device__ __forceinline__ float emb_of(const float* __restrict__ emb, int64_t M, float road) {
  const long long idx = (long long)road;
  return (idx >= 0 && idx < M) ? emb[idx] : 0.0f;        // tarl_policy_edge_logits_fwd's rule
}

// ---- from observations ---------------------------------------------------------------------------------------------------
template <class Tab>
__global__ __launch_bounds__(PR_BLOCK) void k_prior_obs(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                        const float* __restrict__ obs, int64_t M, int64_t N, int64_t E,
                                                        const float* __restrict__ emb, int64_t num_emb, Tab tab, float w,
                                                        float* __restrict__ logits) {
  const int64_t gid = (int64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (gid >= M * E) return;
  const int64_t m = gid / E, e = gid - m * E;
  const float* ou = obs + (m * N + src[e]) * 16;
  const int64_t v = dst[e];
  const float4* ov = reinterpret_cast<const float4*>(obs + (m * N + v) * 16);
  const float4 a = ov[0], c = ov[1];     // {MAXN, NUMBER_OF_AGENT, FF, LENGTH}, {MAX_FLOW, SELECTED_ROAD, ROAD_INDEX, ORIGIN}
  logits[gid] = prior_logit(emb_of(emb, num_emb, c.z), tab(v, ou[8]), a.z, a.x, c.x, a.y, w);
}

template <class Tab>
static int prior_obs(const tarl_plan* plan, const float* obs16, int64_t M, const float* emb, int64_t num_embeddings, Tab tab,
                     float prior_weight, float* logits, tarl_stream stream) {
  TARL_REQUIRE(plan && obs16 && emb && logits, "null argument");
  TARL_REQUIRE(M >= 1 && num_embeddings >= 1, "bad sizes");
  TARL_REQUIRE(prior_weight >= 0.0f && prior_weight <= 3.0e38f, "prior_weight must be finite and >= 0");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0, "obs16 must be 16-byte aligned");
  if (plan->E == 0) return TARL_OK;
  hipLaunchKernelGGL(k_prior_obs<Tab>, dim3((unsigned)ceil_div(M * plan->E, PR_BLOCK)), dim3(PR_BLOCK), 0,
                     (hipStream_t)stream, plan->src, plan->dst, obs16, M, plan->N, plan->E, emb, num_embeddings, tab,
                     prior_weight, logits);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

static int check_all_pairs(const tarl_plan* plan, const float* dist, int64_t dist_n) {
  TARL_REQUIRE(plan && dist, "null argument");
  TARL_REQUIRE(dist_n == plan->N, "distance table is not N x N for this plan");
  return TARL_OK;
}

static int check_per_dest(const tarl_plan* plan, const float* table, int64_t num_dests, const int32_t* dest_slot) {
  TARL_REQUIRE(plan && table && dest_slot, "null argument");
  TARL_REQUIRE(num_dests >= 1, "the per-destination table needs at least one column");
  return TARL_OK;
}

extern "C" int tarl_policy_prior_logits(const tarl_plan* plan, const float* obs16, int64_t M, const float* emb,
                                        int64_t num_embeddings, const float* dist, int64_t dist_n, float prior_weight,
                                        float* logits, tarl_stream stream) {
  int rc = check_all_pairs(plan, dist, dist_n);
  if (rc) return rc;
  return prior_obs(plan, obs16, M, emb, num_embeddings, PriorAllPairs{dist, plan->N}, prior_weight, logits, stream);
}

extern "C" int tarl_policy_prior_logits_dest(const tarl_plan* plan, const float* obs16, int64_t M, const float* emb,
                                             int64_t num_embeddings, const float* table, int64_t num_dests,
                                             const int32_t* dest_slot, float prior_weight, float* logits,
                                             tarl_stream stream) {
  int rc = check_per_dest(plan, table, num_dests, dest_slot);
  if (rc) return rc;
  return prior_obs(plan, obs16, M, emb, num_embeddings, PriorPerDest{table, dest_slot, plan->N, num_dests}, prior_weight,
                   logits, stream);
}

// ---- from the packed state -------------------------------------------------------------------------------------------------
template <class Tab>
__global__ __launch_bounds__(PR_BLOCK) void k_prior_fused(const int32_t* __restrict__ src, const int32_t* __restrict__ out_dst,
                                                          const int32_t* __restrict__ out_eid, int64_t B, int64_t N,
                                                          int64_t E, const uint2* __restrict__ hdp,
                                                          const float4* __restrict__ st0, const float* __restrict__ x0,
                                                          int64_t ldx, int col_maxflow, const float* __restrict__ ag,
                                                          int64_t A, int64_t a_bstride, const float* __restrict__ emb,
                                                          int64_t num_emb, Tab tab, float w, float* __restrict__ logits) {
  __shared__ float tile[PR_TE][PR_TK + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * PR_TE, k0 = (int64_t)blockIdx.y * PR_TK;
  const int64_t b = b0 + lane;
  for (int kk = wv; kk < PR_TK; kk += PR_BLOCK / 64) {     // one CSR position per wave step: u, v wave-uniform
    const int64_t k = k0 + kk;
    if (k >= E) break;
    const int64_t e = out_eid[k], u = src[e], v = out_dst[k];
    float l = 0.0f;
    if (b < B) {
      const uint32_t hu = hdp[u * B + b].x, hv = hdp[v * B + b].x;
      const long long head = (long long)(hu >> 8);
      const float dest = ag[b * a_bstride + ((head >= 0 && head < A) ? head : 0) * AG_COLS + AG_DEST];
      const float4 st = st0[v];    // {MAXN, FF, ROAD_INDEX, congestion_constant}
      l = prior_logit(emb_of(emb, num_emb, st.z), tab(v, dest), st.y, st.x, x0[v * ldx + col_maxflow],
                      (float)(hv & HD_CNT), w);
    }
    tile[lane][kk] = l;
  }
  __syncthreads();
  const int64_t k = k0 + lane;
  if (k >= E) return;
  const int64_t e = out_eid[k];
  for (int r = wv; r < PR_TE; r += PR_BLOCK / 64) {
    const int64_t bb = b0 + r;
    if (bb < B) logits[bb * E + e] = tile[r][lane];
  }
}

static int check_prior_state(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, const float* x,
                             const float* agent_features, int64_t A, const float* emb, int64_t num_embeddings,
                             float prior_weight) {
  TARL_REQUIRE(plan && f && x && agent_features && emb, "null argument");
  TARL_REQUIRE(B >= 1 && A >= 1 && num_embeddings >= 1, "bad sizes");
  TARL_REQUIRE(prior_weight >= 0.0f && prior_weight <= 3.0e38f, "prior_weight must be finite and >= 0");
  TARL_REQUIRE(ceil_div(plan->E, PR_TK) < 65536 && ceil_div(B, PR_TE) < 65536, "too many tiles for one grid dimension");
  return tarl_check_fused_core(plan, f, B, Nmax);
}

template <class Tab>
static int launch_prior_fused(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, const float* x,
                              int64_t ldx, const float* agent_features, int64_t A, int64_t a_bstride, const float* emb,
                              int64_t num_embeddings, Tab tab, float prior_weight, float* logits, hipStream_t s) {
  const FusedBufs fb = tarl_to_bufs(f);
  const Layout L{Nmax, ldx, 0};
  hipLaunchKernelGGL(k_prior_fused<Tab>, dim3((unsigned)ceil_div(B, PR_TE), (unsigned)ceil_div(plan->E, PR_TK)),
                     dim3(PR_BLOCK), 0, s, plan->src, plan->out_dst, plan->out_eid, B, plan->N, plan->E, fb.hdp, fb.st0, x,
                     ldx, L.col_maxflow(), agent_features, A, a_bstride, emb, num_embeddings, tab, prior_weight, logits);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

template <class Tab>
static int fused_prior(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t ldx, int32_t Nmax,
                       const float* agent_features, int64_t num_agents, int64_t a_bstride, const float* emb,
                       int64_t num_embeddings, Tab tab, float prior_weight, float* logits, tarl_stream stream) {
  TARL_REQUIRE(logits, "null argument");
  int rc = check_prior_state(plan, f, B, Nmax, x, agent_features, num_agents, emb, num_embeddings, prior_weight);
  if (rc) return rc;
  if (plan->E == 0) return TARL_OK;
  return launch_prior_fused(plan, f, B, Nmax, x, ldx, agent_features, num_agents, a_bstride, emb, num_embeddings, tab,
                            prior_weight, logits, (hipStream_t)stream);
}

extern "C" int tarl_fused_prior_logits(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B,
                                       int64_t x_bstride, int64_t ldx, int32_t Nmax, const float* agent_features,
                                       int64_t num_agents, int64_t a_bstride, const float* emb, int64_t num_embeddings,
                                       const float* dist, int64_t dist_n, float prior_weight, float* logits,
                                       tarl_stream stream) {
  (void)x_bstride;    // the static columns of environment 0 speak for all
  int rc = check_all_pairs(plan, dist, dist_n);
  if (rc) return rc;
  return fused_prior(plan, f, x, B, ldx, Nmax, agent_features, num_agents, a_bstride, emb, num_embeddings,
                     PriorAllPairs{dist, plan->N}, prior_weight, logits, stream);
}

extern "C" int tarl_fused_prior_logits_dest(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B,
                                            int64_t x_bstride, int64_t ldx, int32_t Nmax, const float* agent_features,
                                            int64_t num_agents, int64_t a_bstride, const float* emb,
                                            int64_t num_embeddings, const float* table, int64_t num_dests,
                                            const int32_t* dest_slot, float prior_weight, float* logits,
                                            tarl_stream stream) {
  (void)x_bstride;
  int rc = check_per_dest(plan, table, num_dests, dest_slot);
  if (rc) return rc;
  return fused_prior(plan, f, x, B, ldx, Nmax, agent_features, num_agents, a_bstride, emb, num_embeddings,
                     PriorPerDest{table, dest_slot, plan->N, num_dests}, prior_weight, logits, stream);
}

// ---- the rollout head (rollout_heads.h): kept observation rows and the prior logits of one frame ----------------------------
template <class Tab>
struct PriorHead {
  const float* emb;
  int64_t num_embeddings;
  Tab tab;
  float prior_weight;
};

template <class Tab>
static int prior_frame(const HeadRollout& a, void* ctx, int64_t, const int32_t* env, const int32_t* slot, int64_t n) {
  const PriorHead<Tab>& h = *(const PriorHead<Tab>*)ctx;
  const int rc = tarl_head_keep_rows(a, env, slot, n);
  if (rc || a.plan->E == 0) return rc;
  return launch_prior_fused(a.plan, a.f, a.B, a.Nmax, a.x, a.ldx, a.agent_features, a.A, a.a_bstride, h.emb, h.num_embeddings,
                            h.tab, h.prior_weight, a.logits_scratch, (hipStream_t)a.stream);
}

template <class Tab>
static int rollout_prior(const HeadRollout& a, const float* emb, int64_t num_embeddings, Tab tab, float prior_weight) {
  int rc = check_prior_state(a.plan, a.f, a.B, a.Nmax, a.x, a.agent_features, a.A, emb, num_embeddings, prior_weight);
  if (rc) return rc;
  TARL_REQUIRE(a.temperature > 0.0f, "temperature must be positive");
  PriorHead<Tab> h{emb, num_embeddings, tab, prior_weight};
  return tarl_rollout_head(a, prior_frame<Tab>, &h);
}

extern "C" int tarl_fused_rollout_prior(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                        const float* times_host, float prev_time, const float* x, int64_t x_bstride,
                                        int64_t ldx, float* agent_features, int64_t A, int64_t a_bstride,
                                        const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong,
                                        const float* emb, int64_t num_embeddings, const float* dist, int64_t dist_n,
                                        float prior_weight, float temperature, uint64_t policy_seed,
                                        uint64_t policy_counter0, uint64_t seed, uint64_t counter0,
                                        const int64_t* keep_ptr_host, const int32_t* keep_env, const int32_t* keep_slot,
                                        float* obs_keep, float* logits_scratch, void* dist_scratch, int32_t* ins_scratch,
                                        uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                                        tarl_stream stream) {
  int rc = check_all_pairs(plan, dist, dist_n);
  if (rc) return rc;
  return rollout_prior(HeadRollout{plan, f, B, Nmax, T, times_host, prev_time, x, x_bstride, ldx, agent_features, A, a_bstride,
                                   edge_attr, log_edge_attr, log_eps, use_cong, temperature, policy_seed, policy_counter0, seed,
                                   counter0, keep_ptr_host, keep_env, keep_slot, obs_keep, logits_scratch, dist_scratch,
                                   ins_scratch, choice8, log_prob, reward, counts, 0, nullptr, nullptr, nullptr, stream},
                       emb, num_embeddings, PriorAllPairs{dist, plan->N}, prior_weight);
}

extern "C" int tarl_fused_rollout_prior_dest(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                             const float* times_host, float prev_time, const float* x, int64_t x_bstride,
                                             int64_t ldx, float* agent_features, int64_t A, int64_t a_bstride,
                                             const float* edge_attr, const float* log_edge_attr, float log_eps,
                                             int use_cong, const float* emb, int64_t num_embeddings, const float* table,
                                             int64_t num_dests, const int32_t* dest_slot, float prior_weight,
                                             float temperature, uint64_t policy_seed, uint64_t policy_counter0,
                                             uint64_t seed, uint64_t counter0, const int64_t* keep_ptr_host,
                                             const int32_t* keep_env, const int32_t* keep_slot, float* obs_keep,
                                             float* logits_scratch, void* dist_scratch, int32_t* ins_scratch,
                                             uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                                             tarl_stream stream) {
  int rc = check_per_dest(plan, table, num_dests, dest_slot);
  if (rc) return rc;
  return rollout_prior(HeadRollout{plan, f, B, Nmax, T, times_host, prev_time, x, x_bstride, ldx, agent_features, A, a_bstride,
                                   edge_attr, log_edge_attr, log_eps, use_cong, temperature, policy_seed, policy_counter0, seed,
                                   counter0, keep_ptr_host, keep_env, keep_slot, obs_keep, logits_scratch, dist_scratch,
                                   ins_scratch, choice8, log_prob, reward, counts, 0, nullptr, nullptr, nullptr, stream},
                       emb, num_embeddings, PriorPerDest{table, dest_slot, plan->N, num_dests}, prior_weight);
}
