// decision_credit.hip — per-decision PPO credit: the factored update in which every road's categorical is
// credited with the delay of the traveller it decided for. Not in the reference; off unless asked for.
//
//   k_fused_head_rows        the head agent id of every road of the kept (environment, slot) pairs, read from the packed
//                            state's hdp words alone (0 on an empty road): who each decision of the frame was taken for.
//   k_decision_advantage     per (kept row, road): the head's frames still owed from the row's frame until it was withdrawn
//                            (or until the segment ends) against its free-flow frames to go, both through S(n) in fp64.
//   k_decision_stats_*       {sum, sum of squares, count} of the raw advantage over the live decisions, tarl_advantage_stats'
//                            two-stage fp64 scheme with a mask.
//   k_fused_head_rows_due    the same word where the head is also DUE at the frame's clock (credit scope "due"):
//                            the draw of a road whose head is still travelling reaches nobody.
//   k_fused_agent_roads      the road every agent is queued on (-1: nowhere), from the packed FIFOs alone: where the horizon
//                            bootstrap of k_decision_advantage continues from.
//   k_graphdist_node_logprob log(p_choice + 1e-8) per node, k_softmax's expressions.
//   k_graphdist_decision_ppo the clipped objective per live node, forward and backward, plus k_decision_ppo_reduce per sample.
//
// All per-node kernels have tile_sums.h's launch shape (one lane per node, the (row, tile) pairs flattened into grid.x); on
// a source-sorted edge list (CSR position == edge id) the edge-id indirection is skipped. No floating-point atomics: the
// sums are tile_sums.h's fixed trees.
#include <mutex>
#include <unordered_map>

#include "rollout_heads.h"
#include "tile_sums.h"

#define DC_STAT_BLOCKS 256
#define DC_STD_FLOOR 1e-6f                 // = TARL_ADV_STD_FLOOR (ppo.hip): the rule of tarl_advantage_normalize

// ---- (1) the heads of the kept rows ---------------------------------------------------------------------------------------
// Must move per (pair, road): the 4-byte hd word of hdp[u][env] (a stride of 8 B bytes between the lanes of a wave: the packed
// state is env-minor and a kept pair is one environment, as for tarl_fused_obs16_rows) and one coalesced 4-byte store.
__global__ __launch_bounds__(TS_TILE) void k_fused_head_rows(const uint32_t* __restrict__ hdp_words, int64_t N, uint32_t B,
                                                             uint32_t tiles, const int32_t* __restrict__ env,
                                                             const int32_t* __restrict__ slot,
                                                             int32_t* __restrict__ head_keep) {
  const auto [j, u] = ts_at(tiles);
  if (u >= N) return;
  const int32_t b = env[j];
  int32_t v = 0;
  if (b >= 0 && (uint32_t)b < B) {
    const uint32_t hd = hdp_words[2 * (u * B + b)];                 // hdp[u][b].x; N * B < 2^31 (checked by the caller)
    if ((hd & HD_CNT) != 0u) v = (int32_t)(hd >> 8);
  }
  head_keep[(int64_t)slot[j] * N + u] = v;
}

int tarl_launch_head_rows(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* env,
                          const int32_t* slot, int64_t n, int32_t* head_keep) {
  const int64_t tiles = ts_tiles(plan);
  hipLaunchKernelGGL(k_fused_head_rows, dim3((unsigned)(n * tiles)), dim3(TS_TILE), 0, s, (const uint32_t*)f->hdp, plan->N,
                     (uint32_t)B, (uint32_t)tiles, env, slot, head_keep);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

int tarl_check_head_rows(const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t n) {
  TARL_REQUIRE(plan && f && f->hdp, "null argument");
  TARL_REQUIRE(B >= 1 && plan->N * B < ((int64_t)1 << 31), "bad sizes (N * B must stay below 2^31)");
  TARL_REQUIRE(n >= 0, "bad sizes");
  TS_REQUIRE_PAIRS(n, ts_tiles(plan));
  return TARL_OK;
}

extern "C" int tarl_fused_head_rows(const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* env,
                                    const int32_t* slot, int64_t n, int32_t* head_keep, tarl_stream stream) {
  const int rc = tarl_check_head_rows(plan, f, B, n);
  if (rc != TARL_OK) return rc;
  if (n == 0 || plan->N == 0) return TARL_OK;
  TARL_REQUIRE(env && slot && head_keep, "null argument");
  return tarl_launch_head_rows((hipStream_t)stream, plan, f, B, env, slot, n, head_keep);
}

// ---- (1b) credit scope "due"  ------------------------------------------------------------------------------------
// k_fused_head_rows reading the whole 8-byte hdp word (the same lines: hd and dep are adjacent): the head id where the road
// holds somebody AND its head's departure has come at the clock the frame is stepped with (Direction's fp32 test,
// fused_direction.hip), 0 elsewhere. The count test comes first: an empty road's dep word may be stale (lazy rows,
// fused_common.h). counts2 (optional) += {headed, due}, one integer atomic each per wave.
__global__ __launch_bounds__(TS_TILE) void k_fused_head_rows_due(const uint2* __restrict__ hdp, int64_t N, uint32_t B,
                                                                 uint32_t tiles, float t_clock,
                                                                 const int32_t* __restrict__ env,
                                                                 const int32_t* __restrict__ slot,
                                                                 int32_t* __restrict__ head_keep,
                                                                 int32_t* __restrict__ counts2) {
  const auto [j, u] = ts_at(tiles);
  bool headed = false, due = false;
  if (u < N) {
    const int32_t b = env[j];
    int32_t v = 0;
    if (b >= 0 && (uint32_t)b < B) {
      const uint2 w = hdp[u * B + b];                                 // N * B < 2^31 (checked by the caller)
      headed = (w.x & HD_CNT) != 0u;
      due = headed && __uint_as_float(w.y) <= t_clock;
      if (due) v = (int32_t)(w.x >> 8);
    }
    head_keep[(int64_t)slot[j] * N + u] = v;
  }
  if (counts2) {
    const int32_t c_headed = (int32_t)__popcll(__ballot(headed)), c_due = (int32_t)__popcll(__ballot(due));
    if ((threadIdx.x & 63) == 0) {              // integer atomics: the result does not depend on scheduling
      if (c_headed) atomicAdd(counts2, c_headed);
      if (c_due) atomicAdd(counts2 + 1, c_due);
    }
  }
}

int tarl_launch_head_rows_due(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, float t_clock,
                              const int32_t* env, const int32_t* slot, int64_t n, int32_t* head_keep, int32_t* counts2) {
  const int64_t tiles = ts_tiles(plan);
  hipLaunchKernelGGL(k_fused_head_rows_due, dim3((unsigned)(n * tiles)), dim3(TS_TILE), 0, s, (const uint2*)f->hdp, plan->N,
                     (uint32_t)B, (uint32_t)tiles, t_clock, env, slot, head_keep, counts2);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_fused_head_rows_due(const tarl_plan* plan, const tarl_fused* f, int64_t B, float t_clock,
                                        const int32_t* env, const int32_t* slot, int64_t n, int32_t* head_keep,
                                        int32_t* counts2, tarl_stream stream) {
  const int rc = tarl_check_head_rows(plan, f, B, n);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(std::isfinite(t_clock), "t_clock must be finite");
  if (n == 0 || plan->N == 0) return TARL_OK;
  TARL_REQUIRE(env && slot && head_keep, "null argument");
  return tarl_launch_head_rows_due((hipStream_t)stream, plan, f, B, t_clock, env, slot, n, head_keep, counts2);
}

// ---- the switch of the one-call rollouts -------------------------------------------------------------------------------------
// tarl_fused does not grow: the capture buffer lives beside the handle, keyed by its address, and bit TARL_HEAD_CAPTURE of
// tarl_fused.policy_hold says that the loop queues the launch above (departures.hip has the scheme).
struct HeadCapture {
  int32_t* head_keep;
  int scope;            // 0 = headed (k_fused_head_rows), 1 = due (k_fused_head_rows_due): tarl_fused_set_head_capture_scope
  int32_t* counts2;     // scope 1: {headed, due} of the captured rows, or NULL
};
static std::mutex g_capture_mutex;
static std::unordered_map<const tarl_fused*, HeadCapture> g_capture;

int32_t* tarl_head_capture_of(const tarl_fused* f) {
  std::lock_guard<std::mutex> lock(g_capture_mutex);
  const auto it = g_capture.find(f);
  return it == g_capture.end() ? nullptr : it->second.head_keep;
}

int tarl_head_capture_scope_of(const tarl_fused* f, int32_t** counts2) {
  std::lock_guard<std::mutex> lock(g_capture_mutex);
  const auto it = g_capture.find(f);
  *counts2 = it == g_capture.end() ? nullptr : it->second.counts2;
  return it == g_capture.end() ? 0 : it->second.scope;
}

extern "C" int tarl_fused_set_head_capture(tarl_fused* f, int on, int32_t* head_keep) {
  TARL_REQUIRE(f, "null argument");
  TARL_REQUIRE(on == 0 || on == 1, "on must be 0 or 1");
  TARL_REQUIRE(on ? head_keep != nullptr : head_keep == nullptr, "the switch and its buffer go together");
  std::lock_guard<std::mutex> lock(g_capture_mutex);
  if (on) g_capture[f] = HeadCapture{head_keep, 0, nullptr};      // (switching on starts from scope "headed")
  else g_capture.erase(f);
  f->policy_hold = on ? (f->policy_hold | TARL_HEAD_CAPTURE) : (f->policy_hold & ~TARL_HEAD_CAPTURE);
  return TARL_OK;
}

extern "C" int tarl_fused_set_head_capture_scope(tarl_fused* f, int scope, int32_t* counts2) {
  TARL_REQUIRE(f, "null argument");
  TARL_REQUIRE(scope == 0 || scope == 1, "scope must be 0 (headed) or 1 (due)");
  TARL_REQUIRE(scope == 1 || counts2 == nullptr, "counts2 belongs to scope 1 (due)");
  std::lock_guard<std::mutex> lock(g_capture_mutex);
  const auto it = g_capture.find(f);
  TARL_REQUIRE(it != g_capture.end() && (f->policy_hold & TARL_HEAD_CAPTURE) != 0,
               "the head capture is off for this handle (tarl_fused_set_head_capture)");
  it->second.scope = scope;
  it->second.counts2 = counts2;
  return TARL_OK;
}

// ---- where every agent stands ----------------------------------------------------------------------------------
// Lanes over (u, b) with b minor: the dense words hdp / tl coalesce; each lane walks logical slots 0 .. count - 1 of its own
// FIFO (the slot AT the count holds the pending garbage triple and is never read). Must move per (road, environment): 8 + 4
// bytes of dense words, and per queued agent one 4-byte id read and one 4-byte integer atomicMax (an agent is queued on one
// road, so the max has one candidate and the result does not depend on scheduling). Writes nothing of the packed state.
__global__ __launch_bounds__(TS_TILE) void k_fused_agent_roads(const uint2* __restrict__ hdp, const uint32_t* __restrict__ tl,
                                                               const float* __restrict__ slots, int64_t lds, int64_t NB,
                                                               uint32_t B, int32_t Nmax, int64_t A,
                                                               int32_t* __restrict__ agent_road, int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * TS_TILE + threadIdx.x;      // = u * B + b
  if (i >= NB) return;
  int32_t cnt = (int32_t)(hdp[i].x & HD_CNT);
  if (cnt == 0) return;
  const int hoff = tl_hoff(tl[i]);
  int32_t n_bad = 0;
  if (hoff >= Nmax) {                           // no ring of this store starts there: nothing is read
    n_bad = cnt;
    cnt = 0;
  } else if (cnt > Nmax) {
    n_bad = cnt - Nmax;
    cnt = Nmax;
  }
  const int32_t u = (int32_t)(i / B);
  const int64_t b = i - (int64_t)u * B;
  const float* row = slots + i * lds;
  for (int32_t k = 0; k < cnt; ++k) {
    const float idf = row[SLW * phys(hoff, k, Nmax)];
    if (idf >= 1.0f && idf < (float)A) atomicMax(agent_road + b * A + (int64_t)idf, u);
    else ++n_bad;
  }
  if (n_bad) atomicAdd(bad, n_bad);             // (off the defined domain only)
}

extern "C" int tarl_fused_agent_roads(const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, int32_t Nmax,
                                      int32_t* agent_road, int32_t* bad, tarl_stream stream) {
  TARL_REQUIRE(plan && f && agent_road && bad, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc) return rc;
  TARL_REQUIRE(A >= 1 && A <= ((int64_t)1 << 24) && B * A < ((int64_t)1 << 31), "bad agent table size");
  TARL_REQUIRE(plan->N * B < ((int64_t)1 << 31), "bad sizes (N * B must stay below 2^31)");
  hipStream_t s = (hipStream_t)stream;
  TARL_CHECK_HIP(hipMemsetAsync(agent_road, 0xFF, (size_t)(B * A) * sizeof(int32_t), s));      // -1: queued nowhere
  if (plan->N == 0) return TARL_OK;
  const FusedBufs fb = tarl_to_bufs(f);
  const int64_t NB = plan->N * B;
  hipLaunchKernelGGL(k_fused_agent_roads, dim3((unsigned)ceil_div(NB, TS_TILE)), dim3(TS_TILE), 0, s, (const uint2*)fb.hdp,
                     (const uint32_t*)fb.tl, (const float*)fb.slots, fb.lds, NB, (uint32_t)B, Nmax, A, agent_road, bad);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- (2) the raw advantage of every decision of a segment's kept rows ------------------------------------------------------
// S(n) = n for gamma == 1, (1 - gamma^n) / (1 - gamma) otherwise; fp64.
__device__ __forceinline__ double dc_owed(double n, double gamma) {
  return gamma == 1.0 ? n : (1.0 - pow(gamma, n)) / (1.0 - gamma);
}

// Must move per (row, road): 4 B of head_keep read (and 4 B written back where the decision is not live), 4 B of adv_raw
// written; on a headed road four scattered gathers (destination, DONE, ARRIVAL_TIME, dist) and a binary search of the
// segment's clocks (at most log2 T 4-byte loads of one short array every lane shares).
// BOOT (horizon "bootstrap"): a traveller still under way when the segment ends continues, in free flow, from the
// road r it is queued on (agent_road): n = (t_end - t) + dist[s][r] / timestep, counted in `bootstrapped`; one queued nowhere
// (lost) or with no finite dist[s][r] keeps the charge and counts in `truncated`. Two more scattered gathers on such a lane.
template <bool BOOT>
__global__ __launch_bounds__(TS_TILE) void k_decision_advantage(
    const int32_t* __restrict__ out_ptr, int64_t N, uint32_t tiles, int32_t* __restrict__ head_keep,
    const int32_t* __restrict__ frame, const int32_t* __restrict__ env, const int32_t* __restrict__ slot, int64_t B,
    const float* __restrict__ ag, int64_t A, int64_t a_bstride, const float* __restrict__ times, int32_t t_end,
    const double* __restrict__ dist, const int32_t* __restrict__ dest_slot, int64_t D, double timestep, double gamma,
    float* __restrict__ adv_raw, int32_t* __restrict__ truncated, int32_t* __restrict__ bad,
    const int32_t* __restrict__ agent_road, int32_t* __restrict__ bootstrapped) {
  const auto [j, u] = ts_at(tiles);
  bool is_bad = false, is_trunc = false, is_boot = false;
  if (u < N) {
    const int64_t at = (int64_t)slot[j] * N + u;
    const int32_t a = head_keep[at], t = frame[j], b = env[j];
    bool live = false;
    double adv = 0.0;
    if (a > 0 && t >= 0 && t < t_end && b >= 0 && b < B) {
      is_bad = a >= A;
      if (!is_bad && out_ptr[u + 1] > out_ptr[u]) {
        const float* row = ag + (int64_t)b * a_bstride + (int64_t)a * AG_COLS;
        const float df = row[AG_DEST];
        if (df >= 0.0f && df < (float)N) {
          const int64_t d = (int64_t)df;
          const int32_t s = d < N ? dest_slot[d] : -1;
          if (s >= 0 && s < D) {
            const double du = dist[(int64_t)s * N + u];
            if (isfinite(du)) {
              int32_t n = t_end - t;
              double n_go = 0.0;                // BOOT: the free-flow frames still to go beyond the horizon
              if (row[AG_DONE] == 1.0f) {       // frames k in [t, t_end) with times[k] < ARRIVAL_TIME: a lower bound search
                const float arr = row[AG_ARR];
                int32_t lo = t, hi = t_end;
                while (lo < hi) {
                  const int32_t mid = lo + ((hi - lo) >> 1);
                  if (times[mid] < arr) lo = mid + 1;
                  else hi = mid;
                }
                n = lo - t;
              } else {
                if (BOOT) {
                  const int32_t r = agent_road[(int64_t)b * A + a];
                  if (r >= 0 && r < N) {
                    const double dr = dist[(int64_t)s * N + r];
                    if (isfinite(dr)) {
                      n_go = dr / timestep;
                      is_boot = true;
                    }
                  }
                }
                is_trunc = !is_boot;
              }
              adv = dc_owed(du / timestep, gamma) -                                // G - G_ff = -S(n) + S(n_ff)
                    dc_owed(BOOT && is_boot ? (double)n + n_go : (double)n, gamma);
              live = true;
            }
          }
        }
      }
    }
    adv_raw[at] = live ? (float)adv : 0.0f;
    if (!live && a != 0) head_keep[at] = 0;
  }
  const int32_t c_bad = (int32_t)__popcll(__ballot(is_bad)), c_trunc = (int32_t)__popcll(__ballot(is_trunc));
  if ((threadIdx.x & 63) == 0) {              // integer atomics: the result does not depend on scheduling
    if (c_bad) atomicAdd(bad, c_bad);
    if (c_trunc) atomicAdd(truncated, c_trunc);
  }
  if (BOOT) {
    const int32_t c_boot = (int32_t)__popcll(__ballot(is_boot));
    if ((threadIdx.x & 63) == 0 && c_boot) atomicAdd(bootstrapped, c_boot);
  }
}

static int decision_advantage_impl(const tarl_plan* plan, int32_t* head_keep, const int32_t* frame, const int32_t* env,
                                   const int32_t* slot, int64_t rows, int64_t B, const float* agent_features,
                                   int64_t num_agents, int64_t a_bstride, const float* times, int64_t num_times,
                                   int64_t t_end, const double* dist, const int32_t* dest_slot, int64_t num_dests,
                                   float timestep, double decision_gamma, float* adv_raw, int32_t* truncated, int32_t* bad,
                                   const int32_t* agent_road, int bootstrap, int32_t* bootstrapped, tarl_stream stream) {
  TARL_REQUIRE(bootstrap == 0 || bootstrap == 1, "bootstrap must be 0 or 1");
  TARL_REQUIRE(!bootstrap || (agent_road && bootstrapped), "bootstrap needs agent_road and bootstrapped");
  TARL_REQUIRE(plan && head_keep && frame && env && slot && agent_features && times && dist && dest_slot && adv_raw &&
                   truncated && bad, "null argument");
  TARL_REQUIRE(rows >= 0 && B >= 1 && num_agents >= 1 && num_agents <= ((int64_t)1 << 24) && num_dests >= 1, "bad sizes");
  TARL_REQUIRE(B == 1 || a_bstride >= num_agents * AG_COLS, "a_bstride smaller than one agent table");
  TARL_REQUIRE(t_end >= 1 && t_end <= num_times && num_times < ((int64_t)1 << 31), "t_end outside the clocks");
  TARL_REQUIRE(timestep > 0.0f && std::isfinite(timestep), "timestep must be positive and finite");
  TARL_REQUIRE(decision_gamma > 0.0 && decision_gamma <= 1.0, "decision_gamma must be in (0, 1]");
  const int64_t tiles = ts_tiles(plan);
  TS_REQUIRE_PAIRS(rows, tiles);
  if (rows == 0 || plan->N == 0) return TARL_OK;
#define DC_LAUNCH(BOOT_)                                                                                                   \
  hipLaunchKernelGGL(k_decision_advantage<BOOT_>, dim3((unsigned)(rows * tiles)), dim3(TS_TILE), 0, (hipStream_t)stream,   \
                     plan->out_ptr, plan->N, (uint32_t)tiles, head_keep, frame, env, slot, B, agent_features, num_agents,  \
                     a_bstride, times, (int32_t)t_end, dist, dest_slot, num_dests, (double)timestep, decision_gamma,       \
                     adv_raw, truncated, bad, agent_road, bootstrapped)
  if (bootstrap)
    DC_LAUNCH(true);
  else
    DC_LAUNCH(false);
#undef DC_LAUNCH
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_decision_advantage(const tarl_plan* plan, int32_t* head_keep, const int32_t* frame, const int32_t* env,
                                       const int32_t* slot, int64_t rows, int64_t B, const float* agent_features,
                                       int64_t num_agents, int64_t a_bstride, const float* times, int64_t num_times,
                                       int64_t t_end, const double* dist, const int32_t* dest_slot, int64_t num_dests,
                                       float timestep, double decision_gamma, float* adv_raw, int32_t* truncated,
                                       int32_t* bad, tarl_stream stream) {
  return decision_advantage_impl(plan, head_keep, frame, env, slot, rows, B, agent_features, num_agents, a_bstride, times,
                                 num_times, t_end, dist, dest_slot, num_dests, timestep, decision_gamma, adv_raw, truncated,
                                 bad, nullptr, 0, nullptr, stream);
}

extern "C" int tarl_decision_advantage_boot(const tarl_plan* plan, int32_t* head_keep, const int32_t* frame,
                                            const int32_t* env, const int32_t* slot, int64_t rows, int64_t B,
                                            const float* agent_features, int64_t num_agents, int64_t a_bstride,
                                            const float* times, int64_t num_times, int64_t t_end, const double* dist,
                                            const int32_t* dest_slot, int64_t num_dests, float timestep,
                                            double decision_gamma, float* adv_raw, int32_t* truncated, int32_t* bad,
                                            const int32_t* agent_road, int bootstrap, int32_t* bootstrapped,
                                            tarl_stream stream) {
  return decision_advantage_impl(plan, head_keep, frame, env, slot, rows, B, agent_features, num_agents, a_bstride, times,
                                 num_times, t_end, dist, dest_slot, num_dests, timestep, decision_gamma, adv_raw, truncated,
                                 bad, agent_road, bootstrap, bootstrapped, stream);
}

// ---- (3) statistics over the live decisions ----------------------------------------------------------------------------------
__global__ __launch_bounds__(TS_TILE) void k_decision_stats_partial(const float* __restrict__ a,
                                                                    const int32_t* __restrict__ head, int64_t n,
                                                                    double* __restrict__ partial) {
  __shared__ double s_red[TS_WAVES][3];
  double x[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * TS_TILE + threadIdx.x; i < n; i += (int64_t)gridDim.x * TS_TILE) {
    if (head[i] > 0) {
      const double v = (double)a[i];
      x[0] += v;
      x[1] += v * v;
      x[2] += 1.0;
    }
  }
  ts_wave_sum(x);
  ts_wave_put(s_red, x);
  __syncthreads();
  if (threadIdx.x == 0) ts_waves_in_order(s_red, partial + 3 * blockIdx.x);
}

// the workgroups' sums in order: one row of nblocks entries
__global__ void k_decision_stats_final(const double* __restrict__ partial, int nblocks, double* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ts_row_sum<3>(partial, 0, (uint32_t)nblocks, stats);
}

extern "C" int tarl_decision_stats(const float* adv_raw, const int32_t* head_keep, int64_t elems, double* partial,
                                   double* stats3, tarl_stream stream) {
  TARL_REQUIRE(adv_raw && head_keep && partial && stats3 && elems >= 1, "bad argument");
  const int nb = (int)(ceil_div(elems, TS_TILE) < DC_STAT_BLOCKS ? ceil_div(elems, TS_TILE) : DC_STAT_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_decision_stats_partial, dim3(nb), dim3(TS_TILE), 0, s, adv_raw, head_keep, elems, partial);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_decision_stats_final, dim3(1), dim3(64), 0, s, (const double*)partial, nb, stats3);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- the node's categorical, k_softmax's expressions -----------------------------------------------------------------------------
// z_j = l_j / T, mx = max z, s = sum of exp(z_j - mx) left to right in CSR order; -> the CSR position of edge `ce` in
// [k0, k1) or -1, and mx, s.
template <bool SORTED>
__device__ __forceinline__ int32_t dc_softmax_stats(const int32_t* __restrict__ out_eid, const float* __restrict__ lb,
                                                    int32_t k0, int32_t k1, float temperature, int32_t ce, float* mx_out,
                                                    float* s_out) {
  float mx = -INFINITY;
  int32_t at = -1;
  for (int32_t k = k0; k < k1; ++k) {
    const int32_t e = SORTED ? k : out_eid[k];
    if (e == ce) at = k;
    mx = fmaxf(mx, lb[e] / temperature);
  }
  float s = 0.0f;
  for (int32_t k = k0; k < k1; ++k) s = s + expf(lb[SORTED ? k : out_eid[k]] / temperature - mx);
  *mx_out = mx;
  *s_out = s;
  return at;
}

// ---- (4) log-prob per node -------------------------------------------------------------------------------------------------
template <bool SORTED>
__global__ __launch_bounds__(TS_TILE) void k_graphdist_node_logprob(const int32_t* __restrict__ out_ptr,
                                                                    const int32_t* __restrict__ out_eid,
                                                                    const float* __restrict__ logits, int64_t N, int64_t E,
                                                                    uint32_t tiles, float temperature,
                                                                    const int32_t* __restrict__ choice,
                                                                    float* __restrict__ lp_node) {
  const auto [m, n] = ts_at(tiles);
  if (n >= N) return;
  const float* lb = logits + (int64_t)m * E;
  const int32_t k0 = out_ptr[n], k1 = out_ptr[n + 1];
  const int32_t ce = choice[(int64_t)m * N + n];
  float lp = 0.0f;
  if (ce >= 0 && k1 > k0) {
    float mx, s;
    const int32_t at = dc_softmax_stats<SORTED>(out_eid, lb, k0, k1, temperature, ce, &mx, &s);
    if (at >= 0) lp = logf(expf(lb[ce] / temperature - mx) / s + LOG_EPS_P);
  }
  lp_node[(int64_t)m * N + n] = lp;
}

extern "C" int tarl_graphdist_node_logprob(const tarl_plan* plan, const float* logits, int64_t M, float temperature,
                                           const int32_t* choice, float* lp_node, tarl_stream stream) {
  TARL_REQUIRE(plan && logits && choice && lp_node, "null argument");
  TARL_REQUIRE(M >= 1, "M must be positive");
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  const int64_t tiles = ts_tiles(plan);
  TS_REQUIRE_PAIRS(M, tiles);
  if (plan->N == 0) return TARL_OK;
#define DC_LAUNCH(S_)                                                                                                      \
  hipLaunchKernelGGL(k_graphdist_node_logprob<S_>, dim3((unsigned)(M * tiles)), dim3(TS_TILE), 0, (hipStream_t)stream,     \
                     plan->out_ptr, plan->out_eid, logits, plan->N, plan->E, (uint32_t)tiles, temperature, choice, lp_node)
  if (plan->src_sorted)
    DC_LAUNCH(true);
  else
    DC_LAUNCH(false);
#undef DC_LAUNCH
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- (5) the clipped objective per live decision, forward and backward -----------------------------------------------------------
#define DC_SUMS 4      // per (sample, tile) pair and per sample: {clipped gain, live, ratios outside the clip, lp_old - lp} in fp64

// Must move per (sample, road): head, choice, lp_old, adv_raw (16 B, coalesced); on a live road its out-edges' logits read
// twice (max, sum) and once more in the backward, and their gradient entries read and written once (+=). Every edge has one
// source node, so every element of grad has one writer.
template <bool SORTED>
__global__ __launch_bounds__(TS_TILE) void k_graphdist_decision_ppo(
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_eid, const float* __restrict__ logits, int64_t N,
    int64_t E, uint32_t tiles, float temperature, const int32_t* __restrict__ choice, const int32_t* __restrict__ head,
    const float* __restrict__ lp_old, const float* __restrict__ adv_raw, const double* __restrict__ stats,
    const int32_t* __restrict__ n_live, float clip_eps, float grad_scale, float* __restrict__ grad,
    double* __restrict__ part) {
  __shared__ double s_red[TS_WAVES][DC_SUMS];
  const auto [m, n] = ts_at(tiles);
  const float* lb = logits + (int64_t)m * E;
  double v[DC_SUMS] = {0.0, 0.0, 0.0, 0.0};
  if (n < N && head[(int64_t)m * N + n] > 0) {
    const int32_t k0 = out_ptr[n], k1 = out_ptr[n + 1];
    const int32_t ce = choice[(int64_t)m * N + n];
    float mx, s;
    const int32_t at = (ce >= 0 && k1 > k0) ? dc_softmax_stats<SORTED>(out_eid, lb, k0, k1, temperature, ce, &mx, &s) : -1;
    if (at >= 0) {
      // tarl_advantage_normalize's rule on the live decisions' statistics
      const double cnt = stats[2], mean = stats[0] / cnt;
      double var = (stats[1] - cnt * mean * mean) / (cnt - 1.0);
      if (!(var >= 0.0)) var = 0.0;                               // (a single live decision: 0 / 0)
      float sd = (float)sqrt(var);
      if (sd < DC_STD_FLOOR) sd = DC_STD_FLOOR;
      const float a = (adv_raw[(int64_t)m * N + n] - (float)mean) / sd;
      const float ps = expf(lb[ce] / temperature - mx) / s;
      const float lp = logf(ps + LOG_EPS_P);
      const float lo = lp_old[(int64_t)m * N + n];
      const float r = expf(lp - lo);
      const float g1 = r * a;
      const float g2 = fminf(fmaxf(r, 1.0f - clip_eps), 1.0f + clip_eps) * a;
      const bool flows = g1 <= g2;                                // the unclipped term is the minimum; a tie flows
      v[0] = (double)(flows ? g1 : g2);
      v[1] = 1.0;
      v[2] = (r < 1.0f - clip_eps || r > 1.0f + clip_eps) ? 1.0 : 0.0;
      v[3] = (double)(lo - lp);
      const int32_t L = n_live[0];
      if (grad && flows && L > 0) {
        float* gb = grad + (int64_t)m * E;
        const float coef = -(grad_scale / (float)L) * g1 * (ps / (ps + LOG_EPS_P));
        for (int32_t k = k0; k < k1; ++k) {
          const int32_t e = SORTED ? k : out_eid[k];
          const float p = expf(lb[e] / temperature - mx) / s;
          gb[e] = gb[e] + coef * ((k == at ? 1.0f : 0.0f) - p) / temperature;
        }
      }
    }
  }
  ts_wave_sum(v);
  ts_wave_put(s_red, v);
  __syncthreads();
  if (threadIdx.x == 0) ts_waves_in_order(s_red, part + (int64_t)blockIdx.x * DC_SUMS);
}

__global__ __launch_bounds__(64) void k_decision_ppo_reduce(const double* __restrict__ part, int64_t M, uint32_t tiles,
                                                            double* __restrict__ out4) {
  const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (m < M) ts_row_sum<DC_SUMS>(part, m, tiles, out4);
}

extern "C" int64_t tarl_graphdist_decision_ppo_scratch_bytes(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 1) return -1;
  const int64_t tiles = ts_tiles(plan);
  if (!ts_pairs_fit(M, tiles)) return -1;
  return M * tiles * DC_SUMS * (int64_t)sizeof(double);
}

extern "C" int tarl_graphdist_decision_ppo(const tarl_plan* plan, const float* logits, int64_t M, float temperature,
                                           const int32_t* choice, const int32_t* head, const float* lp_old_node,
                                           const float* adv_raw, const double* stats3, const int32_t* n_live,
                                           float clip_epsilon, float grad_scale, double* out4, float* grad_logits,
                                           void* scratch, tarl_stream stream) {
  TARL_REQUIRE(plan && logits && choice && head && lp_old_node && adv_raw && stats3 && n_live && out4 && scratch,
               "null argument");
  TARL_REQUIRE(M >= 1, "M must be positive");
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  TARL_REQUIRE(clip_epsilon >= 0.0f && clip_epsilon < 1.0f, "clip_epsilon must be in [0, 1)");
  TARL_REQUIRE(((uintptr_t)scratch) % 8 == 0, "scratch must be 8-byte aligned");
  const int64_t tiles = ts_tiles(plan);
  TS_REQUIRE_PAIRS(M, tiles);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)scratch;
#define DC_LAUNCH(S_)                                                                                                       \
  hipLaunchKernelGGL(k_graphdist_decision_ppo<S_>, dim3((unsigned)(M * tiles)), dim3(TS_TILE), 0, s, plan->out_ptr,         \
                     plan->out_eid, logits, plan->N, plan->E, (uint32_t)tiles, temperature, choice, head, lp_old_node,     \
                     adv_raw, stats3, n_live, clip_epsilon, grad_scale, grad_logits, part)
  if (plan->src_sorted)
    DC_LAUNCH(true);
  else
    DC_LAUNCH(false);
#undef DC_LAUNCH
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_decision_ppo_reduce, dim3((unsigned)ceil_div(M, 64)), dim3(64), 0, s, (const double*)part, M,
                     (uint32_t)tiles, out4);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
