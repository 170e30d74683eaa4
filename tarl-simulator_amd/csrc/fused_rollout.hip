// fused_rollout.hip — the host loops of the fused path: one frame (tarl_fused_frame), T frames with the live policy
// (tarl_fused_rollout) and T frames with a state-dependent policy head (tarl_rollout_head: the one loop under
// tarl_fused_rollout_policy here, tarl_fused_rollout_prior[_dest] in prior.hip and tarl_fused_rollout_gt in gt_policy.hip),
// written against the launch functions of the kernel files. (Design: fused_frame.h.)
#include <cmath>

#include "fused_frame.h"
#include "rollout_heads.h"

// the side outputs of frame t of a T-frame rollout: slice t of every series the caller asked for; the event byte gc8 is
// stored for every row in the last frame only (FrameOut::write_gc)
static FrameOut rollout_frame_out(int64_t t, int64_t T, int64_t N, int64_t B, uint8_t* counts, int32_t metrics_envs,
                                  float* dtt_node, uint8_t* events, int32_t* leg) {
  const int64_t m = metrics_envs;
  return FrameOut{counts ? counts + t * N * B : nullptr, nullptr, nullptr, nullptr,   // no frame-API outputs in a rollout
                  events ? events + t * N * m : nullptr, dtt_node ? dtt_node + t * N * m : nullptr, metrics_envs,
                  leg ? leg + t * 2 * B : nullptr, t + 1 == T ? 1 : 0};
}

extern "C" int tarl_fused_frame(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                const float* thresholds, const int64_t* log_probs, const float* entropy1,
                                const float* uniform, uint64_t policy_seed, uint64_t policy_counter,
                                float* agent_features, int64_t A, int64_t a_bstride, const float* edge_attr,
                                const float* log_edge_attr, float log_eps, int use_cong, float time, float prev_time,
                                const float* gumbel, uint64_t seed, uint64_t counter, float* delta_travel_time,
                                uint8_t* popped, uint8_t* withdrawn, int32_t* ins_scratch, int32_t* choice,
                                float* log_prob, float* entropy, float* reward, float* counts, tarl_stream stream) {
  int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc) return rc;
  // thresholds == NULL: SELECTED_ROAD was set by the caller (tarl_fused_apply_choice); no sample / log-prob in this call
  TARL_REQUIRE((thresholds && log_probs && entropy1) || (!thresholds && !log_prob && !entropy && !choice),
               "policy tables missing (call tarl_fused_policy_prepare), or outputs of the skipped choice phase requested");
  rc = tarl_check_frame_args(plan, f, B, agent_features, A, a_bstride, ins_scratch, edge_attr, log_edge_attr);
  if (rc) return rc;
  if (plan->N == 0) return TARL_OK;
  const FusedBufs fb = tarl_to_bufs(f);
  const PlanOut P{plan->out_ptr, plan->out_dst};
  hipStream_t s = (hipStream_t)stream;
  const unsigned threads = tile_threads(B);
  const dim3 grid((unsigned)ceil_div(B, threads), (unsigned)num_chunks(plan));
  if (thresholds) {
    rc = tarl_launch_choice(s, plan, f, B, fb.acc_lp, thresholds, log_probs, uniform, policy_seed, policy_counter, f->sel8,
                            (const uint8_t*)f->sel8, choice, log_prob != nullptr ? 1 : 0);
    if (rc) return rc;
  }
  const FusedBufs* fbd = nullptr;
  rc = tarl_upload_bufs(f, fb, nullptr, s, &fbd);
  if (rc) return rc;
  const bool timed = tarl_prof_mark(s, 0) != nullptr;
  const dim3 grid_d((unsigned)ceil_div(B, threads), (unsigned)ceil_div(plan->N, nchunk_dir()));
  const FrameOut out{nullptr, counts, popped, withdrawn, nullptr, nullptr, 0, nullptr, 1};
  rc = tarl_launch_direction(grid_d, threads, s, plan, f, edge_attr, log_edge_attr, (const uint8_t*)f->sel8, gumbel,
                             delta_travel_time, log_eps, time, prev_time, seed, counter, B, (int)Nmax, out);
  if (rc) return rc;
  if (timed) (void)tarl_prof_mark(s, 1);
  rc = tarl_launch_rows(grid, threads, s, plan, f, fbd, (int)Nmax, B, agent_features, A, a_bstride, time, out);
  if (rc) return rc;
  if (timed) (void)tarl_prof_mark(s, 2);
  rc = tarl_launch_insert(1, s, (int)Nmax, B, plan->N, fbd, P, (const uint8_t*)f->sel8, agent_features, A, a_bstride,
                          use_cong, time, ins_scratch, entropy1, reward, out, log_prob, entropy);
  if (rc) return rc;
  if (timed) (void)tarl_prof_mark(s, 3);
  return TARL_OK;
}

// T consecutive frames with device noise: the collector loop in one foreign call. Each frame is direction -> rows ->
// insert on the caller's stream. The action of frame t is slice t of the action buffer, which is also the
// SELECTED_ROAD column that frame's Direction gather and insert read. With an action buffer and choice_scratch (the
// default, TARL_ROLLOUT_MERGE=2) the live policy's draws for ALL frames are made on a side stream in blocks of
// frames (the sample does not depend on the state: fused_choice.hip, tarl_choice_ahead_queue), the first, short block is
// waited for; otherwise frame t+1's choice shares the launch of frame t's insert (k_fused_insert_choice, mode 1) or is a
// launch of its own (mode 0). Per-frame draws on a side stream and folding them into the row pass were measured and
// rejected.
extern "C" int tarl_fused_rollout(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                  const float* times_host, float prev_time, const float* thresholds,
                                  const int64_t* log_probs, const float* entropy1, uint64_t policy_seed,
                                  uint64_t policy_counter0, float* agent_features, int64_t A, int64_t a_bstride,
                                  const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong,
                                  uint64_t seed, uint64_t counter0, int32_t* ins_scratch, uint8_t* sel_scratch,
                                  int64_t* acc_scratch, int32_t* choice_scratch, uint8_t* choice, float* log_prob,
                                  float* entropy, float* reward,
                                  uint8_t* counts, int32_t metrics_envs, float* dtt_node, uint8_t* events, int32_t* leg,
                                  tarl_stream stream) {
  int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc) return rc;
  TARL_REQUIRE(T >= 1 && times_host, "bad frame count / times");
  TARL_REQUIRE(thresholds && log_probs && entropy1, "policy tables missing (call tarl_fused_policy_prepare)");
  rc = tarl_check_frame_args(plan, f, B, agent_features, A, a_bstride, ins_scratch, edge_attr, log_edge_attr);
  if (rc) return rc;
  TARL_REQUIRE(metrics_envs >= 0 && metrics_envs <= B, "metrics_envs out of range");
  TARL_REQUIRE(metrics_envs > 0 || (!dtt_node && !events), "per-node series need metrics_envs > 0");
  if (plan->N == 0) return TARL_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = plan->N, NB = N * B;
  const unsigned threads = tile_threads(B);
  const dim3 grid((unsigned)ceil_div(B, threads), (unsigned)num_chunks(plan));
  const dim3 grid_c((unsigned)ceil_div(B, threads), (unsigned)ceil_div(N, nchunk_choice()));
  const dim3 grid_d((unsigned)ceil_div(B, threads), (unsigned)ceil_div(N, nchunk_dir()));
  const int want_lp = log_prob != nullptr ? 1 : 0;
  const FusedBufs fb = tarl_to_bufs(f);
  const PlanOut P{plan->out_ptr, plan->out_dst};
  // slice t of the action buffer (or, without one, the ping-pong pair f->sel8 / sel_scratch)
  auto slice = [&](int64_t t) -> uint8_t* {
    if (choice) return choice + t * NB;
    return (sel_scratch && (t & 1)) ? sel_scratch : f->sel8;
  };
  // steady state: frame t's insert and frame t+1's choice share ONE launch (k_fused_insert_choice); needs two distinct
  // SELECTED_ROAD slices and double-buffered log-prob accumulator banks
  // TARL_ROLLOUT_MERGE: 2 (default) = all actions precomputed on a side stream (needs the action buffer + choice_scratch),
  // 1 = frame t+1's choice shares frame t's insert launch, 0 = a choice launch per frame
  const char* knob = getenv("TARL_ROLLOUT_MERGE");
  const int mode = knob ? atoi(knob) : 2;
  const bool ahead = mode >= 2 && choice && choice_scratch && tarl_choice_ahead_fits(plan, T);
  const bool merge = !ahead && mode >= 1 && (choice || sel_scratch) && acc_scratch && T > 1;
  long long* acc_buf[2] = {(long long*)f->acc_lp, merge ? (long long*)acc_scratch : (long long*)f->acc_lp};
  if (merge) TARL_CHECK_HIP(hipMemsetAsync(acc_scratch, 0, (size_t)(f->acc_slots * B) * sizeof(int64_t), s));
  const FusedBufs* fbd = nullptr;      // [0]: the table with acc_buf[0], [1]: with acc_buf[1]
  rc = tarl_upload_bufs(f, fb, acc_buf[1], s, &fbd);
  if (rc) return rc;
  const hipEvent_t* drawn = nullptr;   // ahead: one event per block of frames whose actions the side stream has drawn
  if (ahead)
    rc = tarl_choice_ahead_queue(s, plan, f, B, T, thresholds, log_probs, policy_seed, policy_counter0, choice_scratch, choice,
                                 log_prob, &drawn);
  else
    rc = tarl_launch_choice(s, plan, f, B, acc_buf[0], thresholds, log_probs, nullptr, policy_seed, policy_counter0, slice(0),
                            (const uint8_t*)f->sel8, nullptr, want_lp);
  if (rc) return rc;
  const int epw_packed = tarl_insert_envs_per_wave(f, A, B, T, times_host);
  for (int64_t t = 0; t < T; ++t) {
    const int cur = merge ? (int)(t & 1) : 0;
    const float time = times_host[t];
    const FusedBufs* fbt = fbd + cur;
    const uint8_t* sel_t = slice(t);
    const FrameOut out = rollout_frame_out(t, T, N, B, counts, metrics_envs, dtt_node, events, leg);
    if (ahead) {
      rc = tarl_choice_ahead_wait(s, drawn, t);
      if (rc) return rc;
    }
    const bool timed = tarl_prof_mark(s, 0) != nullptr;
    rc = tarl_launch_direction(grid_d, threads, s, plan, f, edge_attr, log_edge_attr, sel_t, nullptr, nullptr, log_eps, time,
                               t > 0 ? times_host[t - 1] : prev_time, seed, counter0 + (uint64_t)t, B, (int)Nmax, out,
                               (counts && t > 0) ? counts + (t - 1) * NB : nullptr);   // the counts after frame t - 1
    if (rc) return rc;
    if (timed) (void)tarl_prof_mark(s, 1);
    rc = tarl_launch_rows(grid, threads, s, plan, f, fbt, (int)Nmax, B, agent_features, A, a_bstride, time, out);
    if (rc) return rc;
    if (timed) (void)tarl_prof_mark(s, 2);
    float* reward_t = reward ? reward + t * B : nullptr;
    float* lp_t = (log_prob && !ahead) ? log_prob + t * B : nullptr;   // ahead: written by k_fused_choice_all
    float* ent_t = entropy ? entropy + t * B : nullptr;
    if (merge && t + 1 < T) {
      const ChoiceArgs C{plan->out_ptr, plan->out_eid, plan->group_of_node, plan->G, thresholds,
                         (const long long*)log_probs, policy_seed, policy_counter0 + (uint64_t)(t + 1), nchunk_choice(),
                         want_lp, slice(t + 1), acc_buf[cur ^ 1], grid_c.x, grid_c.x * grid_c.y};
      rc = tarl_launch_insert_choice(C, threads, s, (int)Nmax, B, N, fbt, P, sel_t, agent_features, A, a_bstride, use_cong,
                                     time, ins_scratch, entropy1, reward_t, out, lp_t, ent_t);
    } else {
      rc = tarl_launch_insert(ahead ? epw_packed : 1, s, (int)Nmax, B, N, fbt, P, sel_t, agent_features, A, a_bstride,
                              use_cong, time, ins_scratch, entropy1, reward_t, out, lp_t, ent_t);
      if (!rc && !ahead && t + 1 < T)   // unmerged: the next frame's choice as its own launch
        rc = tarl_launch_choice(s, plan, f, B, acc_buf[cur], thresholds, log_probs, nullptr, policy_seed,
                                policy_counter0 + (uint64_t)(t + 1), slice(t + 1), sel_t, nullptr, want_lp);
    }
    if (rc) return rc;
    if (timed) (void)tarl_prof_mark(s, 3);
  }
  if (slice(T - 1) != f->sel8)   // the last frame's SELECTED_ROAD lives in the action buffer / scratch: bring it home
    TARL_CHECK_HIP(hipMemcpyAsync(f->sel8, slice(T - 1), (size_t)NB, hipMemcpyDeviceToDevice, s));
  return TARL_OK;
}

// ---- T frames with a STATE-DEPENDENT policy head in one foreign call (rollout_heads.h) ----------------------------------------
// Nothing of GraphDistribution can be hoisted: per frame [with tarl_fused_set_head_capture: the head ids of the frame's kept
// pairs, decision_credit.hip; the due heads alone under tarl_fused_set_head_capture_scope] -> the head's logits from the
// packed state (`frame`) -> action +
// log-prob + SELECTED_ROAD (tarl_graphdist_rollout) -> [with tarl_fused_set_policy_hold: the hold rule on SELECTED_ROAD,
// policy_hold.hip; the action buffer keeps the draw] -> [with tarl_fused_set_departure_router: the first hop of the agents
// about to depart from an empty road, departures.hip] -> Direction -> rows -> insert -> [with tarl_fused_set_trip_reward: the
// trip reward over the insert's reward, trip_reward.hip], queued back to back by one host loop
// in C (the same entry points a caller could queue himself, minus a foreign-call round trip per launch and the checks per
// frame). The arguments are checked and the pointer table is uploaded once per call; the count bytes are the frame
// kernels' own (FrameOut::counts8), the event byte is stored in the last frame only and the insert is packed
// (tarl_insert_envs_per_wave). The observations of the frames an optimiser minibatch will use are drawn beforehand (the draw
// does not depend on the data): keep_ptr_host[t] .. keep_ptr_host[t + 1] index the (environment, slot) pairs of frame t.
int tarl_rollout_head(const HeadRollout& a, head_frame_fn frame, void* ctx) {
  const tarl_plan* plan = a.plan;
  const tarl_fused* f = a.f;
  const int64_t B = a.B, T = a.T;
  int rc = tarl_check_fused_core(plan, f, B, a.Nmax);
  if (rc) return rc;
  TARL_REQUIRE(T >= 1 && a.times_host, "bad frame count / times");
  TARL_REQUIRE(a.x && a.logits_scratch && a.dist_scratch, "state / logits / sampler scratch missing");
  TARL_REQUIRE(!a.keep_ptr_host || (a.keep_env && a.keep_slot && a.obs_keep), "keep list without its arrays");
  rc = tarl_check_frame_args(plan, f, B, a.agent_features, a.A, a.a_bstride, a.ins_scratch, a.edge_attr, a.log_edge_attr);
  if (rc) return rc;
  TARL_REQUIRE(a.metrics_envs >= 0 && a.metrics_envs <= B, "metrics_envs out of range");
  TARL_REQUIRE(a.metrics_envs > 0 || (!a.dtt_node && !a.events), "per-node series need metrics_envs > 0");
  if (plan->N == 0) return TARL_OK;
  hipStream_t s = (hipStream_t)a.stream;
  const int64_t N = plan->N, NB = N * B;
  const unsigned threads = tile_threads(B);
  const dim3 grid((unsigned)ceil_div(B, threads), (unsigned)num_chunks(plan));
  const dim3 grid_d((unsigned)ceil_div(B, threads), (unsigned)ceil_div(N, nchunk_dir()));
  const FusedBufs* fb = nullptr;
  rc = tarl_upload_bufs(f, tarl_to_bufs(f), nullptr, s, &fb);
  if (rc) return rc;
  const PlanOut P{plan->out_ptr, plan->out_dst};
  const int epw_packed = tarl_insert_envs_per_wave(f, a.A, B, T, a.times_host);
  const bool route_departures = (f->policy_hold & TARL_DEPARTURE_ROUTER) != 0;   // tarl_fused_set_departure_router
  DepartureRouter router{};
  if (route_departures) {
    rc = tarl_departure_router_of(plan, f, &router);
    if (rc) return rc;
    for (int64_t t = 0; t < T; ++t) TARL_REQUIRE(std::isfinite(a.times_host[t]), "non-finite time");
  }
  const bool trip_reward = (f->policy_hold & TARL_TRIP_REWARD) != 0 && a.reward;     // tarl_fused_set_trip_reward
  int32_t* trip_parts = nullptr;
  if (trip_reward) {
    rc = tarl_check_trip_reward(f, B, a.A);
    if (rc) return rc;
    for (int64_t t = 0; t < T; ++t) TARL_REQUIRE(std::isfinite(a.times_host[t]), "non-finite time");
    trip_parts = tarl_trip_reward_parts_of(f);
  }
  int32_t* head_keep = nullptr;     // tarl_fused_set_head_capture: whom the kept pairs' roads decide for (decision_credit.hip)
  int head_scope = 0;
  int32_t* head_counts2 = nullptr;
  if ((f->policy_hold & TARL_HEAD_CAPTURE) != 0 && a.keep_ptr_host) {
    head_keep = tarl_head_capture_of(f);
    TARL_REQUIRE(head_keep, "head capture switched on without its buffer");
    for (int64_t t = 0; t < T; ++t) {
      rc = tarl_check_head_rows(plan, f, B, a.keep_ptr_host[t + 1] - a.keep_ptr_host[t]);
      if (rc) return rc;
    }
    head_scope = tarl_head_capture_scope_of(f, &head_counts2);      // tarl_fused_set_head_capture_scope: 1 = due heads only
    if (head_scope == 1)
      for (int64_t t = 0; t < T; ++t) TARL_REQUIRE(std::isfinite(a.times_host[t]), "non-finite time");
  }
  for (int64_t t = 0; t < T; ++t) {
    const bool keep_t = a.keep_ptr_host && a.keep_ptr_host[t + 1] > a.keep_ptr_host[t];
    const int64_t lo = keep_t ? a.keep_ptr_host[t] : 0, n = keep_t ? a.keep_ptr_host[t + 1] - lo : 0;
    if (head_keep && n) {
      rc = head_scope == 1 ? tarl_launch_head_rows_due(s, plan, f, B, a.times_host[t], a.keep_env + lo, a.keep_slot + lo, n,
                                                       head_keep, head_counts2)
                           : tarl_launch_head_rows(s, plan, f, B, a.keep_env + lo, a.keep_slot + lo, n, head_keep);
      if (rc) return rc;
    }
    rc = frame(a, ctx, t, a.keep_env + lo, a.keep_slot + lo, n);
    if (rc) return rc;
    rc = tarl_graphdist_rollout_at(plan, a.logits_scratch, B, a.temperature, nullptr, a.policy_seed,
                                   a.policy_counter0 + (uint64_t)t, a.dist_scratch, nullptr,
                                   a.choice8 ? a.choice8 + t * NB : nullptr, f->sel8, a.log_prob ? a.log_prob + t * B : nullptr,
                                   f->env_base, a.stream);
    if (rc) return rc;
    if (f->policy_hold & 1) {   // tarl_fused_set_policy_hold: the hold rule on f->sel8; a.choice8 keeps the draw (policy_hold.hip)
      rc = tarl_launch_policy_hold(s, plan, f, B, a.agent_features, a.A, a.a_bstride, nullptr, f->policy_held);
      if (rc) return rc;
    }
    const float time = a.times_host[t];
    if (route_departures) {     // empty origin rows select for their departing agent (departures.hip); a.choice8 keeps the draw
      rc = tarl_launch_departure_router(s, plan, f, B, a.A, time, router);
      if (rc) return rc;
    }
    const FrameOut out = rollout_frame_out(t, T, N, B, a.counts, a.metrics_envs, a.dtt_node, a.events, a.leg);
    rc = tarl_launch_direction(grid_d, threads, s, plan, f, a.edge_attr, a.log_edge_attr, (const uint8_t*)f->sel8, nullptr,
                               nullptr, a.log_eps, time, t > 0 ? a.times_host[t - 1] : a.prev_time, a.seed,
                               a.counter0 + (uint64_t)t, B, (int)a.Nmax, out);
    if (rc) return rc;
    rc = tarl_launch_rows(grid, threads, s, plan, f, fb, (int)a.Nmax, B, a.agent_features, a.A, a.a_bstride, time, out);
    if (rc) return rc;
    rc = tarl_launch_insert(epw_packed, s, (int)a.Nmax, B, N, fb, P, (const uint8_t*)f->sel8, a.agent_features, a.A,
                            a.a_bstride, a.use_cong, time, a.ins_scratch, nullptr, a.reward ? a.reward + t * B : nullptr, out,
                            nullptr, nullptr);
    if (rc) return rc;
    if (trip_reward) {          // the frame is complete: the travellers owed over the insert's queue reward (trip_reward.hip)
      rc = tarl_launch_trip_reward(s, f, B, a.A, time, a.reward + t * B, trip_parts ? trip_parts + t * B * 2 : nullptr);
      if (rc) return rc;
    }
  }
  return TARL_OK;
}

// ---- the per-edge MLP head: observation (tarl_fused_obs16) -> logits (tarl_policy_edge_mlp_fwd) ---------------------------------
__global__ __launch_bounds__(FB) void k_obs_keep(const float4* __restrict__ obs, int64_t row4,
                                                 const int32_t* __restrict__ env, const int32_t* __restrict__ slot,
                                                 float4* __restrict__ keep) {
  const int64_t j = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (j >= row4) return;
  keep[(int64_t)slot[blockIdx.y] * row4 + j] = obs[(int64_t)env[blockIdx.y] * row4 + j];
}

struct EdgeMlpHead {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int precision;
  float* obs_scratch;
};

static int edge_mlp_frame(const HeadRollout& a, void* ctx, int64_t, const int32_t* env, const int32_t* slot, int64_t n) {
  const EdgeMlpHead& h = *(const EdgeMlpHead*)ctx;
  hipStream_t s = (hipStream_t)a.stream;
  const bool obs_bf16 = h.precision == 1;
  const int64_t row4 = a.plan->N * 4;
  TARL_REQUIRE(n < 65536, "more than 65535 kept observations in one frame");
  // bf16 logits read bf16 observations (half the bytes written here and gathered by the MLP); the fp32 rows an
  // optimiser step keeps are evaluated for their few environments only. fp32 observations: the kept rows are copies
  int rc = obs_bf16 ? tarl_fused_obs16_bf16(a.plan, a.f, a.x, a.B, a.x_bstride, a.ldx, a.Nmax, a.agent_features, a.A,
                                            a.a_bstride, (uint16_t*)h.obs_scratch, a.stream)
                    : tarl_fused_obs16(a.plan, a.f, a.x, a.B, a.x_bstride, a.ldx, a.Nmax, a.agent_features, a.A, a.a_bstride,
                                       h.obs_scratch, a.stream);
  if (!rc && obs_bf16) rc = tarl_head_keep_rows(a, env, slot, n);
  if (rc) return rc;
  if (n && !obs_bf16) {
    hipLaunchKernelGGL(k_obs_keep, dim3((unsigned)ceil_div(row4, FB), (unsigned)n), dim3(FB), 0, s,
                       (const float4*)h.obs_scratch, row4, env, slot, (float4*)a.obs_keep);
    TARL_LAUNCH_CHECK();
  }
  // (live timing, bench.py: HIP events around the per-edge MLP of the timed frames — slot 0 of tarl_prof_collect)
  const bool timed = tarl_prof_mark(s, 0) != nullptr;
  rc = tarl_policy_edge_mlp_fwd(a.plan, h.obs_scratch, a.B, a.edge_attr, h.w1, h.b1, h.w2, h.b2, h.w3, h.b3,
                                h.precision == 1 ? 2 : (h.precision == 2 ? 3 : 0), a.logits_scratch, a.stream);
  if (rc) return rc;
  if (timed) (void)tarl_prof_mark(s, 1);
  return TARL_OK;
}

extern "C" int tarl_fused_rollout_policy(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                         const float* times_host, float prev_time, const float* x, int64_t x_bstride,
                                         int64_t ldx, float* agent_features, int64_t A, int64_t a_bstride,
                                         const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong,
                                         const float* w1, const float* b1, const float* w2, const float* b2,
                                         const float* w3, const float* b3, int precision, float temperature,
                                         uint64_t policy_seed, uint64_t policy_counter0, uint64_t seed,
                                         uint64_t counter0, const int64_t* keep_ptr_host, const int32_t* keep_env,
                                         const int32_t* keep_slot, float* obs_keep, float* obs_scratch,
                                         float* logits_scratch, void* dist_scratch, int32_t* ins_scratch,
                                         uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                                         int32_t metrics_envs, float* dtt_node, uint8_t* events, int32_t* leg,
                                         tarl_stream stream) {
  TARL_REQUIRE(obs_scratch, "observation scratch missing");
  TARL_REQUIRE(precision >= 0 && precision <= 2,
               "precision: 0 = fp32 MFMA logits, 1 = bf16 logits on bf16 observations, 2 = fp32-accurate logits on the bf16 pipe (bf16x3)");
  EdgeMlpHead h{w1, b1, w2, b2, w3, b3, precision, obs_scratch};
  return tarl_rollout_head(HeadRollout{plan, f, B, Nmax, T, times_host, prev_time, x, x_bstride, ldx, agent_features, A,
                                       a_bstride, edge_attr, log_edge_attr, log_eps, use_cong, temperature, policy_seed,
                                       policy_counter0, seed, counter0, keep_ptr_host, keep_env, keep_slot, obs_keep,
                                       logits_scratch, dist_scratch, ins_scratch, choice8, log_prob, reward, counts,
                                       metrics_envs, dtt_node, events, leg, stream},
                           edge_mlp_frame, &h);
}
