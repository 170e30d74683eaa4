// rollout_heads.h — internal: the T-frame rollout of a STATE-DEPENDENT policy head, written once (tarl_rollout_head,
// fused_rollout.hip). A head — the per-edge MLP (fused_rollout.hip), the shortest-path prior (prior.hip), the graph
// transformer (gt_policy.hip) — is "how the packed state of frame t becomes logits_scratch"; what a rollout frame is
// (sampler, Direction, rows, insert, the side outputs) lives in the loop alone.
#pragma once
#include "fused_common.h"

// what every head's entry point takes, in the order of the extern "C" signatures (include/tarl_hip.h)
struct HeadRollout {
  const tarl_plan* plan;
  const tarl_fused* f;
  int64_t B;
  int32_t Nmax;
  int64_t T;
  const float* times_host;
  float prev_time;
  const float* x;
  int64_t x_bstride, ldx;
  float* agent_features;
  int64_t A, a_bstride;
  const float *edge_attr, *log_edge_attr;
  float log_eps;
  int use_cong;
  float temperature;
  uint64_t policy_seed, policy_counter0, seed, counter0;
  const int64_t* keep_ptr_host;     // keep_ptr_host[t] .. keep_ptr_host[t + 1]: the (environment, slot) pairs kept of frame t
  const int32_t *keep_env, *keep_slot;
  float *obs_keep, *logits_scratch;
  void* dist_scratch;
  int32_t* ins_scratch;
  uint8_t* choice8;
  float *log_prob, *reward;
  uint8_t* counts;
  int32_t metrics_envs;             // the per-step logs: the edge MLP's entry point alone has the arguments
  float* dtt_node;
  uint8_t* events;
  int32_t* leg;
  tarl_stream stream;
};

// Frame t of a head, from the packed state as frame t - 1 left it: the observation rows of the n kept pairs (env[j], slot[j])
// -> obs_keep (n may be 0), the logits of all environments -> logits_scratch. State-independent work belongs to t == 0.
typedef int (*head_frame_fn)(const HeadRollout& a, void* ctx, int64_t t, const int32_t* env, const int32_t* slot, int64_t n);

// Checks the common arguments once, then queues per frame: [the head ids of the frame's kept pairs, where bit
// TARL_HEAD_CAPTURE of tarl_fused.policy_hold is set] -> head -> tarl_graphdist_rollout_at (action bytes, log-prob,
// SELECTED_ROAD) -> [the hold rule, where bit 0 of tarl_fused.policy_hold is set] -> [the pending table and the first-hop
// route launch, where its bit TARL_DEPARTURE_ROUTER is set] -> Direction -> rows -> insert, the count bytes written by the
// frame kernels -> [the trip reward over the insert's reward, where its bit TARL_TRIP_REWARD is set].
int tarl_rollout_head(const HeadRollout& a, head_frame_fn frame, void* ctx);

// policy_hold.hip: the launch of k_fused_hold_policy_actions alone (handle and agent table checked by the caller)
int tarl_launch_policy_hold(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, const float* agent_features,
                            int64_t A, int64_t a_bstride, uint8_t* choice8, int32_t* held);

// departures.hip: first-hop routing inside the loop (tarl_fused_set_departure_router; bit TARL_DEPARTURE_ROUTER of
// tarl_fused.policy_hold). tarl_departure_router_of: what the setter registered for the handle, checked against the plan;
// tarl_launch_departure_router: the pending table and the table-lookup route launch of one frame whose clock is t.
struct DepartureRouter {
  const int32_t *dest_slot, *next_hop;
  int64_t nh_bstride, D;
  int32_t *pend, *routed;
};
int tarl_departure_router_of(const tarl_plan* plan, const tarl_fused* f, DepartureRouter* r);
int tarl_launch_departure_router(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, float t,
                                 const DepartureRouter& r);

// trip_reward.hip: the trip reward inside the loop (tarl_fused_set_trip_reward; bit TARL_TRIP_REWARD of
// tarl_fused.policy_hold). tarl_check_trip_reward: the agent buffers and sizes; tarl_trip_reward_parts_of: the parts buffer the
// setter registered for the handle, or NULL; tarl_launch_trip_reward: the launches of one frame whose clock is t.
int tarl_check_trip_reward(const tarl_fused* f, int64_t B, int64_t A);
int32_t* tarl_trip_reward_parts_of(const tarl_fused* f);
int tarl_launch_trip_reward(hipStream_t s, const tarl_fused* f, int64_t B, int64_t A, float t, float* reward, int32_t* parts);

// decision_credit.hip: the head capture inside the loop (tarl_fused_set_head_capture; bit TARL_HEAD_CAPTURE of
// tarl_fused.policy_hold). tarl_head_capture_of: the buffer the setter registered for the handle, or NULL;
// tarl_check_head_rows: the sizes of one launch over n pairs; tarl_launch_head_rows: the launch alone (n >= 1).
int32_t* tarl_head_capture_of(const tarl_fused* f);
int tarl_check_head_rows(const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t n);
int tarl_launch_head_rows(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* env,
                          const int32_t* slot, int64_t n, int32_t* head_keep);
// credit scope "due" (tarl_fused_set_head_capture_scope): tarl_head_capture_scope_of: 0 = headed (also when the setter was
// never called), 1 = due, and the {headed, due} counters it registered, or NULL; tarl_launch_head_rows_due: the launch that
// takes tarl_launch_head_rows' place under scope 1, with the clock the frame is stepped with.
int tarl_head_capture_scope_of(const tarl_fused* f, int32_t** counts2);
int tarl_launch_head_rows_due(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, float t_clock,
                              const int32_t* env, const int32_t* slot, int64_t n, int32_t* head_keep, int32_t* counts2);

// the kept rows straight from the packed state (a head whose logits do not leave fp32 observations behind)
static inline int tarl_head_keep_rows(const HeadRollout& a, const int32_t* env, const int32_t* slot, int64_t n) {
  if (n == 0) return TARL_OK;
  return tarl_fused_obs16_rows(a.plan, a.f, a.x, a.B, a.x_bstride, a.ldx, a.Nmax, a.agent_features, a.A, a.a_bstride, env, slot,
                               n, a.obs_keep, a.stream);
}
