/* tarl_hip.h — C ABI of libtarl_hip.so: hand-written HIP kernels (gfx950 / MI355X) for TARL-simulator's MPNN + PPO
 * routing hot path.
 *
 * The reference (OliBus801/TARL-simulator) is pure Python and has no FFI of its own; the path sits behind Python
 * classes. Each entry point below names the reference interface it replaces (file:line in the
 * reference tree). The host-side mirror of those classes (tarl-simulator_amd/src/...) binds this library with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - Every data pointer is a DEVICE pointer unless the name ends in `_host`. Buffers are caller-owned (torch
 *    allocations); the library borrows them for the duration of the call and never allocates per call.
 *  - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the host is never synchronised
 *    (except tarl_plan_create, which uploads the static plan with blocking copies).
 *  - Return value: 0 = ok, negative = tarl_status error; tarl_last_error() returns a thread-local message.
 *  - Batched state: B independent environments over ONE static graph. x is fp32 [B][R][ldx] with
 *    ldx >= F = 3*Nmax+7 (row stride in floats) and x_bstride (env stride in floats); column map as in
 *    src/feature_helpers.py:38-54. agent_features is fp32 [B][A][9] (src/feature_helpers.py:59-71).
 *  - Randomness is an input: pass explicit noise tensors for parity, or NULL to draw Philox4x32-10 on device from
 *    (seed, counter).
 */
#ifndef TARL_HIP_H
#define TARL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TARL_ABI_VERSION 5

typedef enum {
  TARL_OK = 0,
  TARL_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, index out of range) */
  TARL_ERR_HIP = -2,       /* a HIP runtime call failed */
  TARL_ERR_NOMEM = -3,
  TARL_ERR_UNSUPPORTED = -4
} tarl_status;

/* bits of a device status word (sticky; the caller reads it at its next synchronisation point) */
#define TARL_FLAG_COUNT_AT_NMAX 1
#define TARL_FLAG_AMBIGUOUS_EDGES 2
#define TARL_FLAG_PACK_RANGE 4
#define TARL_FLAG_CHOICE_OVERFLOW 8

typedef struct tarl_plan tarl_plan; /* opaque static per-graph plan */
typedef void* tarl_stream;          /* hipStream_t */

int tarl_abi_version(void);
/* The experiment flags (-DTARL_EXP_... of `make variant`) this library was built with; "" for the product build. The test
 * suite refuses to run against a library that reports any (tests/conftest.py): a timing-only developer build must never
 * stand in for the product in a parity run. */
const char* tarl_build_flags(void);
const char* tarl_last_error(void);

/* ---- static plan ---------------------------------------------------------------------------------------------
 * Replaces the per-step sort/argsort/unique of GraphDistribution.__init__ (src/reinforcement_learning.py:21-35)
 * and PyG's per-call gather indices (src/direction_mpnn.py:230, src/response_mpnn.py:40): int32 CSC (in-edges by
 * destination, ascending original edge id) and CSR (out-edges by source) built once.
 * edge_index_host: int64 [2][E] on the HOST. src_order_host (nullable): permutation of 0..E-1 that sorts
 * edge_index[0]; NULL = stable order (the reference's pinned CPU behaviour). */
int tarl_plan_create(const int64_t* edge_index_host, int64_t num_edges, int64_t num_nodes,
                     const int64_t* src_order_host, tarl_plan** out);
void tarl_plan_destroy(tarl_plan* plan);
/* info[0..5] = num_nodes, num_edges, num_groups (distinct sources), max_in_degree, max_out_degree, src_sorted */
int tarl_plan_info(const tarl_plan* plan, int64_t* info6_host);
/* launch-geometry facts of the plan (diagnostics / tests): info3_host = {siblings4: the rows 4c .. 4c+3 share their first
 * four in-edge sources for every c (Direction gather reads them once per chunk), row_siblings: the row pass walks the
 * row-chunk table (rows grouped by their out-edge targets), num_row_chunks} */
int tarl_plan_geometry(const tarl_plan* plan, int64_t* info3_host);

/* ---- traffic-flow step ---------------------------------------------------------------------------------------
 * tarl_direction_step == DirectionMPNN.forward: message + aggregate + update (src/direction_mpnn.py:44-196,210-236).
 *   edge_attr [E]; log_edge_attr [E] = log(edge_attr + 1e-12) and log_eps = log(1e-12), both evaluated by the host
 *   (so the Gumbel scores are bit-identical to the reference's fp32 ones); congestion_constant [R] or NULL
 *   (then recomputed from x as src/simulation_core_model.py:55-67 does); gumbel [B][E] or NULL (device Philox);
 *   delta_travel_time [B][E] or NULL (side output, src/direction_mpnn.py:94-96); chosen [B][R] scratch/out.
 *   x is updated in place (every row, also when nothing was chosen).
 *   status: int32[1] device status word or NULL: TARL_FLAG_COUNT_AT_NMAX is OR-ed in when a count reaches Nmax (a
 *   gridlock-relief move into a full FIFO): the reference raises IndexError at its next update (:172-191). */
int tarl_direction_step(const tarl_plan* plan, float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                        int64_t num_roads, const float* edge_attr, const float* log_edge_attr, float log_eps,
                        const float* congestion_constant, float time, const float* gumbel, uint64_t seed,
                        uint64_t counter, float* delta_travel_time, float* chosen, int32_t* status, tarl_stream stream);

/* tarl_response_step == ResponseMPNN.forward: message + max-aggregate + update (src/response_mpnn.py:25-127).
 *   popped [B][R] uint8 out (the update mask appended to update_history, :125); any_popped: int32[1] or NULL,
 *   set to 1 iff any row of any environment popped (the `.any()` of :106, kept on device). */
int tarl_response_step(const tarl_plan* plan, float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                       int64_t num_roads, uint8_t* popped, int32_t* any_popped, tarl_stream stream);

/* tarl_core_step == SimulationCoreModel.forward (src/simulation_core_model.py:41-83): both rounds, same outputs as
 * the two calls above, fused into fewer launches. */
int tarl_core_step(const tarl_plan* plan, float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                   int64_t num_roads, const float* edge_attr, const float* log_edge_attr, float log_eps,
                   const float* congestion_constant, float time, const float* gumbel, uint64_t seed, uint64_t counter,
                   float* delta_travel_time, float* chosen, uint8_t* popped, int32_t* any_popped, int32_t* status,
                   tarl_stream stream);

/* ---- environment step around the core (src/reinforcement_learning.py:222-309, src/agents/base.py:244-403) -------
 * tarl_apply_action: x[b, src(e), SELECTED_ROAD] = dst(e) for every edge with action[b][e] != 0 (:223-231).
 *   Exactly one of action_onehot (int64 [B][E], the reference's action format) / choice (int32 [B][N]: chosen edge id
 *   per source node, -1 = none) must be non-NULL. */
int tarl_apply_action(const tarl_plan* plan, float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                      const int64_t* action_onehot, const int32_t* choice, tarl_stream stream);

/* tarl_withdraw_step == Agents.withdraw_agent_from_network (src/agents/base.py:348-403) over all num_nodes rows;
 *   adjacency = the plan's edge set (replaces the dense N x N bool matrix). withdrawn [B][num_nodes] uint8 or NULL. */
int tarl_withdraw_step(const tarl_plan* plan, float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax,
                       int64_t num_nodes, float* agent_features, int64_t num_agents, int64_t a_bstride, float time,
                       uint8_t* withdrawn, tarl_stream stream);

/* tarl_insert_step == Agents.insert_agent_into_network (src/agents/base.py:247-331), stable (agent-id) order within
 *   a road. congestion_constant [num_nodes] or NULL (then time_congestion = 0, as :312-313).
 *   ready_scratch: int32 [B][2 * num_agents]. Also emits, when non-NULL, reward [B] = -sum_rows NUMBER_OF_AGENT
 *   (src/reinforcement_learning.py:266-267) and counts [B][num_nodes] (the NUMBER_OF_AGENT column, the critic input). */
int tarl_insert_step(float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax, int64_t num_nodes,
                     float* agent_features, int64_t num_agents, int64_t a_bstride, const float* congestion_constant,
                     float time, int32_t* ready_scratch, float* reward, float* counts, tarl_stream stream);

/* tarl_reset_state == TransportationSimulator.reset + Agents.reset (src/transportation_simulator.py:353-358,
 *   src/agents/base.py:496-503): zero FIFO blocks and NUMBER_OF_AGENT, clear ON_WAY / DONE. agent_features nullable. */
int tarl_reset_state(float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax, int64_t num_nodes,
                     float* agent_features, int64_t num_agents, int64_t a_bstride, tarl_stream stream);

/* ---- GraphDistribution (src/reinforcement_learning.py:15-96) ---------------------------------------------------
 * tarl_graphdist_softmax: proba = scatter_softmax(logits / temperature, src) (:25); logits/proba [B][E] in original
 *   edge order. */
int tarl_graphdist_softmax(const tarl_plan* plan, const float* logits, int64_t B, float temperature, float* proba,
                           tarl_stream stream);
/* tarl_graphdist_sample (:62-80 with the cumsum of :38-42): per source node the first out-edge (plan order) with
 *   u < cum, cum = fp32(fp32(base + s) - fp32(base)) with base/s accumulated in double like torch's CPU cumsum.
 *   uniform [B][num_groups] or NULL (Philox). Outputs (each nullable): action_onehot int64 [B][E]; choice int32 [B][N]
 *   (edge id or -1). group_sums: double scratch [B][num_groups + 1]. */
int tarl_graphdist_sample(const tarl_plan* plan, const float* proba, int64_t B, const float* uniform, uint64_t seed,
                          uint64_t counter, double* group_sums, int64_t* action_onehot, int32_t* choice,
                          tarl_stream stream);
/* tarl_graphdist_rollout: the action draw of one rollout frame in ONE launch for a policy whose logits [B][E] change every
 *   frame: GraphDistribution(logits / temperature).sample() and .log_prob(action) (src/reinforcement_learning.py:16-96),
 *   i.e. tarl_graphdist_softmax -> tarl_graphdist_sample -> tarl_graphdist_logprob_entropy_fwd with identical arithmetic and
 *   summation orders (actions and log-probs are bit-identical to that chain), without materialising the probabilities.
 *   uniform [B][num_groups] or NULL (Philox keyed by seed / counter / b * num_groups + g, as tarl_graphdist_sample).
 *   scratch: tarl_graphdist_rollout_scratch_bytes(plan, B) bytes, 8-byte aligned. Outputs, each nullable: choice int32
 *   [B][N] (edge id, -1 = none); choice8 uint8 [B][N] = the rank byte of the rollout buffers (rank of the chosen
 *   out-edge, or 0x80 | previous rank where nothing was drawn); sel8 uint8 [N][B] = tarl_fused.sel8, updated in place
 *   (== tarl_fused_apply_choice of the drawn action: the choice phase of SimulatorEnv._step, :228-233); log_prob [B].
 *   choice8 / sel8 need out-degree <= 126 (bit 7 of the byte means "drew nothing"): refused otherwise, before any
 *   launch; choice alone has no such limit. */
int64_t tarl_graphdist_rollout_scratch_bytes(const tarl_plan* plan, int64_t B);
int tarl_graphdist_rollout(const tarl_plan* plan, const float* logits, int64_t B, float temperature, const float* uniform,
                           uint64_t seed, uint64_t counter, void* scratch, int32_t* choice, uint8_t* choice8,
                           uint8_t* sel8, float* log_prob, tarl_stream stream);
/* tarl_graphdist_mode (:45-55): one-hot (fp32, like zeros_like(proba)) of the per-node argmax, first maximum wins. */
int tarl_graphdist_mode(const tarl_plan* plan, const float* proba, int64_t B, float* mode_onehot, int32_t* choice,
                        tarl_stream stream);
/* tarl_graphdist_mode_rollout: the MODE counterpart of tarl_graphdist_rollout — the deterministic action of
 *   GraphDistribution(logits / temperature) (:45-55: per source node the out-edge with the largest PROBABILITY, the first
 *   maximum in original edge order wins; torchrl's ExplorationType.MODE, src/rl/ppo_trainer.py:149) and its log_prob
 *   (:82-96) for per-frame logits [B][E] in ONE launch, without materialising the probabilities. The comparison is made on
 *   p as tarl_graphdist_softmax computes it, not on the logits (unequal logits may round to equal p; a node whose
 *   candidates all carry the prior head's -1e20 sentinel has equal p everywhere: the first edge wins). Action and log_prob
 *   are bit-identical to tarl_graphdist_softmax -> tarl_graphdist_mode -> tarl_graphdist_logprob_entropy_fwd.
 *   Outputs, each nullable (at least one given), as tarl_graphdist_rollout: choice int32 [B][N] (edge id, -1 = none);
 *   choice8 uint8 [B][N] (rank of the chosen out-edge in the node's CSR list, 0x80 | previous rank for a node without
 *   out-edges); sel8 uint8 [N][B] = tarl_fused.sel8, updated in place (== tarl_fused_apply_choice of the action);
 *   log_prob [B]. No scratch, no noise. */
int tarl_graphdist_mode_rollout(const tarl_plan* plan, const float* logits, int64_t B, float temperature, int32_t* choice,
                                uint8_t* choice8, uint8_t* sel8, float* log_prob, tarl_stream stream);
/* tarl_episode_summary: what an evaluation reports (src/rl/ppo_trainer.py:89-127: the return is the sum of the rewards;
 *   src/runner.py:147-150: arrived agents = DONE == 1 and their mean ARRIVAL_TIME - DEPARTURE_TIME; the leg histogram's
 *   "on the way" = the ON_WAY flag count), per environment, from agent_features fp32 [B][num_agents][9] (environment stride
 *   a_bstride floats; row 0 is the dummy and is skipped):
 *   counts int32 [B][3] = {arrived (DONE == 1), on the way (ON_WAY == 1 and not arrived), not yet departed (neither)};
 *   sums fp64 [B][3] = {sum tt, sum tt^2, max tt} over the arrived agents, tt = ARRIVAL_TIME - DEPARTURE_TIME (fp32
 *     difference, widened); max tt = 0 where nobody arrived; fixed summation order, no floating-point atomics;
 *   episode_return fp64 [B] (nullable) = sum over t < T of reward [T][B] (nullable when T == 0) in frame order;
 *   hist int32 [B][num_bins] (nullable; 1 <= num_bins <= 16384, bin_width > 0): travel-time histogram of the arrived
 *     agents, bin min(floor(tt / bin_width), num_bins - 1), tt < 0 (or NaN) counted in bin 0. */
int tarl_episode_summary(const float* agent_features, int64_t B, int64_t num_agents, int64_t a_bstride,
                         const float* reward, int64_t T, float bin_width, int32_t num_bins, int32_t* counts, double* sums,
                         double* episode_return, int32_t* hist, tarl_stream stream);
/* tarl_graphdist_logprob_entropy_fwd (:82-96): log_prob [B] = sum_e a_e log(p_e + 1e-8), -inf when the action is not
 *   exactly one edge per source node; entropy [B] = -sum_e p_e log(p_e + 1e-8). Action given as one-hot or choice.
 *   Outputs nullable. One workgroup per batch row, fixed reduction order. */
int tarl_graphdist_logprob_entropy_fwd(const tarl_plan* plan, const float* proba, int64_t B,
                                       const int64_t* action_onehot, const int32_t* choice, float* log_prob,
                                       float* entropy, tarl_stream stream);
/* backward of (log_prob, entropy) w.r.t. logits through the segment softmax: grad_logits [B][E] (overwritten).
 *   grad_log_prob / grad_entropy [B] nullable (= 0). log_prob_fwd [B] nullable: rows whose forward log_prob is -inf
 *   get zero log-prob gradient (the reference assigns -inf through a mask, :91). */
int tarl_graphdist_logprob_entropy_bwd(const tarl_plan* plan, const float* proba, int64_t B, float temperature,
                                       const int64_t* action_onehot, const int32_t* choice,
                                       const float* grad_log_prob, const float* grad_entropy,
                                       const float* log_prob_fwd, float* grad_logits, tarl_stream stream);

/* ---- policy / critic (src/agents/mpnn_agent.py) ------------------------------------------------------------------
 * tarl_policy_edge_logits_fwd: live MPNNPolicyNet.forward (:175-178,215-217):
 *   logits[b][e] = emb[(int) road_index[b][dst(e)]]; road_index points at the ROAD_INDEX observation column with
 *   element strides (ri_bstride, ri_nstride); emb [num_embeddings]. */
int tarl_policy_edge_logits_fwd(const tarl_plan* plan, const float* road_index, int64_t ri_bstride,
                                int64_t ri_nstride, int64_t B, const float* emb, int64_t num_embeddings,
                                float* logits, tarl_stream stream);
/* backward: grad_emb [num_embeddings] += sum_b sum_{e: dst(e)=n} grad_logits[b][e], one fp32 add per (node, embedding) run
 *   of batch rows (bit-reproducible while ROAD_INDEX is one-to-one). scratch (nullable): fp32,
 *   tarl_policy_edge_logits_bwd_scratch_floats(plan, B) elements — with it, a broadcast observation (ri_bstride == 0) and
 *   >= 256 rows the sum over the rows runs in parallel chunks of 64 rows whose partial sums are added in chunk order. */
int64_t tarl_policy_edge_logits_bwd_scratch_floats(const tarl_plan* plan, int64_t B);
int tarl_policy_edge_logits_bwd(const tarl_plan* plan, const float* road_index, int64_t ri_bstride,
                                int64_t ri_nstride, int64_t B, const float* grad_logits, float* grad_emb,
                                int64_t num_embeddings, float* scratch, tarl_stream stream);

/* ---- the per-edge MLP head of MPNNPolicyNet (src/agents/mpnn_agent.py:35-41; evaluation spelled out at :227-231) -----
 * logits[m][e] = W3 relu(W2 relu(W1 cat(x[m][src(e)], x[m][dst(e)], edge_attr[e]) + b1) + b2) + b3, 33 -> 64 -> 32 -> 1,
 * weights in the reference's state-dict layout (edge_mlp.{0,2,4}.{weight,bias}: w1 [64][33], w2 [32][64], w3 [32]).
 * obs16 [M][N][16] = x = cat(node_features (7), agent_features[agent_index] (9)) per node (:166-178), built by
 *   tarl_policy_obs16 (from the reference's observation tensors: node_features [M][N][>=7] with row stride nf_ld,
 *   agent_index int64 [M][N], agent_features [A][9] shared (a_mstride = 0) or per sample) or by tarl_fused_obs16 (from the
 *   packed state of the fused engine, environment b = sample m; x supplies the static LENGTH / MAX_FLOW columns).
 * precision 0: fp32 MFMA (v_mfma_f32_32x32x2_f32; exact fp32 products); 1: bf16 MFMA (v_mfma_f32_32x32x16_bf16; inputs,
 *   weights and the first hidden activation rounded to bf16, fp32 accumulation) — BASELINE config 5's bf16 features;
 *   2: as 1 with obs16 pointing at bf16 observations, uint16 [M][N][16] (tarl_fused_obs16_bf16): same values, half the
 *   bytes gathered, deeper prefetch; 3: fp32 ACCURACY on the bf16 pipe — fp32 observations, weights and the first hidden
 *   activation each split into three exact bf16 pieces, the six piece products of order >= 2^-16 accumulated in fp32
 *   (logits within a few fp32 ulp of precision 0's; 50 bf16 MFMAs instead of 66 fp32 MFMAs of twice the passes).
 * tarl_policy_edge_mlp_bwd ACCUMULATES (+=) the gradients of sum(grad_logits * logits) into gw1 [64][33], gb1 [64],
 *   gw2 [32][64], gb2 [32], gw3 [32], gb3 [1] (fp32, fixed reduction order); scratch: fp32
 *   [tarl_policy_edge_mlp_bwd_scratch_floats(plan, M)]. Observations receive no gradient. */
int tarl_policy_obs16(const float* node_features, int64_t nf_ld, const int64_t* agent_index,
                      const float* agent_features, int64_t num_agents, int64_t a_mstride, int64_t M, int64_t num_nodes,
                      float* obs16, tarl_stream stream);
int tarl_policy_edge_mlp_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr,
                             const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                             const float* b3, int precision, float* logits, tarl_stream stream);
int64_t tarl_policy_edge_mlp_bwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_policy_edge_mlp_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr,
                             const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                             const float* b3, const float* grad_logits, float* scratch, float* gw1, float* gb1,
                             float* gw2, float* gb2, float* gw3, float* gb3, tarl_stream stream);

/* tarl_critic_mlp_fwd == MPNNValueNetSimple.forward (:428-450): value = W3 relu(W2 relu(W1 [counts, time] + b1) + b2) + b3
 *   with the reference's state-dict layout: w1 [64][N+1] (last input column = time), w2 [64][64], w3 [64] (= [1][64]).
 *   counts [M][ldc] = the NUMBER_OF_AGENT observation column per node (row stride ldc >= N); time_rows[m / rows_per_time]
 *   is row m's clock (rows_per_time = B for a time-major [T][B] rollout buffer, 1 for per-row times).
 *   value [M]; h1_out / h2_out [M][64] nullable (post-ReLU activations kept for the backward). fp32 MFMA
 *   (v_mfma_f32_32x32x2_f32, exact fp32 products), hidden tile kept in LDS. */
int tarl_critic_mlp_fwd(const float* counts, int64_t ldc, int64_t M, int64_t N, const float* time_rows,
                        int64_t rows_per_time, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, float* value, float* h1_out, float* h2_out,
                        tarl_stream stream);
/* backward for minibatch-sized M: ACCUMULATES (+=) into gw1 [64][N+1], gb1 [64], gw2 [64][64], gb2 [64], gw3 [64],
 *   gb3 [1]; scratch: fp32, tarl_critic_mlp_bwd_scratch_floats(M, N) elements ([2][M][64] for the reference's sub-batch of a
 *   few dozen rows; from 512 rows on the reductions over the rows run in parallel row chunks that leave partial sums there,
 *   added in chunk order: deterministic, no atomics). */
int64_t tarl_critic_mlp_bwd_scratch_floats(int64_t M, int64_t N);
int tarl_critic_mlp_bwd(const float* counts, int64_t ldc, int64_t M, int64_t N, const float* time_rows,
                        int64_t rows_per_time, const float* w1, const float* w2, const float* w3, const float* h1,
                        const float* h2, const float* grad_value, float* scratch, float* gw1, float* gb1, float* gw2,
                        float* gb2, float* gw3, float* gb3, tarl_stream stream);

/* ---- PPO update (src/rl/ppo_trainer.py:35-37,129-145; torchrl 0.5.0 GAE / ClipPPOLoss formulas) ---------
 * tarl_gae: GAE(gamma, lmbda) over time-major [T][B] tensors; next_value[t] = V(next obs of frame t) (for an unbroken
 *   rollout pass value + B of a [T+1][B] buffer); done / terminated uint8 nullable (= all false).
 *   advantage (un-normalised) and value_target = advantage + value are written. */
int tarl_gae(const float* reward, const float* value, const float* next_value, const uint8_t* done,
             const uint8_t* terminated, int64_t T, int64_t B, float gamma, float lmbda, float* advantage,
             float* value_target, tarl_stream stream);
/* average_gae=True: stats = {sum, sum of squares, count} in double (partial: double scratch [512]); all-reduce stats
 *   across ranks if the statistic must be global, then tarl_advantage_normalize applies
 *   A <- (A - mean) / max(std_unbiased, 1e-6). */
int tarl_advantage_stats(const float* advantage, int64_t n, double* partial, double* stats3, tarl_stream stream);
int tarl_advantage_normalize(float* advantage, int64_t n, const double* stats3, tarl_stream stream);
/* tarl_ppo_loss == ClipPPOLoss(clip_epsilon) forward + gradient seeds in one launch. out6 = {loss_objective,
 *   loss_critic, loss_entropy, clip_fraction, kl_approx, ESS}; grad_* [M] nullable: d(loss_objective + loss_critic +
 *   loss_entropy) / d(log_prob_new | entropy | value), multiplied by grad_scale (1/world_size for averaged DP grads). */
int tarl_ppo_loss(const float* log_prob_new, const float* log_prob_old, const float* advantage, const float* value,
                  const float* value_target, const float* entropy, int64_t M, float clip_epsilon, float entropy_coef,
                  float critic_coef, float grad_scale, float* out6, float* grad_log_prob, float* grad_entropy,
                  float* grad_value, tarl_stream stream);
/* tarl_adam_step == torch.optim.Adam single-tensor update (src/rl/ppo_trainer.py:37,144) on a flat fp32 buffer;
 *   step is 1-based; grad is multiplied by grad_scale first. */
int tarl_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                   double lr, double beta1, double beta2, double eps, float grad_scale, tarl_stream stream);

/* tarl_critic_mlp_fwd_splitk: the same network for FEW rows (the optimiser minibatch: 32 rows x N columns would
 *   otherwise be one MFMA tile walking all columns on one CU). The first layer is split over blocks of 64 input
 *   columns (partial sums in scratch, tarl_critic_splitk_scratch_floats(M, N) floats), added in block order by a second
 *   launch that finishes the network: deterministic; differs from tarl_critic_mlp_fwd only by the order of the fp32
 *   additions. Same arguments otherwise. */
int64_t tarl_critic_splitk_scratch_floats(int64_t M, int64_t N);
int tarl_critic_mlp_fwd_splitk(const float* counts, int64_t ldc, int64_t M, int64_t N, const float* time_rows,
                               int64_t rows_per_time, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* w3, const float* b3, float* scratch, float* value, float* h1_out,
                               float* h2_out, tarl_stream stream);

/* tarl_critic_mlp_fwd_slabs: same network on the env-minor rollout buffer counts [M / rows_per_slab][N][rows_per_slab]
 *   (= [frame][node][env]); rows_per_slab must be a multiple of 128 and M a whole number of slabs. value [M] is in
 *   (frame, env) order. */
int tarl_critic_mlp_fwd_slabs(const float* counts, int64_t rows_per_slab, int64_t M, int64_t N, const float* time_rows,
                              int64_t rows_per_time, const float* w1, const float* b1, const float* w2, const float* b2,
                              const float* w3, const float* b3, float* value, tarl_stream stream);

/* the same two forwards on the rollout buffers' count bytes (uint8 NUMBER_OF_AGENT, widened to fp32 in the LDS staging:
 *   identical values): tarl_critic_mlp_fwd_u8 reads counts uint8 [M][ldc] (the env-major buffer of tarl_rollout_env),
 *   tarl_critic_mlp_fwd_slabs_u8 counts uint8 [M / rows_per_slab][N][rows_per_slab] (the env-minor buffer of
 *   tarl_fused_rollout). With split_scratch (tarl_critic_split_scratch_bytes(N) bytes, 16-byte aligned) the first layer runs
 *   on the bf16 matrix cores at fp32 accuracy: the counts are exact in bf16 and W1 is split into three bf16 pieces with
 *   hi + mid + lo == W1 exactly, every product exact, fp32 accumulation (the value differs from the fp32 chain only by
 *   the order of the fp32 additions, ~1e-7 relative); NULL: fp32 MFMA on the widened bytes. */
int64_t tarl_critic_split_scratch_bytes(int64_t N);
int tarl_critic_mlp_fwd_u8(const uint8_t* counts, int64_t ldc, int64_t M, int64_t N, const float* time_rows,
                           int64_t rows_per_time, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, const float* b3, float* value, float* h1_out, float* h2_out,
                           tarl_stream stream);
int tarl_critic_mlp_fwd_slabs_u8(const uint8_t* counts, int64_t rows_per_slab, int64_t M, int64_t N,
                                 const float* time_rows, int64_t rows_per_time, const float* w1, const float* b1,
                                 const float* w2, const float* b2, const float* w3, const float* b3, void* split_scratch,
                                 float* value, tarl_stream stream);

/* ---- MPNNValueNet (src/agents/mpnn_agent.py:265-402; the message-passing critic the reference defines but never
 * instantiates) in evaluation mode (Dropout = identity), M samples:
 *   value[m] = W_f . [tanh(w_n * mean_{e=(u->v)} tanh(W_m . [node_features[m][v] (7), agent_rows[m][v] (9), edge_features[m][e]] + b_m) + b_n) for u, time_net(time[m])] + b_f
 * node_features [M][N][7]; agent_rows [M][N][9] = agent_features[agent_index] gathered by the caller (NULL: zeros);
 * edge_features [M][E] with stride ef_mstride (0 = shared); time [M].
 * params / grads: HOST arrays of 12 device pointers in the order message_mlp.1.{weight [17], bias}, node_mlp.0.{weight,
 * bias}, final_mlp.0.{weight [N+1], bias}, time_net.0.{weight [32], bias [32]}, time_net.3.{weight [32][32], bias [32]},
 * time_net.6.{weight [32], bias}. fwd optionally saves node_act / agg [M][N] (needed by bwd). bwd ACCUMULATES into grads. */
int tarl_value_mpnn_fwd(const tarl_plan* plan, const float* node_features, int64_t M, const float* agent_rows,
                        const float* edge_features, int64_t ef_mstride, const float* time, const float* const* params,
                        float* value, float* node_act, float* agg, tarl_stream stream);
int tarl_value_mpnn_bwd(const tarl_plan* plan, const float* node_features, int64_t M, const float* agent_rows,
                        const float* edge_features, int64_t ef_mstride, const float* time, const float* const* params,
                        const float* grad_value, const float* node_act, const float* agg, float* const* grads,
                        tarl_stream stream);

/* ---- fused rollout frame (vectorised fast path; same results as the entry points above, 3-4 launches per frame) --------
 * ENV-MINOR layout: every per-(node, environment) buffer is stored [node][environment], so that a wavefront holds 64
 * environments of one node: topology / table loads are wave-uniform and record gathers are coalesced.
 * Caller-owned side buffers that mirror x / agent_features (all device memory, 32-byte aligned). Packed words ("v11"):
 *   hdp  uint32 [N][B][2] = {head_id << 8 | NUMBER_OF_AGENT, bits of the head's departure time}
 *   tl   uint32 [N][B]    = tail_id << 8 | ring-buffer head offset << 1 | bit 0: gc8 is authoritative for the last frame
 *   post uint32 [N][B]    = state after the Direction update: tail' << 8 | non-empty' << 1 | arrived
 *   gc8  uint8  [N][B]    = pending-garbage count + 1; only WRITTEN, and only by rows where something moves in a frame
 *                           (ABI version 4; version 3 kept an 8-byte word {head arrival, code} here: the head's arrival
 *                           time is the arrival field of the head's slot record and is no longer stored twice)
 *   sel8 uint8  [N][B]    = SELECTED_ROAD as the rank of the chosen out-edge in the node's CSR list (bit 7: carried over
 *                           from the previous frame; 0x7F: the fp32 value in sel [N][B] is authoritative)
 *   static records built by pack and shared by all environments (read through the scalar cache): node_rec int32/fp32
 *   [N][36] = {CSC start, in-degree, CSR start, out-degree, MAX_NUMBER_OF_AGENT, FREE_FLOW, ROAD_INDEX, congestion_constant,
 *   travel time at count 0, 3 pad words, the target rows of the first four out-edges, the first four in_rec records};
 *   in_rec [E + 4][5] (CSC order) = {upstream row, the sel8 rank of that row which heads for this road (0xFE: none),
 *   edge_attr, MAX_NUMBER_OF_AGENT of the upstream row, edge id}; out_pad int32 [E + 4] (CSR order) = target row of each
 *   out-edge (sizes are checked against csrc/fused_common.h by static_assert; tarl_hip/ops.py:FusedState allocates them)
 *   st0  [N][4]    = {MAX_NUMBER_OF_AGENT, FREE_FLOW_TIME_TRAVEL, ROAD_INDEX, congestion_constant} (static, shared)
 *   slots [N][B][ld_slots]: slot-interleaved FIFO store, slot s at floats 3s..3s+2 = {agent id, arrival, departure};
 *                  ld_slots = tarl_fused_slot_floats(Nmax) (>= 3*Nmax, padded to a multiple of 16 floats)
 *   acc_lp int64 [acc_slots][B], acc_n / acc_w fp32 [acc_slots][B]: per-frame accumulator banks (log-prob in 2^-32 fixed
 *   point, sum of counts, agents withdrawn; zeroed by pack; acc_slots >= 1 banks spread the atomics of the many
 *   workgroups that serve one environment). Every call leaves all banks zero; acc_lp is filled, read and re-armed only
 *   by calls that are given a log_prob pointer)
 *   a_origin / a_dest int32 [B][A], a_dep fp32 [B][A], a_status uint8 [B][A] (0 waiting, 1 on the way, 2 done);
 *   a_order int32 [B][A] (optional, may be NULL): each environment's agent ids sorted by DEPARTURE_TIME — with it the
 *   insert kernel scans a window of that order from the cursor cur_lo int32 [B] instead of every agent every frame;
 *   a_dep_sorted fp32 [B][A] (required with a_order): DEPARTURE_TIME in that order, so the scan reads departures
 *   sequentially and touches the per-agent arrays only for the few entries that are due. With a_order also a_rank int32
 *   [B][A] (the inverse permutation: position of agent a in that order), a_win uint32 [B][A][4] and a_ins uint8 [B][A]
 *   (both filled by pack, in that order): the window record {departure bits, origin, agent id, 0} and the "already
 *   inserted" flag, so that one scan step is ONE pair of independent loads instead of a chain of four gathers.
 *   flags int32 [1]: sticky device status word (cleared by pack): TARL_FLAG_COUNT_AT_NMAX = a FIFO count reached Nmax
 *   (the reference raises IndexError there, src/direction_mpnn.py:172-191: the state is outside its defined domain),
 *   TARL_FLAG_AMBIGUOUS_EDGES = two out-edges of a node lead to the same ROAD_INDEX, TARL_FLAG_PACK_RANGE = a packed
 *   count above 255 / agent id at or above 2^24. The caller reads it at its next synchronisation point.
 * Domain of the fused path: Nmax <= 127, out-degree <= 126, agent ids < 2^24 (refused / flagged otherwise).
 * tarl_fused_pack imports x / agent_features (call after construction, reset, or any external write to x); between
 * pack and export the packed state is authoritative for the FIFO columns, NUMBER_OF_AGENT and SELECTED_ROAD;
 * tarl_fused_export writes them back into x in the reference's column layout, bit-identical to the unfused path.
 * agent_features is updated in place by every call. */
typedef struct tarl_fused {
  void* hdp;
  void* tl;
  uint8_t* gc8;
  void* post;
  float* st0;
  float* slots;
  int64_t ld_slots;
  uint8_t* sel8;
  float* sel;
  void* node_rec;
  void* in_rec;
  int32_t* out_pad;
  int64_t* acc_lp;
  float* acc_n;
  float* acc_w;
  int32_t* a_origin;
  int32_t* a_dest;
  float* a_dep;
  uint8_t* a_status;
  const int32_t* a_order;
  int32_t* cur_lo;
  const float* a_dep_sorted;
  void* a_win;
  uint8_t* a_ins;
  const int32_t* a_rank;
  int64_t acc_slots;
  int32_t* flags;
  /* GLOBAL id of environment 0 of this batch (default 0). The device noise streams — the action draws of the policy and the
   * Gumbel races of DirectionMPNN.aggregate — are Philox streams indexed by (env_base + b), not by the lane that happens to
   * serve b: a batch is a window into one global population of environments, so a shard of a larger batch (another
   * rank's slice in a data-parallel job, or a few environments run alone) reproduces, bit for bit, the trajectories those
   * environments have inside the larger batch. The reference has a single environment (env_base + b = 0). */
  int64_t env_base;
  /* hint, 0 = unknown: agents that become due per second and environment at the busiest time of the departure schedule
   * (DEPARTURE_TIME column, src/agents/base.py:244-262). The rollout launcher sizes the insert kernel's share of a wave
   * per environment by it (a frame of dt seconds brings ~due_rate * dt candidates). Never changes a result. */
  float due_rate;
  /* the policy hold rule of the state-dependent rollouts (tarl_fused_set_policy_hold below; 0 = off, the default — the word
   * was reserved and zero until the rule existed, so a caller that never heard of it has it off). Bit 0 is that rule; bit 1
   * (TARL_DEPARTURE_ROUTER) is the first-hop routing of tarl_fused_set_departure_router, whose arguments the library keeps
   * beside the handle: the struct itself does not grow. Bit 2 (TARL_TRIP_REWARD) is the trip reward of
   * tarl_fused_set_trip_reward, kept the same way; bit 3 (TARL_HEAD_CAPTURE) the head capture of
   * tarl_fused_set_head_capture, likewise. Each setter leaves the others' bits alone. */
  int32_t policy_hold;
  /* device scratch of tarl_fused_bufs_bytes() bytes, 16-byte aligned (required by the frame / rollout entry points): the
   * library keeps a device-resident copy of this table of pointers there (written by a one-thread launch at the head of every
   * such call, on the call's stream), and the row pass and the insert kernels read the pointers they need from it through the
   * scalar cache instead of carrying all of them as kernel arguments — 27 pointer arguments cost those kernels a dozen
   * scalar-register pairs each, most of them spilled (csrc/fused_pack.hip: k_set_bufs). */
  void* bufs_dev;
  /* int32 [B] or NULL, read ONLY while policy_hold != 0 (a caller with the shorter, earlier struct never sets that word):
   * += the rows held, per environment, by every frame of a state-dependent rollout (tarl_fused_set_policy_hold) */
  int32_t* policy_held;
} tarl_fused;

/* floats per (node, environment) row of tarl_fused.slots for FIFOs of Nmax slots */
int64_t tarl_fused_slot_floats(int32_t Nmax);
/* bytes of tarl_fused.bufs_dev */
int64_t tarl_fused_bufs_bytes(void);
int tarl_fused_pack(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                    int64_t ldx, int32_t Nmax, const float* congestion_constant, const float* edge_attr,
                    const float* agent_features, int64_t num_agents, int64_t a_bstride, tarl_stream stream);
/* tarl_fused_reset == tarl_reset_state applied to the packed state (SimulatorEnv._reset): empty every FIFO (count 0, row
 *   CLEAN: its slots are logically zero from here on, the store itself is not touched), zero the
 *   counters, keep SELECTED_ROAD, clear ON_WAY / DONE in agent_features (for the agents the status SoA marks as on the
 *   way / done, i.e. everything that changed since tarl_fused_pack) and the status SoA, re-arm the insert cursor. */
int tarl_fused_reset(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, float* agent_features,
                     int64_t num_agents, int64_t a_bstride, tarl_stream stream);
/* last_step_time: the clock value passed to the most recent tarl_fused_frame (stamps the pending garbage slots). */
int tarl_fused_export(const tarl_plan* plan, const tarl_fused* f, float* x, int64_t B, int64_t x_bstride, int64_t ldx,
                      int32_t Nmax, float last_step_time, tarl_stream stream);
/* The live policy (MPNNPolicyNet.forward: logits = emb[ROAD_INDEX(dst)]) does not read the dynamic state, so
 * GraphDistribution's probabilities are the same for every environment and frame between two optimiser steps.
 * tarl_fused_policy_prepare evaluates them once per parameter update — same arithmetic and reduction trees as
 * tarl_policy_edge_logits_fwd + tarl_graphdist_softmax + the cumsum of tarl_graphdist_sample +
 * tarl_graphdist_logprob_entropy_fwd — into per-edge tables in plan (CSR) order: thresholds [E] (fp32 inverse-CDF
 * thresholds), log_probs int64 [E] (log(p + 1e-8) in 2^-32 fixed point: the unit the frame kernels accumulate in),
 * entropy1 [1]; group_base: double scratch [num_groups + 1]. */
int tarl_fused_policy_prepare(const tarl_plan* plan, const tarl_fused* f, const float* emb, int64_t num_embeddings,
                              float temperature, double* group_base, float* thresholds, int64_t* log_probs,
                              float* entropy1, tarl_stream stream);
/* tarl_fused_frame == one collector frame for B environments: GraphDistribution.sample() + log_prob() (+ entropy) and
 *   the choice phase, then tarl_core_step + tarl_withdraw_step + tarl_insert_step, in four launches.
 *   uniform [B][num_groups] or NULL (Philox keyed by policy_seed / policy_counter); gumbel [B][E] or NULL (Philox keyed
 *   by seed / counter). prev_time: the clock of the previous frame on this state (an idle empty FIFO's head arrival, used
 *   by delta_travel_time only). Nullable outputs: delta_travel_time [B][E], popped / withdrawn uint8 [B][N] (env-major,
 *   like the unfused entry points); choice int32 [N][B] (chosen edge id, -1: none) and counts fp32 [N][B] (ENV-MINOR);
 *   log_prob, entropy, reward [B].
 *   thresholds == NULL skips the choice phase: SELECTED_ROAD is what tarl_fused_apply_choice (an externally sampled
 *   action, e.g. of a state-dependent policy) left; choice / log_prob / entropy must then be NULL.
 *   log_prob sums the same terms as tarl_graphdist_logprob_entropy_fwd, accumulated in 2^-32 fixed point (order-
 *   independent, hence deterministic): equal to fp32 rounding, not bit-identical. use_cong = 0 reproduces a graph without congestion_constant in insert. */
int tarl_fused_frame(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, const float* thresholds,
                     const int64_t* log_probs, const float* entropy1, const float* uniform, uint64_t policy_seed,
                     uint64_t policy_counter, float* agent_features, int64_t num_agents, int64_t a_bstride,
                     const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong, float time,
                     float prev_time, const float* gumbel, uint64_t seed, uint64_t counter, float* delta_travel_time,
                     uint8_t* popped, uint8_t* withdrawn, int32_t* ins_scratch, int32_t* choice, float* log_prob,
                     float* entropy, float* reward, float* counts, tarl_stream stream);
/* tarl_fused_apply_choice == the choice phase of SimulatorEnv._step (src/reinforcement_learning.py:223-231) on the packed
 *   state for an action sampled elsewhere: choice int32 [B][N] = chosen edge id per source node, -1 = none (the node keeps
 *   its SELECTED_ROAD). */
int tarl_fused_apply_choice(const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* choice,
                            tarl_stream stream);

/* tarl_fused_rollout == T consecutive tarl_fused_frame calls with device noise (uniform = gumbel = NULL), frame t at
 *   clock times_host[t] (HOST array of T floats; prev_time = the clock of the frame before the first, if any) with policy
 *   counter policy_counter0 + t and noise counter counter0 + t — the collector loop of ppo_train
 *   (src/rl/ppo_trainer.py:129-133) in one call, same results as the frame-by-frame calls.
 *   Outputs, each frame-major and nullable: choice uint8 [T][N][B] (the action: rank of the chosen out-edge in the source
 *   node's CSR list = tarl_plan order; bit 7 set: the node drew nothing — the action is infeasible there / the node has no
 *   out-edges), counts uint8 [T][N][B] (NUMBER_OF_AGENT after frame t; ENV-MINOR inside a frame), log_prob / entropy /
 *   reward fp32 [T][B].
 *   What SimulatorEnv._step logs per step (src/reinforcement_learning.py:278-294), device-side: leg int32 [T][B][2] =
 *   {agents departed, agents arrived} per frame (the leg histogram's series); for the first metrics_envs environments the
 *   per-node series dtt_node fp32 [T][N][metrics_envs] (delta_travel_time of the node's out-edges,
 *   src/direction_mpnn.py:94-96) and events uint8 [T][N][metrics_envs] (bit 0: Response pop, bit 1: withdraw — the masks
 *   of update_history / withdraw_history).
 *   Scratch (device): ins_scratch int32 [B][2A]; sel_scratch uint8 [N][B] (only used without a choice buffer);
 *   acc_scratch int64 [acc_slots][B]; choice_scratch int32 [tarl_fused_rollout_scratch_ints(plan, T, B)], 16-byte aligned,
 *   ZERO before its first use. Layout: draw-fixup list | policy records | per-node draw records | log-prob accumulators
 *   int64 [T][B] (last: no other offset depends on T, so one buffer sized for the longest rollout serves shorter ones).
 *   The library re-arms (zeroes) exactly the accumulators a call used; the record tables are rebuilt by every call.
 *   Scheduling of the GraphDistribution sample (state-independent for the live policy, so the T actions are T independent
 *   draws from one set of tables; same Philox streams and arithmetic in every mode, identical results):
 *     with a choice buffer and choice_scratch (default, TARL_ROLLOUT_MERGE=2) the whole action buffer is filled in blocks
 *     of 32 frames on a side stream, in the shadow of the latency-bound frame kernels, and each frame is three launches
 *     (Direction gather, row pass, insert); with acc_scratch and two distinct SELECTED_ROAD slices (TARL_ROLLOUT_MERGE=1)
 *     frame t+1's choice shares ONE launch with frame t's insert; otherwise (TARL_ROLLOUT_MERGE=0) a launch per frame. */
int64_t tarl_fused_rollout_scratch_ints(const tarl_plan* plan, int64_t T, int64_t B);
int tarl_fused_rollout(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                       const float* times_host, float prev_time, const float* thresholds, const int64_t* log_probs,
                       const float* entropy1, uint64_t policy_seed, uint64_t policy_counter0, float* agent_features,
                       int64_t num_agents, int64_t a_bstride, const float* edge_attr, const float* log_edge_attr,
                       float log_eps, int use_cong, uint64_t seed, uint64_t counter0, int32_t* ins_scratch,
                       uint8_t* sel_scratch, int64_t* acc_scratch, int32_t* choice_scratch, uint8_t* choice,
                       float* log_prob, float* entropy, float* reward, uint8_t* counts, int32_t metrics_envs,
                       float* dtt_node, uint8_t* events, int32_t* leg, tarl_stream stream);

/* x = cat(node_features, agent_features[head of the FIFO]) [B][N][16] of the packed state (see tarl_policy_obs16) */
int tarl_fused_obs16(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                     int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents, int64_t a_bstride,
                     float* obs16, tarl_stream stream);
/* tarl_fused_obs16_bf16: the same observation rounded to bf16 (RNE), uint16 [B][N][16] — the input of
 *   tarl_policy_edge_mlp_fwd(precision = 2) ("bf16 MPNN features": half the bytes written and gathered).
 * tarl_fused_obs16_rows: the fp32 observation of a FEW environments: row (env[j], i) -> obs_rows[slot[j]][i][16],
 *   j < rows (< 65536); env / slot int32 device arrays. */
int tarl_fused_obs16_bf16(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                          int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents, int64_t a_bstride,
                          uint16_t* obs16, tarl_stream stream);
int tarl_fused_obs16_rows(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                          int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents, int64_t a_bstride,
                          const int32_t* env, const int32_t* slot, int64_t rows, float* obs_rows, tarl_stream stream);

/* tarl_rollout_env == tarl_fused_rollout with the other mapping: ONE workgroup per environment keeps that environment's
 *   hot records and static columns in LDS (56 B per road + 16 KB; tarl_rollout_env_supported(plan) tells whether the
 *   graph fits the CU's 160 KB, i.e. up to ~2 600 roads) and runs all T frames inside a single launch, with workgroup barriers where the env-minor path has kernel
 *   boundaries. Same packed state in / out (tarl_fused), same noise streams, identical states / agents / actions /
 *   rewards / counts / log-probs. Differences at the interface: times_dev is a DEVICE array of T floats, and the
 *   per-frame outputs are ENV-MAJOR: choice uint8 [T][B][N], counts uint8 [T][B][N], dtt_node fp32 [T][metrics_envs][N],
 *   events uint8 [T][metrics_envs][N] (log_prob / entropy / reward [T][B], leg [T][B][2]).
 *   static_scratch: tarl_rollout_env_scratch_bytes(plan) bytes of 16-byte aligned device memory (the per-edge statics
 *   are packed into 16-byte records there by every call). */
int tarl_rollout_env_supported(const tarl_plan* plan);
int64_t tarl_rollout_env_scratch_bytes(const tarl_plan* plan);
int tarl_rollout_env(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                     const float* times_dev, float prev_time, const float* thresholds, const int64_t* log_probs,
                     const float* entropy1, uint64_t policy_seed, uint64_t policy_counter0, float* agent_features,
                     int64_t num_agents, int64_t a_bstride, const float* edge_attr, const float* log_edge_attr,
                     float log_eps, int use_cong, uint64_t seed, uint64_t counter0, int32_t* ins_scratch,
                     void* static_scratch, uint8_t* choice, float* log_prob, float* entropy, float* reward,
                     uint8_t* counts, int32_t metrics_envs, float* dtt_node, uint8_t* events, int32_t* leg,
                     tarl_stream stream);
/* tarl_fused_set_actions: load one frame's ENV-MAJOR action bytes (choice8 uint8 [B][N]: rank of the chosen out-edge in the
 *   road's CSR list, as tarl_graphdist_rollout / tarl_rollout_env / tarl_fused_rollout_policy write them) as the SELECTED_ROAD
 *   column of the packed state (tarl_fused.sel8, env-minor) — apply_action (src/transportation_simulator.py:411-414) for
 *   recorded or externally sampled actions, as 64 x 64 byte tiles turned through LDS. A byte with bit 7 set means "this road
 *   drew nothing": the road keeps its previous SELECTED_ROAD, and the completed code (previous rank | 0x80) is written back
 *   into choice8. */
int tarl_fused_set_actions(const tarl_plan* plan, const tarl_fused* f, int64_t B, uint8_t* choice8, tarl_stream stream);

/* tarl_fused_rollout_policy: T consecutive frames of SimulatorEnv._step under a STATE-DEPENDENT policy — the per-edge MLP
 *   head (MPNNPolicyNet.edge_mlp, src/agents/mpnn_agent.py:35-41, 227-231) — in one foreign call. Nothing of
 *   GraphDistribution can be hoisted out of the frame; per frame the call queues, on the caller's stream,
 *     tarl_fused_obs16 -> tarl_policy_edge_mlp_fwd(precision) -> tarl_graphdist_rollout(temperature; policy counter
 *     policy_counter0 + t; writes the action into tarl_fused.sel8) -> Direction gather -> row pass -> insert (noise counter
 *     counter0 + t),
 *   with the same results as those calls made one by one. x / x_bstride / ldx: the reference state tensor (static node
 *   columns of the observation). Minibatch observations: the (frame, environment) pairs an optimiser step will use are
 *   drawn BEFORE the rollout; keep_ptr_host (HOST int64 [T + 1], nullable) delimits, per frame, the entries of keep_env /
 *   keep_slot (device int32): observation row keep_env[j] of that frame is copied to obs_keep [slot][N][16].
 *   Scratch (device): obs_scratch fp32 [B][N][16] (16-byte aligned), logits_scratch fp32 [B][E], dist_scratch
 *   (tarl_graphdist_rollout_scratch_bytes), ins_scratch int32 [B][2A].
 *   Outputs, frame-major, nullable: choice8 uint8 [T][B][N] (ENV-MAJOR rank bytes, bit 7: nothing drawn), log_prob /
 *   reward fp32 [T][B], counts uint8 [T][N][B] (env-minor, after frame t), and the per-step logs of tarl_fused_rollout.
 *   precision (of the rollout's logits; the PPO update always evaluates the head with exact fp32 products): 0 = fp32 MFMA
 *   (tarl_policy_edge_mlp_fwd precision 0), 1 = bf16 MFMA on bf16 observations (its precision 2), 2 = fp32-accurate on the
 *   bf16 pipe (its precision 3: operands split into exact bf16 pieces). */
int tarl_fused_rollout_policy(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                              const float* times_host, float prev_time, const float* x, int64_t x_bstride, int64_t ldx,
                              float* agent_features, int64_t num_agents, int64_t a_bstride, const float* edge_attr,
                              const float* log_edge_attr, float log_eps, int use_cong, const float* w1, const float* b1,
                              const float* w2, const float* b2, const float* w3, const float* b3, int precision,
                              float temperature, uint64_t policy_seed, uint64_t policy_counter0, uint64_t seed,
                              uint64_t counter0, const int64_t* keep_ptr_host, const int32_t* keep_env,
                              const int32_t* keep_slot, float* obs_keep, float* obs_scratch, float* logits_scratch,
                              void* dist_scratch, int32_t* ins_scratch, uint8_t* choice8, float* log_prob, float* reward,
                              uint8_t* counts, int32_t metrics_envs, float* dtt_node, uint8_t* events, int32_t* leg,
                              tarl_stream stream);
/* ---- the shortest-path prior head of MPNNPolicyNet (policy_head = "embedding_dijkstra"; csrc/prior.hip) -------------------
 * The live forward of the reference computes a Dijkstra prior and leaves its addition commented out
 * (src/agents/mpnn_agent.py:180-190, compute_dijkstra_logits :81-113). This head adds it, weighted:
 *   logit[m][e] = emb[ROAD_INDEX(v)] + prior_weight * ((-dist[v][dest(u)]) - time_travel(v)),   u = src(e), v = dst(e),
 *   time_travel(v) = max(FF, FF * (MAXN + 10 - MAX_FLOW * FF / 3600) / (MAXN + 10 - NUMBER_OF_AGENT)) of road v (:181-184),
 *   dest(u) = (long) DESTINATION of u's head agent (:186-187; the head rule of tarl_policy_obs16 / tarl_fused_obs16).
 * fp32 in the reference's operation order; prior_weight = 1 is the reference's literal sum. ROAD_INDEX outside
 * [0, num_embeddings) contributes 0 (tarl_policy_edge_logits_fwd). dist [dist_n][dist_n] fp32 = MPNNPolicyNet.dist_matrix
 * (tarl_apsp on the free-flow weights), dist_n must equal the plan's N; prior_weight finite and >= 0.
 * Unreachable (dist = +inf, or dest outside [0, N)): the prior term is the finite sentinel -1e20 instead of -inf — such a
 * candidate has probability exactly 0 next to a reachable one, and a node whose every candidate is unreachable (NaN in the
 * reference) draws uniformly among its out-edges. No inf / NaN is emitted. Gradients w.r.t. emb: tarl_policy_edge_logits_bwd.
 * tarl_policy_prior_logits: from observations obs16 [M][N][16] (tarl_policy_obs16 layout, 16-byte aligned) -> logits [M][E].
 * tarl_fused_prior_logits: from the fused engine's packed state (count byte and head agent of every road) and the static
 *   columns of x -> logits [B][E], no observation written (the rollout's hot path). Same values as the observation path. */
int tarl_policy_prior_logits(const tarl_plan* plan, const float* obs16, int64_t M, const float* emb,
                             int64_t num_embeddings, const float* dist, int64_t dist_n, float prior_weight, float* logits,
                             tarl_stream stream);
int tarl_fused_prior_logits(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                            int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents, int64_t a_bstride,
                            const float* emb, int64_t num_embeddings, const float* dist, int64_t dist_n, float prior_weight,
                            float* logits, tarl_stream stream);
/* tarl_fused_rollout_prior: tarl_fused_rollout_policy with the prior head — T frames in one foreign call, per frame
 *   [tarl_fused_obs16_rows of the kept environments] -> tarl_fused_prior_logits -> tarl_graphdist_rollout (temperature;
 *   policy counter policy_counter0 + t; writes the action into tarl_fused.sel8) -> Direction gather -> row pass -> insert
 *   with that action (noise counter counter0 + t; the frame kernels write the count bytes), the loop of
 *   tarl_fused_rollout_policy with another head: arguments checked once per call, same results as tarl_fused_prior_logits,
 *   tarl_graphdist_rollout and tarl_fused_frame called one by one.
 *   keep_ptr_host / keep_env / keep_slot / obs_keep: as tarl_fused_rollout_policy (fp32 observations of the pre-drawn
 *   minibatch frames: what the PPO update needs to recompute the prior exactly). Scratch (device): logits_scratch fp32
 *   [B][E], dist_scratch (tarl_graphdist_rollout_scratch_bytes), ins_scratch int32 [B][2A]. Outputs, frame-major, nullable:
 *   choice8 uint8 [T][B][N] (ENV-MAJOR rank bytes, bit 7: nothing drawn), log_prob / reward fp32 [T][B], counts uint8
 *   [T][N][B] (env-minor, after frame t). The per-step logs of tarl_fused_rollout (leg, dtt_node, events) are not produced. */
int tarl_fused_rollout_prior(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                             const float* times_host, float prev_time, const float* x, int64_t x_bstride, int64_t ldx,
                             float* agent_features, int64_t num_agents, int64_t a_bstride, const float* edge_attr,
                             const float* log_edge_attr, float log_eps, int use_cong, const float* emb,
                             int64_t num_embeddings, const float* dist, int64_t dist_n, float prior_weight,
                             float temperature, uint64_t policy_seed, uint64_t policy_counter0, uint64_t seed,
                             uint64_t counter0, const int64_t* keep_ptr_host, const int32_t* keep_env,
                             const int32_t* keep_slot, float* obs_keep, float* logits_scratch, void* dist_scratch,
                             int32_t* ins_scratch, uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                             tarl_stream stream);
/* ---- the same prior from a per-destination table (MPNNPolicyNet.prior_method = "per_destination") -------------------------
 * The prior only reads dist[v][dest] for destinations some agent has: the N x N table of tarl_apsp is replaced by a
 * candidate-major [N][num_dests] fp32 table with one column per destination (csrc/dest_trees.hip, csrc/prior.hip).
 * tarl_prior_dest_table: table[u][j] = the fp32 rounding of tarl_dest_trees' fp64 distance u -> dests[j] (the distance
 *   phase alone: no next hops, no fp64 [num_dests][N] output); +inf where unreachable, 0 at the destination itself, a column
 *   of +inf for an out-of-range dests[j]. weights fp32 [E] in original edge order (the free-flow weights for the prior),
 *   dests int64 [num_dests] on the device. Where tarl_dest_trees' 28-bit condition holds on every path, each column equals
 *   tarl_apsp's dist[:, dests[j]] bit for bit. scratch: tarl_prior_dest_table_scratch_bytes(plan, num_dests) bytes of
 *   device memory (O(min(num_dests, 1024) x N)); -1 on a bad argument. Graphs up to N = 655 360 nodes.
 * tarl_policy_prior_logits_dest / tarl_fused_prior_logits_dest / tarl_fused_rollout_prior_dest: tarl_policy_prior_logits /
 *   tarl_fused_prior_logits / tarl_fused_rollout_prior with dist[v][dest] read as table[v][dest_slot[dest]]. table fp32
 *   [N][num_dests] (num_dests >= 1), dest_slot int32 [N]: the column of each destination, -1 = none. A destination outside
 *   [0, N), or one whose slot is -1 or outside [0, num_dests), is unreachable: its candidates get the sentinel -1e20, as
 *   an unreachable pair does. Every other argument, rule and output as the all-pairs entry points; on the same distances
 *   the logits, draws, log-probs and frames are bit-identical. */
int64_t tarl_prior_dest_table_scratch_bytes(const tarl_plan* plan, int64_t num_dests);
int tarl_prior_dest_table(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests,
                          void* scratch, int64_t scratch_bytes, float* table, tarl_stream stream);
int tarl_policy_prior_logits_dest(const tarl_plan* plan, const float* obs16, int64_t M, const float* emb,
                                  int64_t num_embeddings, const float* table, int64_t num_dests, const int32_t* dest_slot,
                                  float prior_weight, float* logits, tarl_stream stream);
int tarl_fused_prior_logits_dest(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                                 int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents,
                                 int64_t a_bstride, const float* emb, int64_t num_embeddings, const float* table,
                                 int64_t num_dests, const int32_t* dest_slot, float prior_weight, float* logits,
                                 tarl_stream stream);
int tarl_fused_rollout_prior_dest(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                  const float* times_host, float prev_time, const float* x, int64_t x_bstride, int64_t ldx,
                                  float* agent_features, int64_t num_agents, int64_t a_bstride, const float* edge_attr,
                                  const float* log_edge_attr, float log_eps, int use_cong, const float* emb,
                                  int64_t num_embeddings, const float* table, int64_t num_dests, const int32_t* dest_slot,
                                  float prior_weight, float temperature, uint64_t policy_seed, uint64_t policy_counter0,
                                  uint64_t seed, uint64_t counter0, const int64_t* keep_ptr_host, const int32_t* keep_env,
                                  const int32_t* keep_slot, float* obs_keep, float* logits_scratch, void* dist_scratch,
                                  int32_t* ins_scratch, uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts,
                                  tarl_stream stream);
/* ---- the graph-transformer head of MPNNPolicyNet (policy_head = "graph_transformer"; csrc/gt_policy.hip) ------------------
 * The edge output (raw=True) of GraphTransformerNet (src/transformer/model.py:140-178) as MLAgents builds it
 * (src/agents/transformer_agent.py:30-39: hidden 16, 4 heads, gate=True, 2 GTConv layers; node input 16 = obs16), in
 * evaluation mode: BatchNorm on running_mean / running_var (eps 1e-5), dropout = identity. GTConv: src/transformer/gt_conv.py:144-232
 * (attention softmax over the in-edges of the target as torch_geometric.utils.softmax: max subtracted, + 1e-16).
 * w: host array of TARL_GT_NUM_TENSORS device pointers, fp32 nn.Linear layouts: the TARL_GT_NUM_PARAMS trainable tensors that
 *   reach the logits, in this order (state-dict names of GraphTransformerNet):
 *     node_emb.weight, pe_emb.weight, edge_emb.weight,
 *     gt_layers.0.{WQ.weight, WK.weight, WV.weight, n_gate.weight, n_gate.bias, WO.weight, WO.bias, norm1.weight,
 *       norm1.bias, ffn.mlp.0.weight, ffn.mlp.0.bias, ffn.mlp.3.weight, ffn.mlp.3.bias, norm2.weight, norm2.bias},
 *     gt_layers.L.{WE.weight, WE.bias, WOe.weight, WOe.bias, norm1e.weight, norm1e.bias, ffn_e.mlp.0.weight,
 *       ffn_e.mlp.0.bias, ffn_e.mlp.3.weight, ffn_e.mlp.3.bias, norm2e.weight, norm2e.bias} for L = 0, then
 *     gt_layers.1.{WQ.weight, WK.weight}, the same twelve for L = 1, edge_linear.weight, edge_linear.bias;
 *   then the running statistics: gt_layers.0.{norm1, norm2, norm1e, norm2e}.{running_mean, running_var},
 *   gt_layers.1.{norm1e, norm2e}.{running_mean, running_var}. The rest of the module (gt_layers.1's node side, e_gate,
 *   mu_mlp, log_var_mlp) does not reach the logits (gt_conv.py:218-222 overwrites the e_gate product).
 * pe [N][16]: the positional encoding (Laplacian eigenvectors, transformer_agent.py:153-200), 16-byte aligned;
 * obs16 [M][N][16] as tarl_policy_obs16; edge_attr [E] (edge_dim_in = 1); logits [M][E], original edge order.
 * tarl_policy_gt_fwd: scratch fp32 of at least tarl_policy_gt_fwd_scratch_floats(plan, M), 16-byte aligned.
 * tarl_policy_gt_bwd ACCUMULATES (+=) the gradients of sum(grad_logits * logits) into grads (host array of
 *   TARL_GT_NUM_PARAMS device pointers, same order and shapes as w), the forward recomputed inside; scratch: at least
 *   tarl_policy_gt_bwd_scratch_floats(plan, M) floats. Deterministic: no atomics, per-node sums over in- / out-edges in
 *   CSC / CSR order, weight gradients summed over fixed chunks of items, then the chunks in order. */
#define TARL_GT_NUM_PARAMS 46
#define TARL_GT_NUM_TENSORS 58
int64_t tarl_policy_gt_fwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_policy_gt_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr, const float* pe,
                       const float* const* w, float* scratch, int64_t scratch_floats, float* logits, tarl_stream stream);
int64_t tarl_policy_gt_bwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_policy_gt_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr, const float* pe,
                       const float* const* w, const float* grad_logits, float* scratch, int64_t scratch_floats,
                       float* const* grads, tarl_stream stream);
/* tarl_fused_rollout_gt: tarl_fused_rollout_prior with the graph-transformer head — T frames in one foreign call, per frame
 *   [tarl_fused_obs16_rows of the kept environments] -> tarl_fused_obs16 (obs_scratch fp32 [B][N][16]) -> the forward above
 *   (gt_scratch: tarl_policy_gt_fwd_scratch_floats(plan, B) floats; the state-independent terms once per call) ->
 *   tarl_graphdist_rollout (temperature; policy counter policy_counter0 + t; writes tarl_fused.sel8) -> Direction gather ->
 *   row pass -> insert (noise counter counter0 + t; the frame kernels write the count bytes): the same loop again, same
 *   results as those calls and tarl_fused_frame made one by one. Other arguments and outputs as tarl_fused_rollout_prior. */
int tarl_fused_rollout_gt(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                          const float* times_host, float prev_time, const float* x, int64_t x_bstride, int64_t ldx,
                          float* agent_features, int64_t num_agents, int64_t a_bstride, const float* edge_attr,
                          const float* log_edge_attr, float log_eps, int use_cong, const float* pe, const float* const* w,
                          float temperature, uint64_t policy_seed, uint64_t policy_counter0, uint64_t seed,
                          uint64_t counter0, const int64_t* keep_ptr_host, const int32_t* keep_env,
                          const int32_t* keep_slot, float* obs_keep, float* obs_scratch, float* gt_scratch,
                          int64_t gt_scratch_floats, float* logits_scratch, void* dist_scratch, int32_t* ins_scratch,
                          uint8_t* choice8, float* log_prob, float* reward, uint8_t* counts, tarl_stream stream);
/* ---- the graph-transformer critic (value_head = "graph_transformer"; csrc/gt_value.hip) -------------------------------------
 * ValueNet(MLAgents) (src/agents/transformer_agent.py:257-323): value = mu_mlp(sum over all N nodes of x2) of a second
 * GraphTransformerNet (model.py:174-178, raw=True; hidden 16, 4 heads, gate=True, 2 GTConv layers; node input 16 = obs16),
 * evaluation mode as the policy head above. The node path never reads edge features (the score is (Q_i K_j).sum / sqrt(d_k),
 * gt_conv.py:222): edge_emb, WE, WOe, ffn_e, norm1e / norm2e, e_gate, edge_linear and log_var_mlp do not reach the value.
 * w: host array of TARL_GTV_NUM_TENSORS device pointers, fp32 nn.Linear layouts: the TARL_GTV_NUM_PARAMS trainable tensors
 *   that reach the value, in this order (state-dict names of GraphTransformerNet):
 *     node_emb.weight, pe_emb.weight,
 *     gt_layers.L.{WQ.weight, WK.weight, WV.weight, n_gate.weight, n_gate.bias, WO.weight, WO.bias, norm1.weight,
 *       norm1.bias, ffn.mlp.0.weight, ffn.mlp.0.bias, ffn.mlp.3.weight, ffn.mlp.3.bias, norm2.weight, norm2.bias} for L = 0, 1,
 *     mu_mlp.mlp.0.weight, mu_mlp.mlp.0.bias, mu_mlp.mlp.2.weight, mu_mlp.mlp.2.bias;
 *   then the running statistics gt_layers.L.{norm1, norm2}.{running_mean, running_var} for L = 0, 1.
 * pe [N][16]: the positional encoding; obs16 [M][N][16] as tarl_policy_obs16 (16-byte aligned); value [M].
 * tarl_value_gt_fwd: scratch fp32 of at least tarl_value_gt_fwd_scratch_floats(plan, M), 16-byte aligned.
 * tarl_value_gt_bwd ACCUMULATES (+=) the gradients of sum(grad_value * value) into grads (host array of TARL_GTV_NUM_PARAMS
 *   device pointers, same order and shapes as w), the forward recomputed inside; scratch: at least
 *   tarl_value_gt_bwd_scratch_floats(plan, M) floats; M at most tarl_value_gt_bwd_max_samples(plan) (one row of the weight
 *   gradients' grid per 1 024 (sample, node) items). Deterministic: no atomics, the node sum of the pooling in a fixed
 *   order, per-node sums over in- / out-edges in CSC / CSR order, weight gradients summed over fixed chunks of items, then
 *   the chunks in order. */
#define TARL_GTV_NUM_PARAMS 36
#define TARL_GTV_NUM_TENSORS 44
int64_t tarl_value_gt_fwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_value_gt_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe, const float* const* w,
                      float* scratch, int64_t scratch_floats, float* value, tarl_stream stream);
int64_t tarl_value_gt_bwd_max_samples(const tarl_plan* plan);
int64_t tarl_value_gt_bwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_value_gt_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe, const float* const* w,
                      const float* grad_value, float* scratch, int64_t scratch_floats, float* const* grads,
                      tarl_stream stream);
/* the action / count bytes of a rollout back in the formats of the unfused entry points: choice_eid int32 [rows][N] =
 *   chosen edge id (-1: none), counts_f fp32 [rows][N], for `rows` (frame, environment) pairs given as flat indices
 *   idx int64 [rows] = t * B + b (NULL: all T * B pairs in order). env_minor != 0: the buffers are [T][N][B], else
 *   [T][B][N]. Either output / input pair may be NULL. (The minibatch gather of ppo_train, src/rl/ppo_trainer.py:134.) */
int tarl_rollout_gather(const tarl_plan* plan, const uint8_t* choice, const uint8_t* counts, int64_t T, int64_t B,
                        int env_minor, const int64_t* idx, int64_t rows, int32_t* choice_eid, float* counts_f,
                        tarl_stream stream);

/* ---- shortest-path routing -----------------------------------------------------------------------
 * tarl_edge_travel_time == the edge weights of DijkstraAgents.choice (src/agents/base.py:541-550):
 *   travel_time[b][e] = max(FREE_FLOW[u], congestion_constant[v] / (MAX[u] + 10 - N[u])), u = src(e), v = dst(e),
 *   original edge order, fp32.
 * tarl_apsp == nx.all_pairs_dijkstra_path + the next-hop extraction of src/agents/base.py:556-570, and
 *   nx.shortest_path_length of MPNNPolicyNet.refresh_dijkstra (src/agents/mpnn_agent.py:53-79), for B weight sets
 *   (w_bstride = 0 shares one). Distances accumulate in double like networkx's Python floats; ties are broken exactly
 *   as networkx 3.x's heap does ((distance, push order), successors in edge order), so next_hop is reproducible.
 *   next_hop int64 [B][N][N]: first node after s on the path s -> t, s on the diagonal, -1 when unreachable.
 *   dist fp32 [B][N][N]: +inf when unreachable, 0 on the diagonal. Either output may be NULL.
 *   scratch: tarl_apsp_scratch_bytes(plan, B) bytes of device memory (0 => NULL is fine: state kept in LDS).
 *   The graph must be simple (no duplicate (u, v) edges: a DiGraph would merge them).
 * tarl_select_next_hop == src/agents/base.py:572-580: SELECTED_ROAD[i] = next_hop[i][DESTINATION[head agent of i]]
 *   for every row i (rows with an empty FIFO read agent 0). nh_bstride = 0 shares one table between environments. */
int tarl_edge_travel_time(const tarl_plan* plan, const float* x, int64_t B, int64_t x_bstride, int64_t ldx,
                          int32_t Nmax, const float* congestion_constant, float* travel_time, tarl_stream stream);
int64_t tarl_apsp_scratch_bytes(const tarl_plan* plan, int64_t B);
int tarl_apsp(const tarl_plan* plan, const float* weights, int64_t B, int64_t w_bstride, void* scratch,
              int64_t scratch_bytes, int64_t* next_hop, float* dist, tarl_stream stream);
/* tarl_apsp_f64: tarl_apsp with float64 edge weights (run_msa keeps its link costs in double).
 * tarl_msa_assign == the all-or-nothing step of run_msa (src/algorithms/user_equilibrium_msa.py:117-131): every OD pair
 *   p walks od_origin[p] -> od_dest[p] along next_hop [N][N] and adds od_volume[p] to aux_flow[v] (double, ACCUMULATED)
 *   for every node v entered with is_road[v] != 0 (the origin is skipped; unreachable pairs contribute nothing). */
int tarl_apsp_f64(const tarl_plan* plan, const double* weights, int64_t B, int64_t w_bstride, void* scratch,
                  int64_t scratch_bytes, int64_t* next_hop, float* dist, tarl_stream stream);
int tarl_msa_assign(const int64_t* next_hop, int64_t num_nodes, const int64_t* od_origin, const int64_t* od_dest,
                    const double* od_volume, int64_t num_pairs, const uint8_t* is_road, double* aux_flow,
                    tarl_stream stream);
int tarl_select_next_hop(float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax, int64_t num_nodes,
                         const float* agent_features, int64_t num_agents, int64_t a_bstride, const int64_t* next_hop,
                         int64_t nh_bstride, tarl_stream stream);

/* ---- per-origin shortest-path trees (MSA on large graphs) ------------------------------------------------------------------
 * The all-or-nothing step of run_msa (src/algorithms/user_equilibrium_msa.py:117-131) needs one shortest-path tree per
 * distinct origin of the demand, not an all-pairs table: O(E) work and O(N) state per tree (csrc/msa.hip).
 *   weights: float64 [E] in ORIGINAL edge order (run_msa passes cost[edge_index[1]]), non-negative (+inf allowed).
 *   dist[v] = the minimum over paths s -> v of the left-to-right fp64 sum ((0 + w1) + w2) + ... — the reference's
 *   Dijkstra (nx.shortest_path, src/algorithms/user_equilibrium_msa.py:121) bit for bit; +inf when unreachable.
 *   Tie rule of pred: among the TIGHT in-edges (fl(dist[u] + w) == dist[v]) take the fewest hops from s over tight edges,
 *   then the smallest predecessor node id. Independent of scheduling; hops strictly increase, so the tree is acyclic.
 *   scratch: tarl_msa_scratch_bytes(plan, num_sources) bytes of device memory (O(min(num_sources, 1024) x N)); -1 on a
 *   bad argument. Graphs up to N = 327 680 nodes (the LDS bitmaps). Source / OD ids live on the device: an
 *   out-of-range id writes nothing.
 * tarl_sssp_f64: dist_out float64 [num_sources][N], pred_out int32 [num_sources][N] (-1 for the source itself and for
 *   unreachable nodes); either may be NULL (then only the range check runs).
 * tarl_msa_assign_sssp == src/algorithms/user_equilibrium_msa.py:117-131 for OD pairs SORTED BY ORIGIN: the pairs of
 *   origins[j] are od_dest / od_volume [od_ptr[j], od_ptr[j+1]) (od_ptr int64 [num_origins + 1]); each walks d -> o along
 *   the tree and adds its volume to aux_flow[v] (double, ACCUMULATED) for every node v != o of the path with is_road[v] != 0,
 *   the semantics of tarl_msa_assign. */
int64_t tarl_msa_scratch_bytes(const tarl_plan* plan, int64_t num_sources);
int tarl_sssp_f64(const tarl_plan* plan, const double* weights, const int64_t* sources, int64_t num_sources, void* scratch,
                  int64_t scratch_bytes, double* dist_out, int32_t* pred_out, tarl_stream stream);
int tarl_msa_assign_sssp(const tarl_plan* plan, const double* weights, const int64_t* origins, int64_t num_origins,
                         const int64_t* od_ptr, const int64_t* od_dest, const double* od_volume, const uint8_t* is_road,
                         void* scratch, int64_t scratch_bytes, double* aux_flow, tarl_stream stream);

/* ---- equilibrium metrics: assignment with its gap, and the step between two assignments (src/algorithms/equilibrium.py) ------
 * Model of run_msa: entering road node v costs t_v(f) = ff_v (1 + 0.15 (f_v / max(cap_v, 1e-8))^4), other nodes cost 0. The
 * system optimum is the same problem on the marginal cost m_v(f) = d(f t_v)/df = ff_v (1 + 0.75 (f_v / cap_v)^4).
 * tarl_msa_assign_sssp_gap == tarl_msa_assign_sssp plus, out of the same launch and the same scratch row,
 *   sptt_part[j] = the sum over the OD pairs of origins[j], in pair order, of fl(volume * dist[dest]) for reachable
 *   destinations (the demand's shortest-path travel time at `weights`), and unrouted_part[j] = the volume of its pairs no
 *   path serves. float64 [num_origins], one thread each, no atomics: two calls give the same bits. Entries of out-of-range
 *   origins are not written (zero the arrays first).
 * tarl_msa_assign_gap == tarl_msa_assign that also reads node_cost float64 [num_nodes] and writes pair_cost float64
 *   [num_pairs]: ((0 + cost[v1]) + cost[v2]) + ... over the nodes entered on the walk (Dijkstra's own sum along that path),
 *   +inf for a pair without a path or with an id out of range. (tarl_apsp_f64's dist is fp32: not usable for this.)
 * tarl_bpr_step: everything between two all-or-nothing assignments, one launch, nothing read back by the host.
 *   flow f, aon_flow y, target_prev, free_flow, capacity float64 [num_nodes]; is_road uint8 [num_nodes]. cost = t (UE) or
 *   m (SO), H_v = d cost_v / df at f_v. iteration <= 1 (the first load; f is not a feasible flow yet): s = y, lambda = 1.
 *   Otherwise (i) the target: s = y for MSA and FW; for CFW s = a * target_prev + (1 - a) * y, a = Nn / Dn,
 *   Nn = sum (target_prev - f) H (y - f), Dn = sum (target_prev - f) H (y - target_prev); a = 0 when Dn == 0 or a is not
 *   positive, at most 0.99. (ii) the step: msa_step for MSA; else 1 when g(1) <= 0, else the root of
 *   g(l) = sum (s - f) cost(f + l (s - f)) on [0, 1] by bisection from [0, 1] (g < 0: the lower half is dropped) until the
 *   midpoint equals an end, at most 60 halvings; lambda = the last midpoint. (iii) in place f <- f + lambda (s - f),
 *   target_prev <- s; cost_out [num_nodes] = cost at the new f (0 off the roads: what the next assignment reads);
 *   record float64 [8] = {a, lambda, sum f t(f), sum f cost(f), g(0), g(1), halvings done, iteration}, sums at the new f.
 *   TARL_BPR_EVAL changes nothing and only writes cost_out and record[2], [3] for the f handed in (aon_flow and
 *   target_prev may be NULL). Every sum is a fixed-shape reduction inside one workgroup: same inputs, same bits. */
enum { TARL_BPR_UE = 0, TARL_BPR_SO = 1 };
enum { TARL_BPR_MSA = 0, TARL_BPR_FW = 1, TARL_BPR_CFW = 2, TARL_BPR_EVAL = 3 };
int tarl_msa_assign_sssp_gap(const tarl_plan* plan, const double* weights, const int64_t* origins, int64_t num_origins,
                             const int64_t* od_ptr, const int64_t* od_dest, const double* od_volume,
                             const uint8_t* is_road, void* scratch, int64_t scratch_bytes, double* aux_flow,
                             double* sptt_part, double* unrouted_part, tarl_stream stream);
int tarl_msa_assign_gap(const int64_t* next_hop, int64_t num_nodes, const int64_t* od_origin, const int64_t* od_dest,
                        const double* od_volume, int64_t num_pairs, const uint8_t* is_road, const double* node_cost,
                        double* aux_flow, double* pair_cost, tarl_stream stream);
int tarl_bpr_step(double* flow, const double* aon_flow, double* target_prev, const double* free_flow,
                  const double* capacity, const uint8_t* is_road, int64_t num_nodes, int objective, int rule,
                  double msa_step, int64_t iteration, double* cost_out, double* record, tarl_stream stream);

/* ---- per-destination shortest-path trees (the dijkstra agent on large graphs) ------------------------------------------------
 * DijkstraAgents.choice (src/agents/base.py:519-584) only reads next_hop[u][dest] for the destination of each row's head
 * agent: one reverse shortest-path tree per distinct destination replaces the N x N table of tarl_apsp (csrc/dest_trees.hip).
 * tarl_dest_trees == nx.all_pairs_dijkstra_path + the next-hop extraction of src/agents/base.py:556-570, restricted to
 *   the columns dests[0 .. num_dests):
 *   weights: fp32 [E] in ORIGINAL edge order (what tarl_edge_travel_time writes), non-negative (+inf allowed).
 *   dist_out float64 [num_dests][N]: dist[j][u] = the minimum over paths u -> dests[j] of the fp64 sum w1 + (w2 + (...));
 *   0 at the destination, +inf when unreachable. networkx sums left to right from u; both orders are exact, and the
 *   distances equal networkx's bit for bit, while on every path the exponent span of the weights (in bits) plus
 *   ceil(log2 hops) stays at or below 28.
 *   next_hop_out int32 [num_dests][N]: the successor of u on a TIGHT out-edge (fl(w(u,v) + dist[v]) == dist[u]); tie rule:
 *   the fewest hops to the destination over tight edges, then the smallest successor id. The destination itself holds
 *   its own id, unreachable nodes -1 (tarl_apsp's conventions). Either output may be NULL, not both.
 *   scratch: tarl_dest_trees_scratch_bytes(plan, num_dests) bytes of device memory (O(min(num_dests, 1024) x N)); -1 on a
 *   bad argument. Graphs up to N = 327 680 nodes (the LDS bitmaps). dests int64 [num_dests] live on the device: an
 *   out-of-range id writes nothing for its slot.
 * tarl_select_next_hop_dest == src/agents/base.py:572-580 on that table: SELECTED_ROAD[i] =
 *   next_hop[dest_slot[DESTINATION[head agent of i]]][i] for every row i, with tarl_select_next_hop's rules (rows with an
 *   empty FIFO read agent 0; an out-of-range head or destination leaves the row untouched). dest_slot int32 [num_nodes]:
 *   the row of next_hop [num_dests][num_nodes] holding each destination's tree, -1 = none (the row is left untouched).
 *   One table is shared by the B environments. */
int64_t tarl_dest_trees_scratch_bytes(const tarl_plan* plan, int64_t num_dests);
int tarl_dest_trees(const tarl_plan* plan, const float* weights, const int64_t* dests, int64_t num_dests, void* scratch,
                    int64_t scratch_bytes, int32_t* next_hop_out, double* dist_out, tarl_stream stream);
int tarl_select_next_hop_dest(float* x, int64_t B, int64_t x_bstride, int64_t ldx, int32_t Nmax, int64_t num_nodes,
                              const float* agent_features, int64_t num_agents, int64_t a_bstride, const int32_t* dest_slot,
                              const int32_t* next_hop, int64_t num_dests, tarl_stream stream);

/* ---- the shortest-path baseline on the packed state (vectorised evaluation of the dijkstra agent) -----------------------------
 * K environments that each route on their own congested travel times, on the fused path (csrc/baseline.hip,
 * csrc/dest_trees.hip). Every refresh: tarl_fused_edge_travel_time, then tarl_dest_trees_batched; every frame:
 * tarl_fused_select_next_hop_dest, then tarl_fused_frame with the action taken from the packed state.
 * tarl_fused_edge_travel_time == tarl_edge_travel_time on the packed state: travel_time fp32 [B][E], original edge order,
 *   max(FREE_FLOW[u], congestion_constant[v] / (MAX[u] + 10 - N[u])) from the count byte of tarl_fused.hdp and the static
 *   node records. Bit-identical to tarl_edge_travel_time on the x that tarl_fused_export writes.
 * tarl_dest_trees_batched == tarl_dest_trees for B weight sets: weights fp32 [B][E] with w_bstride floats between the sets
 *   (0 shares one set), next_hop_out int32 [B][num_dests][N]; slice [b] is tarl_dest_trees on weights[b] bit for bit (the
 *   same kernel, its workgroups striding over the B * num_dests pairs): distances, tie rule and conventions as above, an
 *   out-of-range destination writes nothing for its slots.
 *   scratch: tarl_dest_trees_batched_scratch_bytes(plan, B, num_dests) bytes (O(min(B * num_dests, 1024) x N)); -1 on a
 *   bad argument (B < 1, num_dests < 0).
 * tarl_fused_select_next_hop_dest == tarl_select_next_hop_dest on the packed state: for every row i and environment b the
 *   head id comes from tarl_fused.hdp, the destination from tarl_fused.a_dest [B][num_agents], the next hop from
 *   next_hop[b * nh_bstride + dest_slot[dest] * N + i] (nh_bstride in int32 elements; 0 shares one table). Written: the sel8
 *   code = the rank of the out-edge of i whose target is the next hop, or the raw code with the value in tarl_fused.sel when
 *   no out-edge of i matches (the destination itself, -1, a foreign entry): such a row moves nobody, as in the reference.
 *   tarl_select_next_hop_dest's rules hold: an empty FIFO reads agent 0; a head, destination or slot out of range leaves the
 *   row's previous selection untouched. After this call the SELECTED_ROAD column of tarl_fused_export equals, bit for bit,
 *   the column tarl_select_next_hop_dest writes into the exported x of the same state with environment b's table.
 *   choice8 (optional) uint8 [B][N]: the rows' sel8 bytes after the call, env-major.
 * tarl_fused_select_next_hop_hold: the same kernel, arguments and host checks with ONE rule added, and NOT
 *   DijkstraAgents.choice (src/agents/base.py:572-580): where the next hop read from the table equals the head agent's
 *   destination (integers compared, before the conversion to float) the row's own id i is written instead of the next hop.
 *   Why: in the environment's step order (SimulatorEnv._step, src/reinforcement_learning.py:222-309: choice, core,
 *   withdraw / insert, reward) the core moves a due agent from the last road before its destination onto the destination
 *   road, and the withdraw rule (Agents.withdraw_agent_from_network, src/agents/base.py:348-403: agents on a road ADJACENT
 *   to their destination whose departure there is due) never collects it. Held one road short, the agent is withdrawn as soon as it is due there. The own id, not -1: insert
 *   (Agents.insert_agent_into_network, src/agents/base.py:247-331) reads
 *   SELECTED_ROAD of an agent's origin row as the road to enter (a ready agent whose origin row holds enters the origin road
 *   itself), and -1 would index the last row in the reference's torch indexing. The row's own id matches no out-edge (the
 *   network builders make no self-loops; with one, a holding agent would take the loop — not handled), so the code is the
 *   raw one and the row moves nobody. On the destination road itself the table already holds i: nothing changes there. */
int tarl_fused_edge_travel_time(const tarl_plan* plan, const tarl_fused* f, int64_t B, float* travel_time,
                                tarl_stream stream);
int64_t tarl_dest_trees_batched_scratch_bytes(const tarl_plan* plan, int64_t B, int64_t num_dests);
int tarl_dest_trees_batched(const tarl_plan* plan, const float* weights, int64_t B, int64_t w_bstride, const int64_t* dests,
                            int64_t num_dests, void* scratch, int64_t scratch_bytes, int32_t* next_hop_out,
                            tarl_stream stream);
int tarl_fused_select_next_hop_dest(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                    const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride,
                                    int64_t num_dests, uint8_t* choice8, tarl_stream stream);
int tarl_fused_select_next_hop_hold(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                    const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride,
                                    int64_t num_dests, uint8_t* choice8, tarl_stream stream);

/* ---- per-road link counts of a vectorised evaluation ------------------------------------------------------------------------
 * The reference's compute_node_metrics / plot_daily_counts (src/transportation_simulator.py:563-746) concatenate the per-step
 * masks response_mpnn.update_history (roads whose head was popped) and agent.withdraw_history (roads with at least one agent
 * withdrawn), each stamped with the clock at which the step STARTED, bin them by time // 3600 and sum them.
 * tarl_link_counts_accumulate: counts int32 [B][H][N] += over the F frames f (clock_f = t0 + f * timestep, bin
 *   h_f = clock_f / bin_seconds - first_bin) of popped[f][b][n] + withdrawn[f][b][n]; popped / withdrawn uint8 [F][B][N], each
 *   slice as tarl_fused_frame wrote it (0 / 1; only bit 0 of a byte is read, so any other value stays memory-safe and cannot
 *   carry into a neighbour). One launch for all F frames, one writer per element, no atomics.
 *   1 <= F <= TARL_LINK_COUNTS_MAX_FRAMES (partial sums are packed 8 bits each and grow by at most 2 per frame). Refused on
 *   the host, before anything is launched: a first frame below first_bin, a last frame in a bin >= H, timestep < 0,
 *   bin_seconds < 1.
 * tarl_link_count_stats: over the K environments of counts_a int32 [K][H][N] — or, with counts_b (nullable, same shape), of
 *   the per-environment difference a - b (the paired form) — per (row, n), row < H a bin and row == H the episode total
 *   (the sum over the bins, per environment): sum and sumsq int64 [H + 1][N] (sum d, sum d^2), vmin and vmax int32
 *   [H + 1][N]. Integer arithmetic only; the caller keeps K * max|d|^2 below 2^63. */
#define TARL_LINK_COUNTS_MAX_FRAMES 127
int tarl_link_counts_accumulate(const uint8_t* popped, const uint8_t* withdrawn, int64_t F, int64_t B, int64_t N, int64_t t0,
                                int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t H, int32_t* counts,
                                tarl_stream stream);
int tarl_link_count_stats(const int32_t* counts_a, const int32_t* counts_b, int64_t K, int64_t H, int64_t N, int64_t* sum,
                          int64_t* sumsq, int32_t* vmin, int32_t* vmax, tarl_stream stream);

/* ---- per-road occupancy of a vectorised evaluation --------------------------------------------------------------------------
 * Sums over frames of NUMBER_OF_AGENT, the quantity the reward is made of (reward = -sum over n of NUMBER_OF_AGENT after the
 * step), binned like the link counts: frame f of a call starts at clock_f = t0 + f * timestep and belongs to bin
 * h_f = clock_f / bin_seconds - first_bin.
 * tarl_occupancy_accumulate: ring fp32 [F][N][K], F consecutive frames' `counts` slices exactly as tarl_fused_frame writes
 *   them (env-minor, the value AFTER the frame); thr int32 [N], the count from which a road admits nobody
 *   (ceil(MAX - 3): the negation of Direction's has_room and of the insert's capacity rule; a road with thr <= 0 is at
 *   capacity in every frame). With c = the ring's value converted by truncation, NaN or negative -> 0, above 255 -> 255 (a
 *   foreign value miscounts its own element and nothing else):
 *     veh  int32 [K][H][N] += sum over the frames f in bin h of c[f][n][k]        (vehicle-frames)
 *     full int32 [K][H][N] += the number of frames f in bin h with c[f][n][k] >= thr[n]
 *     peak int32 [K][1][N]  = max(peak, max over f of c[f][n][k])
 *   so a second call continues the first. The layouts are those of tarl_link_count_stats, which serves veh and full as they
 *   are (one- and two-input form) and peak with H = 1. One launch for all F frames; one workgroup owns a tile of 64
 *   environments x 64 roads for all frames and bins and is its only writer, no atomics.
 *   1 <= F <= 2^23: the partial sums of one call are int32 and 255 * 2^23 < 2^31 (no cap of 127 as for the link counts; the
 *   caller keeps the accumulated totals within int32, e.g. 255 * frames per bin). Refused on the host, before anything is
 *   launched and with the accumulators untouched: a null argument, a first frame below first_bin, a last frame in a bin
 *   >= H, timestep < 0, bin_seconds < 1, K, N, H, K * N * H or F * K * N at or above 2^40. */
int tarl_occupancy_accumulate(const float* ring, const int32_t* thr, int64_t F, int64_t K, int64_t N, int64_t t0,
                              int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t H, int32_t* veh,
                              int32_t* full, int32_t* peak, tarl_stream stream);

/* ---- per-turn movement counts of a vectorised evaluation -------------------------------------------------------------------
 * How many vehicles crossed each route edge e = (u -> v) (DirectionMPNN.aggregate chose e for v and the chosen agent id is
 * not 0: that agent enters v in this frame, src/direction_mpnn.py) and how many agents the U-turn double pop lost on which
 * road (an agent that moves from v into an EMPTY road u whose edge u -> v exists too is accepted on both edges by
 * ResponseMPNN, src/response_mpnn.py: u is popped although nothing left it, and the agent is gone), binned like the link
 * counts: frame f of a call starts at clock_f = t0 + f * timestep and belongs to bin h_f = clock_f / bin_seconds - first_bin.
 * tarl_turn_counts_accumulate: rings of F consecutive frames exactly as tarl_fused_frame leaves them: popped uint8
 *   [F][K][N] (env-major; only bit 0 of a byte is read), sel8 uint8 [F][N][K] (tarl_fused.sel8 AFTER frame f: the
 *   SELECTED_ROAD byte the frame ran with; bit 7 is ignored) and counts fp32 [F][N][K] (NUMBER_OF_AGENT after frame f), both
 *   env-minor; prev_counts fp32 [N][K] (nullable: every road empty, as after a reset) = the counts slice of the frame before
 *   the call's first. With n_pre = counts[f - 1] (prev_counts for f = 0) and N, E the plan's, for every (f, k, u) with
 *   popped[f][k][u] & 1:
 *     not n_pre[u][k] > 0 (0, -0.0, NaN)              -> lost  int32 [K][H][N]: lost[k][h_f][u] += 1
 *     else r = sel8[f][u][k] & 0x7F < out-degree(u)  -> turns int32 [K][H][E]: turns[k][h_f][e] += 1, e = the ORIGINAL edge
 *                                                       id of the r-th out-edge of u in the plan's CSR order
 *     else (0x7F, 0x7E, a rank >= the out-degree)     -> unresolved int32 [K]: unresolved[k] += 1
 *   so every popped bit lands in exactly one table and a second call continues the first. turns and lost have the layout
 *   of tarl_link_count_stats (its last axis is generic: pass E or N). One launch for all F frames; one thread owns an
 *   (environment, road) pair and is the only writer of its elements of turns and lost, no atomics there.
 *   1 <= F <= 2^23. Refused on the host, before anything is launched and with the tables untouched: a null argument
 *   (prev_counts excepted), a first frame below first_bin, a last frame in a bin >= H, timestep < 0, bin_seconds < 1, a plan
 *   without an edge, K, H, K * N * H, K * E * H or F * K * N at or above 2^40. */
int tarl_turn_counts_accumulate(const tarl_plan* plan, const uint8_t* popped, const uint8_t* sel8, const float* counts,
                                const float* prev_counts, int64_t F, int64_t K, int64_t t0, int64_t timestep,
                                int64_t bin_seconds, int64_t first_bin, int64_t H, int32_t* turns, int32_t* lost,
                                int32_t* unresolved, tarl_stream stream);

/* ---- per-trip report of a vectorised evaluation ------------------------------------------------------------------------------
 * What an episode leaves behind in the K agent tables, agents fp32 [K][A][9] with environment k at agents + k * a_bstride
 * (as tarl_episode_summary takes them; row 0, the dummy, is skipped). An agent has ARRIVED when DONE == 1; its travel time is
 * tt = ARRIVAL_TIME - DEPARTURE_TIME in fp32, widened to fp64 (so that sum tt agrees with tarl_episode_summary's sums); it is
 * ON THE WAY when it has not arrived and ON_WAY == 1. No floating-point atomics; every fp64 sum follows the fixed order
 * written at the top of csrc/trips.hip, which does not depend on a_bstride: two runs on one input are bit-identical.
 * tarl_trip_agent_stats: over the K environments, per agent; every output has A entries and entry 0 is written as zero.
 *   n_done, n_way int32: the environments in which the agent arrived / was on the way at the end; tt_sum, tt_sumsq fp64 over
 *   the environments in which it arrived; tt_min, tt_max fp32 (+inf / -inf where n_done == 0). agents_b (nullable; same K and
 *   A, its own b_bstride): the baseline run. Environment k is a usable pair for agent a when a arrived in BOTH runs; with
 *   d = (double)tt_a - (double)tt_b over the usable pairs: n_both int32, d_sum, d_sumsq fp64, n_faster (d < 0) and n_slower
 *   (d > 0) int32. The five paired outputs are required with agents_b and ignored (may be null) without it. ff (nullable)
 *   fp64 [A], a free-flow time per agent, and n_under int32 (both or neither): the environments in which the agent arrived
 *   with (double)tt < ff[a] (never for ff = +inf, which means none), which shows how good a yardstick ff is (it is a reference value, not a lower bound).
 * tarl_trip_bin_stats: over the agents, per (environment, time bin); every output is [K][H]. The bin of a clock value c is
 *   clamp((int64)floorf(c) / bin_seconds - first_bin, 0, H - 1) (a NaN or negative clock counts as 0, one from 2^62 on falls
 *   in the last bin). The departure of an agent is the same in every environment, so the caller sorts the agents by departure
 *   bin once per population: perm int32 [max(A - 1, 1)] lists the agents 1 .. A - 1 bin by bin (within a bin in the order in
 *   which their travel times are to be added) and seg int32 [H + 1] the start of every bin's segment in perm, seg[H] = A - 1.
 *   An entry of perm outside [1, A) is skipped and seg is clamped to [0, A - 1]: foreign values miscount, nothing is read or
 *   written out of bounds. dep_done, dep_way int32: the agents of departure bin h that arrived / are on the way at the end;
 *   dep_tt fp64: sum tt over the arrived agents of departure bin h; arr int32: the agents that arrived, binned by
 *   ARRIVAL_TIME (the arrivals curve of the leg histogram). ff (nullable) fp64 [A]: a free-flow time per agent, +inf = none;
 *   with it dep_ff fp64 = sum ff over the arrived agents of departure bin h with a finite ff and dep_ff_n int32 their number
 *   (both required with ff, ignored without it), so that the mean free-flow time by departure time, dep_ff / dep_ff_n, is taken
 *   over the right set (the mean delay is dep_tt / dep_done - dep_ff / dep_ff_n; the two sets are equal where every arrived
 *   agent has a finite ff).
 * Refused on the host, before anything is launched and with the outputs untouched: a null argument, K or A < 1 or >= 2^31,
 *   a_bstride < 9 A, bin_seconds < 1, first_bin < 0, H outside [1, TARL_TRIP_MAX_BINS], K * H >= 2^31. */
#define TARL_TRIP_MAX_BINS 4096
int tarl_trip_agent_stats(const float* agents, const float* agents_b, const double* ff, int64_t K, int64_t num_agents,
                          int64_t a_bstride, int64_t b_bstride, int32_t* n_under, int32_t* n_done, int32_t* n_way, double* tt_sum, double* tt_sumsq, float* tt_min,
                          float* tt_max, int32_t* n_both, double* d_sum, double* d_sumsq, int32_t* n_faster, int32_t* n_slower,
                          tarl_stream stream);
int tarl_trip_bin_stats(const float* agents, int64_t K, int64_t num_agents, int64_t a_bstride, const int32_t* perm,
                        const int32_t* seg, const double* ff, int64_t bin_seconds, int64_t first_bin, int64_t H,
                        int32_t* dep_done, int32_t* dep_way, int32_t* arr, double* dep_tt, double* dep_ff, int32_t* dep_ff_n,
                        tarl_stream stream);

/* ---- dynamic relative gap of a vectorised evaluation -----------------------------------------------------------------------------
 * How far the simulated trips are from the best path in hindsight under the time-dependent road times the episode itself
 * produced (csrc/td_paths.hip states every formula; all arithmetic fp64 unless said otherwise). Bins as tarl_trip_bin_stats:
 * bin h of H is the absolute bin first_bin + h of bin_seconds seconds, S(h) = (first_bin + h) * bin_seconds.
 * tarl_td_road_times: veh int32 [K][H][N] and frames_per_bin int32 [H] (the occupancy sums of tarl_occupancy_accumulate and
 *   the frames that fell into each bin), max_agents / free_flow / cong fp32 [N] (MAX_NUMBER_OF_AGENT, FREE_FLOW_TIME_TRAVEL and
 *   the congestion constant of every road) -> tau fp32 [K][H][N] = (float) max(FF, cong / ((MAX + 10) - veh / frames)), FF for a
 *   bin without frames and +inf for a denominator <= 0, and env fp64 [K][H + 1][N]: env[k][H][n] = +inf,
 *   env[k][h][n] = min(S(h) + tau[k][h][n], env[k][h + 1][n]). One thread per (k, n), every element written.
 * tarl_td_hindsight: per (environment k, agent a) of the agent tables (fp32 [K][A][9], environment k at agents + k *
 *   a_bstride) the earliest clock at which a left its destination road: with leave(n, t) = min(t + tau[k][h][n],
 *   env[k][h + 1][n]) at h = clamp((int64)floor(t) / bin_seconds - first_bin, 0, H - 1), L[origin] = leave(origin, DEPARTURE_TIME)
 *   and L[v] = min over in-edges (u -> v) of leave(v, L[u]), best[k][a] = L[destination]. best fp64 [K][A], every entry
 *   written: +inf for an unreachable destination, an id outside [0, N), the dummy row 0 and an agent with DONE != 1 (not
 *   searched). A NaN tau counts as +inf. One 256-thread workgroup per search over at most 1 024 workgroups, each with an fp64
 *   label row of N in `scratch` (tarl_td_hindsight_scratch_bytes(plan, K, A) bytes; -1 for a bad argument); the result does
 *   not depend on the schedule: two runs are bit-identical.
 * Refused on the host, before anything is launched and with the outputs untouched: a null argument, K, A or N < 1, K >= 65 536
 *   (road times) or 2^31, a_bstride < 9 A, bin_seconds < 1, first_bin < 0, H outside [1, TARL_TRIP_MAX_BINS], a graph beyond
 *   the limit of tarl_dest_trees (N > 327 680), a scratch smaller than tarl_td_hindsight_scratch_bytes. */
int tarl_td_road_times(const int32_t* veh, const int32_t* frames_per_bin, const float* max_agents, const float* free_flow,
                       const float* cong, int64_t K, int64_t H, int64_t N, int64_t bin_seconds, int64_t first_bin, float* tau,
                       double* env, tarl_stream stream);
int64_t tarl_td_hindsight_scratch_bytes(const tarl_plan* plan, int64_t K, int64_t num_agents);
int tarl_td_hindsight(const tarl_plan* plan, const float* tau, const double* env, const float* agents, int64_t K,
                      int64_t num_agents, int64_t a_bstride, int64_t bin_seconds, int64_t first_bin, int64_t H, void* scratch,
                      int64_t scratch_bytes, double* best, tarl_stream stream);

/* ---- day-to-day replanning: quickest routes per agent and the router that follows them ---------------------------------------
 * NOT reference semantics: the reference has no replanning loop, no search that returns a path and no router that reads a
 * plan per agent (tarl_hip/replanning.py holds the loop). TARL_ABI_VERSION is unchanged: nothing existing moved.
 * tarl_td_routes: tarl_td_hindsight's search (same tables, same leave(), same labels L) for EVERY agent a >= 1 whose origin and
 *   destination lie in [0, N), whatever its DONE flag, from its DEPARTURE_TIME; best fp64 [K][A] = L[destination]. After the
 *   labels have converged the path is walked back from the destination: at v != origin the in-neighbour u with
 *   leave(v, L[u]) == L[v] (fp64 equality), among several the SMALLEST ROAD ID whatever the order of the in-list. The route is
 *   stored forward, routes int32 [K][A][max_hops]: routes[k][a][0] = origin .. routes[k][a][len - 1] = destination with
 *   len = route_len[k][a] (int32 [K][A]); origin == destination gives len 1. len = 0 and best = +inf: an unreachable
 *   destination, the dummy row 0, an id out of range. len = -(true length): the route is longer than max_hops; the row's
 *   words are then left as allocated. (len = 0 with a finite best: no tight in-edge, and
 *   len = -1: more than N roads — neither occurs with tau >= FF > 0, where the labels fall strictly along the walk.) Every best
 *   and route_len entry is written; route words from len on are left as allocated. Launch shape as tarl_td_hindsight; each
 *   workgroup's scratch row holds the fp64 labels and, behind them, the walk's stack of max_hops road ids
 *   (tarl_td_routes_scratch_bytes; -1 for a bad argument); two runs are bit-identical.
 * Refused on the host, before anything is launched and with the outputs untouched: what tarl_td_hindsight refuses, and
 *   max_hops outside [1, 2^20].
 * tarl_fused_select_route: SELECTED_ROAD of every row of the packed state = the road that follows the row on its HEAD agent's
 *   route. The head decode (an empty row reads agent 0, a DIRTY row its slot), the rank code and the writes to sel8 / sel /
 *   choice8 are tarl_fused_select_next_hop_hold's. With r = routes[b][head] and len = route_len[b][head] — r_bstride ints between
 *   two environments' route tables (>= num_agents * max_hops; route_len is then dense [B][A]), or 0: one plan [A][max_hops] and
 *   [A] shared by all environments — a head outside [0, num_agents) or a len outside [1, max_hops] leaves the row untouched, and
 *   so does a row that is not on the route. Else with j the smallest index with r[j] == row: the row itself for j == len - 1
 *   (the destination), else r[j + 1], and the row itself where r[j + 1] == r[len - 1]: the hold rule, compared on the integers. */
int64_t tarl_td_routes_scratch_bytes(const tarl_plan* plan, int64_t K, int64_t num_agents, int64_t max_hops);
int tarl_td_routes(const tarl_plan* plan, const float* tau, const double* env, const float* agents, int64_t K,
                   int64_t num_agents, int64_t a_bstride, int64_t bin_seconds, int64_t first_bin, int64_t H, int64_t max_hops,
                   void* scratch, int64_t scratch_bytes, double* best, int32_t* routes, int32_t* route_len, tarl_stream stream);
int tarl_fused_select_route(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                            const int32_t* routes, const int32_t* route_len, int64_t r_bstride, int64_t max_hops,
                            uint8_t* choice8, tarl_stream stream);

/* ---- the hold rule on a POLICY's action (an action shield) -------------------------------------------------------
 * NOT reference semantics, off by default. The environment's step order (SimulatorEnv._step,
 * src/reinforcement_learning.py:222-309) is choice, core, withdraw / insert, reward, and the withdraw rule
 * (Agents.withdraw_agent_from_network, src/agents/base.py:334-403) collects an agent at the head of a road ADJACENT to its
 * destination once its departure there is due. The core runs first and moves that agent onto the road its row selected: a
 * policy that picks the destination road strands its agent on it, whatever it has learned. tarl_fused_select_next_hop_hold
 * fixes this for the routers; this is the same rule as a post-pass over the bytes ANY policy head has just written. The draw,
 * its log-prob and the PPO update are untouched. TARL_ABI_VERSION is unchanged: nothing existing moved.
 * tarl_fused_hold_policy_actions: for every row i and environment b of the packed state, on integers throughout: the row
 *   HOLDS when its FIFO is non-empty (count bits of tarl_fused.hdp != 0), its head agent h = hdp >> 8 lies in
 *   [0, num_agents), its sel8 byte is a rank c < 0x7F without the carried bit (bit 7) that names one of its out-edges, and
 *   that edge's target out_dst[out_ptr[i] + c] equals (int) DESTINATION of agent h in agent_features (fp32
 *   [B][num_agents][9], environment b at agent_features + b * a_bstride). A holding row gets sel8 = the raw code 0x7F and
 *   tarl_fused.sel = (float) i, tarl_fused_select_next_hop_hold's encoding: the core moves nobody from it and the insert puts
 *   a departing agent of that origin onto the origin road. Every other row keeps exactly what the policy wrote.
 *   ONE difference from the routers' rule: an EMPTY row is never touched — no dummy agent 0, no decode of a DIRTY row's slot
 *   store. The policy's action on an empty row is what the insert reads, and it stays the policy's.
 *   Not handled (as there): a self-loop. Not done, on purpose: a row adjacent to the destination that chose another road is
 *   not held, and an agent the insert places directly onto its destination road is not saved.
 *   choice8 (optional) uint8 [B][N]: the rows' sel8 bytes after the call, env-major, as the select kernels give them.
 *   held (optional) int32 [B]: += the rows held by this call (integer atomics).
 *   Host checks: tarl_fused_select_next_hop_dest's on plan, handle, B and Nmax; a null agent table, num_agents outside
 *   [1, 2^24] or (B > 1) a_bstride < 9 num_agents are refused, all before any HIP call.
 * tarl_fused_set_policy_hold: the switch for the T-frame rollouts of the state-dependent heads (tarl_fused_rollout_policy,
 *   tarl_fused_rollout_prior[_dest], tarl_fused_rollout_gt). With on = 1 their shared loop queues the launch above in every
 *   frame between the draw (tarl_graphdist_rollout) and the Direction launch, WITHOUT choice8 — the rollout's action buffer
 *   keeps the policy's draw, which the update needs — and with `held` (int32 [B], optional, caller-owned and caller-zeroed).
 *   With on = 0 (held must then be NULL) the loop queues exactly the launches it queued before the switch existed. Sets
 *   tarl_fused.policy_hold / policy_held; a null handle, on outside {0, 1} or a counter without the switch are refused. */
int tarl_fused_hold_policy_actions(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                   const float* agent_features, int64_t num_agents, int64_t a_bstride, uint8_t* choice8,
                                   int32_t* held, tarl_stream stream);
int tarl_fused_set_policy_hold(tarl_fused* f, int on, int32_t* held);

/* ---- first-hop routing: empty origin roads select for their departing agent ---------------------------------------
 * NOT reference semantics, off by default. The insert rule (Agents.insert_agent_into_network, src/agents/base.py:247-331) puts
 * a departing agent onto SELECTED_ROAD[origin]; every writer of that value decides for the row's HEAD agent and an empty row
 * reads the dummy agent 0, so the first hop of every trip heads for agent 0's destination. The rule, per environment b in
 * the frame whose clock is t, after the head (and the hold launch) has written SELECTED_ROAD and before Direction:
 *   agent a is READY as the insert has it: a_status == 0 && a_dep <= t (every row of the table, agent 0 included);
 *   pend(u) = the SMALLEST ready agent id with ORIGIN == u, -1 where there is none (the first one the insert admits);
 *   road u is ROUTED when its FIFO count (count bits of tarl_fused.hdp; a DIRTY empty row is empty) is 0 and pend(u) >= 0. A
 *   non-empty row keeps its head's choice. Every row that is not routed keeps sel8 / sel byte for byte.
 * tarl_fused_pending_departures: pend int32 [N][B], all N * B entries written. With the departure window (a_order, a_win,
 *   cur_lo, a_dep_sorted) the scan starts at cur_lo[b] and stops at the first entry that is not due; without a_order every
 *   agent is looked at. Both give the same table; integer atomics only, the result does not depend on scheduling. Reads the
 *   agent arrays alone: neither the cursor nor a_ins is touched. num_agents: the A of the handle's agent arrays, which the
 *   handle does not carry.
 * tarl_fused_route_departures: the TABLE lookup for every routed row, with p = pend(u) as the head: the chain of
 *   tarl_fused_select_next_hop_hold (d = a_dest[b][p] outside [0, N), slot = dest_slot[d] outside [0, num_dests): untouched;
 *   nh = next_hop[b or 0][slot][u]; nh == d -> u, the hold rule on integers), except that an unreachable destination
 *   (nh < 0) leaves the row untouched. Written as the select kernels write: the rank byte, sel where the code is 0x7F,
 *   choice8 (optional) uint8 [B][N] = the rows' bytes after the call, routed (optional) int32 [B] += the rows written.
 * tarl_fused_route_departures_plan: the same kernel with the PLAN lookup of tarl_fused_select_route (len check, the
 *   smallest j with r[j] == u, the destination row -> u, r[j + 1] == r[len - 1] -> u; no route or off the route: untouched).
 * tarl_fused_set_departure_router: the switch for the T-frame rollouts of the state-dependent heads. With on = 1 their shared
 *   loop queues tarl_fused_pending_departures into pend (int32 [N][B], caller-owned) and the table lookup (WITHOUT choice8,
 *   with routed: int32 [B], optional, caller-zeroed) in every frame, after the optional hold launch, with that frame's clock.
 *   With on = 0 (every pointer NULL) the loop queues exactly what it queued before. The tables must outlive the switch.
 * Host checks, all before any HIP call: null arguments, tarl_fused_select_next_hop_dest's on plan, handle, B and Nmax,
 *   num_agents outside [1, 2^24], a non-finite t, num_dests < 1, 0 < nh_bstride < num_dests * N or r_bstride < num_agents *
 *   max_hops (tables overlap), max_hops outside [1, 2^20], on outside {0, 1}, on without a table, a table without on. */
#define TARL_DEPARTURE_ROUTER 2
int tarl_fused_pending_departures(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                  float t, int32_t* pend, tarl_stream stream);
int tarl_fused_route_departures(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                const int32_t* pend, const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride,
                                int64_t num_dests, uint8_t* choice8, int32_t* routed, tarl_stream stream);
int tarl_fused_route_departures_plan(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                     const int32_t* pend, const int32_t* routes, const int32_t* route_len, int64_t r_bstride,
                                     int64_t max_hops, uint8_t* choice8, int32_t* routed, tarl_stream stream);
int tarl_fused_set_departure_router(tarl_fused* f, int on, const int32_t* dest_slot, const int32_t* next_hop,
                                    int64_t nh_bstride, int64_t num_dests, int32_t* pend, int32_t* routed);

/* ---- the trip reward: a lost agent is no longer free ------------------------------------------------------------------
 * NOT reference semantics, off by default. The reward the insert launch writes is -sum_rows NUMBER_OF_AGENT, the vehicles
 * standing in FIFOs after the frame: an agent lost to the U-turn double pop is queued nowhere and costs nothing
 * from then on, and an agent that is due but kept out by a full origin road costs nothing either. The trip reward counts the
 * travellers who should be under way and have not arrived. Per environment b, after the frame whose clock is t has run
 * completely (Direction, rows, withdraw, insert):
 *   on_way(b) = #{ a in [0, A) : a_status[b][a] == 1 }
 *   ready(b)  = #{ a in [0, A) : a_status[b][a] == 0 && a_dep[b][a] <= t }       (the insert's own test, the same fp32 compare)
 *   reward[b] = -(float)(on_way(b) + ready(b))                                    (exact: A <= 2^24)
 * Every row of the agent table counts, agent 0 included. With queued = -(the queue reward of the same frame):
 *   owed = queued + lost + ready,  lost = on_way - queued.
 * tarl_fused_trip_reward: reward fp32 [B] and parts int32 [B][2] = {on_way, ready} (optional), every element overwritten.
 *   on_way is one pass over the B * A status bytes by 16-byte loads (the unaligned head and tail bytes of every row one by
 *   one; nothing outside [b * A, (b + 1) * A) is read); ready is the walk of tarl_fused_pending_departures with the departure
 *   window (from cur_lo[b] while the sorted departure is <= t) and a test of a_dep beside the status byte without a_order.
 *   Both give the same numbers. Integer arithmetic and integer atomics only: the result does not depend on scheduling. Reads
 *   the agent arrays alone: neither the cursor nor a_ins nor any other word of the packed state is written. num_agents: the
 *   A of the handle's agent arrays.
 * tarl_fused_set_trip_reward: the switch for the T-frame rollouts of the state-dependent heads (bit TARL_TRIP_REWARD of
 *   tarl_fused.policy_hold). With on = 1 their shared loop queues tarl_fused_trip_reward in every frame after the insert
 *   launch, on the same stream, with that frame's clock, into reward + t * B (and parts + t * B * 2 where parts, int32
 *   [T_max][B][2], caller-owned, is given): the reward buffer of the rollout then holds the trip reward instead of the queue
 *   reward. A rollout without a reward buffer queues nothing. With on = 0 (parts NULL) the loop queues exactly what it queued
 *   before. Action bytes, log-probs and count bytes are the same either way.
 * Host checks, all before any HIP call (a refused call writes nothing): null plan, handle or reward,
 *   tarl_fused_select_next_hop_dest's on B and Nmax, num_agents outside [1, 2^24], a non-finite t, missing agent buffers,
 *   on outside {0, 1}, parts without on. */
#define TARL_TRIP_REWARD 4
int tarl_fused_trip_reward(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents, float t,
                           float* reward, int32_t* parts, tarl_stream stream);
int tarl_fused_set_trip_reward(tarl_fused* f, int on, int32_t* parts);

/* ---- behaviour cloning of the shortest-path router ----------------------------------------------------------------
 * NOT in the reference: a warm start for the learned heads. TARL_ABI_VERSION is unchanged: nothing existing moved.
 * tarl_fused_expert_labels: the expert's action of every row in the POLICY's action space, WITHOUT touching the packed state
 *   (sel8, sel and every other word stay as they are: a rollout driven by the policy can be labelled). For row i of
 *   environment b, labels[b][i] (uint8 [B][N], env-major) = the rank byte tarl_fused_select_next_hop_dest (hold off) would
 *   write for that row — same head decode, table lookup and rank search, out-lists longer than four included — and
 *   TARL_BC_IGNORE where the row is empty (count bits of hdp = 0; tested first, before any gather), where the head,
 *   destination or table slot is out of range (the select kernel leaves such a row untouched) and where the next hop matches
 *   no out-edge of i (the select kernel writes the raw code: the destination row itself, -1, a foreign entry).
 *   Taken before the hold: the destination road is named as a rank, and tarl_fused_hold_policy_actions turns exactly that
 *   pick into the hold. n_labelled (optional) int32 [B]: += the labelled rows of each environment (integer atomics, one
 *   instruction per wave). Arguments and host checks: tarl_fused_select_next_hop_dest's, and a null `labels` is refused.
 * tarl_graphdist_bc: cross-entropy of GraphDistribution(logits / temperature) on labelled nodes, forward and backward.
 *   logits fp32 [M][E] in original edge order; labels uint8 [M][N]. Node n of sample m is LABELLED when labels[m][n] <
 *   min(out-degree(n), 0x7F); every other byte is ignored. For a labelled node with out-edges e_0 .. e_{d-1} in the plan's
 *   CSR order, in fp32: z_j = logits[e_j] / temperature, mx = max z_j, s = sum_j exp(z_j - mx) left to right,
 *   loss = log s + mx - z_label. nll[m] (fp64) = the sum of the losses of sample m: per tile of 256 nodes a fixed tree
 *   (lanes l and l + 32, 16, .., 1 of each 64-node wave, then the tile's four waves in order), then the tiles in order.
 *   n_labelled[m], n_hit[m] (int32, overwritten): the labelled nodes, and those whose first maximum of z in CSR order is the
 *   label (tarl_graphdist_mode's tie rule). grad_logits (optional) fp32 [M][E], overwritten in full:
 *   (grad_scale * (exp(z_j - mx) / s - [j == label])) / temperature on the out-edges of a labelled node, 0 elsewhere.
 *   Deterministic (no floating-point atomics): two runs are bit-identical. scratch: tarl_graphdist_bc_scratch_bytes(plan, M)
 *   bytes, 8-byte aligned (16 per (sample, tile)); -1 for a null plan, M < 1 or 2^24 or more (sample, tile) pairs (the
 *   launch is one block of 256 threads per pair: below 2^32 threads), which tarl_graphdist_bc refuses too.
 *   Refused on the host, before any HIP call: a null argument (grad_logits alone may be null), M < 1, temperature <= 0, a
 *   misaligned scratch. A refused call leaves the outputs untouched. */
#define TARL_BC_IGNORE 0xFFu
int tarl_fused_expert_labels(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                             const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride, int64_t num_dests,
                             uint8_t* labels, int32_t* n_labelled, tarl_stream stream);
int64_t tarl_graphdist_bc_scratch_bytes(const tarl_plan* plan, int64_t M);
int tarl_graphdist_bc(const tarl_plan* plan, const float* logits, int64_t M, float temperature, const uint8_t* labels,
                      float grad_scale, double* nll, int32_t* n_labelled, int32_t* n_hit, float* grad_logits, void* scratch,
                      tarl_stream stream);

/* ---- the goal-conditioned policy head (policy_head = "goal_mlp"; csrc/goal_mlp.hip) ------------------------------
 * NOT in the reference: a trainable per-edge MLP 8 -> 16 -> 1 on destination-relative features, the head the cloned router
 * can be learned by. TARL_ABI_VERSION is unchanged: nothing existing moved. For a route edge e = (u -> v), in fp32 with IEEE
 * operations only (no FMA):
 *   d = (long) DESTINATION of u's head agent, read as the prior head reads it; D = table[v][d] through the prior's lookup
 *   (+inf: unreachable, d outside [0, N), no column); tt = the prior's time_travel(v); c = D + tt. e is REACHABLE when c is
 *   finite; cmin(u) = the exact minimum of c over u's reachable out-edges; S = time_scale.
 *   g0 = min((c - cmin) / S, 8) (8 when unreachable); g1 = [v == d]; g2 = min(tt / FF(v) - 1, 8), 0 unless FF(v) > 0;
 *   g3 = NUMBER_OF_AGENT(v) / MAXN(v), 0 where MAXN <= 0; g4 = the same of u; g5 = min(D / S, 64) / 8;
 *   g6 = [NUMBER_OF_AGENT(u) == 0]; g7 = min(FF(v) / S, 8).
 *   pre_j = b1[j] + sum_k W1[j][k] * g_k (k = 0..7 ascending, multiply then add); h_j = pre_j > 0 ? pre_j : 0;
 *   logit = b2 + sum_j w2[j] * h_j (j = 0..15 ascending). An unreachable edge's logit is exactly -1e20 (the prior head's
 *   sentinel and its consequences: probability 0 next to a reachable candidate, a uniform draw where all are unreachable).
 * weights / grads: 161 floats, W1 [16][8] at 0, b1 [16] at 128, w2 [16] at 144, b2 at 160.
 * table, table_cols, dest_slot: dest_slot == NULL -> table is the all-pairs [N][N] table and table_cols must equal N;
 *   otherwise table is the per-destination [N][table_cols] table of tarl_prior_dest_table and dest_slot int32 [N] its
 *   column map (-1: none). time_scale: finite and > 0 (the mean FREE_FLOW over the roads, computed by the host).
 * tarl_policy_goal_features: obs16 [M][N][16] (tarl_policy_obs16 layout, 16-byte aligned) -> feats fp32 [M][E][8] (16-byte
 *   aligned), original edge order; every element is written.
 * tarl_policy_goal_mlp_fwd: obs16 -> logits [M][E].
 * tarl_policy_goal_mlp_bwd ACCUMULATES (+=) the gradients of sum(grad_logits * logits) over the reachable (sample, edge)
 *   pairs into grads [161], as tarl_policy_edge_mlp_bwd does; an unreachable pair's grad_logits entry is not read.
 *   Features are recomputed from obs16. Deterministic: a fixed partition of the pairs over workgroups writes [partition][161]
 *   partial sums into scratch (fp32, 16-byte aligned, tarl_policy_goal_mlp_bwd_scratch_floats(plan, M) elements, every one
 *   written before it is read), a second kernel adds them in partition order; no floating-point atomics, two runs are
 *   bit-identical. The size query answers -1 for a null plan, M < 1 or 2^31 * 256 or more pairs, which the calls refuse too.
 * tarl_fused_goal_mlp_logits: the same logits from the fused engine's packed state -> logits [B][E], bit-identical to
 *   tarl_policy_goal_mlp_fwd on tarl_fused_obs16's observations of that state.
 * tarl_fused_rollout_goal: tarl_fused_rollout_prior with this head (per frame kept observation rows -> the logits launch ->
 *   the shared loop's sampler, hold rule, Direction, rows, insert); other arguments and outputs as there.
 * Refused on the host, before any HIP call: a null argument, M or B < 1, time_scale not finite or <= 0, table_cols not
 *   matching, a misaligned obs16 / feats / scratch, too many tiles for a grid dimension. A refused call writes nothing. */
int tarl_policy_goal_features(const tarl_plan* plan, const float* obs16, int64_t M, const float* table, int64_t table_cols,
                              const int32_t* dest_slot, float time_scale, float* feats, tarl_stream stream);
int tarl_policy_goal_mlp_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* table, int64_t table_cols,
                             const int32_t* dest_slot, float time_scale, const float* weights, float* logits,
                             tarl_stream stream);
int64_t tarl_policy_goal_mlp_bwd_scratch_floats(const tarl_plan* plan, int64_t M);
int tarl_policy_goal_mlp_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* table, int64_t table_cols,
                             const int32_t* dest_slot, float time_scale, const float* weights, const float* grad_logits,
                             float* grads, float* scratch, tarl_stream stream);
int tarl_fused_goal_mlp_logits(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                               int64_t ldx, int32_t Nmax, const float* agent_features, int64_t num_agents, int64_t a_bstride,
                               const float* table, int64_t table_cols, const int32_t* dest_slot, float time_scale,
                               const float* weights, float* logits, tarl_stream stream);
int tarl_fused_rollout_goal(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                            const float* times_host, float prev_time, const float* x, int64_t x_bstride, int64_t ldx,
                            float* agent_features, int64_t num_agents, int64_t a_bstride, const float* edge_attr,
                            const float* log_edge_attr, float log_eps, int use_cong, const float* table, int64_t table_cols,
                            const int32_t* dest_slot, float time_scale, const float* weights, float temperature,
                            uint64_t policy_seed, uint64_t policy_counter0, uint64_t seed, uint64_t counter0,
                            const int64_t* keep_ptr_host, const int32_t* keep_env, const int32_t* keep_slot, float* obs_keep,
                            float* logits_scratch, void* dist_scratch, int32_t* ins_scratch, uint8_t* choice8, float* log_prob,
                            float* reward, uint8_t* counts, tarl_stream stream);

/* ---- per-decision PPO credit (credit = "decision"; csrc/decision_credit.hip) -------------------------------------
 * NOT in the reference, off by default. TARL_ABI_VERSION is unchanged: nothing existing moved and tarl_fused did not grow.
 * Every road's categorical is credited with the delay of the traveller it decided for: the FIFO head of the packed state as
 * the frame before left it. wave64, no floating-point atomics: two runs are bit-identical.
 * tarl_fused_head_rows: head_keep[slot[j]][u] (int32, row length N) = the head id of road u in environment env[j]
 *   (hdp.x >> 8) where the count bits of hdp.x are not 0, and 0 otherwise, for j in [0, n). Reads hdp alone and writes
 *   nothing of the packed state; a pair whose environment is outside [0, B) gets a row of zeros. env / slot: int32 [n] on the
 *   device; the slots are the caller's (rows of head_keep).
 * tarl_fused_set_head_capture: the switch for the T-frame rollouts of the state-dependent heads (bit TARL_HEAD_CAPTURE of
 *   tarl_fused.policy_hold; head_keep is kept beside the handle and must outlive the switch). With on = 1 their shared loop
 *   queues tarl_fused_head_rows for the kept pairs of frame t in front of that frame's head call, on the same stream, with
 *   the slots of the observation keep list. With on = 0 (head_keep NULL) the loop queues exactly what it queued before.
 * tarl_decision_advantage: the raw advantage of `rows` kept rows of ONE episode segment, before the engine is reset (it reads
 *   the live agent table). Row j is frame[j], environment env[j], row slot[j] of head_keep / adv_raw (int32 [rows] each, on
 *   the device). A decision (row, road u) with a = head_keep[slot][u] is LIVE when a > 0, a < num_agents, u has an out-edge,
 *   d = (long) DESTINATION of agent a lies in [0, N), s = dest_slot[d] lies in [0, num_dests) and dist[s][u] (fp64
 *   [num_dests][N], tarl_dest_trees' distances) is finite. a >= num_agents adds 1 to bad[0]. For a live decision, in fp64:
 *   n = the number of frames k in [t, t_end) with times[k] < ARRIVAL_TIME (a lower-bound search of the clocks, times fp32
 *   [num_times] on the device) where DONE == 1, else n = t_end - t and truncated[0] += 1; S(n) = n for decision_gamma == 1
 *   and (1 - gamma^n) / (1 - gamma) otherwise; adv_raw = S(dist[s][u] / timestep) - S(n), rounded to fp32. adv_raw [.][N] is
 *   written for every road of every listed row (0 where the decision is not live) and head_keep is set to 0 where it is not
 *   live: head_keep > 0 is the live mask from then on. truncated / bad: int32 [1], integer atomics.
 * tarl_decision_stats: stats3 = {sum, sum of squares, count} of adv_raw over the `elems` elements with head_keep > 0: the
 *   layout and the two-stage fp64 scheme of tarl_advantage_stats (partial: 768 doubles of scratch), in a fixed order.
 * tarl_graphdist_node_logprob: lp_node[m][u] = log(p_choice + 1e-8) with p = softmax(logits / temperature) over u's
 *   out-edges in k_softmax's fp32 expressions (max subtracted, the sum left to right in CSR order); 0 where choice[m][u]
 *   (int32 [M][N], an edge id in original order or -1) names no out-edge of u. Every element is written.
 * tarl_graphdist_decision_ppo: the clipped objective on the live decisions (head[m][u] > 0 and a valid choice), in fp32:
 *   A = (adv_raw - mean) / max(std, 1e-6) from stats3 (tarl_advantage_normalize's rule, unbiased std), lp as above,
 *   r = exp(lp - lp_old_node), s = min(r A, clamp(r, 1 - eps, 1 + eps) A). out4 fp64 [M][4] = per sample {sum of s, live
 *   decisions, those with r outside [1 - eps, 1 + eps], sum of (lp_old - lp)}, a fixed tree per tile of 256 nodes and the
 *   tiles in order. grad_logits (optional) fp32 [M][E]: += on the out-edges e_j of a live node where the unclipped term is
 *   the minimum (a tie flows), -grad_scale / L * r A * (p_c / (p_c + 1e-8)) * ([j == c] - p_j) / temperature with L =
 *   n_live[0] (int32 on the device; nothing is added while L <= 0); every other element is left as it was. Every edge has one
 *   source node, so every element has one writer. scratch: tarl_graphdist_decision_ppo_scratch_bytes(plan, M) bytes, 8-byte
 *   aligned, every byte written before it is read; -1 for a null plan, M < 1 or 2^24 or more (sample, tile) pairs.
 * Refused on the host, before any HIP call (a refused call writes nothing): a null argument (grad_logits alone may be null;
 *   env / slot / head_keep of tarl_fused_head_rows only matter for n > 0), sizes below 1 or beyond the launch limits, N * B of
 *   2^31 or more, num_agents outside [1, 2^24], t_end outside [1, num_times], timestep <= 0, decision_gamma outside (0, 1],
 *   temperature <= 0, clip_epsilon outside [0, 1), a misaligned scratch, on outside {0, 1}, on without a buffer or a buffer
 *   without on. */
#define TARL_HEAD_CAPTURE 8
int tarl_fused_head_rows(const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* env, const int32_t* slot,
                         int64_t n, int32_t* head_keep, tarl_stream stream);
int tarl_fused_set_head_capture(tarl_fused* f, int on, int32_t* head_keep);
int tarl_decision_advantage(const tarl_plan* plan, int32_t* head_keep, const int32_t* frame, const int32_t* env,
                            const int32_t* slot, int64_t rows, int64_t B, const float* agent_features, int64_t num_agents,
                            int64_t a_bstride, const float* times, int64_t num_times, int64_t t_end, const double* dist,
                            const int32_t* dest_slot, int64_t num_dests, float timestep, double decision_gamma,
                            float* adv_raw, int32_t* truncated, int32_t* bad, tarl_stream stream);
int tarl_decision_stats(const float* adv_raw, const int32_t* head_keep, int64_t elems, double* partial, double* stats3,
                        tarl_stream stream);
int tarl_graphdist_node_logprob(const tarl_plan* plan, const float* logits, int64_t M, float temperature,
                                const int32_t* choice, float* lp_node, tarl_stream stream);
int64_t tarl_graphdist_decision_ppo_scratch_bytes(const tarl_plan* plan, int64_t M);
int tarl_graphdist_decision_ppo(const tarl_plan* plan, const float* logits, int64_t M, float temperature,
                                const int32_t* choice, const int32_t* head, const float* lp_old_node, const float* adv_raw,
                                const double* stats3, const int32_t* n_live, float clip_epsilon, float grad_scale,
                                double* out4, float* grad_logits, void* scratch, tarl_stream stream);

/* ---- credit scope "due" and the horizon bootstrap (csrc/decision_credit.hip) -------------------------------------
 * NOT in the reference, off by default. TARL_ABI_VERSION is unchanged: nothing existing moved and tarl_fused did not grow.
 * tarl_fused_head_rows_due: tarl_fused_head_rows on the whole 8-byte hdp word: head_keep[slot[j]][u] = the head id where the
 *   count bits of hdp.x are not 0 AND the fp32 value of hdp.y (the head's departure) is <= t_clock, the clock the frame is
 *   stepped with (Direction's own test); 0 elsewhere. The count is tested first: an empty road's hdp.y may be stale. A head
 *   that is due but blocked by a full target is in scope. counts2 (int32 [2] on the device, or NULL) += {roads with a head,
 *   roads with a due head} over the listed pairs, integer atomics. tarl_fused_head_rows' host checks, plus a finite t_clock.
 * tarl_fused_set_head_capture_scope: scope 0 = headed (tarl_fused_head_rows, what the loop queued before), 1 = due: the
 *   shared loop queues tarl_fused_head_rows_due with times_host[t] (all of them finite) and counts2 in its place. Refused
 *   unless the capture is on for the handle; tarl_fused_set_head_capture(f, 1, ..) starts from scope 0 and (f, 0, NULL) clears
 *   the scope. counts2 (nullable, scope 1 only) must outlive the switch.
 * tarl_fused_agent_roads: agent_road (int32 [B][A]) = -1 everywhere (an asynchronous fill on the stream), then u for every id
 *   in logical slots 0 .. count - 1 of road u's FIFO in environment b: count from hdp.x, the ring offset from tl, slot k at
 *   its physical place in slots. The slot at the count (the pending garbage triple) is never read. Written by an integer
 *   atomicMax: the result does not depend on scheduling. Ids outside [1, A), a ring offset >= Nmax and the part of a count
 *   above Nmax add to bad[0] (int32 on the device) and are not followed. Writes nothing of the packed state. The host checks
 *   of the frame entry points on (plan, f, B, Nmax), A in [1, 2^24], B * A < 2^31.
 * tarl_decision_advantage_boot: tarl_decision_advantage plus the horizon rule. bootstrap == 0: the same kernel, the same
 *   output bit for bit (agent_road / bootstrapped may be NULL). bootstrap == 1: a live decision whose traveller has DONE != 1
 *   when the segment ends, with r = agent_road[b][a] in [0, N) and dist[s][r] finite, gets n = (t_end - t) + dist[s][r] /
 *   timestep in fp64 (the free-flow time from the road it is queued on: an optimistic continuation) and adds to
 *   bootstrapped[0], not to truncated[0]; every other such decision (queued nowhere: lost; unreachable) is charged t_end - t
 *   and adds to truncated[0] as before. */
int tarl_fused_head_rows_due(const tarl_plan* plan, const tarl_fused* f, int64_t B, float t_clock, const int32_t* env,
                             const int32_t* slot, int64_t n, int32_t* head_keep, int32_t* counts2, tarl_stream stream);
int tarl_fused_set_head_capture_scope(tarl_fused* f, int scope, int32_t* counts2);
int tarl_fused_agent_roads(const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, int32_t Nmax,
                           int32_t* agent_road, int32_t* bad, tarl_stream stream);
int tarl_decision_advantage_boot(const tarl_plan* plan, int32_t* head_keep, const int32_t* frame, const int32_t* env,
                                 const int32_t* slot, int64_t rows, int64_t B, const float* agent_features,
                                 int64_t num_agents, int64_t a_bstride, const float* times, int64_t num_times, int64_t t_end,
                                 const double* dist, const int32_t* dest_slot, int64_t num_dests, float timestep,
                                 double decision_gamma, float* adv_raw, int32_t* truncated, int32_t* bad,
                                 const int32_t* agent_road, int bootstrap, int32_t* bootstrapped, tarl_stream stream);

/* ---- the learned per-decision critic (credit_baseline = "learned"; csrc/decision_critic.hip) ---------------------
 * NOT in the reference, off by default. TARL_ABI_VERSION is unchanged: nothing existing moved and tarl_fused did not grow.
 * A baseline of the per-decision advantage that reads the state in front of the decision and never the action. The common
 * inputs: obs16 fp32 [M][N][16] (the kept observations, 16-byte aligned), head int32 [M][N] (> 0: the decision is live, the
 * mask tarl_decision_advantage leaves), frames_left int32 [M] (t_end - t of the row's segment), dist fp64 [num_dests][N] and
 * dest_slot int32 [N] (the free-flow table of tarl_decision_advantage), timestep. For a live (m, u), with d = (long)
 * DESTINATION of obs16[m][u], s = dest_slot[d], n_ff(x) = dist[s][x] / timestep in fp64 (+inf where d lies outside [0, N) or
 * s outside [0, num_dests)), h = frames_left[m], fill(x) = NUMBER_OF_AGENT(x) / MAXN(x) (0 where MAXN <= 0) and v* the
 * out-neighbour of u with the smallest finite dist[s][v] (CSR order, the first wins a tie), eight fp32 features:
 *   f0 = (float)min(n_ff(u), 512) / 64, f1 = (float)min(h, 512) / 64, f2 = fill(u), f3 = fill(v*), f4 = the mean of fill(v)
 *   over the reachable out-neighbours (the sum in CSR order, one divide), f5 = [v* == d], f6 = [n_ff(u) > h] (fp64),
 *   f7 = min(FF(u) / timestep, 64) / 8; f3 = f4 = f5 = 0 where no neighbour is reachable.
 * The network is 8 -> 16 (ReLU) -> 1 in tarl_policy_goal_mlp_fwd's flat layout of 161 floats (W1 at 0, b1 at 128, w2 at
 * 144, b2 at 160), a multiply then an add, k and j ascending.
 * tarl_decision_critic_features: feats fp32 [M][N][8] (16-byte aligned), every element written, zeros where not live.
 * tarl_decision_critic_fwd: value[M][N] = the network's output, 0 where not live; adv_out (optional) = adv_raw +
 *   delay_scale * value in fp32 (a multiply, then an add), 0 where not live. The M * N elements of value, adv_out and
 *   adv_raw may not overlap (ranges are compared, not base pointers alone).
 * tarl_decision_critic_loss: the smooth-L1 loss of the value against y = -adv_raw / delay_scale over the live decisions,
 *   e = value - y, l = 0.5 e^2 for |e| < 1 and |e| - 0.5 otherwise. out5 fp64 [M][5] = per row {sum of l, live decisions,
 *   sum of y, sum of y^2, sum of (y - value)^2}, a fixed tree per tile of 256 nodes and the tiles in order. grads
 *   (optional) fp32 [161]: += the gradient of grad_scale * coef / L * sum of l with L = n_live[0] (int32 on the device;
 *   zeros are added while L <= 0). No floating-point atomics: the (row, tile) pairs are split into at most 1024 runs by M
 *   and N alone, the live decisions of a run are added in (row, node) order and the runs through a fixed tree (lane l of a
 *   wave takes the runs l, l + 64, .. in order, then lanes l and l + 32, 16, .., 1): two runs are bit-identical.
 *   scratch: tarl_decision_critic_loss_scratch_bytes(plan, M) bytes, 8-byte aligned, every byte written before it is read;
 *   -1 for a null plan, M < 1 or 2^24 or more (row, tile) pairs.
 * Refused on the host, before any HIP call (a refused call writes nothing): a null argument (adv_out and grads alone may be
 *   null), M or num_dests below 1, 2^24 or more (row, tile) pairs, timestep <= 0, delay_scale not finite or <= 0, coef < 0
 *   or not finite, a misaligned obs16 / feats / scratch, overlapping outputs. */
int tarl_decision_critic_features(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                                  const int32_t* frames_left, const double* dist, const int32_t* dest_slot,
                                  int64_t num_dests, float timestep, float* feats, tarl_stream stream);
int tarl_decision_critic_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                             const int32_t* frames_left, const double* dist, const int32_t* dest_slot, int64_t num_dests,
                             float timestep, const float* weights, float delay_scale, const float* adv_raw, float* value,
                             float* adv_out, tarl_stream stream);
int64_t tarl_decision_critic_loss_scratch_bytes(const tarl_plan* plan, int64_t M);
int tarl_decision_critic_loss(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                              const int32_t* frames_left, const double* dist, const int32_t* dest_slot, int64_t num_dests,
                              float timestep, const float* weights, float delay_scale, const float* adv_raw,
                              const int32_t* n_live, float coef, float grad_scale, double* out5, float* grads, void* scratch,
                              tarl_stream stream);

/* ---- the device noise, written out (test hook; nothing on the product path calls it) ---------------------------------------
 * The rollouts draw their own randomness: per frame one Gumbel value per in-edge for DirectionMPNN.aggregate's race (the
 * reference: torch.rand_like + -log(-log(u)), src/direction_mpnn.py:136-139) and one uniform per source node for
 * GraphDistribution.sample (src/reinforcement_learning.py:66) — Philox4x32-10 streams keyed by (seed, counter of the frame)
 * and indexed by the environment's GLOBAL id (tarl_fused.env_base + b). tarl_noise_export evaluates the same device
 * functions for the listed environments: kind 0 -> out [num_envs][E] fp32 Gumbel values in ORIGINAL edge order (the layout
 * of the `gumbel` argument of tarl_direction_step / tarl_fused_frame), for frame t of a rollout seed = its `seed`, counter =
 * its `counter0 + t`; kind 1 -> out [num_envs][G] uniforms of the action draw (seed = `policy_seed`, counter =
 * `policy_counter0 + t`; G = nodes with out-edges, in node order). env_ids: int64 [num_envs] global environment ids
 * (device). A CPU checker fed these values replays a device rollout bit for bit (tests/test_gpu_bench_geometry.py). */
int tarl_noise_export(const tarl_plan* plan, int kind, uint64_t seed, uint64_t counter, const int64_t* env_ids,
                      int64_t num_envs, float* out, tarl_stream stream);

/* ---- measurement hook (bench.py roofline leg; nothing comparable in the reference) ------------------------------------
 * tarl_prof_enable(n > 0) brackets the frame kernels of the next n fused frames (Direction message+aggregate, the row
 * pass, the insert [+ next frame's choice] launch) with HIP events on their launch stream; tarl_prof_enable(0) turns it
 * off. tarl_prof_collect synchronises those events and returns, per kernel slot k = 0 (Direction gather), 1 (row pass),
 * 2 (insert [+ choice]), the summed kernel time in ms over all timed frames (ms_all[3]) and over the timed frames with
 * index >= first_late_frame (ms_late[3]); frames[0], frames[1] = the number of frames behind each sum. */
int tarl_prof_enable(int64_t max_frames);
int tarl_prof_collect(int64_t first_late_frame, double* ms_all_host, double* ms_late_host, int64_t* frames_host);

/* ---- per-agent path trace of the vectorised evaluation (--eval-paths; csrc/path_trace.hip) -----------------------
 * NOT in the reference: which roads every (environment, agent) was seen on as a FIFO head, the free-flow cost of the hops
 * between them and how much of it was detour. TARL_ABI_VERSION is unchanged: nothing existing moved, tarl_fused did not grow.
 * State, caller-owned, per (environment b, agent a), row 0 the dummy and never touched by the pass:
 *   last_road, roads, revisits, off_tree int32 [B][A]; path_cost, excess fp64 [B][A]; route int32 [B][A][L] (NULL iff L == 0);
 *   bad int32 [B].
 * tarl_path_trace_reset: last_road = -1, route = -1, everything else 0 (not all zero: a memset does not do).
 * tarl_fused_path_trace: the SIGHTING PASS, one launch after a frame has run completely. READS the packed state (word 0 of
 *   tarl_fused.hdp, and tarl_fused.a_dest when weights are given) and writes nothing of it. For every road u and environment b
 *   whose count bits (hdp.x & 0x7F) are not 0, with a = hdp.x >> 8: a == 0 -> nothing; a >= num_agents -> bad[b] += 1;
 *   p = last_road[b][a], p == u -> nothing; else, h = roads[b][a]:
 *     p >= 0: e = the first entry of p's CSR out-list whose target is u; none -> bad[b] += 1, no cost. With weights:
 *       w = (double) weights[original edge id of e]; path_cost += w; s = dest_slot[a_dest[b][a]]; destination outside [0, N),
 *       s outside [0, num_dests) or dist[s][u] / dist[s][p] not finite -> off_tree += 1; else
 *       excess += (w + dist[s][u]) - dist[s][p], fp64, in this order.
 *     route[b][a][i] == u for some i < min(h, L) -> revisits += 1 (the kept prefix only); h < L -> route[b][a][h] = u;
 *     roads = h + 1; last_road = u.
 *   weights fp32 [E] (original edge order), dist fp64 [num_dests][N] and dest_slot int32 [N] (tarl_dest_trees) are optional
 *   AS A GROUP; without them path_cost, excess and off_tree stay as they are. With dist the distances under the same weights
 *   every term is a reduced cost: >= 0 up to rounding, exactly 0.0 on a hop of the tree the distances came from.
 *   Every (b, a) element has one writer per launch (an agent heads at most one non-empty road): no atomics, but the integer
 *   atomicAdd of bad[b], which must stay 0. A second launch on the same packed state changes nothing.
 * tarl_path_agent_stats: after the episode, per agent over the K environments, agents fp32 [K][A][9] (environment k at
 *   agents + k * a_bstride) for the DONE flag. out_i32 [8][A]: n_done, n_zero_excess (excess == 0 and off_tree == 0), n_loop
 *   (revisits > 0), n_trunc (roads > L) over the environments in which the agent is DONE; n_seen (roads > 0), n_loop_all,
 *   max roads over all; n_both. out_f64 [10][A]: sum and sum of squares of moves = max(roads - 1, 0), of path_cost and of
 *   excess over the DONE environments; with roads_b, excess_b, agents_b (b_bstride) of a second run — all three or none — of
 *   moves - moves_b and excess - excess_b over the environments DONE in both (rows 7 of out_i32 and 6..9 of out_f64, left alone
 *   without them). One thread per agent adds k = 0, 1, ... in order from +0.0: bit-identical from run to run. Entry 0 is zero.
 * Host checks, all before any HIP call (a refused call writes nothing): a null plan, handle, state pointer or output,
 *   tarl_fused_select_next_hop_dest's rules on B and Nmax, num_agents outside [1, 2^24], L outside [0, TARL_PATH_MAX_HOPS],
 *   route missing with L > 0, weights without dist or dest_slot and the reverse, sizes whose products overflow, agent tables
 *   that overlap. What they cannot see: num_agents must be the A the handle's agent buffers were allocated for —
 *   tarl_fused.a_dest is read as [b * num_agents + a], as tarl_fused_trip_reward reads the status bytes (ops.fused_path_trace
 *   passes the handle's own A and refuses a state of another shape). */
#define TARL_PATH_MAX_HOPS 4096
int tarl_path_trace_reset(int64_t B, int64_t num_agents, int64_t L, int32_t* last_road, int32_t* roads, int32_t* revisits,
                          int32_t* off_tree, double* path_cost, double* excess, int32_t* route, int32_t* bad,
                          tarl_stream stream);
int tarl_fused_path_trace(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents, int64_t L,
                          int32_t* last_road, int32_t* roads, int32_t* revisits, int32_t* off_tree, double* path_cost,
                          double* excess, int32_t* route, int32_t* bad, const float* weights, const double* dist,
                          const int32_t* dest_slot, int64_t num_dests, tarl_stream stream);
int tarl_path_agent_stats(const int32_t* roads, const int32_t* revisits, const int32_t* off_tree, const double* path_cost,
                          const double* excess, const float* agents, int64_t a_bstride, const int32_t* roads_b,
                          const double* excess_b, const float* agents_b, int64_t b_bstride, int64_t K, int64_t num_agents,
                          int64_t L, int32_t* out_i32, double* out_f64, tarl_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* TARL_HIP_H */
