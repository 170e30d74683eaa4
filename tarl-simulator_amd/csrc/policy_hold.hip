// policy_hold.hip — the HOLD rule of DESIGN 4.13a applied to the action a POLICY head has just written: an
// environment-side rule (an action shield), off by default and NOT in the reference. The policy's draw, its log-prob and the
// PPO update never see it: it rewrites the SELECTED_ROAD bytes of the packed state between the draw and the Direction launch.
//
// Why: the environment's step order (SimulatorEnv._step, src/reinforcement_learning.py:222-309) is choice, core, withdraw /
// insert, reward, and the withdraw rule (Agents.withdraw_agent_from_network, src/agents/base.py:334-403) collects an agent at
// the head of a road ADJACENT to its destination once its departure there is due. The core runs first and moves that agent
// onto the road its row selected: a policy that picks the destination road strands its agent on it. Held one road short, the
// agent is withdrawn as soon as it is due.
//
//   k_fused_hold_policy_actions: one thread per (row i, environment b), flat index gid = i * B + b with the environment
//   fastest — the shape of the select kernels (fused_select.h): the [N][B] words are read and written coalesced and for
//   B >= 64 the node record is uniform over the wave. Every condition is made on integers. The row HOLDS when
//     its FIFO is non-empty (count bits of hdp != 0),
//     its head agent h = hdp >> 8 lies in [0, A),
//     its byte is a rank c < SEL_RAW without SEL_CARRIED (and c < the row's out-degree: a rank names an out-edge),
//     the target v = out_dst[out_ptr[i] + c] equals d = (int) DESTINATION of agent h in environment b.
//   A holding row gets sel8 = SEL_RAW and sel = (float) i, the encoding of k_fused_select_next_hop_dest<HOLD>: the core moves
//   nobody from it and the insert puts a departing agent of that origin onto the origin road. Every other row keeps exactly
//   what the policy wrote.
//   THE ONE DIFFERENCE from the routers' select kernels: an EMPTY row is never touched. There is no dummy agent 0 and no
//   decode of a DIRTY row's slot store (fs_head_agent is not used): the policy's action on an empty row is what the insert
//   reads, and it stays the policy's. The test comes first, before the agent gather: on a sparsely loaded network most
//   lanes stop after one 4-byte load.
//   Not handled, as in 4.13a: a self-loop (the builders make none; a holding head would take it). Not done, on purpose: a row
//   adjacent to d that chose ANOTHER road is not held (the policy keeps its say), and an agent the insert places directly
//   onto its destination road is not saved.
//   Must move per (row, environment): 8 B of hdp (4 used); on occupied rows 1 B of sel8, the node record (uniform, cached),
//   one 4-byte agent gather and, where the row holds, 1 + 4 B stored and one integer atomic. Plain vector stores, no LDS, no
//   floating-point atomics.
#include "fused_select.h"
#include "rollout_heads.h"

__global__ __launch_bounds__(FS_BLOCK) void k_fused_hold_policy_actions(
    const uint2* __restrict__ hdp, const NodeRec* __restrict__ nodes, const int32_t* __restrict__ out_pad,
    const float* __restrict__ agents, int64_t A, int64_t a_bstride, uint32_t B, uint32_t NB, int64_t N,
    uint8_t* __restrict__ sel8, float* __restrict__ sel, uint8_t* __restrict__ choice8, int32_t* __restrict__ held) {
  const uint32_t gid = blockIdx.x * FS_BLOCK + threadIdx.x;      // N * B < 2^31 (tarl_check_fused_core)
  if (gid >= NB) return;
  const uint32_t i = gid / B, b = gid - i * B;
  const uint32_t hd = hdp[gid].x;
  bool hold = false;
  if ((hd & HD_CNT) != 0u) {                                      // an empty row: the policy's byte stays, nothing else is read
    const uint32_t c = sel8[gid];
    const int64_t h = (int64_t)(hd >> 8);
    if (c < SEL_RAW && h < A) {                                   // (c >= SEL_RAW: the raw code, or SEL_CARRIED set)
      const NodeRec& nr = nodes[i];
      if ((int32_t)c < nr.out_deg) {
        const int32_t v = c < 4u ? nr.out4[c] : out_pad[nr.out0 + (int32_t)c];
        const int32_t d = (int32_t)agents[(int64_t)b * a_bstride + h * AG_COLS + AG_DEST];
        hold = v == d;
      }
    }
  }
  if (hold) {
    sel8[gid] = (uint8_t)SEL_RAW;
    sel[gid] = (float)i;
    if (held) atomicAdd(held + b, 1);
  }
  // env-major copy of the row's byte as it stands now (the select kernels' test hook, one scattered byte)
  if (choice8) choice8[(int64_t)b * N + i] = hold ? (uint8_t)SEL_RAW : sel8[gid];
}

// the launch alone: the caller has checked the handle (tarl_check_fused_core) and the agent table
int tarl_launch_policy_hold(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, const float* agent_features,
                            int64_t A, int64_t a_bstride, uint8_t* choice8, int32_t* held) {
  const int64_t NB = plan->N * B;
  hipLaunchKernelGGL(k_fused_hold_policy_actions, dim3((unsigned)ceil_div(NB, FS_BLOCK)), dim3(FS_BLOCK), 0, s,
                     (const uint2*)f->hdp, (const NodeRec*)f->node_rec, (const int32_t*)f->out_pad, agent_features, A,
                     a_bstride, (uint32_t)B, (uint32_t)NB, plan->N, f->sel8, f->sel, choice8, held);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int tarl_fused_hold_policy_actions(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                              const float* agent_features, int64_t num_agents, int64_t a_bstride,
                                              uint8_t* choice8, int32_t* held, tarl_stream stream) {
  TARL_REQUIRE(plan && f && agent_features, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(num_agents >= 1 && num_agents <= ((int64_t)1 << 24), "bad sizes");
  TARL_REQUIRE(B == 1 || a_bstride >= num_agents * AG_COLS, "agent stride smaller than one population");
  if (plan->N == 0) return TARL_OK;
  return tarl_launch_policy_hold((hipStream_t)stream, plan, f, B, agent_features, num_agents, a_bstride, choice8, held);
}

extern "C" int tarl_fused_set_policy_hold(tarl_fused* f, int on, int32_t* held) {
  TARL_REQUIRE(f, "null argument");
  TARL_REQUIRE(on == 0 || on == 1, "on must be 0 or 1");
  TARL_REQUIRE(on || !held, "a held counter without the switch");
  f->policy_hold = (f->policy_hold & ~1) | on;      // (the other bits belong to their own setters)
  f->policy_held = held;
  return TARL_OK;
}
