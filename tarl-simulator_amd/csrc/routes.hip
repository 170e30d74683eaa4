// routes.hip — the router that follows a PER-AGENT route on the packed state (head "routes" of the vectorised evaluation, the
// day-to-day replanning loop of tarl_hip/replanning.py). NOT reference semantics: the reference has no
// replanning loop and no router that reads a plan per agent. The routes come from tarl_td_routes (td_paths.hip).
//
//   k_fused_select_route: SELECTED_ROAD of every row = the road that follows the row on its head agent's route, as the rank
//   byte sel8. The shape and the rules of k_fused_select_next_hop_dest<HOLD = true> (baseline.hip): one thread per (row i,
//   environment b), flat index i * B + b with the environment fastest, the head decode and the rank code of fused_select.h,
//   the same writes to sel8 / sel / choice8. Only the lookup in the middle differs. For the row's head agent, with
//   r = routes[b or 0][head] (int32 [max_hops]) and len = route_len[b or 0][head]:
//     head out of range, len <= 0 or len > max_hops      the row is left untouched (an agent without a route)
//     no j < len with r[j] == i                          the row is left untouched (an agent standing off its route)
//     j the smallest such index, j == len - 1            nh = i: the row is the destination
//     else nh = r[j + 1]; nh == r[len - 1]               nh = i: the HOLD rule of DESIGN 4.13a, compared on the integers before
//                                                        the conversion — held one road short of its destination the head is
//                                                        withdrawn as soon as it is due
//   The scan is a dependent, scattered read of up to len words per (row, environment): route_len is read first and a row
//   whose head has no route leaves before it touches the route. Must move per (row, environment): 8 B of hdp (4 used), 4 B of
//   route_len, the j + 2 words of the scan and 1 B stored. What the scan costs against the table lookup of the hold router
//   is measured, not guessed: profiles/replan_time.log.
#include "fused_select.h"

__global__ __launch_bounds__(FS_BLOCK) void k_fused_select_route(
    const uint2* __restrict__ hdp, const uint32_t* __restrict__ tl, const uint8_t* __restrict__ gc8,
    const float* __restrict__ slots, int64_t lds, int Nmax, const NodeRec* __restrict__ nodes,
    const int32_t* __restrict__ out_pad, int64_t A, uint32_t B, uint32_t NB, int64_t N, const int32_t* __restrict__ routes,
    const int32_t* __restrict__ route_len, int64_t r_bstride, int64_t len_bstride, int32_t max_hops,
    uint8_t* __restrict__ sel8, float* __restrict__ sel, uint8_t* __restrict__ choice8) {
  const uint32_t gid = blockIdx.x * FS_BLOCK + threadIdx.x;      // N * B < 2^31 (tarl_check_fused_core)
  if (gid >= NB) return;
  const uint32_t i = gid / B, b = gid - i * B;
  const long long head = fs_head_agent(hdp[gid].x, gid, tl, gc8, slots, lds, Nmax);
  bool write = false;
  uint32_t code = SEL_RAW;
  if (head >= 0 && head < A) {
    const int32_t len = route_len[(int64_t)b * len_bstride + head];
    if (len > 0 && len <= max_hops) {
      const int32_t* r = routes + (int64_t)b * r_bstride + head * (int64_t)max_hops;
      int32_t j = 0;
      while (j < len && r[j] != (int32_t)i) ++j;
      if (j < len) {
        int32_t nh = (int32_t)i;
        if (j < len - 1) {
          nh = r[j + 1];
          if (nh == r[len - 1]) nh = (int32_t)i;
        }
        const float sv = (float)nh;
        code = fs_rank_code(nodes[i], out_pad, sv);
        if (code == SEL_RAW) sel[gid] = sv;
        sel8[gid] = (uint8_t)code;
        write = true;
      }
    }
  }
  // env-major copy of the row's byte as it stands now (the evaluator's action record: a test hook, one scattered byte)
  if (choice8) choice8[(int64_t)b * N + i] = write ? (uint8_t)code : sel8[gid];
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int tarl_fused_select_route(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                       int64_t num_agents, const int32_t* routes, const int32_t* route_len, int64_t r_bstride,
                                       int64_t max_hops, uint8_t* choice8, tarl_stream stream) {
  TARL_REQUIRE(plan && f && routes && route_len, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(num_agents >= 1 && num_agents < ((int64_t)1 << 31), "bad sizes");
  TARL_REQUIRE(max_hops >= 1 && max_hops <= ((int64_t)1 << 20), "max_hops must be in [1, 2^20]");
  TARL_REQUIRE(r_bstride == 0 || r_bstride >= num_agents * max_hops, "route tables overlap");
  if (plan->N == 0) return TARL_OK;
  const int64_t NB = plan->N * B;
  hipLaunchKernelGGL(k_fused_select_route, dim3((unsigned)ceil_div(NB, FS_BLOCK)), dim3(FS_BLOCK), 0, (hipStream_t)stream,
                     (const uint2*)f->hdp, (const uint32_t*)f->tl, (const uint8_t*)f->gc8, (const float*)f->slots,
                     f->ld_slots, (int)Nmax, (const NodeRec*)f->node_rec, (const int32_t*)f->out_pad, num_agents,
                     (uint32_t)B, (uint32_t)NB, plan->N, routes, route_len, r_bstride, r_bstride ? num_agents : (int64_t)0,
                     (int32_t)max_hops, f->sel8, f->sel, choice8);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
