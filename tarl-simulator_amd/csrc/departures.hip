// departures.hip — FIRST-HOP routing: an EMPTY origin road selects for the agent that is about to depart from it.
// An environment-side rule in the style of policy_hold.hip, off by default and NOT in the reference. The insert rule
// (Agents.insert_agent_into_network, src/agents/base.py:247-331) puts a departing agent onto SELECTED_ROAD[origin], and every
// writer of that byte decides for the row's HEAD agent: an empty row reads the dummy agent 0 (fs_head_agent), so the first hop
// of every trip heads for agent 0's destination. Two launches per frame, after the head (and the optional hold launch) has
// written SELECTED_ROAD and before Direction. A policy's draw, its log-prob, the stored action and the PPO update never see
// them.
//
//   k_pending_window / k_pending_all: pend[u][b] = the SMALLEST agent id among the READY agents of environment b with
//   ORIGIN == u, -1 where there is none. Ready is the insert rule's: a_status == 0 && a_dep <= t; every row of the table
//   counts, agent 0 included. All ready agents of one origin are inserted onto the same road in one frame, so one speaks for
//   all: the smallest id is the first one the insert admits. The table is set to 0xFF bytes (-1) and the ids go in by an
//   UNSIGNED integer atomicMin: the result does not depend on scheduling. With the departure window (a_order, a_win, cur_lo)
//   one wave per environment walks the window from cur_lo[b] while the sorted departure is <= t, the lanes along k: a_win is
//   16 B per entry and contiguous in k, so a wave step is one 1 KB run, plus one status byte per due entry. Everything before
//   the cursor is known not to wait any more (fused_insert.hip), everything after the first entry that is not due is not due
//   either. Without a_order every agent is looked at: one thread per (environment, agent). Both give the same table. Neither
//   touches the cursor or a_ins.
//
//   k_fused_route_departures<Lookup>: one thread per (row u, environment b), flat index gid = u * B + b with the environment
//   fastest — the select kernels' shape (fused_select.h). pend[gid] is read FIRST and a lane leaves unless it is >= 0; then
//   the count bits of hdp (a DIRTY empty row is empty; a non-empty row keeps its head's choice: the head moves on that byte
//   in the same frame); only then the gather. On a sparsely departing network most lanes stop after one 4-byte load.
//     TableLookup: fs_next_hop_code<HOLD = true> with p = pend as the head — destination, slot, next_hop[b or 0][slot][u],
//                  next hop == destination -> u (the agent is inserted onto its origin road and withdrawn there once it is
//                  due). ONE difference from the select kernel: an unreachable destination (next hop < 0) leaves the row
//                  untouched; the select kernel writes a -1 the insert cannot take.
//     PlanLookup:  the middle of k_fused_select_route (routes.hip) with p as the head: len check, smallest j with r[j] == u,
//                  destination row -> u, r[j + 1] == r[len - 1] -> u; no route or off the route: untouched.
//   A routed row is written as the select kernels write: the rank byte (fs_rank_code) into sel8, the value into sel where the
//   code is SEL_RAW, the env-major choice8 test hook, and routed[b] += 1 (an integer atomic, as `held` is). Every other row
//   keeps sel8 / sel byte for byte.
//   Must move per frame: 4 N B bytes of pend set, 16 + 1 B per due window entry, 4 B per ready agent (atomic), 4 N B bytes of
//   pend read, 4 B of hdp per pending row, and per routed row the destination, slot and table word, 1 (+ 4) B stored.
//   Plain vector stores, no LDS, no floating-point atomics.
#include <cmath>
#include <mutex>
#include <unordered_map>

#include "fused_select.h"
#include "rollout_heads.h"

#define PD_WAVE 64

__global__ __launch_bounds__(PD_WAVE) void k_pending_window(const uint4* __restrict__ a_win,
                                                            const uint8_t* __restrict__ a_status,
                                                            const int32_t* __restrict__ cur_lo, int64_t A, int64_t B, int64_t N,
                                                            float t, uint32_t* __restrict__ pend) {
  const int64_t b = blockIdx.x;
  const uint4* win = a_win + b * A;
  const uint8_t* st = a_status + b * A;
  const int32_t lo = cur_lo[b];
  for (int64_t k0 = lo < 0 ? 0 : lo; k0 < A; k0 += PD_WAVE) {     // one wave: no barrier, the vote is the wave's
    const int64_t k = k0 + threadIdx.x;
    bool notdue = false;
    if (k < A) {
      const uint4 w = win[k];
      notdue = !(__uint_as_float(w.x) <= t);
      if (!notdue && (int64_t)w.z < A && (int64_t)w.y < N && st[w.z] == 0) atomicMin(pend + (int64_t)w.y * B + b, w.z);
    }
    if (__any(notdue ? 1 : 0)) break;                             // sorted by departure: nothing beyond this step is due
  }
}

__global__ __launch_bounds__(FS_BLOCK) void k_pending_all(const float* __restrict__ a_dep, const uint8_t* __restrict__ a_status,
                                                          const int32_t* __restrict__ a_origin, int64_t A, int64_t B, int64_t N,
                                                          float t, uint32_t* __restrict__ pend) {
  const int64_t gid = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x;
  if (gid >= A * B) return;
  if (a_status[gid] != 0 || !(a_dep[gid] <= t)) return;
  const int64_t b = gid / A, a = gid - b * A;
  const int32_t u = a_origin[gid];
  if (u >= 0 && u < N) atomicMin(pend + (int64_t)u * B + b, (uint32_t)a);
}

struct TableLookup {
  const int32_t *a_dest, *dest_slot, *next_hop;
  int64_t nh_bstride, D;
  __device__ __forceinline__ bool operator()(long long p, uint32_t u, uint32_t b, const NodeRec* __restrict__ nodes,
                                             const int32_t* __restrict__ out_pad, int64_t A, int64_t N, uint32_t* code,
                                             float* sv) const {
    return fs_next_hop_code<true>(p, u, b, nodes, out_pad, a_dest, A, N, dest_slot, next_hop, nh_bstride, D, code, sv) &&
           *sv >= 0.0f;      // (a held row has its own id here: only an unreachable destination is negative)
  }
};

struct PlanLookup {
  const int32_t *routes, *route_len;
  int64_t r_bstride, len_bstride;
  int32_t max_hops;
  __device__ __forceinline__ bool operator()(long long p, uint32_t u, uint32_t b, const NodeRec* __restrict__ nodes,
                                             const int32_t* __restrict__ out_pad, int64_t A, int64_t, uint32_t* code,
                                             float* sv) const {
    if (p < 0 || p >= A) return false;
    const int32_t len = route_len[(int64_t)b * len_bstride + p];
    if (len <= 0 || len > max_hops) return false;
    const int32_t* r = routes + (int64_t)b * r_bstride + p * (int64_t)max_hops;
    int32_t j = 0;
    while (j < len && r[j] != (int32_t)u) ++j;
    if (j >= len) return false;
    int32_t nh = (int32_t)u;
    if (j < len - 1) {
      nh = r[j + 1];
      if (nh == r[len - 1]) nh = (int32_t)u;
    }
    *sv = (float)nh;
    *code = fs_rank_code(nodes[u], out_pad, *sv);
    return true;
  }
};

template <class Lookup>
__global__ __launch_bounds__(FS_BLOCK) void k_fused_route_departures(
    const int32_t* __restrict__ pend, const uint2* __restrict__ hdp, const NodeRec* __restrict__ nodes,
    const int32_t* __restrict__ out_pad, int64_t A, uint32_t B, uint32_t NB, int64_t N, Lookup look,
    uint8_t* __restrict__ sel8, float* __restrict__ sel, uint8_t* __restrict__ choice8, int32_t* __restrict__ routed) {
  const uint32_t gid = blockIdx.x * FS_BLOCK + threadIdx.x;      // N * B < 2^31 (tarl_check_fused_core)
  if (gid >= NB) return;
  const uint32_t u = gid / B, b = gid - u * B;
  const int32_t p = pend[gid];
  bool write = false;
  uint32_t code = SEL_RAW;
  if (p >= 0 && (hdp[gid].x & HD_CNT) == 0u) {                    // nobody departs here, or the row's head keeps its choice
    float sv = 0.0f;
    write = look((long long)p, u, b, nodes, out_pad, A, N, &code, &sv);
    if (write) {
      if (code == SEL_RAW) sel[gid] = sv;
      sel8[gid] = (uint8_t)code;
      if (routed) atomicAdd(routed + b, 1);
    }
  }
  // env-major copy of the row's byte as it stands now (the select kernels' test hook, one scattered byte)
  if (choice8) choice8[(int64_t)b * N + u] = write ? (uint8_t)code : sel8[gid];
}

// ---- the launches alone (handle and arguments checked by the caller) ----------------------------------------------------------
int tarl_launch_pending_departures(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, float t,
                                   int32_t* pend) {
  const int64_t N = plan->N;
  TARL_CHECK_HIP(hipMemsetAsync(pend, 0xFF, (size_t)(N * B) * sizeof(int32_t), s));
  if (f->a_order && f->a_win) {
    hipLaunchKernelGGL(k_pending_window, dim3((unsigned)B), dim3(PD_WAVE), 0, s, (const uint4*)f->a_win,
                       (const uint8_t*)f->a_status, (const int32_t*)f->cur_lo, A, B, N, t, (uint32_t*)pend);
  } else {
    hipLaunchKernelGGL(k_pending_all, dim3((unsigned)ceil_div(A * B, FS_BLOCK)), dim3(FS_BLOCK), 0, s, (const float*)f->a_dep,
                       (const uint8_t*)f->a_status, (const int32_t*)f->a_origin, A, B, N, t, (uint32_t*)pend);
  }
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

template <class Lookup>
static int launch_route(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, const int32_t* pend,
                        const Lookup& look, uint8_t* choice8, int32_t* routed) {
  const int64_t NB = plan->N * B;
  hipLaunchKernelGGL(k_fused_route_departures<Lookup>, dim3((unsigned)ceil_div(NB, FS_BLOCK)), dim3(FS_BLOCK), 0, s, pend,
                     (const uint2*)f->hdp, (const NodeRec*)f->node_rec, (const int32_t*)f->out_pad, A, (uint32_t)B,
                     (uint32_t)NB, plan->N, look, f->sel8, f->sel, choice8, routed);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- the switch of the one-call rollouts -------------------------------------------------------------------------------------
// tarl_fused ends where the hold rule's pointer was appended; the router's arguments live beside it, keyed by the handle's
// address, and bit 1 of tarl_fused.policy_hold says that an entry is there (a fresh handle has the word zero, whatever an
// earlier handle at the same address had registered).
static std::mutex g_router_mutex;
static std::unordered_map<const tarl_fused*, DepartureRouter> g_routers;

// what tarl_fused_set_departure_router registered for f, checked against the plan (the setter has no plan to know N by)
int tarl_departure_router_of(const tarl_plan* plan, const tarl_fused* f, DepartureRouter* r) {
  {
    std::lock_guard<std::mutex> lock(g_router_mutex);
    const auto it = g_routers.find(f);
    TARL_REQUIRE(it != g_routers.end(), "the departure router is switched on but was never set");
    *r = it->second;
  }
  TARL_REQUIRE(r->nh_bstride == 0 || r->nh_bstride >= r->D * plan->N, "next-hop tables overlap");
  TARL_REQUIRE(f->a_dest && f->a_origin && f->a_dep && f->a_status, "fused agent buffers missing");
  return TARL_OK;
}

int tarl_launch_departure_router(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t A, float t,
                                 const DepartureRouter& r) {
  const int rc = tarl_launch_pending_departures(s, plan, f, B, A, t, r.pend);
  if (rc) return rc;
  return launch_route(s, plan, f, B, A, r.pend, TableLookup{f->a_dest, r.dest_slot, r.next_hop, r.nh_bstride, r.D}, nullptr,
                      r.routed);
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
static int check_sizes(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents) {
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(num_agents >= 1 && num_agents <= ((int64_t)1 << 24), "bad sizes");
  return TARL_OK;
}

extern "C" int tarl_fused_pending_departures(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                             int64_t num_agents, float t, int32_t* pend, tarl_stream stream) {
  TARL_REQUIRE(plan && f && pend, "null argument");
  const int rc = check_sizes(plan, f, B, Nmax, num_agents);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(f->a_origin && f->a_dep && f->a_status, "fused agent buffers missing");
  TARL_REQUIRE(f->a_order == nullptr || (f->cur_lo != nullptr && f->a_dep_sorted != nullptr),
               "a_order needs cur_lo and a_dep_sorted");
  TARL_REQUIRE(ceil_div(num_agents * B, FS_BLOCK) < ((int64_t)1 << 31), "bad sizes");
  TARL_REQUIRE(std::isfinite(t), "non-finite time");
  if (plan->N == 0) return TARL_OK;
  return tarl_launch_pending_departures((hipStream_t)stream, plan, f, B, num_agents, t, pend);
}

static int check_table(const tarl_plan* plan, const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride,
                       int64_t num_dests) {
  TARL_REQUIRE(dest_slot && next_hop, "null argument");
  TARL_REQUIRE(num_dests >= 1, "num_dests must be >= 1");
  TARL_REQUIRE(nh_bstride == 0 || (plan && nh_bstride >= num_dests * plan->N), "next-hop tables overlap");
  return TARL_OK;
}

extern "C" int tarl_fused_route_departures(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                           int64_t num_agents, const int32_t* pend, const int32_t* dest_slot,
                                           const int32_t* next_hop, int64_t nh_bstride, int64_t num_dests, uint8_t* choice8,
                                           int32_t* routed, tarl_stream stream) {
  TARL_REQUIRE(plan && f && pend && dest_slot && next_hop, "null argument");
  int rc = check_sizes(plan, f, B, Nmax, num_agents);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(f->a_dest, "fused agent buffers missing");
  rc = check_table(plan, dest_slot, next_hop, nh_bstride, num_dests);
  if (rc != TARL_OK) return rc;
  if (plan->N == 0) return TARL_OK;
  return launch_route((hipStream_t)stream, plan, f, B, num_agents, pend,
                      TableLookup{f->a_dest, dest_slot, next_hop, nh_bstride, num_dests}, choice8, routed);
}

extern "C" int tarl_fused_route_departures_plan(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                                int64_t num_agents, const int32_t* pend, const int32_t* routes,
                                                const int32_t* route_len, int64_t r_bstride, int64_t max_hops,
                                                uint8_t* choice8, int32_t* routed, tarl_stream stream) {
  TARL_REQUIRE(plan && f && pend && routes && route_len, "null argument");
  const int rc = check_sizes(plan, f, B, Nmax, num_agents);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(max_hops >= 1 && max_hops <= ((int64_t)1 << 20), "max_hops must be in [1, 2^20]");
  TARL_REQUIRE(r_bstride == 0 || r_bstride >= num_agents * max_hops, "route tables overlap");
  if (plan->N == 0) return TARL_OK;
  return launch_route((hipStream_t)stream, plan, f, B, num_agents, pend,
                      PlanLookup{routes, route_len, r_bstride, r_bstride ? num_agents : (int64_t)0, (int32_t)max_hops},
                      choice8, routed);
}

extern "C" int tarl_fused_set_departure_router(tarl_fused* f, int on, const int32_t* dest_slot, const int32_t* next_hop,
                                               int64_t nh_bstride, int64_t num_dests, int32_t* pend, int32_t* routed) {
  TARL_REQUIRE(f, "null argument");
  TARL_REQUIRE(on == 0 || on == 1, "on must be 0 or 1");
  if (on) {
    TARL_REQUIRE(dest_slot && next_hop && pend, "the switch without a table");
    TARL_REQUIRE(num_dests >= 1, "num_dests must be >= 1");
    TARL_REQUIRE(nh_bstride == 0 || nh_bstride >= num_dests, "next-hop tables overlap");
  } else {
    TARL_REQUIRE(!dest_slot && !next_hop && !pend && !routed, "a table or a routed counter without the switch");
  }
  std::lock_guard<std::mutex> lock(g_router_mutex);
  if (on) {
    g_routers[f] = DepartureRouter{dest_slot, next_hop, nh_bstride, num_dests, pend, routed};
    f->policy_hold |= TARL_DEPARTURE_ROUTER;
  } else {
    g_routers.erase(f);
    f->policy_hold &= ~TARL_DEPARTURE_ROUTER;
  }
  return TARL_OK;
}
