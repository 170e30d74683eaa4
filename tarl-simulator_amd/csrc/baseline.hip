// baseline.hip — the shortest-path (Dijkstra) baseline on the PACKED state: what a vectorised evaluation of the classical
// router needs beyond dest_trees.hip's trees. Reference semantics restated: DijkstraAgents.choice, src/agents/base.py:541-550
// (the edge weights) and :572-580 (SELECTED_ROAD = the next hop towards the destination of the row's head agent).
//
//   k_fused_edge_travel_time      == k_edge_travel_time (routing.hip) reading the count byte of hdp and the static node
//                                    records instead of x: every refresh, K environments at once.
//   k_fused_select_next_hop_dest  == k_select_next_hop_dest (dest_trees.hip) reading the packed words and the agent SoA and
//                                    writing the rank byte sel8 instead of a float into a 3 Nmax + 7 float row: every frame.
// Both are bit-identical, through tarl_fused_export, to their unfused counterparts on the exported x.
#include "fused_select.h"

// ---- (a) per-edge travel time -------------------------------------------------------------------------------------------
// The packed words are ENV-MINOR [N][B], the output is ENV-MAJOR [B][E]: a 64 edges x 64 environments tile of count bytes
// is turned through LDS. Read side: a wave takes one edge of the tile at a time and its 64 lanes read the count words of
// the edge's source row for 64 consecutive environments (512 contiguous bytes, the low word of each 8-byte hdp entry). A
// source row is read once per out-edge, not once: the repeats (out-degree, ~4 on a road network) are served by L2, and in
// exchange the kernel needs no src-sorted edge order. Write side: lane = edge, so a wave stores 256 contiguous bytes of
// one environment's row. The tile's row stride is 68 bytes = 17 words: the column reads of the write side fall into 32
// distinct banks.
#define TT_TILE 64
#define TT_BLOCK 256
__global__ __launch_bounds__(TT_BLOCK) void k_fused_edge_travel_time(const int32_t* __restrict__ src,
                                                                     const int32_t* __restrict__ dst,
                                                                     const uint2* __restrict__ hdp,
                                                                     const NodeRec* __restrict__ nodes, int64_t B,
                                                                     int64_t E, float* __restrict__ out) {
  __shared__ uint8_t s_n[TT_TILE][TT_TILE + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t e0 = (int64_t)blockIdx.x * TT_TILE, b0 = (int64_t)blockIdx.y * TT_TILE;
  for (int r = wave; r < TT_TILE && e0 + r < E; r += TT_BLOCK / 64)
    if (b0 + lane < B) s_n[r][lane] = (uint8_t)(hdp[(int64_t)src[e0 + r] * B + b0 + lane].x & HD_CNT);
  __syncthreads();
  const int64_t e = e0 + lane;
  if (e >= E) return;
  const int32_t u = src[e];
  const float maxn = nodes[u].maxn, ff = nodes[u].ff, cong = nodes[dst[e]].cong;
  for (int q = wave; q < TT_TILE && b0 + q < B; q += TT_BLOCK / 64) {
    // k_edge_travel_time's expressions, word for word
    const float tc = cong / ((maxn + 10.0f) - (float)s_n[lane][q]);
    out[(b0 + q) * E + e] = (tc > ff || tc != tc) ? tc : ff;
  }
}

// ---- (c) SELECTED_ROAD = next hop towards the head agent's destination, as the rank byte -----------------------------------
// One thread per (row i, environment b), flat index i * B + b with the environment fastest: the hdp loads and the sel8
// stores of a wave are contiguous for every B (a wave spans several rows when B < 64), and for B >= 64 the row — and with
// it the node record — is uniform over the wave. Inherently scattered: a_dest[b][head] (one 4-byte gather) and
// next_hop[b][slot][i] (one 4-byte gather; lanes of one row differ in b and slot). dest_slot is a small shared table.
// Must move per (row, environment): 8 B of hdp (4 used) + 4 + 4 + 4 B of gathers + 1 B stored = 21 B.
// k_select_next_hop_dest's rules, word for word: an empty FIFO reads agent 0 — x[i][0] of an empty row is 0 (the pending
// garbage triple, or a clean row's dead slot) unless the row is DIRTY with no garbage pending, where it is whatever the
// slot store holds at the ring offset (k_export_rows); a head, destination or slot out of range leaves the row untouched.
// The value written is (float)next_hop; the code is the rank of the first out-edge of i whose target converts to that
// value (k_pack_nodes' rule), else SEL_RAW with the value in `sel`: the destination itself, -1, an entry no out-edge matches.
// HOLD (tarl_fused_select_next_hop_hold; NOT DijkstraAgents.choice): where the next hop IS the destination, the row's own id
// is written instead. The comparison is made on the integers, before the conversion. In the environment's step order
// (SimulatorEnv._step: choice, core, withdraw / insert, reward) the core would carry that head onto its destination road,
// which the withdraw rule (roads adjacent to the destination) never collects from; held one road short, the head is
// collected as soon as it is due. No out-edge targets the row itself (the builders make no self-loops; on such a graph a
// holding head would take the loop), so a holding row stores SEL_RAW and its id and the core moves nobody from it. On the
// destination road the table already holds the road's id: nothing changes there. Same 21 B per (row, environment).
// The head decode and the rank code are fused_select.h's, shared with k_fused_select_route (routes.hip).
template <bool HOLD>
__global__ __launch_bounds__(FS_BLOCK) void k_fused_select_next_hop_dest(
    const uint2* __restrict__ hdp, const uint32_t* __restrict__ tl, const uint8_t* __restrict__ gc8,
    const float* __restrict__ slots, int64_t lds, int Nmax, const NodeRec* __restrict__ nodes,
    const int32_t* __restrict__ out_pad, const int32_t* __restrict__ a_dest, int64_t A, uint32_t B, uint32_t NB, int64_t N,
    const int32_t* __restrict__ dest_slot, const int32_t* __restrict__ next_hop, int64_t nh_bstride, int64_t D,
    uint8_t* __restrict__ sel8, float* __restrict__ sel, uint8_t* __restrict__ choice8) {
  const uint32_t gid = blockIdx.x * FS_BLOCK + threadIdx.x;      // N * B < 2^31 (tarl_check_fused_core)
  if (gid >= NB) return;
  const uint32_t i = gid / B, b = gid - i * B;
  const long long head = fs_head_agent(hdp[gid].x, gid, tl, gc8, slots, lds, Nmax);
  uint32_t code = SEL_RAW;
  float sv = 0.0f;
  const bool write = fs_next_hop_code<HOLD>(head, i, b, nodes, out_pad, a_dest, A, N, dest_slot, next_hop, nh_bstride, D,
                                            &code, &sv);
  if (write) {
    if (code == SEL_RAW) sel[gid] = sv;
    sel8[gid] = (uint8_t)code;
  }
  // env-major copy of the row's byte as it stands now (the evaluator's action record: a test hook, one scattered byte)
  if (choice8) choice8[(int64_t)b * N + i] = write ? (uint8_t)code : sel8[gid];
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int tarl_fused_edge_travel_time(const tarl_plan* plan, const tarl_fused* f, int64_t B, float* travel_time,
                                           tarl_stream stream) {
  TARL_REQUIRE(plan && f && travel_time, "null argument");
  TARL_REQUIRE(f->hdp && f->node_rec, "fused node buffers missing");
  TARL_REQUIRE(B >= 1 && plan->N * B < ((int64_t)1 << 31), "bad sizes");
  if (plan->E == 0) return TARL_OK;
  TARL_REQUIRE(ceil_div(B, TT_TILE) < 65536, "too many environments for one launch");
  hipLaunchKernelGGL(k_fused_edge_travel_time, dim3((unsigned)ceil_div(plan->E, TT_TILE), (unsigned)ceil_div(B, TT_TILE)),
                     dim3(TT_BLOCK), 0, (hipStream_t)stream, plan->src, plan->dst, (const uint2*)f->hdp,
                     (const NodeRec*)f->node_rec, B, plan->E, travel_time);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

template <bool HOLD>
static int fused_select_launch(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                               const int32_t* dest_slot, const int32_t* next_hop, int64_t nh_bstride, int64_t num_dests,
                               uint8_t* choice8, tarl_stream stream) {
  TARL_REQUIRE(plan && f && dest_slot && next_hop, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(f->a_dest && num_agents >= 1, "fused agent buffers missing");
  TARL_REQUIRE(num_dests >= 0 && nh_bstride >= 0, "bad sizes");
  if (plan->N == 0) return TARL_OK;
  const int64_t NB = plan->N * B;
  hipLaunchKernelGGL(k_fused_select_next_hop_dest<HOLD>, dim3((unsigned)ceil_div(NB, FS_BLOCK)), dim3(FS_BLOCK), 0,
                     (hipStream_t)stream, (const uint2*)f->hdp, (const uint32_t*)f->tl, (const uint8_t*)f->gc8,
                     (const float*)f->slots, f->ld_slots, (int)Nmax, (const NodeRec*)f->node_rec,
                     (const int32_t*)f->out_pad, (const int32_t*)f->a_dest, num_agents, (uint32_t)B, (uint32_t)NB, plan->N,
                     dest_slot, next_hop, nh_bstride, num_dests, f->sel8, f->sel, choice8);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_fused_select_next_hop_dest(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                               int64_t num_agents, const int32_t* dest_slot, const int32_t* next_hop,
                                               int64_t nh_bstride, int64_t num_dests, uint8_t* choice8, tarl_stream stream) {
  return fused_select_launch<false>(plan, f, B, Nmax, num_agents, dest_slot, next_hop, nh_bstride, num_dests, choice8, stream);
}

extern "C" int tarl_fused_select_next_hop_hold(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                               int64_t num_agents, const int32_t* dest_slot, const int32_t* next_hop,
                                               int64_t nh_bstride, int64_t num_dests, uint8_t* choice8, tarl_stream stream) {
  return fused_select_launch<true>(plan, f, B, Nmax, num_agents, dest_slot, next_hop, nh_bstride, num_dests, choice8, stream);
}
