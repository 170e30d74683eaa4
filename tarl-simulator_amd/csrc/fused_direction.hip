// fused_direction.hip — the Direction gather of a frame (k_fused_direction) and its launch dispatch. (Design: fused_frame.h.)
#include "fused_frame.h"

// ---- Direction gather on the dense words (env-minor: lane = environment) ---------------------------------------------------
// Two passes inside the workgroup. Pass 1 (every (node, environment) pair of the chunk): admissibility masks and the
// summed turn probability P — no random numbers — and the default post word (nobody chosen). A pair needs the Gumbel
// race only when P > 0, i.e. when some in-edge is admissible; that is a few percent of the pairs, but scattered over all
// lanes, so every wave would still pay for the Philox block and the two logs per edge. The pairs with P > 0 are
// therefore appended to an LDS list and pass 2 walks that list densely (one lane per pair), evaluating the pair again, now
// with its noise — same Philox indices, same expressions: the result is bit-identical to evaluating everything.
// WORD TABLE (NCH = 4): pass 2 needs nothing pass 1 did not hold a moment earlier, and the kernel writes only `post`. The
// lane that lists a pair therefore leaves the pair's dense words beside the list entry — the four upstream head words, the
// four upstream SELECTED_ROAD codes and the row's own count, 40 bytes, indexed by the list position (s_wh / s_wc) — and the
// chunk's NCH rows' statics (in-degree, CSC base, the row's limits, the four embedded in-edge records and their
// log turn probabilities: DirStat) are staged once per workgroup from scalar loads. A table-served pair with at most four
// in-edges reaches its post store without a global vector load; in-edges of rank >= 4 are gathered one by one as before.
// The table holds DIR_WORDS entries: a pair listed beyond it, every pair of a workgroup that repeats its pass in exact form
// (the list is rebuilt from global words then), and the NCH = 1 / 2 instantiations take the gather path — node record,
// own head words, then the upstream words: two dependent rounds in front of the race.
#define DIR_LIST (TILE * 8)
#define DIR_WORDS 128   // entries of the word table (5 KB; with the list and the statics 9.9 KB of LDS per workgroup)
struct __attribute__((aligned(16))) DirStat {   // what pass 2 reads of a row's node record, + log_edge_attr of in4's edges
  int32_t in0, in_deg;
  float maxn, road;
  InRec in4[4];
  float le[4];
};
// does upstream row j (dense words hj, SELECTED_ROAD code cj) send its head to the row behind an in-edge of rank code rk?
// EXACT: a raw SELECTED_ROAD (cj == SEL_RAW: a value pack found among none of j's out-edges) is compared as a value.
template <bool EXACT>
__device__ __forceinline__ bool edge_admissible(uint32_t cj, int32_t rk, const float* __restrict__ sel_raw, int64_t jrow,
                                                uint2 hj, float max_j, float road_i, float n_i, float max_i, float t) {
  bool heads_here = cj == (uint32_t)rk;   // ranks are < SEL_RAW: a raw code never matches here
  if (EXACT && cj == SEL_RAW) heads_here = sel_raw[jrow] == road_i;
  const float dep = __uint_as_float(hj.y), n_j = (float)(hj.x & HD_CNT);
  // (bitwise on purpose: lane masks and'ed / or'ed by the scalar unit, no short-circuit control flow)
  const bool m1 = (dep <= t) & (n_i < max_i - TARL_CONGESTION_FILE) & (n_j > 0.0f);
  const bool m2 = ((dep - t) < -10.0f) & ((max_j - TARL_CONGESTION_FILE) <= n_j) & ((max_j - n_j) <= (max_i - n_i));
  return heads_here & (m1 | m2);
}

// Every read-only array is its own `const __restrict__` kernel argument: topology, statics and edge constants are
// wave-uniform and must compile to SCALAR loads (through a struct member the compiler has to assume they alias the post
// stores and falls back to dependent vector loads — measured: 48 -> 85 us per launch).
// CNT: the row's own count comes from a byte per (row, environment) — in a rollout the count buffer's slice of the frame
// before, which the row pass and the insert kernel have just written — instead of its 8-byte head words: of its own row the
// dense pass needs the count and the tail word only (12 -> 5 bytes per pair).
template <int NCH, bool SIB, bool CNT, bool O32>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fused_direction(
    const NodeRec* __restrict__ nodes, const InRec* __restrict__ in_rec, const int32_t* __restrict__ in_eid,
    const float* __restrict__ log_edge_attr, const uint2* __restrict__ hdp, const uint32_t* __restrict__ tl,
    const uint8_t* __restrict__ cnt8, const uint8_t* __restrict__ gc8, const float* __restrict__ slots, int64_t lds,
    int Nmax, int32_t wcap, const uint8_t* __restrict__ sel8,
    const float* __restrict__ sel_raw,
    const float* __restrict__ gumbel, float* __restrict__ dtt, uint32_t* __restrict__ post, float log_eps, float t,
    float t_prev, uint64_t seed, uint64_t counter, uint32_t E, uint32_t B, uint32_t N, FrameOut out, uint64_t env_base) {
  constexpr bool TABLE = NCH == 4;
  __shared__ int32_t s_n;
  __shared__ uint16_t s_item[DIR_LIST];   // (node offset in the chunk) * TILE + lane
  // the word table (see above), structure of arrays: lane = list position in pass 2. The first wcap (<= DIR_WORDS) list
  // positions have an entry
  __shared__ uint2 s_wh[4][TABLE ? DIR_WORDS : 1];   // upstream head words hj[.][q]
  __shared__ uint2 s_wc[TABLE ? DIR_WORDS : 1];      // {cj[.][0..3], a byte each; the row's own count}
  __shared__ DirStat s_stat[TABLE ? NCH : 1];
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;   // row indices are 32-bit: N * B < 2^31 (host check)
  const bool valid = b < B;
  // The chunks are walked from the LAST to the first: the row pass before this launch (and the one after it) walks them
  // from the first to the last, so each of the two kernels starts on the quarter of the state the other has just touched —
  // what the 256 MB Infinity Cache still holds of a 1.7 GB frame. Forward order here: Direction 203 us and row pass 215 us
  // per launch instead of 188 and 205 (same box).
  const uint32_t i0 = (gridDim.y - 1u - blockIdx.y) * NCH;
  if (threadIdx.x == 0) s_n = 0;
  // pass 1, branch-free form: a raw SELECTED_ROAD code is only noted; if any lane of the workgroup saw one (never in a
  // rollout: every node with out-edges draws an action in every frame) the pass is repeated in its exact form.
  // NCH rows per lane, ALL their loads (own words + the first four in-edges' gathers) issued before anything is used:
  // the pass is bound by memory latency and by scalar-instruction issue, so requests in flight per wave and address
  // arithmetic per request are what counts: one node record + one base address fetch a row's statics.
  bool raw_seen = false;
  uint2 hj[NCH][4];
  uint32_t ncnt[NCH];   // the row's own count
  uint32_t tlw[NCH], cj[NCH][4];
  if (valid) {
    // SIB: sibling rows — the roads that leave one intersection — have the same upstream rows. When every chunk's rows
    // list the same first four sources (checked once per graph, tarl_plan::siblings4), the upstream words are gathered
    // once per chunk instead of once per row: 16 requests per lane instead of 40.
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      const uint32_t i = (i0 + r < N) ? i0 + r : N - 1;
      const uint32_t row = i * B + b;
      ncnt[r] = CNT ? (uint32_t)cnt8[row] : (at32<O32>(hdp, row).x & HD_CNT);
      tlw[r] = at32<O32>(tl, row);
      const InRec* ir = nodes[i].in4;   // the first four in-edge records travel in the node record
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (SIB && r > 0) {
          hj[r][q] = hj[0][q];
          cj[r][q] = cj[0][q];
        } else {
          const uint32_t jrow = (uint32_t)ir[q].src * B + b;
          hj[r][q] = at32<O32>(hdp, jrow);
          cj[r][q] = sel8[jrow] & 0x7Fu;
        }
      }
    }
  }
  // The gathers are in flight. The barrier that orders s_n = 0 before the first list entry stands HERE, not in front of the
  // loads, and the statics are staged in front of it: their second scalar round (log_edge_attr behind the record's edge
  // ids) and the wait for the other waves pass beside the gathers (the barrier alone: 334 -> 318 us per launch).
  if (TABLE) {   // the rows' statics for pass 2: row r by wave r (modulo the waves there are), from scalar loads
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x) >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      const uint32_t owner = nw == 1u ? 0u : ((uint32_t)r < nw ? (uint32_t)r : (uint32_t)r - nw);
      if (wid == owner) {   // wave-uniform
        const NodeRec& nr = nodes[(i0 + r < N) ? i0 + r : N - 1];
        DirStat st;
        st.in0 = nr.in0, st.in_deg = nr.in_deg, st.maxn = nr.maxn, st.road = nr.road;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const InRec& rq = nr.in4[q];   // field by field: a struct copy is lowered to vector loads
          st.in4[q].src = rq.src, st.in4[q].rank = rq.rank, st.in4[q].ea = rq.ea, st.in4[q].max_src = rq.max_src;
          st.in4[q].eid = rq.eid;
          st.le[q] = q < nr.in_deg ? log_edge_attr[rq.eid] : 0.0f;   // (beyond the in-degree: never read)
        }
        s_stat[r] = st;   // wave-uniform values, every lane the same store: no divergent branch, the loads stay scalar
      }
    }
  }
  __syncthreads();
  if (valid) {
    // SIB: the chunk's rows share their upstream rows, so what depends on the upstream row alone is evaluated once per
    // chunk and folded into two floats per upstream row: x1 = 0 where its head is due and it holds somebody (else NaN),
    // slk = its free slots where its head is overdue by more than 10 s and it is full (else NaN). Per (row, in-edge) the
    // two admissibility tests of edge_admissible are then `n_i + x1 < MAX_i - 3` and `slk <= MAX_i - n_i` (a NaN compares
    // false; n_i + 0 is n_i): the same comparisons on the same values, 6 instead of 14 vector instructions per pair.
    float x1[4], slk[4];
    if (SIB) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 hq = hj[0][q];
        const float max_j = nodes[i0].in4[q].max_src;     // (beyond the in-degree: padding, masked by the rank test)
        const float dep = __uint_as_float(hq.y), n_j = (float)(hq.x & HD_CNT);
        const bool a1 = (dep <= t) & (n_j > 0.0f);
        const bool a2 = ((dep - t) < -10.0f) & ((max_j - TARL_CONGESTION_FILE) <= n_j);
        x1[q] = a1 ? 0.0f : __uint_as_float(0x7fc00000u);
        slk[q] = a2 ? (max_j - n_j) : __uint_as_float(0x7fc00000u);
        // a raw SELECTED_ROAD code upstream sends the workgroup to the exact pass; noted per upstream row, whatever the
        // rows' in-degrees (a padding entry names row 0: at worst a repeat that was not needed)
        raw_seen = raw_seen | (cj[0][q] == SEL_RAW);
      }
    }
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      const uint32_t i = i0 + r;   // i, and everything indexed by it alone, is wave-uniform
      if (i < N) {
        const uint32_t row = i * B + b;
        const NodeRec& nr = nodes[i];
        const InRec* ir4 = nr.in4;
        const InRec* ir = in_rec + nr.in0;
        const float max_i = nr.maxn, n_i = (float)ncnt[r], road_i = nr.road;
        const float lim_i = max_i - TARL_CONGESTION_FILE, room_i = max_i - n_i;
        float P = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < nr.in_deg) {   // wave-uniform
            if (!SIB) raw_seen = raw_seen | (cj[r][q] == SEL_RAW);
            bool m;
            if (SIB)
              m = (cj[0][q] == (uint32_t)ir4[q].rank) & (((n_i + x1[q]) < lim_i) | (slk[q] <= room_i));
            else
              m = edge_admissible<false>(cj[r][q], ir4[q].rank, sel_raw, 0, hj[r][q], ir4[q].max_src, road_i, n_i, max_i, t);
            P = P + ir4[q].ea * (m ? 1.0f : 0.0f);
          }
        }
        for (int32_t q = 4; q < nr.in_deg; ++q) {   // in-degree above four: the rest one by one
          const uint32_t jrow = (uint32_t)ir[q].src * B + b;
          const uint2 hx = hdp[jrow];
          const uint32_t cx = sel8[jrow] & 0x7Fu;
          raw_seen = raw_seen | (cx == SEL_RAW);
          const bool m = edge_admissible<false>(cx, ir[q].rank, sel_raw, 0, hx, ir[q].max_src, road_i, n_i, max_i, t);
          P = P + ir[q].ea * (m ? 1.0f : 0.0f);
        }
        // nobody chosen (pass 2 overwrites). A row that idled in the last frame (tail word without TLF_AUTH) still holds
        // exactly this word from the frame before: whatever changes a row's tail, empties or fills it, or hands it an
        // arrival makes it an event row, and event rows and inserts set the flag
        if (tlw[r] & TLF_AUTH) at32<O32>(post, row) = (tlw[r] & ~0xFFu) | (ncnt[r] ? PF_NONEMPTY : 0u) | PF_TLAUTH;
        if (P > 0.0f) {
          const int32_t pos = atomicAdd(&s_n, 1);
          s_item[pos] = (uint16_t)(r * TILE + threadIdx.x);
          if (TABLE && pos < wcap) {
            const int rs = SIB ? 0 : r;   // siblings share their upstream rows
#pragma unroll
            for (int q = 0; q < 4; ++q) s_wh[q][pos] = hj[rs][q];
            s_wc[pos] = make_uint2(cj[rs][0] | (cj[rs][1] << 8) | (cj[rs][2] << 16) | (cj[rs][3] << 24), ncnt[r]);
          }
        }
      }
    }
  }
  const bool redo = __syncthreads_or(raw_seen ? 1 : 0) != 0;
  if (out.dtt_node && valid && b < (uint32_t)out.m_env) {   // metric environments: delta_travel_time once per upstream node
    for (uint32_t i = i0; i < i0 + NCH && i < N; ++i) {
      const uint32_t row = i * B + b;
      const uint2 mw = hdp[row];
      const uint32_t tw = tl[row];
      const bool lazy_i = (mw.x & HD_CNT) == 0u && !(tw & TLF_AUTH);   // empty and idle in the last frame: its garbage
      const float arr_i = head_arrival(slots, lds, gc8, row, mw.x, tw, Nmax, t_prev);   // head arrived at that frame's clock and
      const float dep_i = lazy_i ? t_prev + nodes[i].tt0 : __uint_as_float(mw.y);   // departs tt0 later (never stored)
      const float d = (dep_i - arr_i) - nodes[i].ff;
      out.dtt_node[(int64_t)i * out.m_env + b] = d > 0.0f ? d : (d != d ? d : 0.0f);
    }
  }
  if (redo || dtt) {   // exact form and / or the per-edge delta_travel_time of the frame API (uniform branch)
    if (redo && threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (valid) {
      for (uint32_t i = i0; i < i0 + NCH && i < N; ++i) {
        const uint32_t row = i * B + b;
        const uint2 mw = hdp[row];
        const NodeRec& nr = nodes[i];
        const InRec* ir = in_rec + nr.in0;
        const float max_i = nr.maxn, n_i = (float)(mw.x & HD_CNT), road_i = nr.road;
        float P = 0.0f;
        for (int32_t q = 0; q < nr.in_deg; ++q) {
          const int32_t j = ir[q].src;
          const uint32_t jrow = (uint32_t)j * B + b;
          const uint2 hx = hdp[jrow];
          if (redo) {
            const bool m = edge_admissible<true>(sel8[jrow] & 0x7Fu, ir[q].rank, sel_raw, jrow, hx, ir[q].max_src, road_i,
                                                 n_i, max_i, t);
            P = P + ir[q].ea * (m ? 1.0f : 0.0f);
          }
          if (dtt) {   // per-edge side output of DirectionMPNN.message (src/direction_mpnn.py:94-96): a property of j
            const uint32_t tj = tl[jrow];
            const bool lazy_j = (hx.x & HD_CNT) == 0u && !(tj & TLF_AUTH);
            const float arr_j = head_arrival(slots, lds, gc8, jrow, hx.x, tj, Nmax, t_prev);
            const float dep_j = lazy_j ? t_prev + nodes[j].tt0 : __uint_as_float(hx.y);
            const float d = (dep_j - arr_j) - nodes[j].ff;
            dtt[(int64_t)b * E + in_eid[nr.in0 + q]] = d > 0.0f ? d : (d != d ? d : 0.0f);
          }
        }
        if (redo && P > 0.0f) s_item[atomicAdd(&s_n, 1)] = (uint16_t)((i - i0) * TILE + threadIdx.x);
      }
    }
    __syncthreads();
  }
  const int32_t cnt = s_n;
  // list positions below wn carry their words (none after the exact pass, which re-lists from global words)
  const int32_t wn = (TABLE && !redo) ? (cnt < wcap ? cnt : wcap) : 0;
  for (int32_t idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
    const int32_t item = s_item[idx];
    const uint32_t i = i0 + item / TILE;
    const uint32_t bb = blockIdx.x * blockDim.x + (item % TILE);
    const uint32_t row = i * B + bb;
    int32_t in0, in_deg;
    float max_i, n_i, road_i;
    float P = 0.0f, best = -FLT_MAX;
    uint32_t best_id = 0u;
    PhiloxRun rng;
    InRec rc4[4];
    uint2 hx4[4];
    uint32_t cx4[4];
    float le4[4];
    if (TABLE && idx < wn) {   // everything from LDS: the row's statics by its offset in the chunk, the words by position
      const DirStat& st = s_stat[item / TILE];
      in0 = st.in0, in_deg = st.in_deg, max_i = st.maxn, road_i = st.road;
      const uint2 wc = s_wc[idx];
      n_i = (float)wc.y;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        rc4[q] = st.in4[q];
        le4[q] = st.le[q];
        hx4[q] = s_wh[q][idx];
        cx4[q] = (wc.x >> (8 * q)) & 0x7Fu;
      }
    } else {
      const uint2 mw = hdp[row];
      const NodeRec& nr = nodes[i];
      in0 = nr.in0, in_deg = nr.in_deg;
      max_i = nr.maxn, n_i = (float)(mw.x & HD_CNT), road_i = nr.road;
      // the first four in-edges: their records travel in the node record, so the gathers (upstream words, edge constant)
      // are ONE dependent round behind the node record; all four are requested before the first is used
#pragma unroll
      for (int q = 0; q < 4; ++q) rc4[q] = nr.in4[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t jrow = (uint32_t)rc4[q].src * B + bb;     // beyond in_deg: row 0 (valid, ignored)
        hx4[q] = hdp[jrow];
        cx4[q] = sel8[jrow] & 0x7Fu;
        le4[q] = log_edge_attr[rc4[q].eid];
      }
    }
    auto race = [&](int32_t q, const InRec& rc, const uint2 hx, const uint32_t cx, const float le) {
      const int32_t k = in0 + q;
      const uint32_t jrow = (uint32_t)rc.src * B + bb;
      const bool m = edge_admissible<true>(cx, rc.rank, sel_raw, jrow, hx, rc.max_src, road_i, n_i, max_i, t);
      P = P + rc.ea * (m ? 1.0f : 0.0f);
      float g;
      if (gumbel) {
        g = gumbel[(int64_t)bb * E + rc.eid];
      } else {
        const float u = rng.uniform(seed, counter, (env_base + (uint64_t)bb) * E + (uint64_t)k);
        g = gumbel_from_u01(u);
      }
      const float score = (m ? le : log_eps) + g;
      if (score > best) {
        best = score;
        best_id = hx.x >> 8;
      }
    };
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < in_deg) race(q, rc4[q], hx4[q], cx4[q], le4[q]);
    for (int32_t q = 4; q < in_deg; ++q) {
      const InRec rc = in_rec[in0 + q];
      const uint32_t jrow = (uint32_t)rc.src * B + bb;
      race(q, rc, hdp[jrow], sel8[jrow] & 0x7Fu, log_edge_attr[rc.eid]);
    }
    const uint32_t who = (P > 0.0f) ? best_id : 0u;
    if (who != 0u) post[row] = (who << 8) | PF_NONEMPTY | PF_ARRIVED;
  }
}

// rows per lane of the Direction gather (TARL_NCHUNK_DIR = 1, 2 or 4)
// cnt8: a byte per (row, environment) holding every row's current count (a rollout's count slice of the frame before), or NULL
int tarl_launch_direction(dim3 grid, unsigned threads, hipStream_t s, const tarl_plan* plan, const tarl_fused* f,
                          const float* edge_attr, const float* log_edge_attr, const uint8_t* sel8, const float* gumbel,
                          float* dtt, float log_eps, float time, float prev_time, uint64_t seed, uint64_t counter,
                          int64_t B, int Nmax, const FrameOut& out, const uint8_t* cnt8) {
#define DIR_LAUNCH_(NCH, SIB, CNT, O32)                                                                                   \
  hipLaunchKernelGGL((k_fused_direction<NCH, SIB, CNT, O32>), grid, dim3(threads), 0, s, (const NodeRec*)f->node_rec,          \
                     (const InRec*)f->in_rec, plan->in_eid, log_edge_attr, (const uint2*)f->hdp, (const uint32_t*)f->tl,  \
                     cnt8, (const uint8_t*)f->gc8, (const float*)f->slots, f->ld_slots, Nmax, (int32_t)wcap, sel8, (const float*)f->sel, gumbel, \
                     dtt, (uint32_t*)f->post, log_eps, time,   \
                     prev_time, seed, counter, (uint32_t)plan->E, (uint32_t)B, (uint32_t)plan->N, out, (uint64_t)f->env_base)
#define DIR_LAUNCH(NCH, SIB, CNT)                                                                                         \
  do {                                                                                                                     \
    if (o32) {                                                                                                             \
      DIR_LAUNCH_(NCH, SIB, CNT, true);                                                                                    \
    } else {                                                                                                               \
      DIR_LAUNCH_(NCH, SIB, CNT, false);                                                                                   \
    }                                                                                                                      \
  } while (0)
  const bool o32 = addr32_ok() && plan->N * B < ((int64_t)1 << 29);   // 8-byte words through 32-bit byte offsets (at32)
  // gc8 invariant (fused_common.h: head_arrival): a rollout stores the event byte in its LAST frame only (FrameOut::write_gc) —
  // and every frame for the metric environments, whose dtt_node reads it — while the tail word says "gc8 authoritative"
  // (TLF_AUTH) after every event. The per-edge delta_travel_time reads gc8 of EVERY environment: it may only be requested
  // by a caller whose frames all store the byte (the frame API does), and the per-node series only for metric environments.
  TARL_REQUIRE(dtt == nullptr || out.write_gc != 0,
               "per-edge delta_travel_time needs the event byte of every frame (FrameOut::write_gc): not available inside a rollout");
  // TARL_DIR_SIBLINGS=0 keeps the per-row gathers on a sibling graph (developer knob)
  const bool sib_ok = env_flag_on("TARL_DIR_SIBLINGS");
  // TARL_DIR_COUNT_BYTE=0 keeps the head words as the count's source (developer knob)
  if (!env_flag_on("TARL_DIR_COUNT_BYTE")) cnt8 = nullptr;
  // TARL_DIR_WORDS=n limits the word table of pass 2 to n entries (developer knob; 0: every listed pair takes the gather path)
  const int wknob = env_int("TARL_DIR_WORDS", DIR_WORDS);
  const int wcap = wknob < 0 ? 0 : (wknob > DIR_WORDS ? DIR_WORDS : wknob);
  switch (nchunk_dir()) {
    case 1: DIR_LAUNCH(1, false, false); break;
    case 2: DIR_LAUNCH(2, false, false); break;
    default:
      if (sib_ok && plan->siblings4) {
        if (cnt8) {
          DIR_LAUNCH(4, true, true);
        } else {
          DIR_LAUNCH(4, true, false);
        }
      } else {
        if (cnt8) {
          DIR_LAUNCH(4, false, true);
        } else {
          DIR_LAUNCH(4, false, false);
        }
      }
      break;
  }
#undef DIR_LAUNCH
#undef DIR_LAUNCH_
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
