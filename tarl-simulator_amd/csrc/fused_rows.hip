// fused_rows.hip — the row pass of a frame (k_fused_rows) and its launch dispatch. (Design: fused_frame.h.)
#include "fused_frame.h"

// ---- the row pass: Direction update + Response pop + withdraw on the slot store, then refresh the dense words -----------
// The pass has two phases inside the workgroup (the trick of the Direction gather, for the same reason). Phase A: every
// (row, environment) pair, on registers only — Response test from the prefetched post words, idle / event decision, and
// for an IDLE row (nothing enqueued, no pop, head not due: ~90 % of the pairs in a filling network) the refreshed dense
// words. EVENT rows (something moves: slot store, event word, agent rows) are only LISTED in LDS. Phase B walks that
// list densely, one lane per event row. The event path is hundreds of instructions long; issued per wave it ran for every
// wave (some lane nearly always has an event) at a few active lanes — the kernel is issue-bound, so that was its cost.
struct RowHead {      // what phase A derives from a row's dense words and hands to phase B through registers / the list
  uint32_t n0i, head_id0, tail0, who, arrived;
  bool pop;
};

// the statics of a row that phase A needs, loaded (scalar) at the head of the kernel instead of where they are used, behind
// the waits for the vector loads (one dependent scalar round per row there: -2 % on the pass)
struct RowStat {
  int32_t out_deg, out0;
  float tt0, maxn;
};
// phase A of one row: returns true when the row is an event row (nothing written), false when it was idle (words written)
// FAPI: the frame API's outputs (fp32 counts, env-major pop / withdraw masks) may be present; rollouts instantiate without
// them (their null tests, addresses and registers leave the idle path)
template <bool FAPI, bool O32>
__device__ __forceinline__ bool row_phase_a(uint32_t i, uint32_t b, const RowStat nr, const uint32_t* __restrict__ post,
                                            uint32_t pa, uint2 hp, uint32_t tlw, const uint32_t (&pj4)[4], int Nmax,
                                            uint32_t B, uint32_t N, const FusedBufs& fb, int64_t A, float t,
                                            const FrameOut& out, bool* pop_out, float* n_out) {
  const uint32_t row = i * B + b;   // 32-bit row indices: N * B < 2^31 (host check)
  const uint32_t n0i = hp.x & HD_CNT, head_id0 = hp.x >> 8;
  const uint32_t arrived = pa & PF_ARRIVED;
  const uint32_t who = arrived ? (pa >> 8) : 0u;   // the agent the Direction update enqueues
  // Response message + max-aggregate from the post words (state after the Direction update of every row)
  bool pop = false;
  {
    const uint32_t head = (n0i == 0u) ? who : head_id0;   // head after the Direction update
    const bool up = (n0i + arrived) > 0u;
    // (bitwise on purpose: four lane masks and'ed / or'ed, no short-circuit control flow)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      pop = pop | ((q < nr.out_deg) & up & ((pj4[q] & PF_NONEMPTY) != 0u) & ((pj4[q] >> 8) == head));
    for (int32_t q = 4; q < nr.out_deg; ++q) {   // out-degree above four: the rest one by one
      const int32_t j = glob(&fb.out_pad[nr.out0 + q]);
      const uint32_t pj = at32<O32>(post, (uint32_t)j * B + b);
      pop = pop | (up & ((pj & PF_NONEMPTY) != 0u) & ((pj >> 8) == head));
    }
  }
  const int q = (int)n0i;
  const bool lazy = (who == 0u) & (q < Nmax - 1);
  const uint32_t ni = n0i + arrived;   // count after the Direction update
  if ((int)ni >= Nmax) glob(fb.flags).atomic_or(FLAG_COUNT_AT_NMAX);
  const uint32_t head_id = (n0i == 0u) ? who : head_id0;
  // an empty row's head is this frame's garbage triple (0, t, t + tt): its departure needs the division only there
  const float head_dep = (n0i == 0u) ? t + nr.tt0 : __uint_as_float(hp.y);
  // is the (unpopped) head a withdraw candidate? (the first two tests of the withdraw scan, on registers)
  const bool due = (!pop) & (ni > 0u) & ((int64_t)head_id < A) & (head_dep <= t);
  *pop_out = pop;
  // the row's count after the pass is ni - pop - (agents withdrawn): all but the last term is known here, so the row's
  // share of the environment's count sum rides on the idle rows' coalesced atomic; the event path adds only what it
  // withdraws (rare) instead of one scattered global atomic per event row
  *n_out = (float)(ni - (pop ? 1u : 0u));
  // The count byte of EVERY row goes out here, from the lane that owns the row (whole-wave, coalesced): an event row's count
  // after the pass is ni - pop - (agents withdrawn), and all but the last term is known; phase B rewrites the byte only
  // when it withdraws somebody (rare). One scattered store per event row less on the event path (an extra 4-byte store
  // per event row was measured at +13 ... +30 % on the pass).
  if (out.counts8) __builtin_nontemporal_store((uint8_t)(ni - (pop ? 1u : 0u)), &at32<O32>(out.counts8, row));
  if (!(lazy & !pop & !due)) return true;
  // IDLE ROW: nothing moves, and (almost) nothing is written. With agents, the row keeps its head and count: its word
  // is already what a refresh would store. Empty, its garbage head departs at t + tt0, which changes every frame — but
  // nobody reads the departure of an empty row that was idle (tail word without TLF_AUTH): this pass recomputes it, the
  // Direction gather's tests need an agent in the row or MAX_NUMBER_OF_AGENT <= 3 (rows that small keep the eager word),
  // export and delta_travel_time derive it from the clock. The tail word changes only when its flag has to go.
  if (n0i == 0u && nr.maxn <= TARL_CONGESTION_FILE)
    gat<O32>(fb.hdp, row) = make_uint2((head_id << 8) | ni | (hp.x & HD_DIRTY), __float_as_uint(head_dep));
  if (tlw & TLF_AUTH) {
    gat<O32>(fb.tl, row) = tlw & ~TLF_AUTH;      // tail and ring offset stay
    // ... and the post word's mirror of the flag goes with it (other workgroups may be gathering this word for their
    // Response test right now: they look at PF_NONEMPTY and the tail id, which do not change)
    gat<O32>(fb.post, row) = pa & ~PF_TLAUTH;
  }
  if (FAPI && out.countsf) __builtin_nontemporal_store((float)ni, &out.countsf[row]);
  if (FAPI && out.popped) out.popped[(int64_t)b * N + i] = 0;
  if (FAPI && out.withdrawn) out.withdrawn[(int64_t)b * N + i] = 0;
  if (out.events && b < out.m_env) out.events[(int64_t)i * out.m_env + b] = 0;
  return false;
}

// phase B of one EVENT row (its dense words travel with the list entry): Direction update on the slot store,
// Response pop, withdraw, refreshed dense words + event word. -> {count after the pass, agents withdrawn}
// Round 4, measured and rejected on this function and its caller (same-box A/B at 16 384 environments, profiles/README.md):
// (1) every load whose address follows from the list entry requested at the head of the function — the record a pop
// exposes, the destination of the scan's first candidate, the withdraw test's out-edge targets from the node record — for
// every event row: row pass +7 % / +15 % (headline / loaded network), 7 M more scattered requests per launch; the same only
// for heads that are due and without re-reading the record the scan stopped at: +2 % / +1 %, 14 spilled VGPRs in the hot
// idle path. (2) DENSE rows: for a wave-row with >= 4 / 8 / 16 event lanes the refreshed words handed back through the
// list and stored by the owning lanes as FULL 64-byte lines after a second barrier (re-read from L2, flag clears of the idle
// lanes folded in): loaded network +14 % / +15 % / +2 % slower, and the extra LDS table and live state put scratch traffic
// into the idle path (headline 181 -> 312 us). (3) 32-byte slot records (full-sector stores): fused_common.h, TARL_SLW.
// What did pay: one store fewer per event row (the 8-byte event word rec1 became the byte gc8: -10 % / -17 %).
template <bool FAPI>
__device__ __forceinline__ float2 row_phase_b(uint32_t i, uint32_t b, bool pop, uint32_t pa, uint2 hp, uint32_t tlw,
                                              const NodeRec& nr, const int32_t* __restrict__ out_ptr,
                                              const int32_t* __restrict__ out_dst, int Nmax, uint32_t B, uint32_t N,
                                              const FusedBufs& fb, float* __restrict__ ag, int64_t A, int64_t a_bstride,
                                              float t, const FrameOut& out) {
  const PlanOut P{out_ptr, out_dst};
  const uint32_t row = i * B + b;
  const float4 st = make_float4(nr.maxn, nr.ff, nr.road, nr.cong);
  const uint32_t n0i = hp.x & HD_CNT, head_id0 = hp.x >> 8, tail0 = tlw >> 8;
  const uint32_t arrived = pa & PF_ARRIVED;
  const uint32_t who = arrived ? (pa >> 8) : 0u;
  const float n0 = (float)n0i;
  const int q = (int)n0i;
  // exact, slot-by-slot bookkeeping of the dead slots: rows that are dirty already, and from the moment the FIFO touches
  // its last slot (count >= Nmax - 1: no dead slot is left above the one this update writes, so nothing has to be
  // materialised at the transition). A clean row's dead slots are zero by the invariant (fused_common.h) whatever the
  // store holds: its pops and withdraws neither read nor write them.
  const bool exact = (hp.x & HD_DIRTY) != 0u || q >= Nmax - 1;
  // Direction update (every row, also when nothing was chosen): one 12-byte store — or, for a row that received
  // nobody, nothing at all (lazy garbage slot, see the file header).
  const float dep_new = t + entry_tt(st, n0);
  const bool lazy = (who == 0u) && (q < Nmax - 1);
  const uint32_t ni = n0i + arrived;   // count after the Direction update
  uint32_t head_id = (n0i == 0u) ? who : head_id0;
  float head_dep = (n0i == 0u) ? dep_new : __uint_as_float(hp.y);
  {
    // The FIFO is a ring buffer: logical slot s lives at physical slot (hoff + s) mod Nmax.
    const auto sl = gbase(fb.slots) + (int64_t)row * fb.lds;  // slot s = sl[3s .. 3s+2] = {id, arrival, departure}
    int hoff = tl_hoff(tlw);     // (the event byte gc8 is write-only here: no load sits between the row and its slots)
    if (!lazy && q < Nmax) {
      slot_store(sl + SLW * phys(hoff, q, Nmax), (float)who, t, dep_new);
    }
    int n = (int)ni;
    uint32_t tail_id = arrived ? who : tail0;

    // Response pop: logical shift by one where the LAST slot keeps its value. Ring form: the slot that falls off the
    // front becomes the new logical last slot, so it receives a copy of the old last slot; then the head advances.
    int shift = 0;
    if (pop) {
      if (exact) {
        const SlotRec last = slot_load(sl + SLW * phys(hoff, Nmax - 1, Nmax));
        slot_store(sl + SLW * hoff, last.id, last.arr, last.dep);
      }
      hoff = phys(hoff, 1, Nmax);
      shift = 1;
      n = n - 1;
    }
    // withdraw: leading run of the (popped) row
    int c = 0;
    if (n > 0) {
      const long long road = (long long)st.z;
      int32_t w0 = -1, w1 = 0;   // out-list of this row's road: fetched only when a head is actually due
      for (int sx = 0; sx < Nmax && sx < n; ++sx) {
        float idf, depf;
        if (sx == 0 && shift == 0) {   // the head is in registers unless the pop just exposed a new one
          idf = (float)head_id;
          depf = head_dep;
        } else {
          const SlotRec rd = slot_load(sl + SLW * phys(hoff, sx, Nmax));
          idf = rd.id;
          depf = rd.dep;
        }
        const long long id = (long long)idf;
        if (id < 0 || id >= A) break;
        if (!(depf <= t)) break;  // tested first: most heads are still travelling, and the lookup below is a gather
        const int32_t dest32 = glob(&fb.a_dest[(int64_t)b * A + id]);
        const long long dest = (long long)dest32;
        if (w0 < 0) {
          w0 = 0;
          if (road >= 0 && road < N) {
            w0 = P.out_ptr[road];
            w1 = P.out_ptr[road + 1];
          }
        }
        bool conn = false;
        for (int32_t k = w0; k < w1; ++k) conn = conn || ((long long)P.out_dst[k] == dest);
        if (!conn) break;
        float* a = ag + (int64_t)b * a_bstride + id * AG_COLS;
        a[AG_DONE] = 1.0f;
        a[AG_ON_WAY] = 0.0f;
        a[AG_ARR] = t;
        glob(&fb.a_status[(int64_t)b * A + id]) = (uint8_t)2;
        ++c;
      }
    }
    // withdraw = logical shift by c with zero fill: the c slots that fall off the front become the zeroed tail
    for (int k = 0; exact && k < c; ++k) {
      slot_store(sl + SLW * phys(hoff, k, Nmax), 0.0f, 0.0f, 0.0f);
    }
    if (c > 0) {
      hoff = phys(hoff, c, Nmax);   // c <= Nmax
      n = n - c;
    }
    if (shift + c > 0) {
      if (lazy && n == 0) {  // the row emptied: its head slot is the (unmaterialised) garbage slot
        head_id = 0u;
        head_dep = dep_new;
      } else if (!exact && n == 0) {   // a clean row emptied by the pop of the agent it has just received: a dead slot, zero
        head_id = 0u;
        head_dep = 0.0f;
      } else {
        const SlotRec hd = slot_load(sl + SLW * hoff);
        head_id = (uint32_t)(long long)hd.id;
        head_dep = hd.dep;
      }
      // the agents that stay keep their order: the tail is who it was (the arrival, or the tail word's id) unless nobody
      // stays. (A count at Nmax is outside the domain and flagged; the store is re-read there as the reference would.)
      if (n == 0)
        tail_id = 0u;
      else if (n >= Nmax)
        tail_id = (n == Nmax) ? (uint32_t)(long long)sl[SLW * phys(hoff, n - 1, Nmax)] : 0u;
    }
    glob(&fb.hdp[row]) = make_uint2((head_id << 8) | (uint32_t)n | (exact ? HD_DIRTY : 0u), __float_as_uint(head_dep));
    glob(&fb.tl[row]) = tl_word(tail_id, hoff, TLF_AUTH);
    if (out.write_gc || b < (uint32_t)out.m_env) glob(&fb.gc8[row]) = (uint8_t)r1_code(lazy ? q : -1);
    // per-node count before insertion (the insert kernel adds this frame's arrivals)
    if (out.counts8 && c > 0) out.counts8[row] = (uint8_t)n;      // (phase A stored ni - pop for this row already)
    if (FAPI && out.countsf) out.countsf[row] = (float)n;
    if (FAPI && out.popped) out.popped[(int64_t)b * N + i] = pop ? 1 : 0;
    if (FAPI && out.withdrawn) out.withdrawn[(int64_t)b * N + i] = c > 0 ? 1 : 0;
    if (out.events && b < out.m_env) out.events[(int64_t)i * out.m_env + b] = (uint8_t)((pop ? 1 : 0) | (c > 0 ? 2 : 0));
    return make_float2((float)n, (float)c);
  }
}

// NCH rows per lane: ALL their loads (dense words, downstream post words) are issued before the first row is processed,
// so a wave keeps 8 * NCH independent requests in flight instead of one row's dependent phases.
// SIB (NCH == 4): the chunk's rows come from the plan's row-chunk table — rows with the same ordered out-edge target list,
// on a road network the roads that ENTER one intersection — so their four downstream post words are gathered ONCE per
// chunk instead of once per row (those gathers were a quarter of the pass's reads once a frame's words no longer fit the
// Infinity Cache: 20 -> 8 post requests per lane and chunk; 923 -> 691 MB read per launch at 16 384 environments, same
// time: the pass is not bound by its reads). Same rows, same arithmetic, another visiting order.
// Measured and rejected in round 3: the event path as a launch of its own over lists in global memory
// (158 + 94 us instead of 236: its stores then hit lines that have left the L2, and a partial-line store to a cold line is a
// read-modify-write at the memory side, profiles/r03_pmc_calibration.txt); a list for every pair and no in-place fall-back
// (no spilled register left, 18 KB of LDS: 250 us); the event path's pointers and statics through a block in LDS with
// further list rounds instead of the in-place fall-back (no spilled SGPR, 7 KB: 275 us); the pop's two slot reads requested
// before anything is stored (same time).
struct __attribute__((aligned(32))) RowChunk {
  int32_t row[4];    // -1: none (a group's remainder)
  int32_t out4[4];   // the shared first four out-edge targets
};
template <int NCH, bool SIB, bool FAPI, bool O32>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fused_rows(const NodeRec* __restrict__ nodes,
                                                     const int32_t* __restrict__ out_pad,
                                                     const int32_t* __restrict__ out_ptr,
                                                     const int32_t* __restrict__ out_dst,
                                                     const RowChunk* __restrict__ rchunks,
                                                     const uint32_t* __restrict__ post, int Nmax, uint32_t B, uint32_t N,
                                                     const FusedBufs* __restrict__ fbp, float* __restrict__ ag, int64_t A,
                                                     int64_t a_bstride, float t, FrameOut out) {
  // The table of pointers lives in device memory (tarl_fused.bufs_dev, written by k_set_bufs at the head of the call): what
  // the pass needs of it is read where it is needed, through the scalar cache, instead of travelling as 27 kernel arguments
  // that the register allocator keeps alive across the whole pass (round 5, static figures of tools/kernel_resources.sh for
  // this instantiation: 45 -> 13 spilled SGPRs, 173 -> 48 v_readlane / v_writelane, 1 135 -> 1 029 vector instructions).
  const FusedBufs& fb = *fbp;
  static_assert(!SIB || NCH == 4, "row chunks hold four rows");
  __shared__ int32_t s_cnt;
  // the event list holds EV_CAP of the TILE * NCH pairs (a filling network lists ~2 %, a loaded one ~30 %); a pair that
  // finds it full runs its event path in place. 7 KB instead of 18: the workgroups a CU holds are bounded by its wave
  // slots, not by LDS, and the waves that have no list entry leave early
#ifndef TARL_EV_CAP
#define TARL_EV_CAP 384      // (developer override through `make variant EXPFLAGS=-DTARL_EV_CAP=...`: 512 and 768 measure the same)
#endif
  constexpr int EV_CAP = TARL_EV_CAP;
  __shared__ uint16_t s_item[EV_CAP];       // (row offset in the chunk) << 9 | pop << 8 | lane
  __shared__ uint4 s_words[EV_CAP];         // the listed row's {post word, hd, head_dep bits, tl}
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = b < B;
  // the chunk's rows (wave-uniform): consecutive, or the table's
  int32_t ri[NCH];
  bool live[NCH];
  if (SIB) {
    const RowChunk& rc = rchunks[blockIdx.y];
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      live[r] = rc.row[r] >= 0;
      ri[r] = live[r] ? rc.row[r] : rc.row[0];   // a missing row is loaded as the first one and never used
    }
  } else {
    const uint32_t i0 = blockIdx.y * NCH;
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      live[r] = i0 + r < N;
      ri[r] = live[r] ? (int32_t)(i0 + r) : (int32_t)(N - 1);   // clamped: the tail rows are loaded twice, used once
    }
  }
  RowStat rs[NCH];
#pragma unroll
  for (int r = 0; r < NCH; ++r) {
    const NodeRec& nr = nodes[ri[r]];
    rs[r] = RowStat{nr.out_deg, nr.out0, nr.tt0, nr.maxn};
  }
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  float nsum = 0.0f;
  if (valid) {
    uint32_t pa[NCH], tlw[NCH], pj[NCH][4];
    uint2 hp[NCH];
    uint32_t ovf = 0u;       // bit r: row r found the event list full; bit 4 + r: its pop flag
    // (the rows' own post words in front of the downstream ones: the second round below needs the former alone)
#pragma unroll
    for (int r = 0; r < NCH; ++r) pa[r] = at32<O32>(post, (uint32_t)ri[r] * B + b);
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      if (SIB) {
        if (r == 0) {
          const int32_t* od = rchunks[blockIdx.y].out4;
#pragma unroll
          for (int q = 0; q < 4; ++q) pj[0][q] = at32<O32>(post, (uint32_t)od[q] * B + b);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) pj[r][q] = pj[0][q];
        }
      } else {
        const int32_t* od = nodes[ri[r]].out4;   // the first four targets travel in the node record
#pragma unroll
        for (int q = 0; q < 4; ++q) pj[r][q] = at32<O32>(post, (uint32_t)od[q] * B + b);
      }
    }
    // The post word already says whether the row holds anybody (PF_NONEMPTY), receives somebody (PF_ARRIVED) or still
    // carries the flag of an event in its tail word (PF_TLAUTH). A row with none of the three is empty and idle: its
    // head words are {0, unused} and its tail word is flag-free whatever its stale tail id — they are not fetched. In a
    // filling network that is most rows; the second round of loads only touches the sectors of the others.
#pragma unroll
    for (int r = 0; r < NCH; ++r) {
      const uint32_t row = (uint32_t)ri[r] * B + b;
      hp[r] = make_uint2(0u, 0u);
      tlw[r] = 0u;
      if (Nmax < 2 || (pa[r] & (PF_ARRIVED | PF_NONEMPTY | PF_TLAUTH))) {   // (a one-slot FIFO has no lazy garbage slot)
        hp[r] = gat<O32>(fb.hdp, row);
        tlw[r] = gat<O32>(fb.tl, row);
      }
    }
#pragma unroll
    for (int r = 0; r < NCH; ++r)
      if (live[r]) {
        bool pop;
        float n = 0.0f;
        const uint32_t i = (uint32_t)ri[r];
        const bool ev = row_phase_a<FAPI, O32>(i, b, rs[r], post, pa[r], hp[r], tlw[r], pj[r], Nmax, B, N, fb, A, t, out, &pop, &n);
        nsum += n;
        if (ev) {
          const int32_t pos = atomicAdd(&s_cnt, 1);
          if (pos < EV_CAP) {
            s_item[pos] = (uint16_t)((r << 9) | (pop ? 256 : 0) | threadIdx.x);
            s_words[pos] = make_uint4(pa[r], hp[r].x, hp[r].y, tlw[r]);
          } else {
            ovf |= (1u << r) | (pop ? (16u << r) : 0u);   // the list is full: served in place below
          }
        }
      }
    // In-place fall-back for the pairs that found the list full (a loaded network; never in a filling one). ONE rolled copy
    // of the event path behind the four rows, not one inside each row's body: with four inlined copies the idle path
    // carried their registers and 145 spilled SGPRs (row pass 222 -> 208 us without them, timing-only build).
    if (ovf != 0u) {
#pragma unroll 1
      for (int r = 0; r < NCH; ++r) {
        if (!((ovf >> r) & 1u)) continue;
        uint32_t pa_r = pa[0], tl_r = tlw[0];
        uint2 hp_r = hp[0];
        int32_t i_r = ri[0];
#pragma unroll
        for (int q = 1; q < NCH; ++q) {
          pa_r = (r == q) ? pa[q] : pa_r;
          tl_r = (r == q) ? tlw[q] : tl_r;
          hp_r.x = (r == q) ? hp[q].x : hp_r.x;
          hp_r.y = (r == q) ? hp[q].y : hp_r.y;
          i_r = (r == q) ? ri[q] : i_r;
        }
        const float2 nc = row_phase_b<FAPI>((uint32_t)i_r, b, ((ovf >> (4 + r)) & 1u) != 0u, pa_r, hp_r, tl_r, nodes[i_r], out_ptr,
                                      out_dst, Nmax, B, N, fb, ag, A, a_bstride, t, out);
        nsum -= nc.y;
        if (nc.y != 0.0f) glob(&fb.acc_w[(int64_t)(blockIdx.y % (unsigned)fb.acc_slots) * B + b]).atomic_add(nc.y);
      }
    }
  }
  // idle rows' share of the environment's count sum goes out now: a wave without a list entry is done after the barrier
  // (its slots go to the next workgroup while the event path, a chain of dependent loads a few lanes wide, runs on)
  const int64_t bank0 = (int64_t)(blockIdx.y % (unsigned)fb.acc_slots) * B;
  if (valid && nsum != 0.0f) glob(&fb.acc_n[bank0 + b]).atomic_add(nsum);
  __syncthreads();
  const int32_t cnt = s_cnt < EV_CAP ? s_cnt : EV_CAP;
  for (int32_t idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
    const uint32_t item = s_item[idx];
    const uint32_t r = item >> 9, lane2 = item & 255u;
    const uint4 wd = s_words[idx];
    const uint32_t b2 = blockIdx.x * blockDim.x + lane2;
    int32_t i2 = ri[0];
#pragma unroll
    for (int q = 1; q < NCH; ++q) i2 = (r == (uint32_t)q) ? ri[q] : i2;
    const float2 nc = row_phase_b<FAPI>((uint32_t)i2, b2, (item & 256u) != 0u, wd.x, make_uint2(wd.y, wd.z), wd.w, nodes[i2],
                                  out_ptr, out_dst, Nmax, B, N, fb, ag, A, a_bstride, t, out);
    if (nc.y != 0.0f) {      // withdrawn agents leave the count sum (small integers: exact in fp32 in any order)
      glob(&fb.acc_n[bank0 + b2]).atomic_add(-nc.y);
      glob(&fb.acc_w[bank0 + b2]).atomic_add(nc.y);
    }
  }
}

// rows per lane of the row pass (TARL_NCHUNK = 1, 2 or 4); on a graph whose rows group by their out-edge targets (plan
// row_siblings) the four-row form walks the plan's row-chunk table instead of consecutive rows (TARL_ROWS_SIBLINGS=0 keeps
// the consecutive chunks: developer knob)
static bool rows_sib(const tarl_plan* plan) {
  return env_flag_on("TARL_ROWS_SIBLINGS") && nchunk_rows() == 4 && plan->row_siblings && plan->row_chunks;
}
static int64_t num_row_chunks(const tarl_plan* plan) { return rows_sib(plan) ? plan->num_row_chunks : num_chunks(plan); }
int tarl_launch_rows(dim3 grid, unsigned threads, hipStream_t s, const tarl_plan* plan, const tarl_fused* f,
                     const FusedBufs* fb, int Nmax, int64_t B, float* agent_features, int64_t A, int64_t a_bstride,
                     float time, const FrameOut& out) {
#define ROWS_LAUNCH_(NCH, SIB, FAPI, O32)                                                                                  \
  hipLaunchKernelGGL((k_fused_rows<NCH, SIB, FAPI, O32>), grid, dim3(threads), 0, s, (const NodeRec*)f->node_rec,               \
                     (const int32_t*)f->out_pad, plan->out_ptr, plan->out_dst, (const RowChunk*)plan->row_chunks,         \
                     (const uint32_t*)f->post, Nmax, (uint32_t)B, (uint32_t)plan->N, fb, agent_features, A, a_bstride,    \
                     time, out)
#define ROWS_LAUNCH(NCH, SIB)                                                                                              \
  do {                                                                                                                     \
    if (fapi) {                                                                                                            \
      ROWS_LAUNCH_(NCH, SIB, true, false);                                                                                 \
    } else if (o32) {                                                                                                      \
      ROWS_LAUNCH_(NCH, SIB, false, true);                                                                                 \
    } else {                                                                                                               \
      ROWS_LAUNCH_(NCH, SIB, false, false);                                                                                \
    }                                                                                                                      \
  } while (0)
  const bool fapi = out.countsf || out.popped || out.withdrawn;
  const bool o32 = addr32_ok() && plan->N * B < ((int64_t)1 << 29);   // 8-byte words through 32-bit byte offsets
  grid.y = (unsigned)num_row_chunks(plan);
  switch (nchunk_rows()) {
    case 1: ROWS_LAUNCH(1, false); break;
    case 2: ROWS_LAUNCH(2, false); break;
    default:
      if (rows_sib(plan)) {
        ROWS_LAUNCH(4, true);
      } else {
        ROWS_LAUNCH(4, false);
      }
      break;
  }
#undef ROWS_LAUNCH
#undef ROWS_LAUNCH_
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
