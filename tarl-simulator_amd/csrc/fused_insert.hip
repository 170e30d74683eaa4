// fused_insert.hip — the insert kernels of a frame (insert + reward + log-prob reduction: one workgroup per environment, several
// environments per wave, and the merged insert + choice launch) and their launch dispatch. (Design: fused_frame.h.)
#include "fused_choice.h"

// ---- insert + reward + log-prob reduction (one wave per environment) -----------------------------------------------------
// The accumulator banks (tarl_fused.acc_lp / acc_n / acc_w, [acc_slots][B], bank = blockIdx.y % acc_slots of the writer):
//   acc_n  (fp32)   the row pass: the frame's count sum, one coalesced atomic per lane and workgroup; every mode, every frame
//   acc_w  (fp32)   the row pass: agents withdrawn in the frame (its event rows; zero for most (bank, environment) pairs)
//   acc_lp (int64)  the per-frame choice (fused_choice_body: k_fused_choice, the choice role of k_fused_insert_choice), and
//                   only when the caller asked for a log-prob (want_lp): the frame API, TARL_ROLLOUT_MERGE = 0 and 1 (mode 1
//                   alternates between acc_lp and the caller's acc_scratch by frame parity). The all-frames draw of mode 2
//                   (k_fused_choice_all) and the state-dependent heads write the log-prob themselves and never touch it.
// RULE: every bank holds zero bits on entry to and on exit from every call, in every mode. The insert launch of a frame is
// the banks' only reader; it re-arms what it read, and only where the value loaded was not zero already. It reads acc_lp
// exactly where the same call's choice filled it — where its log_prob pointer is not null (template parameter LP, chosen by
// launch_insert from the pointer) — so a launch without a log-prob finds acc_lp zero and leaves it alone. An environment of
// the packed kernel that goes to the one-environment body afterwards has its banks reduced and re-armed there, once.
// The sums are exact in any order (small integers in fp32, fixed point in int64): acc_slots changes no result.
__device__ __forceinline__ bool fused_target(const FusedBufs& fb, PlanOut P, const uint8_t* __restrict__ sel8, int64_t b,
                                             int64_t B, int64_t N, int32_t origin, int32_t* road, int32_t* cap) {
  if (origin < 0 || origin >= N) return false;
  const int64_t orow = (int64_t)origin * B + b;
  const uint32_t c = sel8[orow] & 0x7Fu;
  const long long r = (long long)(c == SEL_RAW ? (float)glob(&fb.sel[orow]) : (float)P.out_dst[P.out_ptr[origin] + (int32_t)c]);
  if (r < 0 || r >= N) return false;
  const float maxn = glob(&fb.st0[r].x);
  const uint32_t hd = glob(&fb.hdp[r * B + b].x);
  const long long room = (long long)(maxn - TARL_CONGESTION_FILE - (float)(hd & HD_CNT));
  *road = (int32_t)r;
  *cap = (int32_t)(room > 0x7fffffff ? 0x7fffffff : room);
  return room > 0;
}

// The same test with the words the admission phase needs afterwards: the target row's count word and tail word come back
// with it (they are stashed beside the candidate, so that phase reads nothing dynamic again), and a rank below four
// resolves through the origin's node record (one round: the record and the SELECTED_ROAD byte travel together)
// instead of out_ptr -> out_dst (two).
__device__ __forceinline__ bool fused_target_words(const FusedBufs& fb, PlanOut P, const uint8_t* __restrict__ sel8,
                                                   int64_t b, int64_t B, int64_t N, int32_t origin, int32_t* road,
                                                   uint32_t* hd_out, uint32_t* tl_out) {
  if (origin < 0 || origin >= N) return false;
  const int64_t orow = (int64_t)origin * B + b;
  const uint32_t c = sel8[orow] & 0x7Fu;
  const int32_t* o4 = fb.nodes[origin].out4;
  const int32_t t0 = glob(o4), t1 = glob(o4 + 1), t2 = glob(o4 + 2), t3 = glob(o4 + 3);
  long long r;
  if (c < 4u)
    r = (long long)(float)(c == 0u ? t0 : (c == 1u ? t1 : (c == 2u ? t2 : t3)));
  else
    r = (long long)(c == SEL_RAW ? (float)glob(&fb.sel[orow]) : (float)P.out_dst[P.out_ptr[origin] + (int32_t)c]);
  if (r < 0 || r >= N) return false;
  const uint32_t hd = glob(&fb.hdp[r * B + b].x);
  *tl_out = glob(&fb.tl[r * B + b]);
  const float maxn = glob(&fb.st0[r].x);
  const long long room = (long long)(maxn - TARL_CONGESTION_FILE - (float)(hd & HD_CNT));
  *road = (int32_t)r;
  *hd_out = hd;
  return room > 0;
}

// The insert kernels' LDS block (one per workgroup; the one-environment body and the two-environment kernel share it, so
// that the latter's rare fall-back into the former costs no second block: 3.9 KB, 41 workgroups per CU)
struct InsLds {
  int32_t wave[INSB / 64];
  int32_t cnt, adm, lo;
  int32_t cnt2[8], adm2[8], lo2[8];   // k_fused_insert2: one set per environment of the wave
  int32_t un_agent[INS_CAP], un_road[INS_CAP], un_k[INS_CAP];
  uint32_t un_hd[INS_CAP], un_tl[INS_CAP];
};

// The per-entry step of the departure window (a_order + a_win), in two halves: between them sits the cursor update, which the
// one-environment body shares with its sequential-departure path. The load: ONE pair of independent loads, the {departure,
// origin, agent} record and the "already inserted" byte.
__device__ __forceinline__ void insert_window_load(const FusedBufs& fb, int64_t b, int64_t A, int64_t k, float t, bool* due,
                                                   bool* waiting, int32_t* origin, int32_t* a) {
  const uint4 w = glob(&fb.a_win[b * A + k]);
  const uint8_t ins = glob(&fb.a_ins[b * A + k]);
  *waiting = ins == 0;
  *due = __uint_as_float(w.x) <= t;
  *origin = (int32_t)w.y;
  *a = (int32_t)w.z;
}
// The append: a due, waiting entry whose target road has room goes, unordered and with the target row's words, into the `cap`
// list entries at `base` (counted in *cnt beyond cap: the caller then takes another path). sel8 carries no __restrict__ here:
// with it the merged kernel's SGPR count moves (tools/kernel_resources.sh), and the callers' parameters already say it.
__device__ __forceinline__ void insert_window_append(InsLds& L, int base, int cap, int32_t* cnt, const FusedBufs& fb, PlanOut P,
                                                     const uint8_t* sel8, int64_t b, int64_t B, int64_t N, int64_t k,
                                                     int32_t origin, int32_t a) {
  int32_t road = 0;
  uint32_t hdw = 0u, tlw = 0u;
  if (fused_target_words(fb, P, sel8, b, B, N, origin, &road, &hdw, &tlw)) {
    const int32_t pos = atomicAdd(cnt, 1);
    if (pos < cap) {
      L.un_agent[base + pos] = a;
      L.un_road[base + pos] = road;
      L.un_k[base + pos] = (int32_t)k;
      L.un_hd[base + pos] = hdw;
      L.un_tl[base + pos] = tlw;
    }
  }
}

// Admission straight from the LDS list (window path; entries base .. base + Lc, this lane takes first, first + stride, ...):
// a candidate's rank on its road is the number of candidates for the same road with a smaller agent id (the reference admits
// in stable agent-id order), so the list needs no sorting, and the target row's words were stashed with it: nothing dynamic
// is read here. The rank-0 candidate of a road owns its count word (the head too when the road was empty), event word and
// count outputs; the last admitted owns the tail. *adm: the environment's admitted agents (LDS).
__device__ __forceinline__ void insert_admit_list(const InsLds& L, int base, int32_t Lc, int first, int stride, int32_t* adm,
                                                  const FusedBufs& fb, float* __restrict__ agb, int64_t b, int64_t B, int64_t A,
                                                  int Nmax, int use_cong, float t, const FrameOut& out) {
  for (int32_t idx = first; idx < Lc; idx += stride) {
    const int32_t r = L.un_road[base + idx];
    const int32_t a = L.un_agent[base + idx];
    int32_t rank = 0, total = 0;
    for (int32_t k = 0; k < Lc; ++k) {
      const bool same = L.un_road[base + k] == r;
      total += same ? 1 : 0;
      rank += (same && L.un_agent[base + k] < a) ? 1 : 0;
    }
    const int64_t rrow = (int64_t)r * B + b;
    const float4 str = glob(&fb.st0[r]);
    const uint32_t hd = L.un_hd[base + idx];
    const uint32_t n0i = hd & HD_CNT;
    const float n0 = (float)n0i;
    const long long cap = (long long)(str.x - TARL_CONGESTION_FILE - n0);
    if (rank < cap) {
      const long long m = total < cap ? total : cap;  // arrivals admitted on this road
      const long long slot = (long long)n0i + rank;
      const float t_cong = use_cong ? str.w / (str.x + 10.0f - n0) : 0.0f;
      const float tt = (t_cong != t_cong) ? t_cong : fmaxf(str.y, t_cong);
      const int hoff = tl_hoff(L.un_tl[base + idx]);
      if (slot >= 0 && slot < Nmax) {
        slot_store(gbase(fb.slots) + rrow * fb.lds + SLW * phys(hoff, (int)slot, Nmax), (float)a, t, t + tt);
      }
      agb[(int64_t)a * AG_COLS + AG_ON_WAY] = 1.0f;
      glob(&fb.a_status[b * A + a]) = (uint8_t)1;
      glob(&fb.a_ins[b * A + L.un_k[base + idx]]) = (uint8_t)1;
      if (rank == m - 1) glob(&fb.tl[rrow]) = tl_word((uint32_t)a, hoff, TLF_AUTH);  // new tail; gc8 authoritative from here on
      if (rank == 0) {
        const uint32_t cnt = n0i + (uint32_t)m;      // n0 + m <= MAX - 3 < 255
        if (n0i == 0u) {   // new head: id + departure, arrival
          glob(&fb.hdp[rrow]) = make_uint2(((uint32_t)a << 8) | cnt | (hd & HD_DIRTY), __float_as_uint(t + tt));
        } else {
          glob(&fb.hdp[rrow].x) = hd + (uint32_t)m;
        }
        if (out.write_gc || b < out.m_env) glob(&fb.gc8[rrow]) = (uint8_t)r1_code(-1);   // the arrivals overwrote a pending garbage slot: none pending now
        if (out.counts8) out.counts8[rrow] = (uint8_t)cnt;
        if (out.countsf) out.countsf[rrow] = (float)cnt;
        atomicAdd(adm, (int32_t)m);
      }
    }
  }
}

template <bool LP>
__device__ __forceinline__ void fused_insert_body(InsLds& L, int64_t b, int Nmax, int64_t B, int64_t N, const FusedBufs& fb, PlanOut P,
                                                  const uint8_t* __restrict__ sel8, float* __restrict__ ag, int64_t A,
                                                  int64_t a_bstride, int use_cong, float t,
                                                  int32_t* __restrict__ scratch, const float* __restrict__ entropy_in,
                                                  float* __restrict__ reward, FrameOut out,
                                                  float* __restrict__ log_prob, float* __restrict__ entropy) {
  // (window path: un_k = the candidate's position in the departure order, un_hd / un_tl = its target row's count / tail words)
  float* agb = ag + b * a_bstride;
  int32_t* cand_agent = scratch + b * 2 * A;
  int32_t* cand_road = cand_agent + A;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // phase 1: candidates (ready agent whose target road has room). Candidates are rare (a handful per frame), so they
  // are appended unordered to an LDS list with an atomic counter and then ranked by agent id (deterministic: the
  // reference admits agents in stable agent-id order). A backlog larger than the LDS list falls back to the ordered
  // ballot compaction into the global scratch.
  if (tid == 0) {
    L.cnt = 0;
    L.adm = 0;
  }
  // the frame's accumulator banks (filled by the choice kernel and the row pass, complete before this launch) depend on
  // nothing below: they are requested first and reduced last. A bank is re-armed only where it does not already hold
  // zero bits; the log-prob banks are neither read nor written without LP (nobody filled them: see the section header)
  long long lpf = 0;
  float nf = 0.0f, wf = 0.0f;
  if (wid == 0) {
    for (int64_t sl_ = lane; sl_ < fb.acc_slots; sl_ += 64) {
      const float n = glob(&fb.acc_n[sl_ * B + b]), w = glob(&fb.acc_w[sl_ * B + b]);
      long long v = 0;
      if constexpr (LP) v = glob(&fb.acc_lp[sl_ * B + b]);
      nf += n;
      wf += w;
      lpf += v;
      if (__float_as_uint(n) != 0u) glob(&fb.acc_n[sl_ * B + b]) = 0.0f;
      if (__float_as_uint(w) != 0u) glob(&fb.acc_w[sl_ * B + b]) = 0.0f;
      if constexpr (LP) {
        if (v != 0) glob(&fb.acc_lp[sl_ * B + b]) = 0ll;
      }
    }
  }
  __syncthreads();
  if (fb.a_order) {
    // Windowed scan: agents sorted by departure time; everything before cur_lo is known not to be waiting any more and
    // everything after the first not-yet-due entry is not due either, so a frame normally looks at one chunk.
    const auto ord = gbase(fb.a_order) + b * A;
    const auto dsort = gbase(fb.a_dep_sorted) + b * A;
    const int32_t lo = glob(&fb.cur_lo[b]);
    if (tid == 0) L.lo = 0x7fffffff;
    __syncthreads();
    for (int64_t k0 = lo; k0 < A; k0 += INSB) {
      const int64_t k = k0 + tid;
      bool notdue = false;
      if (k < A) {
        bool due, waiting;
        int32_t a, origin;
        if (fb.a_win) {
          insert_window_load(fb, b, A, k, t, &due, &waiting, &origin, &a);
        } else {            // sequential departures; per-agent arrays only for entries that are due
          due = dsort[k] <= t;
          a = due ? ord[k] : 0;
          waiting = due && gbase(fb.a_status)[b * A + a] == 0;
          origin = waiting ? gbase(fb.a_origin)[b * A + a] : 0;
        }
        notdue = !due;
        if (!due) {
          atomicMin(&L.lo, (int32_t)k);          // the cursor may not pass this entry
        } else if (waiting) {
          atomicMin(&L.lo, (int32_t)k);
          int32_t road = 0, cap = 0;
          if (fb.a_win) {
            insert_window_append(L, 0, INS_CAP, &L.cnt, fb, P, sel8, b, B, N, k, origin, a);
          } else if (fused_target(fb, P, sel8, b, B, N, origin, &road, &cap)) {
            const int32_t pos = atomicAdd(&L.cnt, 1);
            if (pos < INS_CAP) {
              L.un_agent[pos] = a;
              L.un_road[pos] = road;
            }
          }
        }
      }
      if (__syncthreads_or(notdue ? 1 : 0)) break;   // sorted by departure: nothing beyond this chunk is due
    }
    __syncthreads();
    if (tid == 0) glob(&fb.cur_lo[b]) = L.lo == 0x7fffffff ? (int32_t)A : L.lo;
  } else {
    for (int64_t a0 = tid; a0 < A; a0 += 4 * INSB) {  // 4 independent (status, departure) loads in flight per thread
      uint8_t stt[4];
      float dp[4];
  #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t a = a0 + (int64_t)j * INSB;
        stt[j] = a < A ? gbase(fb.a_status)[b * A + a] : (uint8_t)1;
        dp[j] = a < A ? gbase(fb.a_dep)[b * A + a] : 0.0f;
      }
  #pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (stt[j] == 0 && dp[j] <= t) {
          const int64_t a = a0 + (int64_t)j * INSB;
          int32_t road = 0, cap = 0;
          if (fused_target(fb, P, sel8, b, B, N, gbase(fb.a_origin)[b * A + a], &road, &cap)) {
            const int32_t pos = atomicAdd(&L.cnt, 1);
            if (pos < INS_CAP) {
              L.un_agent[pos] = (int32_t)a;
              L.un_road[pos] = road;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  int32_t Lc = L.cnt;
  const bool stashed = fb.a_order && fb.a_win && Lc <= INS_CAP;
  if (stashed) {   // the window path with its list in LDS: admission straight from it
    insert_admit_list(L, 0, Lc, tid, INSB, &L.adm, fb, agb, b, B, A, Nmax, use_cong, t, out);
    __syncthreads();
  } else {
  if (Lc <= INS_CAP) {
    for (int32_t idx = tid; idx < Lc; idx += INSB) {
      const int32_t a = L.un_agent[idx];
      int32_t pos = 0;
      for (int32_t k = 0; k < Lc; ++k) pos += (L.un_agent[k] < a) ? 1 : 0;
      cand_agent[pos] = a;
      cand_road[pos] = L.un_road[idx];
    }
    __threadfence_block();
    __syncthreads();
  } else {
    int32_t basec = 0;
    for (int64_t a0 = 0; a0 < A; a0 += INSB) {
      const int64_t a = a0 + tid;
      bool cnd = false;
      int32_t road = 0, cap = 0;
      if (a < A && gbase(fb.a_status)[b * A + a] == 0 && gbase(fb.a_dep)[b * A + a] <= t)
        cnd = fused_target(fb, P, sel8, b, B, N, gbase(fb.a_origin)[b * A + a], &road, &cap);
      const unsigned long long bal = __ballot(cnd);
      const int lane_off = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) L.wave[wid] = __popcll(bal);
      __syncthreads();
      int32_t wbase = 0, tot = 0;
      for (int w = 0; w < INSB / 64; ++w) {
        const int32_t v = L.wave[w];
        if (w < wid) wbase += v;
        tot += v;
      }
      if (cnd) {
        cand_agent[basec + wbase + lane_off] = (int32_t)a;
        cand_road[basec + wbase + lane_off] = road;
      }
      basec += tot;
      __syncthreads();
    }
    Lc = basec;
    __threadfence_block();
    __syncthreads();
  }

  // phase 2: rank within road (stable), admit the first min(count, capacity), write slots / dense words.
  // Per admitted road: the rank-0 candidate owns hdp / gc8 (the count's byte of hd is committed after the barrier), the
  // last admitted candidate owns tl. Everybody else only READS the count byte, which nobody changes in this phase.
  for (int32_t idx = tid; idx < Lc; idx += INSB) {
    const int32_t r = cand_road[idx];
    const int32_t a = cand_agent[idx];
    int32_t rank = 0, total = 0;
    for (int32_t k = 0; k < Lc; ++k) {
      const bool same = cand_road[k] == r;
      total += same ? 1 : 0;
      rank += (same && k < idx) ? 1 : 0;
    }
    const int64_t rrow = (int64_t)r * B + b;
    const float4 str = glob(&fb.st0[r]);
    const uint32_t hd = glob(&fb.hdp[rrow].x);
    const uint32_t n0i = hd & HD_CNT;
    const float n0 = (float)n0i;
    const long long cap = (long long)(str.x - TARL_CONGESTION_FILE - n0);
    int32_t commit = 0;
    if (rank < cap) {
      const long long m = total < cap ? total : cap;  // arrivals admitted on this road
      const long long slot = (long long)n0i + rank;
      const float t_cong = use_cong ? str.w / (str.x + 10.0f - n0) : 0.0f;
      const float tt = (t_cong != t_cong) ? t_cong : fmaxf(str.y, t_cong);
      const int hoff = tl_hoff(glob(&fb.tl[rrow]));   // the tail word's owner below rewrites it with the same offset
      if (slot >= 0 && slot < Nmax) {
        slot_store(gbase(fb.slots) + rrow * fb.lds + SLW * phys(hoff, (int)slot, Nmax), (float)a, t, t + tt);
      }
      agb[(int64_t)a * AG_COLS + AG_ON_WAY] = 1.0f;
      glob(&fb.a_status[b * A + a]) = (uint8_t)1;
      if (fb.a_ins) gbase(fb.a_ins)[b * A + gbase(fb.a_rank)[b * A + a]] = 1;
      if (rank == 0 && n0i == 0u) {   // new head: id + departure (count byte unchanged), arrival
        glob(&fb.hdp[rrow]) = make_uint2(((uint32_t)a << 8) | n0i | (hd & HD_DIRTY), __float_as_uint(t + tt));
      }
      if (rank == m - 1) glob(&fb.tl[rrow]) = tl_word((uint32_t)a, hoff, TLF_AUTH);  // new tail; gc8 authoritative from here on
      if (rank == 0) commit = (int32_t)m;
    }
    cand_agent[idx] = commit;
  }
  __threadfence_block();
  __syncthreads();
  // phase 3: commit the counters; the arrivals overwrote a pending garbage slot: no garbage pending, keep the head offset
  for (int32_t idx = tid; idx < Lc; idx += INSB) {
    const int32_t cmt = cand_agent[idx];
    if (cmt > 0) {
      const int64_t rrow = (int64_t)cand_road[idx] * B + b;
      if (out.write_gc || b < out.m_env) glob(&fb.gc8[rrow]) = (uint8_t)r1_code(-1);
      const uint32_t hd = glob(&fb.hdp[rrow].x) + (uint32_t)cmt;   // count byte: n0 + cmt <= MAX - 3 < 255
      glob(&fb.hdp[rrow].x) = hd;
      if (out.counts8) out.counts8[rrow] = (uint8_t)(hd & HD_CNT);
      if (out.countsf) out.countsf[rrow] = (float)(hd & HD_CNT);
      atomicAdd(&L.adm, cmt);
    }
  }
  __syncthreads();
  }
  // phase 4: the frame's accumulator banks (requested at the top) -> reward, log-prob
  if (wid == 0) {
    for (int off = 32; off > 0; off >>= 1) {
      if constexpr (LP) lpf += __shfl_down(lpf, off);
      nf += __shfl_down(nf, off);      // sums of small integers: exact in fp32 in any order
      wf += __shfl_down(wf, off);
    }
    if (lane == 0) {
      if (reward) reward[b] = -(nf + (float)L.adm);
      if constexpr (LP) {
        if (log_prob) log_prob[b] = (lpf < -(1ll << 49)) ? -INFINITY : (float)((double)lpf / LP_FIX);
      }
      if (entropy) entropy[b] = entropy_in[0];
      if (out.leg) {
        out.leg[2 * b + 0] = L.adm;
        out.leg[2 * b + 1] = (int32_t)wf;
      }
    }
  }
}

template <bool LP>
__global__ __launch_bounds__(INSB) void k_fused_insert(int Nmax, int64_t B, int64_t N, const FusedBufs* __restrict__ fbp, PlanOut P,
                                                       const uint8_t* __restrict__ sel8, float* __restrict__ ag,
                                                       int64_t A, int64_t a_bstride, int use_cong, float t,
                                                       int32_t* __restrict__ scratch,
                                                       const float* __restrict__ entropy_in,
                                                       float* __restrict__ reward, FrameOut out,
                                                       float* __restrict__ log_prob, float* __restrict__ entropy) {
  __shared__ InsLds L;
  fused_insert_body<LP>(L, blockIdx.x, Nmax, B, N, *fbp, P, sel8, ag, A, a_bstride, use_cong, t, scratch, entropy_in, reward,
                    out, log_prob, entropy);
}

// SEVERAL environments per wave (EPW = 2, 4 or 8: 32, 16 or 8 lanes each; chosen by the population size). With one wave per environment a
// launch of more than 8 192 environments does not fit the chip's wave slots and runs in two rounds of a latency chain —
// and below that, fewer waves walk the same chain faster (18 instead of 23 us at 4 096 environments). A frame's window
// chunk is a handful of entries and the accumulator banks are 32 wide, so a fraction of a wave does an environment's
// work as fast. Same phases, same order, same results as fused_insert_body on its departure-window path (a_order +
// a_win): scan from the cursor, candidates unordered in LDS (each environment its share of the block), admission by
// rank among the candidates of the same road. An environment with more candidates than its share of the list holds
// sits the packed part out and is handed, afterwards, to the one-environment body on the whole wave (which rescans from
// the cursor this kernel has already advanced — the same cursor it would have computed — and reduces the accumulator
// banks itself: nothing else of that environment has been written by then). 16 384 environments: 65 us with one wave
// each, 50 / 40 / 36 us with 2 / 4 / 8 per wave.
template <int EPW, bool LP>
__global__ __launch_bounds__(INSB) void k_fused_insert2(int Nmax, int64_t B, int64_t N, const FusedBufs* __restrict__ fbp, PlanOut P,
                                                        const uint8_t* __restrict__ sel8, float* __restrict__ ag,
                                                        int64_t A, int64_t a_bstride, int use_cong, float t,
                                                        int32_t* __restrict__ scratch,
                                                        const float* __restrict__ entropy_in,
                                                        float* __restrict__ reward, FrameOut out,
                                                        float* __restrict__ log_prob, float* __restrict__ entropy) {
  __shared__ InsLds L;
  const FusedBufs& fb = *fbp;              // the pointer table in device memory (k_set_bufs): 88 -> 38 spilled SGPRs at EPW = 8
  constexpr int LPE = 64 / EPW;            // lanes per environment
  constexpr int INS_CAP2 = INS_CAP / EPW;  // its share of the candidate list
  const int tid = threadIdx.x, h = tid / LPE, l = tid % LPE;
  const int64_t b0 = EPW * (int64_t)blockIdx.x, b = b0 + h;
  const bool live = b < B;
  const int base = h * INS_CAP2;
  if (l == 0) {
    L.cnt2[h] = 0;
    L.adm2[h] = 0;
    L.lo2[h] = 0x7fffffff;
  }
  // the frame's accumulator banks: requested first, consumed (and re-armed) only once the environment is known to stay
  // here. Bit i of a mask: the value this lane loaded in step i of the bank loop does not hold zero bits and must be
  // re-armed (steps beyond the mask's 32 bits are re-armed unconditionally). Without LP the log-prob banks are not touched.
  long long lpf = 0;
  float nf = 0.0f, wf = 0.0f;
  uint32_t nz_n = 0u, nz_w = 0u, nz_lp = 0u;
  if (live) {
    int it = 0;
    for (int64_t sl_ = l; sl_ < fb.acc_slots; sl_ += LPE, ++it) {
      const uint32_t bit = it < 32 ? (1u << it) : 0u;
      const float n = glob(&fb.acc_n[sl_ * B + b]), w = glob(&fb.acc_w[sl_ * B + b]);
      nf += n;
      wf += w;
      nz_n |= __float_as_uint(n) != 0u ? bit : 0u;
      nz_w |= __float_as_uint(w) != 0u ? bit : 0u;
      if constexpr (LP) {
        const long long v = glob(&fb.acc_lp[sl_ * B + b]);
        lpf += v;
        nz_lp |= v != 0 ? bit : 0u;
      }
    }
  }
  const int32_t lo = live ? gbase(fb.cur_lo)[b] : 0;
  __syncthreads();
  // phase 1: the departure window, LPE entries per environment and step
  bool done = !live;
  int64_t k0 = lo;
  if (live && k0 >= A) done = true;
  while (true) {
    bool notdue = false;
    if (!done) {
      const int64_t k = k0 + l;
      if (k < A) {
        bool due, waiting;
        int32_t origin, a;
        insert_window_load(fb, b, A, k, t, &due, &waiting, &origin, &a);
        notdue = !due;
        if (!due) {
          atomicMin(&L.lo2[h], (int32_t)k);          // the cursor may not pass this entry
        } else if (waiting) {
          atomicMin(&L.lo2[h], (int32_t)k);
          insert_window_append(L, base, INS_CAP2, &L.cnt2[h], fb, P, sel8, b, B, N, k, origin, a);
        }
      }
    }
    const unsigned long long nd = __ballot(notdue);
    if (!done) {
      if (((nd >> (LPE * h)) & ((1ull << LPE) - 1ull)) != 0ull || k0 + LPE >= A)
        done = true;       // sorted by departure: nothing beyond this chunk is due
      else
        k0 += LPE;
    }
    if (__ballot(!done) == 0ull) break;
  }
  __syncthreads();
  // an environment with more candidates than its share of the list holds sits this part out (nothing of it is written
  // but the cursor) and goes through the one-environment body afterwards
  bool over = false;
#pragma unroll
  for (int e = 0; e < EPW; ++e) over = over || (L.cnt2[e] > INS_CAP2);
  if (live && l == 0) glob(&fb.cur_lo[b]) = L.lo2[h] == 0x7fffffff ? (int32_t)A : L.lo2[h];
  const bool mine = live && L.cnt2[h] <= INS_CAP2;
  if (mine) {
    int it = 0;
    for (int64_t sl_ = l; sl_ < fb.acc_slots; sl_ += LPE, ++it) {   // the banks are consumed: re-arm what is not zero
      const uint32_t bit = it < 32 ? (1u << it) : 0u;
      if (bit == 0u || (nz_n & bit)) glob(&fb.acc_n[sl_ * B + b]) = 0.0f;
      if (bit == 0u || (nz_w & bit)) glob(&fb.acc_w[sl_ * B + b]) = 0.0f;
      if constexpr (LP) {
        if (bit == 0u || (nz_lp & bit)) glob(&fb.acc_lp[sl_ * B + b]) = 0ll;
      }
    }
    // phase 2: admission straight from the list, by rank among the candidates of the same road
    insert_admit_list(L, base, L.cnt2[h], l, LPE, &L.adm2[h], fb, ag + b * a_bstride, b, B, A, Nmax, use_cong, t, out);
  }
  __syncthreads();
  // phase 3: the accumulator banks -> reward, log-prob (LPE-lane reductions)
  for (int off = LPE / 2; off > 0; off >>= 1) {
    if constexpr (LP) lpf += __shfl_down(lpf, off, LPE);
    nf += __shfl_down(nf, off, LPE);      // sums of small integers: exact in fp32 in any order
    wf += __shfl_down(wf, off, LPE);
  }
  if (mine && l == 0) {
    if (reward) reward[b] = -(nf + (float)L.adm2[h]);
    if constexpr (LP) {
      if (log_prob) log_prob[b] = (lpf < -(1ll << 49)) ? -INFINITY : (float)((double)lpf / LP_FIX);
    }
    if (entropy) entropy[b] = entropy_in[0];
    if (out.leg) {
      out.leg[2 * b + 0] = L.adm2[h];
      out.leg[2 * b + 1] = (int32_t)wf;
    }
  }
  if (over) {   // wave-uniform, rare: the long backlogs, one environment after the other on the whole wave
    __syncthreads();
    for (int e = 0; e < EPW; ++e) {
      if (b0 + e < B && L.cnt2[e] > INS_CAP2)
        fused_insert_body<LP>(L, b0 + e, Nmax, B, N, fb, P, sel8, ag, A, a_bstride, use_cong, t, scratch, entropy_in, reward,
                          out, log_prob, entropy);
      __syncthreads();
    }
  }
}

// One launch, two roles (rollout steady state): the first B workgroups run frame t's insert (one wave each; the other
// three waves of such a workgroup retire at once, so its barriers only count the live wave), the remaining
// `choice_blocks` workgroups draw frame t+1's action into the NEXT slice of the action buffer and the other half of the
// double-buffered log-prob accumulators.
// The insert kernel is a latency chain that leaves the chip idle and the live policy's sample does not depend on the
// state, so the choice work rides in its shadow — without the cross-stream events that made a two-stream variant
// slower — and still completes right before the Direction kernel that consumes it (Infinity-Cache adjacency).
template <bool LP>
__global__ __launch_bounds__(TILE) void k_fused_insert_choice(ChoiceArgs C, int Nmax, int64_t B, int64_t N,
                                                              const FusedBufs* __restrict__ fbp,
                                                              PlanOut P, const uint8_t* __restrict__ sel8,
                                                              float* __restrict__ ag, int64_t A, int64_t a_bstride,
                                                              int use_cong, float t, int32_t* __restrict__ scratch,
                                                              const float* __restrict__ entropy_in,
                                                              float* __restrict__ reward, FrameOut out,
                                                              float* __restrict__ log_prob,
                                                              float* __restrict__ entropy) {
  // insert workgroups first: their dependent-load chains start at once and the choice workgroups fill the chip around them
  __shared__ InsLds L;
  if (blockIdx.x < (unsigned)B) {
    if (threadIdx.x >= INSB) return;   // whole waves leave before any barrier
    fused_insert_body<LP>(L, (int64_t)blockIdx.x, Nmax, B, N, *fbp, P, sel8, ag, A, a_bstride, use_cong, t, scratch, entropy_in,
                      reward, out, log_prob, entropy);
  } else {
    const unsigned cb = blockIdx.x - (unsigned)B;
    fused_choice_body(cb % C.gx, cb / C.gx, C.out_ptr, C.out_eid, C.group_of_node, C.G, B, N, C.acc_next, fbp->acc_slots,
                      C.thr, C.lgt, nullptr, C.pseed, C.pcounter, C.sel_next, sel8, nullptr, C.nchunk, C.want_lp, fbp->env_base);
  }
}

// Environments per wave of the packed insert kernel (k_fused_insert2; TARL_INSERT_EPW = 1, 2, 4 or 8 forces it; 1 = one
// workgroup per environment, k_fused_insert). A frame's window holds the agents due in it, and an environment's share of the
// wave (64 / EPW lanes, INS_CAP / EPW list entries) should take them in one step: an environment with more candidates than
// its share of the list sits the packed part out and is served alone afterwards, one after the other (measured with ~27 due
// per frame and EPW = 8: 260 us per launch instead of 36). With the schedule's due rate known (tarl_fused.due_rate, from
// pack): the largest EPW whose list share holds twice the expected candidates of a frame. Without it, by the size of the
// population: 8 up to 20 000 agents (BASELINE config 4: ~5 due per frame) when the launch is large, 4 up to 32 768, 2 up to
// 65 536, one wave per environment beyond (config 5: 262 144 agents, ~70 per frame).
int tarl_insert_envs_per_wave(const tarl_fused* f, int64_t A, int64_t B, int64_t T, const float* times_host) {
  const int epw_env = env_int("TARL_INSERT_EPW", 0);
  int epw = A <= 20000 && B >= 12288 ? 8 : (A <= 32768 ? 4 : (A <= 65536 ? 2 : 1));
  if (f->due_rate > 0.0f) {
    const float dt = T > 1 ? times_host[1] - times_host[0] : 1.0f;
    const float per_frame = f->due_rate * (dt > 0.0f ? dt : 1.0f);
    while (epw > 1 && 2.0f * per_frame > (float)(INS_CAP / epw)) epw >>= 1;
  }
  if (epw_env == 1 || epw_env == 2 || epw_env == 4 || epw_env == 8) epw = epw_env;
  return (env_flag_on("TARL_INSERT_PAIR") && f->a_order && f->a_win) ? epw : 1;
}

// the insert launch of a frame whose action is already in `sel_t` (no choice part): packed (epw = 2, 4 or 8 environments per
// wave) or one workgroup per environment
int tarl_launch_insert(int epw, hipStream_t s, int Nmax, int64_t B, int64_t N, const FusedBufs* fbt, PlanOut P,
                       const uint8_t* sel_t, float* agent_features, int64_t A, int64_t a_bstride, int use_cong, float time,
                       int32_t* ins_scratch, const float* entropy1, float* reward_t, const FrameOut& out, float* lp_t,
                       float* ent_t) {
  // the log-prob banks are part of the launch only where a log-prob is asked for (lp_t): a compile-time parameter, so the
  // 64-bit sum, its shuffles and its registers are not in the other instantiation at all
  using Kernel = decltype(&k_fused_insert<false>);   // the eight kernels take the same arguments
  static const Kernel kernels[2][4] = {
      {k_fused_insert<false>, k_fused_insert2<2, false>, k_fused_insert2<4, false>, k_fused_insert2<8, false>},
      {k_fused_insert<true>, k_fused_insert2<2, true>, k_fused_insert2<4, true>, k_fused_insert2<8, true>}};
  const int w = epw == 8 ? 3 : (epw == 4 ? 2 : (epw == 2 ? 1 : 0));   // log2 of the environments per wave
  hipLaunchKernelGGL(kernels[lp_t ? 1 : 0][w], dim3((unsigned)ceil_div(B, 1 << w)), dim3(INSB), 0, s, Nmax, B, N, fbt, P,
                     sel_t, agent_features, A, a_bstride, use_cong, time, ins_scratch, entropy1, reward_t, out, lp_t, ent_t);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// rollout mode 1: frame t's insert (one workgroup per environment) and frame t + 1's choice (C) in one launch
int tarl_launch_insert_choice(const ChoiceArgs& C, unsigned threads, hipStream_t s, int Nmax, int64_t B, int64_t N,
                              const FusedBufs* fbt, PlanOut P, const uint8_t* sel_t, float* agent_features, int64_t A,
                              int64_t a_bstride, int use_cong, float time, int32_t* ins_scratch, const float* entropy1,
                              float* reward_t, const FrameOut& out, float* lp_t, float* ent_t) {
  hipLaunchKernelGGL(lp_t ? k_fused_insert_choice<true> : k_fused_insert_choice<false>, dim3(C.choice_blocks + (unsigned)B),
                     dim3(threads), 0, s, C, Nmax, B, N, fbt, P, sel_t, agent_features, A, a_bstride, use_cong, time,
                     ins_scratch, entropy1, reward_t, out, lp_t, ent_t);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
