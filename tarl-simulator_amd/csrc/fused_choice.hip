// fused_choice.hip — the live policy's action draw: the per-parameter-update tables, the per-frame draw (k_fused_choice), the
// all-frames draw of a rollout on its side stream, and the conversions of externally sampled actions. (Design: fused_frame.h.)
#include "fused_choice.h"

// ---- policy tables ------------------------------------------------------------------------------------------------------
// The live policy's logits depend only on (emb, static ROAD_INDEX of the target road): they are identical for every
// environment and every frame between two optimiser steps. k_policy_tables evaluates, ONCE per parameter update and with
// exactly the arithmetic / reduction trees of k_edge_logits_fwd + k_softmax + k_sample + k_logprob_entropy_fwd, the
// per-edge tables (CSR order): thr[k] = fp32 inverse-CDF threshold, lg[k] = log(p + 1e-8), plus the entropy.
__device__ __forceinline__ float fb_block_sum(float v, float* s_red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();
  if (lane == 0) s_red[wid] = v;
  __syncthreads();
  float tot = 0.0f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += s_red[w];
  return tot;
}

__device__ __forceinline__ float live_logit(const float* __restrict__ emb, int64_t M, const float4* __restrict__ st0,
                                            int32_t dst) {
  const long long idx = (long long)st0[dst].z;
  return (idx >= 0 && idx < M) ? emb[idx] : 0.0f;
}

__global__ __launch_bounds__(ENVB) void k_policy_tables(const int32_t* __restrict__ out_ptr,
                                                        const int32_t* __restrict__ out_dst,
                                                        const int32_t* __restrict__ node_of_group, int64_t N, int64_t G,
                                                        const float* __restrict__ emb, int64_t M, float temperature,
                                                        const float4* __restrict__ st0, double* __restrict__ base,
                                                        float* __restrict__ thr, long long* __restrict__ lgt,
                                                        float* __restrict__ entropy_out) {
  __shared__ double s_wave[ENVB / 64];
  __shared__ float s_red[ENVB / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double running = 0.0;
  for (int64_t g0 = 0; g0 < G; g0 += ENVB) {
    const int64_t g = g0 + tid;
    double s = 0.0;
    if (g < G) {
      const int32_t i = node_of_group[g];
      const int32_t k0 = out_ptr[i], k1 = out_ptr[i + 1];
      float mx = -INFINITY;
      for (int32_t k = k0; k < k1; ++k) mx = fmaxf(mx, live_logit(emb, M, st0, out_dst[k]) / temperature);
      float sum = 0.0f;
      for (int32_t k = k0; k < k1; ++k) sum = sum + expf(live_logit(emb, M, st0, out_dst[k]) / temperature - mx);
      for (int32_t k = k0; k < k1; ++k) s += (double)(expf(live_logit(emb, M, st0, out_dst[k]) / temperature - mx) / sum);
    }
    double inc = s;
    for (int off = 1; off < 64; off <<= 1) {
      const double v = __shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    double wbase = 0.0, tot = 0.0;
    for (int w = 0; w < ENVB / 64; ++w) {
      const double v = s_wave[w];
      if (w < wid) wbase += v;
      tot += v;
    }
    double exc = __shfl_up(inc, 1);
    if (lane == 0) exc = 0.0;
    if (g < G) base[g] = running + wbase + exc;
    running += tot;
    __syncthreads();
  }
  float ent = 0.0f;
  for (int64_t i = tid; i < N; i += ENVB) {
    const int32_t k0 = out_ptr[i], k1 = out_ptr[i + 1];
    if (k0 == k1) continue;
    float mx = -INFINITY;
    for (int32_t k = k0; k < k1; ++k) mx = fmaxf(mx, live_logit(emb, M, st0, out_dst[k]) / temperature);
    float sum = 0.0f;
    for (int32_t k = k0; k < k1; ++k) sum = sum + expf(live_logit(emb, M, st0, out_dst[k]) / temperature - mx);
    int64_t g = i;
    if (G != N) {
      int64_t lo = 0, hi = G - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (node_of_group[mid] < i) lo = mid + 1; else hi = mid;
      }
      g = lo;
    }
    const double bg = base[g];
    const float bg32 = (float)bg;
    double run = bg;
    for (int32_t k = k0; k < k1; ++k) {
      const float p = expf(live_logit(emb, M, st0, out_dst[k]) / temperature - mx) / sum;
      const float lg = logf(p + LOG_EPS_P);
      ent -= p * lg;
      run += (double)p;
      thr[k] = (float)run - bg32;
      lgt[k] = (long long)((double)lg * LP_FIX);   // the frame kernels only ever add it up in 2^-32 fixed point
    }
  }
  const float ent_t = fb_block_sum(ent, s_red);
  if (tid == 0) entropy_out[0] = ent_t;
}

__global__ __launch_bounds__(TILE) void k_fused_choice(const int32_t* __restrict__ out_ptr,
                                                       const int32_t* __restrict__ out_eid,
                                                       const int32_t* __restrict__ group_of_node, int64_t G, int64_t B,
                                                       int64_t N, long long* __restrict__ acc_lp, int64_t acc_slots,
                                                       const float* __restrict__ thr,
                                                       const long long* __restrict__ lgt,
                                                       const float* __restrict__ uniform, uint64_t pseed,
                                                       uint64_t pcounter, uint8_t* __restrict__ sel_out,
                                                       const uint8_t* __restrict__ sel_prev,
                                                       int32_t* __restrict__ choice, int nchunk, int want_lp,
                                                       int64_t env_base) {
  fused_choice_body(blockIdx.x, blockIdx.y, out_ptr, out_eid, group_of_node, G, B, N, acc_lp, acc_slots, thr, lgt,
                    uniform, pseed, pcounter, sel_out, sel_prev, choice, nchunk, want_lp, env_base);
}

// ---- the whole rollout's actions in one pass (state-independent policy) -----------------------------------------------------
// The live policy's distribution does not read the state, so the T actions of a rollout are T independent draws from ONE
// set of tables: instead of a choice launch per frame (instruction-bound: ~16 us of scalar table walks that the frame loop
// had to wait for), the action buffer [T][N][B] is filled by launches of 32 frames each on a side stream, in the shadow of
// the latency-bound frame kernels. One workgroup = one (environment tile, frame): it walks ALL nodes, so a frame's
// log-prob is a register sum (no atomics) — the same Philox indices, thresholds and 2^-32 fixed-point terms as the
// per-frame kernel, hence the same bits.
// A node that draws nothing (u at / beyond its last threshold through rounding, ~1e-7 per draw) keeps the PREVIOUS frame's
// SELECTED_ROAD: frames are concurrent here, so such an entry is marked SEL_UNRESOLVED, listed, and resolved by
// k_choice_fixup (walk back to the last frame that drew something; before frame 0: the packed state's code).
#define SEL_UNRESOLVED 0xFEu      // = SEL_CARRIED | 0x7E: no rank (out-degree <= 126) and not SEL_RAW
#define FIX_CAP 65536
struct __attribute__((aligned(4))) PRec {   // per out-edge (CSR order, padded by 4): inverse-CDF threshold + log-prob
  float thr;
  int32_t lg_lo, lg_hi;                      // log(p + 1e-8) in 2^-32 fixed point
  int32_t pad;
};

__global__ __launch_bounds__(FB) void k_pack_ptab(int64_t E, const float* __restrict__ thr,
                                                  const long long* __restrict__ lgt, PRec* __restrict__ ptab) {
  const int64_t k = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (k >= E + 4) return;
  if (k < E) {
    const long long lg = lgt[k];
    ptab[k] = PRec{thr[k], (int32_t)(uint32_t)(lg & 0xffffffffll), (int32_t)(lg >> 32), 0};
  } else {
    ptab[k] = PRec{2.0f, 0, 0, 0};
  }
}

// per node: everything the all-frames draw needs about it in ONE aligned scalar read whose address depends on the node
// index alone (through the CSR range it would be two dependent scalar rounds per node). The thresholds are kept as
// INTEGERS: a draw is u = f(m) = ((float)m + 0.5f) * 2^-24 of the 24-bit m = word >> 8, f is non-decreasing, so
// u >= thr  <=>  m >= ithr with ithr = min{m : f(m) >= thr} (2^24: never) — found by bisection with f itself, so the
// comparison is the same for every m and the three conversion instructions per draw are not issued. The log-prob terms
// (second half of the record) are copied into LDS per workgroup and looked up by the count.
struct __attribute__((aligned(64))) PNode {
  int32_t gi, deg, out0, pad;
  uint32_t ithr[4];                          // 2^24 beyond the out-degree
  int32_t lg_lo[4], lg_hi[4];
};
static_assert(sizeof(PNode) == 64, "PNode: a 32-byte scalar read + 32 bytes of log-prob terms");
typedef int32_t i32x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(FB) void k_pack_pnode(int64_t N, const NodeRec* __restrict__ nodes,
                                                   const int32_t* __restrict__ group_of_node,
                                                   const float* __restrict__ thr, const long long* __restrict__ lgt,
                                                   PNode* __restrict__ pnode) {
  const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (i >= N) return;
  PNode pn;
  pn.gi = group_of_node[i];
  pn.deg = nodes[i].out_deg;
  pn.out0 = nodes[i].out0;
  pn.pad = 0;
  for (int q = 0; q < 4; ++q) {
    const bool in = q < pn.deg;
    const long long lg = in ? lgt[pn.out0 + q] : 0ll;
    const float th = in ? thr[pn.out0 + q] : INFINITY;
    uint32_t lo = 0u, hi = 1u << 24;         // the first m with f(m) >= th (NaN / +inf: none)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (u01_open(mid << 8) >= th)
        hi = mid;
      else
        lo = mid + 1u;
    }
    pn.ithr[q] = lo;
    pn.lg_lo[q] = (int32_t)(uint32_t)(lg & 0xffffffffll);
    pn.lg_hi[q] = (int32_t)(lg >> 32);
  }
  pnode[i] = pn;
}

#define CHOICE_SEG 128    // nodes per workgroup of the all-frames choice (a frame's log-prob = the sum of its segments)
// one node's draw from the first half of its record v and the 24 random bits m: the inverse CDF is a count — thresholds
// are non-decreasing (fp32 roundings of a running double sum), so the first q with u < thr[q] is the number of thresholds
// at or below u. lgn: the node's four log-prob terms in LDS (one entry of slack behind them).
__device__ __forceinline__ void choice_node(const i32x8 v, const uint32_t m, const long long* lgn,
                                            const PRec* __restrict__ ptab, uint32_t row, int64_t t,
                                            uint8_t* __restrict__ out, long long& lp, bool& bad,
                                            int32_t* __restrict__ fix, int32_t* __restrict__ flags) {
  const int32_t deg = v[1];
  const PRec* pr = ptab + v[2];
  uint32_t cnt = (m >= (uint32_t)v[4] ? 1u : 0u) + (m >= (uint32_t)v[5] ? 1u : 0u) + (m >= (uint32_t)v[6] ? 1u : 0u) +
                 (m >= (uint32_t)v[7] ? 1u : 0u);
  long long lpn = lgn[cnt < 4u ? cnt : 4u];
  if (deg > 4) {                         // wave-uniform: the thresholds further down the table, as floats
    const float u = u01_open(m << 8);
    for (int32_t q = 4; q < deg; ++q) cnt += (u >= pr[q].thr) ? 1u : 0u;
    if (cnt >= 4u && cnt < (uint32_t)deg) {
      const PRec px = pr[cnt];
      lpn = ((long long)px.lg_hi << 32) | (long long)(uint32_t)px.lg_lo;
    }
  }
  const bool found = cnt < (uint32_t)deg;
  lp += lpn;                             // a node that drew nothing poisons the whole sum below
  if (!found) {
    bad = true;
    const int32_t pos = atomicAdd(&fix[0], 1);
    if (pos < FIX_CAP) {
      fix[2 + 2 * pos] = (int32_t)t;
      fix[3 + 2 * pos] = (int32_t)row;
    } else {
      atomicOr(flags, FLAG_CHOICE_OVERFLOW);
    }
  }
  out[row] = (uint8_t)(found ? cnt : SEL_UNRESOLVED);
}

// QUAD (every node has out-edges and their number is a multiple of four: draw index = b * N + i, so nodes 4k .. 4k + 3
// of an environment share one Philox block): four nodes per step on the block's four words, without the block compare
// and the word select of the general form. Same indices, same words: the same draws.
template <bool QUAD>
__global__ __launch_bounds__(TILE) void k_fused_choice_all(const PNode* __restrict__ pnode, const PRec* __restrict__ ptab,
                                                           const int32_t* __restrict__ group_of_node, uint32_t G,
                                                           uint32_t B, uint32_t N, int64_t t0, uint64_t pseed,
                                                           uint64_t pcounter0, const uint8_t* __restrict__ sel0,
                                                           uint8_t* __restrict__ choice, long long* __restrict__ lp_acc,
                                                           int32_t* __restrict__ fix, int32_t* __restrict__ flags,
                                                           uint64_t env_base) {
  __shared__ long long s_lg[CHOICE_SEG * 4 + 4];
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t t = t0 + blockIdx.z;
  const uint32_t i0 = blockIdx.y * CHOICE_SEG;
  const uint32_t i1 = (i0 + CHOICE_SEG < N) ? i0 + CHOICE_SEG : N;
  for (uint32_t e = threadIdx.x; e < (i1 - i0) * 4; e += blockDim.x) {
    const PNode& pn = pnode[i0 + (e >> 2)];
    s_lg[e] = ((long long)pn.lg_hi[e & 3] << 32) | (long long)(uint32_t)pn.lg_lo[e & 3];
  }
  __syncthreads();
  if (b >= B) return;
  uint8_t* out = choice + t * (int64_t)N * B;
  long long lp = 0;
  bool bad = false;
  // The node loop issues no vector load at all (a conditional load inside it makes the compiler wait for the previous
  // iteration's store, vmcnt(0), every time round) and ONE scalar read per node, the first half of its PNode record, read
  // as one 8-dword vector (member by member the compiler splits it into dependent reads around the out-degree test).
  // Nodes without out-edges (they keep SELECTED_ROAD) get a loop of their own.
  if (QUAD) {
    const uint64_t blk0 = (env_base + (uint64_t)b) * (G >> 2);
    const uint64_t counter = pcounter0 + (uint64_t)t;
    for (uint32_t i = i0; i < i1; i += 4) {   // i0 and i1 are multiples of four
      const uint64_t blk = blk0 + (i >> 2);
      uint32_t o[4];
      philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)pseed,
                    (uint32_t)(pseed >> 32), o);
      const uint32_t row = i * B + b;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const i32x8 v = *(const i32x8*)(pnode + i + r);
        choice_node(v, o[r] >> 8, s_lg + (i - i0 + r) * 4, ptab, row + r * B, t, out, lp, bad, fix, flags);
      }
    }
  } else {
    PhiloxRun rng;
    for (uint32_t i = i0; i < i1; ++i) {      // i, and everything indexed by it alone, is wave-uniform
      const i32x8 v = *(const i32x8*)(pnode + i);
      if (v[1] == 0) continue;                // no out-edges (== no group)
      const uint32_t w = rng.word(pseed, pcounter0 + (uint64_t)t, (env_base + (uint64_t)b) * G + (uint64_t)v[0]);
      choice_node(v, w >> 8, s_lg + (i - i0) * 4, ptab, i * B + b, t, out, lp, bad, fix, flags);
    }
  }
  if (G != N) {
    for (uint32_t i = i0; i < i1; ++i)
      if (group_of_node[i] < 0) {
        const uint32_t row = i * B + b;
        out[row] = (uint8_t)((sel0[row] & 0x7Fu) | SEL_CARRIED);   // no out-edges: SELECTED_ROAD never changes
      }
  }
  // order-independent 2^-32 fixed-point sum over the node segments; an action with a node that drew nothing is poisoned
  // far beyond any legitimate sum (it is infeasible: log_prob = -inf, src/reinforcement_learning.py:88-92)
  if (lp_acc) atomicAdd((unsigned long long*)&lp_acc[t * B + b], (unsigned long long)(bad ? -(1ll << 50) : lp));
}

__global__ __launch_bounds__(FB) void k_choice_lp_finish(int64_t n, long long* __restrict__ lp_acc,
                                                         float* __restrict__ log_prob) {
  const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (i >= n) return;
  const long long v = lp_acc[i];
  lp_acc[i] = 0;     // re-armed for the next rollout
  log_prob[i] = (v < -(1ll << 49)) ? -INFINITY : (float)((double)v / LP_FIX);
}

__global__ __launch_bounds__(ENVB) void k_choice_fixup(uint32_t B, uint32_t N, const uint8_t* __restrict__ sel0,
                                                       uint8_t* __restrict__ choice, int32_t* __restrict__ fix) {
  int32_t cnt = fix[0];
  if (cnt > FIX_CAP) cnt = FIX_CAP;
  const int64_t NB = (int64_t)N * B;
  for (int32_t idx = threadIdx.x; idx < cnt; idx += ENVB) {
    const int64_t t = fix[2 + 2 * idx];
    const int64_t row = fix[3 + 2 * idx];
    uint32_t c = SEL_UNRESOLVED;
    for (int64_t tt = t - 1; tt >= 0 && c == SEL_UNRESOLVED; --tt) c = choice[tt * NB + row];
    if (c == SEL_UNRESOLVED) c = sel0[row];
    choice[t * NB + row] = (uint8_t)((c & 0x7Fu) | SEL_CARRIED);   // a concurrent reader sees the marker or this: same walk
  }
  __syncthreads();
  if (threadIdx.x == 0) fix[0] = 0;
}

extern "C" int tarl_fused_policy_prepare(const tarl_plan* plan, const tarl_fused* f, const float* emb,
                                         int64_t num_embeddings, float temperature, double* group_base,
                                         float* thresholds, int64_t* log_probs, float* entropy1, tarl_stream stream) {
  TARL_REQUIRE(plan && f && f->st0 && emb && group_base && thresholds && log_probs && entropy1, "null argument");
  TARL_REQUIRE(num_embeddings >= 1, "bad sizes");
  if (plan->N == 0) return TARL_OK;
  hipLaunchKernelGGL(k_policy_tables, dim3(1), dim3(ENVB), 0, (hipStream_t)stream, plan->out_ptr, plan->out_dst,
                     plan->node_of_group, plan->N, plan->G, emb, num_embeddings, temperature, (const float4*)f->st0,
                     group_base, thresholds, (long long*)log_probs, entropy1);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// one frame's draw as a launch of its own: the frame API, the first frame of rollout modes 0 and 1, every frame of mode 0
int tarl_launch_choice(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, long long* acc_lp,
                       const float* thresholds, const int64_t* log_probs, const float* uniform, uint64_t pseed,
                       uint64_t pcounter, uint8_t* sel_out, const uint8_t* sel_prev, int32_t* choice, int want_lp) {
  const unsigned threads = tile_threads(B);
  const dim3 grid_c((unsigned)ceil_div(B, threads), (unsigned)ceil_div(plan->N, nchunk_choice()));
  hipLaunchKernelGGL(k_fused_choice, grid_c, dim3(threads), 0, s, plan->out_ptr, plan->out_eid, plan->group_of_node, plan->G,
                     B, plan->N, acc_lp, f->acc_slots, thresholds, (const long long*)log_probs, uniform, pseed, pcounter,
                     sel_out, sel_prev, choice, nchunk_choice(), want_lp, f->env_base);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
// x[b, src(e), SELECTED_ROAD] = dst(e) for the chosen edge of every node, on the packed state (the choice phase of
// SimulatorEnv._step for an externally sampled action): choice int32 [B][N] = chosen edge id per node, -1 = none.
__global__ __launch_bounds__(FB) void k_apply_choice8(const int32_t* __restrict__ choice, const int32_t* __restrict__ out_ptr,
                                                      const int32_t* __restrict__ out_eid, int64_t B, int64_t N,
                                                      uint8_t* __restrict__ sel8) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;  // gid = i * B + b
  if (gid >= B * N) return;
  const int64_t i = gid / B, b = gid - i * B;
  const int32_t e = choice[b * N + i];
  uint32_t code = (sel8[gid] & 0x7Fu) | SEL_CARRIED;
  if (e >= 0) {
    const int32_t k0 = out_ptr[i], k1 = out_ptr[i + 1];
    for (int32_t k = k0; k < k1; ++k)
      if (out_eid[k] == e) code = (uint32_t)(k - k0);
  }
  sel8[gid] = (uint8_t)code;
}

extern "C" int tarl_fused_apply_choice(const tarl_plan* plan, const tarl_fused* f, int64_t B, const int32_t* choice,
                                       tarl_stream stream) {
  TARL_REQUIRE(plan && f && f->sel8 && choice && B >= 1, "null argument");
  if (plan->N == 0) return TARL_OK;
  hipLaunchKernelGGL(k_apply_choice8, dim3((unsigned)ceil_div(B * plan->N, FB)), dim3(FB), 0, (hipStream_t)stream, choice,
                     plan->out_ptr, plan->out_eid, B, plan->N, f->sel8);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// tarl_fused_set_actions: env-major action bytes (choice8 [B][N], what the samplers and the LDS-resident rollout write) ->
// the SELECTED_ROAD column the frame kernels read (sel8 [N][B]): 64 x 64 byte tiles turned through LDS, whole 64-byte runs on
// both sides. A road that drew nothing (bit 7) keeps its previous value: the code is completed from the old sel8 byte and
// written back to the action buffer as well. (Measured as a replacement for the per-frame sampler's own scattered sel8
// stores in tarl_fused_rollout_policy, B = 2048: sampler 102.7 -> 99.5 us, this kernel 8.9 us — not taken there.)
__global__ __launch_bounds__(256) void k_sel8_from_choice8(uint8_t* __restrict__ choice8, uint8_t* __restrict__ sel8,
                                                           int64_t B, int64_t N) {
  __shared__ uint8_t tile[64][68];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * 64, i0 = (int64_t)blockIdx.y * 64;
#pragma unroll 4
  for (int r = w; r < 64; r += 4) {            // row r = environment b0 + r, lanes along the roads
    const int64_t b = b0 + r, i = i0 + lane;
    tile[r][lane] = (b < B && i < N) ? choice8[b * N + i] : (uint8_t)0;
  }
  __syncthreads();
#pragma unroll 4
  for (int r = w; r < 64; r += 4) {            // row r = road i0 + r, lanes along the environments
    const int64_t i = i0 + r, b = b0 + lane;
    if (b < B && i < N) {
      uint32_t c = tile[lane][r];
      if (c & SEL_CARRIED) {
        c = (sel8[i * B + b] & 0x7Fu) | SEL_CARRIED;
        choice8[b * N + i] = (uint8_t)c;
      }
      sel8[i * B + b] = (uint8_t)c;
    }
  }
}

extern "C" int tarl_fused_set_actions(const tarl_plan* plan, const tarl_fused* f, int64_t B, uint8_t* choice8,
                                      tarl_stream stream) {
  TARL_REQUIRE(plan && f && f->sel8 && choice8, "null argument");
  TARL_REQUIRE(B >= 1, "bad batch size");
  if (plan->N == 0) return TARL_OK;
  hipLaunchKernelGGL(k_sel8_from_choice8, dim3((unsigned)ceil_div(B, 64), (unsigned)ceil_div(plan->N, 64)), dim3(256), 0,
                     (hipStream_t)stream, choice8, f->sel8, B, plan->N);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// side stream + events of the all-frames choice (one set per device, created on first use, kept for the process lifetime)
#define CHOICE_CHUNK 32          // frames per side-stream block (the first block is CHOICE_FIRST frames: it is waited for)
#define CHOICE_FIRST 4
#define CHOICE_MAX_CHUNKS 256
struct ChoiceSide {
  hipStream_t stream;
  hipEvent_t start;
  hipEvent_t done[CHOICE_MAX_CHUNKS];
  bool ready;
};
static ChoiceSide g_choice_side[64];

static int choice_side(ChoiceSide** out) {
  int dev = 0;
  TARL_CHECK_HIP(hipGetDevice(&dev));
  ChoiceSide* cs = &g_choice_side[dev & 63];
  if (!cs->ready) {
    TARL_CHECK_HIP(hipStreamCreateWithFlags(&cs->stream, hipStreamNonBlocking));
    TARL_CHECK_HIP(hipEventCreateWithFlags(&cs->start, hipEventDisableTiming));
    for (int i = 0; i < CHOICE_MAX_CHUNKS; ++i) TARL_CHECK_HIP(hipEventCreateWithFlags(&cs->done[i], hipEventDisableTiming));
    cs->ready = true;
  }
  *out = cs;
  return TARL_OK;
}

extern "C" int64_t tarl_fused_rollout_scratch_ints(const tarl_plan* plan, int64_t T, int64_t B) {
  // unresolved-draw list | packed policy records | per-node draw records (64-byte aligned) | per-(frame, environment)
  // log-prob accumulators (int64; last, so that every other offset is independent of T)
  return plan && T >= 1 && B >= 1 ? (int64_t)(4 + 2 * FIX_CAP) + 4 * (plan->E + 4) + 2 * T * B + 16 * (plan->N + 1) : -1;
}

// ---- the all-frames draw of a rollout, queued on the side stream (rollout mode 2) ------------------------------------------
bool tarl_choice_ahead_fits(const tarl_plan* plan, int64_t T) {
  return ceil_div(T, CHOICE_CHUNK) + 1 <= CHOICE_MAX_CHUNKS && ceil_div(plan->N, CHOICE_SEG) < 65536;
}

// Queues the draws of all T frames in blocks (the first CHOICE_FIRST frames, then CHOICE_CHUNK each) behind what the caller's
// stream s holds so far. *done: one event per block; the frame loop waits on them through tarl_choice_ahead_wait.
int tarl_choice_ahead_queue(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t T,
                            const float* thresholds, const int64_t* log_probs, uint64_t policy_seed,
                            uint64_t policy_counter0, int32_t* choice_scratch, uint8_t* choice, float* log_prob,
                            const hipEvent_t** done) {
  ChoiceSide* side = nullptr;
  const int rc = choice_side(&side);
  if (rc) return rc;
  const int64_t N = plan->N;
  const unsigned threads = tile_threads(B);
  int32_t* fix = choice_scratch;
  PRec* ptab = (PRec*)(choice_scratch + 4 + 2 * FIX_CAP);
  TARL_REQUIRE(((uintptr_t)ptab) % 16 == 0, "choice_scratch must be 16-byte aligned");
  // the side stream starts behind everything already queued on the caller's stream (tables, reset, earlier rollouts)
  TARL_CHECK_HIP(hipEventRecord(side->start, s));
  TARL_CHECK_HIP(hipStreamWaitEvent(side->stream, side->start, 0));
  TARL_CHECK_HIP(hipMemsetAsync(fix, 0, 2 * sizeof(int32_t), side->stream));
  hipLaunchKernelGGL(k_pack_ptab, dim3((unsigned)ceil_div(plan->E + 4, FB)), dim3(FB), 0, side->stream, plan->E,
                     thresholds, (const long long*)log_probs, ptab);
  TARL_LAUNCH_CHECK();
  // the per-node records come BEFORE the log-prob accumulators, so that no offset depends on T: a caller may reuse one
  // scratch buffer for rollouts of different lengths (an episode end splits a collector batch), and the accumulators
  // [T][B] — zero between rollouts, k_choice_lp_finish re-arms what a rollout used — must never be overlaid by a record
  // table of another call
  PNode* pnode = (PNode*)(((uintptr_t)(ptab + plan->E + 4) + 63) & ~(uintptr_t)63);
  long long* lp_acc = (long long*)(pnode + N);
  hipLaunchKernelGGL(k_pack_pnode, dim3((unsigned)ceil_div(N, FB)), dim3(FB), 0, side->stream, N,
                     (const NodeRec*)f->node_rec, plan->group_of_node, thresholds, (const long long*)log_probs, pnode);
  TARL_LAUNCH_CHECK();
  for (int64_t c = 0, t0 = 0; t0 < T; ++c) {
    const int64_t want = c == 0 ? CHOICE_FIRST : CHOICE_CHUNK;
    const unsigned nf = (unsigned)(T - t0 < want ? T - t0 : want);
    // TARL_CHOICE_QUAD=0 keeps the one-node-per-step form (developer knob)
    const bool quad = env_flag_on("TARL_CHOICE_QUAD") && plan->G == N && N % 4 == 0;
    hipLaunchKernelGGL(quad ? k_fused_choice_all<true> : k_fused_choice_all<false>,
                       dim3((unsigned)ceil_div(B, threads), (unsigned)ceil_div(N, CHOICE_SEG), nf),
                       dim3(threads), 0, side->stream, (const PNode*)pnode, (const PRec*)ptab,
                       plan->group_of_node, (uint32_t)plan->G, (uint32_t)B, (uint32_t)N, t0, policy_seed,
                       policy_counter0, (const uint8_t*)f->sel8, choice, log_prob ? lp_acc : nullptr, fix, f->flags,
                       (uint64_t)f->env_base);
    TARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_choice_fixup, dim3(1), dim3(ENVB), 0, side->stream, (uint32_t)B, (uint32_t)N,
                       (const uint8_t*)f->sel8, choice, fix);
    TARL_LAUNCH_CHECK();
    if (log_prob) {
      hipLaunchKernelGGL(k_choice_lp_finish, dim3((unsigned)ceil_div((int64_t)nf * B, FB)), dim3(FB), 0, side->stream,
                         (int64_t)nf * B, lp_acc + t0 * B, log_prob + t0 * B);
      TARL_LAUNCH_CHECK();
    }
    TARL_CHECK_HIP(hipEventRecord(side->done[c], side->stream));
    t0 += nf;
  }
  *done = side->done;
  return TARL_OK;
}

// before frame t of the rollout: when t is the first frame of a block, the caller's stream waits for that block's draws
int tarl_choice_ahead_wait(hipStream_t s, const hipEvent_t* done, int64_t t) {
  if (t == 0 || (t >= CHOICE_FIRST && (t - CHOICE_FIRST) % CHOICE_CHUNK == 0))
    TARL_CHECK_HIP(hipStreamWaitEvent(s, done[t == 0 ? 0 : 1 + (t - CHOICE_FIRST) / CHOICE_CHUNK], 0));
  return TARL_OK;
}
