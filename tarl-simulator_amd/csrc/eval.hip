// eval.hip — what a vectorised policy evaluation needs beyond the rollout's kernels: the deterministic (MODE) action of
// GraphDistribution written as the packed state's rank bytes, and the per-environment episode summary.
//
// Reference semantics restated: src/reinforcement_learning.py:45-55 (GraphDistribution.mode: scatter_max over the
// probabilities, first maximum wins), :82-96 (log_prob), src/rl/ppo_trainer.py:89-127 (_evaluate: return = sum of the
// rewards), src/runner.py:147-150 (arrived agents and their mean travel time), src/transportation_simulator.py leg
// histogram (ON_WAY flag count).
#include <math.h>

#include "tarl_common.h"

#define SEL_CARRIED 0x80u   // = fused_common.h: rank byte of a node that drew nothing
#define LOG_EPS_P 1e-8f     // log(p + 1e-8), src/reinforcement_learning.py:27
#define MR_BLOCK 1024       // = ENV_BLOCK of dist.hip: the log-prob reduction tree of k_logprob_entropy_fwd has 1024 leaves
#define MR_REG_DEG 4        // out-degrees up to this are evaluated out of registers
#define MR_ENVS 8           // environments per workgroup == bytes of one sel8 row segment (one 8-byte store)

// ---- MODE action + log-prob in one launch ------------------------------------------------------------------------------
// Bit-identical to tarl_graphdist_softmax -> tarl_graphdist_mode -> tarl_graphdist_logprob_entropy_fwd:
//  * per node the chain's own expressions in the chain's order (sequential max, sequential fp32 sum, expf(l/T - max) / sum,
//    k_mode's comparison on the PROBABILITIES with the lower edge id winning a tie) — recomputed instead of re-read, as
//    k_graphdist_rollout does;
//  * the log-prob of an environment is k_logprob_entropy_fwd's tree: leaf v in [0, 1024) sums the nodes v, v + 1024, ... in
//    order, 64 leaves are folded by the shfl_down tree, the wave sums are added left to right. A leaf without nodes holds
//    +0.0f and x + 0.0f == x, so only the VT = min(1024, pow2 >= N) leaves that can own a node are evaluated.
// Mapping: nothing here is serial across nodes (no global prefix), so a workgroup is not one environment. It owns MR_ENVS
// consecutive environments; its 1024 threads are (1024 / VT) environments x VT leaves per pass, so a small graph still fills
// every wave; logits are read along the edge axis (coalesced, env-major), choice / choice8 written along the node axis
// (coalesced, env-major). sel8 is ENV-MINOR: the rank bytes go through an LDS tile [node][MR_ENVS] and leave as one 8-byte
// store per node row instead of MR_ENVS single bytes a cache line apart.
// A node with up to MR_REG_DEG out-edges keeps its logits, l / T and expf in registers (each evaluated once); walking it
// three times like the chain made the kernel instruction-bound (158 -> 83 us at config 4, B = 4096).
__device__ __forceinline__ void mr_softmax_stats(const float* __restrict__ lb, const int32_t* __restrict__ out_eid,
                                                 int32_t k0, int32_t k1, float temperature, bool sorted, float* mx_out,
                                                 float* sum_out) {
  float mx = -INFINITY;
  for (int32_t k = k0; k < k1; ++k) mx = fmaxf(mx, lb[sorted ? k : out_eid[k]] / temperature);
  float sum = 0.0f;
  for (int32_t k = k0; k < k1; ++k) sum = sum + expf(lb[sorted ? k : out_eid[k]] / temperature - mx);
  *mx_out = mx;
  *sum_out = sum;
}

template <bool SORTED>
__global__ __launch_bounds__(MR_BLOCK, 8) void k_graphdist_mode_rollout(
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_eid, const float* __restrict__ logits, int64_t B,
    int64_t N, int64_t E, float temperature, int vt_shift, int32_t* __restrict__ choice_eid, uint8_t* __restrict__ choice8,
    uint8_t* __restrict__ sel8, float* __restrict__ log_prob, int vec8) {
  __shared__ __attribute__((aligned(16))) uint8_t s_code[MR_BLOCK][MR_ENVS];
  __shared__ float s_red[MR_ENVS][MR_BLOCK / 64];
  __shared__ float s_lp[MR_ENVS][MR_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int VT = 1 << vt_shift;                 // leaves per environment that can own a node (128 .. 1024)
  const int vt = tid & (VT - 1), esub = tid >> vt_shift;
  const int EP = MR_BLOCK >> vt_shift;          // environments per pass (1 .. 8)
  const int npass = MR_ENVS / EP;
  const int64_t b0 = (int64_t)blockIdx.x * MR_ENVS;
  const bool unit_t = temperature == 1.0f;
  // leaf sums, one per (pass, thread): thread-private LDS words, so that the passes are a plain loop (fully unrolled with
  // the sums in registers the kernel took 96 VGPRs, one resident workgroup per CU instead of two)
  for (int q = 0; q < npass; ++q) s_lp[q][tid] = 0.0f;

  for (int64_t i0 = 0; i0 < N; i0 += VT) {      // one trip unless N > 1024 (then VT == 1024)
    const int64_t i = i0 + vt;
    int32_t k0 = 0, k1 = 0;
    if (i < N) {
      k0 = out_ptr[i];
      k1 = out_ptr[i + 1];
    }
    for (int q = 0; q < npass; ++q) {
      const int e_loc = q * EP + esub;
      const int64_t b = b0 + e_loc;
      if (i < N && b < B) {
        const float* lb = logits + b * E;
        int32_t pick = -1, rank = 0;
        if (k0 != k1 && k1 - k0 <= MR_REG_DEG) {
          // up to four out-edges (a road network's junction): every logit is loaded once, l / T, expf and p are evaluated
          // once per edge and held in registers — the same functions of the same arguments as the chain's three passes
          const int32_t deg = k1 - k0;
          float xs[MR_REG_DEG];
#pragma unroll
          for (int r = 0; r < MR_REG_DEG; ++r) {
            const int32_t kk = k0 + (r < deg ? r : 0);
            xs[r] = lb[SORTED ? kk : out_eid[kk]];
          }
          float mx = -INFINITY;
#pragma unroll
          for (int r = 0; r < MR_REG_DEG; ++r) {
            xs[r] = unit_t ? xs[r] : xs[r] / temperature;        // (l / 1.0f == l exactly)
            if (r < deg) mx = fmaxf(mx, xs[r]);
          }
          float sum = 0.0f;
#pragma unroll
          for (int r = 0; r < MR_REG_DEG; ++r) {
            xs[r] = expf(xs[r] - mx);
            if (r < deg) sum = sum + xs[r];
          }
          float best = -INFINITY;
#pragma unroll
          for (int r = 0; r < MR_REG_DEG; ++r) {
            const float p = xs[r] / sum;
            const int32_t e = SORTED ? k0 + r : out_eid[k0 + (r < deg ? r : 0)];
            if (r < deg && (pick < 0 || p > best || (p == best && e < pick))) {   // k_mode's test, word for word
              best = p;
              pick = e;
              rank = r;
            }
          }
          s_lp[q][tid] += logf(best + LOG_EPS_P);
        } else if (k0 != k1) {
          float mx, sum;
          mr_softmax_stats(lb, out_eid, k0, k1, temperature, SORTED, &mx, &sum);
          float best = -INFINITY;
          for (int32_t k = k0; k < k1; ++k) {
            const int32_t e = SORTED ? k : out_eid[k];
            const float p = expf(lb[e] / temperature - mx) / sum;
            if (pick < 0 || p > best || (p == best && e < pick)) {   // k_mode's test, word for word
              best = p;
              pick = e;
              rank = k - k0;
            }
          }
          s_lp[q][tid] += logf(best + LOG_EPS_P);
        }
        uint32_t code = (uint32_t)rank;
        if (pick < 0) code = ((sel8 ? sel8[i * B + b] : 0u) & 0x7Fu) | SEL_CARRIED;
        if (choice_eid) choice_eid[b * N + i] = pick;
        if (choice8) choice8[b * N + i] = (uint8_t)code;
        s_code[vt][e_loc] = (uint8_t)code;
      }
    }
    if (sel8) {      // (uniform) the tile leaves env-minor: row i, environments b0 .. b0 + MR_ENVS - 1
      __syncthreads();
      const int64_t iw = i0 + tid;
      if (tid < VT && iw < N) {
        if (vec8) {
          *reinterpret_cast<uint2*>(sel8 + iw * B + b0) = *reinterpret_cast<const uint2*>(&s_code[tid][0]);
        } else {
          for (int q = 0; q < MR_ENVS && b0 + q < B; ++q) sel8[iw * B + b0 + q] = s_code[tid][q];
        }
      }
      __syncthreads();
    }
  }
  if (!log_prob) return;
  for (int q = 0; q < npass; ++q) {
    float v = s_lp[q][tid];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) s_red[q * EP + esub][vt >> 6] = v;
  }
  __syncthreads();
  if (tid < MR_ENVS && b0 + tid < B) {
    float tot = 0.0f;
    for (int w = 0; w < (VT >> 6); ++w) tot += s_red[tid][w];
    log_prob[b0 + tid] = tot;      // (the chain's -inf branch needs an action that is not one edge per node: not a MODE)
  }
}

extern "C" int tarl_graphdist_mode_rollout(const tarl_plan* plan, const float* logits, int64_t B, float temperature,
                                           int32_t* choice, uint8_t* choice8, uint8_t* sel8, float* log_prob,
                                           tarl_stream stream) {
  TARL_REQUIRE(plan && logits, "null argument");
  TARL_REQUIRE(B >= 1 && B < ((int64_t)1 << 31), "bad B");
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  TARL_REQUIRE(choice || choice8 || sel8 || log_prob, "no output requested");
  TARL_REQUIRE(plan->max_out <= 126, "out-degree above 126 has no rank byte");
  if (plan->N == 0) return TARL_OK;
  int vt_shift = 7;
  while (vt_shift < 10 && ((int64_t)1 << vt_shift) < plan->N) ++vt_shift;
  const int vec8 = (B % MR_ENVS == 0) && (((uintptr_t)sel8) % 8 == 0);
  const dim3 grid((unsigned)ceil_div(B, MR_ENVS)), block(MR_BLOCK);
  if (plan->src_sorted)
    hipLaunchKernelGGL((k_graphdist_mode_rollout<true>), grid, block, 0, (hipStream_t)stream, plan->out_ptr, plan->out_eid,
                       logits, B, plan->N, plan->E, temperature, vt_shift, choice, choice8, sel8, log_prob, vec8);
  else
    hipLaunchKernelGGL((k_graphdist_mode_rollout<false>), grid, block, 0, (hipStream_t)stream, plan->out_ptr, plan->out_eid,
                       logits, B, plan->N, plan->E, temperature, vt_shift, choice, choice8, sel8, log_prob, vec8);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- episode summary ---------------------------------------------------------------------------------------------------
// One workgroup per environment over its agent table [A][9] (row 0, the dummy, is skipped). Integer outputs (the three
// counts, the travel-time histogram through LDS atomics) do not depend on the order; the fp64 sums are taken in a fixed
// order: thread t over the agents 1 + t, 1 + t + 256, ..., the shfl_down tree inside a wave, the four waves left to right.
// The episode return is the fp64 sum of reward[t][b] in frame order (wave 0 fetches 64 frames at a time, every lane adds them
// in the same order).
#define ES_BLOCK 256
#define ES_MAX_BINS 16384

__global__ __launch_bounds__(ES_BLOCK) void k_episode_summary(const float* __restrict__ ag, int64_t A, int64_t a_bstride,
                                                              int64_t B, const float* __restrict__ reward, int64_t T,
                                                              float bin_width, int32_t num_bins,
                                                              int32_t* __restrict__ counts, double* __restrict__ sums,
                                                              double* __restrict__ episode_return,
                                                              int32_t* __restrict__ hist) {
  extern __shared__ int32_t s_hist[];
  __shared__ double s_d[3][ES_BLOCK / 64];
  __shared__ int32_t s_c[3][ES_BLOCK / 64];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (hist) {
    for (int32_t k = tid; k < num_bins; k += ES_BLOCK) s_hist[k] = 0;
    __syncthreads();
  }
  const float* agb = ag + b * a_bstride;
  int32_t n_done = 0, n_way = 0, n_wait = 0;
  double s1 = 0.0, s2 = 0.0, mx = -INFINITY;
  for (int64_t a = 1 + tid; a < A; a += ES_BLOCK) {
    const float* row = agb + a * AG_COLS;
    if (row[AG_DONE] == 1.0f) {
      const float tt = row[AG_ARR] - row[AG_DEP];
      const double d = (double)tt;
      ++n_done;
      s1 += d;
      s2 += d * d;
      mx = fmax(mx, d);
      if (hist) {
        const float q = floorf(tt / bin_width);
        const int32_t bin = !(q >= 0.0f) ? 0 : (q >= (float)(num_bins - 1) ? num_bins - 1 : (int32_t)q);
        atomicAdd(&s_hist[bin], 1);
      }
    } else if (row[AG_ON_WAY] == 1.0f) {
      ++n_way;
    } else {
      ++n_wait;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    n_done += __shfl_down(n_done, off);
    n_way += __shfl_down(n_way, off);
    n_wait += __shfl_down(n_wait, off);
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
    mx = fmax(mx, __shfl_down(mx, off));
  }
  if (lane == 0) {
    s_c[0][wid] = n_done;
    s_c[1][wid] = n_way;
    s_c[2][wid] = n_wait;
    s_d[0][wid] = s1;
    s_d[1][wid] = s2;
    s_d[2][wid] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t c0 = 0, c1 = 0, c2 = 0;
    double t1 = 0.0, t2 = 0.0, tm = -INFINITY;
    for (int w = 0; w < ES_BLOCK / 64; ++w) {
      c0 += s_c[0][w];
      c1 += s_c[1][w];
      c2 += s_c[2][w];
      t1 += s_d[0][w];
      t2 += s_d[1][w];
      tm = fmax(tm, s_d[2][w]);
    }
    counts[b * 3 + 0] = c0;
    counts[b * 3 + 1] = c1;
    counts[b * 3 + 2] = c2;
    sums[b * 3 + 0] = t1;
    sums[b * 3 + 1] = t2;
    sums[b * 3 + 2] = c0 > 0 ? tm : 0.0;
  }
  if (hist)      // (the barrier above ordered the LDS atomics of every thread before these reads)
    for (int32_t k = tid; k < num_bins; k += ES_BLOCK) hist[b * num_bins + k] = s_hist[k];
  if (episode_return && wid == 0) {
    double r = 0.0;
    for (int64_t t0 = 0; t0 < T; t0 += 64) {
      const float v = (reward && t0 + lane < T) ? reward[(t0 + lane) * B + b] : 0.0f;
      const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
      for (int j = 0; j < n; ++j) r += (double)__shfl(v, j);
    }
    if (lane == 0) episode_return[b] = r;
  }
}

extern "C" int tarl_episode_summary(const float* agent_features, int64_t B, int64_t num_agents, int64_t a_bstride,
                                    const float* reward, int64_t T, float bin_width, int32_t num_bins, int32_t* counts,
                                    double* sums, double* episode_return, int32_t* hist, tarl_stream stream) {
  TARL_REQUIRE(agent_features && counts && sums, "null argument");
  TARL_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && num_agents >= 1, "bad sizes");
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TARL_REQUIRE(T >= 0 && (T == 0 || reward), "T frames need a reward buffer");
  if (hist) {
    TARL_REQUIRE(num_bins >= 1 && num_bins <= ES_MAX_BINS, "num_bins must be in [1, 16384]");
    TARL_REQUIRE(bin_width > 0.0f, "bin_width must be positive");
  }
  const size_t lds = hist ? (size_t)num_bins * sizeof(int32_t) : 0;
  hipLaunchKernelGGL(k_episode_summary, dim3((unsigned)B), dim3(ES_BLOCK), lds, (hipStream_t)stream, agent_features,
                     num_agents, a_bstride, B, reward, T, bin_width, num_bins, counts, sums, episode_return, hist);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
