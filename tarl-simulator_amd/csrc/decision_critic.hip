// decision_critic.hip — the learned per-decision critic of credit = "decision" (DESIGN 4.27): a baseline that reads the state
// in front of a decision and never the action, so that the per-decision advantage keeps its expectation. Not in the
// reference; off unless asked for.
//
// A live decision is a (kept row m, road u) pair with head[m][u] > 0 (the mask tarl_decision_advantage leaves). With
//     d = (long) DESTINATION of obs16[m][u],  s = dest_slot[d],  tau = timestep,  h = frames_left[m],
//     n_ff(x) = dist[s][x] / tau in fp64      (+inf where d lies outside [0, N) or s outside [0, num_dests)),
//     fill(x) = NUMBER_OF_AGENT(x) / MAXN(x), 0 where MAXN <= 0,
//     v* = the out-neighbour of u with the smallest finite dist[s][v], the first in CSR order on a tie,
// its eight fp32 features are
//     f0 = (float)min(n_ff(u), 512) / 64          f4 = (sum of fill(v) over the reachable v in CSR order) / their number
//     f1 = (float)min(h, 512) / 64                f5 = v* == d ? 1 : 0
//     f2 = fill(u)                                f6 = n_ff(u) > h ? 1 : 0     (fp64: cannot finish even at free flow)
//     f3 = fill(v*)                               f7 = min(FF(u) / tau, 64) / 8
// (f3 = f4 = f5 = 0 where no neighbour is reachable), and the network is goal_mlp.hip's 8 -> 16 (ReLU) -> 1 in its flat
// layout of 161 floats, a multiply then an add with k and j ascending (-ffp-contract=off: no FMA), so that a numpy fp32
// restatement reproduces features and values bit for bit.
//
//   k_dcr_feats   the features, zeros where the decision is not live (test hook).
//   k_dcr_fwd     value = y^ and optionally adv_out = adv_raw + delay_scale * y^, zeros where not live.
//   k_dcr_loss    features, forward, smooth-L1 loss against y = -adv_raw / delay_scale and the backward in one launch;
//   k_dcr_sum     the ordered sums behind it.
//
// One lane per node, tiles of DCR_TILE nodes, the (row, tile) pairs flattened, decision_credit.hip's shape. In the loss
// kernel a workgroup owns a fixed run of consecutive pairs (a function of M and N alone). The live lanes of a tile are
// compacted through LDS in node order (a ballot and a prefix count per wave, the waves in order), and threads 0..160 each
// add one gradient element over the compacted decisions in that order: goal_mlp.hip's [partition][161] scheme without the
// dead lanes, which are most of a tile (measured: 14.3 / 15.4 / 13.5 us against 17.0 / 17.4 / 17.1 us without the compaction,
// DESIGN 4.27); the partitions then meet in a fixed tree. No floating-point atomics: two runs are
// bit-identical.
#include <math.h>

#include "tarl_common.h"

#define DCR_TILE 256
#define DCR_MAX_BLOCKS ((int64_t)1 << 24)   // (row, tile) pairs of one launch, as decision_credit.hip
#define DCR_MAX_PARTS 1024                  // partial-sum rows of the loss at most
#define DCR_NF 8
#define DCR_NH 16
#define DCR_NW 161
#define DCR_B1 128
#define DCR_W2 144
#define DCR_B2 160
#define DCR_OBS_DEST 8                      // obs16 columns: {MAXN, NUMBER_OF_AGENT, FF, ..., [8] = DESTINATION of the head}

static inline int64_t dcr_tiles(const tarl_plan* plan) { return ceil_div(plan->N > 0 ? plan->N : 1, DCR_TILE); }

struct DcrIn {
  const int32_t *out_ptr, *out_dst;
  int64_t N;
  uint32_t tiles;
  const float* obs;            // [M][N][16]
  const int32_t* head;         // [M][N]
  const int32_t* frames_left;  // [M]
  const double* dist;          // [D][N]
  const int32_t* dest_slot;    // [N]
  int64_t D;
  double tau;
};

__device__ __forceinline__ float dcr_fill(const float* __restrict__ om, int64_t x) {
  const float2 a = *reinterpret_cast<const float2*>(om + x * 16);      // {MAXN, NUMBER_OF_AGENT}
  return a.x > 0.0f ? a.y / a.x : 0.0f;
}

// the features of the live decision (row om = obs + m * N * 16, road u)
__device__ __forceinline__ void dcr_features(const DcrIn& in, const float* __restrict__ om, int64_t u, int32_t h,
                                             float f[DCR_NF]) {
  const float dest = om[u * 16 + DCR_OBS_DEST];
  const double* drow = nullptr;
  long long d = -1;
  if (dest >= 0.0f && dest < (float)in.N) {
    d = (long long)dest;
    const int32_t s = in.dest_slot[d];
    if (s >= 0 && s < in.D) drow = in.dist + (int64_t)s * in.N;
  }
  const double nff = drow ? drow[u] / in.tau : INFINITY;
  f[0] = (float)fmin(nff, 512.0) / 64.0f;
  f[1] = (float)(h < 512 ? h : 512) / 64.0f;
  f[2] = dcr_fill(om, u);
  double best = INFINITY;
  int64_t vstar = -1;
  float sum = 0.0f;
  int32_t reach = 0;
  if (drow) {
    for (int32_t k = in.out_ptr[u], k1 = in.out_ptr[u + 1]; k < k1; ++k) {
      const int64_t v = in.out_dst[k];
      const double dv = drow[v];
      if (isfinite(dv)) {
        sum = sum + dcr_fill(om, v);
        ++reach;
        if (dv < best) {      // strict: the first in CSR order wins a tie
          best = dv;
          vstar = v;
        }
      }
    }
  }
  f[3] = vstar >= 0 ? dcr_fill(om, vstar) : 0.0f;
  f[4] = reach > 0 ? sum / (float)reach : 0.0f;
  f[5] = (vstar >= 0 && vstar == d) ? 1.0f : 0.0f;
  f[6] = nff > (double)h ? 1.0f : 0.0f;
  f[7] = fminf(om[u * 16 + 2] / (float)in.tau, 64.0f) / 8.0f;
}

__device__ __forceinline__ float dcr_eval(const float* __restrict__ w, const float f[DCR_NF]) {
  float y = w[DCR_B2];
#pragma unroll
  for (int j = 0; j < DCR_NH; ++j) {
    float pre = w[DCR_B1 + j];
#pragma unroll
    for (int k = 0; k < DCR_NF; ++k) pre = pre + w[j * DCR_NF + k] * f[k];
    y = y + w[DCR_W2 + j] * (pre > 0.0f ? pre : 0.0f);
  }
  return y;
}

// Must move per (row, road): 4 B of head; on a live road 64 B of its observation row, per out-neighbour 8 B of dist and
// 8 B of observation (scattered), and 32 B of features written (zeros elsewhere).
__global__ __launch_bounds__(DCR_TILE) void k_dcr_feats(DcrIn in, float* __restrict__ feats) {
  const uint32_t m = blockIdx.x / in.tiles, tile = blockIdx.x - m * in.tiles;
  const int64_t u = (int64_t)tile * DCR_TILE + threadIdx.x;
  if (u >= in.N) return;
  const int64_t at = (int64_t)m * in.N + u;
  float f[DCR_NF];
#pragma unroll
  for (int k = 0; k < DCR_NF; ++k) f[k] = 0.0f;
  if (in.head[at] > 0) dcr_features(in, in.obs + (int64_t)m * in.N * 16, u, in.frames_left[m], f);
  float4* o = reinterpret_cast<float4*>(feats + at * DCR_NF);
  o[0] = make_float4(f[0], f[1], f[2], f[3]);
  o[1] = make_float4(f[4], f[5], f[6], f[7]);
}

__global__ __launch_bounds__(DCR_TILE) void k_dcr_fwd(DcrIn in, const float* __restrict__ w, float delay_scale,
                                                      const float* __restrict__ adv_raw, float* __restrict__ value,
                                                      float* __restrict__ adv_out) {
  const uint32_t m = blockIdx.x / in.tiles, tile = blockIdx.x - m * in.tiles;
  const int64_t u = (int64_t)tile * DCR_TILE + threadIdx.x;
  if (u >= in.N) return;
  const int64_t at = (int64_t)m * in.N + u;
  float y = 0.0f, a = 0.0f;
  if (in.head[at] > 0) {
    float f[DCR_NF];
    dcr_features(in, in.obs + (int64_t)m * in.N * 16, u, in.frames_left[m], f);
    y = dcr_eval(w, f);
    if (adv_out) a = adv_raw[at] + delay_scale * y;
  }
  value[at] = y;
  if (adv_out) adv_out[at] = a;
}

struct DcrPartial {
  double loss, live, y1, y2, e2;
};
static_assert(sizeof(DcrPartial) == 40, "scratch layout of tarl_decision_critic_loss");

// Workgroup p owns the pairs [p * per, min((p + 1) * per, M * tiles)). Per pair: every lane evaluates its road, the live
// lanes stage {a_j = r w2_j [pre_j > 0], r relu(pre_j), f_k, r} in node order, threads 0..160 add their element over the
// staged decisions; the five sums of the pair go to pair_out through a fixed tree (lanes l and l + 32, .., 1, the waves
// in order). The hidden layer is evaluated twice (before and after the compaction) rather than kept in 48 registers.
__global__ __launch_bounds__(DCR_TILE) void k_dcr_loss(DcrIn in, const float* __restrict__ w, float delay_scale,
                                                       const float* __restrict__ adv_raw, const int32_t* __restrict__ n_live,
                                                       float coef, float grad_scale, int64_t pairs, int64_t per,
                                                       DcrPartial* __restrict__ pair_out, float* __restrict__ partial) {
  __shared__ float s_a[DCR_TILE][DCR_NH + 1];
  __shared__ float s_h[DCR_TILE][DCR_NH + 1];
  __shared__ float s_f[DCR_TILE][DCR_NF + 1];
  __shared__ float s_r[DCR_TILE];
  __shared__ double s_red[DCR_TILE / 64][5];
  __shared__ int s_cnt[DCR_TILE / 64];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int32_t L = n_live[0];
  const float c = L > 0 ? (coef * grad_scale) / (float)L : 0.0f;
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = (p0 + per < pairs) ? p0 + per : pairs;
  float acc = 0.0f;
  for (int64_t pair = p0; pair < p1; ++pair) {
    const int64_t m = pair / in.tiles;
    const int64_t u = (pair - m * in.tiles) * DCR_TILE + t;
    const int64_t at = m * in.N + u;
    const bool live = u < in.N && in.head[at] > 0;
    float f[DCR_NF], r = 0.0f;
    double v_loss = 0.0, v_live = 0.0, v_y1 = 0.0, v_y2 = 0.0, v_e2 = 0.0;
    if (live) {
      dcr_features(in, in.obs + m * in.N * 16, u, in.frames_left[m], f);
      float yh = w[DCR_B2];
#pragma unroll 1      // ten weights per turn: unrolled, all 161 would be held in scalar registers across the loop over the pairs
      for (int j = 0; j < DCR_NH; ++j) {
        float q = w[DCR_B1 + j];
#pragma unroll
        for (int k = 0; k < DCR_NF; ++k) q = q + w[j * DCR_NF + k] * f[k];
        yh = yh + w[DCR_W2 + j] * (q > 0.0f ? q : 0.0f);
      }
      const float y = (-adv_raw[at]) / delay_scale;
      const float e = yh - y;
      const float ae = fabsf(e);
      const float l = ae < 1.0f ? (0.5f * e) * e : ae - 0.5f;
      const float de = ae < 1.0f ? e : (e > 0.0f ? 1.0f : -1.0f);
      r = c * de;
      v_loss = (double)l;
      v_live = 1.0;
      v_y1 = (double)y;
      v_y2 = (double)y * (double)y;
      v_e2 = (double)e * (double)e;
    }
    const uint64_t ball = __ballot(live);
    __syncthreads();     // the previous pair has been summed
    if (lane == 0) s_cnt[wid] = __popcll(ball);
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int k = 0; k < DCR_TILE / 64; ++k) {
      if (k < wid) base += s_cnt[k];
      n += s_cnt[k];
    }
    if (live) {     // the hidden layer once more (the same operations), straight into the compacted rows
      const int at_s = base + __popcll(ball & (((uint64_t)1 << lane) - 1));
#pragma unroll 1
      for (int j = 0; j < DCR_NH; ++j) {
        float q = w[DCR_B1 + j];
#pragma unroll
        for (int k = 0; k < DCR_NF; ++k) q = q + w[j * DCR_NF + k] * f[k];
        s_a[at_s][j] = q > 0.0f ? r * w[DCR_W2 + j] : 0.0f;
        s_h[at_s][j] = q > 0.0f ? r * q : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < DCR_NF; ++k) s_f[at_s][k] = f[k];
      s_r[at_s] = r;
    }
    for (int off = 32; off > 0; off >>= 1) {
      v_loss += __shfl_down(v_loss, off);
      v_live += __shfl_down(v_live, off);
      v_y1 += __shfl_down(v_y1, off);
      v_y2 += __shfl_down(v_y2, off);
      v_e2 += __shfl_down(v_e2, off);
    }
    if (lane == 0) {
      s_red[wid][0] = v_loss;
      s_red[wid][1] = v_live;
      s_red[wid][2] = v_y1;
      s_red[wid][3] = v_y2;
      s_red[wid][4] = v_e2;
    }
    __syncthreads();
    if (t < DCR_B1) {
      const int j = t >> 3, k = t & 7;
      for (int p = 0; p < n; ++p) acc = acc + s_a[p][j] * s_f[p][k];
    } else if (t < DCR_W2) {
      for (int p = 0; p < n; ++p) acc = acc + s_a[p][t - DCR_B1];
    } else if (t < DCR_B2) {
      for (int p = 0; p < n; ++p) acc = acc + s_h[p][t - DCR_W2];
    } else if (t == DCR_B2) {
      for (int p = 0; p < n; ++p) acc = acc + s_r[p];
    } else if (t == DCR_TILE - 1) {
      DcrPartial q = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < DCR_TILE / 64; ++k) {
        q.loss += s_red[k][0];
        q.live += s_red[k][1];
        q.y1 += s_red[k][2];
        q.y2 += s_red[k][3];
        q.e2 += s_red[k][4];
      }
      pair_out[pair] = q;
    }
  }
  if (t < DCR_NW) partial[(int64_t)blockIdx.x * DCR_NW + t] = acc;
}

// blocks 0 .. ceil(M / 64) - 1: out5 of 64 rows each, the tiles in order; the blocks behind them: one wave per gradient
// element, lane l adds the partitions l, l + 64, .. in order and the lanes meet in a fixed tree (l and l + 32, 16, .., 1), so
// that the sum depends on the number of partitions alone. (One thread per element walking up to 1024 partitions one
// dependent load at a time took 130 us at 512 partitions, several times the loss kernel itself.)
__global__ __launch_bounds__(DCR_TILE) void k_dcr_sum(const DcrPartial* __restrict__ pair_out, int64_t M, uint32_t tiles,
                                                      uint32_t row_blocks, double* __restrict__ out5,
                                                      const float* __restrict__ partial, int64_t parts,
                                                      float* __restrict__ grads) {
  const int t = threadIdx.x;
  if (blockIdx.x >= row_blocks) {
    const int e = (int)(blockIdx.x - row_blocks) * (DCR_TILE / 64) + (t >> 6), lane = t & 63;
    if (!grads || e >= DCR_NW) return;       // wave-uniform
    float s = 0.0f;
    for (int64_t p = lane; p < parts; p += 64) s = s + partial[p * DCR_NW + e];
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_down(s, off);
    if (lane == 0) grads[e] = grads[e] + s;
    return;
  }
  const int64_t m = (int64_t)blockIdx.x * 64 + t;
  if (t >= 64 || m >= M) return;
  DcrPartial s = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t k = 0; k < tiles; ++k) {
    const DcrPartial q = pair_out[m * tiles + k];
    s.loss += q.loss;
    s.live += q.live;
    s.y1 += q.y1;
    s.y2 += q.y2;
    s.e2 += q.e2;
  }
  out5[5 * m] = s.loss;
  out5[5 * m + 1] = s.live;
  out5[5 * m + 2] = s.y1;
  out5[5 * m + 3] = s.y2;
  out5[5 * m + 4] = s.e2;
}

// -> the pairs per partition and the number of partitions of M * tiles pairs: a function of M and N alone
static void dcr_partition(int64_t pairs, int64_t* per, int64_t* parts) {
  *per = ceil_div(pairs, DCR_MAX_PARTS);
  *parts = ceil_div(pairs, *per);
}

static int dcr_check(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head, const int32_t* frames_left,
                     const double* dist, const int32_t* dest_slot, int64_t num_dests, float timestep) {
  TARL_REQUIRE(plan && obs16 && head && frames_left && dist && dest_slot, "null argument");
  TARL_REQUIRE(M >= 1 && num_dests >= 1, "bad sizes");
  TARL_REQUIRE(M < DCR_MAX_BLOCKS && M * dcr_tiles(plan) < DCR_MAX_BLOCKS, "too many (row, tile) pairs for one launch");
  TARL_REQUIRE(timestep > 0.0f && std::isfinite(timestep), "timestep must be positive and finite");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0, "obs16 must be 16-byte aligned");
  return TARL_OK;
}

static DcrIn dcr_in(const tarl_plan* plan, const float* obs16, const int32_t* head, const int32_t* frames_left,
                    const double* dist, const int32_t* dest_slot, int64_t num_dests, float timestep) {
  return DcrIn{plan->out_ptr, plan->out_dst, plan->N, (uint32_t)dcr_tiles(plan), obs16, head, frames_left, dist, dest_slot,
               num_dests, (double)timestep};
}

extern "C" int tarl_decision_critic_features(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                                             const int32_t* frames_left, const double* dist, const int32_t* dest_slot,
                                             int64_t num_dests, float timestep, float* feats, tarl_stream stream) {
  const int rc = dcr_check(plan, obs16, M, head, frames_left, dist, dest_slot, num_dests, timestep);
  if (rc) return rc;
  TARL_REQUIRE(feats, "null argument");
  TARL_REQUIRE(((uintptr_t)feats) % 16 == 0, "feats must be 16-byte aligned");
  if (plan->N == 0) return TARL_OK;
  const DcrIn in = dcr_in(plan, obs16, head, frames_left, dist, dest_slot, num_dests, timestep);
  hipLaunchKernelGGL(k_dcr_feats, dim3((unsigned)(M * in.tiles)), dim3(DCR_TILE), 0, (hipStream_t)stream, in, feats);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

static int dcr_check_net(const float* weights, float delay_scale, const float* adv_raw) {
  TARL_REQUIRE(weights && adv_raw, "null argument");
  TARL_REQUIRE(std::isfinite(delay_scale) && delay_scale > 0.0f, "delay_scale must be positive and finite");
  return TARL_OK;
}

extern "C" int tarl_decision_critic_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                                        const int32_t* frames_left, const double* dist, const int32_t* dest_slot,
                                        int64_t num_dests, float timestep, const float* weights, float delay_scale,
                                        const float* adv_raw, float* value, float* adv_out, tarl_stream stream) {
  int rc = dcr_check(plan, obs16, M, head, frames_left, dist, dest_slot, num_dests, timestep);
  if (rc) return rc;
  if ((rc = dcr_check_net(weights, delay_scale, adv_raw))) return rc;
  TARL_REQUIRE(value, "null argument");
  const int64_t mn = M * plan->N;     // elements of adv_raw, value and adv_out: their ranges must not overlap
  auto apart = [mn](const float* a, const float* b) {
    return !a || !b || (uintptr_t)a + (uintptr_t)mn * sizeof(float) <= (uintptr_t)b ||
           (uintptr_t)b + (uintptr_t)mn * sizeof(float) <= (uintptr_t)a;
  };
  TARL_REQUIRE(apart(value, adv_raw) && apart(adv_out, adv_raw) && apart(adv_out, value),
               "value and adv_out may alias neither adv_raw nor each other");
  if (plan->N == 0) return TARL_OK;
  const DcrIn in = dcr_in(plan, obs16, head, frames_left, dist, dest_slot, num_dests, timestep);
  hipLaunchKernelGGL(k_dcr_fwd, dim3((unsigned)(M * in.tiles)), dim3(DCR_TILE), 0, (hipStream_t)stream, in, weights,
                     delay_scale, adv_raw, value, adv_out);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int64_t tarl_decision_critic_loss_scratch_bytes(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 1 || M >= DCR_MAX_BLOCKS) return -1;
  const int64_t pairs = M * dcr_tiles(plan);
  if (pairs >= DCR_MAX_BLOCKS) return -1;
  int64_t per, parts;
  dcr_partition(pairs, &per, &parts);
  return pairs * (int64_t)sizeof(DcrPartial) + parts * DCR_NW * (int64_t)sizeof(float);
}

extern "C" int tarl_decision_critic_loss(const tarl_plan* plan, const float* obs16, int64_t M, const int32_t* head,
                                         const int32_t* frames_left, const double* dist, const int32_t* dest_slot,
                                         int64_t num_dests, float timestep, const float* weights, float delay_scale,
                                         const float* adv_raw, const int32_t* n_live, float coef, float grad_scale,
                                         double* out5, float* grads, void* scratch, tarl_stream stream) {
  int rc = dcr_check(plan, obs16, M, head, frames_left, dist, dest_slot, num_dests, timestep);
  if (rc) return rc;
  if ((rc = dcr_check_net(weights, delay_scale, adv_raw))) return rc;
  TARL_REQUIRE(n_live && out5 && scratch, "null argument");
  TARL_REQUIRE(coef >= 0.0f && std::isfinite(coef) && std::isfinite(grad_scale), "coef must be finite and >= 0, grad_scale "
                                                                                 "finite");
  TARL_REQUIRE(((uintptr_t)scratch) % 8 == 0, "scratch must be 8-byte aligned");
  const DcrIn in = dcr_in(plan, obs16, head, frames_left, dist, dest_slot, num_dests, timestep);
  const int64_t pairs = M * in.tiles;
  int64_t per, parts;
  dcr_partition(pairs, &per, &parts);
  DcrPartial* pair_out = (DcrPartial*)scratch;
  float* partial = (float*)(pair_out + pairs);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_dcr_loss, dim3((unsigned)parts), dim3(DCR_TILE), 0, s, in, weights, delay_scale, adv_raw, n_live, coef,
                     grad_scale, pairs, per, pair_out, partial);
  TARL_LAUNCH_CHECK();
  const unsigned row_blocks = (unsigned)ceil_div(M, 64), grad_blocks = (unsigned)ceil_div(DCR_NW, DCR_TILE / 64);
  hipLaunchKernelGGL(k_dcr_sum, dim3(row_blocks + grad_blocks), dim3(DCR_TILE), 0, s, (const DcrPartial*)pair_out, M,
                     in.tiles, row_blocks, out5, (const float*)partial, parts, grads);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
