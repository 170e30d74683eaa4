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
// (f3 = f4 = f5 = 0 where no neighbour is reachable), and the network is the 8 -> 16 (ReLU) -> 1 of mlp8.h (its operation
// order, its flat layout of MLP8_NW floats), so that a numpy fp32 restatement reproduces features and values bit for bit.
//
//   k_dcr_feats   the features, zeros where the decision is not live (test hook).
//   k_dcr_fwd     value = y^ and optionally adv_out = adv_raw + delay_scale * y^, zeros where not live.
//   k_dcr_loss    features, forward, smooth-L1 loss against y = -adv_raw / delay_scale and the backward in one launch;
//   k_dcr_sum     the ordered sums behind it.
//
// The launch shape and the fp64 sums are tile_sums.h's: one lane per node, the (row, tile) pairs flattened. In the loss
// kernel a workgroup owns a fixed run of consecutive pairs (a function of M and N alone). The live lanes of a tile are
// compacted through LDS in node order (a ballot and a prefix count per wave, the waves in order) and become the staged
// rows of mlp8.h's gradient scheme: the scheme without the dead lanes, which are most of a tile (measured: 14.3 / 15.4 /
// 13.5 us against 17.0 / 17.4 / 17.1 us without the compaction); the partitions then meet in a fixed tree. No
// floating-point atomics: two runs are bit-identical.
#include <math.h>

#include "mlp8.h"
#include "tile_sums.h"

static_assert(MLP8_ROWS == TS_TILE, "a tile's live lanes fill at most one staging tile");
#define DCR_MAX_PARTS 1024                  // partial-sum rows of the loss at most
#define DCR_OBS_DEST 8                      // obs16 columns: {MAXN, NUMBER_OF_AGENT, FF, ..., [8] = DESTINATION of the head}
#define DCR_SUMS 5                          // per (row, tile) pair and per row: {loss, live, y, y^2, (y - value)^2} in fp64

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
                                             float f[MLP8_NF]) {
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

// Must move per (row, road): 4 B of head; on a live road 64 B of its observation row, per out-neighbour 8 B of dist and
// 8 B of observation (scattered), and 32 B of features written (zeros elsewhere).
__global__ __launch_bounds__(TS_TILE) void k_dcr_feats(DcrIn in, float* __restrict__ feats) {
  const auto [m, u] = ts_at(in.tiles);
  if (u >= in.N) return;
  const int64_t at = (int64_t)m * in.N + u;
  float f[MLP8_NF];
#pragma unroll
  for (int k = 0; k < MLP8_NF; ++k) f[k] = 0.0f;
  if (in.head[at] > 0) dcr_features(in, in.obs + (int64_t)m * in.N * 16, u, in.frames_left[m], f);
  float4* o = reinterpret_cast<float4*>(feats + at * MLP8_NF);
  o[0] = make_float4(f[0], f[1], f[2], f[3]);
  o[1] = make_float4(f[4], f[5], f[6], f[7]);
}

__global__ __launch_bounds__(TS_TILE) void k_dcr_fwd(DcrIn in, const float* __restrict__ w, float delay_scale,
                                                      const float* __restrict__ adv_raw, float* __restrict__ value,
                                                      float* __restrict__ adv_out) {
  const auto [m, u] = ts_at(in.tiles);
  if (u >= in.N) return;
  const int64_t at = (int64_t)m * in.N + u;
  float y = 0.0f, a = 0.0f;
  if (in.head[at] > 0) {
    float f[MLP8_NF];
    dcr_features(in, in.obs + (int64_t)m * in.N * 16, u, in.frames_left[m], f);
    y = mlp8_eval(w, f);
    if (adv_out) a = adv_raw[at] + delay_scale * y;
  }
  value[at] = y;
  if (adv_out) adv_out[at] = a;
}

// Workgroup p owns the pairs [p * per, min((p + 1) * per, M * tiles)). Per pair: every lane evaluates its road, the live
// lanes become the staged rows (mlp8.h) in node order; the pair's DCR_SUMS sums go to pair_out through tile_sums.h's fixed
// tree, whose wave results share the staging's barrier. The hidden layer is evaluated twice (before and after the
// compaction) rather than kept in 48 registers, one hidden unit per turn both times (mlp8.h, UNROLL_J = 1).
__global__ __launch_bounds__(TS_TILE) void k_dcr_loss(DcrIn in, const float* __restrict__ w, float delay_scale,
                                                      const float* __restrict__ adv_raw, const int32_t* __restrict__ n_live,
                                                      float coef, float grad_scale, int64_t pairs, int64_t per,
                                                      double* __restrict__ pair_out, float* __restrict__ partial) {
  MLP8_STAGE_ARRAYS;
  __shared__ double s_red[TS_WAVES][DCR_SUMS];
  __shared__ int s_cnt[TS_WAVES];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int32_t L = n_live[0];
  const float c = L > 0 ? (coef * grad_scale) / (float)L : 0.0f;
  const int64_t p0 = (int64_t)blockIdx.x * per, p1 = (p0 + per < pairs) ? p0 + per : pairs;
  float acc = 0.0f;
  for (int64_t pair = p0; pair < p1; ++pair) {
    const int64_t m = pair / in.tiles;
    const int64_t u = (pair - m * in.tiles) * TS_TILE + t;
    const int64_t at = m * in.N + u;
    const bool live = u < in.N && in.head[at] > 0;
    float f[MLP8_NF], r = 0.0f;
    double v[DCR_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
      dcr_features(in, in.obs + m * in.N * 16, u, in.frames_left[m], f);
      const float yh = mlp8_eval<1>(w, f);
      const float y = (-adv_raw[at]) / delay_scale;
      const float e = yh - y;
      const float ae = fabsf(e);
      const float l = ae < 1.0f ? (0.5f * e) * e : ae - 0.5f;
      const float de = ae < 1.0f ? e : (e > 0.0f ? 1.0f : -1.0f);
      r = c * de;
      v[0] = (double)l;
      v[1] = 1.0;
      v[2] = (double)y;
      v[3] = (double)y * (double)y;
      v[4] = (double)e * (double)e;
    }
    const uint64_t ball = __ballot(live);
    __syncthreads();     // the previous pair has been summed
    if (lane == 0) s_cnt[wid] = __popcll(ball);
    __syncthreads();
    int base = 0, n = 0;
#pragma unroll
    for (int k = 0; k < TS_WAVES; ++k) {
      if (k < wid) base += s_cnt[k];
      n += s_cnt[k];
    }
    if (live) {     // the hidden layer once more (the same operations), straight into the compacted rows
      const int at_s = base + __popcll(ball & (((uint64_t)1 << lane) - 1));
#pragma unroll 1
      for (int j = 0; j < MLP8_NH; ++j) mlp8_row_unit(w, f, r, j, &s_a[at_s][j], &s_h[at_s][j]);
#pragma unroll
      for (int k = 0; k < MLP8_NF; ++k) s_f[at_s][k] = f[k];
      s_r[at_s] = r;
    }
    ts_wave_sum(v);
    ts_wave_put(s_red, v);
    __syncthreads();
    MLP8_ACCUMULATE(acc, t, n)
    else if (t == TS_TILE - 1) ts_waves_in_order(s_red, pair_out + pair * DCR_SUMS);
  }
  mlp8_write_partial(partial, blockIdx.x, t, acc);
}

// blocks 0 .. ceil(M / 64) - 1: out5 of 64 rows each, the tiles in order; the blocks behind them: one wave per gradient
// element, lane l adds the partitions l, l + 64, .. in order and the lanes meet in the wave tree, so that the sum depends on
// the number of partitions alone. (One thread per element walking up to 1024 partitions one dependent load at a time took
// 130 us at 512 partitions, several times the loss kernel itself.) That walk is k_goal_bwd_sum's (goal_mlp.hip), which keeps
// it: the two add in different orders, and sharing either would change the other's gradient bits (mlp8.h).
__global__ __launch_bounds__(TS_TILE) void k_dcr_sum(const double* __restrict__ pair_out, int64_t M, uint32_t tiles,
                                                     uint32_t row_blocks, double* __restrict__ out5,
                                                     const float* __restrict__ partial, int64_t parts,
                                                     float* __restrict__ grads) {
  const int t = threadIdx.x;
  if (blockIdx.x >= row_blocks) {
    const int e = (int)(blockIdx.x - row_blocks) * TS_WAVES + (t >> 6), lane = t & 63;
    if (!grads || e >= MLP8_NW) return;       // wave-uniform
    float s[1] = {0.0f};
    for (int64_t p = lane; p < parts; p += 64) s[0] = s[0] + partial[p * MLP8_NW + e];
    ts_wave_sum(s);
    if (lane == 0) grads[e] = grads[e] + s[0];
    return;
  }
  const int64_t m = (int64_t)blockIdx.x * 64 + t;
  if (t < 64 && m < M) ts_row_sum<DCR_SUMS>(pair_out, m, tiles, out5);
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
  TS_REQUIRE_PAIRS(M, ts_tiles(plan));
  TARL_REQUIRE(timestep > 0.0f && std::isfinite(timestep), "timestep must be positive and finite");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0, "obs16 must be 16-byte aligned");
  return TARL_OK;
}

static DcrIn dcr_in(const tarl_plan* plan, const float* obs16, const int32_t* head, const int32_t* frames_left,
                    const double* dist, const int32_t* dest_slot, int64_t num_dests, float timestep) {
  return DcrIn{plan->out_ptr, plan->out_dst, plan->N, (uint32_t)ts_tiles(plan), obs16, head, frames_left, dist, dest_slot,
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
  hipLaunchKernelGGL(k_dcr_feats, dim3((unsigned)(M * in.tiles)), dim3(TS_TILE), 0, (hipStream_t)stream, in, feats);
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
  hipLaunchKernelGGL(k_dcr_fwd, dim3((unsigned)(M * in.tiles)), dim3(TS_TILE), 0, (hipStream_t)stream, in, weights,
                     delay_scale, adv_raw, value, adv_out);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int64_t tarl_decision_critic_loss_scratch_bytes(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 1 || !ts_pairs_fit(M, ts_tiles(plan))) return -1;
  const int64_t pairs = M * ts_tiles(plan);
  int64_t per, parts;
  dcr_partition(pairs, &per, &parts);
  return pairs * DCR_SUMS * (int64_t)sizeof(double) + parts * MLP8_NW * (int64_t)sizeof(float);
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
  double* pair_out = (double*)scratch;
  float* partial = (float*)(pair_out + pairs * DCR_SUMS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_dcr_loss, dim3((unsigned)parts), dim3(TS_TILE), 0, s, in, weights, delay_scale, adv_raw, n_live, coef,
                     grad_scale, pairs, per, pair_out, partial);
  TARL_LAUNCH_CHECK();
  const unsigned row_blocks = (unsigned)ceil_div(M, 64), grad_blocks = (unsigned)ceil_div(MLP8_NW, TS_WAVES);
  hipLaunchKernelGGL(k_dcr_sum, dim3(row_blocks + grad_blocks), dim3(TS_TILE), 0, s, (const double*)pair_out, M,
                     in.tiles, row_blocks, out5, (const float*)partial, parts, grads);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
