// equilibrium.hip — what a link-based equilibrium solver (src/algorithms/equilibrium.py) needs beside the shortest-path
// launches: the step between two all-or-nothing assignments (k_bpr_step) and the all-pairs walk that also returns every
// pair's path cost (k_msa_assign_gap). The per-origin counterpart of the latter lives in msa.hip (k_msa_trees).
//
// k_bpr_step: ONE workgroup of 1024 threads. The step is a chain of up to ~63 dependent full-vector sums (the conjugate
// weights, g(0) / g(1), one g per bisection halving, the closing totals): every sum needs the previous one's result, so
// more workgroups would buy a grid-wide barrier per sum, which costs about what one pass over 25 000 elements costs in a
// single workgroup. Thread t owns the elements t, t + 1024, ... for the whole launch (it re-reads only what it wrote
// itself: no global fence), adds its terms in that order, then a fixed tree: 6 wave shuffles, 16 wave partials through
// LDS, added in wave order by every thread. Same inputs, same bits; no atomics. All arithmetic is fp64 without
// contraction; the fourth power is (r * r) * (r * r).
#include "tarl_common.h"

#define EQ_BLOCK 1024
#define EQ_WAVES (EQ_BLOCK / 64)
#define EQ_MAX_HALVINGS 60
#define EQ_ALPHA_MAX 0.99

// link cost ff * (1 + c * (x / cap)^4): c = 0.15 is the BPR travel time t, c = 0.75 its marginal cost d(x t)/dx
__device__ __forceinline__ double bpr_cost(double ff, double cap, double x, double c) {
  const double r = x / cap;
  const double r2 = r * r;
  return ff * (1.0 + c * (r2 * r2));
}

// d cost / dx = ff * 4c * r^3 / cap
__device__ __forceinline__ double bpr_dcost(double ff, double cap, double x, double c) {
  const double r = x / cap;
  return ff * (4.0 * c) * ((r * r) * r) / cap;
}

// sums of K values over the workgroup, the result in every thread. `red` holds two buffers used in turn, so one barrier
// per call is enough: a thread can only reach the call after next once every thread has left this one.
template <int K>
__device__ __forceinline__ void block_sum(double (&a)[K], double* red, int& phase) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
  double* buf = red + phase * (2 * EQ_WAVES);
  phase ^= 1;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) buf[k * EQ_WAVES + wave] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = buf[k * EQ_WAVES];
    for (int w = 1; w < EQ_WAVES; ++w) s += buf[k * EQ_WAVES + w];
    a[k] = s;
  }
}

__global__ __launch_bounds__(EQ_BLOCK) void k_bpr_step(double* f, const double* y, double* s_prev,
                                                       const double* __restrict__ ff, const double* __restrict__ cap,
                                                       const uint8_t* __restrict__ is_road, int64_t N, int objective,
                                                       int rule, double msa_step, int64_t iteration,
                                                       double* __restrict__ cost_out, double* __restrict__ record) {
  __shared__ double red[2 * 2 * EQ_WAVES];
  int phase = 0;
  const int tid = threadIdx.x;
  const double c = objective == TARL_BPR_SO ? 0.75 : 0.15;
  double alpha = 0.0, lambda = 0.0, g0 = 0.0, g1 = 0.0, halvings = 0.0;

  if (rule != TARL_BPR_EVAL) {
    // the first iteration loads the network: there is no feasible flow to search from yet
    const bool first = iteration <= 1;
    // (i) conjugate weight of the previous target
    if (rule == TARL_BPR_CFW && !first) {
      double a[2] = {0.0, 0.0};
      for (int64_t v = tid; v < N; v += EQ_BLOCK) {
        if (!is_road[v]) continue;
        const double fv = f[v], sp = s_prev[v], yv = y[v];
        const double dh = (sp - fv) * bpr_dcost(ff[v], fmax(cap[v], 1e-8), fv, c);
        a[0] += dh * (yv - fv);
        a[1] += dh * (yv - sp);
      }
      block_sum<2>(a, red, phase);
      if (a[1] != 0.0) {
        alpha = a[0] / a[1];
        if (!(alpha > 0.0)) alpha = 0.0;
        else if (alpha > EQ_ALPHA_MAX) alpha = EQ_ALPHA_MAX;
      }
    }
    // the target s (kept in s_prev from here on), g(0) and g(1)
    {
      double a[2] = {0.0, 0.0};
      for (int64_t v = tid; v < N; v += EQ_BLOCK) {
        const double yv = y[v];
        const double sv = alpha != 0.0 ? alpha * s_prev[v] + (1.0 - alpha) * yv : yv;
        s_prev[v] = sv;
        if (!is_road[v]) continue;
        const double fv = f[v], d = sv - fv, fe = ff[v], cp = fmax(cap[v], 1e-8);
        a[0] += d * bpr_cost(fe, cp, fv, c);
        a[1] += d * bpr_cost(fe, cp, fv + 1.0 * d, c);
      }
      block_sum<2>(a, red, phase);
      g0 = a[0];
      g1 = a[1];
    }
    // (ii) the step
    if (first) lambda = 1.0;
    else if (rule == TARL_BPR_MSA) lambda = msa_step;
    else if (g1 <= 0.0) lambda = 1.0;
    else {
      double lo = 0.0, hi = 1.0;
      for (int it = 0; it < EQ_MAX_HALVINGS; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;       // the last bit of an fp64 lambda
        double a[1] = {0.0};
        for (int64_t v = tid; v < N; v += EQ_BLOCK) {
          if (!is_road[v]) continue;
          const double fv = f[v], d = s_prev[v] - fv;
          a[0] += d * bpr_cost(ff[v], fmax(cap[v], 1e-8), fv + mid * d, c);
        }
        block_sum<1>(a, red, phase);             // the same value in every thread: the branch below is uniform
        if (a[0] < 0.0) lo = mid;
        else hi = mid;
        halvings += 1.0;
      }
      lambda = 0.5 * (lo + hi);
    }
  }

  // (iii) the new flows, their costs and the totals
  double a[2] = {0.0, 0.0};
  for (int64_t v = tid; v < N; v += EQ_BLOCK) {
    double fn = f[v];
    if (rule != TARL_BPR_EVAL) {
      fn = fn + lambda * (s_prev[v] - fn);
      f[v] = fn;
    }
    double cv = 0.0;
    if (is_road[v]) {
      const double fe = ff[v], cp = fmax(cap[v], 1e-8);
      const double t = bpr_cost(fe, cp, fn, 0.15);
      cv = objective == TARL_BPR_SO ? bpr_cost(fe, cp, fn, 0.75) : t;
      a[0] += fn * t;
      a[1] += fn * cv;
    }
    cost_out[v] = cv;
  }
  block_sum<2>(a, red, phase);
  if (tid == 0) {
    record[0] = alpha;
    record[1] = lambda;
    record[2] = a[0];
    record[3] = a[1];
    record[4] = g0;
    record[5] = g1;
    record[6] = halvings;
    record[7] = (double)iteration;
  }
}

// ---- all-pairs walk with the path cost (k_msa_assign of routing.hip plus pair_cost) ----------------------------------------
// One thread per OD pair. pair_cost[p] = ((0 + cost[v1]) + cost[v2]) + ... over the nodes entered, the sum Dijkstra forms
// along that path; +inf when there is no path or an id is out of range. One writer per element: repeatable bit for bit.
#define EQ_PAIR_BLOCK 256
__global__ __launch_bounds__(EQ_PAIR_BLOCK) void k_msa_assign_gap(
    const int64_t* __restrict__ next_hop, int64_t N, const int64_t* __restrict__ od_o, const int64_t* __restrict__ od_d,
    const double* __restrict__ od_vol, int64_t P, const uint8_t* __restrict__ is_road,
    const double* __restrict__ node_cost, double* __restrict__ aux_flow, double* __restrict__ pair_cost) {
  const int64_t p = (int64_t)blockIdx.x * EQ_PAIR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const int64_t o = od_o[p], d = od_d[p];
  const double vol = od_vol[p];
  if (o < 0 || o >= N || d < 0 || d >= N || next_hop[o * N + d] < 0) {
    pair_cost[p] = INF;
    return;
  }
  const bool load = vol > 0.0;
  double sum = 0.0;
  int64_t node = o;
  for (int64_t hops = 0; node != d && hops < N; ++hops) {
    node = next_hop[node * N + d];
    if (node < 0 || node >= N) break;
    sum += node_cost[node];
    if (load && is_road[node]) atomicAdd(&aux_flow[node], vol);
  }
  pair_cost[p] = node == d ? sum : INF;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
extern "C" int tarl_bpr_step(double* flow, const double* aon_flow, double* target_prev, const double* free_flow,
                             const double* capacity, const uint8_t* is_road, int64_t num_nodes, int objective, int rule,
                             double msa_step, int64_t iteration, double* cost_out, double* record, tarl_stream stream) {
  TARL_REQUIRE(flow && free_flow && capacity && is_road && cost_out && record, "null argument");
  TARL_REQUIRE(objective == TARL_BPR_UE || objective == TARL_BPR_SO, "objective must be TARL_BPR_UE or TARL_BPR_SO");
  TARL_REQUIRE(rule >= TARL_BPR_MSA && rule <= TARL_BPR_EVAL, "rule must be one of TARL_BPR_MSA / FW / CFW / EVAL");
  TARL_REQUIRE(rule == TARL_BPR_EVAL || (aon_flow && target_prev), "null argument");
  TARL_REQUIRE(num_nodes >= 0, "bad sizes");
  TARL_REQUIRE(rule != TARL_BPR_MSA || (msa_step >= 0.0 && msa_step <= 1.0), "msa_step must lie in [0, 1]");
  hipLaunchKernelGGL(k_bpr_step, dim3(1), dim3(EQ_BLOCK), 0, (hipStream_t)stream, flow, aon_flow, target_prev,
                     free_flow, capacity, is_road, num_nodes, objective, rule, msa_step, iteration, cost_out, record);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_msa_assign_gap(const int64_t* next_hop, int64_t num_nodes, const int64_t* od_origin,
                                   const int64_t* od_dest, const double* od_volume, int64_t num_pairs,
                                   const uint8_t* is_road, const double* node_cost, double* aux_flow, double* pair_cost,
                                   tarl_stream stream) {
  TARL_REQUIRE(next_hop && od_origin && od_dest && od_volume && is_road && node_cost && aux_flow && pair_cost,
               "null argument");
  TARL_REQUIRE(num_nodes >= 1 && num_pairs >= 0, "bad sizes");
  if (num_pairs == 0) return TARL_OK;
  hipLaunchKernelGGL(k_msa_assign_gap, dim3((unsigned)ceil_div(num_pairs, EQ_PAIR_BLOCK)), dim3(EQ_PAIR_BLOCK), 0,
                     (hipStream_t)stream, next_hop, num_nodes, od_origin, od_dest, od_volume, num_pairs, is_road,
                     node_cost, aux_flow, pair_cost);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
