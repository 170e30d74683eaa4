// trips.hip — per-trip report of the vectorised evaluation: what an episode leaves behind in the K agent tables
// (fp32 [K][A][9], environment k at agents + k * a_bstride, row 0 the dummy) reduced per agent over the environments
// (tarl_trip_agent_stats) and per (environment, time bin) over the agents (tarl_trip_bin_stats).
//
// Reference semantics restated: src/runner.py:147-150 (arrived agents and their mean travel time) and the leg histogram of
// src/transportation_simulator.py:344-351 (departures, arrivals and agents en route per time bin). As in k_episode_summary
// (eval.hip): an agent has ARRIVED when DONE == 1 and its travel time is tt = row[ARRIVAL_TIME] - row[DEPARTURE_TIME] in
// fp32, widened to fp64; it is ON THE WAY when it has not arrived and ON_WAY == 1.
//
// Order of every fp64 sum (the integer results, the minima and the maxima do not depend on an order; no floating-point
// atomics anywhere in this file):
//   tarl_trip_agent_stats, per agent: wave w of the TA_WAVES = 16 waves of a workgroup adds the environments w, w + 16,
//     w + 32, ... in ascending order into its own accumulator, starting from +0.0; the 16 accumulators are then added
//     w = 0, 1, ..., 15, again starting from +0.0. The order depends on K alone.
//   tarl_trip_bin_stats, per (environment, bin): the agents of the bin in the order of `perm` (ascending agent id as
//     ops.trip_departure_order builds it), element j of the segment to leaf j % 256; a leaf adds its elements in ascending j
//     from +0.0; the 64 leaves of a wave are folded by the shfl_down tree (offsets 32, 16, ..., 1); the four wave sums are
//     added left to right from +0.0. The order depends on the segment alone.
// Neither order depends on a_bstride, on the grid or on the run: two runs on the same input are bit-identical.
#include <math.h>

#include "tarl_common.h"

#define TA_WAVES 16                 // environments in flight per agent: K = 1 024 gives each wave 64 rows per agent
#define TA_AGENTS 64                // agents per workgroup: lane l of every wave owns agent a0 + l
#define TA_BLOCK (TA_WAVES * TA_AGENTS)
#define TB_BLOCK 256                // leaves of one (environment, bin) segment
#define TB_ARR_BLOCK 1024           // threads of the arrivals pass over one environment
#define TRIP_MAX_BINS 4096          // = TARL_TRIP_MAX_BINS: the arrivals histogram of one environment in LDS (16 KB)

// ---- per agent over the environments -------------------------------------------------------------------------------------
// A transposed reduction: consecutive agents are 36 B apart and consecutive environments a_bstride floats. Lane l of each of
// the 16 waves owns agent a0 + l, so one load instruction of a wave covers 64 consecutive rows (2 304 contiguous bytes, 18
// cache lines, which the loads of the four columns share) and the 16 waves of a workgroup keep 16 environments in flight
// per agent: ceil(A / 64) workgroups x 16 waves, 4 112 waves at A = 16 385. All four columns are loaded unconditionally
// (no divergence; the values of an agent that has not arrived are dropped by a select). The partial results of the waves
// meet in LDS as [quantity][wave][lane] (the 64 lanes of one access are consecutive words: conflict-free), first the fp64
// sums, then in the same 32 KB the counts and extrema; wave 0 adds them in wave order and stores: every output element has
// one writer.
struct trip_acc {
  int32_t n_done, n_way, n_under, n_both, n_faster, n_slower;
  double s1, s2, d1, d2;
  float mn, mx;
};

template <bool PAIR>
__device__ __forceinline__ void trip_row(const float* __restrict__ ra, const float* __restrict__ rb, double ff, trip_acc& c) {
  const float dep = ra[AG_DEP], arr = ra[AG_ARR], way = ra[AG_ON_WAY], dn = ra[AG_DONE];
  const bool done = dn == 1.0f;
  const float tt = arr - dep;
  const double t = (double)tt;
  c.n_done += done ? 1 : 0;
  c.n_way += (!done && way == 1.0f) ? 1 : 0;
  c.n_under += (done && t < ff) ? 1 : 0;
  c.s1 += done ? t : 0.0;
  c.s2 += done ? t * t : 0.0;
  c.mn = done ? fminf(c.mn, tt) : c.mn;
  c.mx = done ? fmaxf(c.mx, tt) : c.mx;
  if (PAIR) {
    const float depb = rb[AG_DEP], arrb = rb[AG_ARR], dnb = rb[AG_DONE];
    const bool both = done && dnb == 1.0f;
    const double d = t - (double)(arrb - depb);
    c.n_both += both ? 1 : 0;
    c.d1 += both ? d : 0.0;
    c.d2 += both ? d * d : 0.0;
    c.n_faster += (both && d < 0.0) ? 1 : 0;
    c.n_slower += (both && d > 0.0) ? 1 : 0;
  }
}

template <bool PAIR>
__global__ __launch_bounds__(TA_BLOCK) void k_trip_agent_stats(
    const float* __restrict__ ag, const float* __restrict__ agb, const double* __restrict__ ff, int64_t K, int64_t A,
    int64_t a_bstride, int64_t b_bstride, int32_t* __restrict__ n_under, int32_t* __restrict__ n_done,
    int32_t* __restrict__ n_way, double* __restrict__ tt_sum, double* __restrict__ tt_sumsq, float* __restrict__ tt_min,
    float* __restrict__ tt_max, int32_t* __restrict__ n_both, double* __restrict__ d_sum, double* __restrict__ d_sumsq,
    int32_t* __restrict__ n_faster, int32_t* __restrict__ n_slower) {
  // one 32 KB buffer, used twice: the four fp64 quantities first, then the eight 32-bit ones
  __shared__ double s_f64[4][TA_WAVES][TA_AGENTS];
  int32_t(*s_i32)[TA_WAVES][TA_AGENTS] = reinterpret_cast<int32_t(*)[TA_WAVES][TA_AGENTS]>(&s_f64[0][0][0]);
  float(*s_f32)[TA_WAVES][TA_AGENTS] = reinterpret_cast<float(*)[TA_WAVES][TA_AGENTS]>(&s_f64[3][0][0]);
  const int l = threadIdx.x & (TA_AGENTS - 1), w = threadIdx.x / TA_AGENTS;
  const int64_t a = (int64_t)blockIdx.x * TA_AGENTS + l;
  const bool live = a >= 1 && a < A;      // the dummy row and the lanes past the last agent read nothing
  const bool writer = w == 0 && a < A;
  trip_acc c = {0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
  if (live) {
    const float* ra = ag + a * AG_COLS;
    const float* rb = PAIR ? agb + a * AG_COLS : nullptr;
    double f = ff ? ff[a] : -INFINITY;      // without a finite ff no travel time lies below it
    f = isfinite(f) ? f : -INFINITY;
#pragma unroll 4
    for (int64_t k = w; k < K; k += TA_WAVES) trip_row<PAIR>(ra + k * a_bstride, PAIR ? rb + k * b_bstride : nullptr, f, c);
  }
  trip_acc t = {0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
  s_f64[0][w][l] = c.s1;
  s_f64[1][w][l] = c.s2;
  if (PAIR) {
    s_f64[2][w][l] = c.d1;
    s_f64[3][w][l] = c.d2;
  }
  __syncthreads();
  if (writer)
    for (int v = 0; v < TA_WAVES; ++v) {      // wave order: the fixed order of the fp64 sums
      t.s1 += s_f64[0][v][l];
      t.s2 += s_f64[1][v][l];
      if (PAIR) {
        t.d1 += s_f64[2][v][l];
        t.d2 += s_f64[3][v][l];
      }
    }
  __syncthreads();
  s_i32[0][w][l] = c.n_done;      // s_i32[0 .. 5] and s_f32[0 .. 1] = words 6 and 7: 8 x 4 KB of the same buffer
  s_i32[1][w][l] = c.n_way;
  s_i32[2][w][l] = c.n_under;
  s_f32[0][w][l] = c.mn;
  s_f32[1][w][l] = c.mx;
  if (PAIR) {
    s_i32[3][w][l] = c.n_both;
    s_i32[4][w][l] = c.n_faster;
    s_i32[5][w][l] = c.n_slower;
  }
  __syncthreads();
  if (!writer) return;
  for (int v = 0; v < TA_WAVES; ++v) {
    t.n_done += s_i32[0][v][l];
    t.n_way += s_i32[1][v][l];
    t.n_under += s_i32[2][v][l];
    t.mn = fminf(t.mn, s_f32[0][v][l]);
    t.mx = fmaxf(t.mx, s_f32[1][v][l]);
    if (PAIR) {
      t.n_both += s_i32[3][v][l];
      t.n_faster += s_i32[4][v][l];
      t.n_slower += s_i32[5][v][l];
    }
  }
  n_done[a] = t.n_done;
  n_way[a] = t.n_way;
  if (n_under) n_under[a] = t.n_under;
  tt_sum[a] = t.s1;
  tt_sumsq[a] = t.s2;
  tt_min[a] = a == 0 ? 0.0f : t.mn;       // entry 0 is written as zero; an agent that never arrived keeps +inf / -inf
  tt_max[a] = a == 0 ? 0.0f : t.mx;
  if (PAIR) {
    n_both[a] = t.n_both;
    d_sum[a] = t.d1;
    d_sumsq[a] = t.d2;
    n_faster[a] = t.n_faster;
    n_slower[a] = t.n_slower;
  }
}

extern "C" int tarl_trip_agent_stats(const float* agents, const float* agents_b, const double* ff, int64_t K,
                                     int64_t num_agents, int64_t a_bstride, int64_t b_bstride, int32_t* n_under,
                                     int32_t* n_done, int32_t* n_way, double* tt_sum, double* tt_sumsq, float* tt_min,
                                     float* tt_max, int32_t* n_both, double* d_sum, double* d_sumsq, int32_t* n_faster,
                                     int32_t* n_slower, tarl_stream stream) {
  TARL_REQUIRE(agents && n_done && n_way && tt_sum && tt_sumsq && tt_min && tt_max, "null argument");
  TARL_REQUIRE(!ff == !n_under, "null argument: ff and n_under come together");
  TARL_REQUIRE(!agents_b || (n_both && d_sum && d_sumsq && n_faster && n_slower),
               "null argument: agents_b needs the paired outputs");
  const int64_t lim = (int64_t)1 << 31;
  TARL_REQUIRE(K >= 1 && K < lim && num_agents >= 1 && num_agents < lim, "bad sizes");
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TARL_REQUIRE(!agents_b || b_bstride >= num_agents * AG_COLS, "agent tables overlap (agents_b)");
  const dim3 grid((unsigned)ceil_div(num_agents, TA_AGENTS)), block(TA_BLOCK);
  if (agents_b)
    hipLaunchKernelGGL(k_trip_agent_stats<true>, grid, block, 0, (hipStream_t)stream, agents, agents_b, ff, K, num_agents,
                       a_bstride, b_bstride, n_under, n_done, n_way, tt_sum, tt_sumsq, tt_min, tt_max, n_both, d_sum, d_sumsq,
                       n_faster, n_slower);
  else
    hipLaunchKernelGGL(k_trip_agent_stats<false>, grid, block, 0, (hipStream_t)stream, agents, agents_b, ff, K, num_agents,
                       a_bstride, b_bstride, n_under, n_done, n_way, tt_sum, tt_sumsq, tt_min, tt_max, n_both, d_sum, d_sumsq,
                       n_faster, n_slower);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- per (environment, time bin) over the agents ------------------------------------------------------------------------
// The bin of a clock value c: clamp((int64)floorf(c) / bin_seconds - first_bin, 0, H - 1). A NaN or a negative clock is
// taken as 0 and a clock from 2^62 on belongs to the last bin, so that the conversion is defined for every float;
// first_bin >= 0, so a negative clock falls in bin 0 either way.
__device__ __forceinline__ int32_t trip_bin(float c, int64_t bin_seconds, int64_t first_bin, int32_t H) {
  if (!(c > 0.0f)) c = 0.0f;
  if (c >= 4611686018427387904.0f) return H - 1;
  const int64_t q = (int64_t)floorf(c) / bin_seconds - first_bin;
  return q < 0 ? 0 : (q > H - 1 ? H - 1 : (int32_t)q);
}

// Binned by departure. The departure of an agent is the same in every environment, so the caller sorts the agents by
// departure bin once per population: perm int32 [A - 1] lists the agents 1 .. A - 1 bin by bin and seg int32 [H + 1] the
// start of every bin's segment in perm (seg[H] = A - 1). Workgroup (k, h) reduces segment h of environment k: a gather of
// rows (4 of their 9 columns), the counts and fp64 sums through the tree described at the top of the file, one writer per
// output element. An entry of perm outside [1, A) is skipped and seg is clamped to [0, A - 1]: foreign values miscount,
// they never leave the tables.
template <bool FF>
__global__ __launch_bounds__(TB_BLOCK) void k_trip_bins_departure(
    const float* __restrict__ ag, int64_t A, int64_t a_bstride, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ seg, const double* __restrict__ ff, int64_t H, int32_t* __restrict__ dep_done,
    int32_t* __restrict__ dep_way, double* __restrict__ dep_tt, double* __restrict__ dep_ff, int32_t* __restrict__ dep_ff_n) {
  __shared__ double s_f64[2][TB_BLOCK / 64];
  __shared__ int32_t s_i32[3][TB_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t k = (int64_t)blockIdx.x / H, h = (int64_t)blockIdx.x % H;
  const float* agk = ag + k * a_bstride;
  int64_t j0 = seg[h], j1 = seg[h + 1];
  j0 = j0 < 0 ? 0 : (j0 > A - 1 ? A - 1 : j0);
  j1 = j1 < j0 ? j0 : (j1 > A - 1 ? A - 1 : j1);
  int32_t n_done = 0, n_way = 0, n_ff = 0;
  double s_tt = 0.0, s_ff = 0.0;
  for (int64_t j = j0 + tid; j < j1; j += TB_BLOCK) {
    const int64_t a = perm[j];
    if (a < 1 || a >= A) continue;
    const float* row = agk + a * AG_COLS;
    if (row[AG_DONE] == 1.0f) {
      const float tt = row[AG_ARR] - row[AG_DEP];
      ++n_done;
      s_tt += (double)tt;
      if (FF) {
        const double f = ff[a];
        if (isfinite(f)) {
          s_ff += f;
          ++n_ff;
        }
      }
    } else if (row[AG_ON_WAY] == 1.0f) {
      ++n_way;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    n_done += __shfl_down(n_done, off);
    n_way += __shfl_down(n_way, off);
    s_tt += __shfl_down(s_tt, off);
    if (FF) {
      n_ff += __shfl_down(n_ff, off);
      s_ff += __shfl_down(s_ff, off);
    }
  }
  if (lane == 0) {
    s_i32[0][wid] = n_done;
    s_i32[1][wid] = n_way;
    s_i32[2][wid] = n_ff;
    s_f64[0][wid] = s_tt;
    s_f64[1][wid] = s_ff;
  }
  __syncthreads();
  if (tid != 0) return;
  int32_t c0 = 0, c1 = 0, c2 = 0;
  double t0 = 0.0, t1 = 0.0;
  for (int v = 0; v < TB_BLOCK / 64; ++v) {
    c0 += s_i32[0][v];
    c1 += s_i32[1][v];
    c2 += s_i32[2][v];
    t0 += s_f64[0][v];
    t1 += s_f64[1][v];
  }
  dep_done[blockIdx.x] = c0;
  dep_way[blockIdx.x] = c1;
  dep_tt[blockIdx.x] = t0;
  if (FF) {
    dep_ff[blockIdx.x] = t1;
    dep_ff_n[blockIdx.x] = c2;
  }
}

// Binned by arrival, which differs between the environments: one workgroup per environment over its table, the histogram
// in LDS through integer atomics (independent of the order), every bin stored by one thread.
__global__ __launch_bounds__(TB_ARR_BLOCK) void k_trip_bins_arrival(const float* __restrict__ ag, int64_t A,
                                                                    int64_t a_bstride, int64_t bin_seconds,
                                                                    int64_t first_bin, int32_t H,
                                                                    int32_t* __restrict__ arr) {
  extern __shared__ int32_t s_arr[];
  const int tid = threadIdx.x;
  for (int32_t i = tid; i < H; i += TB_ARR_BLOCK) s_arr[i] = 0;
  __syncthreads();
  const float* agk = ag + (int64_t)blockIdx.x * a_bstride;
  for (int64_t a = 1 + tid; a < A; a += TB_ARR_BLOCK) {
    const float* row = agk + a * AG_COLS;
    if (row[AG_DONE] == 1.0f) atomicAdd(&s_arr[trip_bin(row[AG_ARR], bin_seconds, first_bin, H)], 1);
  }
  __syncthreads();
  for (int32_t i = tid; i < H; i += TB_ARR_BLOCK) arr[(int64_t)blockIdx.x * H + i] = s_arr[i];
}

extern "C" int tarl_trip_bin_stats(const float* agents, int64_t K, int64_t num_agents, int64_t a_bstride,
                                   const int32_t* perm, const int32_t* seg, const double* ff, int64_t bin_seconds,
                                   int64_t first_bin, int64_t H, int32_t* dep_done, int32_t* dep_way, int32_t* arr,
                                   double* dep_tt, double* dep_ff, int32_t* dep_ff_n, tarl_stream stream) {
  TARL_REQUIRE(agents && perm && seg && dep_done && dep_way && arr && dep_tt, "null argument");
  TARL_REQUIRE(!ff || (dep_ff && dep_ff_n), "null argument: ff needs dep_ff and dep_ff_n");
  const int64_t lim = (int64_t)1 << 31;
  TARL_REQUIRE(K >= 1 && K < lim && num_agents >= 1 && num_agents < lim, "bad sizes");
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TARL_REQUIRE(bin_seconds >= 1 && bin_seconds < ((int64_t)1 << 40), "bin_seconds must be positive");
  TARL_REQUIRE(first_bin >= 0 && first_bin < ((int64_t)1 << 40), "first_bin must be in [0, 2^40)");
  TARL_REQUIRE(H >= 1 && H <= TRIP_MAX_BINS, "H must be in [1, 4096] (TARL_TRIP_MAX_BINS)");
  TARL_REQUIRE(K * H < lim, "bad sizes: too many (environment, bin) pairs for one launch");
  const dim3 grid((unsigned)(K * H)), block(TB_BLOCK);
  if (ff)
    hipLaunchKernelGGL(k_trip_bins_departure<true>, grid, block, 0, (hipStream_t)stream, agents, num_agents, a_bstride, perm,
                       seg, ff, H, dep_done, dep_way, dep_tt, dep_ff, dep_ff_n);
  else
    hipLaunchKernelGGL(k_trip_bins_departure<false>, grid, block, 0, (hipStream_t)stream, agents, num_agents, a_bstride, perm,
                       seg, ff, H, dep_done, dep_way, dep_tt, dep_ff, dep_ff_n);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_trip_bins_arrival, dim3((unsigned)K), dim3(TB_ARR_BLOCK), (size_t)H * sizeof(int32_t),
                     (hipStream_t)stream, agents, num_agents, a_bstride, bin_seconds, first_bin, (int32_t)H, arr);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
