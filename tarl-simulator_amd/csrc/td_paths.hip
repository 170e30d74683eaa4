// td_paths.hip — the dynamic relative gap of the vectorised evaluation: time-dependent road times from the occupancy sums of
// an episode (tarl_td_road_times) and, per (environment, agent), the earliest clock at which the agent could have left its
// destination road had it known them (tarl_td_hindsight). DESIGN 4.17. For the day-to-day replanning loop the same search also
// returns the PATH (tarl_td_routes).
//
// Road time. veh int32 [K][H][N] and frames_per_bin int32 [H] are the occupancy accumulators of §4.15; with
// cbar = (double)veh / (double)frames_per_bin the time of road n in bin h of environment k is
//   tau[k][h][n] = (float) max(FF[n], cc[n] / ((MAX[n] + 10) - cbar))        (fp64; the sum MAX + 10 first)
// the simulator's own law (oracle/sim.py::direction_update) at the bin's mean count after the frame. A bin without frames
// gets FF[n]; a denominator <= 0 gives +inf; `max` is (v > FF ? v : FF), so a NaN quotient gives FF.
//
// Leaving a road. S(h) = (first_bin + h) * bin_seconds as an integer, converted; env[k][H][n] = +inf and
//   env[k][h][n] = min(S(h) + tau[k][h][n], env[k][h + 1][n])                 (min(x, m) = x < m ? x : m: a NaN x gives m)
// the earliest leaving time over the bins from h on, entered at their start. An agent that enters road n at clock t, in bin
// h = clamp(floor(t) / bin_seconds - first_bin, 0, H - 1) (the clamp of trips.hip: NaN and negatives as 0, 2^62 and above the
// last bin), has left it at leave(n, t) = min(t + tau[k][h][n], env[k][h + 1][n]): waiting for a later, faster bin is allowed,
// which makes leave non-decreasing in t. t = +inf or NaN gives +inf. A NaN tau is +inf in both minima.
//
// Hindsight arrival of agent a in environment k (origin o, destination d, departure t0, fp32 widened):
//   L[o] = leave(o, t0),  L[v] = min over in-edges (u -> v) of leave(v, L[u]),  best[k][a] = L[d]
// the least fixed point, reached by td_labels below from any schedule of the relaxations because leave is non-decreasing:
// every label is at every moment the value of a real path (or +inf), labels only decrease, and a label that changed puts
// its out-neighbours back among the candidates. best = +inf where d is unreachable, an id is out of range, for the dummy row
// 0, and where the agent has DONE != 1 (not searched).
//
// One 256-thread workgroup per search, grid-strided over at most SPT_MAX_WG workgroups; the workgroup owns an fp64 label row
// of N in global scratch and two N-bit bitmaps (frontier, candidates) in LDS: the scheme of sp_trees.h's spt_distances,
// whose functions this file leaves alone. No floating-point atomics; the result does not depend on the schedule, so two
// runs are bit-identical.
#include <math.h>

#include "sp_trees.h"

#define TD_BLOCK 256
#define TD_MAX_BINS 4096              // = TARL_TRIP_MAX_BINS: the bins are those of the per-trip report

// The bin schedule, with the division by bin_seconds prepared on the host. For a clock below 2^32 the quotient is
// umulhi64(magic, clock) with magic = floor((2^64 - 1) / bin_seconds) + 1 = ceil(2^64 / bin_seconds): exact for every 32-bit
// numerator and every divisor >= 2 (Lemire, Kaser, Kurz, "Faster remainder by direct computation", 2019, Theorem 1 with
// N = 32, F = 64). bin_seconds = 1 has magic = 0 (2^64 wraps) and the quotient is the clock itself. A clock from 2^32 on takes
// the 64-bit division; no episode reaches it (136 years of seconds).
struct td_bins {
  int64_t bin_seconds, first_bin;
  uint64_t magic;
  int32_t H;
};

static inline td_bins td_make_bins(int64_t bin_seconds, int64_t first_bin, int64_t H) {
  td_bins b;
  b.bin_seconds = bin_seconds;
  b.first_bin = first_bin;
  b.magic = bin_seconds == 1 ? 0ull : 0xFFFFFFFFFFFFFFFFull / (uint64_t)bin_seconds + 1ull;
  b.H = (int32_t)H;
  return b;
}

__device__ __forceinline__ int32_t td_bin(double t, const td_bins& b) {
  if (!(t > 0.0)) t = 0.0;
  if (t >= 4611686018427387904.0) return b.H - 1;
  const int64_t c = (int64_t)floor(t);
  int64_t q;
  if (c < ((int64_t)1 << 32))
    q = (int64_t)(b.magic ? __umul64hi(b.magic, (uint64_t)c) : (uint64_t)c);
  else
    q = c / b.bin_seconds;
  q -= b.first_bin;
  return q < 0 ? 0 : (q > b.H - 1 ? b.H - 1 : (int32_t)q);
}

// tau_k, env_k: environment k's [H][N] and [H + 1][N] tables
__device__ __forceinline__ double td_leave(const float* __restrict__ tau_k, const double* __restrict__ env_k, int64_t N,
                                           int32_t n, double t, const td_bins& b) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  if (!(t < INF)) return INF;
  const int64_t h = td_bin(t, b);
  const double x = t + (double)tau_k[h * N + n];
  const double m = env_k[(h + 1) * N + n];
  return x < m ? x : m;
}

// ---- road times and their envelope ---------------------------------------------------------------------------------------
// One thread per (k, n), h downwards: consecutive lanes are consecutive roads, every access of a wave is one contiguous
// segment of veh, tau and env.
__global__ __launch_bounds__(TD_BLOCK) void k_td_road_times(const int32_t* __restrict__ veh, const int32_t* __restrict__ fpb,
                                                            const float* __restrict__ mx, const float* __restrict__ ff,
                                                            const float* __restrict__ cc, int64_t H, int64_t N,
                                                            int64_t bin_seconds, int64_t first_bin, float* __restrict__ tau,
                                                            double* __restrict__ env) {
  const int64_t n = (int64_t)blockIdx.x * TD_BLOCK + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (n >= N) return;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const double f = (double)ff[n], c = (double)cc[n], room = (double)mx[n] + 10.0;
  const int32_t* vk = veh + k * H * N;
  float* tk = tau + k * H * N;
  double* ek = env + k * (H + 1) * N;
  double m = INF;
  ek[H * N + n] = m;
  for (int64_t h = H - 1; h >= 0; --h) {
    const int32_t frames = fpb[h];      // wave-uniform
    double t = f;
    if (frames > 0) {
      const double den = room - (double)vk[h * N + n] / (double)frames;
      const double v = den > 0.0 ? c / den : INF;
      t = v > f ? v : f;
    }
    const float t32 = (float)t;
    tk[h * N + n] = t32;
    const double x = (double)((first_bin + h) * bin_seconds) + (double)t32;
    m = x < m ? x : m;
    ek[h * N + n] = m;
  }
}

// ---- the label phase -----------------------------------------------------------------------------------------------------
// Beside spt_distances (sp_trees.h), with leave() in place of dist + w: L [N] (the workgroup's scratch row) <- the earliest
// leaving time of every road for a trip that enters road o at clock t0. Marks over the CSR out-lists, pulls over the CSC
// in-lists. F and C are W-word LDS bitmaps (C is left all zero). Ends on a barrier.
__device__ __forceinline__ void td_labels(const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                          const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                          const float* __restrict__ tau_k, const double* __restrict__ env_k, int64_t N,
                                          int32_t W, int tid, int32_t o, double t0, const td_bins& b, double* L, uint32_t* F,
                                          uint32_t* C) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  for (int64_t v = tid; v < N; v += SPT_BLOCK) L[v] = INF;
  for (int32_t i = tid; i < W; i += SPT_BLOCK) {
    F[i] = 0u;
    C[i] = 0u;
  }
  __syncthreads();
  if (tid == 0) {
    L[o] = td_leave(tau_k, env_k, N, o, t0, b);
    F[o >> 5] = 1u << (o & 31);
  }
  __syncthreads();

  // at most N rounds: after round r every label is at most the best over the paths of r edges
  for (int64_t round = 0; round < N; ++round) {
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
      uint32_t m = F[i];
      while (m) {
        const int32_t u = (i << 5) + __builtin_ctz(m);
        m &= m - 1u;
        const int32_t k1 = out_ptr[u + 1];
        for (int32_t k = out_ptr[u]; k < k1; ++k) {
          const int32_t v = out_dst[k];
          atomicOr(&C[v >> 5], 1u << (v & 31));
        }
      }
    }
    __syncthreads();
    int any = 0;
    for (int32_t i = tid; i < W; i += SPT_BLOCK) {
      uint32_t c = C[i];
      uint32_t nf = 0u;
      if (c) C[i] = 0u;
      while (c) {
        const int bit = __builtin_ctz(c);
        c &= c - 1u;
        const int32_t v = (i << 5) + bit;
        const double old = L[v];
        double best = old;
        const int32_t k1 = in_ptr[v + 1];
        for (int32_t k = in_ptr[v]; k < k1; ++k) {
          const double d = td_leave(tau_k, env_k, N, v, L[in_src[k]], b);
          if (d < best) best = d;
        }
        if (best < old) {
          L[v] = best;
          nf |= 1u << bit;
        }
      }
      F[i] = nf;
      any |= (nf != 0u);
    }
    if (!__syncthreads_or(any)) break;
  }
}

__global__ __launch_bounds__(SPT_BLOCK) void k_td_hindsight(
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, const int32_t* __restrict__ in_ptr,
    const int32_t* __restrict__ in_src, const float* __restrict__ tau, const double* __restrict__ env, int64_t N,
    const float* __restrict__ ag, int64_t K, int64_t A, int64_t a_bstride, td_bins b, uint8_t* __restrict__ scratch,
    int64_t row_bytes, double* __restrict__ best) {
  extern __shared__ uint32_t td_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  uint32_t* F = td_lds;
  uint32_t* C = F + W;
  double* L = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const float Nf = (float)N;      // N <= 327 680: exact

  for (int64_t j = blockIdx.x; j < K * A; j += gridDim.x) {
    const int64_t k = j / A, a = j - k * A;
    const float* row = ag + k * a_bstride + a * AG_COLS;
    const float of = row[AG_ORIGIN], df = row[AG_DEST];
    // uniform over the workgroup: the dummy row, an agent that has not arrived and a foreign id are not searched
    const bool search = a >= 1 && row[AG_DONE] == 1.0f && of >= 0.0f && of < Nf && df >= 0.0f && df < Nf;
    if (!search) {
      if (tid == 0) best[j] = INF;
      continue;
    }
    const int32_t o = (int32_t)of, d = (int32_t)df;
    td_labels(out_ptr, out_dst, in_ptr, in_src, tau + k * b.H * N, env + k * ((int64_t)b.H + 1) * N, N, W, tid, o,
              (double)row[AG_DEP], b, L, F, C);
    if (tid == 0) best[j] = L[d];
    __syncthreads();   // the next search re-initialises the row thread 0 may still be reading
  }
}

// ---- the quickest route per (environment, agent) (NOT reference semantics: the reference has no replanning) ------
// The labels of k_td_hindsight, then the PATH: every agent a >= 1 whose origin and destination are in range is searched from
// its DEPARTURE_TIME whatever its DONE flag (a plan is needed for everybody); best[k][a] = L[d] as above. After the labels
// have converged wave 0 walks back from d: at v != o the in-neighbour u with leave(v, L[u]) == L[v] (fp64 equality; one exists
// at the least fixed point), among several the SMALLEST ROAD ID whatever the order of the in-list — the lanes take the
// in-edges 64 at a time and a wave minimum picks u, so v stays uniform over the wave. With tau >= FF > 0 the labels fall
// strictly along the walk and it cannot cycle; it is nevertheless bounded: a road without a tight in-edge ends it (len = 0)
// and so do more than N roads (len = -1; tau = 0 may close a tight cycle). The walk meets the roads from d backwards, so lane
// 0 pushes them onto a stack of max_hops words behind the workgroup's label row as long as they fit and keeps counting when
// they do not; a route that fits is then copied out forwards, 64 words at a time: routes[k][a][0] = o ..
// routes[k][a][len - 1] = d, o == d gives len = 1. Nothing else of the row is touched.
//   route_len = 0: unreachable destination (best = +inf), dummy row 0, an id out of range (best = +inf), no tight in-edge
//   route_len = -(true length): the route is longer than max_hops; nothing of its row is written.
// Every route_len and best entry is written; route entries from len on are left as allocated.
__global__ __launch_bounds__(SPT_BLOCK) void k_td_routes(
    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, const int32_t* __restrict__ in_ptr,
    const int32_t* __restrict__ in_src, const float* __restrict__ tau, const double* __restrict__ env, int64_t N,
    const float* __restrict__ ag, int64_t K, int64_t A, int64_t a_bstride, td_bins b, uint8_t* __restrict__ scratch,
    int64_t row_bytes, int64_t label_bytes, int32_t max_hops, double* __restrict__ best, int32_t* __restrict__ routes,
    int32_t* __restrict__ route_len) {
  extern __shared__ uint32_t td_lds[];
  const int tid = threadIdx.x;
  const int32_t W = (int32_t)((N + 31) >> 5);
  uint32_t* F = td_lds;
  uint32_t* C = F + W;
  double* L = (double*)(scratch + (int64_t)blockIdx.x * row_bytes);
  int32_t* stack = (int32_t*)(scratch + (int64_t)blockIdx.x * row_bytes + label_bytes);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const float Nf = (float)N;      // N <= 327 680: exact
  const int32_t NONE = 0x7FFFFFFF;

  for (int64_t j = blockIdx.x; j < K * A; j += gridDim.x) {
    const int64_t k = j / A, a = j - k * A;
    const float* row = ag + k * a_bstride + a * AG_COLS;
    const float of = row[AG_ORIGIN], df = row[AG_DEST];
    // uniform over the workgroup: the dummy row and a foreign id are not searched
    const bool search = a >= 1 && of >= 0.0f && of < Nf && df >= 0.0f && df < Nf;
    if (!search) {
      if (tid == 0) {
        best[j] = INF;
        route_len[j] = 0;
      }
      continue;
    }
    const int32_t o = (int32_t)of, d = (int32_t)df;
    const float* tau_k = tau + k * b.H * N;
    const double* env_k = env + k * ((int64_t)b.H + 1) * N;
    td_labels(out_ptr, out_dst, in_ptr, in_src, tau_k, env_k, N, W, tid, o, (double)row[AG_DEP], b, L, F, C);
    if (tid < 64) {      // wave 0; everything below is uniform over it but `u` before the minimum
      const double ld = L[d];
      int64_t cnt = 0;
      if (ld < INF) {
        int32_t v = d;
        cnt = 1;
        if (tid == 0) stack[0] = d;      // (max_hops >= 1)
        while (v != o) {
          const double lv = L[v];
          int32_t u = NONE;
          const int32_t k1 = in_ptr[v + 1];
          for (int32_t e = in_ptr[v] + tid; e < k1; e += 64) {
            const int32_t s = in_src[e];
            if (s < u && td_leave(tau_k, env_k, N, v, L[s], b) == lv) u = s;
          }
          for (int off = 32; off >= 1; off >>= 1) {
            const int32_t w = __shfl_xor(u, off, 64);
            u = w < u ? w : u;
          }
          if (u == NONE) {
            cnt = 0;
            break;
          }
          v = u;
          if (++cnt > N) {
            cnt = -1;
            break;
          }
          if (cnt <= max_hops && tid == 0) stack[cnt - 1] = v;
        }
      }
      if (cnt > max_hops) cnt = -cnt;
      if (cnt > 0) {
        __threadfence_block();      // lane 0's words, before the other lanes read them
        int32_t* r = routes + j * (int64_t)max_hops;
        for (int64_t q = tid; q < cnt; q += 64) r[q] = stack[cnt - 1 - q];
      }
      if (tid == 0) {
        best[j] = ld;
        route_len[j] = (int32_t)cnt;
      }
    }
    __syncthreads();   // the next search re-initialises the row and the stack wave 0 may still be reading
  }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------
#define TD_REQUIRE_BINS()                                                                                      \
  do {                                                                                                         \
    TARL_REQUIRE(bin_seconds >= 1 && bin_seconds < ((int64_t)1 << 40), "bin_seconds must be positive");      \
    TARL_REQUIRE(first_bin >= 0 && first_bin < ((int64_t)1 << 40), "first_bin must be in [0, 2^40)");        \
    TARL_REQUIRE(H >= 1 && H <= TD_MAX_BINS, "H must be in [1, 4096] (TARL_TRIP_MAX_BINS)");                   \
  } while (0)

extern "C" int tarl_td_road_times(const int32_t* veh, const int32_t* frames_per_bin, const float* max_agents,
                                  const float* free_flow, const float* cong, int64_t K, int64_t H, int64_t N,
                                  int64_t bin_seconds, int64_t first_bin, float* tau, double* env, tarl_stream stream) {
  TARL_REQUIRE(veh && frames_per_bin && max_agents && free_flow && cong && tau && env, "null argument");
  const int64_t lim = (int64_t)1 << 31;
  TARL_REQUIRE(K >= 1 && K < 65536 && N >= 1 && N < lim, "bad sizes");
  TD_REQUIRE_BINS();
  TARL_REQUIRE(K * (H + 1) * N < ((int64_t)1 << 40), "bad sizes: K * (H + 1) * N must stay below 2^40");
  const dim3 grid((unsigned)ceil_div(N, TD_BLOCK), (unsigned)K), block(TD_BLOCK);
  hipLaunchKernelGGL(k_td_road_times, grid, block, 0, (hipStream_t)stream, veh, frames_per_bin, max_agents, free_flow, cong,
                     H, N, bin_seconds, first_bin, tau, env);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int64_t tarl_td_hindsight_scratch_bytes(const tarl_plan* plan, int64_t K, int64_t num_agents) {
  if (!plan || K < 1 || num_agents < 1 || K >= ((int64_t)1 << 31) || num_agents >= ((int64_t)1 << 31)) return -1;
  return spt_scratch_bytes(plan, K * num_agents, 8);
}

extern "C" int tarl_td_hindsight(const tarl_plan* plan, const float* tau, const double* env, const float* agents, int64_t K,
                                 int64_t num_agents, int64_t a_bstride, int64_t bin_seconds, int64_t first_bin, int64_t H,
                                 void* scratch, int64_t scratch_bytes, double* best, tarl_stream stream) {
  TARL_REQUIRE(plan && tau && env && agents && best, "null argument");
  const int64_t lim = (int64_t)1 << 31;
  TARL_REQUIRE(K >= 1 && K < lim && num_agents >= 1 && num_agents < lim && K * num_agents < ((int64_t)1 << 40), "bad sizes");
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TD_REQUIRE_BINS();
  const int64_t N = plan->N;
  // the limit of tarl_dest_trees (four bitmaps there, two here): one graph-size limit for every per-road report
  TARL_REQUIRE(4 * 4 * ((N + 31) / 32) <= SPT_LDS_MAX, "graph too large for the hindsight searches (N > 327680)");
  TARL_REQUIRE(N >= 1, "bad sizes: the graph has no road");
  TARL_REQUIRE(scratch && scratch_bytes >= spt_scratch_bytes(plan, K * num_agents, 8),
               "scratch too small (tarl_td_hindsight_scratch_bytes)");
  const int64_t lds = 4 * 2 * ((N + 31) / 32);
  if (lds > 64 * 1024)   // the dynamic-LDS limit only needs raising above the 64 KB default
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_td_hindsight, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_td_hindsight, dim3((unsigned)spt_workgroups(K * num_agents)), dim3(SPT_BLOCK), (size_t)lds,
                     (hipStream_t)stream, plan->out_ptr, plan->out_dst, plan->in_ptr, plan->in_src, tau, env, N, agents, K,
                     num_agents, a_bstride, td_make_bins(bin_seconds, first_bin, H), (uint8_t*)scratch, spt_row_bytes(N, 8),
                     best);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

static bool td_routes_sizes_ok(const tarl_plan* plan, int64_t K, int64_t num_agents, int64_t max_hops) {
  const int64_t lim = (int64_t)1 << 31;
  return plan && K >= 1 && K < lim && num_agents >= 1 && num_agents < lim && K * num_agents < ((int64_t)1 << 40) &&
         max_hops >= 1 && max_hops <= ((int64_t)1 << 20);
}

// a workgroup's scratch row: the fp64 labels of N roads, then the walk's stack of max_hops road ids
static int64_t td_routes_row_bytes(int64_t N, int64_t max_hops) { return spt_row_bytes(N, 8) + (4 * max_hops + 255) / 256 * 256; }

extern "C" int64_t tarl_td_routes_scratch_bytes(const tarl_plan* plan, int64_t K, int64_t num_agents, int64_t max_hops) {
  if (!td_routes_sizes_ok(plan, K, num_agents, max_hops)) return -1;
  return spt_workgroups(K * num_agents) * td_routes_row_bytes(plan->N, max_hops);
}

extern "C" int tarl_td_routes(const tarl_plan* plan, const float* tau, const double* env, const float* agents, int64_t K,
                              int64_t num_agents, int64_t a_bstride, int64_t bin_seconds, int64_t first_bin, int64_t H,
                              int64_t max_hops, void* scratch, int64_t scratch_bytes, double* best, int32_t* routes,
                              int32_t* route_len, tarl_stream stream) {
  TARL_REQUIRE(plan && tau && env && agents && best && routes && route_len, "null argument");
  TARL_REQUIRE(max_hops >= 1 && max_hops <= ((int64_t)1 << 20), "max_hops must be in [1, 2^20]");
  TARL_REQUIRE(td_routes_sizes_ok(plan, K, num_agents, max_hops), "bad sizes");
  TARL_REQUIRE(a_bstride >= num_agents * AG_COLS, "agent tables overlap");
  TD_REQUIRE_BINS();
  const int64_t N = plan->N;
  TARL_REQUIRE(4 * 4 * ((N + 31) / 32) <= SPT_LDS_MAX, "graph too large for the route searches (N > 327680)");
  TARL_REQUIRE(N >= 1, "bad sizes: the graph has no road");
  TARL_REQUIRE(scratch && scratch_bytes >= spt_workgroups(K * num_agents) * td_routes_row_bytes(N, max_hops),
               "scratch too small (tarl_td_routes_scratch_bytes)");
  const int64_t lds = 4 * 2 * ((N + 31) / 32);
  if (lds > 64 * 1024)   // the dynamic-LDS limit only needs raising above the 64 KB default
    TARL_CHECK_HIP(hipFuncSetAttribute((const void*)k_td_routes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_td_routes, dim3((unsigned)spt_workgroups(K * num_agents)), dim3(SPT_BLOCK), (size_t)lds,
                     (hipStream_t)stream, plan->out_ptr, plan->out_dst, plan->in_ptr, plan->in_src, tau, env, N, agents, K,
                     num_agents, a_bstride, td_make_bins(bin_seconds, first_bin, H), (uint8_t*)scratch,
                     td_routes_row_bytes(N, max_hops), spt_row_bytes(N, 8), (int32_t)max_hops, best, routes, route_len);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
