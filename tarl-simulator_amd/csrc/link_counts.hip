// link_counts.hip — per-road link counts of the vectorised evaluation: the frame masks of tarl_fused_frame summed per
// (environment, time bin, road) on the device, and the integer moments of those counts over the environments.
//
// Reference semantics restated: src/transportation_simulator.py:563-746 (compute_node_metrics, plot_daily_counts): the
// per-step masks response_mpnn.update_history (roads whose head was popped) and agent.withdraw_history (roads with at least
// one agent withdrawn), each stamped with the clock at which the step STARTED, are concatenated, binned by
// time // 3600 and summed. So count[b][h][n] = sum over the frames t with floor(clock_t / bin_seconds) == h of
// popped_t[b][n] + withdrawn_t[b][n]; a road popped and withdrawn from in one frame counts 2.
#include "eval_bins.h"

#define LC_BLOCK 256
#define LC_LANES 4   // (b, n) elements per thread == partial sums packed into one 32-bit register, 8 bits each

// ---- accumulate -------------------------------------------------------------------------------------------------------
// [B][N] is one flat axis of M = B * N elements; a frame's masks are M contiguous bytes at f * M. Thread i owns the flat
// elements 4 i .. 4 i + 3 for every frame and every bin and is their only writer: no atomics, and integer sums do not depend
// on an order. Per frame it reads one 32-bit word of each mask where the frame's slice starts on a 4-byte boundary (every
// frame when M % 4 == 0, every fourth frame otherwise; the test is uniform over the launch) and single bytes otherwise; the
// thread that owns the last, partial group always reads bytes, each bounded by M. Only bit 0 of a mask byte is read, so the
// four 8-bit partial sums grow by at most 2 per frame and TARL_LINK_COUNTS_MAX_FRAMES = 127 frames keep every one below 256
// whatever the bytes hold. The partial sums stay in the register for a run of frames in one bin and are added to
// counts[b][h][n] when the bin changes (and after the last frame); every such h is in [0, H) (eval_bins.h).
__device__ __forceinline__ uint32_t lc_load4(const uint8_t* __restrict__ p, int64_t e0, int n_own, bool word) {
  if (word) return *reinterpret_cast<const uint32_t*>(p + e0);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < LC_LANES; ++j)
    if (j < n_own) w |= (uint32_t)p[e0 + j] << (8 * j);
  return w;
}

__global__ __launch_bounds__(LC_BLOCK) void k_link_counts_accumulate(const uint8_t* __restrict__ popped,
                                                                     const uint8_t* __restrict__ withdrawn, int64_t F,
                                                                     int64_t M, int64_t N, int64_t H, int64_t t0,
                                                                     int64_t timestep, int64_t bin_seconds,
                                                                     int64_t first_bin, int32_t* __restrict__ counts) {
  const int64_t e0 = ((int64_t)blockIdx.x * LC_BLOCK + threadIdx.x) * LC_LANES;
  if (e0 >= M) return;
  const int n_own = (int)((M - e0) < LC_LANES ? (M - e0) : LC_LANES);
  for (int64_t f = 0; f < F;) {
    int64_t h, f1 = bin_run(t0, timestep, bin_seconds, first_bin, f, F, h);      // the run [f, f1) of frames in bin h
    uint32_t acc = 0;
#pragma unroll 4
    for (; f < f1; ++f) {
      const uint8_t* pp = popped + f * M;
      const uint8_t* pw = withdrawn + f * M;
      const bool wp = n_own == LC_LANES && (((uintptr_t)pp) & 3) == 0;
      const bool ww = n_own == LC_LANES && (((uintptr_t)pw) & 3) == 0;
      acc += (lc_load4(pp, e0, n_own, wp) & 0x01010101u) + (lc_load4(pw, e0, n_own, ww) & 0x01010101u);
    }
    if (acc != 0) {
#pragma unroll
      for (int j = 0; j < LC_LANES; ++j) {
        const int32_t v = (int32_t)((acc >> (8 * j)) & 0xFFu);
        if (j < n_own && v != 0) {
          const int64_t e = e0 + j, b = e / N;
          counts[(b * H + h) * N + (e - b * N)] += v;
        }
      }
    }
  }
}

extern "C" int tarl_link_counts_accumulate(const uint8_t* popped, const uint8_t* withdrawn, int64_t F, int64_t B, int64_t N,
                                           int64_t t0, int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t H,
                                           int32_t* counts, tarl_stream stream) {
  TARL_REQUIRE(popped && withdrawn && counts, "null argument");
  TARL_REQUIRE(F >= 1 && F <= TARL_LINK_COUNTS_MAX_FRAMES, "F must be in [1, TARL_LINK_COUNTS_MAX_FRAMES]");
  const int64_t lim = (int64_t)1 << 40;
  TARL_REQUIRE(B >= 1 && N >= 1 && H >= 1 && B < lim && N < lim && H < lim && B * N < lim && B * N * H < lim, "bad sizes");
  TARL_REQUIRE_BINS(t0, timestep, bin_seconds, first_bin, F, H);
  const int64_t M = B * N;
  hipLaunchKernelGGL(k_link_counts_accumulate, dim3((unsigned)ceil_div(ceil_div(M, LC_LANES), LC_BLOCK)), dim3(LC_BLOCK), 0,
                     (hipStream_t)stream, popped, withdrawn, F, M, N, H, t0, timestep, bin_seconds, first_bin, counts);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- statistics over the environments -----------------------------------------------------------------------------------
// Per (row, road): d_k = a[k][row][n] (- b[k][row][n]) for row < H and d_k = sum over h of that for the totals row H;
// sum d_k and sum d_k^2 in int64, min and max as int32. A workgroup is 64 roads x 4 slices of the environment axis (k = y,
// y + 4, ...; loads along n coalesced), folded through LDS: integer arithmetic, so the split changes nothing.
#define LS_COLS 64
#define LS_SLICES 4

__global__ __launch_bounds__(LS_COLS* LS_SLICES) void k_link_count_stats(const int32_t* __restrict__ a,
                                                                         const int32_t* __restrict__ b, int64_t K, int64_t H,
                                                                         int64_t N, int64_t* __restrict__ sum,
                                                                         int64_t* __restrict__ sumsq,
                                                                         int32_t* __restrict__ vmin,
                                                                         int32_t* __restrict__ vmax) {
  __shared__ int64_t s_s[LS_SLICES][LS_COLS], s_q[LS_SLICES][LS_COLS], s_lo[LS_SLICES][LS_COLS], s_hi[LS_SLICES][LS_COLS];
  const int x = threadIdx.x, y = threadIdx.y;
  const int64_t n = (int64_t)blockIdx.x * LS_COLS + x, row = blockIdx.y;
  const int64_t h0 = row < H ? row : 0, h1 = row < H ? row + 1 : H;
  int64_t s = 0, q = 0, lo = INT64_MAX, hi = INT64_MIN;
  if (n < N) {
    for (int64_t k = y; k < K; k += LS_SLICES) {
      int64_t d = 0;
      for (int64_t h = h0; h < h1; ++h) {
        const int64_t i = (k * H + h) * N + n;
        d += (int64_t)a[i] - (b ? (int64_t)b[i] : 0);
      }
      s += d;
      q += d * d;
      lo = d < lo ? d : lo;
      hi = d > hi ? d : hi;
    }
  }
  s_s[y][x] = s;
  s_q[y][x] = q;
  s_lo[y][x] = lo;
  s_hi[y][x] = hi;
  __syncthreads();
  if (y == 0 && n < N) {
    for (int j = 1; j < LS_SLICES; ++j) {
      s += s_s[j][x];
      q += s_q[j][x];
      lo = s_lo[j][x] < lo ? s_lo[j][x] : lo;
      hi = s_hi[j][x] > hi ? s_hi[j][x] : hi;
    }
    const int64_t o = row * N + n;
    sum[o] = s;
    sumsq[o] = q;
    vmin[o] = (int32_t)lo;
    vmax[o] = (int32_t)hi;
  }
}

extern "C" int tarl_link_count_stats(const int32_t* counts_a, const int32_t* counts_b, int64_t K, int64_t H, int64_t N,
                                     int64_t* sum, int64_t* sumsq, int32_t* vmin, int32_t* vmax, tarl_stream stream) {
  TARL_REQUIRE(counts_a && sum && sumsq && vmin && vmax, "null argument");
  const int64_t lim = (int64_t)1 << 40;
  TARL_REQUIRE(K >= 1 && H >= 1 && N >= 1 && K < lim && N < lim && H < 65535 && K * H * N < lim, "bad sizes");
  hipLaunchKernelGGL(k_link_count_stats, dim3((unsigned)ceil_div(N, LS_COLS), (unsigned)(H + 1)), dim3(LS_COLS, LS_SLICES), 0,
                     (hipStream_t)stream, counts_a, counts_b, K, H, N, sum, sumsq, vmin, vmax);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
