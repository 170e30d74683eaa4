// occupancy.hip — per-road occupancy of the vectorised evaluation: the NUMBER_OF_AGENT column that tarl_fused_frame offers
// per frame (`counts`, fp32 [N][B], env-minor, the value AFTER the frame) summed per (environment, time bin, road) on the
// device, with the frames at capacity and the episode's peak.
//
// Reference semantics restated: the reward is -sum_n NUMBER_OF_AGENT after the step (src/rl/environment.py), Direction's
// has_room = n_i < max_i - CONGESTION_FILE (src/direction_mpnn.py) and the insert's capacity rule are its negation
// count >= ceil(MAX - 3) =: thr. So with c_t[b][n] the count after frame t and frame t in bin h_t (the clock at which the
// step STARTED, as link_counts.hip bins it):
//   veh[b][h][n]  = sum over t in bin h of c_t[b][n]            (vehicle-frames)
//   full[b][h][n] = #{t in bin h : c_t[b][n] >= thr[n]}         (frames in which the road admits nobody)
//   peak[b][0][n] = max over t of c_t[b][n]
#include "eval_bins.h"

#define OC_TILE 64              // environments x roads of one workgroup
#define OC_PAD (OC_TILE + 1)    // row stride of the LDS tile, in int32
#define OC_WAVES 4
#define OC_ROWS (OC_TILE / OC_WAVES)      // roads per thread
#define OC_MAX_FRAMES ((int64_t)1 << 23)  // 255 * 2^23 < 2^31: the int32 partial sums of one call cannot overflow

// A value of the ring -> a count in [0, 255] by truncation; NaN and negative values count 0 (`v > 0` is false for NaN),
// anything above 255 counts 255: a foreign value miscounts its own element and nothing else.
__device__ __forceinline__ int32_t oc_count(float v) { return v > 0.0f ? (v >= 255.0f ? 255 : (int32_t)v) : 0; }

// ---- accumulate -------------------------------------------------------------------------------------------------------
// The ring is env-minor ([F][N][K]) and the accumulators env-major ([K][H][N]): a tiled transposition with accumulation.
// One workgroup of 4 waves owns a tile of 64 environments x 64 roads for every frame and every bin and is its only writer:
// no atomics, and integer sums and maxima do not depend on an order.
//   Load side: lane l of wave w owns environment k0 + l of the roads n0 + w + 4 i, i < 16. A wave's load of one road is 64
//   consecutive floats of the ring (256 B along the environment axis). The thread keeps veh / full of the current bin and
//   peak of the whole call in registers (3 x 16 int32) over a run of frames in one bin: per frame there are 16 loads, a
//   conversion, an add, a compare and a max, and nothing else: no division and no LDS traffic.
//   Store side, when the bin changes and after the last frame: each accumulator goes through the LDS tile
//   s[road][environment] and comes back with lane l = road n0 + l and the environments k0 + w + 4 i, so that a wave's
//   read-modify-write of one environment is 64 consecutive int32 along the road axis.
//   Banks (ds_write_b32 / ds_read_b32: bank = dword address % 32, conflicts only within a 32-lane half): the row stride is
//   65 dwords. The write puts lane l at (w + 4 i) * 65 + l: 32 consecutive dwords per half, 32 distinct banks. The
//   transposed read takes lane l at l * 65 + (w + 4 i): bank (l * 65 + c) % 32 = (l + c) % 32 because 65 % 32 = 1, again 32
//   distinct banks per half. Both are conflict-free (a stride of 64 would put all 32 lanes of the read on one bank); where
//   the compiler pairs two reads as ds_read2_b32, the LDS serves them as two such ds_read_b32 accesses.
// Tiles at the K and N edges are partial: a load outside reads the nearest element inside instead (in bounds, and the
// frame loop stays free of branches), the LDS tile is always written in full, and the stores are predicated per element.
//
// oc_flush: the thread's 16 partial results through the tile into dst[i * k_stride], i < k_rows: this lane's road of the
// environments k0 + w + 4 i that exist (k_rows is uniform over the wave). PEAK: max-merge instead of add.
template <bool PEAK>
__device__ __forceinline__ void oc_flush(int32_t (*s)[OC_PAD], const int32_t (&acc)[OC_ROWS], int32_t* dst, int64_t k_stride,
                                         int k_rows, bool n_in, int w, int l) {
  __syncthreads();      // the previous flush's reads are done
#pragma unroll
  for (int i = 0; i < OC_ROWS; ++i) s[w + OC_WAVES * i][l] = acc[i];
  __syncthreads();
  if (!n_in) return;
#pragma unroll 4
  for (int i = 0; i < k_rows; ++i, dst += k_stride) {
    const int32_t v = s[l][w + OC_WAVES * i];
    if (PEAK ? v > *dst : v != 0) *dst = PEAK ? v : *dst + v;
  }
}

__global__ __launch_bounds__(OC_TILE* OC_WAVES) void k_occupancy_accumulate(const float* __restrict__ ring,
                                                                            const int32_t* __restrict__ thr, int64_t F,
                                                                            int64_t K, int64_t N, int64_t H, int64_t t0,
                                                                            int64_t timestep, int64_t bin_seconds,
                                                                            int64_t first_bin, int64_t k_tiles,
                                                                            int32_t* __restrict__ veh,
                                                                            int32_t* __restrict__ full,
                                                                            int32_t* __restrict__ peak) {
  __shared__ int32_t s[OC_TILE][OC_PAD];
  const int l = threadIdx.x & (OC_TILE - 1);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / OC_TILE);      // uniform over the wave: thr[] loads are scalar
  const int64_t k0 = ((int64_t)blockIdx.x % k_tiles) * OC_TILE, n0 = ((int64_t)blockIdx.x / k_tiles) * OC_TILE;
  const bool n_in = n0 + l < N;       // store side: this lane's road exists
  // Load side: an element outside the tile's part of [N][K] reads the nearest one inside (road N - 1, environment K - 1):
  // every load is in bounds and unconditional, and what it accumulates is never stored (the store side is predicated).
  const int64_t kc = k0 + l < K ? k0 + l : K - 1;
  int64_t off[OC_ROWS];
  int32_t th[OC_ROWS], pk[OC_ROWS];
#pragma unroll
  for (int i = 0; i < OC_ROWS; ++i) {
    const int64_t n = n0 + w + OC_WAVES * i < N ? n0 + w + OC_WAVES * i : N - 1;
    off[i] = n * K;
    th[i] = thr[n];
    pk[i] = 0;
  }
  // store side: this lane's road n0 + l of the environments k0 + w + 4 i, i < k_rows
  const int64_t k_left = K - k0 - w;
  const int k_rows = k_left <= 0 ? 0 : (int)(k_left >= OC_TILE ? OC_ROWS : (k_left + OC_WAVES - 1) / OC_WAVES);
  const int64_t e0 = (k0 + w) * H * N + n0 + l;      // element [k0 + w][0][n0 + l] of veh and full
  for (int64_t f = 0; f < F;) {
    int64_t h, f1 = bin_run(t0, timestep, bin_seconds, first_bin, f, F, h);      // the run [f, f1) of frames in bin h
    int32_t av[OC_ROWS], af[OC_ROWS];
#pragma unroll
    for (int i = 0; i < OC_ROWS; ++i) av[i] = af[i] = 0;
    for (; f < f1; ++f) {
      const float* p = ring + f * N * K + kc;
      float v[OC_ROWS];
#pragma unroll
      for (int i = 0; i < OC_ROWS; ++i) v[i] = p[off[i]];      // 16 independent loads in flight
#pragma unroll
      for (int i = 0; i < OC_ROWS; ++i) {
        const int32_t c = oc_count(v[i]);
        av[i] += c;
        af[i] += c >= th[i] ? 1 : 0;
        pk[i] = c > pk[i] ? c : pk[i];
      }
    }
    oc_flush<false>(s, av, veh + e0 + h * N, OC_WAVES * H * N, k_rows, n_in, w, l);
    oc_flush<false>(s, af, full + e0 + h * N, OC_WAVES * H * N, k_rows, n_in, w, l);
  }
  oc_flush<true>(s, pk, peak + (k0 + w) * N + n0 + l, OC_WAVES * N, k_rows, n_in, w, l);
}

extern "C" int tarl_occupancy_accumulate(const float* ring, const int32_t* thr, int64_t F, int64_t K, int64_t N, int64_t t0,
                                         int64_t timestep, int64_t bin_seconds, int64_t first_bin, int64_t H, int32_t* veh,
                                         int32_t* full, int32_t* peak, tarl_stream stream) {
  TARL_REQUIRE(ring && thr && veh && full && peak, "null argument");
  TARL_REQUIRE(F >= 1 && F <= OC_MAX_FRAMES, "F must be in [1, 2^23] (255 F must fit the int32 partial sums)");
  const int64_t lim = (int64_t)1 << 40;
  TARL_REQUIRE(K >= 1 && N >= 1 && H >= 1 && K < lim && N < lim && H < lim && K * N < lim && K * N * H < lim &&
                   K * N * F < lim,
               "bad sizes");
  TARL_REQUIRE_BINS(t0, timestep, bin_seconds, first_bin, F, H);
  const int64_t k_tiles = ceil_div(K, OC_TILE), tiles = k_tiles * ceil_div(N, OC_TILE);
  TARL_REQUIRE(tiles < ((int64_t)1 << 31), "bad sizes: too many tiles for one launch");
  hipLaunchKernelGGL(k_occupancy_accumulate, dim3((unsigned)tiles), dim3(OC_TILE * OC_WAVES), 0, (hipStream_t)stream, ring,
                     thr, F, K, N, H, t0, timestep, bin_seconds, first_bin, k_tiles, veh, full, peak);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
