// tile_sums.h — internal: the launch shape and the ordered sums of the per-decision kernels (decision_credit.hip,
// decision_critic.hip), written once.
//
// Shape: one lane per node, tiles of TS_TILE nodes, the (row, tile) pairs flattened into grid.x (ts_at), fewer than
// TS_MAX_BLOCKS of them in one launch (TS_REQUIRE_PAIRS).
//
// Sums: no floating-point atomics, a fixed order instead — lanes l and l + 32, 16, .., 1 of a wave (ts_wave_sum), the tile's
// waves in order (ts_wave_put, a barrier of the caller's, ts_waves_in_order), the tiles of a row in order (ts_row_sum) — so
// that two runs are bit-identical. K values travel together as double[K]; a (row, tile) pair's K sums are K consecutive
// doubles of the caller's scratch.
#pragma once
#include "tarl_common.h"

#define TS_TILE 256
#define TS_WAVES (TS_TILE / 64)
#define TS_MAX_BLOCKS ((int64_t)1 << 24)     // (row, tile) pairs of one launch: grid.x * TS_TILE stays below 2^32 threads

static inline int64_t ts_tiles(const tarl_plan* plan) { return ceil_div(plan->N > 0 ? plan->N : 1, TS_TILE); }

// false where rows x tiles does not fit one launch (rows first: the product cannot overflow)
static inline bool ts_pairs_fit(int64_t rows, int64_t tiles) { return rows < TS_MAX_BLOCKS && rows * tiles < TS_MAX_BLOCKS; }
#define TS_REQUIRE_PAIRS(rows, tiles) TARL_REQUIRE(ts_pairs_fit(rows, tiles), "too many (row, tile) pairs for one launch")

// the row of this workgroup and the node of this lane (which may lie past N in the last tile of a row)
struct TsAt {
  uint32_t row;
  int64_t node;
};
__device__ __forceinline__ TsAt ts_at(uint32_t tiles) {
  const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  return TsAt{row, (int64_t)tile * TS_TILE + threadIdx.x};
}

// lane 0 of every wave ends with the wave's K sums
template <class T, int K>
__device__ __forceinline__ void ts_wave_sum(T (&v)[K]) {
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] += __shfl_down(v[i], off);
  }
}

// after ts_wave_sum: the wave's sums -> s_red[wave]. Brings no barrier: the caller places one in front of ts_waves_in_order.
template <int K>
__device__ __forceinline__ void ts_wave_put(double (*s_red)[K], const double (&v)[K]) {
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < K; ++i) s_red[threadIdx.x >> 6][i] = v[i];
  }
}

// one thread: the tile's K sums, the waves in order -> out[0 .. K)
template <int K>
__device__ __forceinline__ void ts_waves_in_order(const double (*s_red)[K], double* __restrict__ out) {
  double t[K];
#pragma unroll
  for (int i = 0; i < K; ++i) t[i] = 0.0;
  for (int w = 0; w < TS_WAVES; ++w) {
#pragma unroll
    for (int i = 0; i < K; ++i) t[i] += s_red[w][i];
  }
#pragma unroll
  for (int i = 0; i < K; ++i) out[i] = t[i];
}

// one thread: out[K m .. K m + K) = the K sums of row m over its `tiles` entries of part [rows][tiles][K], in order
template <int K>
__device__ __forceinline__ void ts_row_sum(const double* __restrict__ part, int64_t m, uint32_t tiles,
                                           double* __restrict__ out) {
  double s[K];
#pragma unroll
  for (int i = 0; i < K; ++i) s[i] = 0.0;
  for (uint32_t k = 0; k < tiles; ++k) {
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] += part[(m * tiles + k) * K + i];
  }
#pragma unroll
  for (int i = 0; i < K; ++i) out[K * m + i] = s[i];
}
