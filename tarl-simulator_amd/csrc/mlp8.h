// mlp8.h — internal: the 8 -> 16 (ReLU) -> 1 network of the goal head (goal_mlp.hip) and of the decision critic
// (decision_critic.hip), written once: its flat layout, its forward, and the gradient scheme of both backward kernels.
//
//     pre_j = b1[j] + sum_{k = 0..7} W1[j][k] * f_k   (k ascending, a multiply then an add: -ffp-contract=off, no FMA)
//     y     = b2 + sum_{j = 0..15} w2[j] * relu(pre_j) (j ascending)
//
// so that a numpy fp32 restatement reproduces every value bit for bit. weights / grads: 161 floats, W1 [16][8] at 0, b1 [16]
// at 128, w2 [16] at 144, b2 at 160 (ops.GoalMlpWeights.flat; the trainer hands both networks to the kernels as one run of
// its flat buffer).
//
// UNROLL_J is the unroll count of the loop over the hidden units: MLP8_NH (whole) by default; k_dcr_loss passes 1, because
// unrolled all 161 weights would be held in scalar registers across its loop over the pairs.
//
// The gradient scheme: a workgroup of MLP8_ROWS threads stages up to MLP8_ROWS rows {a_j = r w2_j [pre_j > 0], r relu(pre_j),
// f_k, r} in LDS (r: the row's upstream gradient), threads 0..160 each own one of the 161 elements and add the staged rows
// in row order, and the workgroup's sums leave as one row of partial [partition][161]. Which rows are staged is the
// caller's: every lane of a tile (k_goal_bwd) or the live lanes compacted (k_dcr_loss). The barriers are the caller's too.
// No floating-point atomics: two runs are bit-identical.
#pragma once
#include "tarl_common.h"

#define MLP8_NF 8
#define MLP8_NH 16
#define MLP8_NW 161
#define MLP8_B1 128
#define MLP8_W2 144
#define MLP8_B2 160
#define MLP8_ROWS 256       // rows of one staging tile = threads of the workgroup that fills and sums it

__device__ __forceinline__ float mlp8_pre(const float* __restrict__ w, const float f[MLP8_NF], int j) {
  float pre = w[MLP8_B1 + j];
#pragma unroll
  for (int k = 0; k < MLP8_NF; ++k) pre = pre + w[j * MLP8_NF + k] * f[k];
  return pre;
}

template <int UNROLL_J = MLP8_NH>
__device__ __forceinline__ float mlp8_eval(const float* __restrict__ w, const float f[MLP8_NF]) {
  float y = w[MLP8_B2];
#pragma unroll UNROLL_J
  for (int j = 0; j < MLP8_NH; ++j) {
    const float pre = mlp8_pre(w, f, j);
    y = y + w[MLP8_W2 + j] * (pre > 0.0f ? pre : 0.0f);
  }
  return y;
}

// the staging tile: four LDS arrays of the kernel's own, declared by MLP8_STAGE_ARRAYS under the names the helpers and
// MLP8_ACCUMULATE use. (As one struct behind function arguments the same code cost both backward kernels about 2 %:
// profiles/decision_shared_core.txt.)
typedef float Mlp8Hidden[MLP8_ROWS][MLP8_NH + 1];
typedef float Mlp8Feats[MLP8_ROWS][MLP8_NF + 1];
#define MLP8_STAGE_ARRAYS                                                           \
  __shared__ Mlp8Hidden s_a;             /* r * w2[j] * [pre_j > 0] */              \
  __shared__ Mlp8Hidden s_h;             /* r * relu(pre_j) */                      \
  __shared__ Mlp8Feats s_f;                                                         \
  __shared__ float s_r[MLP8_ROWS]

// hidden unit j of the staged row of one evaluation: features f, upstream gradient r
__device__ __forceinline__ void mlp8_row_unit(const float* __restrict__ w, const float f[MLP8_NF], float r, int j, float* a,
                                              float* h) {
  const float pre = mlp8_pre(w, f, j);
  *a = pre > 0.0f ? r * w[MLP8_W2 + j] : 0.0f;
  *h = pre > 0.0f ? r * pre : 0.0f;
}

// Thread t's element (W1[j][k] at t = 8 j + k, b1[j], w2[j], b2; nothing for t > 160): acc += rows 0 .. n - 1 in row order.
// An if / else-if chain without a last else, so that a kernel may hang one more branch for a thread above 160 on it.
#define MLP8_ACCUMULATE(acc, t, n)                                                  \
  if ((t) < MLP8_B1) {                                                              \
    const int j_ = (t) >> 3, k_ = (t) & 7;                                          \
    for (int p = 0; p < (n); ++p) acc = acc + s_a[p][j_] * s_f[p][k_];              \
  } else if ((t) < MLP8_W2) {                                                       \
    for (int p = 0; p < (n); ++p) acc = acc + s_a[p][(t) - MLP8_B1];                \
  } else if ((t) < MLP8_B2) {                                                       \
    for (int p = 0; p < (n); ++p) acc = acc + s_h[p][(t) - MLP8_W2];                \
  } else if ((t) == MLP8_B2) {                                                      \
    for (int p = 0; p < (n); ++p) acc = acc + s_r[p];                               \
  }

__device__ __forceinline__ void mlp8_write_partial(float* __restrict__ partial, int64_t partition, int t, float acc) {
  if (t < MLP8_NW) partial[partition * MLP8_NW + t] = acc;
}
// The partitions are then summed by the caller's own kernel, and the two are NOT one: k_goal_bwd_sum walks the partitions
// in order with one thread per element, the gradient half of k_dcr_sum gives an element to a wave (lane l adds partitions
// l, l + 64, .., then a tree over the lanes). The orders of addition differ, so sharing one would change the other's bits.
