// gt_value.hip — the graph-transformer critic (value_head = "graph_transformer"): ValueNet(MLAgents) of the reference
// (src/agents/transformer_agent.py:257-323) = the node output of a second GraphTransformerNet (model.py:140-178, raw=True:
// mu_mlp(global_pool(x2, batch))) as MLAgents builds it (hidden 16, 4 heads of d_k = 4, gate=True, two GTConv layers), in
// evaluation mode (BatchNorm on its running statistics, dropout = identity). Edge e = (u -> v), PyG source_to_target.
//
//   x0 = node_emb(obs16) + pe_emb(pe)                                                                  (model.py:160-162)
//   per layer (gt_conv.py:144-232):  Q, K, V = WQ x, WK x, WV x;  G = n_gate x + b
//     score_e,h = sum_{d in h} Q_v K_u / 2;  alpha = softmax of the scores over the in-edges of v (PyG 2.5: max subtracted,
//     + 1e-16 in the denominator);  x' = BN2(y + FFN(y)),  y = BN1(WO(sum_u alpha V_u sigmoid(G_u)) + x)
//   value = mu_mlp(sum over the N nodes of x2)         mu_mlp = Linear(16,16) -> ReLU -> Linear(16,1)   (model.py:174-176)
//
// The node path never reads the edge features (the score is (Q_i K_j).sum / sqrt(d_k), gt_conv.py:222; eij feeds the edge
// output alone), so edge_emb, WE, WOe, ffn_e, norm1e / norm2e, e_gate, edge_linear and log_var_mlp are not read here.
// fp32 on the vector ALU, one thread per (sample, node); weights are wave-uniform (scalar loads from a pointer table).
//
// Passes (forward): hoist (P = pe_emb(pe) per node) -> node pass A (x0; Q, K, V sigmoid(G) of layer 0) -> node pass B<0>
//   (softmax over the CSC in-edges, WO, BN, FFN, BN -> x1; Q, K, V sigmoid(G) of layer 1) -> node pass B<1> (-> x2) ->
//   pool (one workgroup per sample: the node sum in a fixed order, then mu_mlp -> value [M]).
// Backward (forward recomputed inside, activations kept in per-item records): pool<bwd> (mu_mlp backwards -> g of the
//   pooled vector = g of every node's x2) -> node pass D (layer 1 backwards to its attention, softmax backward over the
//   in-edges) -> node pass E<1> (Q / K / V / G of layer 1 by walks of the in- and out-edges in CSC / CSR order -> g x1,
//   layer 0 backwards to its attention, softmax backward) -> node pass E<0> (-> g x0). Weight gradients: sums over items
//   (sample, node) or (sample) of products of two recorded vectors — stage 1 sums fixed chunks of items per output in item
//   order, stage 2 adds the chunk partials in chunk order into the caller's buffers. No atomics: bit-reproducible.
//
// The node side (the helpers, embedding, projections, the attention + layer body forwards and backwards, the Q / K / V / G
// gradient walk, the weight-gradient reduction) is gt_core.h, shared with the policy head (gt_policy.hip), whose last layer
// stops at Q and K. This file keeps the parameter table, the pool and the entry points.
#include "gt_core.h"

// ---- the pointer table: trainable parameters in kernel order (GV_NP), then the BatchNorm running statistics --------------
// per node layer gt_core.h's block of 15 parameters from node_par(L) and 4 running statistics from node_run(L)
enum {
  V_NODE_EMB = 0, V_PE_EMB,
  V_MU0_W = 2 + 2 * L_NP, V_MU0_B, V_MU2_W, V_MU2_B,
  GV_NP_,
  GV_NW_ = GV_NP_ + 2 * L_NR
};
static_assert(GV_NP_ == TARL_GTV_NUM_PARAMS, "parameter table out of step with the header");
static_assert(GV_NW_ == TARL_GTV_NUM_TENSORS, "tensor table out of step with the header");
__host__ __device__ constexpr int node_par(int L) { return 2 + L * L_NP; }
__host__ __device__ constexpr int node_run(int L) { return GV_NP_ + L * L_NR; }

struct GvW {
  const float* p[GV_NW_];
};

// ---- record layouts --------------------------------------------------------------------------------------------------------
// node record (sample, node), gt_core.h's per-layer scheme. The forward keeps the first NF_SLOTS: per layer {Q, K,
// V sigmoid(G), input x} and x2; the backward also the per-layer activations and gradients, then obs16, pe and g x0.
enum { NX2 = 2 * F_LAYER, NF_SLOTS };
enum { NOBS = NF_SLOTS + 2 * B_LAYER, NPE, NGX0, NB_SLOTS };
static_assert(NF_SLOTS == 9 && NB_SLOTS == 48, "the scratch sizes are part of the ABI");
template <int L>
using Ly = GtLayer<node_par(L), node_run(L), L * F_LAYER, NF_SLOTS + L * B_LAYER>;
// sample record (backward): pooled x2, mu_mlp hidden pre- / post-ReLU, their gradients, g value (in [0]), g pooled
enum { SPOOL = 0, SH, SR, SGH, SGOUT, SGPOOL, S_SLOTS };

// ---- hoist: P = pe_emb(pe) per node (state-independent) ----------------------------------------------------------------------
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_hoist(GvW W, const float* __restrict__ pe, int64_t N,
                                                        float* __restrict__ hoist) {
  const int64_t n = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (n < N) pe_hoist(W.p[V_PE_EMB], pe + n * 16, hoist + n * 16);
}

// ---- node pass A: x0 and layer 0's projections ---------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_nodeA(GvW W, const float* __restrict__ obs, const float* __restrict__ pe,
                                                        const float* __restrict__ P, int64_t MN, int64_t N,
                                                        float* __restrict__ nrec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t n = gid % N;
  float o[16], x0[16], t[16], g[16];
  embed(W.p[V_NODE_EMB], obs + gid * 16, P + n * 16, o, x0);
  float* r = nrec + gid * NS;
  node_proj<Ly<0>, BWD, false>(W, x0, r, t, g);
  if (BWD) {
    float p[16];
    st16(r + NOBS * 16, o);
    ld16(pe + n * 16, p);
    st16(r + NPE * 16, p);
  }
}

// ---- node pass B<L>: segment softmax + aggregation, WO, BN1, FFN, BN2 -> x_{L+1} (L = 0: and layer 1's projections) -----------
template <int L, bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_nodeB(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        int64_t MN, int64_t N, int64_t E, float* __restrict__ nrec,
                                                        float* __restrict__ alpha) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, v = gid - m * N;
  float* r = nrec + gid * NS;
  float xo[16], t[16], g[16];
  layer_fwd<Ly<L>, NS, BWD>(W, in_src, in_eid, in_ptr[v], in_ptr[v + 1], r, nrec + m * N * NS,
                            BWD ? alpha + m * E * 4 : nullptr, xo);
  if constexpr (L == 0) {
    node_proj<Ly<1>, BWD, false>(W, xo, r, t, g);
  } else {
    st16(r + NX2 * 16, xo);
  }
}

// ---- pool: per sample, the sum of x2 over the nodes in a fixed order, then mu_mlp (backward: and its gradients) ----------------
// thread t sums nodes t, t + 256, ... in order; the 256 partials are added by a fixed binary tree
template <bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_pool(GvW W, const float* __restrict__ nrec, int64_t N,
                                                       float* __restrict__ value, const float* __restrict__ grad_value,
                                                       float* __restrict__ srec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  __shared__ float red[GT_BLOCK][17];
  const int64_t m = blockIdx.x;
  const int t = threadIdx.x;
  float acc[16], x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  for (int64_t n = t; n < N; n += GT_BLOCK) {
    ld16(nrec + (m * N + n) * NS + NX2 * 16, x);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += x[i];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[t][i] = acc[i];
  __syncthreads();
  for (int s = GT_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int i = 0; i < 16; ++i) red[t][i] += red[t + s][i];
    }
    __syncthreads();
  }
  if (t != 0) return;
  float pool[16], h[16], r[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) pool[i] = red[0][i];
  lin16(W.p[V_MU0_W], W.p[V_MU0_B], pool, h);
  float a = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    r[j] = fmaxf(h[j], 0.0f);
    a += W.p[V_MU2_W][j] * r[j];
  }
  if (!BWD) {
    value[m] = a + W.p[V_MU2_B][0];
    return;
  }
  const float g = grad_value[m];
  float gh[16], gp[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) gh[j] = h[j] > 0.0f ? g * W.p[V_MU2_W][j] : 0.0f;
  lin16t(W.p[V_MU0_W], gh, gp, false);
  float* sr = srec + m * (S_SLOTS * 16);
  st16(sr + SPOOL * 16, pool);
  st16(sr + SH * 16, h);
  st16(sr + SR * 16, r);
  st16(sr + SGH * 16, gh);
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = 0.0f;
  x[0] = g;
  st16(sr + SGOUT * 16, x);
  st16(sr + SGPOOL * 16, gp);
}

// ---- node pass D: layer 1 backwards from g x2 (= g of the pooled vector) to its attention scores -------------------------------
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_nodeD(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        int64_t MN, int64_t N, int64_t E, float* __restrict__ nrec,
                                                        const float* __restrict__ srec, const float* __restrict__ alpha1,
                                                        float* __restrict__ gscore1) {
  constexpr int NS = NB_SLOTS * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  float gx[16], gt[16], gagg[16];
  ld16(srec + m * (S_SLOTS * 16) + SGPOOL * 16, gx);
  body_bwd<Ly<1>>(W, r, gx, gt, gagg);
  softmax_bwd<Ly<1>, NS>(in_src, in_eid, in_ptr[n], in_ptr[n + 1], nrec + m * N * NS, gagg, alpha1 + m * E * 4,
                         gscore1 + m * E * 4);
}

// ---- node pass E<L>: gradients of layer L's Q / K / V / G (in- and out-edge walks) -> g of its input x; L = 1: then layer 0
// backwards to its attention scores (g x1 is layer 0's output gradient); L = 0: g x0 -------------------------------------------
template <int L>
__global__ __launch_bounds__(GT_BLOCK) void k_gtv_nodeE(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        const int32_t* __restrict__ out_ptr,
                                                        const int32_t* __restrict__ out_dst,
                                                        const int32_t* __restrict__ out_eid, int64_t MN, int64_t N, int64_t E,
                                                        float* __restrict__ nrec, const float* __restrict__ alphaL,
                                                        const float* __restrict__ gscoreL, const float* __restrict__ alpha0,
                                                        float* __restrict__ gscore0) {
  constexpr int NS = NB_SLOTS * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  const float* base = nrec + m * N * NS;
  float gx[16];
  qkvg_bwd<Ly<L>, NS, 0>(W, in_src, in_eid, in_ptr[n], in_ptr[n + 1], out_dst, out_eid, out_ptr[n], out_ptr[n + 1], r, base,
                         alphaL + m * E * 4, gscoreL + m * E * 4, nullptr, gx);
  if constexpr (L == 0) {
    st16(r + NGX0 * 16, gx);
  } else {
    float gt[16], gagg[16];
    body_bwd<Ly<0>>(W, r, gx, gt, gagg);
    softmax_bwd<Ly<0>, NS>(in_src, in_eid, in_ptr[n], in_ptr[n + 1], base, gagg, alpha0 + m * E * 4, gscore0 + m * E * 4);
  }
}

// ---- the weight gradients' terms (gt_core.h); second stream: the sample records -------------------------------------------------------
static GtTermList<GV_NP_> make_terms() {
  GtTermList<GV_NP_> T;
  T.add(V_NODE_EMB, 0, NGX0, NOBS, T_OUTER, 16, 16);
  T.add(V_PE_EMB, 0, NGX0, NPE, T_OUTER, 16, 16);
  T.add_node_layer<Ly<0>>();
  T.add_node_layer<Ly<1>>();
  T.add(V_MU0_W, 1, SGH, SPOOL, T_OUTER, 16, 16);
  T.add(V_MU0_B, 1, SGH, 0, T_BIAS, 16, 1);
  T.add(V_MU2_W, 1, SGOUT, SR, T_OUTER, 1, 16);
  T.add(V_MU2_B, 1, SGOUT, 0, T_BIAS, 1, 1);
  return T;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
extern "C" int64_t tarl_value_gt_fwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  return plan->N * 16 + M * plan->N * NF_SLOTS * 16;
}

extern "C" int64_t tarl_value_gt_bwd_max_samples(const tarl_plan* plan) {
  if (!plan) return -1;
  return (int64_t)GT_MAX_CHUNKS * GT_CHUNK / (plan->N > 0 ? plan->N : 1);
}

extern "C" int64_t tarl_value_gt_bwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  const int64_t chunks = ceil_div(M * plan->N, GT_CHUNK);     // N >= 1 in every call: never fewer (sample, node) items than samples
  return plan->N * 16 + M * plan->N * NB_SLOTS * 16 + M * plan->E * 16 + M * S_SLOTS * 16 + chunks * make_terms().nout;
}

static int gv_check(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe, const float* const* w,
                    float* scratch, GvW* W) {
  TARL_REQUIRE(plan && obs16 && pe && w && scratch, "null argument");
  TARL_REQUIRE(M >= 1, "bad sample count");
  TARL_REQUIRE(plan->N >= 1, "empty graph");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0 && ((uintptr_t)pe) % 16 == 0 && ((uintptr_t)scratch) % 16 == 0,
               "obs16 / pe / scratch must be 16-byte aligned");
  TARL_REQUIRE(gt_table(w, W->p, GV_NW_), "parameter pointer is null");
  return TARL_OK;
}

extern "C" int tarl_value_gt_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe,
                                 const float* const* w, float* scratch, int64_t scratch_floats, float* value,
                                 tarl_stream stream) {
  GvW W;
  int rc = gv_check(plan, obs16, M, pe, w, scratch, &W);
  if (rc) return rc;
  TARL_REQUIRE(value, "null value");
  TARL_REQUIRE(scratch_floats >= tarl_value_gt_fwd_scratch_floats(plan, M),
               "scratch smaller than tarl_value_gt_fwd_scratch_floats");
  TARL_REQUIRE(M <= 0x7fffffff, "too many samples for one grid dimension");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = plan->N, E = plan->E, MN = M * N;
  float* hoist = scratch;
  float* nrec = scratch + N * 16;
  hipLaunchKernelGGL(k_gtv_hoist, dim3((unsigned)ceil_div(N, GT_BLOCK)), dim3(GT_BLOCK), 0, s, W, pe, N, hoist);
  TARL_LAUNCH_CHECK();
  const unsigned gn = (unsigned)ceil_div(MN, GT_BLOCK);
  hipLaunchKernelGGL(k_gtv_nodeA<false>, dim3(gn), dim3(GT_BLOCK), 0, s, W, obs16, pe, (const float*)hoist, MN, N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<0, false>), dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<1, false>), dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_pool<false>, dim3((unsigned)M), dim3(GT_BLOCK), 0, s, W, (const float*)nrec, N, value,
                     (const float*)nullptr, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_value_gt_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe,
                                 const float* const* w, const float* grad_value, float* scratch, int64_t scratch_floats,
                                 float* const* grads, tarl_stream stream) {
  GvW W;
  int rc = gv_check(plan, obs16, M, pe, w, scratch, &W);
  if (rc) return rc;
  TARL_REQUIRE(grad_value && grads, "null grad_value / grads");
  TARL_REQUIRE(scratch_floats >= tarl_value_gt_bwd_scratch_floats(plan, M),
               "scratch smaller than tarl_value_gt_bwd_scratch_floats");
  TARL_REQUIRE(M <= tarl_value_gt_bwd_max_samples(plan), "more samples than tarl_value_gt_bwd_max_samples");
  GtGrads<GV_NP_> G;
  TARL_REQUIRE(gt_table(grads, G.p, GV_NP_), "gradient pointer is null");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = plan->N, E = plan->E, MN = M * N, ME = M * E;
  float* hoist = scratch;
  float* nrec = hoist + N * 16;
  float* alpha0 = nrec + MN * NB_SLOTS * 16;
  float* alpha1 = alpha0 + ME * 4;
  float* gscore0 = alpha1 + ME * 4;
  float* gscore1 = gscore0 + ME * 4;
  float* srec = gscore1 + ME * 4;
  float* partial = srec + M * S_SLOTS * 16;
  const unsigned gn = (unsigned)ceil_div(MN, GT_BLOCK);
  hipLaunchKernelGGL(k_gtv_hoist, dim3((unsigned)ceil_div(N, GT_BLOCK)), dim3(GT_BLOCK), 0, s, W, pe, N, hoist);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeA<true>, dim3(gn), dim3(GT_BLOCK), 0, s, W, obs16, pe, (const float*)hoist, MN, N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<0, true>), dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, alpha0);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<1, true>), dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, alpha1);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_pool<true>, dim3((unsigned)M), dim3(GT_BLOCK), 0, s, W, (const float*)nrec, N, (float*)nullptr,
                     grad_value, srec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeD, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, MN, N, E,
                     nrec, (const float*)srec, (const float*)alpha1, gscore1);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeE<1>, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     plan->out_ptr, plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)alpha1,
                     (const float*)gscore1, (const float*)alpha0, gscore0);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeE<0>, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     plan->out_ptr, plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)alpha0,
                     (const float*)gscore0, (const float*)nullptr, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  // MN >= M items: the sample terms need fewer rows, and the limit was checked above
  return gt_wgrad_launch(__func__, "more samples than tarl_value_gt_bwd_max_samples", make_terms(), G, nrec, NB_SLOTS * 16, MN,
                         srec, S_SLOTS * 16, M, partial, s);
}
