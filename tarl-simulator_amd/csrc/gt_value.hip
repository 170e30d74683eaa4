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
#include <math.h>

#include "tarl_common.h"

#define GV_BLOCK 256
#define GV_CHUNK 1024      // items per stage-1 partial sum of the weight gradients

// ---- the pointer table: trainable parameters in kernel order (GV_NP), then the BatchNorm running statistics --------------
// per node layer, 15 parameters from node_par(L): WQ, WK, WV, n_gate.{w,b}, WO.{w,b}, norm1.{w,b}, ffn.mlp.0.{w,b},
// ffn.mlp.3.{w,b}, norm2.{w,b}; 4 running statistics from node_run(L): norm1.{mean,var}, norm2.{mean,var}
enum { LWQ = 0, LWK, LWV, LNG_W, LNG_B, LWO_W, LWO_B, LN1_W, LN1_B, LF0_W, LF0_B, LF3_W, LF3_B, LN2_W, LN2_B, L_NP };
enum { LN1_M = 0, LN1_V, LN2_M, LN2_V, L_NR };
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
// node record (sample, node): 16-float slots. The forward keeps the first NF_SLOTS: per layer {Q, K, V sigmoid(G), input x}
// and x2; the backward also the per-layer activations and gradients, then obs16, pe and g x0.
enum { FQ = 0, FK, FVG, FX, F_LAYER };
enum { NX2 = 2 * F_LAYER, NF_SLOTS };
enum { BV = 0, BSG, BAGG, BTH, BY, BH, BR, BSH, BGQ, BGK, BGV, BGG, BGX, BGS, BGH, BGY, BGT, BGAGG, B_LAYER };
enum { NOBS = NF_SLOTS + 2 * B_LAYER, NPE, NGX0, NB_SLOTS };
__host__ __device__ constexpr int fs(int L, int k) { return L * F_LAYER + k; }
__host__ __device__ constexpr int bs(int L, int k) { return NF_SLOTS + L * B_LAYER + k; }
// sample record (backward): pooled x2, mu_mlp hidden pre- / post-ReLU, their gradients, g value (in [0]), g pooled
enum { SPOOL = 0, SH, SR, SGH, SGOUT, SGPOOL, S_SLOTS };

__device__ __forceinline__ void ld16(const float* __restrict__ p, float* v) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = q[i];
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
}
__device__ __forceinline__ void st16(float* __restrict__ p, const float* v) {
  float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}
// y = W x (+ b), W [16][16] row-major (nn.Linear), ascending input index
__device__ __forceinline__ void lin16(const float* __restrict__ W, const float* __restrict__ b, const float* x, float* y) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) a += W[i * 16 + j] * x[j];
    y[i] = b ? a + b[i] : a;
  }
}
// y (+)= W^T g
__device__ __forceinline__ void lin16t(const float* __restrict__ W, const float* g, float* y, bool acc) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += W[i * 16 + j] * g[i];
    y[j] = acc ? y[j] + a : a;
  }
}
// evaluation-mode BatchNorm1d: out = (x - mean) / sqrt(var + 1e-5) * w + b; xh = the normalised input
__device__ __forceinline__ void bn16(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ rm,
                                     const float* __restrict__ rv, const float* x, float* xh, float* out) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    xh[i] = (x[i] - rm[i]) / sqrtf(rv[i] + 1e-5f);
    out[i] = xh[i] * w[i] + b[i];
  }
}
// gradient through it: g_in = g_out * w / sqrt(var + 1e-5)
__device__ __forceinline__ void bn16_bwd(const float* __restrict__ w, const float* __restrict__ rv, const float* g, float* gi) {
#pragma unroll
  for (int i = 0; i < 16; ++i) gi[i] = g[i] * w[i] / sqrtf(rv[i] + 1e-5f);
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- hoist: P = pe_emb(pe) per node (state-independent) ----------------------------------------------------------------------
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_hoist(GvW W, const float* __restrict__ pe, int64_t N,
                                                        float* __restrict__ hoist) {
  const int64_t n = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  if (n >= N) return;
  float p[16], q[16];
  ld16(pe + n * 16, p);
  lin16(W.p[V_PE_EMB], nullptr, p, q);
  st16(hoist + n * 16, q);
}

// layer L's projections of its input x into the record: Q, K, V sigmoid(G), x (and V, sigmoid(G) for the backward)
template <int L, bool BWD>
__device__ __forceinline__ void node_proj(const GvW& W, const float* x, float* r) {
  constexpr int P = node_par(L);
  float t[16], g[16];
  lin16(W.p[P + LWQ], nullptr, x, t);
  st16(r + fs(L, FQ) * 16, t);
  lin16(W.p[P + LWK], nullptr, x, t);
  st16(r + fs(L, FK) * 16, t);
  st16(r + fs(L, FX) * 16, x);
  lin16(W.p[P + LWV], nullptr, x, t);
  lin16(W.p[P + LNG_W], W.p[P + LNG_B], x, g);
#pragma unroll
  for (int i = 0; i < 16; ++i) g[i] = sigmoidf_(g[i]);
  if (BWD) {
    st16(r + bs(L, BV) * 16, t);
    st16(r + bs(L, BSG) * 16, g);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = t[i] * g[i];
  st16(r + fs(L, FVG) * 16, t);
}

// ---- node pass A: x0 and layer 0's projections ---------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_nodeA(GvW W, const float* __restrict__ obs, const float* __restrict__ pe,
                                                        const float* __restrict__ P, int64_t MN, int64_t N,
                                                        float* __restrict__ nrec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t n = gid % N;
  float o[16], x0[16], p[16];
  ld16(obs + gid * 16, o);
  ld16(P + n * 16, p);
  lin16(W.p[V_NODE_EMB], nullptr, o, x0);
#pragma unroll
  for (int i = 0; i < 16; ++i) x0[i] = x0[i] + p[i];
  float* r = nrec + gid * NS;
  node_proj<0, BWD>(W, x0, r);
  if (BWD) {
    st16(r + NOBS * 16, o);
    ld16(pe + n * 16, p);
    st16(r + NPE * 16, p);
  }
}

// attention score of in-edge (u -> v) for head h: sum_{d in h} Q_v[d] K_u[d] / 2
__device__ __forceinline__ void scores4(const float* q, const float* __restrict__ ku, float* s) {
  float k[16];
  ld16(ku, k);
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    float a = 0.0f;
#pragma unroll
    for (int d = 0; d < 4; ++d) a += q[4 * h + d] * k[4 * h + d];
    s[h] = a / 2.0f;
  }
}

// ---- node pass B<L>: segment softmax + aggregation, WO, BN1, FFN, BN2 -> x_{L+1} (L = 0: and layer 1's projections) -----------
template <int L, bool BWD>
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_nodeB(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        int64_t MN, int64_t N, int64_t E, float* __restrict__ nrec,
                                                        float* __restrict__ alpha) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16, P = node_par(L), R = node_run(L);
  const int64_t gid = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, v = gid - m * N;
  float* r = nrec + gid * NS;
  const float* base = nrec + m * N * NS;
  float q[16], s[4], mx[4], den[4], agg[16];
  ld16(r + fs(L, FQ) * 16, q);
  const int k0 = in_ptr[v], k1 = in_ptr[v + 1];
#pragma unroll
  for (int h = 0; h < 4; ++h) { mx[h] = -INFINITY; den[h] = 0.0f; }
  for (int k = k0; k < k1; ++k) {
    scores4(q, base + (int64_t)in_src[k] * NS + fs(L, FK) * 16, s);
#pragma unroll
    for (int h = 0; h < 4; ++h) mx[h] = fmaxf(mx[h], s[h]);
  }
  for (int k = k0; k < k1; ++k) {
    scores4(q, base + (int64_t)in_src[k] * NS + fs(L, FK) * 16, s);
#pragma unroll
    for (int h = 0; h < 4; ++h) den[h] += expf(s[h] - mx[h]);
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) den[h] = den[h] + 1e-16f;
#pragma unroll
  for (int i = 0; i < 16; ++i) agg[i] = 0.0f;
  for (int k = k0; k < k1; ++k) {
    const int64_t u = in_src[k];
    scores4(q, base + u * NS + fs(L, FK) * 16, s);
    float vg[16];
    ld16(base + u * NS + fs(L, FVG) * 16, vg);
    float a[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) a[h] = expf(s[h] - mx[h]) / den[h];
    if (BWD) *reinterpret_cast<float4*>(alpha + (m * E + in_eid[k]) * 4) = make_float4(a[0], a[1], a[2], a[3]);
#pragma unroll
    for (int i = 0; i < 16; ++i) agg[i] += a[i >> 2] * vg[i];
  }
  float x[16], t[16], th[16], y[16], hh[16], rr[16], f[16], sh[16], xo[16];
  ld16(r + fs(L, FX) * 16, x);
  lin16(W.p[P + LWO_W], W.p[P + LWO_B], agg, t);       // WO(out) + x_ (gt_conv.py:183)
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = t[i] + x[i];
  bn16(W.p[P + LN1_W], W.p[P + LN1_B], W.p[R + LN1_M], W.p[R + LN1_V], t, th, y);
  lin16(W.p[P + LF0_W], W.p[P + LF0_B], y, hh);
#pragma unroll
  for (int i = 0; i < 16; ++i) rr[i] = fmaxf(hh[i], 0.0f);
  lin16(W.p[P + LF3_W], W.p[P + LF3_B], rr, f);
#pragma unroll
  for (int i = 0; i < 16; ++i) f[i] = y[i] + f[i];    // norm2(ffn_in + out) (gt_conv.py:192)
  bn16(W.p[P + LN2_W], W.p[P + LN2_B], W.p[R + LN2_M], W.p[R + LN2_V], f, sh, xo);
  if constexpr (L == 0) {
    node_proj<1, BWD>(W, xo, r);
  } else {
    st16(r + NX2 * 16, xo);
  }
  if (BWD) {
    st16(r + bs(L, BAGG) * 16, agg);
    st16(r + bs(L, BTH) * 16, th);
    st16(r + bs(L, BY) * 16, y);
    st16(r + bs(L, BH) * 16, hh);
    st16(r + bs(L, BR) * 16, rr);
    st16(r + bs(L, BSH) * 16, sh);
  }
}

// ---- pool: per sample, the sum of x2 over the nodes in a fixed order, then mu_mlp (backward: and its gradients) ----------------
// thread t sums nodes t, t + 256, ... in order; the 256 partials are added by a fixed binary tree
template <bool BWD>
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_pool(GvW W, const float* __restrict__ nrec, int64_t N,
                                                       float* __restrict__ value, const float* __restrict__ grad_value,
                                                       float* __restrict__ srec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  __shared__ float red[GV_BLOCK][17];
  const int64_t m = blockIdx.x;
  const int t = threadIdx.x;
  float acc[16], x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  for (int64_t n = t; n < N; n += GV_BLOCK) {
    ld16(nrec + (m * N + n) * NS + NX2 * 16, x);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += x[i];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[t][i] = acc[i];
  __syncthreads();
  for (int s = GV_BLOCK / 2; s > 0; s >>= 1) {
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

// layer L backwards from the gradient of its output gx to the attention: the record's gradient slots, gt (the residual's
// gradient) and gagg
template <int L>
__device__ __forceinline__ void body_bwd(const GvW& W, float* r, const float* gx, float* gt, float* gagg) {
  constexpr int P = node_par(L), R = node_run(L);
  float gs[16], gh[16], gy[16], a[16];
  bn16_bwd(W.p[P + LN2_W], W.p[R + LN2_V], gx, gs);
  lin16t(W.p[P + LF3_W], gs, gh, false);
  ld16(r + bs(L, BH) * 16, a);
#pragma unroll
  for (int i = 0; i < 16; ++i) gh[i] = a[i] > 0.0f ? gh[i] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) gy[i] = gs[i];
  lin16t(W.p[P + LF0_W], gh, gy, true);
  bn16_bwd(W.p[P + LN1_W], W.p[R + LN1_V], gy, gt);
  lin16t(W.p[P + LWO_W], gt, gagg, false);
  st16(r + bs(L, BGX) * 16, gx);
  st16(r + bs(L, BGS) * 16, gs);
  st16(r + bs(L, BGH) * 16, gh);
  st16(r + bs(L, BGY) * 16, gy);
  st16(r + bs(L, BGT) * 16, gt);
  st16(r + bs(L, BGAGG) * 16, gagg);
}

// softmax backward over the in-edges of node n (CSC order) for layer L: g_score = alpha (g_alpha - sum_k alpha_k g_alpha_k),
// g_alpha = <g_agg, V_u sigmoid(G_u)>_head
template <int L>
__device__ __forceinline__ void softmax_bwd(const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid, int k0,
                                            int k1, const float* __restrict__ base, const float* gagg,
                                            const float* __restrict__ alpha, float* __restrict__ gscore) {
  constexpr int NS = NB_SLOTS * 16;
  float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[16];
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = k0; k < k1; ++k) {
      const int64_t eid = in_eid[k];
      ld16(base + (int64_t)in_src[k] * NS + fs(L, FVG) * 16, b);
      const float4 al = *reinterpret_cast<const float4*>(alpha + eid * 4);
      const float av[4] = {al.x, al.y, al.z, al.w};
      float ga[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < 4; ++d) s += gagg[4 * h + d] * b[4 * h + d];
        ga[h] = s;
      }
      if (pass == 0) {
#pragma unroll
        for (int h = 0; h < 4; ++h) dot[h] += av[h] * ga[h];
      } else {
        *reinterpret_cast<float4*>(gscore + eid * 4) =
            make_float4(av[0] * (ga[0] - dot[0]), av[1] * (ga[1] - dot[1]), av[2] * (ga[2] - dot[2]), av[3] * (ga[3] - dot[3]));
      }
    }
  }
}

// ---- node pass D: layer 1 backwards from g x2 (= g of the pooled vector) to its attention scores -------------------------------
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_nodeD(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        int64_t MN, int64_t N, int64_t E, float* __restrict__ nrec,
                                                        const float* __restrict__ srec, const float* __restrict__ alpha1,
                                                        float* __restrict__ gscore1) {
  constexpr int NS = NB_SLOTS * 16;
  const int64_t gid = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  float gx[16], gt[16], gagg[16];
  ld16(srec + m * (S_SLOTS * 16) + SGPOOL * 16, gx);
  body_bwd<1>(W, r, gx, gt, gagg);
  softmax_bwd<1>(in_src, in_eid, in_ptr[n], in_ptr[n + 1], nrec + m * N * NS, gagg, alpha1 + m * E * 4, gscore1 + m * E * 4);
}

// ---- node pass E<L>: gradients of layer L's Q / K / V / G (in- and out-edge walks) -> g of its input x; L = 1: then layer 0
// backwards to its attention scores (g x1 is layer 0's output gradient); L = 0: g x0 -------------------------------------------
template <int L>
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_nodeE(GvW W, const int32_t* __restrict__ in_ptr,
                                                        const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                        const int32_t* __restrict__ out_ptr,
                                                        const int32_t* __restrict__ out_dst,
                                                        const int32_t* __restrict__ out_eid, int64_t MN, int64_t N, int64_t E,
                                                        float* __restrict__ nrec, const float* __restrict__ alphaL,
                                                        const float* __restrict__ gscoreL, const float* __restrict__ alpha0,
                                                        float* __restrict__ gscore0) {
  constexpr int NS = NB_SLOTS * 16, P = node_par(L);
  const int64_t gid = (int64_t)blockIdx.x * GV_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  const float* base = nrec + m * N * NS;
  const float* al_m = alphaL + m * E * 4;
  const float* gs_m = gscoreL + m * E * 4;
  float gQ[16], gK[16], gVG[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { gQ[i] = 0.0f; gK[i] = 0.0f; gVG[i] = 0.0f; }
  for (int k = in_ptr[n]; k < in_ptr[n + 1]; ++k) {        // n is the target: d score / d Q_v = K_u / 2
    const float4 gsc = *reinterpret_cast<const float4*>(gs_m + (int64_t)in_eid[k] * 4);
    const float gv[4] = {gsc.x, gsc.y, gsc.z, gsc.w};
    ld16(base + (int64_t)in_src[k] * NS + fs(L, FK) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gQ[i] += gv[i >> 2] * b[i] / 2.0f;
  }
  for (int k = out_ptr[n]; k < out_ptr[n + 1]; ++k) {      // n is the source: d score / d K_u = Q_v / 2; messages V_u sigma(G_u)
    const int64_t eid = out_eid[k], v = out_dst[k];
    const float4 gsc = *reinterpret_cast<const float4*>(gs_m + eid * 4);
    const float gv[4] = {gsc.x, gsc.y, gsc.z, gsc.w};
    ld16(base + v * NS + fs(L, FQ) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gK[i] += gv[i >> 2] * b[i] / 2.0f;
    const float4 al = *reinterpret_cast<const float4*>(al_m + eid * 4);
    const float av[4] = {al.x, al.y, al.z, al.w};
    ld16(base + v * NS + bs(L, BGAGG) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gVG[i] += av[i >> 2] * b[i];
  }
  float V[16], sg[16], gV[16], gG[16], gx[16];
  ld16(r + bs(L, BV) * 16, V);
  ld16(r + bs(L, BSG) * 16, sg);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    gV[i] = gVG[i] * sg[i];
    gG[i] = gVG[i] * V[i] * (sg[i] * (1.0f - sg[i]));
  }
  ld16(r + bs(L, BGT) * 16, gx);                 // the residual of WO(out) + x_
  lin16t(W.p[P + LWQ], gQ, gx, true);
  lin16t(W.p[P + LWK], gK, gx, true);
  lin16t(W.p[P + LWV], gV, gx, true);
  lin16t(W.p[P + LNG_W], gG, gx, true);
  st16(r + bs(L, BGQ) * 16, gQ);
  st16(r + bs(L, BGK) * 16, gK);
  st16(r + bs(L, BGV) * 16, gV);
  st16(r + bs(L, BGG) * 16, gG);
  if constexpr (L == 0) {
    st16(r + NGX0 * 16, gx);
  } else {
    float gt[16], gagg[16];
    body_bwd<0>(W, r, gx, gt, gagg);
    softmax_bwd<0>(in_src, in_eid, in_ptr[n], in_ptr[n + 1], base, gagg, alpha0 + m * E * 4, gscore0 + m * E * 4);
  }
}

// ---- weight gradients: sum over items of g[i] * a[j] (outer), g[i] (bias) or g[i] * a[i] (BatchNorm weight) ------------------------
enum { T_OUTER = 0, T_BIAS, T_DIAG };
struct GvTerm {
  int16_t param, sample, g, a, kind, rows, cols;
  int32_t off;    // offset of the parameter's outputs in the partial-sum rows
};
struct GvTerms {
  GvTerm t[GV_NP_];
};
struct GvG {
  float* p[GV_NP_];
};

static GvTerms make_terms(int* nout) {
  GvTerms T{};
  int k = 0, off = 0;
  auto add = [&](int param, int sample, int g, int a, int kind, int rows, int cols) {
    T.t[k] = GvTerm{(int16_t)param, (int16_t)sample, (int16_t)g, (int16_t)a, (int16_t)kind, (int16_t)rows, (int16_t)cols, off};
    off += rows * cols;
    ++k;
  };
  add(V_NODE_EMB, 0, NGX0, NOBS, T_OUTER, 16, 16);
  add(V_PE_EMB, 0, NGX0, NPE, T_OUTER, 16, 16);
  for (int L = 0; L < 2; ++L) {
    const int P = node_par(L);
    add(P + LWQ, 0, bs(L, BGQ), fs(L, FX), T_OUTER, 16, 16);
    add(P + LWK, 0, bs(L, BGK), fs(L, FX), T_OUTER, 16, 16);
    add(P + LWV, 0, bs(L, BGV), fs(L, FX), T_OUTER, 16, 16);
    add(P + LNG_W, 0, bs(L, BGG), fs(L, FX), T_OUTER, 16, 16);
    add(P + LNG_B, 0, bs(L, BGG), 0, T_BIAS, 16, 1);
    add(P + LWO_W, 0, bs(L, BGT), bs(L, BAGG), T_OUTER, 16, 16);
    add(P + LWO_B, 0, bs(L, BGT), 0, T_BIAS, 16, 1);
    add(P + LN1_W, 0, bs(L, BGY), bs(L, BTH), T_DIAG, 16, 1);
    add(P + LN1_B, 0, bs(L, BGY), 0, T_BIAS, 16, 1);
    add(P + LF0_W, 0, bs(L, BGH), bs(L, BY), T_OUTER, 16, 16);
    add(P + LF0_B, 0, bs(L, BGH), 0, T_BIAS, 16, 1);
    add(P + LF3_W, 0, bs(L, BGS), bs(L, BR), T_OUTER, 16, 16);
    add(P + LF3_B, 0, bs(L, BGS), 0, T_BIAS, 16, 1);
    add(P + LN2_W, 0, bs(L, BGX), bs(L, BSH), T_DIAG, 16, 1);
    add(P + LN2_B, 0, bs(L, BGX), 0, T_BIAS, 16, 1);
  }
  add(V_MU0_W, 1, SGH, SPOOL, T_OUTER, 16, 16);
  add(V_MU0_B, 1, SGH, 0, T_BIAS, 16, 1);
  add(V_MU2_W, 1, SGOUT, SR, T_OUTER, 1, 16);
  add(V_MU2_B, 1, SGOUT, 0, T_BIAS, 1, 1);
  *nout = off;
  return T;
}

// stage 1: block (term, chunk), one thread per output, items of the chunk in ascending order
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_wgrad1(GvTerms T, const float* __restrict__ nrec,
                                                         const float* __restrict__ srec, int64_t n_node, int64_t n_sample,
                                                         int nout, float* __restrict__ partial) {
  const GvTerm& t = T.t[blockIdx.x];
  const int64_t items = t.sample ? n_sample : n_node;
  const int64_t i0 = (int64_t)blockIdx.y * GV_CHUNK;
  const int o = threadIdx.x;
  if (i0 >= items || o >= t.rows * t.cols) return;
  const int64_t stride = t.sample ? S_SLOTS * 16 : NB_SLOTS * 16;
  const float* S = t.sample ? srec : nrec;
  const int gi = t.g * 16 + (t.kind == T_OUTER ? o / t.cols : o);
  const int ai = t.a * 16 + (t.kind == T_OUTER ? o % t.cols : o);
  const int64_t i1 = i0 + GV_CHUNK < items ? i0 + GV_CHUNK : items;
  float acc = 0.0f;
  if (t.kind == T_BIAS) {
    for (int64_t it = i0; it < i1; ++it) acc += S[it * stride + gi];
  } else {
    for (int64_t it = i0; it < i1; ++it) acc += S[it * stride + gi] * S[it * stride + ai];
  }
  partial[(int64_t)blockIdx.y * nout + t.off + o] = acc;
}

// stage 2: the chunk partials in chunk order, added to the caller's gradient
__global__ __launch_bounds__(GV_BLOCK) void k_gtv_wgrad2(GvTerms T, GvG G, int64_t n_node, int64_t n_sample, int nout,
                                                         const float* __restrict__ partial) {
  const GvTerm& t = T.t[blockIdx.x];
  const int o = threadIdx.x;
  if (o >= t.rows * t.cols) return;
  const int64_t chunks = ((t.sample ? n_sample : n_node) + GV_CHUNK - 1) / GV_CHUNK;
  float acc = 0.0f;
  for (int64_t c = 0; c < chunks; ++c) acc += partial[c * nout + t.off + o];
  G.p[t.param][o] += acc;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
static int gv_nout() {
  static int n = -1;
  if (n < 0) make_terms(&n);
  return n;
}
// grid rows of stage 1: one per GV_CHUNK (sample, node) items, at most 65 535
#define GV_MAX_CHUNKS 65535

extern "C" int64_t tarl_value_gt_fwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  return plan->N * 16 + M * plan->N * NF_SLOTS * 16;
}

extern "C" int64_t tarl_value_gt_bwd_max_samples(const tarl_plan* plan) {
  if (!plan) return -1;
  return (int64_t)GV_MAX_CHUNKS * GV_CHUNK / (plan->N > 0 ? plan->N : 1);
}

extern "C" int64_t tarl_value_gt_bwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  const int64_t chunks = ceil_div(M * plan->N, GV_CHUNK);
  return plan->N * 16 + M * plan->N * NB_SLOTS * 16 + M * plan->E * 16 + M * S_SLOTS * 16 + chunks * gv_nout();
}

static int gv_check(const tarl_plan* plan, const float* obs16, int64_t M, const float* pe, const float* const* w,
                    float* scratch, GvW* W) {
  TARL_REQUIRE(plan && obs16 && pe && w && scratch, "null argument");
  TARL_REQUIRE(M >= 1, "bad sample count");
  TARL_REQUIRE(plan->N >= 1, "empty graph");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0 && ((uintptr_t)pe) % 16 == 0 && ((uintptr_t)scratch) % 16 == 0,
               "obs16 / pe / scratch must be 16-byte aligned");
  for (int i = 0; i < GV_NW_; ++i) {
    TARL_REQUIRE(w[i] != nullptr, "parameter pointer is null");
    W->p[i] = w[i];
  }
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
  hipLaunchKernelGGL(k_gtv_hoist, dim3((unsigned)ceil_div(N, GV_BLOCK)), dim3(GV_BLOCK), 0, s, W, pe, N, hoist);
  TARL_LAUNCH_CHECK();
  const unsigned gn = (unsigned)ceil_div(MN, GV_BLOCK);
  hipLaunchKernelGGL(k_gtv_nodeA<false>, dim3(gn), dim3(GV_BLOCK), 0, s, W, obs16, pe, (const float*)hoist, MN, N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<0, false>), dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<1, false>), dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_pool<false>, dim3((unsigned)M), dim3(GV_BLOCK), 0, s, W, (const float*)nrec, N, value,
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
  GvG G;
  for (int i = 0; i < GV_NP_; ++i) {
    TARL_REQUIRE(grads[i] != nullptr, "gradient pointer is null");
    G.p[i] = grads[i];
  }
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
  const unsigned gn = (unsigned)ceil_div(MN, GV_BLOCK);
  hipLaunchKernelGGL(k_gtv_hoist, dim3((unsigned)ceil_div(N, GV_BLOCK)), dim3(GV_BLOCK), 0, s, W, pe, N, hoist);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeA<true>, dim3(gn), dim3(GV_BLOCK), 0, s, W, obs16, pe, (const float*)hoist, MN, N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<0, true>), dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, alpha0);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_gtv_nodeB<1, true>), dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     MN, N, E, nrec, alpha1);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_pool<true>, dim3((unsigned)M), dim3(GV_BLOCK), 0, s, W, (const float*)nrec, N, (float*)nullptr,
                     grad_value, srec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeD, dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, MN, N, E,
                     nrec, (const float*)srec, (const float*)alpha1, gscore1);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeE<1>, dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     plan->out_ptr, plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)alpha1,
                     (const float*)gscore1, (const float*)alpha0, gscore0);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_nodeE<0>, dim3(gn), dim3(GV_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid,
                     plan->out_ptr, plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)alpha0,
                     (const float*)gscore0, (const float*)nullptr, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  int nout = 0;
  const GvTerms T = make_terms(&nout);
  const int64_t chunks = ceil_div(MN, GV_CHUNK);     // MN >= M items: the sample terms need fewer rows
  hipLaunchKernelGGL(k_gtv_wgrad1, dim3(GV_NP_, (unsigned)chunks), dim3(GV_BLOCK), 0, s, T, (const float*)nrec,
                     (const float*)srec, MN, M, nout, partial);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gtv_wgrad2, dim3(GV_NP_), dim3(GV_BLOCK), 0, s, T, G, MN, M, nout, (const float*)partial);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
