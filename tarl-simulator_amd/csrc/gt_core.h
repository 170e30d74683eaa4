// gt_core.h — the shared core of the two graph-transformer kernels: the policy head (gt_policy.hip) and the critic
// (gt_value.hip) evaluate the same GraphTransformerNet(16 -> 16, 4 heads of d_k = 4, gate, two GTConv layers) of the
// reference in evaluation mode, and everything on its node side is here exactly once:
//   the 16-wide helpers; the node-layer parameter block and record layout; x0 = node_emb(obs16) + pe_emb(pe) and the pe_emb
//   hoist; a layer's projections Q, K, V * sigmoid(G); the attention + layer body forwards (three walks of the CSC
//   in-segment: max, denominator + 1e-16, aggregate; WO + residual, BN1, FFN, residual, BN2); the body backwards; the softmax
//   backward; the Q / K / V / G gradient walk over the in- and out-edges; the deterministic weight-gradient reduction.
// The files keep their parameter tables, what is theirs alone (the edge side; the pool) and their entry points.
//
// fp32 on the vector ALU, one thread per (sample, node); the weights are wave-uniform (scalar loads from a pointer table
// WT { const float* p[]; } passed to the kernel by value). Every fp32 expression is written once and in one operand order
// (-ffp-contract=off): what the two heads compute cannot drift apart.
//
// The device functions take the thread's record r, its sample's first record `base`, the segment bounds and the sample's
// alpha / g_score rows from the kernel instead of deriving them again from gid; NS (floats per record) is a template
// argument, as the forward's records are shorter than the backward's.
#pragma once
#include <math.h>

#include "tarl_common.h"

#define GT_BLOCK 256
#define GT_CHUNK 1024            // items per stage-1 partial sum of the weight gradients
#define GT_MAX_CHUNKS 65535      // grid rows of stage 1: one per GT_CHUNK items

// ---- one node layer: its parameter block, its running statistics, its slots of the node record ---------------------------
// 15 parameters from P: WQ, WK, WV, n_gate.{w,b}, WO.{w,b}, norm1.{w,b}, ffn.mlp.0.{w,b}, ffn.mlp.3.{w,b}, norm2.{w,b};
// 4 running statistics from R: norm1.{mean,var}, norm2.{mean,var}
enum { LWQ = 0, LWK, LWV, LNG_W, LNG_B, LWO_W, LWO_B, LN1_W, LN1_B, LF0_W, LF0_B, LF3_W, LF3_B, LN2_W, LN2_B, L_NP };
enum { LN1_M = 0, LN1_V, LN2_M, LN2_V, L_NR };
// node record (sample, node): 16-float slots. Per layer the forward keeps {Q, K, V sigmoid(G), input x} from slot F, the
// backward also its activations and gradients from slot B (GX: the gradient of the layer's output, GT: of WO(out) + x).
enum { FQ = 0, FK, FVG, FX, F_LAYER };
enum { BV = 0, BSG, BAGG, BTH, BY, BH, BR, BSH, BGQ, BGK, BGV, BGG, BGX, BGS, BGH, BGY, BGT, BGAGG, B_LAYER };
template <int P_, int R_, int F_, int B_>
struct GtLayer {
  static constexpr int P = P_, R = R_, F = F_, B = B_;
};

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

// ---- embedding ---------------------------------------------------------------------------------------------------------------
// the state-independent part of x0 for one node: P = pe_emb(pe)
__device__ __forceinline__ void pe_hoist(const float* __restrict__ pe_emb, const float* __restrict__ pe_n,
                                         float* __restrict__ P_n) {
  float p[16], q[16];
  ld16(pe_n, p);
  lin16(pe_emb, nullptr, p, q);
  st16(P_n, q);
}
// o = the observation row, x0 = node_emb(o) + P
__device__ __forceinline__ void embed(const float* __restrict__ node_emb, const float* __restrict__ obs_row,
                                      const float* __restrict__ P_n, float* o, float* x0) {
  float p[16];
  ld16(obs_row, o);
  ld16(P_n, p);
  lin16(node_emb, nullptr, o, x0);
#pragma unroll
  for (int i = 0; i < 16; ++i) x0[i] = x0[i] + p[i];
}

// ---- a layer's projections of its input x into the record r: Q, K, V sigmoid(G), x (and V, sigmoid(G) for the backward) -----
// QK_ONLY: Q and K alone (the policy's last layer: V and G feed x2, which the logits never read; x is the caller's to keep).
// t, g: two 16-float temporaries of the caller's (g unused when QK_ONLY). They are not locals of this function on purpose:
// with arrays of its own the compiler orders the packed fp32 products of pass A differently once this is inlined, and
// k_gt_nodeA needs 256 VGPRs (1 wave / SIMD) instead of 72 (7) — profiles/gt_core_ab.txt.
template <class Ly, bool BWD, bool QK_ONLY, class WT>
__device__ __forceinline__ void node_proj(const WT& W, const float* x, float* r, float* t, float* g) {
  constexpr int P = Ly::P;
  lin16(W.p[P + LWQ], nullptr, x, t);
  st16(r + (Ly::F + FQ) * 16, t);
  lin16(W.p[P + LWK], nullptr, x, t);
  st16(r + (Ly::F + FK) * 16, t);
  if constexpr (!QK_ONLY) {
    st16(r + (Ly::F + FX) * 16, x);
    lin16(W.p[P + LWV], nullptr, x, t);
    lin16(W.p[P + LNG_W], W.p[P + LNG_B], x, g);
#pragma unroll
    for (int i = 0; i < 16; ++i) g[i] = sigmoidf_(g[i]);
    if (BWD) {
      st16(r + (Ly::B + BV) * 16, t);
      st16(r + (Ly::B + BSG) * 16, g);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = t[i] * g[i];
    st16(r + (Ly::F + FVG) * 16, t);
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

// ---- a layer forwards for one (sample, node): segment softmax over the in-edges [k0, k1) + aggregation, WO, BN1, FFN, BN2 ----
// -> xo, the layer's output; BWD: alpha of every in-edge to alpha_m (the sample's [E][4]) and the activations to the record
template <class Ly, int NS, bool BWD, class WT>
__device__ __forceinline__ void layer_fwd(const WT& W, const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                          int k0, int k1, float* r, const float* base, float* alpha_m, float* xo) {
  static_assert(Ly::R >= 0 && Ly::B >= 0, "a layer that stops at Q and K has no body");
  constexpr int P = Ly::P, R = Ly::R, KS = (Ly::F + FK) * 16, VS = (Ly::F + FVG) * 16;
  float q[16], s[4], mx[4], den[4], agg[16];
  ld16(r + (Ly::F + FQ) * 16, q);
#pragma unroll
  for (int h = 0; h < 4; ++h) { mx[h] = -INFINITY; den[h] = 0.0f; }
  for (int k = k0; k < k1; ++k) {
    scores4(q, base + (int64_t)in_src[k] * NS + KS, s);
#pragma unroll
    for (int h = 0; h < 4; ++h) mx[h] = fmaxf(mx[h], s[h]);
  }
  for (int k = k0; k < k1; ++k) {
    scores4(q, base + (int64_t)in_src[k] * NS + KS, s);
#pragma unroll
    for (int h = 0; h < 4; ++h) den[h] += expf(s[h] - mx[h]);
  }
#pragma unroll
  for (int h = 0; h < 4; ++h) den[h] = den[h] + 1e-16f;
#pragma unroll
  for (int i = 0; i < 16; ++i) agg[i] = 0.0f;
  for (int k = k0; k < k1; ++k) {
    const int64_t u = in_src[k];
    scores4(q, base + u * NS + KS, s);
    float vg[16];
    ld16(base + u * NS + VS, vg);
    float a[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) a[h] = expf(s[h] - mx[h]) / den[h];
    if (BWD) *reinterpret_cast<float4*>(alpha_m + (int64_t)in_eid[k] * 4) = make_float4(a[0], a[1], a[2], a[3]);
#pragma unroll
    for (int i = 0; i < 16; ++i) agg[i] += a[i >> 2] * vg[i];
  }
  float x[16], t[16], th[16], y[16], hh[16], rr[16], f[16], sh[16];
  ld16(r + (Ly::F + FX) * 16, x);
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
  if (BWD) {
    st16(r + (Ly::B + BAGG) * 16, agg);
    st16(r + (Ly::B + BTH) * 16, th);
    st16(r + (Ly::B + BY) * 16, y);
    st16(r + (Ly::B + BH) * 16, hh);
    st16(r + (Ly::B + BR) * 16, rr);
    st16(r + (Ly::B + BSH) * 16, sh);
  }
}

// ---- a layer backwards from the gradient of its output gx to the attention: the record's gradient slots, gt (the
// residual's gradient) and gagg ---------------------------------------------------------------------------------------------
template <class Ly, class WT>
__device__ __forceinline__ void body_bwd(const WT& W, float* r, const float* gx, float* gt, float* gagg) {
  static_assert(Ly::R >= 0 && Ly::B >= 0, "a layer that stops at Q and K has no body");
  constexpr int P = Ly::P, R = Ly::R;
  float gs[16], gh[16], gy[16], a[16];
  bn16_bwd(W.p[P + LN2_W], W.p[R + LN2_V], gx, gs);
  lin16t(W.p[P + LF3_W], gs, gh, false);
  ld16(r + (Ly::B + BH) * 16, a);
#pragma unroll
  for (int i = 0; i < 16; ++i) gh[i] = a[i] > 0.0f ? gh[i] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) gy[i] = gs[i];
  lin16t(W.p[P + LF0_W], gh, gy, true);
  bn16_bwd(W.p[P + LN1_W], W.p[R + LN1_V], gy, gt);
  lin16t(W.p[P + LWO_W], gt, gagg, false);
  st16(r + (Ly::B + BGX) * 16, gx);
  st16(r + (Ly::B + BGS) * 16, gs);
  st16(r + (Ly::B + BGH) * 16, gh);
  st16(r + (Ly::B + BGY) * 16, gy);
  st16(r + (Ly::B + BGT) * 16, gt);
  st16(r + (Ly::B + BGAGG) * 16, gagg);
}

// softmax backward over the in-edges [k0, k1) of a node (CSC order), two passes: g_score = alpha (g_alpha - sum_k alpha_k
// g_alpha_k), g_alpha = <g_agg, V_u sigmoid(G_u)>_head
template <class Ly, int NS>
__device__ __forceinline__ void softmax_bwd(const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid, int k0,
                                            int k1, const float* base, const float* gagg, const float* __restrict__ alpha_m,
                                            float* __restrict__ gscore_m) {
  float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[16];
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = k0; k < k1; ++k) {
      const int64_t eid = in_eid[k];
      ld16(base + (int64_t)in_src[k] * NS + (Ly::F + FVG) * 16, b);
      const float4 al = *reinterpret_cast<const float4*>(alpha_m + eid * 4);
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
        *reinterpret_cast<float4*>(gscore_m + eid * 4) =
            make_float4(av[0] * (ga[0] - dot[0]), av[1] * (ga[1] - dot[1]), av[2] * (ga[2] - dot[2]), av[3] * (ga[3] - dot[3]));
      }
    }
  }
}

// ---- gradients of a layer's Q / K / V / G by walks of the in-edges [i0, i1) (CSC) and the out-edges [o0, o1) (CSR) of the
// node, then gx = the gradient of the layer's input x (residual first, then WQ, WK, WV, n_gate) -----------------------------
// ES > 0: each edge adds a term of its own to the score's gradient, per channel, read from egq + eid * ES (the policy's edge
// layer: eij = WE(e) * q_e); ES = 0: the attention alone
template <class Ly, int NS, int ES, class WT>
__device__ __forceinline__ void qkvg_bwd(const WT& W, const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                         int i0, int i1, const int32_t* __restrict__ out_dst,
                                         const int32_t* __restrict__ out_eid, int o0, int o1, float* r, const float* base,
                                         const float* __restrict__ alpha_m, const float* __restrict__ gscore_m,
                                         const float* __restrict__ egq, float* gx) {
  constexpr int P = Ly::P;
  float gQ[16], gK[16], gVG[16], a[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { gQ[i] = 0.0f; gK[i] = 0.0f; gVG[i] = 0.0f; }
  for (int k = i0; k < i1; ++k) {                          // the node is the target: d score / d Q_v = K_u / 2
    const int64_t eid = in_eid[k];
    if constexpr (ES > 0) ld16(egq + eid * ES, a);
    const float4 gsc = *reinterpret_cast<const float4*>(gscore_m + eid * 4);
    const float gv[4] = {gsc.x, gsc.y, gsc.z, gsc.w};
    ld16(base + (int64_t)in_src[k] * NS + (Ly::F + FK) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if constexpr (ES > 0) gQ[i] += (a[i] + gv[i >> 2]) * b[i] / 2.0f;
      else gQ[i] += gv[i >> 2] * b[i] / 2.0f;
    }
  }
  for (int k = o0; k < o1; ++k) {                          // the source: d score / d K_u = Q_v / 2; messages V_u sigma(G_u)
    const int64_t eid = out_eid[k], v = out_dst[k];
    if constexpr (ES > 0) ld16(egq + eid * ES, a);
    const float4 gsc = *reinterpret_cast<const float4*>(gscore_m + eid * 4);
    const float gv[4] = {gsc.x, gsc.y, gsc.z, gsc.w};
    ld16(base + v * NS + (Ly::F + FQ) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if constexpr (ES > 0) gK[i] += (a[i] + gv[i >> 2]) * b[i] / 2.0f;
      else gK[i] += gv[i >> 2] * b[i] / 2.0f;
    }
    const float4 al = *reinterpret_cast<const float4*>(alpha_m + eid * 4);
    const float av[4] = {al.x, al.y, al.z, al.w};
    ld16(base + v * NS + (Ly::B + BGAGG) * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gVG[i] += av[i >> 2] * b[i];
  }
  float V[16], sg[16], gV[16], gG[16];
  ld16(r + (Ly::B + BV) * 16, V);
  ld16(r + (Ly::B + BSG) * 16, sg);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    gV[i] = gVG[i] * sg[i];
    gG[i] = gVG[i] * V[i] * (sg[i] * (1.0f - sg[i]));
  }
  ld16(r + (Ly::B + BGT) * 16, gx);              // the residual of WO(out) + x_
  lin16t(W.p[P + LWQ], gQ, gx, true);
  lin16t(W.p[P + LWK], gK, gx, true);
  lin16t(W.p[P + LWV], gV, gx, true);
  lin16t(W.p[P + LNG_W], gG, gx, true);
  st16(r + (Ly::B + BGQ) * 16, gQ);
  st16(r + (Ly::B + BGK) * 16, gK);
  st16(r + (Ly::B + BGV) * 16, gV);
  st16(r + (Ly::B + BGG) * 16, gG);
}

// ---- weight gradients: sum over items of g[i] * a[j] (outer), g[i] (bias) or g[i] * a[i] (BatchNorm weight) ------------------
// Every one is a sum over the items of one of two record streams — the node records (sample, node), or the head's second
// stream (the policy's edge records, the critic's sample records) — of products of two recorded slots. Stage 1 sums fixed
// chunks of items per output in item order, stage 2 adds the chunk partials in chunk order into the caller's buffers.
// No atomics: bit-reproducible. One term per parameter: NT = the number of parameters.
enum { T_OUTER = 0, T_BIAS, T_DIAG };
struct GtTerm {
  int16_t param, second, g, a, kind, rows, cols;    // second: the slots g, a are of the second stream's records
  int32_t off;                                      // offset of the parameter's outputs in the partial-sum rows
};
template <int NT>
struct GtTerms {
  GtTerm t[NT];
};
template <int NT>
struct GtGrads {
  float* p[NT];
};
// the term list as the host builds it; nout = outputs per partial-sum row
template <int NT>
struct GtTermList {
  GtTerms<NT> T{};
  int k = 0, nout = 0;
  void add(int param, int second, int g, int a, int kind, int rows, int cols) {
    T.t[k++] = GtTerm{(int16_t)param, (int16_t)second, (int16_t)g, (int16_t)a, (int16_t)kind, (int16_t)rows, (int16_t)cols, nout};
    nout += rows * cols;
  }
  // the 15 parameters of a node layer from its record slots (x: the slot of the layer's input)
  template <class Ly>
  void add_node_layer() {
    static_assert(Ly::R >= 0 && Ly::B >= 0, "a layer that stops at Q and K has no body");
    constexpr int P = Ly::P, B = Ly::B, x = Ly::F + FX;
    add(P + LWQ, 0, B + BGQ, x, T_OUTER, 16, 16);
    add(P + LWK, 0, B + BGK, x, T_OUTER, 16, 16);
    add(P + LWV, 0, B + BGV, x, T_OUTER, 16, 16);
    add(P + LNG_W, 0, B + BGG, x, T_OUTER, 16, 16);
    add(P + LNG_B, 0, B + BGG, 0, T_BIAS, 16, 1);
    add(P + LWO_W, 0, B + BGT, B + BAGG, T_OUTER, 16, 16);
    add(P + LWO_B, 0, B + BGT, 0, T_BIAS, 16, 1);
    add(P + LN1_W, 0, B + BGY, B + BTH, T_DIAG, 16, 1);
    add(P + LN1_B, 0, B + BGY, 0, T_BIAS, 16, 1);
    add(P + LF0_W, 0, B + BGH, B + BY, T_OUTER, 16, 16);
    add(P + LF0_B, 0, B + BGH, 0, T_BIAS, 16, 1);
    add(P + LF3_W, 0, B + BGS, B + BR, T_OUTER, 16, 16);
    add(P + LF3_B, 0, B + BGS, 0, T_BIAS, 16, 1);
    add(P + LN2_W, 0, B + BGX, B + BSH, T_DIAG, 16, 1);
    add(P + LN2_B, 0, B + BGX, 0, T_BIAS, 16, 1);
  }
};

// stage 1: block (term, chunk), one thread per output, items of the chunk in ascending order. rec0 / rec1: the node
// records and the second stream's, stride0 / stride1 floats apart, n0 / n1 items.
template <int NT>
__global__ __launch_bounds__(GT_BLOCK) void k_gt_wgrad1(GtTerms<NT> T, const float* __restrict__ rec0,
                                                        const float* __restrict__ rec1, int stride0, int stride1,
                                                        int64_t n0, int64_t n1, int nout, float* __restrict__ partial) {
  const GtTerm& t = T.t[blockIdx.x];
  const int64_t items = t.second ? n1 : n0;
  const int64_t i0 = (int64_t)blockIdx.y * GT_CHUNK;
  const int o = threadIdx.x;
  if (i0 >= items || o >= t.rows * t.cols) return;
  const int64_t stride = t.second ? stride1 : stride0;
  const float* S = t.second ? rec1 : rec0;
  const int gi = t.g * 16 + (t.kind == T_OUTER ? o / t.cols : o);
  const int ai = t.a * 16 + (t.kind == T_OUTER ? o % t.cols : o);
  const int64_t i1 = i0 + GT_CHUNK < items ? i0 + GT_CHUNK : items;
  float acc = 0.0f;
  if (t.kind == T_BIAS) {
    for (int64_t it = i0; it < i1; ++it) acc += S[it * stride + gi];
  } else {
    for (int64_t it = i0; it < i1; ++it) acc += S[it * stride + gi] * S[it * stride + ai];
  }
  partial[(int64_t)blockIdx.y * nout + t.off + o] = acc;
}

// stage 2: the chunk partials in chunk order, added to the caller's gradient
template <int NT>
__global__ __launch_bounds__(GT_BLOCK) void k_gt_wgrad2(GtTerms<NT> T, GtGrads<NT> G, int64_t n0, int64_t n1, int nout,
                                                        const float* __restrict__ partial) {
  const GtTerm& t = T.t[blockIdx.x];
  const int o = threadIdx.x;
  if (o >= t.rows * t.cols) return;
  const int64_t chunks = ((t.second ? n1 : n0) + GT_CHUNK - 1) / GT_CHUNK;
  float acc = 0.0f;
  for (int64_t c = 0; c < chunks; ++c) acc += partial[c * nout + t.off + o];
  G.p[t.param][o] += acc;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// partial-sum rows of one backward call
static inline int64_t gt_wgrad_chunks(int64_t n0, int64_t n1) { return ceil_div(n0 > n1 ? n0 : n1, GT_CHUNK); }

// both stages; more rows than one grid dimension holds is refused in the caller's words (entry: its name, as TARL_REQUIRE
// would lead the message)
template <int NT>
static int gt_wgrad_launch(const char* entry, const char* too_many, const GtTermList<NT>& L, const GtGrads<NT>& G,
                           const float* rec0, int stride0, int64_t n0, const float* rec1, int stride1, int64_t n1,
                           float* partial, hipStream_t s) {
  const int64_t chunks = gt_wgrad_chunks(n0, n1);
  if (chunks > GT_MAX_CHUNKS) {
    tarl_set_error("%s: requirement failed: %s", entry, too_many);
    return TARL_ERR_INVALID;
  }
  hipLaunchKernelGGL(k_gt_wgrad1<NT>, dim3(NT, (unsigned)chunks), dim3(GT_BLOCK), 0, s, L.T, rec0, rec1, stride0, stride1, n0,
                     n1, L.nout, partial);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gt_wgrad2<NT>, dim3(NT), dim3(GT_BLOCK), 0, s, L.T, G, n0, n1, L.nout, (const float*)partial);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// fills a kernel's pointer table from the caller's array of n pointers; false if one of them is null
template <class T>
static inline bool gt_table(T* const* src, T** dst, int n) {
  for (int i = 0; i < n; ++i) {
    if (!src[i]) return false;
    dst[i] = src[i];
  }
  return true;
}
