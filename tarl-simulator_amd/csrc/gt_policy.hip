// gt_policy.hip — the graph-transformer policy head of MPNNPolicyNet (policy_head = "graph_transformer"): the edge output of
// the reference's GraphTransformerNet (src/transformer/model.py:140-178, raw=True) as MLAgents builds it
// (src/agents/transformer_agent.py:30-39: 16 -> 16 hidden, 4 heads of d_k = 4, gate=True, two GTConv layers), in evaluation
// mode (BatchNorm on its running statistics, dropout = identity). Edge e = (u -> v), PyG source_to_target: i = v, j = u.
//
//   x0 = node_emb(obs16) + pe_emb(pe)              e0 = edge_emb(edge_attr)                       (model.py:160-164)
//   per layer (gt_conv.py:144-232):  Q, K, V = WQ x, WK x, WV x;  G = n_gate x + b
//     q_e = Q_v * K_u / 2 (per channel);  eij = WE(e) * q_e;  score_e,h = sum_{d in h} Q_v K_u / 2
//     alpha = softmax of the scores over the in-edges of v (PyG 2.5: group max subtracted, + 1e-16 in the denominator)
//     x' = BN2(y + FFN(y)),  y = BN1(WO(sum_u alpha V_u sigmoid(G_u)) + x)
//     e' = BN2e(z + FFN_e(z)), z = BN1e(WOe(eij) + e)                 FFN = Linear -> ReLU -> (Dropout) -> Linear
//   logits = edge_linear(e2)                                                                          (model.py:174-178)
//
// Only what reaches the logits is computed: the e_gate product is overwritten before use (gt_conv.py:218-222), and in the
// last layer WV, n_gate, WO, norm1, ffn and norm2 feed x2 alone (-> pool / value output). Those parameters receive no
// gradient here. fp32 on the vector ALU, one thread per (sample, node) or (sample, edge); the weights are wave-uniform
// (scalar loads from a pointer table passed by value).
//
// Passes (forward):  hoist (state-independent: P = pe_emb(pe) per node, e0 and E1 = WE1 e0 + b per edge) ->
//   node pass A (x0; Q1, K1, V1 * sigmoid(G1)) -> node pass B (segment softmax over the CSC in-edges, WO, BN, FFN, BN -> x1;
//   Q2, K2) -> edge pass C (both edge layers, edge_linear -> logits [M][E] in original edge order).
// Backward (forward recomputed inside): A, B and C store their activations in per-item records; C runs the edge chain
// backwards; node pass D walks the in- and out-edges (CSC / CSR order) for the gradients of Q2 / K2 and runs the node layer
// backwards to the attention; pass E walks them again for Q1 / K1 / V / G and x0. Weight gradients: every one is a sum over
// items (sample, node) or (sample, edge) of products of two recorded vectors — stage 1 sums fixed chunks of items per output
// in item order, stage 2 adds the chunk partials in chunk order into the caller's buffers. No atomics: bit-reproducible.
//
// The node side (the helpers, embedding, projections, the attention + layer body forwards and backwards, the Q / K / V / G
// gradient walk, the weight-gradient reduction) is gt_core.h, shared with the critic (gt_value.hip). This file keeps the
// parameter table, the edge side, the gather of the gradients of Q2 / K2 from the edge records, and the entry points.
#include "rollout_heads.h"
#include "gt_core.h"

// ---- the pointer table: trainable parameters in kernel order (GT_NP), then the BatchNorm running statistics -------------
enum {
  P_NODE_EMB = 0, P_PE_EMB, P_EDGE_EMB,
  // gt_layers.0
  P0_WQ, P0_WK, P0_WV, P0_NG_W, P0_NG_B, P0_WO_W, P0_WO_B, P0_N1_W, P0_N1_B, P0_F0_W, P0_F0_B, P0_F3_W, P0_F3_B, P0_N2_W,
  P0_N2_B,
  P0_WE_W, P0_WE_B, P0_WOE_W, P0_WOE_B, P0_N1E_W, P0_N1E_B, P0_FE0_W, P0_FE0_B, P0_FE3_W, P0_FE3_B, P0_N2E_W, P0_N2E_B,
  // gt_layers.1 (only what reaches the logits)
  P1_WQ, P1_WK,
  P1_WE_W, P1_WE_B, P1_WOE_W, P1_WOE_B, P1_N1E_W, P1_N1E_B, P1_FE0_W, P1_FE0_B, P1_FE3_W, P1_FE3_B, P1_N2E_W, P1_N2E_B,
  P_LIN_W, P_LIN_B,
  GT_NP_,
  // running_mean / running_var
  R0_N1_M = GT_NP_, R0_N1_V, R0_N2_M, R0_N2_V, R0_N1E_M, R0_N1E_V, R0_N2E_M, R0_N2E_V, R1_N1E_M, R1_N1E_V, R1_N2E_M,
  R1_N2E_V,
  GT_NW_
};
static_assert(GT_NP_ == TARL_GT_NUM_PARAMS, "parameter table out of step with the header");
static_assert(GT_NW_ == TARL_GT_NUM_TENSORS, "tensor table out of step with the header");

struct GtW {
  const float* p[GT_NW_];
};

// first parameter index of each edge layer's block (WE_W .. N2E_B) and its running statistics
__host__ __device__ constexpr int edge_par(int L) { return L == 0 ? P0_WE_W : P1_WE_W; }
__host__ __device__ constexpr int edge_run(int L) { return L == 0 ? R0_N1E_M : R1_N1E_M; }

// ---- record layouts --------------------------------------------------------------------------------------------------------
// node record (sample, node), gt_core.h's per-layer scheme: the forward keeps layer 0's {Q, K, V sigmoid(G), x0} and layer
// 1's Q, K (NF_SLOTS); the backward also layer 0's activations and gradients, then x1, obs16, pe and the gradients of Q2,
// K2 and x0 (NB_SLOTS)
enum { NQ2 = F_LAYER + FQ, NK2, NF_SLOTS };
enum { NX1 = NF_SLOTS + B_LAYER, NOBS, NPE, NGQ2, NGK2, NGX0, NB_SLOTS };
static_assert(NF_SLOTS == 6 && NB_SLOTS == 30, "the scratch sizes are part of the ABI");
using L0 = GtLayer<P0_WQ, R0_N1_M, 0, NF_SLOTS>;
using L1 = GtLayer<P1_WQ, -1, F_LAYER, -1>;          // Q and K alone: no statistics, no backward slots of its own
static_assert(P0_N2_B - P0_WQ == LN2_B && P1_WK - P1_WQ == LWK && R0_N2_V - R0_N1_M == LN2_V, "not gt_core.h's layer block");
enum { NQ1 = L0::F + FQ, NK1 = L0::F + FK };
// edge record (sample, edge), backward only: 18 slots per layer, then the edge attribute and the logit's gradient
enum { EIN = 0, EE, EQ, EIJ, ETH, EZ, EH, ER, ESH, EOUT, EGE, EGT, EGZ, EGH, EGS, EGOUT, EGIN, EGQ, E_LAYER_SLOTS };
enum { E_ATTR = 2 * E_LAYER_SLOTS, E_GLOGIT, E_SLOTS };
// hoisted per-edge / per-node constants: [E][32] = {e0, E1}, then [N][16] = P
#define HOIST_E 32

// ---- hoist -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GT_BLOCK) void k_gt_hoist(GtW W, const float* __restrict__ edge_attr,
                                                       const float* __restrict__ pe, int64_t N, int64_t E,
                                                       float* __restrict__ hoist) {
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid < E) {
    const float a = edge_attr[gid];
    float e0[16], e1[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) e0[i] = W.p[P_EDGE_EMB][i] * a;
    lin16(W.p[P0_WE_W], W.p[P0_WE_B], e0, e1);
    st16(hoist + gid * HOIST_E, e0);
    st16(hoist + gid * HOIST_E + 16, e1);
  } else if (gid < E + N) {
    const int64_t n = gid - E;
    pe_hoist(W.p[P_PE_EMB], pe + n * 16, hoist + E * HOIST_E + n * 16);
  }
}

// ---- node pass A: x0, Q1, K1, V1 * sigmoid(G1) -------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gt_nodeA(GtW W, const float* __restrict__ obs, const float* __restrict__ pe,
                                                       const float* __restrict__ P, int64_t MN, int64_t N,
                                                       float* __restrict__ nrec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t n = gid % N;
  float o[16], x0[16], t[16], g[16];
  embed(W.p[P_NODE_EMB], obs + gid * 16, P + n * 16, o, x0);
  float* r = nrec + gid * NS;
  node_proj<L0, BWD, false>(W, x0, r, t, g);
  if (BWD) {
    float p[16];
    st16(r + NOBS * 16, o);
    ld16(pe + n * 16, p);
    st16(r + NPE * 16, p);
  }
}

// ---- node pass B: segment softmax + aggregation, WO, BN1, FFN, BN2 -> x1; Q2, K2 ------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gt_nodeB(GtW W, const int32_t* __restrict__ in_ptr,
                                                       const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                       int64_t MN, int64_t N, int64_t E, float* __restrict__ nrec,
                                                       float* __restrict__ alpha) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, v = gid - m * N;
  float* r = nrec + gid * NS;
  float x1[16], t[16];
  layer_fwd<L0, NS, BWD>(W, in_src, in_eid, in_ptr[v], in_ptr[v + 1], r, nrec + m * N * NS,
                         BWD ? alpha + m * E * 4 : nullptr, x1);
  node_proj<L1, BWD, true>(W, x1, r, t, nullptr);
  if (BWD) st16(r + NX1 * 16, x1);
}

// ---- one edge layer -------------------------------------------------------------------------------------------------------------
// forward: ein = e, Ee = WE e + b; qv / ku = Q of the target, K of the source -> eout; rec (nullable) = the layer's record
template <int L>
__device__ __forceinline__ void edge_layer_fwd(const GtW& W, const float* ein, const float* Ee, const float* qv,
                                               const float* ku, float* eout, float* rec) {
  constexpr int P = edge_par(L), R = edge_run(L);
  float q[16], eij[16], t[16], th[16], z[16], h[16], r[16], s[16], sh[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    q[i] = (qv[i] * ku[i]) / 2.0f;                     // (Q_i * K_j) / sqrt(d_k) (gt_conv.py:214)
    eij[i] = Ee[i] * q[i];                             // E * qijk (:218)
  }
  lin16(W.p[P + 2], W.p[P + 3], eij, t);               // WOe(out_eij) + edge_attr_ (:205)
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = t[i] + ein[i];
  bn16(W.p[P + 4], W.p[P + 5], W.p[R + 0], W.p[R + 1], t, th, z);
  lin16(W.p[P + 6], W.p[P + 7], z, h);
#pragma unroll
  for (int i = 0; i < 16; ++i) r[i] = fmaxf(h[i], 0.0f);
  lin16(W.p[P + 8], W.p[P + 9], r, s);
#pragma unroll
  for (int i = 0; i < 16; ++i) s[i] = z[i] + s[i];
  bn16(W.p[P + 10], W.p[P + 11], W.p[R + 2], W.p[R + 3], s, sh, eout);
  if (rec) {
    st16(rec + EIN * 16, ein);
    st16(rec + EE * 16, Ee);
    st16(rec + EQ * 16, q);
    st16(rec + EIJ * 16, eij);
    st16(rec + ETH * 16, th);
    st16(rec + EZ * 16, z);
    st16(rec + EH * 16, h);
    st16(rec + ER * 16, r);
    st16(rec + ESH * 16, sh);
    st16(rec + EOUT * 16, eout);
  }
}

// backward of the layer from its record: geout -> gin (gradient of the layer's input edge features); gq -> the record
template <int L>
__device__ __forceinline__ void edge_layer_bwd(const GtW& W, float* rec, const float* geout, float* gin) {
  constexpr int P = edge_par(L), R = edge_run(L);
  float gs[16], gh[16], gz[16], gt[16], geij[16], v[16], w[16];
  bn16_bwd(W.p[P + 10], W.p[R + 3], geout, gs);
  lin16t(W.p[P + 8], gs, gh, false);
  ld16(rec + EH * 16, v);
#pragma unroll
  for (int i = 0; i < 16; ++i) gh[i] = v[i] > 0.0f ? gh[i] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) gz[i] = gs[i];
  lin16t(W.p[P + 6], gh, gz, true);
  bn16_bwd(W.p[P + 4], W.p[R + 1], gz, gt);
  lin16t(W.p[P + 2], gt, geij, false);
  ld16(rec + EQ * 16, v);
  ld16(rec + EE * 16, w);
  float gE[16], gq[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    gE[i] = geij[i] * v[i];
    gq[i] = geij[i] * w[i];
    gin[i] = gt[i];
  }
  lin16t(W.p[P + 0], gE, gin, true);
  st16(rec + EGOUT * 16, geout);
  st16(rec + EGS * 16, gs);
  st16(rec + EGH * 16, gh);
  st16(rec + EGZ * 16, gz);
  st16(rec + EGT * 16, gt);
  st16(rec + EGE * 16, gE);
  st16(rec + EGQ * 16, gq);
  st16(rec + EGIN * 16, gin);
}

// ---- edge pass C: both edge layers and edge_linear (forward: logits; backward: the records and the edge chain's gradients) ----
template <bool BWD>
__global__ __launch_bounds__(GT_BLOCK) void k_gt_edge(GtW W, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                      const float* __restrict__ edge_attr, const float* __restrict__ hoist,
                                                      const float* __restrict__ nrec, int64_t M, int64_t N, int64_t E,
                                                      float* __restrict__ logits, const float* __restrict__ grad_logits,
                                                      float* __restrict__ erec) {
  constexpr int NS = (BWD ? NB_SLOTS : NF_SLOTS) * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= M * E) return;
  const int64_t m = gid / E, e = gid - m * E;
  const float* nu = nrec + (m * N + src[e]) * NS;
  const float* nv = nrec + (m * N + dst[e]) * NS;
  float* rec = BWD ? erec + gid * (E_SLOTS * 16) : nullptr;
  float e0[16], Ee[16], qv[16], ku[16], e1[16], e2[16];
  ld16(hoist + e * HOIST_E, e0);
  ld16(hoist + e * HOIST_E + 16, Ee);
  ld16(nv + NQ1 * 16, qv);
  ld16(nu + NK1 * 16, ku);
  edge_layer_fwd<0>(W, e0, Ee, qv, ku, e1, rec);
  lin16(W.p[P1_WE_W], W.p[P1_WE_B], e1, Ee);
  ld16(nv + NQ2 * 16, qv);
  ld16(nu + NK2 * 16, ku);
  edge_layer_fwd<1>(W, e1, Ee, qv, ku, e2, BWD ? rec + E_LAYER_SLOTS * 16 : nullptr);
  if (!BWD) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) a += W.p[P_LIN_W][j] * e2[j];
    logits[gid] = a + W.p[P_LIN_B][0];
    return;
  }
  const float g = grad_logits[gid];
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.0f;
  v[0] = g;
  st16(rec + E_GLOGIT * 16, v);
  v[0] = edge_attr[e];
  st16(rec + E_ATTR * 16, v);
  float ge[16], gin[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) ge[i] = g * W.p[P_LIN_W][i];
  edge_layer_bwd<1>(W, rec + E_LAYER_SLOTS * 16, ge, gin);
  edge_layer_bwd<0>(W, rec, gin, ge);
}

// ---- node pass D: gradients of Q2 / K2 (walks of the in- and out-edges), node layer backwards, attention scores' gradients ------
__global__ __launch_bounds__(GT_BLOCK) void k_gt_nodeD(GtW W, const int32_t* __restrict__ in_ptr,
                                                       const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                       const int32_t* __restrict__ out_ptr,
                                                       const int32_t* __restrict__ out_dst,
                                                       const int32_t* __restrict__ out_eid, int64_t MN, int64_t N, int64_t E,
                                                       float* __restrict__ nrec, const float* __restrict__ erec,
                                                       const float* __restrict__ alpha, float* __restrict__ gscore) {
  constexpr int NS = NB_SLOTS * 16, ES = E_SLOTS * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  const float* base = nrec + m * N * NS;
  const float* eb = erec + m * E * ES;
  float gQ[16], gK[16], a[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { gQ[i] = 0.0f; gK[i] = 0.0f; }
  for (int k = in_ptr[n]; k < in_ptr[n + 1]; ++k) {        // n is the target: d q / d Q_v = K_u / 2
    ld16(eb + (int64_t)in_eid[k] * ES + (E_LAYER_SLOTS + EGQ) * 16, a);
    ld16(base + (int64_t)in_src[k] * NS + NK2 * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gQ[i] += a[i] * b[i] / 2.0f;
  }
  for (int k = out_ptr[n]; k < out_ptr[n + 1]; ++k) {      // n is the source: d q / d K_u = Q_v / 2
    ld16(eb + (int64_t)out_eid[k] * ES + (E_LAYER_SLOTS + EGQ) * 16, a);
    ld16(base + (int64_t)out_dst[k] * NS + NQ2 * 16, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) gK[i] += a[i] * b[i] / 2.0f;
  }
  float gx1[16], gt[16], gagg[16];
  lin16t(W.p[P1_WQ], gQ, gx1, false);
  lin16t(W.p[P1_WK], gK, gx1, true);
  st16(r + NGQ2 * 16, gQ);
  st16(r + NGK2 * 16, gK);
  body_bwd<L0>(W, r, gx1, gt, gagg);
  softmax_bwd<L0, NS>(in_src, in_eid, in_ptr[n], in_ptr[n + 1], base, gagg, alpha + m * E * 4, gscore + m * E * 4);
}

// ---- node pass E: gradients of Q1 / K1 / V1 / G1 and x0 ------------------------------------------------------------------------------
__global__ __launch_bounds__(GT_BLOCK) void k_gt_nodeE(GtW W, const int32_t* __restrict__ in_ptr,
                                                       const int32_t* __restrict__ in_src, const int32_t* __restrict__ in_eid,
                                                       const int32_t* __restrict__ out_ptr,
                                                       const int32_t* __restrict__ out_dst,
                                                       const int32_t* __restrict__ out_eid, int64_t MN, int64_t N, int64_t E,
                                                       float* __restrict__ nrec, const float* __restrict__ erec,
                                                       const float* __restrict__ alpha, const float* __restrict__ gscore) {
  constexpr int NS = NB_SLOTS * 16, ES = E_SLOTS * 16;
  const int64_t gid = (int64_t)blockIdx.x * GT_BLOCK + threadIdx.x;
  if (gid >= MN) return;
  const int64_t m = gid / N, n = gid - m * N;
  float* r = nrec + gid * NS;
  const float* base = nrec + m * N * NS;
  const float* eb = erec + m * E * ES;
  float gx0[16];
  qkvg_bwd<L0, NS, ES>(W, in_src, in_eid, in_ptr[n], in_ptr[n + 1], out_dst, out_eid, out_ptr[n], out_ptr[n + 1], r, base,
                       alpha + m * E * 4, gscore + m * E * 4, eb + EGQ * 16, gx0);
  st16(r + NGX0 * 16, gx0);
}

// ---- the weight gradients' terms (gt_core.h); second stream: the edge records ---------------------------------------------------------
static GtTermList<GT_NP_> make_terms() {
  GtTermList<GT_NP_> T;
  T.add(P_NODE_EMB, 0, NGX0, NOBS, T_OUTER, 16, 16);
  T.add(P_PE_EMB, 0, NGX0, NPE, T_OUTER, 16, 16);
  T.add(P_EDGE_EMB, 1, EGIN, E_ATTR, T_OUTER, 16, 1);
  T.add_node_layer<L0>();
  for (int L = 0; L < 2; ++L) {
    const int P = edge_par(L), o = L * E_LAYER_SLOTS;
    T.add(P + 0, 1, o + EGE, o + EIN, T_OUTER, 16, 16);
    T.add(P + 1, 1, o + EGE, 0, T_BIAS, 16, 1);
    T.add(P + 2, 1, o + EGT, o + EIJ, T_OUTER, 16, 16);
    T.add(P + 3, 1, o + EGT, 0, T_BIAS, 16, 1);
    T.add(P + 4, 1, o + EGZ, o + ETH, T_DIAG, 16, 1);
    T.add(P + 5, 1, o + EGZ, 0, T_BIAS, 16, 1);
    T.add(P + 6, 1, o + EGH, o + EZ, T_OUTER, 16, 16);
    T.add(P + 7, 1, o + EGH, 0, T_BIAS, 16, 1);
    T.add(P + 8, 1, o + EGS, o + ER, T_OUTER, 16, 16);
    T.add(P + 9, 1, o + EGS, 0, T_BIAS, 16, 1);
    T.add(P + 10, 1, o + EGOUT, o + ESH, T_DIAG, 16, 1);
    T.add(P + 11, 1, o + EGOUT, 0, T_BIAS, 16, 1);
    if (L == 0) {
      T.add(P1_WQ, 0, NGQ2, NX1, T_OUTER, 16, 16);
      T.add(P1_WK, 0, NGK2, NX1, T_OUTER, 16, 16);
    }
  }
  T.add(P_LIN_W, 1, E_GLOGIT, E_LAYER_SLOTS + EOUT, T_OUTER, 1, 16);
  T.add(P_LIN_B, 1, E_GLOGIT, 0, T_BIAS, 1, 1);
  return T;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------
static int64_t hoist_floats(const tarl_plan* plan) { return plan->E * HOIST_E + plan->N * 16; }

extern "C" int64_t tarl_policy_gt_fwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  return hoist_floats(plan) + M * plan->N * NF_SLOTS * 16;
}

extern "C" int64_t tarl_policy_gt_bwd_scratch_floats(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 0) return -1;
  return hoist_floats(plan) + M * plan->N * NB_SLOTS * 16 + M * plan->E * (E_SLOTS * 16 + 8) +
         gt_wgrad_chunks(M * plan->N, M * plan->E) * make_terms().nout;
}

static int gt_check(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr, const float* pe,
                    const float* const* w, GtW* W) {
  TARL_REQUIRE(plan && obs16 && edge_attr && pe && w, "null argument");
  TARL_REQUIRE(M >= 1, "bad sample count");
  TARL_REQUIRE(((uintptr_t)obs16) % 16 == 0 && ((uintptr_t)pe) % 16 == 0, "obs16 / pe must be 16-byte aligned");
  TARL_REQUIRE(gt_table(w, W->p, GT_NW_), "parameter pointer is null");
  return TARL_OK;
}

static int launch_hoist(const tarl_plan* plan, const GtW& W, const float* edge_attr, const float* pe, float* hoist,
                        hipStream_t s) {
  const int64_t n = plan->E + plan->N;
  if (n == 0) return TARL_OK;
  hipLaunchKernelGGL(k_gt_hoist, dim3((unsigned)ceil_div(n, GT_BLOCK)), dim3(GT_BLOCK), 0, s, W, edge_attr, pe, plan->N,
                     plan->E, hoist);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// node passes A, B and the edge pass of the forward (hoist already in scratch)
static int launch_fwd(const tarl_plan* plan, const GtW& W, const float* obs16, const float* pe, int64_t M,
                      const float* edge_attr, float* scratch, float* logits, hipStream_t s) {
  const int64_t N = plan->N, E = plan->E, MN = M * N;
  const float* hoist = scratch;
  float* nrec = scratch + hoist_floats(plan);
  const unsigned gn = (unsigned)ceil_div(MN, GT_BLOCK);
  hipLaunchKernelGGL(k_gt_nodeA<false>, dim3(gn), dim3(GT_BLOCK), 0, s, W, obs16, pe, hoist + E * HOIST_E, MN, N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gt_nodeB<false>, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, MN, N,
                     E, nrec, (float*)nullptr);
  TARL_LAUNCH_CHECK();
  if (E == 0) return TARL_OK;
  hipLaunchKernelGGL(k_gt_edge<false>, dim3((unsigned)ceil_div(M * E, GT_BLOCK)), dim3(GT_BLOCK), 0, s, W, plan->src,
                     plan->dst, edge_attr, hoist, (const float*)nrec, M, N, E, logits, (const float*)nullptr,
                     (float*)nullptr);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_policy_gt_fwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr,
                                  const float* pe, const float* const* w, float* scratch, int64_t scratch_floats,
                                  float* logits, tarl_stream stream) {
  GtW W;
  int rc = gt_check(plan, obs16, M, edge_attr, pe, w, &W);
  if (rc) return rc;
  TARL_REQUIRE(logits && scratch, "null logits / scratch");
  TARL_REQUIRE(((uintptr_t)scratch) % 16 == 0, "scratch must be 16-byte aligned");
  TARL_REQUIRE(scratch_floats >= tarl_policy_gt_fwd_scratch_floats(plan, M), "scratch smaller than tarl_policy_gt_fwd_scratch_floats");
  if (plan->N == 0) return TARL_OK;
  hipStream_t s = (hipStream_t)stream;
  rc = launch_hoist(plan, W, edge_attr, pe, scratch, s);
  if (rc) return rc;
  return launch_fwd(plan, W, obs16, pe, M, edge_attr, scratch, logits, s);
}

extern "C" int tarl_policy_gt_bwd(const tarl_plan* plan, const float* obs16, int64_t M, const float* edge_attr,
                                  const float* pe, const float* const* w, const float* grad_logits, float* scratch,
                                  int64_t scratch_floats, float* const* grads, tarl_stream stream) {
  GtW W;
  int rc = gt_check(plan, obs16, M, edge_attr, pe, w, &W);
  if (rc) return rc;
  TARL_REQUIRE(grad_logits && scratch && grads, "null grad_logits / scratch / grads");
  TARL_REQUIRE(((uintptr_t)scratch) % 16 == 0, "scratch must be 16-byte aligned");
  TARL_REQUIRE(scratch_floats >= tarl_policy_gt_bwd_scratch_floats(plan, M), "scratch smaller than tarl_policy_gt_bwd_scratch_floats");
  GtGrads<GT_NP_> G;
  TARL_REQUIRE(gt_table(grads, G.p, GT_NP_), "gradient pointer is null");
  if (plan->N == 0) return TARL_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = plan->N, E = plan->E, MN = M * N, ME = M * E;
  float* hoist = scratch;
  float* nrec = hoist + hoist_floats(plan);
  float* erec = nrec + MN * NB_SLOTS * 16;
  float* alpha = erec + ME * E_SLOTS * 16;
  float* gscore = alpha + ME * 4;
  float* partial = gscore + ME * 4;
  rc = launch_hoist(plan, W, edge_attr, pe, hoist, s);
  if (rc) return rc;
  const unsigned gn = (unsigned)ceil_div(MN, GT_BLOCK);
  hipLaunchKernelGGL(k_gt_nodeA<true>, dim3(gn), dim3(GT_BLOCK), 0, s, W, obs16, pe, (const float*)(hoist + E * HOIST_E), MN,
                     N, nrec);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gt_nodeB<true>, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, MN, N,
                     E, nrec, alpha);
  TARL_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(k_gt_edge<true>, dim3((unsigned)ceil_div(ME, GT_BLOCK)), dim3(GT_BLOCK), 0, s, W, plan->src,
                       plan->dst, edge_attr, (const float*)hoist, (const float*)nrec, M, N, E, (float*)nullptr, grad_logits,
                       erec);
    TARL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_gt_nodeD, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, plan->out_ptr,
                     plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)erec, (const float*)alpha, gscore);
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gt_nodeE, dim3(gn), dim3(GT_BLOCK), 0, s, W, plan->in_ptr, plan->in_src, plan->in_eid, plan->out_ptr,
                     plan->out_dst, plan->out_eid, MN, N, E, nrec, (const float*)erec, (const float*)alpha,
                     (const float*)gscore);
  TARL_LAUNCH_CHECK();
  return gt_wgrad_launch(__func__, "too many gradient chunks for one grid dimension", make_terms(), G, nrec, NB_SLOTS * 16, MN,
                         erec, E_SLOTS * 16, ME, partial, s);
}

// ---- the rollout head (rollout_heads.h): the state-independent terms once per call, then per frame kept rows -> observation
// -> forward
struct GtHead {
  GtW W;
  const float* pe;
  float *obs_scratch, *gt_scratch;
};

static int gt_frame(const HeadRollout& a, void* ctx, int64_t t, const int32_t* env, const int32_t* slot, int64_t n) {
  const GtHead& h = *(const GtHead*)ctx;
  int rc = t == 0 ? launch_hoist(a.plan, h.W, a.edge_attr, h.pe, h.gt_scratch, (hipStream_t)a.stream) : TARL_OK;
  if (!rc) rc = tarl_head_keep_rows(a, env, slot, n);
  if (rc) return rc;
  rc = tarl_fused_obs16(a.plan, a.f, a.x, a.B, a.x_bstride, a.ldx, a.Nmax, a.agent_features, a.A, a.a_bstride, h.obs_scratch,
                        a.stream);
  if (rc) return rc;
  return launch_fwd(a.plan, h.W, h.obs_scratch, h.pe, a.B, a.edge_attr, h.gt_scratch, a.logits_scratch, (hipStream_t)a.stream);
}

extern "C" int tarl_fused_rollout_gt(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t T,
                                     const float* times_host, float prev_time, const float* x, int64_t x_bstride,
                                     int64_t ldx, float* agent_features, int64_t A, int64_t a_bstride,
                                     const float* edge_attr, const float* log_edge_attr, float log_eps, int use_cong,
                                     const float* pe, const float* const* w, float temperature, uint64_t policy_seed,
                                     uint64_t policy_counter0, uint64_t seed, uint64_t counter0,
                                     const int64_t* keep_ptr_host, const int32_t* keep_env, const int32_t* keep_slot,
                                     float* obs_keep, float* obs_scratch, float* gt_scratch, int64_t gt_scratch_floats,
                                     float* logits_scratch, void* dist_scratch, int32_t* ins_scratch, uint8_t* choice8,
                                     float* log_prob, float* reward, uint8_t* counts, tarl_stream stream) {
  TARL_REQUIRE(plan && obs_scratch && gt_scratch, "plan / observation / forward scratch missing");
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  TARL_REQUIRE(((uintptr_t)obs_scratch) % 16 == 0 && ((uintptr_t)gt_scratch) % 16 == 0, "scratch must be 16-byte aligned");
  TARL_REQUIRE(gt_scratch_floats >= tarl_policy_gt_fwd_scratch_floats(plan, B),
               "gt_scratch smaller than tarl_policy_gt_fwd_scratch_floats(plan, B)");
  GtHead h{{}, pe, obs_scratch, gt_scratch};
  const int rc = gt_check(plan, obs_scratch, B, edge_attr, pe, w, &h.W);
  if (rc) return rc;
  // (no per-step logs: metrics_envs = 0 and null series)
  return tarl_rollout_head(HeadRollout{plan, f, B, Nmax, T, times_host, prev_time, x, x_bstride, ldx, agent_features, A,
                                       a_bstride, edge_attr, log_edge_attr, log_eps, use_cong, temperature, policy_seed,
                                       policy_counter0, seed, counter0, keep_ptr_host, keep_env, keep_slot, obs_keep,
                                       logits_scratch, dist_scratch, ins_scratch, choice8, log_prob, reward, counts, 0, nullptr,
                                       nullptr, nullptr, stream},
                           gt_frame, &h);
}
