// bc.hip — behaviour cloning of the shortest-path router into the policy heads: the expert's action of every
// row as a label that leaves the packed state alone, and the per-node cross-entropy on those labels, forward and backward.
// Not in the reference: a warm start for the learned heads, off unless asked for.
//
//   k_fused_expert_labels   the rank byte k_fused_select_next_hop_dest<false> (baseline.hip) would write for a row, computed
//                           by the same code (fused_select.h: fs_head_agent, fs_next_hop_code, fs_rank_code) and written to an
//                           env-major [B][N] byte array instead of sel8 / sel. TARL_BC_IGNORE (0xFF) on an empty row (the
//                           policy-hold kernel's test, made first: one 4-byte load and the lane is done), where the select
//                           kernel would leave the row untouched, and where it would write the raw code.
//   k_graphdist_bc          per (sample, tile of BC_TILE nodes): the cross-entropy of every labelled node, the gradient with
//                           respect to the logits of EVERY out-edge of the tile's nodes (zero where the node is not labelled),
//                           and the tile's fp64 loss sum and two counts into scratch.
//   k_graphdist_bc_reduce   per sample: the tiles' partial sums in tile order.
#include "fused_select.h"

// ---- (1) labels ------------------------------------------------------------------------------------------------------------
// The select kernels' pairs — one (row i, environment b) per lane, the environment fastest, so that the hdp loads of a wave
// are contiguous — but a lane keeps ITS environment over BC_ROWS passes of rows: the number of labelled rows is then a
// register per lane and the counter costs one atomic instruction per wave (each lane to its own environment's word), not
// one per labelled row. A workgroup takes 256 / B whole rows per pass when B < 256 (lanes beyond rows * B idle: none at
// B = 64, 61 of 256 at B = 65, at worst half), and 256 environments of one row otherwise (grid.y tiles the environments).
// Output: one byte per pair at labels[b][i], written as the select kernels write choice8 (a scattered byte).
// Must move per pair: 8 B of hdp (4 used); on occupied rows the select kernel's three 4-byte gathers; 1 B stored.
#define BC_ROWS 8
__global__ __launch_bounds__(FS_BLOCK) void k_fused_expert_labels(
    const uint2* __restrict__ hdp, const uint32_t* __restrict__ tl, const uint8_t* __restrict__ gc8,
    const float* __restrict__ slots, int64_t lds, int Nmax, const NodeRec* __restrict__ nodes,
    const int32_t* __restrict__ out_pad, const int32_t* __restrict__ a_dest, int64_t A, uint32_t B, uint32_t bt, uint32_t rows,
    int64_t N, const int32_t* __restrict__ dest_slot, const int32_t* __restrict__ next_hop, int64_t nh_bstride, int64_t D,
    uint8_t* __restrict__ labels, int32_t* __restrict__ n_labelled) {
  // bt = environments per workgroup (min(B, 256)), rows = whole rows per pass (256 / bt)
  const uint32_t w = threadIdx.x / bt, b = blockIdx.y * bt + (threadIdx.x - w * bt);
  if (w >= rows || b >= B) return;
  int32_t n_lab = 0;
  for (int k = 0; k < BC_ROWS; ++k) {
    const int64_t i = ((int64_t)blockIdx.x * BC_ROWS + k) * rows + w;
    if (i >= N) break;
    const uint32_t gid = (uint32_t)(i * B + b);                   // N * B < 2^31 (tarl_check_fused_core)
    const uint32_t hd = hdp[gid].x;
    uint32_t lab = TARL_BC_IGNORE;
    if ((hd & HD_CNT) != 0u) {                                    // an empty row: nothing else is read
      uint32_t code = SEL_RAW;
      float sv;
      if (fs_next_hop_code<false>(fs_head_agent(hd, gid, tl, gc8, slots, lds, Nmax), (uint32_t)i, b, nodes, out_pad, a_dest,
                                  A, N, dest_slot, next_hop, nh_bstride, D, &code, &sv) && code != SEL_RAW) {
        lab = code;
        ++n_lab;
      }
    }
    labels[(int64_t)b * N + i] = (uint8_t)lab;
  }
  if (n_labelled && n_lab) atomicAdd(n_labelled + b, n_lab);
}

extern "C" int tarl_fused_expert_labels(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                        int64_t num_agents, const int32_t* dest_slot, const int32_t* next_hop,
                                        int64_t nh_bstride, int64_t num_dests, uint8_t* labels, int32_t* n_labelled,
                                        tarl_stream stream) {
  TARL_REQUIRE(plan && f && dest_slot && next_hop && labels, "null argument");
  const int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(f->a_dest && num_agents >= 1, "fused agent buffers missing");
  TARL_REQUIRE(num_dests >= 0 && nh_bstride >= 0, "bad sizes");
  if (plan->N == 0) return TARL_OK;
  const int64_t bt = B < FS_BLOCK ? B : FS_BLOCK, rows = FS_BLOCK / bt;
  TARL_REQUIRE(ceil_div(B, bt) < 65536, "too many environments for one launch");
  hipLaunchKernelGGL(k_fused_expert_labels, dim3((unsigned)ceil_div(plan->N, BC_ROWS * rows), (unsigned)ceil_div(B, bt)),
                     dim3(FS_BLOCK), 0, (hipStream_t)stream, (const uint2*)f->hdp, (const uint32_t*)f->tl,
                     (const uint8_t*)f->gc8, (const float*)f->slots, f->ld_slots, (int)Nmax, (const NodeRec*)f->node_rec,
                     (const int32_t*)f->out_pad, (const int32_t*)f->a_dest, num_agents, (uint32_t)B, (uint32_t)bt,
                     (uint32_t)rows, plan->N, dest_slot, next_hop, nh_bstride, num_dests, labels, n_labelled);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- (2) cross-entropy on the labelled nodes ---------------------------------------------------------------------------------
// Grid: (tiles of BC_TILE nodes) x M samples, flattened; one lane per node walks its out-list in the plan's CSR order. On a
// source-sorted edge list (SORTED: CSR position == edge id, the builders' graphs) the logits of consecutive lanes are
// adjacent and the edge-id indirection is skipped. All fp32, k_softmax's expressions: z = l / T, mx = max z, s = sum of
// exp(z - mx) left to right, loss = log s + mx - z_label; the gradient of edge j is (grad_scale * (exp(z_j - mx) / s - [j ==
// label])) / T and 0 for every out-edge of a node that is not labelled — every edge has one source node, so every element
// of grad_logits is stored once and nothing needs to be cleared first. The tile's loss sum is taken in fp64 by a fixed tree
// (lanes l and l + 32, 16, ... of each wave, then the four waves in order); the counts are ballots. No atomics.
#define BC_TILE 256
#define BC_MAX_BLOCKS ((int64_t)1 << 24)   // (sample, tile) pairs of one launch: grid.x * BC_TILE stays below 2^32 threads
struct BcPartial {
  double nll;
  int32_t n_lab, n_hit;
};
static_assert(sizeof(BcPartial) == 16, "scratch layout of tarl_graphdist_bc");

template <bool SORTED>
__global__ __launch_bounds__(BC_TILE) void k_graphdist_bc(const int32_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_eid,
                                                          const float* __restrict__ logits, int64_t N, int64_t E,
                                                          uint32_t tiles, float temperature,
                                                          const uint8_t* __restrict__ labels, float grad_scale,
                                                          float* __restrict__ grad, BcPartial* __restrict__ part) {
  __shared__ double s_nll[BC_TILE / 64];
  __shared__ int32_t s_cnt[BC_TILE / 64][2];
  const uint32_t m = blockIdx.x / tiles, tile = blockIdx.x - m * tiles;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t n = (int64_t)tile * BC_TILE + threadIdx.x;
  const float* lb = logits + (int64_t)m * E;
  float* gb = grad ? grad + (int64_t)m * E : nullptr;
  float loss = 0.0f;
  bool labelled = false, hit = false;
  if (n < N) {
    const int32_t k0 = out_ptr[n], k1 = out_ptr[n + 1];
    const int32_t deg = k1 - k0;
    const int32_t lab = (int32_t)labels[(int64_t)m * N + n];
    labelled = lab < (deg < 0x7F ? deg : 0x7F);
    if (labelled) {
      float mx = -INFINITY;
      int32_t arg = 0;
      for (int32_t k = k0; k < k1; ++k) {
        const float z = lb[SORTED ? k : out_eid[k]] / temperature;
        if (z > mx) arg = k - k0;                                 // the FIRST maximum in CSR order
        mx = fmaxf(mx, z);
      }
      float s = 0.0f;
      for (int32_t k = k0; k < k1; ++k) s = s + expf(lb[SORTED ? k : out_eid[k]] / temperature - mx);
      loss = logf(s) + mx - lb[SORTED ? k0 + lab : out_eid[k0 + lab]] / temperature;
      hit = arg == lab;
      if (gb)
        for (int32_t k = k0; k < k1; ++k) {
          const int32_t e = SORTED ? k : out_eid[k];
          const float p = expf(lb[e] / temperature - mx) / s;
          gb[e] = (grad_scale * (p - (k - k0 == lab ? 1.0f : 0.0f))) / temperature;
        }
    } else if (gb) {
      for (int32_t k = k0; k < k1; ++k) gb[SORTED ? k : out_eid[k]] = 0.0f;
    }
  }
  double v = labelled ? (double)loss : 0.0;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int32_t c_lab = (int32_t)__popcll(__ballot(labelled)), c_hit = (int32_t)__popcll(__ballot(hit));
  if (lane == 0) {
    s_nll[wid] = v;
    s_cnt[wid][0] = c_lab;
    s_cnt[wid][1] = c_hit;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    BcPartial p = {0.0, 0, 0};
    for (int w = 0; w < BC_TILE / 64; ++w) {
      p.nll += s_nll[w];
      p.n_lab += s_cnt[w][0];
      p.n_hit += s_cnt[w][1];
    }
    part[blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(64) void k_graphdist_bc_reduce(const BcPartial* __restrict__ part, int64_t M, uint32_t tiles,
                                                            double* __restrict__ nll, int32_t* __restrict__ n_labelled,
                                                            int32_t* __restrict__ n_hit) {
  const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (m >= M) return;
  double s = 0.0;
  int32_t a = 0, h = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const BcPartial p = part[m * tiles + t];
    s += p.nll;
    a += p.n_lab;
    h += p.n_hit;
  }
  nll[m] = s;
  n_labelled[m] = a;
  n_hit[m] = h;
}

extern "C" int64_t tarl_graphdist_bc_scratch_bytes(const tarl_plan* plan, int64_t M) {
  if (!plan || M < 1) return -1;
  const int64_t tiles = ceil_div(plan->N > 0 ? plan->N : 1, BC_TILE);
  if (M * tiles >= BC_MAX_BLOCKS) return -1;
  return M * tiles * (int64_t)sizeof(BcPartial);
}

extern "C" int tarl_graphdist_bc(const tarl_plan* plan, const float* logits, int64_t M, float temperature,
                                 const uint8_t* labels, float grad_scale, double* nll, int32_t* n_labelled, int32_t* n_hit,
                                 float* grad_logits, void* scratch, tarl_stream stream) {
  TARL_REQUIRE(plan && logits && labels && nll && n_labelled && n_hit && scratch, "null argument");
  TARL_REQUIRE(M >= 1, "M must be positive");
  TARL_REQUIRE(temperature > 0.0f, "temperature must be positive");
  TARL_REQUIRE(((uintptr_t)scratch) % 8 == 0, "scratch must be 8-byte aligned");
  const int64_t tiles = ceil_div(plan->N > 0 ? plan->N : 1, BC_TILE);
  TARL_REQUIRE(M * tiles < BC_MAX_BLOCKS, "too many (sample, tile) pairs for one launch");
  hipStream_t s = (hipStream_t)stream;
  BcPartial* part = (BcPartial*)scratch;
#define BC_LAUNCH(S_)                                                                                                      \
  hipLaunchKernelGGL(k_graphdist_bc<S_>, dim3((unsigned)(M * tiles)), dim3(BC_TILE), 0, s, plan->out_ptr, plan->out_eid,   \
                     logits, plan->N, plan->E, (uint32_t)tiles, temperature, labels, grad_scale, grad_logits, part)
  if (plan->src_sorted)
    BC_LAUNCH(true);
  else
    BC_LAUNCH(false);
#undef BC_LAUNCH
  TARL_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_graphdist_bc_reduce, dim3((unsigned)ceil_div(M, 64)), dim3(64), 0, s, part, M, (uint32_t)tiles, nll,
                     n_labelled, n_hit);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
