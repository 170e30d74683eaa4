// fused_pack.hip — the packed state's way in and out: pack / reset / export kernels, the pointer table, the argument checks
// shared by the entry points, and the rollout-bytes gather of the PPO update. (Design and layout: fused_frame.h.)
#include "fused_frame.h"

// ---- pack: build the dense / static words, the slot store and the agent SoA from x / agent_features -------------------
__global__ __launch_bounds__(FB) void k_pack_nodes(const float* __restrict__ x, Layout L, int64_t B, int64_t N,
                                                   const float* __restrict__ cong, FusedBufs fb, float4* st0_out,
                                                   PlanOut P) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;  // gid = i * B + b  (env-minor)
  if (gid >= B * N) return;
  const int64_t i = gid / B;
  const int64_t b = gid - i * B;
  const float* xi = x + b * L.bstride + i * L.ldx;
  const int Nmax = L.Nmax;
  const float n = xi[L.col_n()];
  const int q = (int)n;
  const float tail = (q >= 1 && q <= Nmax) ? xi[q - 1] : 0.0f;
  const float head = xi[0];
  if (q < 0 || q > 127 || !(head >= 0.0f && head < 16777216.0f) || !(tail >= 0.0f && tail < 16777216.0f))
    atomicOr(fb.flags, FLAG_PACK_RANGE);
  // HD_DIRTY: a non-zero dead slot (at or above the count: no garbage is pending after a pack), or a FIFO that has reached
  // its last slot
  bool dirty = q >= Nmax - 1;
  for (int sidx = q < 0 ? 0 : q; sidx < Nmax; ++sidx)
    dirty = dirty || xi[sidx] != 0.0f || xi[Nmax + sidx] != 0.0f || xi[2 * Nmax + sidx] != 0.0f;
  fb.hdp[gid] = make_uint2(((uint32_t)head << 8) | (uint32_t)(q & (int)HD_CNT) | (dirty ? HD_DIRTY : 0u), __float_as_uint(xi[2 * Nmax]));
  fb.tl[gid] = tl_word((uint32_t)tail, 0, TLF_AUTH);
  fb.gc8[gid] = (uint8_t)r1_code(-1);
  fb.post[gid] = ((uint32_t)tail << 8) | (q > 0 ? PF_NONEMPTY : 0u);
  // SELECTED_ROAD: the rank of the out-edge it names, or the raw value when it names none of them
  const float sv = xi[L.col_sel()];
  fb.sel[gid] = sv;
  uint32_t code = SEL_RAW;
  const int32_t k0 = P.out_ptr[i], k1 = P.out_ptr[i + 1];
  for (int32_t k = k1 - 1; k >= k0; --k)
    if ((float)P.out_dst[k] == sv && k - k0 < (int32_t)SEL_RAW) code = (uint32_t)(k - k0);
  fb.sel8[gid] = (uint8_t)code;
  if (i == 0) {
    for (int64_t sl_ = 0; sl_ < fb.acc_slots; ++sl_) {
      fb.acc_lp[sl_ * B + b] = 0;
      fb.acc_n[sl_ * B + b] = 0.0f;
      fb.acc_w[sl_ * B + b] = 0.0f;
    }
  }
  float* sl = fb.slots + gid * fb.lds;
  for (int sidx = 0; sidx < Nmax; ++sidx) slot_store(sl + SLW * sidx, xi[sidx], xi[Nmax + sidx], xi[2 * Nmax + sidx]);
  if (b == 0 && st0_out) {
    const float maxn = xi[L.col_maxn()], ff = xi[L.col_ff()];
    float c;
    if (cong) {
      c = cong[i];
    } else {
      const float critical = xi[L.col_maxflow()] * ff / 3600.0f;
      c = ff * (maxn + 10.0f - critical);
    }
    st0_out[i] = make_float4(maxn, ff, xi[L.col_road()], c);
  }
}

// Static records (fused_common.h). in_rec[k].rank for in-edge k = (j -> i): the rank r of j's out-edges with
// (float)out_dst == ROAD_INDEX(i), i.e. the sel8 code of j that makes "SELECTED_ROAD(j) == ROAD_INDEX(i)"
// (src/direction_mpnn.py:77-79) true; INRANK_NONE when no out-edge of j does. Two matching out-edges (parallel dual
// edges) have no unique rank: FLAG_AMBIGUOUS_EDGES. Runs after k_pack_nodes (reads st0).
__global__ __launch_bounds__(FB) void k_pack_static(int64_t N, int64_t E, const int32_t* __restrict__ in_ptr,
                                                    const int32_t* __restrict__ in_src,
                                                    const int32_t* __restrict__ in_eid, PlanOut P,
                                                    const float* __restrict__ edge_attr,
                                                    const float4* __restrict__ st0, NodeRec* nodes, InRec* in_rec,
                                                    int32_t* out_pad, int32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (i < 4) {   // padding entries: any valid row, never used
    in_rec[E + i] = InRec{0, (int32_t)INRANK_NONE, 0.0f, 0.0f, 0};
    out_pad[E + i] = 0;
  }
  if (i >= N) return;
  const float4 sti = st0[i];
  const int32_t a0 = in_ptr[i], a1 = in_ptr[i + 1], o0 = P.out_ptr[i], o1 = P.out_ptr[i + 1];
  NodeRec nr{a0, a1 - a0, o0, o1 - o0, sti.x, sti.y, sti.z, sti.w, entry_tt(sti, 0.0f), {0, 0, 0}, {0, 0, 0, 0}, {}};
  for (int q = 0; q < 4; ++q) {
    nr.out4[q] = q < o1 - o0 ? P.out_dst[o0 + q] : (int32_t)i;
    nr.in4[q] = InRec{0, (int32_t)INRANK_NONE, 0.0f, 0.0f, 0};
  }
  for (int32_t k = o0; k < o1; ++k) out_pad[k] = P.out_dst[k];
  for (int32_t k = a0; k < a1; ++k) {
    const int32_t j = in_src[k];
    const int32_t k0 = P.out_ptr[j], k1 = P.out_ptr[j + 1];
    int cnt = 0, r = (int)INRANK_NONE;
    for (int32_t kk = k0; kk < k1; ++kk)
      if ((float)P.out_dst[kk] == sti.z) {
        if (cnt == 0) r = kk - k0;
        ++cnt;
      }
    if (cnt > 1 || (cnt == 1 && r >= (int)SEL_RAW)) {
      atomicOr(flags, FLAG_AMBIGUOUS_EDGES);
      r = (int)INRANK_NONE;
    }
    in_rec[k] = InRec{j, r, edge_attr ? edge_attr[in_eid[k]] : 0.0f, st0[j].x, in_eid[k]};
    if (k - a0 < 4) nr.in4[k - a0] = in_rec[k];
  }
  nodes[i] = nr;
}

__global__ __launch_bounds__(FB) void k_pack_agents(const float* __restrict__ ag, int64_t B, int64_t A,
                                                    int64_t a_bstride, FusedBufs fb) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (gid >= B * A) return;
  const int64_t b = gid / A, a = gid - b * A;
  const float* row = ag + b * a_bstride + a * AG_COLS;
  fb.a_origin[gid] = (int32_t)(long long)row[AG_ORIGIN];
  fb.a_dest[gid] = (int32_t)(long long)row[AG_DEST];
  fb.a_dep[gid] = row[AG_DEP];
  fb.a_status[gid] = row[AG_DONE] != 0.0f ? 2 : (row[AG_ON_WAY] != 0.0f ? 1 : 0);
  if (a == 0 && fb.cur_lo) fb.cur_lo[b] = 0;
}

// departure-ordered window records of the insert kernel (after k_pack_agents)
__global__ __launch_bounds__(FB) void k_pack_window(int64_t B, int64_t A, FusedBufs fb, uint4* __restrict__ a_win) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;   // gid = b * A + k (sorted position k)
  if (gid >= B * A) return;
  const int64_t b = gid / A;
  const int32_t a = fb.a_order[gid];
  a_win[gid] = make_uint4(__float_as_uint(fb.a_dep_sorted[gid]), (uint32_t)fb.a_origin[b * A + a], (uint32_t)a, 0u);
  fb.a_ins[gid] = fb.a_status[b * A + a] != 0 ? 1 : 0;
}

// ---- reset: SimulatorEnv._reset on the packed state (zero FIFOs and counters, clear ON_WAY / DONE, re-arm cursors) -------
__global__ __launch_bounds__(FB) void k_fused_reset_nodes(int64_t B, int64_t N, FusedBufs fb) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (gid >= B * N) return;
  fb.hdp[gid] = make_uint2(0u, 0u);
  fb.tl[gid] = TLF_AUTH;
  fb.gc8[gid] = (uint8_t)r1_code(-1);
  fb.post[gid] = 0u;
  if (gid < B) {
    for (int64_t sl_ = 0; sl_ < fb.acc_slots; ++sl_) {
      fb.acc_lp[sl_ * B + gid] = 0;
      fb.acc_n[sl_ * B + gid] = 0.0f;
      fb.acc_w[sl_ * B + gid] = 0.0f;
    }
    if (fb.cur_lo) fb.cur_lo[gid] = 0;
  }
}

__global__ __launch_bounds__(FB) void k_fused_reset_agents(float* __restrict__ ag, int64_t B, int64_t A,
                                                           int64_t a_bstride, FusedBufs fb) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (gid >= B * A) return;
  // only agents that left the "waiting" state have flags to clear (the status SoA mirrors ON_WAY / DONE since the last
  // pack): a sequential 1-byte scan instead of two scattered stores into every 36-byte row
  if (fb.a_status[gid] == 0) return;
  const int64_t b = gid / A, a = gid - b * A;
  float* row = ag + b * a_bstride + a * AG_COLS;
  row[AG_ON_WAY] = 0.0f;
  row[AG_DONE] = 0.0f;
  fb.a_status[gid] = 0;
  if (fb.a_ins) fb.a_ins[b * A + fb.a_rank[gid]] = 0;
}

// ---- export: rebuild the reference's x layout (three FIFO column blocks + NUMBER_OF_AGENT + SELECTED_ROAD) ----------
__global__ __launch_bounds__(FB) void k_export_rows(float* __restrict__ x, Layout L, int64_t B, int64_t N, FusedBufs fb,
                                                    float t_last, PlanOut P) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;
  const int Nmax = L.Nmax;
  if (gid >= B * N * Nmax) return;
  const int64_t row = gid / Nmax;  // row = i * B + b
  const int sidx = (int)(gid - row * Nmax);
  const int64_t i = row / B, b = row - i * B;
  float* xi = x + b * L.bstride + i * L.ldx;
  const uint32_t hd = fb.hdp[row].x;
  const uint32_t code = fb.gc8[row];
  const int n = (int)(hd & HD_CNT);
  const uint32_t tlw = fb.tl[row];
  const int g = pending_g(tlw, n, code, Nmax);
  const float* sl = fb.slots + row * fb.lds + SLW * phys(tl_hoff(tlw), sidx, Nmax);  // un-rotate the ring buffer
  if (g >= 0 && sidx == n) {  // pending garbage write of the last Direction update -> first dead slot
    const float tt = entry_tt(fb.st0[i], (float)g);
    xi[sidx] = 0.0f;
    xi[Nmax + sidx] = t_last;
    xi[2 * Nmax + sidx] = t_last + tt;
  } else if (!(hd & HD_DIRTY) && sidx >= n) {  // clean row: its dead slots are zero, whatever the store still holds there
    xi[sidx] = 0.0f;
    xi[Nmax + sidx] = 0.0f;
    xi[2 * Nmax + sidx] = 0.0f;
  } else {
    xi[sidx] = sl[0];
    xi[Nmax + sidx] = sl[1];
    xi[2 * Nmax + sidx] = sl[2];
  }
  if (sidx == 0) {
    xi[L.col_n()] = (float)n;
    const float sv = sel_value(fb, P.out_ptr, P.out_dst, i, row);
    xi[L.col_sel()] = sv;
    fb.sel[row] = sv;
  }
}

// ---- clean rows <-> exact slot store (hand-over to / from code that maintains every dead slot physically) ------------------
// tarl_fused_dead_slots(materialise = 1): write the zeros a clean row's dead slots stand for into the store (the slot at the
// count only when no garbage is pending there): afterwards the store is exact for every row. (materialise = 0): set each
// row's HD_DIRTY from the store — a non-zero dead slot, or a FIFO at its last slot — as pack does from x. The LDS-resident
// rollout kernel (rollout_env.hip), which keeps the reference's slot-by-slot bookkeeping, runs between the two.
__global__ __launch_bounds__(FB) void k_dead_slots(int64_t B, int64_t N, int Nmax, FusedBufs fb, int materialise) {
  const int64_t row = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (row >= B * N) return;
  const uint32_t hd = fb.hdp[row].x, tlw = fb.tl[row];
  const int n = (int)(hd & HD_CNT), hoff = tl_hoff(tlw);
  const int g = pending_g(tlw, n, fb.gc8[row], Nmax);
  float* sl = fb.slots + row * fb.lds;
  const int first = (g >= 0) ? n + 1 : n;       // the slot at the count holds the pending garbage (never stored) or is dead
  if (materialise) {
    if (hd & HD_DIRTY) return;
    for (int sidx = first; sidx < Nmax; ++sidx) {
      slot_store(sl + SLW * phys(hoff, sidx, Nmax), 0.0f, 0.0f, 0.0f);
    }
  } else {
    bool dirty = n >= Nmax - 1;
    for (int sidx = first; sidx < Nmax; ++sidx) {
      const float* z = sl + SLW * phys(hoff, sidx, Nmax);
      dirty = dirty || z[0] != 0.0f || z[1] != 0.0f || z[2] != 0.0f;
    }
    fb.hdp[row].x = (hd & ~HD_DIRTY) | (dirty ? HD_DIRTY : 0u);
  }
}

int tarl_fused_dead_slots(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int materialise,
                          tarl_stream stream) {
  if (plan->N == 0) return TARL_OK;
  hipLaunchKernelGGL(k_dead_slots, dim3((unsigned)ceil_div(B * plan->N, FB)), dim3(FB), 0, (hipStream_t)stream, B, plan->N,
                     (int)Nmax, tarl_to_bufs(f), materialise);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- the pointer table ---------------------------------------------------------------------------------------------------
FusedBufs tarl_to_bufs(const tarl_fused* f) {
  return FusedBufs{(uint2*)f->hdp,        (uint32_t*)f->tl, f->gc8,          (uint32_t*)f->post, (const float4*)f->st0,
                   f->slots,              f->ld_slots,      f->sel8,         f->sel,             (const NodeRec*)f->node_rec,
                   (const InRec*)f->in_rec, f->out_pad,
                   (long long*)f->acc_lp, f->acc_n,         f->acc_w,        f->a_origin,        f->a_dest,
                   f->a_dep,              f->a_status,      f->a_order,      f->cur_lo,          f->a_dep_sorted,
                   (const uint4*)f->a_win, f->a_ins,        f->a_rank,
                   f->acc_slots,          f->flags,         f->env_base};
}

// The device-resident copies of the pointer table (tarl_fused.bufs_dev): slot 0 = the table as the caller gave it, slot 1 =
// the same with the second log-prob accumulator bank (the merged insert + choice launch double-buffers it by frame parity).
// One thread, the tables by value in its kernel arguments: stream-ordered, no host copy, no synchronisation.
__global__ void k_set_bufs(FusedBufs a, FusedBufs b, FusedBufs* __restrict__ dst) {
  dst[0] = a;
  dst[1] = b;
}
extern "C" int64_t tarl_fused_bufs_bytes(void) { return 2 * (int64_t)sizeof(FusedBufs); }
int tarl_upload_bufs(const tarl_fused* f, const FusedBufs& fb, long long* acc_lp_alt, hipStream_t s, const FusedBufs** dev) {
  TARL_REQUIRE(f->bufs_dev && ((uintptr_t)f->bufs_dev) % 16 == 0, "tarl_fused.bufs_dev missing or misaligned (tarl_fused_bufs_bytes)");
  FusedBufs alt = fb;
  if (acc_lp_alt) alt.acc_lp = acc_lp_alt;
  hipLaunchKernelGGL(k_set_bufs, dim3(1), dim3(1), 0, s, fb, alt, (FusedBufs*)f->bufs_dev);
  TARL_LAUNCH_CHECK();
  *dev = (const FusedBufs*)f->bufs_dev;
  return TARL_OK;
}

int tarl_check_fused_core(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax) {
  TARL_REQUIRE(plan && f, "null argument");
  TARL_REQUIRE(f->hdp && f->tl && f->gc8 && f->post && f->st0 && f->slots && f->sel8 && f->sel && f->acc_lp &&
                   f->acc_n && f->acc_w && f->flags && f->node_rec && f->in_rec && f->out_pad,
               "fused node buffers missing");
  TARL_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && Nmax >= 2, "bad sizes");
  TARL_REQUIRE(plan->N * B < ((int64_t)1 << 31), "N * B must stay below 2^31 (32-bit row indices in the frame kernels)");
  TARL_REQUIRE(Nmax <= 127, "the fused path packs NUMBER_OF_AGENT into one byte and the ring offset into seven bits: "
                            "Nmax must be <= 127 (use the unfused entry points for longer FIFOs)");
  TARL_REQUIRE(plan->max_out <= 126, "the fused path packs the chosen out-edge's rank into 7 bits: out-degree must be <= 126");
  TARL_REQUIRE(f->acc_slots >= 1 && f->acc_slots <= 4096, "acc_slots out of range");
  TARL_REQUIRE(f->ld_slots >= SLW * (int64_t)Nmax && f->ld_slots % SLW_ALIGN == 0, "slot row stride smaller than SLW*Nmax or misaligned (tarl_fused_slot_floats)");
  TARL_REQUIRE(num_chunks(plan) < 65536 && plan->num_row_chunks < 65536 && ceil_div(plan->N, nchunk_choice()) < 65536 &&
                   ceil_div(plan->N, nchunk_dir()) < 65536,
               "too many node chunks for one launch");
  TARL_REQUIRE(((uintptr_t)f->hdp | (uintptr_t)f->st0 | (uintptr_t)f->slots) % 32 == 0 &&
                   ((uintptr_t)f->tl | (uintptr_t)f->post) % 4 == 0,
               "fused records must be 16-byte aligned");
  return TARL_OK;
}

static int check_fused(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t bstride,
                       int64_t ldx, int32_t Nmax) {
  int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc) return rc;
  TARL_REQUIRE(x != nullptr, "x is null");
  TARL_REQUIRE(ldx >= 3 * (int64_t)Nmax + 7, "row stride smaller than F");
  TARL_REQUIRE(B == 1 || bstride >= plan->N * ldx, "environment stride smaller than one environment");
  return TARL_OK;
}

extern "C" int64_t tarl_fused_slot_floats(int32_t Nmax) {
  return SLW == 8 ? (int64_t)8 * Nmax : ((int64_t)SLW * Nmax + 15) / 16 * 16;   // 12-byte slots: rows padded to 64 bytes
}

extern "C" int tarl_fused_pack(const tarl_plan* plan, const tarl_fused* f, const float* x, int64_t B, int64_t x_bstride,
                               int64_t ldx, int32_t Nmax, const float* cong, const float* edge_attr,
                               const float* agent_features, int64_t A, int64_t a_bstride, tarl_stream stream) {
  int rc = check_fused(plan, f, x, B, x_bstride, ldx, Nmax);
  if (rc) return rc;
  TARL_REQUIRE(plan->E == 0 || edge_attr, "edge_attr is null");
  const Layout L{Nmax, ldx, x_bstride};
  const FusedBufs fb = tarl_to_bufs(f);
  const PlanOut P{plan->out_ptr, plan->out_dst};
  hipStream_t s = (hipStream_t)stream;
  TARL_CHECK_HIP(hipMemsetAsync(f->flags, 0, sizeof(int32_t), s));
  if (plan->N > 0) {
    hipLaunchKernelGGL(k_pack_nodes, dim3((unsigned)ceil_div(B * plan->N, FB)), dim3(FB), 0, s, x, L, B, plan->N, cong,
                       fb, (float4*)f->st0, P);
    TARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_static, dim3((unsigned)ceil_div(plan->N > 4 ? plan->N : 4, FB)), dim3(FB), 0, s, plan->N,
                       plan->E, plan->in_ptr, plan->in_src, plan->in_eid, P, edge_attr, (const float4*)f->st0,
                       (NodeRec*)f->node_rec, (InRec*)f->in_rec, f->out_pad, f->flags);
    TARL_LAUNCH_CHECK();
  }
  if (agent_features) {
    TARL_REQUIRE(f->a_origin && f->a_dest && f->a_dep && f->a_status && A >= 1, "fused agent buffers missing");
    TARL_REQUIRE(A <= ((int64_t)1 << 24), "agent ids must stay below 2^24 (they are exact fp32 integers in the reference)");
    hipLaunchKernelGGL(k_pack_agents, dim3((unsigned)ceil_div(B * A, FB)), dim3(FB), 0, s, agent_features, B, A,
                       a_bstride, fb);
    TARL_LAUNCH_CHECK();
    if (f->a_order && f->a_win) {
      TARL_REQUIRE(f->a_ins && f->a_rank && f->a_dep_sorted, "a_win needs a_ins, a_rank and a_dep_sorted");
      hipLaunchKernelGGL(k_pack_window, dim3((unsigned)ceil_div(B * A, FB)), dim3(FB), 0, s, B, A, fb, (uint4*)f->a_win);
      TARL_LAUNCH_CHECK();
    }
  }
  return TARL_OK;
}

extern "C" int tarl_fused_reset(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax,
                                float* agent_features, int64_t A, int64_t a_bstride, tarl_stream stream) {
  int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc) return rc;
  TARL_REQUIRE(agent_features && A >= 1 && f->a_status, "agents missing");
  const FusedBufs fb = tarl_to_bufs(f);
  hipStream_t s = (hipStream_t)stream;
  // The slot store is NOT zeroed: after the reset every row is empty and CLEAN (count byte 0), and a clean row's dead slots
  // are zero by rule whatever the store holds (fused_common.h) — export, head_arrival and tarl_fused_dead_slots apply the
  // rule, the frame kernels never read a clean row's dead slot. (The memset was 1.5 ms of every PPO iteration at 16 384
  // environments with 12-byte slots; with 32-byte records it would be 4 ms.)
  if (plan->N > 0) {
    hipLaunchKernelGGL(k_fused_reset_nodes, dim3((unsigned)ceil_div(B * plan->N, FB)), dim3(FB), 0, s, B, plan->N, fb);
    TARL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_fused_reset_agents, dim3((unsigned)ceil_div(B * A, FB)), dim3(FB), 0, s, agent_features, B, A,
                     a_bstride, fb);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

extern "C" int tarl_fused_export(const tarl_plan* plan, const tarl_fused* f, float* x, int64_t B, int64_t x_bstride,
                                 int64_t ldx, int32_t Nmax, float last_step_time, tarl_stream stream) {
  int rc = check_fused(plan, f, x, B, x_bstride, ldx, Nmax);
  if (rc) return rc;
  if (plan->N == 0) return TARL_OK;
  const Layout L{Nmax, ldx, x_bstride};
  const PlanOut P{plan->out_ptr, plan->out_dst};
  hipLaunchKernelGGL(k_export_rows, dim3((unsigned)ceil_div(B * plan->N * Nmax, FB)), dim3(FB), 0, (hipStream_t)stream,
                     x, L, B, plan->N, tarl_to_bufs(f), last_step_time, P);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

int tarl_check_frame_args(const tarl_plan* plan, const tarl_fused* f, int64_t B, const float* agent_features, int64_t A,
                          int64_t a_bstride, const int32_t* ins_scratch, const float* edge_attr, const float* log_edge_attr) {
  TARL_REQUIRE(agent_features && A >= 1 && ins_scratch, "agents / scratch missing");
  TARL_REQUIRE(f->a_origin && f->a_dest && f->a_dep && f->a_status, "fused agent buffers missing");
  TARL_REQUIRE(f->a_order == nullptr || (f->cur_lo != nullptr && f->a_dep_sorted != nullptr),
               "a_order needs cur_lo and a_dep_sorted");
  TARL_REQUIRE(B == 1 || a_bstride >= A * AG_COLS, "agent stride smaller than one population");
  TARL_REQUIRE(plan->E == 0 || (edge_attr && log_edge_attr), "edge constants missing");
  return TARL_OK;
}

// ---- rollout bytes -> the formats of the unfused entry points (minibatch gather of the PPO update) ------------------------
__global__ __launch_bounds__(FB) void k_rollout_gather(const uint8_t* __restrict__ choice, const uint8_t* __restrict__ counts,
                                                       int64_t B, int64_t N, int env_minor,
                                                       const int64_t* __restrict__ idx, int64_t rows,
                                                       const int32_t* __restrict__ out_ptr,
                                                       const int32_t* __restrict__ out_eid,
                                                       int32_t* __restrict__ choice_eid, float* __restrict__ counts_f) {
  const int64_t gid = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (gid >= rows * N) return;
  const int64_t r = gid / N, i = gid - r * N;
  const int64_t tb = idx ? idx[r] : r;
  const int64_t t = tb / B, b = tb - t * B;
  const int64_t src = env_minor ? ((t * N + i) * B + b) : ((t * B + b) * N + i);
  if (choice_eid) {
    const uint32_t c = choice[src];
    choice_eid[gid] = (c & SEL_CARRIED) ? -1 : out_eid[out_ptr[i] + (int32_t)c];
  }
  if (counts_f) counts_f[gid] = (float)counts[src];
}

extern "C" int tarl_rollout_gather(const tarl_plan* plan, const uint8_t* choice, const uint8_t* counts, int64_t T,
                                   int64_t B, int env_minor, const int64_t* idx, int64_t rows, int32_t* choice_eid,
                                   float* counts_f, tarl_stream stream) {
  TARL_REQUIRE(plan && T >= 1 && B >= 1 && rows >= 0, "bad arguments");
  TARL_REQUIRE((choice != nullptr) == (choice_eid != nullptr) && (counts != nullptr) == (counts_f != nullptr),
               "each output needs its input");
  TARL_REQUIRE(idx || rows == T * B, "without an index list all T * B rows are converted");
  if (rows == 0 || plan->N == 0) return TARL_OK;
  hipLaunchKernelGGL(k_rollout_gather, dim3((unsigned)ceil_div(rows * plan->N, FB)), dim3(FB), 0, (hipStream_t)stream,
                     choice, counts, B, plan->N, env_minor, idx, rows, plan->out_ptr, plan->out_eid, choice_eid, counts_f);
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}
