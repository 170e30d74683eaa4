// fused_select.h — what the SELECTED_ROAD writers on the PACKED state share: k_fused_select_next_hop_dest (baseline.hip, the
// next hop from a per-destination table) and k_fused_select_route (routes.hip, the next hop from a per-agent route). Both
// run one thread per (row i, environment b), flat index gid = i * B + b with the environment fastest, decode the row's head
// agent the same way and turn the value they select into the same rank byte. k_fused_hold_policy_actions (policy_hold.hip),
// the hold rule as a post-pass over a policy's bytes, has the same launch shape and block size but reads no head through
// fs_head_agent: it never touches an empty row.
#pragma once
#include "fused_common.h"

#define FS_BLOCK 256

// The head agent of packed row gid whose hdp word is hd. k_select_next_hop_dest's rule, word for word: an empty FIFO reads
// agent 0 — x[i][0] of an empty row is 0 (the pending garbage triple, or a clean row's dead slot) unless the row is DIRTY
// with no garbage pending, where it is whatever the slot store holds at the ring offset (k_export_rows).
__device__ __forceinline__ long long fs_head_agent(uint32_t hd, uint32_t gid, const uint32_t* __restrict__ tl,
                                                   const uint8_t* __restrict__ gc8, const float* __restrict__ slots,
                                                   int64_t lds, int Nmax) {
  long long head = (long long)(hd >> 8);
  if ((hd & HD_CNT) == 0u) {
    head = 0;
    if (hd & HD_DIRTY) {
      const uint32_t tlw = tl[gid];
      if (pending_g(tlw, 0, (uint32_t)gc8[gid], Nmax) < 0) head = (long long)slots[(int64_t)gid * lds + SLW * tl_hoff(tlw)];
    }
  }
  return head;
}

// The code of the value sv in row i's SELECTED_ROAD byte: the rank of the first out-edge of i whose target converts to that
// value (k_pack_nodes' rule), else SEL_RAW (the value then goes into `sel`): the row itself, -1, an entry no out-edge matches.
__device__ __forceinline__ uint32_t fs_rank_code(const NodeRec& nr, const int32_t* __restrict__ out_pad, float sv) {
  uint32_t code = SEL_RAW;
  const int32_t deg = nr.out_deg;
#pragma unroll
  for (int q = 3; q >= 0; --q)
    if (q < deg && (float)nr.out4[q] == sv) code = (uint32_t)q;
  if (code == SEL_RAW && deg > 4) {
    const int32_t* od = out_pad + nr.out0;
    for (int32_t q = 4; q < deg && q < (int32_t)SEL_RAW; ++q)
      if ((float)od[q] == sv) {
        code = (uint32_t)q;
        break;
      }
  }
  return code;
}

// The next-hop lookup of k_fused_select_next_hop_dest for head agent `head` of row i in environment b, shared with
// k_fused_expert_labels (bc.hip), which wants the byte and no store. false: a head, destination or table slot out of range —
// the select kernel leaves such a row untouched. true: *sv = the value it writes ((float) next hop; with HOLD the row's own
// id where the next hop is the destination, compared on the integers) and *code = that value's rank byte (fs_rank_code).
template <bool HOLD>
__device__ __forceinline__ bool fs_next_hop_code(long long head, uint32_t i, uint32_t b, const NodeRec* __restrict__ nodes,
                                                 const int32_t* __restrict__ out_pad, const int32_t* __restrict__ a_dest,
                                                 int64_t A, int64_t N, const int32_t* __restrict__ dest_slot,
                                                 const int32_t* __restrict__ next_hop, int64_t nh_bstride, int64_t D,
                                                 uint32_t* code, float* sv) {
  if (head < 0 || head >= A) return false;
  const int32_t dest = a_dest[(int64_t)b * A + head];
  if (dest < 0 || dest >= N) return false;
  const int32_t slot = dest_slot[dest];
  if (slot < 0 || slot >= D) return false;
  int32_t nh = next_hop[(int64_t)b * nh_bstride + (int64_t)slot * N + i];
  if (HOLD && nh == dest) nh = (int32_t)i;
  *sv = (float)nh;
  *code = fs_rank_code(nodes[i], out_pad, *sv);
  return true;
}
