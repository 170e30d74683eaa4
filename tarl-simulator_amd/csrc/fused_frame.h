// fused_frame.h — internal header of the fused_*.hip files: the vectorised rollout frame in 3-4 launches, bit-identical
// (state, agents, actions, rewards) to the unfused kernels and therefore to the reference. One file per kernel family:
// fused_pack.hip (pack / reset / export), fused_choice.hip (action draw), fused_direction.hip, fused_rows.hip,
// fused_insert.hip (the three frame kernels, each with its launch dispatch) and fused_rollout.hip (the host loops).
//
// Why: the reference's AoS row (F = 3*Nmax+7 floats, 208 B at Nmax = 15) scatters the ~10 scalars a message needs over
// 2-3 cache lines, and eleven separate launches per frame each re-stream the whole state. Here
//   * ENV-MINOR LAYOUT: every per-(node, env) array is stored [node][env]. A workgroup owns a tile of consecutive
//     environments (one per lane) and walks a chunk of nodes: all topology / table / static loads are wave-uniform
//     (scalar loads through the constant cache) and every record gather is fully coalesced — there is no dependent
//     index -> address -> data chain left in the vector memory path;
//   * DENSE WORDS (fused_common.h): what every row reads and rewrites every frame is 12 bytes — hdp = {head_id << 8 | n,
//     head_dep} and tl = tail_id << 8 | flags — plus a per-node STATIC record st0 = {maxn, ff, road_index, cong} shared by
//     all environments. The Direction gather reads 8 B (+ 1 B of SELECTED_ROAD) per neighbour and never touches the FIFOs;
//   * the Direction gather emits ONE post word per row (tail' << 8 | non-empty' | arrived): the state the row will have
//     after the Direction update. The enqueued agent, the new count and the Response "accepted" test (tail of the
//     downstream row == my head, both non-empty) all follow from it — no second pass over the FIFOs, no extra arrays;
//   * SELECTED_ROAD and the action are the same byte: the rank of the chosen out-edge in the node's CSR list (sel8). In a
//     rollout the action buffer's slice of frame t IS the SELECTED_ROAD column the Direction gather of frame t reads;
//   * the live policy's sample is state-independent (see k_policy_tables): the choice phase is a table walk per
//     (node, env) with Philox blocks shared across consecutive nodes;
//   * ONE row pass applies Direction update + Response pop + withdraw. A row where nothing moves (nobody enqueued, no pop,
//     head not due) touches nothing but its dense words; the EVENT-ONLY byte gc8 (pending-garbage count) and the FIFO
//     store are written only by the rows that move something (the head's arrival time is never stored beside the dense
//     words: it is the arrival field of the head's slot record, fused_common.h: head_arrival);
//   * the FIFO contents live in a slot-interleaved store  slots[node][env][s] = {id, arrival, departure}: the Direction
//     update's per-row write is ONE 12-byte store instead of three dwords in three DRAM sectors (+ counter). (32-byte
//     records — a store then fills its sector, no read-modify-write at the memory side — were measured in round 4 and
//     rejected: fused_common.h, TARL_SLW);
//   * LAZY GARBAGE SLOT: a row that receives nobody still gets (0, t, t + tt) written into its first dead slot by the
//     reference. That value is never read by the simulation, is overwritten by the next frame's update (or
//     by an insertion) before anything can move it, and only shows in x. It is never stored: for a row that was idle in
//     the last frame the count at the write is its count, otherwise gc8 holds it (TLF_AUTH), and the export kernel
//     materialises the triple (same fp32 expression, same slot). The one case where the pop's "last slot keeps its value"
//     rule would duplicate it (count == Nmax-1) is written eagerly;
//   * RING-BUFFER FIFOs: the reference pops by shifting all Nmax slots (and withdraws with a zero-filled shift). Here a
//     per-row head offset makes the pop one triple copy (the slot that falls off the front receives the old last slot,
//     which is exactly the reference's "last slot keeps its value") and a withdraw of c agents c zero-writes; the dead
//     slots end up with exactly the reference's contents and tarl_fused_export un-rotates;
//   * agent bookkeeping scans a 1-byte status + 4-byte departure SoA instead of 36-B AoS rows.
// The packed state is authoritative between tarl_fused_pack and tarl_fused_export; the exported x and agent_features are
// bit-identical to what the unfused kernels (and the reference) produce after every frame (tests/test_gpu_fused.py).
//
// Domain: the plan is built on the same node set as x (plan nodes == rows of x): pure road graphs and MATSim graphs
// with SRC/DEST pseudo-nodes alike. Nmax <= 127, out-degree <= 126, agent ids < 2^24 (checked). A count that reaches Nmax
// leaves the reference's defined domain (it raises IndexError one or two steps later): the kernels set
// FLAG_COUNT_AT_NMAX in the device status word and the host raises when it reads it.
#pragma once
#include <type_traits>

#include "fused_common.h"

struct PlanOut {   // CSR by source
  const int32_t* out_ptr;
  const int32_t* out_dst;
};

// element idx of a [node][env] array. O32: through a 32-bit BYTE offset from the (scalar) base — `global_load ... v_off,
// s[base]` instead of a 64-bit address per lane (one to two vector instructions fewer per access; row pass 212 -> 204 us).
// Valid while N * B * sizeof(T) < 2^32, i.e. N * B < 2^29 for the 8-byte words: launch_rows picks the instantiation.
template <bool O32, class T>
__device__ __forceinline__ T& at32(T* base, uint32_t idx) {
  if (O32) return *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (size_t)(idx * (uint32_t)sizeof(T)));
  return base[idx];
}
template <bool O32, class T>
__device__ __forceinline__ const T& at32(const T* base, uint32_t idx) {
  if (O32) return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)(idx * (uint32_t)sizeof(T)));
  return base[idx];
}

// What is reached through the pointer table (FusedBufs in device memory, tarl_fused.bufs_dev). A pointer that was loaded from
// memory carries no address space: an access through it is compiled as FLAT — no scalar-base form (the O32 addressing above
// is lost on exactly these arrays), counted on vmcnt AND lgkmcnt, and free to return out of order, so the compiler waits
// with a zero count while one is in flight. glob(p) names the element p points at as GLOBAL memory (loads, stores, the two
// atomics the frame kernels use), gat<O32>(base, idx) is at32<> in that address space, gbase(base) the array's base for plain
// indexing of scalar element types (slot records: slot_load / slot_store take either kind of pointer).
#define TARL_GLOBAL __attribute__((address_space(1)))
template <int BYTES> struct GWord;
template <> struct GWord<1> { typedef uint8_t type; };
template <> struct GWord<4> { typedef uint32_t type; };
template <> struct GWord<8> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct GWord<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
// GRef<T>: the proxy the three functions return (T const-qualified when the table's pointer is). It converts to T (a load) and
// takes a T (a store: a compile error through a pointer to const). It is no value: `auto v = glob(p)` keeps the proxy —
// write `T v = glob(p)` or glob(p).load() — and a proxy assigned to a proxy does not compile (say .load() on the right).
template <class T>
struct GRef {   // T as one machine word of its size: the HIP vector classes have no members for another address space
  typedef typename std::remove_const<T>::type V;
  typedef typename GWord<sizeof(T)>::type W;
  W TARL_GLOBAL* p;
  __device__ __forceinline__ V load() const { return __builtin_bit_cast(V, *p); }
  __device__ __forceinline__ operator V() const { return load(); }
  __device__ __forceinline__ void operator=(const V& v) const {
    static_assert(!std::is_const<T>::value, "store through a pointer to const");
    *p = __builtin_bit_cast(W, v);
  }
  void operator=(const GRef&) const = delete;
  // atomicAdd / atomicOr of the HIP headers (relaxed, agent scope) on a global address: 4-byte T (the machine word IS a T)
  __device__ __forceinline__ V atomic_add(V v) const {
    static_assert(sizeof(T) == 4 && !std::is_const<T>::value, "atomic on a 4-byte element that is not const");
    return __hip_atomic_fetch_add((V TARL_GLOBAL*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ V atomic_or(V v) const {
    static_assert(sizeof(T) == 4 && !std::is_const<T>::value, "atomic on a 4-byte element that is not const");
    return __hip_atomic_fetch_or((V TARL_GLOBAL*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
template <class T>
__device__ __forceinline__ T TARL_GLOBAL* gbase(T* base) {
  return (T TARL_GLOBAL*)base;
}
template <class T>
__device__ __forceinline__ GRef<T> glob(T* p) {
  return GRef<T>{(typename GRef<T>::W TARL_GLOBAL*)p};
}
template <bool O32, class T>
__device__ __forceinline__ GRef<T> gat(T* base, uint32_t idx) {
  typedef typename GRef<T>::W W;
  if (O32) {
    // The byte offset is made a value of its own in the block of the access (an empty asm: no instruction). Otherwise the
    // zero-extended offset of a 4-byte element is shared with the post-word loads at the head of the kernel, reaches this block
    // as a 64-bit register pair whose upper half the instruction selector cannot see to be zero, and the access is
    // compiled with a 64-bit address per lane (v_lshl_add_u64) instead of `v_off, s[base]`.
    uint32_t off = idx * (uint32_t)sizeof(T);
    asm("" : "+v"(off));
    return GRef<T>{(W TARL_GLOBAL*)((const char TARL_GLOBAL*)base + (size_t)off)};
  }
  return GRef<T>{(W TARL_GLOBAL*)base + idx};
}

// the choice role of the merged insert + choice launch (fused_insert.hip: k_fused_insert_choice; built by the rollout loop)
struct ChoiceArgs {
  const int32_t* out_ptr;
  const int32_t* out_eid;
  const int32_t* group_of_node;
  int64_t G;
  const float* thr;
  const long long* lgt;
  uint64_t pseed, pcounter;
  int nchunk, want_lp;
  uint8_t* sel_next;       // frame t+1's action / SELECTED_ROAD slice
  long long* acc_next;
  unsigned gx;             // environment tiles (x extent of the choice grid)
  unsigned choice_blocks;  // gx * node chunks
};

// ---- developer knobs (TARL_* environment variables): read once per process and call site --------------------------------
#define env_int(NAME, DEFAULT)                                             \
  ([]() -> int {                                                           \
    static const int v = getenv(NAME) ? atoi(getenv(NAME)) : (DEFAULT);    \
    return v;                                                              \
  }())
#define env_flag_on(NAME) (env_int(NAME, 1) != 0)   // on unless set to 0

// TARL_ADDR32=0 keeps 64-bit addresses in the frame kernels whatever the batch size (developer knob: the instantiations that
// batches of 2^29 pairs and more run)
static inline bool addr32_ok() { return env_flag_on("TARL_ADDR32"); }

// rows per lane, all their loads in flight together: 1, 2 or 4. Row pass (TARL_NCHUNK; measured 63.7 / 57.8 / 56.0 us per
// launch) and Direction gather (TARL_NCHUNK_DIR; measured at B = 2048, config 4: 65.7 / 42.4 / 39.8 us per launch)
static inline int nchunk124(int v) { return v >= 4 ? 4 : (v >= 2 ? 2 : 1); }
static inline int nchunk_rows() { return nchunk124(env_int("TARL_NCHUNK", 4)); }
static inline int nchunk_dir() { return nchunk124(env_int("TARL_NCHUNK_DIR", 4)); }
// the choice kernel is light and ends in one accumulator atomic per lane: it walks longer chunks (TARL_NCHUNK_CHOICE)
static inline int nchunk_choice() {
  const int v = env_int("TARL_NCHUNK_CHOICE", 8);
  return v < 1 ? 1 : v;
}
static inline int64_t num_chunks(const tarl_plan* plan) { return ceil_div(plan->N, nchunk_rows()); }
static inline unsigned tile_threads(int64_t B) { return B >= TILE ? TILE : (unsigned)(ceil_div(B, 64) * 64); }

// ---- host functions used across the fused_*.hip files ----------------------------------------------------------------------
// fused_pack.hip (tarl_to_bufs and tarl_check_fused_core: fused_common.h)
int tarl_upload_bufs(const tarl_fused* f, const FusedBufs& fb, long long* acc_lp_alt, hipStream_t s, const FusedBufs** dev);
int tarl_check_frame_args(const tarl_plan* plan, const tarl_fused* f, int64_t B, const float* agent_features, int64_t A,
                          int64_t a_bstride, const int32_t* ins_scratch, const float* edge_attr, const float* log_edge_attr);
// fused_choice.hip: one frame's draw (k_fused_choice), and the all-frames draw of a rollout on the side stream
int tarl_launch_choice(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, long long* acc_lp,
                       const float* thresholds, const int64_t* log_probs, const float* uniform, uint64_t pseed,
                       uint64_t pcounter, uint8_t* sel_out, const uint8_t* sel_prev, int32_t* choice, int want_lp);
bool tarl_choice_ahead_fits(const tarl_plan* plan, int64_t T);
int tarl_choice_ahead_queue(hipStream_t s, const tarl_plan* plan, const tarl_fused* f, int64_t B, int64_t T,
                            const float* thresholds, const int64_t* log_probs, uint64_t policy_seed,
                            uint64_t policy_counter0, int32_t* choice_scratch, uint8_t* choice, float* log_prob,
                            const hipEvent_t** done);
int tarl_choice_ahead_wait(hipStream_t s, const hipEvent_t* done, int64_t t);
// fused_direction.hip, fused_rows.hip, fused_insert.hip: the frame kernels' launch dispatch
int tarl_launch_direction(dim3 grid, unsigned threads, hipStream_t s, const tarl_plan* plan, const tarl_fused* f,
                          const float* edge_attr, const float* log_edge_attr, const uint8_t* sel8, const float* gumbel,
                          float* dtt, float log_eps, float time, float prev_time, uint64_t seed, uint64_t counter,
                          int64_t B, int Nmax, const FrameOut& out, const uint8_t* cnt8 = nullptr);
int tarl_launch_rows(dim3 grid, unsigned threads, hipStream_t s, const tarl_plan* plan, const tarl_fused* f,
                     const FusedBufs* fb, int Nmax, int64_t B, float* agent_features, int64_t A, int64_t a_bstride,
                     float time, const FrameOut& out);
int tarl_insert_envs_per_wave(const tarl_fused* f, int64_t A, int64_t B, int64_t T, const float* times_host);
int tarl_launch_insert(int epw, hipStream_t s, int Nmax, int64_t B, int64_t N, const FusedBufs* fbt, PlanOut P,
                       const uint8_t* sel_t, float* agent_features, int64_t A, int64_t a_bstride, int use_cong, float time,
                       int32_t* ins_scratch, const float* entropy1, float* reward_t, const FrameOut& out, float* lp_t,
                       float* ent_t);
int tarl_launch_insert_choice(const ChoiceArgs& C, unsigned threads, hipStream_t s, int Nmax, int64_t B, int64_t N,
                              const FusedBufs* fbt, PlanOut P, const uint8_t* sel_t, float* agent_features, int64_t A,
                              int64_t a_bstride, int use_cong, float time, int32_t* ins_scratch, const float* entropy1,
                              float* reward_t, const FrameOut& out, float* lp_t, float* ent_t);
