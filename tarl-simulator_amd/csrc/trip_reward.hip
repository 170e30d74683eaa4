// trip_reward.hip — the TRIP reward: per environment, the travellers who should be under way and have not arrived.
// An environment-side rule in the style of policy_hold.hip and departures.hip, off by default and NOT in the reference. After a
// frame has run completely (Direction, rows, withdraw, insert) with the clock t:
//   on_way(b) = #{ a : a_status[b][a] == 1 }
//   ready(b)  = #{ a : a_status[b][a] == 0 && a_dep[b][a] <= t }      (the insert's own test, the same fp32 compare)
//   reward[b] = -(float)(on_way(b) + ready(b))                        (exact: A <= 2^24)
// Every row of the agent table counts, agent 0 included.
//
//   k_trip_status<WITH_DEP>: the pass over the status bytes, the only term that scales with B * A. The unit of work is one
//   WAVE and one SEGMENT of TR_SEG_GROUPS 16-byte groups (4 KB) of one environment's row: wave task w serves environment
//   w / S, segment w % S, S = max(1, ceil((A / 16) / TR_SEG_GROUPS)) segments per environment (A / 16, rounded down, is the
//   most whole groups a row can hold; the same S for every environment); a workgroup of TR_BLOCK threads takes TR_WAVES
//   consecutive tasks. A small A is one task per environment (four environments per workgroup), config 5 (A = 262 144) is
//   64 tasks = 16 workgroups per environment; from A = 8 208 (S = 3) on an environment can span two workgroups. Row b starts at byte b * A, unaligned
//   whenever A is no multiple of 16: the ALIGNED body [up16(row), down16(row + A)) is read by 16-byte loads, four independent
//   ones per lane and step; the at most 15 head bytes and 15 tail bytes are read one byte per lane (lanes 0..14 and 16..30 of
//   the environment's segment 0). A row that holds no aligned group is head bytes alone. Nothing outside [row, row + A) is
//   read. Bytes equal to 1 are counted four to a word (xor 0x01010101, the zero-byte mask, popcount). WITH_DEP (no departure
//   window): a waiting byte's a_dep is loaded and compared beside it. Integer arithmetic only: lanes -> wave by cross-lane
//   adds, waves -> workgroup through LDS (wave 0 adds the runs of equal environment), workgroup -> environment by ONE integer
//   atomicAdd per (workgroup, environment, count) into a word zeroed ahead of the launch: the result does not depend on the
//   schedule.
//   k_trip_ready_window: with the departure window (a_order, a_win, cur_lo, a_dep_sorted) ready(b) is k_pending_window's walk
//   (departures.hip): one wave per environment from cur_lo[b] while the sorted departure is <= t, the status byte per due
//   entry. Reads the agent arrays alone: neither the cursor nor a_ins is touched. Its lane 0 then writes the outputs.
//   k_trip_finish: without the window, one thread per environment writes the outputs.
//   The accumulator words are the OUTPUTS themselves: with `parts` the two int32 of parts[b], without it the 4 bytes of
//   reward[b] (on_way + ready as one integer, replaced by the float at the end), so the call needs no scratch.
//   Must move: B * A status bytes; with the window 16 + 1 B per due entry behind the cursor, without it 4 B per waiting agent;
//   12 B of output per environment. Plain vector stores, no floating-point atomics.
#include <cmath>
#include <mutex>
#include <unordered_map>

#include "rollout_heads.h"

#define TR_WAVE 64
#define TR_WAVES 4
#define TR_BLOCK (TR_WAVE * TR_WAVES)
#define TR_UNROLL 4
#define TR_SEG_GROUPS (TR_WAVE * TR_UNROLL)     // 16-byte groups per wave task: 4 KB of status bytes

// 0x80 in every byte of x that is zero
__device__ __forceinline__ uint32_t tr_zero_bytes(uint32_t x) {
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

template <bool WITH_DEP>
__device__ __forceinline__ void tr_word(uint32_t w, const float* __restrict__ dep, float t, int32_t& on, int32_t& ready) {
  on += __popc(tr_zero_bytes(w ^ 0x01010101u));
  if (WITH_DEP) {
    uint32_t z = tr_zero_bytes(w);
    while (z) {
      const int j = (__ffs((int)z) - 1) >> 3;
      ready += dep[j] <= t ? 1 : 0;
      z &= z - 1u;
    }
  }
}

__device__ __forceinline__ int32_t tr_wave_sum(int32_t v) {
#pragma unroll
  for (int o = TR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TR_WAVE);
  return v;
}

template <bool WITH_DEP>
__global__ __launch_bounds__(TR_BLOCK) void k_trip_status(const uint8_t* __restrict__ a_status, const float* __restrict__ a_dep,
                                                          int64_t A, int64_t B, int64_t S, float t, int32_t* __restrict__ acc,
                                                          int acc_stride, int ready_off) {
  __shared__ int32_t s_env[TR_WAVES], s_on[TR_WAVES], s_ready[TR_WAVES];
  const int lane = threadIdx.x & (TR_WAVE - 1), wave = threadIdx.x / TR_WAVE;
  const int64_t task = (int64_t)blockIdx.x * TR_WAVES + wave;
  const int64_t b = task / S, seg = task - b * S;
  int32_t on = 0, ready = 0;
  if (b < B) {                                                    // (wave-uniform)
    const uint8_t* row = a_status + b * A;
    const float* dep = WITH_DEP ? a_dep + b * A : nullptr;
    int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u);   // bytes before the first aligned group
    if (head > A) head = A;
    const int64_t groups = (A - head) >> 4;                       // whole aligned 16-byte groups of this row
    const int64_t tail0 = head + (groups << 4);                   // the first byte behind them; A - tail0 <= 15
    const uint4* body = (const uint4*)(row + head);
    const int64_t seg_end = (seg + 1) * (int64_t)TR_SEG_GROUPS, g_end = groups < seg_end ? groups : seg_end;
    const int64_t g = seg * (int64_t)TR_SEG_GROUPS + lane;
    uint4 v[TR_UNROLL];
#pragma unroll
    for (int k = 0; k < TR_UNROLL; ++k) {
      const int64_t gk = g + k * TR_WAVE;
      v[k] = gk < g_end ? body[gk] : make_uint4(0x02020202u, 0x02020202u, 0x02020202u, 0x02020202u);   // "done": counts nowhere
    }
#pragma unroll
    for (int k = 0; k < TR_UNROLL; ++k) {
      const int64_t gk = g + k * TR_WAVE;
      const float* d = WITH_DEP ? dep + head + (gk << 4) : nullptr;       // (dereferenced for a waiting byte of a loaded group only)
      tr_word<WITH_DEP>(v[k].x, d, t, on, ready);
      tr_word<WITH_DEP>(v[k].y, d + 4, t, on, ready);
      tr_word<WITH_DEP>(v[k].z, d + 8, t, on, ready);
      tr_word<WITH_DEP>(v[k].w, d + 12, t, on, ready);
    }
    if (seg == 0) {                                               // the unaligned ends, one byte per lane
      int64_t i = -1;
      if (lane < 15) {
        if (lane < head) i = lane;
      } else if (lane >= 16 && lane < 31) {
        if (tail0 + (lane - 16) < A) i = tail0 + (lane - 16);
      }
      if (i >= 0) {
        const uint8_t st = row[i];
        on += st == 1 ? 1 : 0;
        if (WITH_DEP && st == 0) ready += dep[i] <= t ? 1 : 0;
      }
    }
    on = tr_wave_sum(on);
    if (WITH_DEP) ready = tr_wave_sum(ready);
  }
  if (lane == 0) {
    s_env[wave] = b < B ? (int32_t)b : -1;
    s_on[wave] = on;
    s_ready[wave] = ready;
  }
  __syncthreads();
  if (threadIdx.x < TR_WAVES) {                                   // the first wave of every run of one environment adds the run
    const int w = threadIdx.x;
    const int32_t e = s_env[w];
    if (e >= 0 && (w == 0 || s_env[w - 1] != e)) {
      int32_t so = 0, sr = 0;
      for (int k = w; k < TR_WAVES && s_env[k] == e; ++k) {
        so += s_on[k];
        sr += s_ready[k];
      }
      if (so) atomicAdd(acc + (int64_t)e * acc_stride, so);
      if (WITH_DEP && sr) atomicAdd(acc + (int64_t)e * acc_stride + ready_off, sr);
    }
  }
}

// the outputs of environment b from its integer words (acc aliases parts, or reward where there are no parts)
__device__ __forceinline__ void tr_store(int64_t b, int32_t on, int32_t ready, float* __restrict__ reward,
                                         int32_t* __restrict__ parts) {
  reward[b] = -(float)(on + ready);
  if (parts) {
    parts[2 * b] = on;
    parts[2 * b + 1] = ready;
  }
}

__global__ __launch_bounds__(TR_WAVE) void k_trip_ready_window(const uint4* __restrict__ a_win,
                                                               const uint8_t* __restrict__ a_status,
                                                               const int32_t* __restrict__ cur_lo, int64_t A, float t,
                                                               float* __restrict__ reward, int32_t* __restrict__ parts) {
  const int64_t b = blockIdx.x;
  const uint4* win = a_win + b * A;
  const uint8_t* st = a_status + b * A;
  const int32_t lo = cur_lo[b];
  int32_t ready = 0;
  for (int64_t k0 = lo < 0 ? 0 : lo; k0 < A; k0 += TR_WAVE) {     // one wave: no barrier, the vote is the wave's
    const int64_t k = k0 + threadIdx.x;
    bool notdue = false;
    if (k < A) {
      const uint4 w = win[k];
      notdue = !(__uint_as_float(w.x) <= t);
      if (!notdue && (int64_t)w.z < A && st[w.z] == 0) ++ready;
    }
    if (__any(notdue ? 1 : 0)) break;                             // sorted by departure: nothing beyond this step is due
  }
  ready = tr_wave_sum(ready);
  if (threadIdx.x == 0) {
    const int32_t on = parts ? parts[2 * b] : ((const int32_t*)reward)[b];      // what k_trip_status added up
    tr_store(b, on, ready, reward, parts);
  }
}

__global__ __launch_bounds__(TR_BLOCK) void k_trip_finish(int64_t B, float* __restrict__ reward, int32_t* __restrict__ parts) {
  const int64_t b = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (b >= B) return;
  if (parts) tr_store(b, parts[2 * b], parts[2 * b + 1], reward, nullptr);
  else tr_store(b, ((const int32_t*)reward)[b], 0, reward, nullptr);            // on_way + ready came in as one integer
}

// segments per environment: every whole 16-byte group a row of A bytes can hold (A / 16 of them where it starts aligned)
static inline int64_t tr_segments(int64_t A) {
  const int64_t s = ceil_div(A / 16, TR_SEG_GROUPS);
  return s < 1 ? 1 : s;
}

// ---- the launches alone (handle and arguments checked by the caller) ----------------------------------------------------------
int tarl_launch_trip_reward(hipStream_t s, const tarl_fused* f, int64_t B, int64_t A, float t, float* reward, int32_t* parts) {
  const int64_t S = tr_segments(A);
  const unsigned grid = (unsigned)ceil_div(B * S, TR_WAVES);
  int32_t* acc = parts ? parts : (int32_t*)reward;
  const int stride = parts ? 2 : 1;
  TARL_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)(B * stride) * sizeof(int32_t), s));
  if (f->a_order && f->a_win) {
    hipLaunchKernelGGL(k_trip_status<false>, dim3(grid), dim3(TR_BLOCK), 0, s, (const uint8_t*)f->a_status, (const float*)nullptr,
                       A, B, S, t, acc, stride, 0);
    hipLaunchKernelGGL(k_trip_ready_window, dim3((unsigned)B), dim3(TR_WAVE), 0, s, (const uint4*)f->a_win,
                       (const uint8_t*)f->a_status, (const int32_t*)f->cur_lo, A, t, reward, parts);
  } else {
    hipLaunchKernelGGL(k_trip_status<true>, dim3(grid), dim3(TR_BLOCK), 0, s, (const uint8_t*)f->a_status, (const float*)f->a_dep,
                       A, B, S, t, acc, stride, parts ? 1 : 0);
    hipLaunchKernelGGL(k_trip_finish, dim3((unsigned)ceil_div(B, TR_BLOCK)), dim3(TR_BLOCK), 0, s, B, reward, parts);
  }
  TARL_LAUNCH_CHECK();
  return TARL_OK;
}

// ---- the switch of the one-call rollouts -------------------------------------------------------------------------------------
// tarl_fused does not grow: the parts pointer lives beside the handle, keyed by its address, and bit TARL_TRIP_REWARD of
// tarl_fused.policy_hold says that the reward of the loop is the trip reward (departures.hip has the scheme).
static std::mutex g_trip_mutex;
static std::unordered_map<const tarl_fused*, int32_t*> g_trip_parts;

int32_t* tarl_trip_reward_parts_of(const tarl_fused* f) {
  std::lock_guard<std::mutex> lock(g_trip_mutex);
  const auto it = g_trip_parts.find(f);
  return it == g_trip_parts.end() ? nullptr : it->second;
}

int tarl_check_trip_reward(const tarl_fused* f, int64_t B, int64_t A) {
  TARL_REQUIRE(A >= 1 && A <= ((int64_t)1 << 24), "bad sizes");
  TARL_REQUIRE(f->a_dep && f->a_status, "fused agent buffers missing");
  TARL_REQUIRE(f->a_order == nullptr || (f->cur_lo != nullptr && f->a_dep_sorted != nullptr),
               "a_order needs cur_lo and a_dep_sorted");
  TARL_REQUIRE(ceil_div(B * tr_segments(A), TR_WAVES) < ((int64_t)1 << 31), "bad sizes");
  return TARL_OK;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int tarl_fused_trip_reward(const tarl_plan* plan, const tarl_fused* f, int64_t B, int32_t Nmax, int64_t num_agents,
                                      float t, float* reward, int32_t* parts, tarl_stream stream) {
  TARL_REQUIRE(plan && f && reward, "null argument");
  int rc = tarl_check_fused_core(plan, f, B, Nmax);
  if (rc != TARL_OK) return rc;
  rc = tarl_check_trip_reward(f, B, num_agents);
  if (rc != TARL_OK) return rc;
  TARL_REQUIRE(std::isfinite(t), "non-finite time");
  return tarl_launch_trip_reward((hipStream_t)stream, f, B, num_agents, t, reward, parts);
}

extern "C" int tarl_fused_set_trip_reward(tarl_fused* f, int on, int32_t* parts) {
  TARL_REQUIRE(f, "null argument");
  TARL_REQUIRE(on == 0 || on == 1, "on must be 0 or 1");
  TARL_REQUIRE(on || !parts, "a parts buffer without the switch");
  std::lock_guard<std::mutex> lock(g_trip_mutex);
  if (on && parts) g_trip_parts[f] = parts;
  else g_trip_parts.erase(f);
  f->policy_hold = on ? (f->policy_hold | TARL_TRIP_REWARD) : (f->policy_hold & ~TARL_TRIP_REWARD);
  return TARL_OK;
}
