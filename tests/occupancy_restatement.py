"""TEST INFRASTRUCTURE: numpy restatement of the per-road occupancy accumulation (``tarl_occupancy_accumulate``), the crafted
cases shared by the host and the GPU suite, and the same restatement with ONE deliberate defect at a time. The statistics over
the environments, the moments and the graph / evaluator recipes are those of tests/link_counts_restatement.py, re-exported
here. Plain module: no fixtures; nothing at import time needs a GPU.

Definition: frame t of a call starts at clock ``t0 + t * timestep`` and belongs to bin ``clock // bin_seconds - first_bin``
(the clock at which the step STARTS); c_t[n][k] is NUMBER_OF_AGENT of road n in environment k AFTER frame t.
  veh[k][h][n]  = sum over t in bin h of c_t[n][k]
  full[k][h][n] = #{t in bin h : c_t[n][k] >= thr[n]},  thr[n] = ceil(MAX[n] - 3)
  peak[k][0][n] = max over t of c_t[n][k]"""
from __future__ import annotations

import numpy as np

from link_counts_restatement import (assert_moments_close, assert_stats_equal, deliverable_population,  # noqa: F401
                                     embedding_evaluator, engine_of, moments, oracle_mode, small_graph, small_population,
                                     stats)

TILE = 64
DEFECTS = ("clock_after_step", "count_before_frame", "greater_than", "threshold_max_minus_2", "peak_added",
           "overwrite_second_call", "skip_partial_block", "swap_in_tile")


def threshold(max_agents):
    """thr = ceil(MAX - 3): the negation of has_room = n < MAX - CONGESTION_FILE."""
    return np.ceil(np.asarray(max_agents, dtype=np.float64) - 3.0).astype(np.int32)


def to_count(ring):
    """fp32 -> the count the kernel sees: truncation, NaN and negatives 0, above 255 -> 255."""
    v = np.asarray(ring, dtype=np.float64)
    v = np.where(np.isnan(v) | (v < 0), 0.0, np.minimum(v, 255.0))
    return np.trunc(v).astype(np.int64)


def _swap_in_tile(c):
    """(F, N, K) counts with (n, k) exchanged inside every 64 x 64 tile, where both partners exist."""
    out = c.copy()
    F, N, K = c.shape
    for n in range(N):
        for k in range(K):
            n2, k2 = n // TILE * TILE + k % TILE, k // TILE * TILE + n % TILE
            if n2 < N and k2 < K:
                out[:, n, k] = c[:, n2, k2]
    return out


def accumulate(ring, thr, veh, full, peak, t0, timestep, bin_seconds, first_bin, defect=None, call_index=0):
    """The three accumulators (K, H, N), (K, H, N), (K, 1, N) int32 in place from ``ring`` (F, N, K) fp32. ``defect``: one of
    :data:`DEFECTS` that acts inside one call (the others act in :func:`run_case`)."""
    c = to_count(ring)
    if defect == "swap_in_tile":
        c = _swap_in_tile(c)
    F = c.shape[0]
    H = veh.shape[1]
    t = thr.astype(np.int64) + (1 if defect == "threshold_max_minus_2" else 0)
    add_v, add_f = np.zeros(veh.shape, dtype=np.int64), np.zeros(full.shape, dtype=np.int64)
    for f in range(F):
        clock = t0 + (f + 1 if defect == "clock_after_step" else f) * timestep
        h = clock // bin_seconds - first_bin
        at = c[f] > t[:, None] if defect == "greater_than" else c[f] >= t[:, None]
        if 0 <= h < H:                       # (only a defect can leave the stored bins)
            add_v[:, h, :] += c[f].T
            add_f[:, h, :] += at.T
    pk = c.max(axis=0).T[:, None, :]
    if defect == "overwrite_second_call" and call_index > 0:
        veh[add_v != 0] = 0
        full[add_f != 0] = 0
        peak[...] = 0
    veh[...] = (veh + add_v).astype(np.int32)
    full[...] = (full + add_f).astype(np.int32)
    peak[...] = (peak + pk if defect == "peak_added" else np.maximum(peak, pk)).astype(np.int32)
    return veh, full, peak


# ---- crafted cases ----------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 1), (5, 6, 7), (3, 21, 64), (64, 64, 3), (65, 63, 9), (2, 257, 64), (130, 70, 5))      # (K, N, F)
CLOCKS = (("no-edge", lambda F: (4000, 1, 3600)), ("edge-first", lambda F: (7200, 1, 3600)),
          ("edge-last", lambda F: (7200 - (F - 1), 1, 3600)), ("skipping", lambda F: (1000, 25, 10)))
MAX_VALUES = (0.0, 2.0, 3.0, 5.0, 8.0, 14.0, 129.0)       # thr -3, -1, 0, 2, 5, 11, 126


def _ring(F, N, K, seed):
    """MAX per road from :data:`MAX_VALUES` (roads 0 and 1, where they exist, get MAX 0 and 3: thr <= 0) and every value one
    of {0, thr - 1, thr, thr + 1, 127} (negative ones 0). The first element of the first frame and the last of the last are
    127, so that no shape, however small, is a case of all zeros."""
    rng = np.random.default_rng(seed)
    cap = rng.choice(np.asarray(MAX_VALUES), size=N)
    cap[:2] = (0.0, 3.0)[:min(N, 2)]
    thr = threshold(cap)
    pick = rng.integers(0, 5, size=(F, N, K))
    t = thr.astype(np.int64)[None, :, None]
    ring = np.choose(pick, [np.zeros_like(pick), t - 1 + 0 * pick, t + 0 * pick, t + 1 + 0 * pick, np.full_like(pick, 127)])
    ring = np.maximum(ring, 0).astype(np.float32)
    ring[0, 0, 0] = ring[-1, -1, -1] = 127.0
    return ring, thr, cap


def _case(name, ring, thr, t0, timestep, bin_seconds, block):
    """A sequence of calls as the evaluator issues them: blocks of ``block`` frames, the last one partial where the frames
    do not fill it. One empty bin is stored on either side of the bins the frames reach: it must stay zero."""
    T, N, K = ring.shape
    first_bin = t0 // bin_seconds - 1
    assert first_bin >= 0
    H = (t0 + (T - 1) * timestep) // bin_seconds - first_bin + 2
    calls = [dict(t0=t0 + f0 * timestep, ring=np.ascontiguousarray(ring[f0:f0 + block]), partial=min(block, T - f0) < block)
             for f0 in range(0, T, block)]
    return dict(name=name, K=K, N=N, H=int(H), first_bin=int(first_bin), timestep=timestep, bin_seconds=bin_seconds,
                thr=thr, ring=ring, calls=calls)


def crafted_cases():
    """Every accumulate case of the GPU suite. Per shape: no bin edge inside the call; the edge at its first frame; the edge at
    its last frame; several edges inside with bins skipped (timestep 25, bins of 10 s). Then consecutive calls into the same
    accumulators: 64 + 30 frames with an edge inside the first call and the second continuing its last bin (the last block
    partial), 9 frames in blocks of 4 on a shape with partial tiles on both axes, and a clock that stands still (timestep 0):
    every frame of the call falls in one bin."""
    cases = []
    for i, (K, N, F) in enumerate(SHAPES):
        ring, thr, _ = _ring(F, N, K, seed=300 + i)
        for label, clock in CLOCKS:
            cases.append(_case(f"{K}x{N}x{F}-{label}", ring, thr, *clock(F), F))
    ring, thr, _ = _ring(94, 21, 3, seed=400)
    cases.append(_case("two-calls", ring, thr, 7200 - 40, 1, 3600, 64))
    ring, thr, _ = _ring(9, 63, 65, seed=401)
    cases.append(_case("three-calls", ring, thr, 7200 - 5, 1, 3600, 4))
    ring, thr, _ = _ring(7, 6, 5, seed=402)
    cases.append(_case("5x6x7-timestep-0", ring, thr, 4000, 0, 3600, 7))
    return cases


def run_case(case, defect=None, accumulate_fn=None):
    """The calls of ``case`` into zeroed accumulators -> (veh, full, peak). ``accumulate_fn(call, acc, case)``: the
    implementation under test in place of the restatement (the GPU suite); it returns the three arrays."""
    K, H, N = case["K"], case["H"], case["N"]
    acc = (np.zeros((K, H, N), dtype=np.int32), np.zeros((K, H, N), dtype=np.int32), np.zeros((K, 1, N), dtype=np.int32))
    prev = np.zeros((1, N, K), dtype=np.float32)      # count_before_frame: the count before frame 0 of a reset network
    for j, call in enumerate(case["calls"]):
        ring = call["ring"]
        if defect == "count_before_frame":
            ring, prev = np.concatenate([prev, ring[:-1]]), ring[-1:]
        if defect == "skip_partial_block" and call["partial"]:
            continue
        if accumulate_fn is not None:
            acc = accumulate_fn(call, acc, case)
        else:
            accumulate(ring, case["thr"], *acc, call["t0"], case["timestep"], case["bin_seconds"], case["first_bin"],
                       defect=defect, call_index=j)
    return acc


def binned(counts, thr, clock0, timestep, bin_seconds):
    """All frames at once, without blocks: counts (T, N, K) -> (first_bin, veh, full, peak), H the bins the frames reach."""
    T, N, K = counts.shape
    first_bin = clock0 // bin_seconds
    H = (clock0 + (T - 1) * timestep) // bin_seconds - first_bin + 1
    acc = (np.zeros((K, H, N), dtype=np.int32), np.zeros((K, H, N), dtype=np.int32), np.zeros((K, 1, N), dtype=np.int32))
    accumulate(np.asarray(counts, dtype=np.float32), thr, *acc, clock0, timestep, bin_seconds, first_bin)
    return (int(first_bin),) + acc
