"""TEST INFRASTRUCTURE: numpy restatement of the per-road link counts (``tarl_link_counts_accumulate``,
``tarl_link_count_stats``, the host numbers of ``tarl_hip.evaluator``), the crafted accumulate cases shared by the host and
the GPU suite, the same restatement with ONE deliberate defect at a time, the 8 x 8 torus MODE recipe of
tests/test_gpu_eval.py restated, and a small irregular graph whose road count is no multiple of 4. Plain module: no
fixtures; nothing at import time needs a GPU.

Definition (the reference's compute_node_metrics / plot_daily_counts): count[b][h][n] = sum over the frames t whose START
clock ``t0 + t * timestep`` lies in bin ``first_bin + h`` of popped_t[b][n] + withdrawn_t[b][n]."""
from __future__ import annotations

import math

import numpy as np
import torch

MAX_FRAMES = 127        # TARL_LINK_COUNTS_MAX_FRAMES: 8-bit partial sums, at most 2 per frame
DEFECTS = ("clock_after_step", "drop_withdrawn", "clamp_to_one", "saturate_255", "overwrite_second_block",
           "skip_partial_block")


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
def accumulate(popped, withdrawn, counts, t0, timestep, bin_seconds, first_bin, defect=None, call_index=0):
    """``counts`` (B, H, N) int32 += the per-bin sums of ``popped`` + ``withdrawn`` (F, B, N) uint8, in place. ``defect``:
    one of :data:`DEFECTS` that acts inside one call (the others act in :func:`run_case`)."""
    F = popped.shape[0]
    H = counts.shape[1]
    add = np.zeros_like(counts, dtype=np.int64)
    for f in range(F):
        clock = t0 + (f + 1 if defect == "clock_after_step" else f) * timestep
        h = clock // bin_seconds - first_bin
        v = popped[f].astype(np.int64) + (0 if defect == "drop_withdrawn" else withdrawn[f].astype(np.int64))
        if defect == "clamp_to_one":
            v = np.minimum(v, 1)
        if 0 <= h < H:                       # (only a defect can leave the stored bins)
            add[:, h, :] += v
    if defect == "overwrite_second_block" and call_index > 0:
        touched = add != 0
        counts[touched] = 0
    total = counts.astype(np.int64) + add
    if defect == "saturate_255":
        total = np.minimum(total, 255)
    counts[...] = total.astype(np.int32)
    return counts


def _masks(F, B, N, seed, density=0.3):
    """Random 0/1 masks of the given density; the first element of the first frame is popped and the last element of the
    last frame withdrawn from, so that no shape, however small, is a case of all zeros."""
    rng = np.random.default_rng(seed)
    p, w = (rng.random((F, B, N)) < density).astype(np.uint8), (rng.random((F, B, N)) < density).astype(np.uint8)
    p[0, 0, 0] = 1
    w[-1, -1, -1] = 1
    return p, w


def _case(name, popped, withdrawn, t0, timestep, bin_seconds, block):
    """A sequence of calls as the evaluator issues them: blocks of ``block`` frames, the last one partial where the frames
    do not fill it. One empty bin is stored on either side of the bins the frames reach: it must stay zero."""
    T, B, N = popped.shape
    first_bin = t0 // bin_seconds - 1
    assert first_bin >= 0
    H = (t0 + (T - 1) * timestep) // bin_seconds - first_bin + 2
    calls = [dict(t0=t0 + f0 * timestep, popped=np.ascontiguousarray(popped[f0:f0 + block]),
                  withdrawn=np.ascontiguousarray(withdrawn[f0:f0 + block]), partial=min(block, T - f0) < block)
             for f0 in range(0, T, block)]
    return dict(name=name, B=B, N=N, H=int(H), first_bin=int(first_bin), timestep=timestep, bin_seconds=bin_seconds,
                calls=calls)


SHAPES = ((1, 1, 1), (5, 6, 7), (3, 21, 64), (2, 257, 64))      # (B, N, F): B N % 4 != 0, N odd, one frame, one element


def crafted_cases():
    """Every accumulate case of the GPU suite. Per shape: no bin edge inside the block; the edge at its first frame; the
    edge at its last frame; several edges inside with bins skipped (timestep 25, bins of 10 s). Then two consecutive calls
    into the same counts, the second continuing the first one's last bin (64 + 30 frames, an edge inside the first),
    all-ones masks at the declared maximum F, twice into the same bin: exactly 2 F, then 4 F = 508 > 255, and a clock that
    stands still (timestep 0): every frame of the call falls in one bin."""
    cases = []
    for i, (B, N, F) in enumerate(SHAPES):
        p, w = _masks(F, B, N, seed=100 + i)
        cases.append(_case(f"{B}x{N}x{F}-no-edge", p, w, 4000, 1, 3600, F))
        cases.append(_case(f"{B}x{N}x{F}-edge-first", p, w, 7200, 1, 3600, F))
        cases.append(_case(f"{B}x{N}x{F}-edge-last", p, w, 7200 - (F - 1), 1, 3600, F))
        cases.append(_case(f"{B}x{N}x{F}-skipping", p, w, 1000, 25, 10, F))
    p, w = _masks(94, 3, 21, seed=200)
    cases.append(_case("two-calls", p, w, 7200 - 40, 1, 3600, 64))
    ones = np.ones((2 * MAX_FRAMES, 1, 5), dtype=np.uint8)
    cases.append(_case("all-ones-max-F-twice", ones, ones, 36000, 1, 3600, MAX_FRAMES))
    p, w = _masks(7, 5, 6, seed=201)
    cases.append(_case("5x6x7-timestep-0", p, w, 4000, 0, 3600, 7))
    return cases


def run_case(case, defect=None, accumulate_fn=None):
    """The calls of ``case`` into zeroed counts -> (B, H, N) int32. ``accumulate_fn(call, counts, case)``: the implementation
    under test in place of the restatement (the GPU suite)."""
    counts = np.zeros((case["B"], case["H"], case["N"]), dtype=np.int32)
    for k, call in enumerate(case["calls"]):
        if defect == "skip_partial_block" and call["partial"]:
            continue
        if accumulate_fn is not None:
            counts = accumulate_fn(call, counts, case)
        else:
            accumulate(call["popped"], call["withdrawn"], counts, call["t0"], case["timestep"], case["bin_seconds"],
                       case["first_bin"], defect=defect, call_index=k)
    return counts


def binned(popped, withdrawn, clock0, timestep, bin_seconds):
    """All frames at once, without blocks: (T, B, N) masks -> (first_bin, counts (B, H, N) int32), H the bins the frames
    reach."""
    T, B, N = popped.shape
    first_bin = clock0 // bin_seconds
    H = (clock0 + (T - 1) * timestep) // bin_seconds - first_bin + 1
    counts = np.zeros((B, H, N), dtype=np.int32)
    accumulate(popped, withdrawn, counts, clock0, timestep, bin_seconds, first_bin)
    return int(first_bin), counts


# ---- statistics over the environments -----------------------------------------------------------------------------------------
def differences(a, b=None):
    """(K, H + 1, N) int64: a (- b) per environment with the episode total appended as the last row."""
    d = a.astype(np.int64) - (0 if b is None else b.astype(np.int64))
    return np.concatenate([d, d.sum(axis=1, keepdims=True)], axis=1)


def stats(a, b=None):
    d = differences(a, b)
    return {"sum": d.sum(axis=0), "sumsq": (d * d).sum(axis=0), "min": d.min(axis=0).astype(np.int32),
            "max": d.max(axis=0).astype(np.int32)}


def moments(a, b=None):
    """numpy's own mean / sample standard deviation / standard error / interval of the differences (None for K = 1)."""
    d = differences(a, b).astype(np.float64)
    K = d.shape[0]
    out = {"mean": d.mean(axis=0), "std": None, "se": None, "ci95_lo": None, "ci95_hi": None}
    if K >= 2:
        std = d.std(axis=0, ddof=1)
        se = std / math.sqrt(K)
        out.update(std=std, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def geh(m, c):
    m, c = np.asarray(m, dtype=np.float64), np.asarray(c, dtype=np.float64)
    out = np.zeros(m.shape)
    nz = (m + c) != 0
    out[nz] = np.sqrt(2.0 * (m[nz] - c[nz]) ** 2 / (m[nz] + c[nz]))
    return out


def assert_stats_equal(got, want):
    for k in ("sum", "sumsq", "min", "max"):
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k])
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k


def assert_moments_close(got, want, K):
    """``mean`` is the exact integer sum over K in both: ==. std / se / interval come from sqrt of the exact integer
    K sum d^2 - (sum d)^2 on one side and from numpy's two-pass float64 formula on the other: a few ulp of float64 apart
    (rtol 1e-12, and atol 1e-9 where the spread is 0 and numpy's two-pass sum leaves a rounding residue)."""
    assert np.array_equal(got["mean"], want["mean"])
    for k in ("std", "se", "ci95_lo", "ci95_hi"):
        if K == 1:
            assert got[k] is None and want[k] is None, k
        else:
            assert np.allclose(got[k], want[k], rtol=1e-12, atol=1e-9), k


# ---- the 8 x 8 torus MODE recipe of tests/test_gpu_eval.py, restated -----------------------------------------------------------
def oracle_mode(net, emb):
    """The oracle's MODE action of the embedding head (state-independent): (GraphDist, one-hot (E,) long, successor map)."""
    from oracle import dist, nets
    gd = dist.GraphDist(nets.policy_logits(net.x[:, 3 * net.Nmax:], net.edge_index, emb), net.edge_index)
    action = gd.mode.long()
    succ = torch.empty(net.num_roads, dtype=torch.long)
    chosen = action.nonzero().view(-1)
    succ[net.edge_index[0, chosen]] = net.edge_index[1, chosen]
    return gd, action, succ


def deliverable_population(net, succ, agents=128):
    """synth.population(agents, N, seed=7, t1=EPISODE_START + 200) with the destination of rows 1, 3, 5, ... replaced by the
    road three MODE steps from the row's origin."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    pop = synth.population(agents, net.num_roads, seed=7, t1=EPISODE_START + 200)
    o = pop[1::2, 0].long()
    pop[1::2, 1] = succ[succ[succ[o]]].float()
    return pop


def engine_of(net, pop, K, seed=3, env_base=0):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed, env_base=env_base)


def embedding_evaluator(net, pop, K, seed=3, **kw):
    """VecEvaluator(head "embedding") with the embedding of seed 0 on an engine of ``seed`` -> (evaluator, embedding)."""
    from tarl_hip.evaluator import VecEvaluator
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    return VecEvaluator(engine_of(net, pop, K, seed), "embedding", emb=emb.cuda(), **kw), emb


# ---- a small irregular graph: 21 roads, 49 edges, no dead end ------------------------------------------------------------------
def small_graph():
    import irregular_graphs as ig
    net = ig.road_network(ig.hub_links(((2, 3),), 8, 5), 5)
    assert net.num_roads == 21 and net.edge_index.size(1) == 49
    assert int(torch.bincount(net.edge_index[0], minlength=21).min()) >= 1      # no dead end
    return net


def small_population(net):
    import irregular_graphs as ig
    from tarl_hip.engine import EPISODE_START
    return ig.population(net, 3, seed=5, t0=EPISODE_START, t1=EPISODE_START + 90)
