"""VecEvaluator — evaluate ONE policy on K vectorised environments of a fused :class:`SimEngine`, deterministically
(MODE: ``GraphDistribution.mode``, torchrl's ``ExplorationType.MODE`` of the reference's ``_evaluate``,
src/rl/ppo_trainer.py:89-127,149) or with sampled actions, and report per-environment results with their spread.

The K environments share the network and (unless the caller owns a (K, A, 9) table) the population; they differ in their
noise streams (``env_base + b``: the Gumbel race of DirectionMPNN.aggregate), so one evaluation yields K realisations of the
stochastic simulator instead of the single one of the drop-in ``SimulatorEnv.rollout`` pass.

Per frame, on the caller's stream and without a host synchronisation: the head's logits from the packed state (existing
ops), the action as SELECTED_ROAD bytes (``ops.graphdist_mode_rollout`` / ``ops.graphdist_rollout``), then
``SimEngine.frame_fused(skip_choice=True)`` with the frame's reward written into a (T, K) buffer. The report comes from
``ops.episode_summary`` (one launch); the host only turns K numbers per quantity into mean / spread.

Domain exits: a FIFO count that reaches ``Nmax`` leaves the reference's defined domain (the engine's status word). The
evaluator copies the status word to pinned memory every ``poll_frames`` frames and looks at the copies that have arrived;
once it sees the flag it queues nothing more, and a run that left the domain returns ``domain_exit=True`` with NO statistics.

The shortest-path baseline (head ``"dijkstra"``): the classical router on the same K environments. Every ``refresh_rate``
frames (frame 0 included) every environment's own congested travel times are read from the packed state
(``ops.fused_edge_travel_time``) and one reverse shortest-path tree per (environment, distinct destination of the agent
tables) is rebuilt (``ops.destination_trees_batched``); every frame each row selects the next hop towards its head agent's
destination (``ops.fused_select_next_hop_dest``) and the frame runs with that action. The step order is the ENVIRONMENT's —
choice, core, withdraw / insert, reward (``SimulatorEnv._step``) — and deliberately NOT the classical loop's (insert,
withdraw, choice, core) of the drop-in ``DijkstraAgents``: the baseline faces exactly the environment the policy faces. The
noise streams are keyed by (seed, frame counter, env_base + b), so a baseline run on an engine of the same seed sees the
Gumbel race values of the policy run (common random numbers), and :func:`paired_report` compares the two per environment.
In that order the core moves a due agent from the last road before its destination ONTO the destination road before the
withdraw (which collects from roads ADJACENT to the destination) sees it; there the table names the road itself, the row
moves nobody, and the agent stays: the router delivers only agents whose last hop was delayed.

Head ``"dijkstra_hold"`` is the router that delivers in that order (NOT the reference's rule): a row whose
next hop is its head agent's destination selects ITSELF (``ops.fused_select_next_hop_dest(hold=True)``), the core moves
nobody from it, and the withdraw collects the agent there once it is due. Everything else is the ``"dijkstra"`` head's. With
``refresh_rate=0`` it builds its tables at frame 0 only: after the reset every count is 0, so this is the free-flow
(all-or-nothing) router under the router's own weight expression. (``"dijkstra"`` keeps refusing 0, as it always has.)

Head ``"routes"`` (NOT in the reference, which has no replanning loop) follows a PLAN: one route per agent
(``ops.td_routes``), shared by the environments or one per environment. Every frame each row selects the road that follows
it on its head agent's route (``ops.fused_select_route``, with the hold rule one road short of the destination); a row whose
head has no route or stands off its route keeps its byte. What that byte is decides whether the head delivers: the
environment inserts a departing agent into the road its ORIGIN row selects (``Agents.insert_agent_into_network``), not into
the origin road, and an empty row reads the dummy agent 0, who has no route — so an origin row that nobody stands on keeps a
stale byte and a newcomer seldom lands on its own route. With ``route_fallback=True`` (the default) the free-flow hold router
(the ``"dijkstra_hold"`` head on ONE table built at frame 0 from the empty network and shared by the environments) therefore
writes every row first and the plan overrides it wherever the head is on its route: an agent off its route is led to its
destination by the free-flow tree and follows its plan again from the first road they share. ``route_fallback=False`` is the
select kernel alone. No refresh, no policy tensors, no sampled mode; the step order is the environment's, as for the routers.
``set_routes`` swaps the plan between two runs (``tarl_hip.replanning.Replanner`` does, once per simulated day).
"""
from __future__ import annotations

import math
import time
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .engine import EPISODE_END, EPISODE_START
from .eval_reports import (CONGESTION_FILE, DYNAMIC_GAP_NOTE, LINK_EXPECTED, LINK_PARTIAL_NOTE, LINK_RING_BYTES,  # noqa: F401
                           OCCUPANCY_RING_BYTES, TRIP_CHANCE, TRIP_FF_CHUNK_BYTES, TRIP_FF_NOTE, TURN_RING_BYTES, _CI95_KIND,
                           _interval, _sample_moments,
                           aggregate, capacity_threshold, dynamic_gap_lines, dynamic_gap_paired_lines, dynamic_gap_report,
                           dynamic_gap_summary, geh, link_bin_names, link_count_lines, link_count_report, link_count_summary,
                           link_moments, occupancy_bin_names, occupancy_lines, occupancy_report, occupancy_summary,
                           path_lines, path_report, path_route_rows, path_summary,
                           trip_bin_names, trip_free_flow_times, trip_host_bin, trip_lines, trip_report, trip_summary,
                           turn_bin_names, turn_lines, turn_report, turn_summary)

HEADS = ("embedding", "edge_mlp", "edge_mlp_fp32", "edge_mlp_bf16", "embedding_dijkstra", "graph_transformer", "goal_mlp", "dijkstra",
         "dijkstra_hold", "routes")
PLAN_HEADS = ("routes",)                          # follows a per-agent plan (set_routes): no policy tensors, no sampled mode
ROUTER_HEADS = ("dijkstra", "dijkstra_hold")      # the shortest-path routers: no policy tensors, no sampled mode
# the names of --eval-baseline / ppo_train(eval_baseline=) -> (head, its VecEvaluator arguments); "free_flow": the hold router
# on tables built once from the empty network
EVAL_BASELINES = {"dijkstra": ("dijkstra", {}), "dijkstra_hold": ("dijkstra_hold", {}),
                  "free_flow": ("dijkstra_hold", {"refresh_rate": 0})}
# the names of --dijkstra-router -> (head, refresh_rate override or None for the agent's own)
DIJKSTRA_ROUTERS = {"reference": ("dijkstra", None), "hold": ("dijkstra_hold", None), "free_flow": ("dijkstra_hold", 0)}


def router_label(res):
    """The name a printed block gives a router run: its head, and the static tables where it has them."""
    return res.head + (", refresh_rate 0" if res.settings.get("refresh_rate") == 0 else "")
_MLP_PRECISION = {"edge_mlp": "x3", "edge_mlp_fp32": "fp32", "edge_mlp_bf16": "bf16"}
PER_ENV_KEYS = ("episode_return", "frames", "arrived", "on_way", "not_departed", "avg_travel_time", "std_travel_time",
                "max_travel_time", "p50_travel_time", "p95_travel_time")


def hist_percentile(hist, q, bin_width):
    """The ``q``-quantile (0 < q <= 1) of binned data as the UPPER edge of the bin that holds the sample of rank
    ceil(q n) (the inverted empirical CDF, numpy's ``method="inverted_cdf"``); ``None`` for an empty histogram. The last
    bin collects everything at or above its lower edge, so its upper edge is a lower bound there."""
    h = np.asarray(hist, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return None
    v = n * float(q) - 1.0
    i = math.floor(v)
    idx = min(max(int(i) + (1 if v - i > 0 else 0), 0), n - 1)        # 0-based rank of the sample
    k = int(np.searchsorted(np.cumsum(h), idx + 1, side="left"))
    return float((k + 1) * bin_width)


@dataclass
class EvalResult:
    """Per-environment lists (length ``envs``; ``None`` where undefined) and their aggregates over the environments. After
    a domain exit every per-environment field and ``aggregate`` is ``None``: such a run is never averaged."""
    envs: int
    head: str
    deterministic: bool
    frames_run: int
    domain_exit: bool = False
    domain_exit_frames: tuple | None = None       # (first, last + 1) frame of the polled block that showed the flag
    episode_return: list | None = None            # sum of the rewards = -(sum over frames of the network's occupancy)
    frames: list | None = None
    arrived: list | None = None                   # DONE == 1
    on_way: list | None = None                    # ON_WAY flag count (the reference's leg histogram), NOT the occupancy
    not_departed: list | None = None
    avg_travel_time: list | None = None           # None for an environment without an arrival
    std_travel_time: list | None = None           # population standard deviation over the environment's arrived agents
    max_travel_time: list | None = None
    p50_travel_time: list | None = None           # from the histogram: upper bin edge
    p95_travel_time: list | None = None
    aggregate: dict | None = None
    envs_without_arrival: int | None = None
    settings: dict = field(default_factory=dict)
    computation_time_ms: float = field(default=0.0, compare=False)
    # link_counts=True (never after a domain exit): per-road counts of pops + withdrawals per time bin
    link_counts: np.ndarray | None = field(default=None, compare=False)     # (K, H, N) int32, bin h = link_first_bin + h
    link_first_bin: int | None = None             # floor(EPISODE_START / link_bin_seconds)
    link_bin_seconds: int | None = None
    link_stats: dict | None = field(default=None, compare=False)            # link_moments over the K environments
    # occupancy=True (never after a domain exit): sums over frames of NUMBER_OF_AGENT, the quantity the reward is made of
    occupancy: dict | None = field(default=None, compare=False)             # veh, full (K, H, N), peak (K, 1, N) int32
    occupancy_stats: dict | None = field(default=None, compare=False)       # link_moments of each of the three arrays
    occupancy_frames_per_bin: list | None = None  # frames run in each of the H bins (bin h = occupancy_meta first_bin + h)
    occupancy_meta: dict | None = field(default=None, compare=False)        # first_bin, bin_seconds, timestep, max, thr
    # trips=True (never after a domain exit): the agent tables reduced per agent and per (environment, time bin)
    trips: dict | None = field(default=None, compare=False)                 # ops.trip_agent_stats, numpy arrays (A,)
    trip_bins: dict | None = field(default=None, compare=False)             # ops.trip_bin_stats, numpy arrays (K, H)
    trip_meta: dict | None = field(default=None, compare=False)             # first_bin, bin_seconds, origin, destination,
    #                                                                         departure, free_flow (A,), paired
    # dynamic_gap=True (never after a domain exit): the trips against the best path in hindsight, DESIGN 4.17
    dynamic_gap: dict | None = field(default=None, compare=False)           # best (J, A) fp64, per_agent, per_env, per_bin, meta
    # turns=True (never after a domain exit): vehicles per route edge and time bin, and the agents quirk Q24 loses, DESIGN 4.18
    turn_counts: np.ndarray | None = field(default=None, compare=False)     # (K, H, E) int32, the caller's edge order
    turn_lost: np.ndarray | None = field(default=None, compare=False)       # (K, H, N) int32: phantom pops per road
    turn_stats: dict | None = field(default=None, compare=False)            # link_moments of "turns" and of "lost"
    turn_meta: dict | None = field(default=None, compare=False)             # first_bin, bin_seconds, edge_index, policy_prob
    # policy_hold=True (never after a domain exit): rows the hold rule rewrote, summed over the frames, DESIGN 4.20
    held: np.ndarray | None = field(default=None, compare=False)            # (K,) int64
    # route_departures=True (never after a domain exit): empty origin rows the first-hop rule wrote, summed over the frames,
    # DESIGN 4.23
    departures_routed: np.ndarray | None = field(default=None, compare=False)       # (K,) int64
    # trip_reward=True (never after a domain exit): the trip reward of DESIGN 4.24 beside the queue reward — per environment
    # the sum over the frames of -(on_way + ready), and {on_way, ready} after the last frame
    trip_return: list | None = None
    trip_parts_last: np.ndarray | None = field(default=None, compare=False)         # (K, 2) int64
    # paths=True (never after a domain exit): the per-agent path trace of DESIGN 4.25
    paths: dict | None = field(default=None, compare=False)                 # last_road, roads, revisits, off_tree int32, path_cost,
    #                                                                         excess fp64, done bool: numpy arrays (K, A)
    path_routes: tuple | None = field(default=None, compare=False)          # (routes (K, A, L) int32, route_len (K, A) = min(roads, L))
    path_stats: dict | None = field(default=None, compare=False)            # ops.path_agent_stats, numpy arrays (A,)
    path_meta: dict | None = field(default=None, compare=False)             # max_hops, weights, note, bins, origin, destination,
    #                                                                         departure (A,), paired

    def to_dict(self, per_env=False):
        d = {k: getattr(self, k) for k in ("envs", "head", "deterministic", "frames_run", "domain_exit",
                                           "domain_exit_frames", "aggregate", "envs_without_arrival", "settings",
                                           "computation_time_ms")}
        if per_env:
            d["per_env"] = {k: getattr(self, k) for k in PER_ENV_KEYS}
            if self.trip_return is not None:      # (without trip_reward the document stays as it was)
                d["per_env"]["trip_return"] = self.trip_return
        return d

    def rows(self):
        """One dict per environment (the rows of eval_envs.csv)."""
        if self.domain_exit:
            return []
        extra = () if self.trip_return is None else ("trip_return",)
        return [dict(env=b, **{k: getattr(self, k)[b] for k in PER_ENV_KEYS + extra}) for b in range(self.envs)]

    def summary_lines(self):
        """The aggregate as printable lines."""
        if self.domain_exit:
            a, b = self.domain_exit_frames
            return [f"domain exit: a FIFO count reached Nmax between frames {a} and {b}; no statistics"]
        out = []
        for k in PER_ENV_KEYS + (() if self.trip_return is None else ("trip_return",)):
            g = self.aggregate[k]
            if g["mean"] is None:
                out.append(f"{k + ':':22} no data ({g['missing']} environments without an arrival)")
                continue
            s = f"{k + ':':22} {g['mean']:12.3f}{_interval(g)}  min {g['min']:.3f}  max {g['max']:.3f}  n {g['n']}"
            if g["missing"]:
                s += f"  ({g['missing']} without an arrival left out)"
            out.append(s)
        return out


def summarise(counts, sums, episode_return, hist, frames, bin_width):
    """Host side of the report: the kernel's per-environment numbers (numpy arrays) -> the per-environment lists of
    :class:`EvalResult` and their aggregates."""
    K = counts.shape[0]
    per = {k: [] for k in PER_ENV_KEYS}
    for b in range(K):
        n = int(counts[b, 0])
        per["episode_return"].append(float(episode_return[b]))
        per["frames"].append(int(frames))
        per["arrived"].append(n)
        per["on_way"].append(int(counts[b, 1]))
        per["not_departed"].append(int(counts[b, 2]))
        if n == 0:
            for k in ("avg_travel_time", "std_travel_time", "max_travel_time", "p50_travel_time", "p95_travel_time"):
                per[k].append(None)
            continue
        mean = float(sums[b, 0]) / n
        per["avg_travel_time"].append(mean)
        per["std_travel_time"].append(math.sqrt(max(0.0, float(sums[b, 1]) / n - mean * mean)))
        per["max_travel_time"].append(float(sums[b, 2]))
        per["p50_travel_time"].append(hist_percentile(hist[b], 0.50, bin_width))
        per["p95_travel_time"].append(hist_percentile(hist[b], 0.95, bin_width))
    agg = {k: aggregate(v) for k, v in per.items()}
    return per, agg, sum(1 for n in per["arrived"] if n == 0)


PAIRED_METRICS = (("episode_return", "episode_return"), ("arrivals", "arrived"), ("mean_travel_time", "avg_travel_time"),
                  ("p50_travel_time", "p50_travel_time"), ("p95_travel_time", "p95_travel_time"))
_PAIRED_SETTINGS = ("seed", "env_base", "bin_width", "num_bins")


def paired_report(a: EvalResult, b: EvalResult) -> dict:
    """Per-environment differences a - b of two evaluations of the SAME environments (same K, seed, env_base and bins,
    and for two completed runs the same ``frames_run``: ``ValueError`` otherwise) — e.g. a policy against the
    ``"dijkstra"`` baseline under common random numbers.
    Per metric of :data:`PAIRED_METRICS`: ``n`` usable pairs (a travel-time metric uses only the environments where BOTH
    runs had an arrival), the mean of the differences, their sample standard deviation (ddof = 1), ``se = std / sqrt(n)``
    and ``ci95 = mean -+ 1.96 se``, a NORMAL-APPROXIMATION interval; std, se and ci95 are ``None`` for n < 2, the mean too
    for n = 0. A run that left the domain has no statistics: ``{"available": False, "reason": ...}`` and no numbers."""
    if a.envs != b.envs:
        raise ValueError(f"paired_report needs the same environments: envs {a.envs} / {b.envs}")
    for k in _PAIRED_SETTINGS:
        if a.settings.get(k) != b.settings.get(k):
            raise ValueError(f"paired_report needs equal {k}: {a.settings.get(k)!r} / {b.settings.get(k)!r}")
    head = {"a": a.head, "b": b.head, "envs": a.envs}
    if a.domain_exit or b.domain_exit:      # (such a run stopped early: its frames_run is not compared)
        who = " and ".join(f"{n} ({r.head})" for n, r in (("a", a), ("b", b)) if r.domain_exit)
        return dict(head, available=False, reason=f"domain exit in {who}: a run that left the domain has no statistics")
    if a.frames_run != b.frames_run:
        raise ValueError(f"paired_report needs the same frames: frames_run {a.frames_run} / {b.frames_run}")
    head["frames_run"] = a.frames_run
    metrics = {}
    both_trip = a.trip_return is not None and b.trip_return is not None      # (a row of its own where both runs have it)
    for name, key in PAIRED_METRICS + ((("trip_return", "trip_return"),) if both_trip else ()):
        d = np.asarray([x - y for x, y in zip(getattr(a, key), getattr(b, key)) if x is not None and y is not None],
                       dtype=np.float64)
        metrics[name] = {"n": int(d.size), "dropped": int(a.envs - d.size), **_sample_moments(d), "ci95_kind": _CI95_KIND}
    return dict(head, available=True, metrics=metrics)


def paired_lines(report: dict):
    """:func:`paired_report` as printable lines."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    out = []
    for name, m in report["metrics"].items():
        if m["mean"] is None:
            out.append(f"{name + ':':22} no usable pair")
            continue
        s = f"{name + ':':22} {m['mean']:12.3f}{_interval(m)}  n {m['n']}"
        if m["dropped"]:
            s += f"  ({m['dropped']} environments without an arrival in one of the runs left out)"
        out.append(s)
    return out


def paired_scalars(report: dict):
    """The numbers of :func:`paired_report` as flat ``metric/field`` scalars (the trainer's log records)."""
    if not report["available"]:
        return {"available": 0}
    out = {"available": 1}
    for name, m in report["metrics"].items():
        out[f"{name}/n"] = m["n"]
        for k in ("mean", "se"):
            if m[k] is not None:
                out[f"{name}/{k}"] = m[k]
    return out


class _BinSchedule(namedtuple("_BinSchedule", "t0 timestep bin_seconds first_bin H")):
    """The time bins of one run: frame f starts at clock ``t0 + f * timestep`` and belongs to the stored bin
    ``clock // bin_seconds - first_bin`` of the ``H`` that the run's frames reach."""

    def block(self, done, size):
        """The clock and bin arguments of the accumulate call for the ring block of ``size`` frames that ends at frame
        ``done``, the run's last one perhaps partial."""
        f0 = (done - 1) - (done - 1) % size
        return dict(t0=self.t0 + f0 * self.timestep, timestep=self.timestep, bin_seconds=self.bin_seconds,
                    first_bin=self.first_bin, frames=done - f0)


def _due(done, every, T):      # after `done` of T frames: a block of `every` frames is full, or the run is over
    return done % every == 0 or done == T


def router_buffers(eng, baseline_dests=None, tables=None):
    """The shortest-path routers' buffers on engine ``eng``, shared by the evaluator's router heads and the behaviour-cloning
    expert (tarl_hip.imitation): -> (dests int64 (D,), dest_slot int32 (N,), travel times (K, E), the next-hop table
    (``tables`` or K, D, N) filled with -1, the tree scratch (O(min(K D, 1024) N))). ``baseline_dests`` = (dests, dest_slot)
    of src.agents.base.destination_set over the engine's agent tables (default: computed here by the same rule). Refused
    beyond half the free device memory, like the graph-transformer critic's store."""
    N, E, dev = eng.N, eng.E, eng.device
    K = eng.B if tables is None else int(tables)
    if baseline_dests is None:      # src.agents.base.destination_set's rule: every distinct DESTINATION, row 0 included
        d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
        d = d[(d >= 0) & (d < N)].contiguous()
        slot = torch.full((N,), -1, dtype=torch.int32, device=dev)
        slot[d] = torch.arange(d.numel(), dtype=torch.int32, device=dev)
        baseline_dests = (d, slot)
    dests, dest_slot = baseline_dests
    D = int(dests.numel())
    table_bytes, scratch_bytes = ops.destination_trees_batched_bytes(eng.plan, K, D)
    if scratch_bytes < 0:
        raise _lib.TarlError("tarl_dest_trees_batched_scratch_bytes refused the evaluator's sizes")
    free = int(torch.cuda.mem_get_info(dev)[0])
    if table_bytes + scratch_bytes > free // 2:
        raise _lib.TarlError(f"the shortest-path baseline's next-hop table ({table_bytes / 2**30:.2f} GiB for K = {K} "
                             f"environments x D = {D} destinations x N = {N} nodes) and tree scratch "
                             f"({scratch_bytes / 2**30:.2f} GiB) exceed half the free device memory "
                             f"({free / 2**30:.2f} GiB free): evaluate fewer environments at a time")
    weights = torch.empty((eng.B, E), dtype=torch.float32, device=dev)
    table = torch.full((K, D, N), -1, dtype=torch.int32, device=dev)
    return dests, dest_slot, weights, table, torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device=dev)


def refresh_router_tables(eng, t, refresh_rate, weights, dests, table, scratch):
    """The shortest-path routers' refresh in front of frame ``t``, shared by the evaluator's router heads and the behaviour-
    cloning expert (tarl_hip.imitation): every ``refresh_rate`` frames (0: at frame 0 only) the K environments' congested
    travel times (``weights`` (K, E)) and their next-hop trees (``table`` (K, D, N)) are rebuilt. -> whether it ran."""
    if not (t == 0 if refresh_rate == 0 else t % refresh_rate == 0):
        return False
    ops.fused_edge_travel_time(eng.plan, eng.fs, out=weights)
    ops.destination_trees_batched(eng.plan, weights, dests, out=table, scratch=scratch)
    return True


class VecEvaluator:
    def __init__(self, engine, head="embedding", *, emb=None, temperature=1.0, edge_mlp=None, prior_table=None,
                 dest_slot=None, prior_weight=1.0, gt_pe=None, gt_weights=None, bin_width=10.0, num_bins=720, poll_frames=64,
                 keep_actions=False, refresh_rate=10, baseline_dests=None, link_counts=False, link_bin_seconds=3600,
                 link_block=None, occupancy=False, occupancy_block=None, trips=False, trip_free_flow=None, dynamic_gap=False,
                 dynamic_gap_envs=None, turns=False, turn_block=None, routes=None, route_fallback=True, policy_hold=False,
                 goal_mlp=None, goal_scale=None, route_departures=False, trip_reward=False, paths=False, path_max_hops=None,
                 path_weights=None):
        """``engine``: a fused :class:`SimEngine` with K environments. ``emb``: flat (num_embeddings,) fp32 embedding
        (MPNNPolicyNet.nodes_embedding.weight); ``edge_mlp``: ops.EdgeMlpWeights (edge_mlp* heads); ``prior_table`` (N, N),
        or (N, D) with ``dest_slot`` (embedding_dijkstra); ``gt_pe`` (N, 16) and ``gt_weights``: ops.GtWeights
        (graph_transformer); ``goal_mlp``: ops.GoalMlpWeights with ``goal_scale`` (ops.goal_time_scale) and the prior head's
        ``prior_table`` / ``dest_slot`` (goal_mlp). The tensors are read at every frame: views of live parameters evaluate the
        current policy.
        ``keep_actions``: also record every frame's action bytes in ``actions`` (T, K, N) uint8 (tests).
        Heads ``"dijkstra"`` and ``"dijkstra_hold"`` (the shortest-path baselines, no ``emb``; the second holds a head one
        road short of its destination, module docstring): ``refresh_rate`` frames between two rebuilds of the K
        per-environment next-hop tables, for ``"dijkstra_hold"`` also 0 = built at frame 0 only (the free-flow router); ``baseline_dests`` = (dests int64 (D,), dest_slot int32 (N,)) of
        src.agents.base.destination_set over the engine's agent tables (default: computed here by the same rule). The
        (K, D, N) int32 table and the tree scratch are allocated once; more than half the free device memory is refused.
        Head ``"routes"`` (no ``emb``): ``routes`` = (routes int32 (A, L) or (K, A, L), route_len int32 (A,) or (K, A)) of
        ``ops.td_routes``, held by reference and read at every frame (:meth:`set_routes` swaps it); ``route_fallback``: the
        free-flow hold router writes every row before the plan does (module docstring; ``baseline_dests`` as for the routers).
        ``link_counts``: also count, per environment, road and time bin of ``link_bin_seconds``, the frames in which the
        road's head was popped plus those in which an agent was withdrawn from it (the reference's compute_node_metrics /
        plot_daily_counts, src/transportation_simulator.py:563-746). The frames write their two masks into rings of
        ``link_block`` frames (default: the largest block <= ``poll_frames`` and <= ops.LINK_COUNTS_MAX_FRAMES that keeps
        both rings within 256 MB, at least 1) and one ``ops.link_counts_accumulate`` launch follows every block.
        ``occupancy``: also sum, per environment, road and time bin of ``link_bin_seconds`` (both per-road reports share one
        binning), the road's NUMBER_OF_AGENT after every frame, count the frames in which it was at capacity
        (:func:`capacity_threshold` of the engine's static MAX column, computed once on the host) and keep its peak. The
        frames write their ``counts`` slice into an fp32 ring (F, N, K) of ``occupancy_block`` frames (default: the largest
        block <= ``poll_frames`` that keeps the ring within 256 MB, at least 1) and one ``ops.occupancy_accumulate`` launch
        follows every block. Without the flag nothing is allocated and every frame is called as it always was.
        ``trips``: after the episode also reduce the K agent tables per agent over the environments
        (``ops.trip_agent_stats``) and per environment and time bin of ``link_bin_seconds`` over the agents
        (``ops.trip_bin_stats``): two calls after ``ops.episode_summary``, none per frame. ``run()`` refuses environments
        whose ORIGIN, DESTINATION or DEPARTURE_TIME differ (per-agent statistics over different populations mean nothing).
        ``trip_free_flow`` fp32 (E,): free-flow edge weights; the free-flow time of every agent
        (:func:`trip_free_flow_times`, one ``ops.destination_trees`` pass here) then serves as the reference for its delay.
        ``dynamic_gap``: after the episode also measure every completed trip against the best path in hindsight under the
        time-dependent road times the episode produced: the occupancy accumulators run internally (without
        ``occupancy=True`` the result carries no ``occupancy`` report), ``run()`` checks the population as for ``trips``, and
        for the first ``dynamic_gap_envs`` environments (default: all K) one ``ops.td_road_times`` and one
        ``ops.td_hindsight`` call follow the episode summary, reduced in fp64 on the device. ``run()`` refuses before the
        first frame what does not fit half the free device memory.
        ``turns``: also count, per environment, ROUTE EDGE u -> v and time bin of ``link_bin_seconds``, the vehicles that
        crossed the edge, and per road the agents the reference's U-turn double pop loses. The frames write their
        ``popped`` and ``counts`` slices into rings of ``turn_block`` frames (default: the largest block <= ``poll_frames``
        that keeps the three rings within 256 MB, at least 1; the counts ring is the occupancy ring where that one is on and
        has the same block), the SELECTED_ROAD bytes are copied into the third after every frame, and one
        ``ops.turn_counts_accumulate`` launch follows every block. ``run()`` sizes the (K, H, E) and (K, H, N) tables and
        refuses what exceeds half the free device memory; it raises when a pop could not be attributed to an edge or when
        the lost agents do not add up to the ON_WAY agents that are queued nowhere.
        ``policy_hold`` (an action shield, NOT in the reference; policy heads only — the routers and the plan have
        their own rule): after the head has written a frame's action, a row with a non-empty FIFO whose chosen road IS its
        head agent's destination selects itself instead (``ops.fused_hold_policy_actions``), so that the environment's step
        order withdraws the agent there instead of stranding it on its destination road. ``actions`` stays the policy's own
        choice; ``EvalResult.held`` counts the held rows per environment. Unlike the routers' rule an empty row is never
        touched. The ``"embedding"`` head then takes the per-frame path of the state-dependent heads: its logits are computed
        once and broadcast, the action is drawn per frame (``ops.graphdist_mode_rollout`` / ``ops.graphdist_rollout``), then
        the hold launch and ``frame_fused(skip_choice=True)``. Off, every head runs as it always did.
        ``route_departures`` (an environment-side rule, NOT in the reference; every head but ``"dijkstra"``):
        after the head (and the hold launch) has written a frame's action, every EMPTY road with an agent ready to depart
        from it selects for that agent — the smallest ready id of the origin — instead of for the dummy head agent 0
        (``ops.fused_pending_departures`` + ``ops.fused_route_departures``). ``"dijkstra_hold"`` looks the first hop up in
        its own tables, ``"routes"`` in the plan (its fallback's byte stays where the plan has nothing), a policy head in
        a free-flow per-destination table built once at frame 0 (``baseline_dests`` as for the routers). A non-empty
        origin road keeps its head's choice. ``actions`` stays the head's own choice; ``EvalResult.departures_routed``
        counts the rows written per environment. The ``"embedding"`` head takes its per-frame path, as under
        ``policy_hold``.
        ``trip_reward`` (NOT in the reference; every head, the routers and ``"routes"`` included): after every
        frame one ``ops.fused_trip_reward`` call writes -(on_way + ready) of that frame's clock into a SECOND (T, K) buffer
        and {on_way, ready} into a (T, K, 2) one. The queue ``reward`` buffer, ``episode_return`` and everything read from
        them stay exactly as they are; ``EvalResult.trip_return`` is the sum over the frames per environment (float64 on the
        host), ``trip_parts_last`` the two counts after the last frame, ``aggregate["trip_return"]`` its mean, standard
        error and interval. The frames themselves do not change.
        ``paths`` (NOT in the reference; every head, the routers and ``"routes"`` included): the per-agent path
        trace. ``run()`` resets its state before the first frame and queues one ``ops.fused_path_trace`` after every frame,
        after every other launch of that frame: which roads every (environment, agent) was seen on as a FIFO head, up to
        ``path_max_hops`` kept per trace (default 64; 0 keeps no routes), how many, the free-flow cost of the hops and how
        much of it was detour. ``path_weights`` fp32 (E,): the edge weights of cost and detour (default: ``trip_free_flow``
        where that is given, else none — the trace then counts roads only); the fp64 distances come from one
        ``ops.destination_trees(want_dist=True)`` pass here over the distinct destinations of the agent tables
        (``baseline_dests`` as for the routers). A route array that exceeds half the free device memory is refused here, with
        its size; a distance table that does (measured after the route array is allocated) is left out, and with it the
        weights, which the launch takes only together with it: the trace then counts roads and loops only and the report
        says "path cost and excess not available". After the episode
        summary one ``ops.path_agent_stats`` call; ``run()`` raises when the trace met what must not happen (``bad``: a head id
        beyond the agent table, two sightings no edge connects) and checks the population as for ``trips``. The frames
        themselves do not change; without the flag nothing is allocated and nothing is queued."""
        if engine.fs is None:
            raise _lib.TarlError("VecEvaluator needs the fused engine (ops.fused_path_supported): the packed state cannot "
                                 "represent this graph and there is no fall-back")
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}")
        if head in _MLP_PRECISION and edge_mlp is None:
            raise ValueError(f"head {head!r} needs edge_mlp (ops.EdgeMlpWeights)")
        if head == "embedding_dijkstra" and prior_table is None:
            raise ValueError("head 'embedding_dijkstra' needs prior_table (and dest_slot for a per-destination table)")
        if head == "goal_mlp" and (prior_table is None or goal_mlp is None or goal_scale is None):
            raise ValueError("head 'goal_mlp' needs goal_mlp (ops.GoalMlpWeights), goal_scale and prior_table (and dest_slot "
                             "for a per-destination table)")
        if head == "graph_transformer" and (gt_pe is None or gt_weights is None):
            raise ValueError("head 'graph_transformer' needs gt_pe and gt_weights")
        if head in PLAN_HEADS and routes is None:
            raise ValueError(f"head {head!r} needs routes = (routes, route_len) of ops.td_routes")
        if routes is not None and head not in PLAN_HEADS:
            raise ValueError(f"routes is the plan of the heads {PLAN_HEADS}: head {head!r} does not read it")
        if head not in ROUTER_HEADS + PLAN_HEADS and emb is None:
            raise ValueError(f"head {head!r} needs emb (the flat embedding tensor)")
        if policy_hold and head in ROUTER_HEADS + PLAN_HEADS:
            raise ValueError(f"policy_hold is the hold rule for POLICY heads: head {head!r} has its own rule "
                             "('dijkstra_hold' and 'routes' hold one road short of the destination themselves)")
        if route_departures and head == "dijkstra":
            raise ValueError("route_departures is not for head 'dijkstra': the reference-order router stays the reference's "
                             "(use 'dijkstra_hold', or its free-flow form with refresh_rate=0)")
        if int(poll_frames) < 1:
            raise ValueError("poll_frames must be >= 1")
        if int(refresh_rate) < (0 if head == "dijkstra_hold" else 1):
            raise ValueError("refresh_rate must be >= 1 (head 'dijkstra_hold' also takes 0: tables built at frame 0 only)")
        self.eng, self.head = engine, head
        self.emb = emb
        self.temperature = float(temperature)
        self.edge_mlp, self.prior_table, self.dest_slot = edge_mlp, prior_table, dest_slot
        self.prior_weight, self.gt_pe, self.gt_weights = float(prior_weight), gt_pe, gt_weights
        self.goal_mlp, self.goal_scale = goal_mlp, goal_scale
        self.bin_width, self.num_bins, self.poll_frames = float(bin_width), int(num_bins), int(poll_frames)
        self.keep_actions = bool(keep_actions)
        self.policy_hold = bool(policy_hold)
        self.route_departures = bool(route_departures)
        self.trip_reward = bool(trip_reward)
        self.trip_rw = self.trip_parts = None       # (T, K) fp32 and (T, K, 2) int32, reserved with the reward buffer
        self._per_frame_draw = self.policy_hold or self.route_departures     # "embedding": drawn per frame, as the other heads
        self.refresh_rate = int(refresh_rate)
        K, N, E, dev = engine.B, engine.N, engine.E, engine.device
        plan = engine.plan
        self.link_counts, self.occupancy, self.trips = bool(link_counts), bool(occupancy), bool(trips)
        self.dynamic_gap = bool(dynamic_gap)
        if dynamic_gap_envs is not None and not self.dynamic_gap:
            raise ValueError("dynamic_gap_envs limits the environments of the dynamic gap: it needs dynamic_gap=True")
        if self.dynamic_gap:
            self.dynamic_gap_envs = K if dynamic_gap_envs is None else int(dynamic_gap_envs)
            if not 1 <= self.dynamic_gap_envs <= K:
                raise ValueError(f"dynamic_gap_envs must be in [1, {K}] (the engine's environments), got {dynamic_gap_envs!r}")
        self._occ_acc_on = self.occupancy or self.dynamic_gap      # the gap reads the occupancy sums: accumulated either way
        self.turns = bool(turns)
        if turn_block is not None and not self.turns:
            raise ValueError("turn_block sizes the rings of the turn counts: it needs turns=True")
        self.paths = bool(paths)
        if not self.paths and (path_max_hops is not None or path_weights is not None):
            raise ValueError("path_max_hops and path_weights configure the per-agent path trace: they need paths=True")
        if self.link_counts or self._occ_acc_on or self.trips or self.turns or self.paths:      # one binning for every binned report
            self.link_bin_seconds = int(link_bin_seconds)
            if self.link_bin_seconds < 1:
                raise ValueError("link_bin_seconds must be >= 1")
        if self.link_counts:
            if link_block is None:
                link_block = self._ring_block(LINK_RING_BYTES, 2 * K * N, ops.LINK_COUNTS_MAX_FRAMES)
            self.link_block = int(link_block)
            if not 1 <= self.link_block <= ops.LINK_COUNTS_MAX_FRAMES:
                raise ValueError(f"link_block must be in [1, {ops.LINK_COUNTS_MAX_FRAMES}] (ops.LINK_COUNTS_MAX_FRAMES)")
            self.link_popped = torch.zeros((self.link_block, K, N), dtype=torch.uint8, device=dev)
            self.link_withdrawn = torch.zeros((self.link_block, K, N), dtype=torch.uint8, device=dev)
            self.link_acc = None        # (K, H, N) int32, sized by run() for its frames
        if self._occ_acc_on:
            if occupancy_block is None:
                occupancy_block = self._ring_block(OCCUPANCY_RING_BYTES, 4 * K * N)
            self.occupancy_block = int(occupancy_block)
            if not 1 <= self.occupancy_block <= ops.OCCUPANCY_MAX_FRAMES:
                raise ValueError(f"occupancy_block must be in [1, {ops.OCCUPANCY_MAX_FRAMES}] (ops.OCCUPANCY_MAX_FRAMES)")
            self.occ_ring = torch.zeros((self.occupancy_block, N, K), dtype=torch.float32, device=dev)
            self.occ_max = engine.static_node_features[0, :, 0].detach().cpu().numpy().astype(np.float64)
            self.occ_thr_host = capacity_threshold(self.occ_max)
            self.occ_thr = torch.from_numpy(self.occ_thr_host).to(dev)
            self.occ_acc = None         # veh, full (K, H, N) and peak (K, 1, N) int32, sized by run() for its frames
        if self.turns:
            if turn_block is None:
                turn_block = self._ring_block(TURN_RING_BYTES, 6 * K * N)
            self.turn_block = int(turn_block)
            if not 1 <= self.turn_block <= ops.TURN_COUNTS_MAX_FRAMES:
                raise ValueError(f"turn_block must be in [1, {ops.TURN_COUNTS_MAX_FRAMES}] (ops.TURN_COUNTS_MAX_FRAMES)")
            self.turn_popped = torch.zeros((self.turn_block, K, N), dtype=torch.uint8, device=dev)
            self.turn_sel = torch.zeros((self.turn_block, N, K), dtype=torch.uint8, device=dev)
            if self._occ_acc_on and self.occupancy_block == self.turn_block:
                self.turn_ring = self.occ_ring      # one counts ring serves both
            else:
                self.turn_ring = torch.zeros((self.turn_block, N, K), dtype=torch.float32, device=dev)
            self.turn_prev = torch.zeros((N, K), dtype=torch.float32, device=dev)      # the block before's last counts slice
            self.turn_acc = None        # turns (K, H, E), lost (K, H, N), unresolved (K,) int32, sized by run()
        if self.trips:
            self.trip_ff = None if trip_free_flow is None else trip_free_flow_times(engine, trip_free_flow)
        elif trip_free_flow is not None:
            raise ValueError("trip_free_flow is the reference of the per-trip report: it needs trips=True")
        if self.paths:
            self._init_paths(path_max_hops, trip_free_flow if path_weights is None else path_weights, baseline_dests)
        # scratch, allocated once
        self.log_prob = torch.zeros(K, dtype=torch.float32, device=dev)
        self.action8 = torch.zeros((K, N), dtype=torch.uint8, device=dev)          # the last frame's action bytes
        self.summary = {"counts": torch.zeros((K, 3), dtype=torch.int32, device=dev),
                        "sums": torch.zeros((K, 3), dtype=torch.float64, device=dev),
                        "episode_return": torch.zeros(K, dtype=torch.float64, device=dev),
                        "hist": torch.zeros((K, self.num_bins), dtype=torch.int32, device=dev)}
        self.reward = self.actions = self._flag_host = None
        if self.policy_hold:
            self.held = torch.zeros(K, dtype=torch.int32, device=dev)       # rows held, per environment, in this run
        if self.route_departures:
            self.pend = torch.empty((N, K), dtype=torch.int32, device=dev)  # smallest ready agent id per origin road, or -1
            self.routed = torch.zeros(K, dtype=torch.int32, device=dev)     # rows routed, per environment, in this run
            if head not in ROUTER_HEADS + PLAN_HEADS:   # a policy head: one free-flow table, built at frame 0 as 'free_flow' builds its own
                self.dep_dests, self.dep_slot, self.dep_weights, self.dep_table, self.dep_scratch = \
                    router_buffers(engine, baseline_dests, 1)
        if head == "embedding":
            self.mode8 = torch.zeros((1, N), dtype=torch.uint8, device=dev)
            self.mode_lp = torch.zeros(1, dtype=torch.float32, device=dev)
            if self._per_frame_draw:    # the per-frame path: the logits of every environment, and the sampler's scratch
                self.logits = torch.empty((K, E), dtype=torch.float32, device=dev)
                need = int(_lib.load().tarl_graphdist_rollout_scratch_bytes(plan.handle, K))
                self.dist_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        elif head in ROUTER_HEADS:
            self._init_baseline(baseline_dests)
        elif head in PLAN_HEADS:
            self.set_routes(*routes)
            self.route_fallback = bool(route_fallback)
            if self.route_fallback:
                self._init_baseline(baseline_dests, tables=1)
        else:
            self.logits = torch.empty((K, E), dtype=torch.float32, device=dev)
            need = int(_lib.load().tarl_graphdist_rollout_scratch_bytes(plan.handle, K))
            self.dist_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
            if head == "edge_mlp_bf16":
                self.obs = torch.empty((K, N, 16), dtype=torch.bfloat16, device=dev)
            elif head not in ("embedding_dijkstra", "goal_mlp"):
                self.obs = torch.empty((K, N, 16), dtype=torch.float32, device=dev)
            if head == "graph_transformer":
                n = int(_lib.load().tarl_policy_gt_fwd_scratch_floats(plan.handle, K))
                self.gt_scratch = torch.empty(n, dtype=torch.float32, device=dev)

    def _init_paths(self, max_hops, weights, baseline_dests):
        """The state of the path trace and, with ``weights``, the distance table of its detour measure: once per evaluator."""
        eng = self.eng
        K, A, N, dev = eng.B, eng.A, eng.N, eng.device
        L = 64 if max_hops is None else int(max_hops)
        if not 0 <= L <= ops.PATH_MAX_HOPS:
            raise ValueError(f"path_max_hops must be in [0, {ops.PATH_MAX_HOPS}] (ops.PATH_MAX_HOPS), got {max_hops!r}")
        free = int(torch.cuda.mem_get_info(dev)[0])
        need = 4 * K * A * L
        if need > free // 2:
            raise _lib.TarlError(f"the path trace's route array ({need / 2**30:.2f} GiB for K = {K} environments x A = {A} agents "
                                 f"x path_max_hops = {L}) exceeds half the free device memory ({free / 2**30:.2f} GiB free): "
                                 f"evaluate fewer environments at a time or keep fewer roads per trace")
        self.path_state = ops.path_trace_state(K, A, L, dev)
        free = int(torch.cuda.mem_get_info(dev)[0])      # what is left beside the state
        self.path_w = self.path_dist = self.path_slot = self.path_note = None
        if weights is None:
            return
        w = weights.detach().to(dev, torch.float32).reshape(-1).contiguous()
        if w.numel() != eng.E:
            raise ValueError(f"path_weights must hold one weight per edge ({eng.E}), got {w.numel()}")
        if baseline_dests is None:      # src.agents.base.destination_set's rule, as router_buffers applies it
            d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
            d = d[(d >= 0) & (d < N)].contiguous()
            slot = torch.full((N,), -1, dtype=torch.int32, device=dev)
            slot[d] = torch.arange(d.numel(), dtype=torch.int32, device=dev)
            baseline_dests = (d, slot)
        dests, slot = baseline_dests
        need = 8 * int(dests.numel()) * N
        if need > free // 2:
            self.path_note = (f"path cost and excess not available: the distance table ({need / 2**30:.2f} GiB for D = "
                              f"{int(dests.numel())} destinations x N = {N} roads), without which the launch takes no weights, "
                              f"exceeds half the free device memory ({free / 2**30:.2f} GiB free)")
            return
        if dests.numel() == 0:
            self.path_note = "path cost and excess not available: no destination in range"
            return
        _, self.path_dist = ops.destination_trees(eng.plan, w, dests.contiguous(), want_next_hop=False, want_dist=True)
        self.path_w, self.path_slot = w, slot.contiguous()

    def _ring_block(self, ring_bytes, frame_bytes, cap=None):
        """The default block of a ring of per-frame slices: the most frames that fit ``ring_bytes``, at most ``poll_frames``
        (and ``cap``, where one call of the accumulate kernel takes no more), at least 1."""
        block = min(self.poll_frames, ring_bytes // frame_bytes)
        return max(1, block if cap is None else min(block, cap))

    def _init_baseline(self, baseline_dests, tables=None):
        """The baseline's buffers, once per evaluator (:func:`router_buffers`). ``tables``: the environments that get a table of
        their own (default: all K; 1 for the "routes" head's fallback, whose one table is built from environment 0's empty
        network)."""
        self.dests, self.dest_slot, self.weights, self.table, self.tree_scratch = router_buffers(self.eng, baseline_dests, tables)

    def set_routes(self, routes, route_len):
        """The plan the ``"routes"`` head follows from the next frame on: ``routes`` int32 (A, L) with ``route_len`` (A,)
        — one plan for every environment — or (K, A, L) with (K, A). Held by reference; nothing is copied or rebuilt."""
        if self.head not in PLAN_HEADS:
            raise ValueError(f"set_routes is for the heads {PLAN_HEADS}, not {self.head!r}")
        K, A = self.eng.B, self.eng.A
        for t, name in ((routes, "routes"), (route_len, "route_len")):
            if not t.is_cuda:
                raise _lib.TarlError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
            if t.dtype != torch.int32 or not t.is_contiguous():
                raise TypeError(f"{name} must be a contiguous int32 tensor")
        if routes.dim() not in (2, 3) or tuple(routes.shape[:-1]) not in ((A,), (K, A)) or routes.size(-1) < 1 or \
                tuple(route_len.shape) != tuple(routes.shape[:-1]):
            raise ValueError(f"routes must be ({A}, L) or ({K}, {A}, L) and route_len the same without L, got "
                             f"{tuple(routes.shape)} and {tuple(route_len.shape)}")
        self.routes, self.route_len = routes, route_len

    @classmethod
    def from_policy_net(cls, engine, policy_net, prior_dests=None, **kw):
        """The evaluator of an ``MPNNPolicyNet`` (src/agents/mpnn_agent.py) under its ``policy_head``; the parameter tensors
        are held as views, so later optimiser steps (in place) are seen. ``prior_dests``: for the per-destination prior,
        ``(dests, dest_slot)`` of src.agents.base.destination_set over the engine's agent tables."""
        head = getattr(policy_net, "policy_head", "embedding")
        args = dict(emb=policy_net.nodes_embedding.weight.data.reshape(-1), prior_weight=getattr(policy_net, "prior_weight", 1.0))
        if head in _MLP_PRECISION:
            m = policy_net.edge_mlp
            args["edge_mlp"] = ops.EdgeMlpWeights(*(p.data for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias,
                                                                    m[4].weight, m[4].bias)))
        elif head == "embedding_dijkstra":
            if policy_net.resolve_prior_method() == "all_pairs":
                args["prior_table"] = policy_net.dist_matrix
            else:       # one column per destination of every environment's agent table, as the trainer builds it
                from .trainer import VecPPOTrainer
                if prior_dests is None:
                    raise ValueError("the per-destination prior needs prior_dests = destination_set(engine.agents, N)")
                args["prior_table"], args["dest_slot"] = VecPPOTrainer._build_prior_dest(
                    engine, policy_net.free_flow_weights(), *prior_dests)
        elif head == "goal_mlp":
            m = policy_net.goal_mlp
            args["goal_mlp"] = ops.GoalMlpWeights(*(p.data for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)))
            args["goal_scale"] = float(policy_net.goal_scale)
            if policy_net.resolve_prior_method() == "all_pairs":
                args["prior_table"] = policy_net.dist_matrix
            else:
                from .trainer import VecPPOTrainer
                if prior_dests is None:
                    raise ValueError("the per-destination table needs prior_dests = destination_set(engine.agents, N)")
                args["prior_table"], args["dest_slot"] = VecPPOTrainer._build_prior_dest(
                    engine, policy_net.free_flow_weights(), *prior_dests)
        elif head == "graph_transformer":
            args["gt_pe"] = policy_net.gt_pe
            args["gt_weights"] = ops.GtWeights(policy_net.transformer.kernel_tensors())
        args.update(kw)
        return cls(engine, head, **args)

    # -- sizes ---------------------------------------------------------------------------------------------------------
    @property
    def episode_frames(self):
        """Frames from a reset until the episode ends: the frame whose step pushes the clock past EPISODE_END is the last
        (``break_when_any_done=True`` of the reference's rollout)."""
        return int((EPISODE_END - EPISODE_START) // self.eng.timestep + 1)

    def _reserve(self, T):
        K, N, dev = self.eng.B, self.eng.N, self.eng.device
        if self.reward is None or self.reward.size(0) < T:
            self.reward = torch.zeros((T, K), dtype=torch.float32, device=dev)
            self._flag_host = torch.zeros(T // self.poll_frames + 2, dtype=torch.int32).pin_memory()
            if self.keep_actions:
                self.actions = torch.zeros((T, K, N), dtype=torch.uint8, device=dev)
        if self.trip_reward and (self.trip_rw is None or self.trip_rw.size(0) < T):
            self.trip_rw = torch.zeros((T, K), dtype=torch.float32, device=dev)
            self.trip_parts = torch.zeros((T, K, 2), dtype=torch.int32, device=dev)

    # -- the action of one frame -----------------------------------------------------------------------------------------
    def _logits(self):
        eng, plan, fs = self.eng, self.eng.plan, self.eng.fs
        if self.head == "embedding_dijkstra":
            return ops.fused_prior_logits(plan, fs, eng._x, eng.Nmax, eng.agents, self.emb, self.prior_table,
                                          self.prior_weight, out=self.logits, dest_slot=self.dest_slot)
        if self.head == "goal_mlp":
            return ops.fused_goal_mlp_logits(plan, fs, eng._x, eng.Nmax, eng.agents, self.goal_mlp, self.prior_table,
                                             self.goal_scale, dest_slot=self.dest_slot, out=self.logits)
        if self.head == "edge_mlp_bf16":
            obs = ops.fused_obs16_bf16(plan, fs, eng._x, eng.Nmax, eng.agents, out=self.obs)
            return ops.policy_edge_mlp(plan, obs, eng.ec, self.edge_mlp, out=self.logits)
        obs = ops.fused_obs16(plan, fs, eng._x, eng.Nmax, eng.agents, out=self.obs)
        if self.head == "graph_transformer":
            return ops.policy_gt_logits(plan, obs, eng.ec, self.gt_pe, self.gt_weights, out=self.logits,
                                        scratch=self.gt_scratch)
        return ops.policy_edge_mlp(plan, obs, eng.ec, self.edge_mlp, precision=_MLP_PRECISION[self.head], out=self.logits)

    def _start(self, deterministic):
        """Once per run, after the reset. The embedding head is state-independent: its MODE action is computed once (B = 1)
        and loaded into every environment's SELECTED_ROAD bytes, which the frames leave alone; sampled, the engine draws
        from its own tables."""
        if self.policy_hold:
            self.held.zero_()
        if self.route_departures:
            self.routed.zero_()
        if self.head != "embedding":
            return      # (the baseline builds its tables at frame 0: 0 % refresh_rate == 0)
        eng = self.eng
        if self._per_frame_draw:        # drawn per frame, so that the rules see every frame's state: logits once, broadcast
            logits = ops.policy_edge_logits(eng.plan, eng.static_node_features[0], self.emb).view(1, -1)
            self.logits.copy_(logits.expand_as(self.logits))
            return
        if deterministic:
            logits = ops.policy_edge_logits(eng.plan, eng.static_node_features[0], self.emb).view(1, -1)
            ops.graphdist_mode_rollout(eng.plan, logits, self.temperature, choice8=self.mode8, log_prob=self.mode_lp)
            self.action8.copy_(self.mode8.expand_as(self.action8))
            self.log_prob.copy_(self.mode_lp.expand_as(self.log_prob))
            ops.fused_set_actions(eng.plan, eng.fs, self.action8)
        else:
            eng.prepare_policy(self.emb, self.temperature)

    def _frame(self, t, deterministic):
        eng = self.eng
        rec = self.actions[t] if self.keep_actions else None
        masks = {}
        if self.link_counts:        # this frame's slice of the two rings; without either flag the call is as it always was
            j = t % self.link_block
            masks = dict(popped=self.link_popped[j], withdrawn=self.link_withdrawn[j])
        if self._occ_acc_on:        # and of the counts ring
            masks["counts"] = self.occ_ring[t % self.occupancy_block]
        if self.turns:              # and of the turn rings: the frame writes a slice once, a second ring gets a copy
            jt = t % self.turn_block
            masks.setdefault("popped", self.turn_popped[jt])
            masks.setdefault("counts", self.turn_ring[jt])
        done = self._frame_head(t, deterministic, rec, masks)
        if self.turns:
            if masks["popped"].data_ptr() != self.turn_popped[jt].data_ptr():
                self.turn_popped[jt].copy_(masks["popped"])
            if masks["counts"].data_ptr() != self.turn_ring[jt].data_ptr():
                self.turn_ring[jt].copy_(masks["counts"])
            self.turn_sel[jt].copy_(eng.fs.sel8)        # the SELECTED_ROAD bytes this frame ran with
        return done

    def _route_departures(self, t):
        """The first-hop rule of DESIGN 4.23 on the bytes the head has just written: the pending table of this frame's clock,
        then the route launch with the head's own lookup. ``rec`` keeps the head's choice."""
        eng = self.eng
        ops.fused_pending_departures(eng.plan, eng.fs, float(eng.time), out=self.pend)
        if self.head in PLAN_HEADS:
            ops.fused_route_departures_plan(eng.plan, eng.fs, self.pend, self.routes, self.route_len, routed=self.routed)
        elif self.head in ROUTER_HEADS:
            ops.fused_route_departures(eng.plan, eng.fs, self.pend, self.dest_slot, self.table, routed=self.routed)
        else:
            if t == 0:                  # after the reset every count is 0: free-flow times, the same in every environment
                ops.fused_edge_travel_time(eng.plan, eng.fs, out=self.dep_weights)
                ops.destination_trees_batched(eng.plan, self.dep_weights[:1], self.dep_dests, out=self.dep_table,
                                              scratch=self.dep_scratch)
            ops.fused_route_departures(eng.plan, eng.fs, self.pend, self.dep_slot, self.dep_table[0], routed=self.routed)

    def _frame_head(self, t, deterministic, rec, masks):
        eng = self.eng
        if self.head in ROUTER_HEADS:   # choice -> core -> withdraw / insert -> reward: the environment's step order
            if eng._packed_stale:
                eng.resync()
            refresh_router_tables(eng, t, self.refresh_rate, self.weights, self.dests, self.table, self.tree_scratch)
            ops.fused_select_next_hop_dest(eng.plan, eng.fs, self.dest_slot, self.table, choice8=rec,
                                           hold=self.head == "dijkstra_hold")
            if self.route_departures:
                self._route_departures(t)
            return eng.frame_fused(skip_choice=True, reward=self.reward[t], **masks)
        if self.head in PLAN_HEADS:     # the same order, the choice read from the plan
            if eng._packed_stale:
                eng.resync()
            if self.route_fallback:
                if t == 0:              # after the reset every count is 0: free-flow times, the same in every environment
                    ops.fused_edge_travel_time(eng.plan, eng.fs, out=self.weights)
                    ops.destination_trees_batched(eng.plan, self.weights[:1], self.dests, out=self.table,
                                                  scratch=self.tree_scratch)
                ops.fused_select_next_hop_dest(eng.plan, eng.fs, self.dest_slot, self.table[0], hold=True)
            ops.fused_select_route(eng.plan, eng.fs, self.routes, self.route_len, choice8=rec)
            if self.route_departures:
                self._route_departures(t)
            return eng.frame_fused(skip_choice=True, reward=self.reward[t], **masks)
        if self.head == "embedding" and not self._per_frame_draw:
            if rec is not None and deterministic:
                rec.copy_(self.action8)
            return eng.frame_fused(skip_choice=deterministic, reward=self.reward[t], **masks)
        logits = self.logits if self.head == "embedding" else self._logits()
        if deterministic:
            ops.graphdist_mode_rollout(eng.plan, logits, self.temperature, choice8=rec, sel8=eng.fs.sel8,
                                       log_prob=self.log_prob)
        else:
            ops.graphdist_rollout(eng.plan, logits, self.temperature, seed=eng.seed ^ 0x5DEECE66D,
                                  counter=eng.sample_counter + 1, choice8=rec, sel8=eng.fs.sel8, log_prob=self.log_prob,
                                  scratch=self.dist_scratch)
        if self.policy_hold:            # rec keeps the policy's own choice: the rule rewrites the packed state's bytes alone
            ops.fused_hold_policy_actions(eng.plan, eng.fs, eng.agents, held=self.held)
        if self.route_departures:
            self._route_departures(t)
        return eng.frame_fused(skip_choice=True, reward=self.reward[t], **masks)

    # -- the evaluation ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self, frames=None, deterministic=True, trip_pair=None, path_pair=None):
        """Reset the engine, run ``frames`` frames (default: until the episode ends) and return an :class:`EvalResult`.
        ``trip_pair`` (``trips=True``): the agent tables (K, A, 9) that another run on the same environments left behind
        (its ``engine.agents``, still on the device); this run's per-agent launch then also pairs the two, trip by trip:
        ``trips`` gains n_both, d_sum, d_sumsq, n_faster, n_slower with d = this run - the other (``trip_report`` of the OTHER
        run takes this one as its ``baseline``). ``path_pair`` (``paths=True``): ``(state, agents)`` of another run on the same
        environments — its ``ops.PathTraceState`` (a ``clone()`` where that evaluator runs again) and agent tables; this
        run's ``path_stats`` then also hold the paired sums of moves and excess, this run - the other."""
        t_start = time.perf_counter()
        eng, fs = self.eng, self.eng.fs
        T = self.episode_frames if frames is None else int(frames)
        if T < 1:
            raise ValueError("frames must be >= 1")
        if self.head in ROUTER_HEADS and not deterministic:
            raise ValueError(f"head {self.head!r} has no sampled mode: the shortest-path router is deterministic given the state")
        if self.head in PLAN_HEADS and not deterministic:
            raise ValueError(f"head {self.head!r} has no sampled mode: a plan is followed, nothing is drawn")
        if trip_pair is not None and not self.trips:
            raise ValueError("trip_pair pairs the trips of two runs: it needs trips=True")
        if path_pair is not None and not self.paths:
            raise ValueError("path_pair pairs the path traces of two runs: it needs paths=True")
        self._reserve(T)
        self._flag_host.zero_()
        fs.check_flags()            # whatever an earlier user of this engine left unread is theirs: raised, not averaged
        eng.reset()
        if self.trips or self.dynamic_gap or self.paths:
            pop = eng.agents[:, :, :3]
            if not bool((pop == pop[:1]).all()):
                raise ValueError(f"{'trips=True' if self.trips else ('dynamic_gap=True' if self.dynamic_gap else 'paths=True')} needs the same population in every "
                                 "environment: ORIGIN, DESTINATION or DEPARTURE_TIME differ between the agent tables")
            if trip_pair is not None and (tuple(trip_pair.shape) != tuple(eng.agents.shape) or
                                          not bool((trip_pair[:, :, :3] == pop).all())):
                raise ValueError("trip_pair must hold the same population as this engine's agent tables")
            if path_pair is not None and (tuple(path_pair[1].shape) != tuple(eng.agents.shape) or
                                          not bool((path_pair[1][:, :, :3] == pop).all())):
                raise ValueError("path_pair must hold the same population as this engine's agent tables")
        if self.paths:
            ops.path_trace_reset(self.path_state)
        self._start(bool(deterministic))
        sched = H = None
        if self.link_counts or self._occ_acc_on or self.trips or self.turns or self.paths:      # one binning for every binned report
            t0, step, bins = int(eng.time), int(eng.timestep), self.link_bin_seconds
            H = (t0 + (T - 1) * step) // bins - t0 // bins + 1
            sched = _BinSchedule(t0, step, bins, t0 // bins, H)
        if self.trips and H > ops.TRIP_MAX_BINS:
            raise ValueError(f"trips=True stores at most {ops.TRIP_MAX_BINS} time bins (ops.TRIP_MAX_BINS); {T} frames in bins "
                             f"of {sched.bin_seconds} s reach {H}: widen link_bin_seconds")
        if self.dynamic_gap:
            self._gap_reserve(sched)
        acc = dict(dtype=torch.int32, device=eng.device)
        if self.link_counts:
            if self.link_acc is None or self.link_acc.size(1) != H:
                self.link_acc = torch.empty((eng.B, H, eng.N), **acc)
            self.link_acc.zero_()
        if self._occ_acc_on:
            if self.occ_acc is None or self.occ_acc["veh"].size(1) != H:
                self.occ_acc = {"veh": torch.empty((eng.B, H, eng.N), **acc), "full": torch.empty((eng.B, H, eng.N), **acc),
                                "peak": torch.empty((eng.B, 1, eng.N), **acc)}
            for v in self.occ_acc.values():
                v.zero_()
        if self.turns:
            self._turn_reserve(H)
        polls = []                  # (frames queued when the status word was copied, event)
        seen = False
        done = 0
        for t in range(T):
            clock = float(eng.time)     # this frame's clock: the frame advances it
            self._frame(t, bool(deterministic))
            done = t + 1
            if self.trip_reward:        # the frame is complete: the travellers owed, beside the queue reward
                ops.fused_trip_reward(eng.plan, fs, clock, out=self.trip_rw[t], parts=self.trip_parts[t])
            if self.paths:              # after every other launch of the frame: who heads which road now
                ops.fused_path_trace(eng.plan, fs, self.path_state, self.path_w, self.path_dist, self.path_slot)
            if self.link_counts and _due(done, self.link_block, T):         # one launch per block of the rings
                ops.link_counts_accumulate(self.link_popped, self.link_withdrawn, self.link_acc,
                                           **sched.block(done, self.link_block))
            if self._occ_acc_on and _due(done, self.occupancy_block, T):      # one launch per block of the ring
                ops.occupancy_accumulate(self.occ_ring, self.occ_thr, *self.occ_acc.values(),      # (veh, full, peak)
                                         **sched.block(done, self.occupancy_block))
            if self.turns and _due(done, self.turn_block, T):               # one launch per block of the three rings
                blk = sched.block(done, self.turn_block)
                ops.turn_counts_accumulate(eng.plan, self.turn_popped, self.turn_sel, self.turn_ring, *self.turn_acc.values(),
                                           prev_counts=self.turn_prev if done > blk["frames"] else None, **blk)
                self.turn_prev.copy_(self.turn_ring[blk["frames"] - 1])      # n_pre of the next block's first frame
            if _due(done, self.poll_frames, T):
                self._flag_host[len(polls)].copy_(fs.flags[0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                polls.append((done, ev))
                # look only at copies that have arrived: the launch pipeline is never stalled
                seen = any(e.query() and int(self._flag_host[j]) & _lib.FLAG_COUNT_AT_NMAX for j, (_, e) in enumerate(polls))
                if seen:
                    break
        polls[-1][1].synchronize()
        settings = dict(bin_width=self.bin_width, num_bins=self.num_bins, temperature=self.temperature, seed=eng.seed,
                        env_base=fs.env_base, poll_frames=self.poll_frames, agents=eng.A - 1, nodes=eng.N)
        if self.head in ROUTER_HEADS:
            settings.update(refresh_rate=self.refresh_rate, destinations=int(self.dests.numel()))
        if self.head == "dijkstra_hold":      # (the "dijkstra" head's settings stay as they were)
            settings["hold"] = True
        if self.head in PLAN_HEADS:           # agents a >= 1 without a usable route: unreachable, or longer than max_hops
            settings.update(max_hops=int(self.routes.size(-1)), routes_per_env=self.routes.dim() == 3, hold=True,
                            route_fallback=self.route_fallback,
                            agents_without_route=int((self.route_len[..., 1:] <= 0).sum()))
        if self.policy_hold:                  # (without the flag the settings stay as they were)
            settings["policy_hold"] = True
        if self.route_departures:
            settings["route_departures"] = True
        if self.trip_reward:
            settings["trip_reward"] = True
        if self.paths:                        # (without the flag the settings stay as they were)
            settings.update(paths=True, path_max_hops=self.path_state.L)
        res = EvalResult(envs=eng.B, head=self.head, deterministic=bool(deterministic), frames_run=done, settings=settings)
        first = 0
        for j, (upto, _) in enumerate(polls):
            v = int(self._flag_host[j])
            if v & _lib.FLAG_COUNT_AT_NMAX:
                res.domain_exit, res.domain_exit_frames = True, (first, upto)
                # frames queued behind the flagged block ran on a state outside the domain (memory-safe: csrc/fused_rows.hip
                # bounds every slot index by Nmax); the status word is re-armed so that the engine is usable after reset()
                res.frames_run = upto
                fs.flags.zero_()
                res.computation_time_ms = (time.perf_counter() - t_start) * 1000.0
                return res
            ops.raise_on_flags(v)      # any other bit is a configuration error, as everywhere else
            first = upto
        s = ops.episode_summary(eng.agents, reward=self.reward, frames=done, bin_width=self.bin_width,
                                num_bins=self.num_bins, out=self.summary)
        host = {k: v.cpu().numpy() for k, v in s.items()}
        per, res.aggregate, res.envs_without_arrival = summarise(host["counts"], host["sums"], host["episode_return"],
                                                                 host["hist"], done, self.bin_width)
        for k, v in per.items():
            setattr(res, k, v)
        if self.policy_hold:
            res.held = self.held.cpu().numpy().astype(np.int64)
        if self.route_departures:
            res.departures_routed = self.routed.cpu().numpy().astype(np.int64)
        if self.trip_reward:                  # integers below 2^24 per frame: the float64 sum is exact
            res.trip_return = [float(v) for v in self.trip_rw[:done].double().sum(dim=0).cpu().numpy()]
            res.trip_parts_last = self.trip_parts[done - 1].cpu().numpy().astype(np.int64)
            res.aggregate["trip_return"] = aggregate(res.trip_return)
        if self.link_counts:
            st = ops.link_count_stats(self.link_acc)
            res.link_counts = self.link_acc.cpu().numpy()
            res.link_first_bin, res.link_bin_seconds = sched.first_bin, sched.bin_seconds
            res.link_stats = link_moments({k: v.cpu().numpy() for k, v in st.items()}, eng.B)
        if self.occupancy:
            res.occupancy, res.occupancy_stats = {}, {}
            for k, acc in self.occ_acc.items():
                st = ops.link_count_stats(acc)
                res.occupancy[k] = acc.cpu().numpy()
                res.occupancy_stats[k] = link_moments({j: v.cpu().numpy() for j, v in st.items()}, eng.B)
            bins_of = (sched.t0 + np.arange(done, dtype=np.int64) * sched.timestep) // sched.bin_seconds - sched.first_bin
            res.occupancy_frames_per_bin = [int(x) for x in np.bincount(bins_of, minlength=H)]
            res.occupancy_meta = dict(first_bin=sched.first_bin, bin_seconds=sched.bin_seconds, timestep=sched.timestep,
                                      max=self.occ_max.copy(), thr=self.occ_thr_host.copy())
        if self.turns:
            self._turn_reduce(res, sched, host["counts"][:, 1])
        if self.trips:
            self._trip_reduce(res, trip_pair, sched)
        if self.dynamic_gap:
            self._gap_reduce(res, sched, done)
        if self.paths:
            self._path_reduce(res, path_pair, sched)
        res.computation_time_ms = (time.perf_counter() - t_start) * 1000.0
        return res

    # -- per-turn movement counts -------------------------------------------------------------------------------
    def _turn_reserve(self, H):
        """The tables of the turn counts for the run's H bins, zeroed, before the first frame: turns (K, H, E), lost (K, H, N)
        and unresolved (K,) int32. Refused beyond half the free device memory."""
        eng = self.eng
        K, N, E, dev = eng.B, eng.N, eng.E, eng.device
        if self.turn_acc is None or self.turn_acc["turns"].size(1) != H:
            self.turn_acc = None
            need = 4 * K * H * (E + N)
            free = int(torch.cuda.mem_get_info(dev)[0])
            if need > free // 2:
                raise _lib.TarlError(f"the turn counts' tables ({need / 2**30:.2f} GiB for K = {K} environments x H = {H} bins x "
                                     f"(E = {E} edges + N = {N} roads)) exceed half the free device memory "
                                     f"({free / 2**30:.2f} GiB free): evaluate fewer environments at a time or widen "
                                     f"link_bin_seconds")
            self.turn_acc = {"turns": torch.empty((K, H, E), dtype=torch.int32, device=dev),
                             "lost": torch.empty((K, H, N), dtype=torch.int32, device=dev),
                             "unresolved": torch.empty(K, dtype=torch.int32, device=dev)}
        for v in self.turn_acc.values():
            v.zero_()

    def _turn_reduce(self, res, sched, on_way):
        """The tables of a finished run into ``res``, after the two checks: every pop was attributed, and per environment the
        lost agents are the ON_WAY agents that the network no longer holds (``-reward`` of the last frame is its occupancy)."""
        eng = self.eng
        unresolved = self.turn_acc["unresolved"].cpu().numpy()
        if unresolved.any():
            raise _lib.TarlError(f"turn counts: {int(unresolved.sum())} pops of a non-empty road whose SELECTED_ROAD byte names no "
                                 f"out-edge (per environment: {unresolved.tolist()}); such a run is not reported")
        res.turn_counts, res.turn_lost = self.turn_acc["turns"].cpu().numpy(), self.turn_acc["lost"].cpu().numpy()
        lost = self.turn_acc["lost"].sum(dim=(1, 2)).cpu().numpy()        # (int64 on the device)
        queued = -self.reward[res.frames_run - 1].cpu().numpy().astype(np.float64)
        missing = np.asarray(on_way, dtype=np.float64) - queued
        if not np.array_equal(lost.astype(np.float64), missing):
            raise _lib.TarlError(f"turn counts: the phantom pops per environment {lost.tolist()} are not the ON_WAY agents "
                                 f"queued nowhere {missing.tolist()}")
        res.turn_stats = {}
        for k in ("turns", "lost"):
            st = ops.link_count_stats(self.turn_acc[k])
            res.turn_stats[k] = link_moments({j: v.cpu().numpy() for j, v in st.items()}, eng.B)
        prob = None
        if self.head == "embedding":      # the state-independent policy: its probability of every route edge
            logits = ops.policy_edge_logits(eng.plan, eng.static_node_features[0], self.emb).view(1, -1)
            prob = ops.graphdist_softmax(eng.plan, logits, self.temperature).view(-1).cpu().numpy().astype(np.float64)
        res.turn_meta = dict(first_bin=sched.first_bin, bin_seconds=sched.bin_seconds,
                             edge_index=eng.edge_index.numpy().copy(), on_way=[int(x) for x in on_way],
                             queued=[int(x) for x in queued], policy_prob=prob)

    def _trip_reduce(self, res, trip_pair, sched):
        """The two trip reductions of a finished run into ``res``. Clock values outside the H bins of the frames (a
        departure before the first frame's bin) are clamped into the first / last bin by the kernel."""
        eng = self.eng
        bins = dict(bin_seconds=sched.bin_seconds, first_bin=sched.first_bin, num_bins=sched.H)
        # the agents sorted by departure bin: once per run, for all K environments (run() has checked that they agree)
        order = ops.trip_departure_order(eng.agents[0, :, 2], **bins)
        per_agent = ops.trip_agent_stats(eng.agents, trip_pair, free_flow=self.trip_ff)
        per_bin = ops.trip_bin_stats(eng.agents, free_flow=self.trip_ff, order=order, **bins)
        res.trips = {k: v.cpu().numpy() for k, v in per_agent.items()}
        res.trip_bins = {k: v.cpu().numpy() for k, v in per_bin.items()}
        pop = eng.agents[0, :, :3].cpu().numpy()
        res.trip_meta = dict(first_bin=sched.first_bin, bin_seconds=sched.bin_seconds, origin=pop[:, 0].astype(np.int64),
                             destination=pop[:, 1].astype(np.int64), departure=pop[:, 2].copy(),
                             free_flow=None if self.trip_ff is None else self.trip_ff.cpu().numpy(),
                             paired=trip_pair is not None)

    # -- the per-agent path trace ---------------------------------------------------------------------------------
    def _path_reduce(self, res, path_pair, sched):
        """The trace of a finished run into ``res``: one reduction per agent over the environments, then the check that
        nothing impossible was seen, then the arrays on the host."""
        eng, st = self.eng, self.path_state
        stats = ops.path_agent_stats(st, eng.agents, *(path_pair if path_pair is not None else (None, None)))
        bad = st.bad.cpu().numpy()
        if bad.any():
            raise _lib.TarlError(f"path trace: {int(bad.sum())} sightings of a head id beyond the agent table or of two roads "
                                 f"that no edge connects (per environment: {bad.tolist()}); such a run is not reported")
        res.paths = {k: v.cpu().numpy() for k, v in st.tensors().items() if k not in ("route", "bad")}
        res.paths["done"] = (eng.agents[:, :, 8] == 1.0).cpu().numpy()
        res.path_routes = (st.route.cpu().numpy(), st.route_len.cpu().numpy())
        res.path_stats = {k: v.cpu().numpy() for k, v in stats.items()}
        pop = eng.agents[0, :, :3].cpu().numpy()
        res.path_meta = dict(max_hops=st.L, weights=self.path_w is not None, note=self.path_note, first_bin=sched.first_bin,
                             bin_seconds=sched.bin_seconds, num_bins=sched.H, origin=pop[:, 0].astype(np.int64),
                             destination=pop[:, 1].astype(np.int64), departure=pop[:, 2].copy(), paired=path_pair is not None)

    # -- the dynamic relative gap ---------------------------------------------------------------------------------
    def _gap_reserve(self, sched):
        """The buffers of the dynamic gap for the run's H bins, before the first frame: tau (J, H, N) fp32, env (J, H + 1, N)
        and best (J, A) fp64, the label rows of the searches. Refused beyond half the free device memory."""
        eng = self.eng
        J, H, N, A, dev = self.dynamic_gap_envs, sched.H, eng.N, eng.A, eng.device
        if H > ops.TRIP_MAX_BINS:
            raise ValueError(f"dynamic_gap=True stores at most {ops.TRIP_MAX_BINS} time bins (ops.TRIP_MAX_BINS); the frames "
                             f"reach {H} bins of {sched.bin_seconds} s: widen link_bin_seconds")
        buf = getattr(self, "_gap_buf", None)
        if buf is not None and buf["tau"].shape == (J, H, N):
            return
        self._gap_buf = None
        scratch = ops.td_hindsight_bytes(eng.plan, J, A)
        if scratch < 0:
            raise _lib.TarlError("tarl_td_hindsight_scratch_bytes refused the evaluator's sizes")
        tables = 4 * J * H * N + 8 * J * (H + 1) * N + 8 * J * A
        free = int(torch.cuda.mem_get_info(dev)[0])
        if tables + scratch > free // 2:
            raise _lib.TarlError(f"the dynamic gap's road times and envelope ({tables / 2**30:.2f} GiB for dynamic_gap_envs = {J} "
                                 f"environments x H = {H} bins x N = {N} roads, A = {A} agents) and search scratch "
                                 f"({scratch / 2**30:.2f} GiB) exceed half the free device memory ({free / 2**30:.2f} GiB "
                                 f"free): lower dynamic_gap_envs or widen link_bin_seconds")
        st = eng.static_node_features[0]
        mx, ff = st[:, 0].contiguous(), st[:, 2].contiguous()
        cc = eng.cc
        if cc is None:      # the simulator's own fp32 expression (oracle/sim.py::congestion_constants)
            cc = ff * (mx + 10 - st[:, 4] * ff / 3600)
        self._gap_buf = dict(tau=torch.empty((J, H, N), dtype=torch.float32, device=dev),
                             env=torch.empty((J, H + 1, N), dtype=torch.float64, device=dev),
                             best=torch.empty((J, A), dtype=torch.float64, device=dev),
                             scratch=torch.empty(max(scratch, 1), dtype=torch.uint8, device=dev),
                             frames=torch.zeros(H, dtype=torch.int32, device=dev), max=mx, ff=ff,
                             cc=cc.to(torch.float32).contiguous())

    def _gap_reduce(self, res, sched, done):
        """Road times, searches and the fp64 reductions of a finished run into ``res.dynamic_gap``."""
        eng, b = self.eng, self._gap_buf
        J, H, A = self.dynamic_gap_envs, sched.H, eng.A
        t_start = time.perf_counter()
        bins_of = (sched.t0 + np.arange(done, dtype=np.int64) * sched.timestep) // sched.bin_seconds - sched.first_bin
        frames = np.bincount(bins_of, minlength=H).astype(np.int32)
        b["frames"].copy_(torch.from_numpy(frames))
        kw = dict(bin_seconds=sched.bin_seconds, first_bin=sched.first_bin)
        ag = eng.agents[:J]
        ops.td_road_times(self.occ_acc["veh"][:J], b["frames"], b["max"], b["ff"], b["cc"], out=(b["tau"], b["env"]), **kw)
        best = ops.td_hindsight(eng.plan, b["tau"], b["env"], ag, out=b["best"], scratch=b["scratch"], **kw)
        # plumbing: (J, A) -> per agent, per environment, per (environment, departure bin), fp64 on the device
        done_m = ag[:, :, 8] == 1.0
        t0 = ag[:, :, 2].to(torch.float64)
        tt = (ag[:, :, 3] - ag[:, :, 2]).to(torch.float64)
        ht = best - t0
        use = done_m & torch.isfinite(ht)
        use[:, 0] = False
        zero = torch.zeros((), dtype=torch.float64, device=eng.device)
        g = torch.where(use, tt - torch.where(use, ht, zero), zero)
        neg = use & (g < 0)
        inf = torch.full((), float("inf"), dtype=torch.float64, device=eng.device)
        per_agent = {"n": use.sum(0), "g_sum": g.sum(0), "g_sumsq": (g * g).sum(0), "g_min": torch.where(use, g, inf).amin(0),
                     "g_max": torch.where(use, g, -inf).amax(0), "n_neg": neg.sum(0)}
        per_env = {"tt_sum": torch.where(use, tt, zero).sum(1), "ht_sum": torch.where(use, ht, zero).sum(1), "n": use.sum(1),
                   "n_neg": neg.sum(1), "n_nonpos": (use & (g <= 0)).sum(1)}
        dep_bin = ops.trip_clock_bin(ag[0, :, 2], sched.bin_seconds, sched.first_bin, H)
        idx = dep_bin.unsqueeze(0).expand(J, A)
        per_bin = {"g_sum": torch.zeros((J, H), dtype=torch.float64, device=eng.device).scatter_add_(1, idx, g),
                   "n": torch.zeros((J, H), dtype=torch.int64, device=eng.device).scatter_add_(1, idx, use.to(torch.int64))}
        host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}      # noqa: E731
        pop = ag[0, :, :3].cpu().numpy()
        res.dynamic_gap = dict(best=best.cpu().numpy(), per_agent=host(per_agent), per_env=host(per_env), per_bin=host(per_bin))
        res.dynamic_gap["meta"] = dict(
            envs=J, first_bin=sched.first_bin, bin_seconds=sched.bin_seconds, frames_per_bin=[int(x) for x in frames],
            origin=pop[:, 0].astype(np.int64), destination=pop[:, 1].astype(np.int64), departure=pop[:, 2].copy(),
            searches=int(done_m[:, 1:].sum()), wall_ms=(time.perf_counter() - t_start) * 1000.0)
