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
moves nobody, and the agent stays: the router delivers only agents whose last hop was delayed. Read its
``arrived`` with that in mind; the return (the network's occupancy) compares as it stands.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .engine import EPISODE_END, EPISODE_START

HEADS = ("embedding", "edge_mlp", "edge_mlp_fp32", "edge_mlp_bf16", "embedding_dijkstra", "graph_transformer", "dijkstra")
_MLP_PRECISION = {"edge_mlp": "x3", "edge_mlp_fp32": "fp32", "edge_mlp_bf16": "bf16"}
PER_ENV_KEYS = ("episode_return", "frames", "arrived", "on_way", "not_departed", "avg_travel_time", "std_travel_time",
                "max_travel_time", "p50_travel_time", "p95_travel_time")


def aggregate(values):
    """Mean and spread of one per-environment quantity over the K environments. ``None`` entries (an environment without
    an arrival has no travel time) are left out and counted in ``missing``. ``std`` is the sample standard deviation
    (ddof = 1), ``se = std / sqrt(n)``, ``ci95 = mean -+ 1.96 se``: a NORMAL-APPROXIMATION interval, ``None`` (like std and
    se) when fewer than two environments contribute."""
    v = np.asarray([x for x in values if x is not None], dtype=np.float64)
    out = {"n": int(v.size), "missing": int(len(values) - v.size), "mean": None, "std": None, "se": None, "min": None,
           "max": None, "ci95": None, "ci95_kind": "normal approximation, mean -+ 1.96 se"}
    if v.size == 0:
        return out
    out.update(mean=float(v.mean()), min=float(v.min()), max=float(v.max()))
    if v.size >= 2:
        std = float(v.std(ddof=1))
        se = std / math.sqrt(v.size)
        out.update(std=std, se=se, ci95=(out["mean"] - 1.96 * se, out["mean"] + 1.96 * se))
    return out


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

    def to_dict(self, per_env=False):
        d = {k: getattr(self, k) for k in ("envs", "head", "deterministic", "frames_run", "domain_exit",
                                           "domain_exit_frames", "aggregate", "envs_without_arrival", "settings",
                                           "computation_time_ms")}
        if per_env:
            d["per_env"] = {k: getattr(self, k) for k in PER_ENV_KEYS}
        return d

    def rows(self):
        """One dict per environment (the rows of eval_envs.csv)."""
        if self.domain_exit:
            return []
        return [dict(env=b, **{k: getattr(self, k)[b] for k in PER_ENV_KEYS}) for b in range(self.envs)]

    def summary_lines(self):
        """The aggregate as printable lines."""
        if self.domain_exit:
            a, b = self.domain_exit_frames
            return [f"domain exit: a FIFO count reached Nmax between frames {a} and {b}; no statistics"]
        out = []
        for k in PER_ENV_KEYS:
            g = self.aggregate[k]
            if g["mean"] is None:
                out.append(f"{k + ':':22} no data ({g['missing']} environments without an arrival)")
                continue
            s = f"{k + ':':22} {g['mean']:12.3f}"
            if g["se"] is not None:
                s += f"  +- {g['se']:.3f} (se)  95% [{g['ci95'][0]:.3f}, {g['ci95'][1]:.3f}] (normal approx.)"
            s += f"  min {g['min']:.3f}  max {g['max']:.3f}  n {g['n']}"
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
    for name, key in PAIRED_METRICS:
        d = np.asarray([x - y for x, y in zip(getattr(a, key), getattr(b, key)) if x is not None and y is not None],
                       dtype=np.float64)
        m = {"n": int(d.size), "dropped": int(a.envs - d.size), "mean": None, "std": None, "se": None, "ci95": None,
             "ci95_kind": "normal approximation, mean -+ 1.96 se"}
        if d.size >= 1:
            m["mean"] = float(d.mean())
        if d.size >= 2:
            std = float(d.std(ddof=1))
            se = std / math.sqrt(d.size)
            m.update(std=std, se=se, ci95=(m["mean"] - 1.96 * se, m["mean"] + 1.96 * se))
        metrics[name] = m
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
        s = f"{name + ':':22} {m['mean']:12.3f}"
        if m["se"] is not None:
            s += f"  +- {m['se']:.3f} (se)  95% [{m['ci95'][0]:.3f}, {m['ci95'][1]:.3f}] (normal approx.)"
        s += f"  n {m['n']}"
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


# ---- per-road link counts (VecEvaluator(link_counts=True)) --------------------------------------------------------------------
LINK_RING_BYTES = 256 << 20         # both mask rings of the evaluator together
LINK_EXPECTED = {"msa": "expected_msa", "ue": "ue_flow", "so": "so_flow"}      # expected-flow vector -> its column
LINK_PARTIAL_NOTE = ("counts are not rescaled: a run shorter than the demand's horizon sees only part of the demand, so the "
                     "simulated totals fall short of the expected flows by the trips that had not yet passed")


def link_moments(ints, K):
    """Host side of ``ops.link_count_stats``: its integer arrays ``sum``, ``sumsq`` (int64), ``min``, ``max`` (int32), each
    (H + 1, N) with the episode total in the last row, -> the same plus ``mean`` and, for K >= 2, the sample standard
    deviation ``std`` (ddof = 1, from the exact integer K sum d^2 - (sum d)^2), ``se = std / sqrt(K)`` and ``ci95_lo`` /
    ``ci95_hi = mean -+ 1.96 se`` (normal approximation), all float64; ``None`` for K = 1, as in :func:`aggregate`."""
    K = int(K)
    s, q = np.asarray(ints["sum"], dtype=np.int64), np.asarray(ints["sumsq"], dtype=np.int64)
    out = {"n": K, "sum": s, "sumsq": q, "min": np.asarray(ints["min"], dtype=np.int32),
           "max": np.asarray(ints["max"], dtype=np.int32), "mean": s / float(K), "std": None, "se": None, "ci95_lo": None,
           "ci95_hi": None}
    if K >= 2:
        std = np.sqrt((K * q - s * s) / float(K * (K - 1)))
        se = std / math.sqrt(K)
        out.update(std=std, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def geh(m, c):
    """The GEH statistic ``sqrt(2 (m - c)^2 / (m + c))`` of a simulated count m against an expected count c, elementwise;
    0 where both are 0."""
    m, c = np.asarray(m, dtype=np.float64), np.asarray(c, dtype=np.float64)
    tot = m + c
    return np.sqrt(2.0 * (m - c) ** 2 / np.where(tot == 0, 1.0, tot)) * (tot != 0)


def link_bin_names(first_bin, num_bins, bin_seconds):
    """Column names of the stored bins, by ABSOLUTE bin: ``count_5h``, ``count_6h`` for hourly bins, ``count_bin<k>`` else."""
    return [f"count_{first_bin + h}h" if int(bin_seconds) == 3600 else f"count_bin{first_bin + h}" for h in range(num_bins)]


def _flow_vector(flows, N, name):
    if isinstance(flows, dict):
        v = np.zeros(N, dtype=np.float64)
        for road, flow in flows.items():
            if 0 <= int(road) < N:
                v[int(road)] = float(flow)
        return v
    v = np.asarray(flows, dtype=np.float64).reshape(-1)
    if v.size != N:
        raise ValueError(f"expected flows {name!r} must hold one value per road ({N}), got {v.size}")
    return v


def _pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    den = math.sqrt(float((a * a).sum()) * float((b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


def _paired_link_moments(a: EvalResult, b: EvalResult):
    """The two-input statistics call on the two count tensors (uploaded; the kernel is the only implementation)."""
    dev = torch.device("cuda")
    st = ops.link_count_stats(torch.from_numpy(a.link_counts).to(dev), torch.from_numpy(b.link_counts).to(dev))
    return link_moments({k: v.cpu().numpy() for k, v in st.items()}, a.envs)


def link_count_report(result: EvalResult, expected=None, baseline: EvalResult | None = None) -> dict:
    """Per-road rows and a summary of the link counts of one evaluation (``VecEvaluator(link_counts=True)``).
    Every row: ``road``, the episode total's ``mean``, ``sd``, ``se``, ``ci95_lo``, ``ci95_hi`` (``None`` for K = 1), ``min``,
    ``max`` over the K environments, and the per-bin means (:func:`link_bin_names`). ``expected``: ``{name: flows}`` with
    names of :data:`LINK_EXPECTED` (``msa``, ``ue``, ``so``) and flows a ``{road: flow}`` map (roads it lacks: 0) or an array
    (N,); per name the row gains the flow (column ``expected_msa`` / ``ue_flow`` / ``so_flow``), ``diff_<name>`` = mean -
    expected and ``geh_<name>`` (:func:`geh`), the summary RMSE, mean absolute difference, share of roads with GEH < 5, Pearson
    correlation (nan for a constant vector) and simulated total over expected total. NOTHING is rescaled
    (:data:`LINK_PARTIAL_NOTE`, carried as ``note``). ``baseline``: the evaluation of another head on the same environments
    (same K, seed, frames and bins: ``ValueError`` otherwise); the row gains ``baseline_mean`` and the paired difference
    result - baseline, ``paired_diff_mean`` / ``paired_diff_se`` / ``paired_diff_ci95_lo`` / ``_hi``, from the two-input
    ``ops.link_count_stats``; the summary counts the roads whose interval excludes 0. A run without link counts (a domain
    exit has none): ``{"available": False, "reason": ...}``."""
    if result.domain_exit or result.link_counts is None:
        why = "a run that left the domain has no statistics" if result.domain_exit else "the run did not count links"
        return {"available": False, "reason": why}
    K, H, N = result.link_counts.shape
    st = result.link_stats
    names = link_bin_names(result.link_first_bin, H, result.link_bin_seconds)
    spread = st["std"] is not None
    rows = []
    for n in range(N):
        row = {"road": n, "mean": float(st["mean"][H, n]), "sd": float(st["std"][H, n]) if spread else None,
               "se": float(st["se"][H, n]) if spread else None, "ci95_lo": float(st["ci95_lo"][H, n]) if spread else None,
               "ci95_hi": float(st["ci95_hi"][H, n]) if spread else None, "min": int(st["min"][H, n]),
               "max": int(st["max"][H, n])}
        row.update({name: float(st["mean"][h, n]) for h, name in enumerate(names)})
        rows.append(row)
    mean = st["mean"][H].astype(np.float64)
    summary = {"envs": K, "roads": N, "frames_run": result.frames_run, "simulated_total": float(mean.sum()),
               "roads_counted": int((st["max"][H] > 0).sum()), "expected": {}}
    columns = ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max"] + names
    for name, flows in (expected or {}).items():
        if name not in LINK_EXPECTED:
            raise ValueError(f"expected flows must be named among {tuple(LINK_EXPECTED)}, got {name!r}")
        c = _flow_vector(flows, N, name)
        d, g = mean - c, geh(mean, c)
        col = LINK_EXPECTED[name]
        for n, row in enumerate(rows):
            row.update({col: float(c[n]), f"diff_{name}": float(d[n]), f"geh_{name}": float(g[n])})
        columns += [col, f"diff_{name}", f"geh_{name}"]
        tot = float(c.sum())
        summary["expected"][name] = {"rmse": float(math.sqrt(float((d * d).mean()))), "mean_abs_diff": float(np.abs(d).mean()),
                                     "geh_below_5_share": float((g < 5.0).mean()), "pearson": _pearson(mean, c),
                                     "total_ratio": float(mean.sum()) / tot if tot != 0 else float("nan"),
                                     "expected_total": tot}
    rep = {"available": True, "head": result.head, "bin_seconds": result.link_bin_seconds,
           "first_bin": result.link_first_bin, "bins": names, "note": LINK_PARTIAL_NOTE}
    if baseline is not None:
        if baseline.envs != K:
            raise ValueError(f"link_count_report needs the same environments: envs {K} / {baseline.envs}")
        for k in ("seed", "env_base"):
            if result.settings.get(k) != baseline.settings.get(k):
                raise ValueError(f"link_count_report needs equal {k}: {result.settings.get(k)!r} / {baseline.settings.get(k)!r}")
        if baseline.domain_exit or baseline.link_counts is None:
            summary["paired"] = {"available": False, "reason": "the baseline run has no link counts"}
        else:
            if baseline.link_counts.shape != result.link_counts.shape or baseline.frames_run != result.frames_run or \
                    (baseline.link_first_bin, baseline.link_bin_seconds) != (result.link_first_bin, result.link_bin_seconds):
                raise ValueError("link_count_report needs the same frames and bins in both runs")
            pd = _paired_link_moments(result, baseline)
            pair = pd["std"] is not None
            for n, row in enumerate(rows):
                row.update(baseline_mean=float(baseline.link_stats["mean"][H, n]), paired_diff_mean=float(pd["mean"][H, n]),
                           paired_diff_se=float(pd["se"][H, n]) if pair else None,
                           paired_diff_ci95_lo=float(pd["ci95_lo"][H, n]) if pair else None,
                           paired_diff_ci95_hi=float(pd["ci95_hi"][H, n]) if pair else None)
            columns += ["baseline_mean", "paired_diff_mean", "paired_diff_se", "paired_diff_ci95_lo", "paired_diff_ci95_hi"]
            excl = int(((pd["ci95_lo"][H] > 0) | (pd["ci95_hi"][H] < 0)).sum()) if pair else None
            summary["paired"] = {"available": True, "baseline_head": baseline.head, "roads_interval_excludes_zero": excl,
                                 "mean_abs_paired_diff": float(np.abs(pd["mean"][H]).mean()),
                                 "baseline_total": float(baseline.link_stats["mean"][H].sum())}
    rep.update(columns=columns, rows=rows, summary=summary)
    return rep


def link_count_lines(report: dict):
    """:func:`link_count_report` as printable lines (the ``Link counts`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"{'roads counted:':22} {s['roads_counted']:12d} of {s['roads']}  (pops + withdrawals per road, {s['envs']} "
           f"environments, {s['frames_run']} frames, bins of {report['bin_seconds']} s: {', '.join(report['bins'])})",
           f"{'simulated total:':22} {s['simulated_total']:12.3f}  (sum over the roads of the mean episode total)"]
    if not s["expected"]:
        out.append("expected flows:        not available (the MSA / equilibrium block was skipped): no comparison columns")
    for name, e in s["expected"].items():
        out.append(f"{'vs ' + name + ':':22} RMSE {e['rmse']:.3f}  mean |diff| {e['mean_abs_diff']:.3f}  GEH < 5 on "
                   f"{100.0 * e['geh_below_5_share']:.1f} % of the roads  Pearson r {e['pearson']:.4f}  simulated / expected "
                   f"total {e['total_ratio']:.4f}")
    if s["expected"]:
        out.append(f"note: {report['note']}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        line = f"{'policy - ' + p['baseline_head'] + ':':22} mean |paired diff| {p['mean_abs_paired_diff']:.3f} per road"
        if p["roads_interval_excludes_zero"] is not None:
            line += f"; the 95% interval excludes 0 on {p['roads_interval_excludes_zero']} of {s['roads']} roads (normal approx.)"
        else:
            line += "; one environment: no interval"
        out.append(line)
    return out


def link_count_summary(report: dict):
    """The report without its rows, nan as ``None``: what the JSON files carry (never the K x H x N tensor)."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, float) and math.isnan(v):
            return None
        return v
    return clean({k: v for k, v in report.items() if k != "rows"})


# ---- per-road occupancy and time at capacity (VecEvaluator(occupancy=True)) ----------------------------------------------------
OCCUPANCY_RING_BYTES = 256 << 20    # the fp32 ring of frame_fused's `counts` slices
CONGESTION_FILE = 3                 # src/feature_helpers.py: has_room = n_i < max_i - CONGESTION_FILE


def capacity_threshold(max_agents):
    """``thr[n] = ceil(MAX[n] - 3)`` int32: the count from which road n admits nobody, the negation of Direction's
    ``has_room = n_i < max_i - CONGESTION_FILE`` and of the insert's capacity rule, taken literally (a road with MAX <= 3 is
    at capacity in every frame)."""
    return np.ceil(np.asarray(max_agents, dtype=np.float64) - CONGESTION_FILE).astype(np.int32)


def occupancy_bin_names(first_bin, num_bins, bin_seconds):
    """Column names of the stored bins, by ABSOLUTE bin: ``occ_5h``, ``occ_6h`` for hourly bins, ``occ_bin<k>`` else."""
    return [f"occ_{first_bin + h}h" if int(bin_seconds) == 3600 else f"occ_bin{first_bin + h}" for h in range(num_bins)]


def _paired_occupancy_moments(a: EvalResult, b: EvalResult, key):
    """The two-input statistics call on one of the accumulators of two runs (uploaded; the kernel is the only
    implementation)."""
    dev = torch.device("cuda")
    st = ops.link_count_stats(torch.from_numpy(a.occupancy[key]).to(dev), torch.from_numpy(b.occupancy[key]).to(dev))
    return link_moments({k: v.cpu().numpy() for k, v in st.items()}, a.envs)


def _opt(moments, key, row, n, scale=1.0):
    return float(moments[key][row, n]) * scale if moments[key] is not None else None


def occupancy_report(result: EvalResult, baseline: EvalResult | None = None) -> dict:
    """Per-road rows and a summary of the occupancy of one evaluation (``VecEvaluator(occupancy=True)``), formed in float64
    on the host from the integer accumulators ``veh`` (vehicle-frames per environment, bin and road), ``full`` (frames at
    capacity) and ``peak`` and their integer moments over the K environments.
    Every row: ``road``, ``max_agents`` (MAX) and ``thr``; ``veh_seconds_*`` of the episode (vehicle-frames x timestep):
    mean, sd, se, ci95_lo, ci95_hi (``None`` for K = 1), min, max over K; the mean occupancy per bin
    (:func:`occupancy_bin_names`: veh / frames in the bin, averaged over K; ``None`` for a bin without a frame); ``vc_mean``,
    the time-averaged count / max(MAX, 1) (the reference's v/c ratio); ``peak_mean`` / ``peak_max``; ``full_frames_mean`` /
    ``_min`` / ``_max`` and ``full_share`` of the frames run. ``baseline``: the evaluation of another head on the same
    environments (same K, seed, frames and bins: ``ValueError`` otherwise); the row gains the baseline's means and the paired
    differences result - baseline of veh_seconds and full_frames with se and interval, from the two-input
    ``ops.link_count_stats``. The summary: network vehicle-hours per environment (mean, se, interval over K; paired with a
    baseline), per bin the network mean and population sd of v/c averaged over K, the share of road-frames at capacity,
    the mean number of roads ever at capacity, the roads whose paired interval excludes 0, and the identity
    sum(veh[b]) == -episode_return[b]. A run without occupancy (a domain exit has none):
    ``{"available": False, "reason": ...}``."""
    if result.domain_exit or result.occupancy is None:
        why = "a run that left the domain has no statistics" if result.domain_exit else "the run did not accumulate occupancy"
        return {"available": False, "reason": why}
    veh, full, peak = (result.occupancy[k] for k in ("veh", "full", "peak"))
    K, H, N = veh.shape
    meta, st = result.occupancy_meta, result.occupancy_stats
    step, T = int(meta["timestep"]), int(result.frames_run)
    cap = np.asarray(meta["max"], dtype=np.float64)
    thr = np.asarray(meta["thr"], dtype=np.int64)
    fpb = np.asarray(result.occupancy_frames_per_bin, dtype=np.float64)
    names = occupancy_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    sv, sf, sp = st["veh"], st["full"], st["peak"]
    den = np.maximum(cap, 1.0)
    rows = []
    for n in range(N):
        row = {"road": n, "max_agents": float(cap[n]), "thr": int(thr[n]),
               "veh_seconds_mean": float(sv["mean"][H, n]) * step, "veh_seconds_sd": _opt(sv, "std", H, n, step),
               "veh_seconds_se": _opt(sv, "se", H, n, step), "veh_seconds_ci95_lo": _opt(sv, "ci95_lo", H, n, step),
               "veh_seconds_ci95_hi": _opt(sv, "ci95_hi", H, n, step), "veh_seconds_min": int(sv["min"][H, n]) * step,
               "veh_seconds_max": int(sv["max"][H, n]) * step}
        row.update({name: float(sv["mean"][h, n]) / fpb[h] if fpb[h] > 0 else None for h, name in enumerate(names)})
        row.update(vc_mean=float(sv["mean"][H, n]) / T / den[n], peak_mean=float(sp["mean"][0, n]),
                   peak_max=int(sp["max"][0, n]), full_frames_mean=float(sf["mean"][H, n]), full_frames_min=int(sf["min"][H, n]),
                   full_frames_max=int(sf["max"][H, n]), full_share=float(sf["mean"][H, n]) / T)
        rows.append(row)
    columns = list(rows[0])
    v64, f64 = veh.astype(np.int64), full.astype(np.int64)
    veh_env = v64.sum(axis=(1, 2))                                     # vehicle-frames per environment
    ret = np.asarray(result.episode_return, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = v64 / fpb[None, :, None] / den[None, None, :]             # (K, H, N); nan in a bin without a frame
    vc_mean, vc_sd = vc.mean(axis=2).mean(axis=0), vc.std(axis=2).mean(axis=0)
    summary = {"envs": K, "roads": N, "frames_run": T, "timestep": step,
               "vehicle_hours": aggregate(list(veh_env * step / 3600.0)),
               "vc_mean_per_bin": [float(x) for x in vc_mean], "vc_sd_per_bin": [float(x) for x in vc_sd],
               "frames_per_bin": [int(x) for x in fpb],
               "share_road_frames_at_capacity": float(f64.sum()) / (float(K) * T * N),
               "mean_roads_ever_at_capacity": float((f64.sum(axis=1) > 0).sum(axis=1).mean()),
               "largest_peak": int(peak.max()),
               "identity": {"holds": bool(np.array_equal(veh_env.astype(np.float64), -ret)),
                            "vehicle_frames": [int(x) for x in veh_env], "minus_episode_return": [float(-x) for x in ret]}}
    rep = {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
           "bins": names}
    if baseline is not None:
        if baseline.envs != K:
            raise ValueError(f"occupancy_report needs the same environments: envs {K} / {baseline.envs}")
        for k in ("seed", "env_base"):
            if result.settings.get(k) != baseline.settings.get(k):
                raise ValueError(f"occupancy_report needs equal {k}: {result.settings.get(k)!r} / {baseline.settings.get(k)!r}")
        if baseline.domain_exit or baseline.occupancy is None:
            summary["paired"] = {"available": False, "reason": "the baseline run has no occupancy"}
        else:
            bm = baseline.occupancy_meta
            if baseline.occupancy["veh"].shape != veh.shape or baseline.frames_run != T or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds", "timestep")):
                raise ValueError("occupancy_report needs the same frames and bins in both runs")
            pv, pf = (_paired_occupancy_moments(result, baseline, k) for k in ("veh", "full"))
            bv, bf = baseline.occupancy_stats["veh"], baseline.occupancy_stats["full"]
            for n, row in enumerate(rows):
                row.update(baseline_veh_seconds_mean=float(bv["mean"][H, n]) * step,
                           paired_veh_seconds_mean=float(pv["mean"][H, n]) * step,
                           paired_veh_seconds_se=_opt(pv, "se", H, n, step),
                           paired_veh_seconds_ci95_lo=_opt(pv, "ci95_lo", H, n, step),
                           paired_veh_seconds_ci95_hi=_opt(pv, "ci95_hi", H, n, step),
                           baseline_full_frames_mean=float(bf["mean"][H, n]), paired_full_frames_mean=float(pf["mean"][H, n]),
                           paired_full_frames_se=_opt(pf, "se", H, n), paired_full_frames_ci95_lo=_opt(pf, "ci95_lo", H, n),
                           paired_full_frames_ci95_hi=_opt(pf, "ci95_hi", H, n))
            columns = list(rows[0])
            pair = pv["std"] is not None
            excl = {k: int(((m["ci95_lo"][H] > 0) | (m["ci95_hi"][H] < 0)).sum()) if pair else None
                    for k, m in (("veh_seconds", pv), ("full_frames", pf))}
            base_env = baseline.occupancy["veh"].astype(np.int64).sum(axis=(1, 2))
            summary["paired"] = {"available": True, "baseline_head": baseline.head,
                                 "vehicle_hours": aggregate(list((veh_env - base_env) * step / 3600.0)),
                                 "baseline_vehicle_hours": aggregate(list(base_env * step / 3600.0)),
                                 "roads_interval_excludes_zero": excl}
    rep.update(columns=columns, rows=rows, summary=summary)
    return rep


def _pm(g, unit=""):
    s = f"{g['mean']:12.3f}{unit}"
    if g["se"] is not None:
        s += f"  +- {g['se']:.3f} (se)  95% [{g['ci95'][0]:.3f}, {g['ci95'][1]:.3f}] (normal approx.)"
    return s + f"  min {g['min']:.3f}  max {g['max']:.3f}  n {g['n']}"


def occupancy_lines(report: dict):
    """:func:`occupancy_report` as printable lines (the ``Occupancy`` block), the ten roads with the most frames at capacity
    included."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"{'vehicle-hours:':22} {_pm(s['vehicle_hours'])}  (network total per environment, {s['envs']} environments, "
           f"{s['frames_run']} frames of {s['timestep']} s)"]
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        g = p["vehicle_hours"]
        line = f"{'policy - ' + p['baseline_head'] + ':':22} {g['mean']:12.3f} vehicle-hours"
        if g["se"] is not None:
            line += f"  +- {g['se']:.3f} (se)  95% [{g['ci95'][0]:.3f}, {g['ci95'][1]:.3f}] (normal approx.)"
        e = p["roads_interval_excludes_zero"]
        if e["veh_seconds"] is not None:
            line += (f"; per road the 95% interval excludes 0 on {e['veh_seconds']} (vehicle-seconds) and {e['full_frames']} "
                     f"(frames at capacity) of {s['roads']} roads")
        else:
            line += "; one environment: no interval"
        out.append(line)
    for name, frames, m, sd in zip(report["bins"], s["frames_per_bin"], s["vc_mean_per_bin"], s["vc_sd_per_bin"]):
        out.append(f"{'v/c ' + name + ':':22} mean {m:.4f}  sd {sd:.4f} over the roads, averaged over the environments "
                   f"({frames} frames)")
    out.append(f"{'at capacity:':22} {100.0 * s['share_road_frames_at_capacity']:.3f} % of the road-frames; "
               f"{s['mean_roads_ever_at_capacity']:.2f} of {s['roads']} roads ever at capacity (mean over the environments); "
               f"largest count {s['largest_peak']}")
    i = s["identity"]
    out.append(f"{'identity:':22} sum of vehicle-frames == -episode return in every environment: "
               f"{'yes' if i['holds'] else 'NO'} (environment 0: {i['vehicle_frames'][0]} / {i['minus_episode_return'][0]:.0f})")
    top = sorted(report["rows"], key=lambda r: (-r["full_frames_mean"], r["road"]))[:10]
    out.append("roads with the most frames at capacity (mean over the environments):")
    for r in top:
        out.append(f"  road {r['road']:6d}  full {r['full_frames_mean']:10.2f} frames ({100.0 * r['full_share']:.1f} %)  "
                   f"peak {r['peak_max']:3d} of MAX {r['max_agents']:.0f} (thr {r['thr']})  "
                   f"vehicle-seconds {r['veh_seconds_mean']:.1f}")
    return out


def occupancy_summary(report: dict):
    """The report without its rows, nan as ``None``: what the JSON files carry (never the K x H x N tensors)."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        if isinstance(v, float) and math.isnan(v):
            return None
        return v
    return clean({k: v for k, v in report.items() if k != "rows"})


# ---- per-trip report (VecEvaluator(trips=True)) ----------------------------------------------------------------------------------
TRIP_FF_CHUNK_BYTES = 256 << 20     # the fp64 distance rows of one ops.destination_trees call of the free-flow times
TRIP_CHANCE = 0.025                 # share of agents without an effect whose 95 % interval lies on one side of 0
TRIP_FF_NOTE = ("free_flow is a reference value, not a lower bound: the withdraw rule and the step order decide when a trip "
                "ends, so a travel time can lie below it")


def trip_free_flow_times(engine, weights):
    """The free-flow time of every agent of ``engine`` (environment 0's table) -> fp64 (A,) on the device: FREE_FLOW of its
    origin road plus the distance origin -> destination under the edge weights ``weights`` fp32 (E,) from
    ``ops.destination_trees(want_dist=True)`` over the distinct destinations (src.agents.base.destination_set's rule), built
    a block of destinations at a time; +inf where the destination cannot be reached or an id is out of range, and for the
    dummy row 0. :data:`TRIP_FF_NOTE` applies."""
    N, dev = engine.N, engine.device
    w = weights.detach().to(dev, torch.float32).reshape(-1).contiguous()
    if w.numel() != engine.E:
        raise ValueError(f"trip_free_flow must hold one weight per edge ({engine.E}), got {w.numel()}")
    ag = engine.agents[0]
    o, d = ag[:, 0].to(torch.int64), ag[:, 1].to(torch.int64)
    ok = (o >= 0) & (o < N) & (d >= 0) & (d < N)
    ok[0] = False
    dests = torch.unique(d[ok]).contiguous()
    ff = torch.full((engine.A,), float("inf"), dtype=torch.float64, device=dev)
    if dests.numel() == 0:
        return ff
    slot = torch.full((N,), -1, dtype=torch.int64, device=dev)
    slot[dests] = torch.arange(dests.numel(), dtype=torch.int64, device=dev)
    oc, sl = o.clamp(0, N - 1), slot[d.clamp(0, N - 1)]
    own = engine.static_node_features[0, :, 2].to(torch.float64)        # FREE_FLOW_TIME_TRAVEL of the origin road
    rows = max(1, TRIP_FF_CHUNK_BYTES // (8 * N))
    for c0 in range(0, int(dests.numel()), rows):
        _, dist = ops.destination_trees(engine.plan, w, dests[c0:c0 + rows].contiguous(), want_next_hop=False, want_dist=True)
        here = ok & (sl >= c0) & (sl < c0 + dist.size(0))
        val = own[oc] + dist[(sl - c0).clamp(0, dist.size(0) - 1), oc]
        ff = torch.where(here, val, ff)
    return ff


def _trip_moments(n, s1, s2):
    """mean, sd (ddof 1), se and interval of n values with sum s1 and sum of squares s2, the rules of :func:`aggregate`:
    the mean needs one value, the others two."""
    out = {"mean": None, "sd": None, "se": None, "ci95_lo": None, "ci95_hi": None}
    n = int(n)
    if n >= 1:
        out["mean"] = float(s1) / n
    if n >= 2:
        sd = math.sqrt(max(0.0, (float(s2) - float(s1) * float(s1) / n) / (n - 1)))
        se = sd / math.sqrt(n)
        out.update(sd=sd, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def trip_bin_names(first_bin, num_bins, bin_seconds):
    """Labels of the stored bins, by ABSOLUTE bin: ``5h``, ``6h`` for hourly bins, ``bin<k>`` else."""
    return [f"{first_bin + h}h" if int(bin_seconds) == 3600 else f"bin{first_bin + h}" for h in range(num_bins)]


def _trip_same_population(a: EvalResult, b: EvalResult):
    return all(np.array_equal(a.trip_meta[k], b.trip_meta[k]) for k in ("origin", "destination", "departure"))


def trip_report(result: EvalResult, baseline: EvalResult | None = None) -> dict:
    """Per-agent rows, a by-departure table and a summary of the trips of one evaluation (``VecEvaluator(trips=True)``),
    formed in float64 on the host from the kernels' counts and sums.
    Every row: ``agent``, ``origin``, ``destination``, ``departure``, ``free_flow`` (``None``: none); ``arrival_share`` =
    n_done / K and ``envs_on_way``; ``tt_mean``, ``tt_sd`` (ddof 1), ``tt_se``, ``tt_ci95_lo`` / ``_hi`` (mean -+ 1.96 se, normal
    approximation), ``tt_min``, ``tt_max`` over the environments in which the agent arrived — the mean, min and max ``None``
    without an arrival, the spread ``None`` below two, as in :func:`aggregate`; ``delay_mean`` = tt_mean - free_flow and
    ``delay_ratio`` = tt_mean / free_flow (``None`` without either). :data:`TRIP_FF_NOTE` applies.
    ``baseline``: the evaluation of another head on the same environments, run with ``run(..., trip_pair=<this run's agent
    tables>)`` (same K, seed, env_base, frames, bins and population: ``ValueError`` otherwise). The row gains
    ``baseline_arrival_share``, ``baseline_tt_mean`` and, over the environments in which the agent arrived in BOTH runs, the
    paired difference result - baseline: ``paired_n``, ``paired_diff_mean``, ``paired_diff_se``, ``paired_diff_ci95_lo`` /
    ``_hi``, ``n_faster`` and ``n_slower`` (environments in which the trip was faster / slower than under the baseline).
    The summary classifies every agent with paired_n >= 2 as faster (interval entirely below 0), slower (entirely above) or
    neither, the sign of the mean deciding where se = 0, and sets next to both counts the number expected by chance alone,
    :data:`TRIP_CHANCE` x the classified agents. A run without trips (a domain exit has none):
    ``{"available": False, "reason": ...}``."""
    if result.domain_exit or result.trips is None:
        why = "a run that left the domain has no statistics" if result.domain_exit else "the run did not reduce its trips"
        return {"available": False, "reason": why}
    tr, tb, meta = result.trips, result.trip_bins, result.trip_meta
    K, H = tb["dep_done"].shape
    A = tr["n_done"].shape[0]
    ff = meta["free_flow"]
    has_ff = ff is not None
    pair = None
    if baseline is not None:
        if baseline.envs != K:
            raise ValueError(f"trip_report needs the same environments: envs {K} / {baseline.envs}")
        for k in ("seed", "env_base"):
            if result.settings.get(k) != baseline.settings.get(k):
                raise ValueError(f"trip_report needs equal {k}: {result.settings.get(k)!r} / {baseline.settings.get(k)!r}")
        if baseline.domain_exit or baseline.trips is None:
            pair = {"available": False, "reason": "the baseline run has no trips"}
        else:
            bm = baseline.trip_meta
            if baseline.frames_run != result.frames_run or baseline.trip_bins["dep_done"].shape != (K, H) or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds")):
                raise ValueError("trip_report needs the same frames and bins in both runs")
            if baseline.trips["n_done"].shape[0] != A or not _trip_same_population(result, baseline):
                raise ValueError("trip_report needs the same population in both runs (origin, destination, departure)")
            if not bm.get("paired") or "n_both" not in baseline.trips:
                pair = {"available": False, "reason": "the baseline run was not paired with this one (run(trip_pair=...))"}
            else:
                pair = {"available": True, "baseline_head": baseline.head}
    paired = pair is not None and pair["available"]
    n_done = tr["n_done"].astype(np.int64)
    rows = []
    cls = {"faster": 0, "slower": 0, "neither": 0}
    for a in range(1, A):
        n = int(n_done[a])
        m = _trip_moments(n, tr["tt_sum"][a], tr["tt_sumsq"][a])
        f = float(ff[a]) if has_ff and math.isfinite(float(ff[a])) else None
        row = {"agent": a, "origin": int(meta["origin"][a]), "destination": int(meta["destination"][a]),
               "departure": float(meta["departure"][a]), "free_flow": f, "arrival_share": n / K,
               "envs_on_way": int(tr["n_way"][a]), "tt_mean": m["mean"], "tt_sd": m["sd"], "tt_se": m["se"],
               "tt_ci95_lo": m["ci95_lo"], "tt_ci95_hi": m["ci95_hi"], "tt_min": float(tr["tt_min"][a]) if n else None,
               "tt_max": float(tr["tt_max"][a]) if n else None,
               "delay_mean": m["mean"] - f if n and f is not None else None,
               "delay_ratio": m["mean"] / f if n and f is not None and f > 0 else None}
        if paired:      # the baseline's launch holds d = baseline - result: the difference result - baseline is its negative
            bt = baseline.trips
            nb = int(bt["n_both"][a])
            d = _trip_moments(nb, -float(bt["d_sum"][a]), bt["d_sumsq"][a])
            row.update(baseline_arrival_share=int(bt["n_done"][a]) / K,
                       baseline_tt_mean=float(bt["tt_sum"][a]) / int(bt["n_done"][a]) if int(bt["n_done"][a]) else None,
                       paired_n=nb, paired_diff_mean=d["mean"], paired_diff_se=d["se"], paired_diff_ci95_lo=d["ci95_lo"],
                       paired_diff_ci95_hi=d["ci95_hi"], n_faster=int(bt["n_slower"][a]), n_slower=int(bt["n_faster"][a]))
            if nb >= 2:
                lo, hi = (d["ci95_lo"], d["ci95_hi"]) if d["se"] > 0 else (d["mean"], d["mean"])
                cls["faster" if hi < 0 else ("slower" if lo > 0 else "neither")] += 1
        rows.append(row)
    columns = list(rows[0]) if rows else []
    live = n_done[1:]
    trips_total = int(live.sum())
    summary = {"envs": K, "agents": A - 1, "frames_run": result.frames_run, "trips": trips_total,
               "arrived_in_every": int((live == K).sum()), "arrived_in_some": int(((live > 0) & (live < K)).sum()),
               "arrived_in_none": int((live == 0).sum()), "agents_on_way_somewhere": int((tr["n_way"][1:] > 0).sum()),
               "free_flow": None, "top_delays": []}
    if has_ff:
        f = np.asarray(ff, dtype=np.float64)[1:]
        use = np.isfinite(f) & (live > 0)
        w = live[use].astype(np.float64)
        tts, fs = tr["tt_sum"][1:][use].astype(np.float64), f[use]
        per_delay, per_ratio = tts / w - fs, (tts / w) / np.where(fs > 0, fs, np.nan)
        n_use = int(w.sum())
        spread = lambda v: float(np.nanstd(v, ddof=1)) if np.isfinite(v).sum() >= 2 else None      # noqa: E731
        summary["free_flow"] = {
            "agents": int(use.sum()), "trips": n_use, "note": TRIP_FF_NOTE,
            "mean_delay": float((tts - w * fs).sum()) / n_use if n_use else None,
            "delay_ratio": float(tts.sum()) / float((w * fs).sum()) if n_use and float((w * fs).sum()) > 0 else None,
            "mean_delay_sd_over_agents": spread(per_delay), "delay_ratio_sd_over_agents": spread(per_ratio),
            "share_trips_below_free_flow": int(tr["n_under"][1:].sum()) / n_use if n_use else None}
        top = sorted((r for r in rows if r["delay_mean"] is not None), key=lambda r: (-r["delay_mean"], r["agent"]))[:10]
        summary["top_delays"] = [{k: r[k] for k in ("agent", "origin", "destination", "departure", "free_flow", "tt_mean",
                                                    "delay_mean", "arrival_share")} for r in top]
    # by departure time: per bin over the K environments
    names = trip_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    dep_bin = trip_host_bin(meta["departure"][1:], meta["bin_seconds"], meta["first_bin"], H)
    scheduled = np.bincount(dep_bin, minlength=H)
    dd, dt = tb["dep_done"].astype(np.float64), tb["dep_tt"].astype(np.float64)
    by_rows = []
    for h in range(H):
        g = aggregate(list(dd[:, h]))
        tt = aggregate([dt[k, h] / dd[k, h] if dd[k, h] > 0 else None for k in range(K)])
        row = {"bin": names[h], "scheduled": int(scheduled[h]), "arrived_mean": g["mean"], "arrived_se": g["se"],
               "on_way_mean": float(tb["dep_way"][:, h].mean()), "tt_mean": tt["mean"], "tt_se": tt["se"], "delay_mean": None,
               "delay_se": None, "arrivals_mean": float(tb["arr"][:, h].mean())}
        if has_ff:
            fn, fs = tb["dep_ff_n"].astype(np.float64), tb["dep_ff"].astype(np.float64)
            dl = aggregate([dt[k, h] / dd[k, h] - fs[k, h] / fn[k, h] if dd[k, h] > 0 and fn[k, h] > 0 else None
                            for k in range(K)])
            row.update(delay_mean=dl["mean"], delay_se=dl["se"])
        by_rows.append(row)
    if pair is not None:
        if paired:
            n_cls = sum(cls.values())
            pair.update(agents_classified=n_cls, agents_faster=cls["faster"], agents_slower=cls["slower"],
                        agents_neither=cls["neither"], expected_by_chance=TRIP_CHANCE * n_cls,
                        pairs=int(baseline.trips["n_both"][1:].sum()),
                        mean_paired_diff=(-float(baseline.trips["d_sum"][1:].sum()) / int(baseline.trips["n_both"][1:].sum())
                                          if int(baseline.trips["n_both"][1:].sum()) else None))
        summary["paired"] = pair
    return {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
            "bins": names, "columns": columns, "rows": rows, "by_departure_columns": list(by_rows[0]),
            "by_departure": by_rows, "summary": summary}


def trip_host_bin(clock, bin_seconds, first_bin, num_bins):
    """The kernels' bin rule on the host: ``clamp(floor(c) // bin_seconds - first_bin, 0, num_bins - 1)`` of fp32 clock values
    (NaN and negatives as 0) -> int64."""
    c = np.nan_to_num(np.asarray(clock, dtype=np.float32).astype(np.float64), nan=0.0, posinf=2.0 ** 62, neginf=0.0)
    c = np.clip(np.floor(c), 0.0, 2.0 ** 62)
    return np.clip(c.astype(np.int64) // int(bin_seconds) - int(first_bin), 0, int(num_bins) - 1)


def _f(v, fmt=".2f"):
    return "-" if v is None else format(v, fmt)


def trip_lines(report: dict):
    """:func:`trip_report` as printable lines (the ``Trips`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"{'agents:':22} {s['agents']:12d}   arrived in every environment {s['arrived_in_every']}, in some "
           f"{s['arrived_in_some']}, in none {s['arrived_in_none']} ({s['envs']} environments, {s['frames_run']} frames; "
           f"{s['trips']} trips completed, {s['agents_on_way_somewhere']} agents still on the way somewhere)"]
    f = s["free_flow"]
    if f is None:
        out.append("free flow:             not available (no free-flow weights): no delay columns")
    elif not f["trips"]:
        out.append("free flow:             no completed trip with a free-flow time")
    else:
        out.append(f"{'mean delay:':22} {f['mean_delay']:12.3f} s  (tt - free flow, trip-weighted over {f['trips']} trips of "
                   f"{f['agents']} agents; sd over the agents {_f(f['mean_delay_sd_over_agents'], '.3f')})")
        out.append(f"{'delay ratio:':22} {_f(f['delay_ratio'], '12.4f')}    (sum tt / sum free flow; sd over the agents "
                   f"{_f(f['delay_ratio_sd_over_agents'], '.4f')})")
        out.append(f"{'below free flow:':22} {100.0 * f['share_trips_below_free_flow']:12.2f} % of the trips have tt < free flow "
                   f"(a reference value, not a lower bound)")
        out.append("agents with the largest mean delay:")
        for r in s["top_delays"]:
            out.append(f"  agent {r['agent']:7d}  {r['origin']:6d} -> {r['destination']:6d}  departs {r['departure']:9.1f}  "
                       f"free flow {r['free_flow']:8.1f}  tt {r['tt_mean']:9.2f}  delay {r['delay_mean']:9.2f}  "
                       f"arrived in {100.0 * r['arrival_share']:.0f} %")
    out.append(f"By departure time (bins of {report['bin_seconds']} s; means over the environments, arrived with its standard error):")
    out.append(f"  {'bin':>8} {'scheduled':>9} {'arrived':>18} {'mean tt':>10} {'mean delay':>10} {'arrivals in bin':>15}")
    for r in report["by_departure"]:
        arrived = f"{_f(r['arrived_mean'])}" + (f" +- {_f(r['arrived_se'])}" if r["arrived_se"] is not None else "")
        out.append(f"  {r['bin']:>8} {r['scheduled']:9d} {arrived:>18} {_f(r['tt_mean']):>10} {_f(r['delay_mean']):>10} "
                   f"{_f(r['arrivals_mean']):>15}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        out.append(f"{'policy - ' + p['baseline_head'] + ':':22} {_f(p['mean_paired_diff'], '12.3f')} s mean paired difference "
                   f"over {p['pairs']} trips completed in both runs")
        out.append(f"{'per agent:':22} faster under the policy {p['agents_faster']}, slower {p['agents_slower']}, neither "
                   f"{p['agents_neither']} of {p['agents_classified']} agents with >= 2 pairs (95% interval of the paired "
                   f"difference entirely below / above 0, normal approx.); expected by chance alone: "
                   f"{p['expected_by_chance']:.1f} on either side")
    return out


def trip_summary(report: dict):
    """The report without its per-agent and by-departure rows, nan as ``None``: what the JSON files carry (never the A-row
    tables)."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        if isinstance(v, float) and (math.isnan(v) or math.isinf(v)):
            return None
        return v
    return clean({k: v for k, v in report.items() if k not in ("rows", "by_departure")})


class VecEvaluator:
    def __init__(self, engine, head="embedding", *, emb=None, temperature=1.0, edge_mlp=None, prior_table=None,
                 dest_slot=None, prior_weight=1.0, gt_pe=None, gt_weights=None, bin_width=10.0, num_bins=720, poll_frames=64,
                 keep_actions=False, refresh_rate=10, baseline_dests=None, link_counts=False, link_bin_seconds=3600,
                 link_block=None, occupancy=False, occupancy_block=None, trips=False, trip_free_flow=None):
        """``engine``: a fused :class:`SimEngine` with K environments. ``emb``: flat (num_embeddings,) fp32 embedding
        (MPNNPolicyNet.nodes_embedding.weight); ``edge_mlp``: ops.EdgeMlpWeights (edge_mlp* heads); ``prior_table`` (N, N),
        or (N, D) with ``dest_slot`` (embedding_dijkstra); ``gt_pe`` (N, 16) and ``gt_weights``: ops.GtWeights
        (graph_transformer). The tensors are read at every frame: views of live parameters evaluate the current policy.
        ``keep_actions``: also record every frame's action bytes in ``actions`` (T, K, N) uint8 (tests).
        Head ``"dijkstra"`` (the shortest-path baseline, no ``emb``): ``refresh_rate`` frames between two rebuilds of the K
        per-environment next-hop tables; ``baseline_dests`` = (dests int64 (D,), dest_slot int32 (N,)) of
        src.agents.base.destination_set over the engine's agent tables (default: computed here by the same rule). The
        (K, D, N) int32 table and the tree scratch are allocated once; more than half the free device memory is refused.
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
        (:func:`trip_free_flow_times`, one ``ops.destination_trees`` pass here) then serves as the reference for its delay."""
        if engine.fs is None:
            raise _lib.TarlError("VecEvaluator needs the fused engine (ops.fused_path_supported): the packed state cannot "
                                 "represent this graph and there is no fall-back")
        if head not in HEADS:
            raise ValueError(f"head must be one of {HEADS}")
        if head in _MLP_PRECISION and edge_mlp is None:
            raise ValueError(f"head {head!r} needs edge_mlp (ops.EdgeMlpWeights)")
        if head == "embedding_dijkstra" and prior_table is None:
            raise ValueError("head 'embedding_dijkstra' needs prior_table (and dest_slot for a per-destination table)")
        if head == "graph_transformer" and (gt_pe is None or gt_weights is None):
            raise ValueError("head 'graph_transformer' needs gt_pe and gt_weights")
        if head != "dijkstra" and emb is None:
            raise ValueError(f"head {head!r} needs emb (the flat embedding tensor)")
        if int(poll_frames) < 1:
            raise ValueError("poll_frames must be >= 1")
        if int(refresh_rate) < 1:
            raise ValueError("refresh_rate must be >= 1")
        self.eng, self.head = engine, head
        self.emb = emb
        self.temperature = float(temperature)
        self.edge_mlp, self.prior_table, self.dest_slot = edge_mlp, prior_table, dest_slot
        self.prior_weight, self.gt_pe, self.gt_weights = float(prior_weight), gt_pe, gt_weights
        self.bin_width, self.num_bins, self.poll_frames = float(bin_width), int(num_bins), int(poll_frames)
        self.keep_actions = bool(keep_actions)
        self.refresh_rate = int(refresh_rate)
        K, N, E, dev = engine.B, engine.N, engine.E, engine.device
        plan = engine.plan
        self.link_counts = bool(link_counts)
        if self.link_counts:
            self.link_bin_seconds = int(link_bin_seconds)
            if self.link_bin_seconds < 1:
                raise ValueError("link_bin_seconds must be >= 1")
            if link_block is None:
                link_block = max(1, min(self.poll_frames, ops.LINK_COUNTS_MAX_FRAMES, LINK_RING_BYTES // (2 * K * N)))
            self.link_block = int(link_block)
            if not 1 <= self.link_block <= ops.LINK_COUNTS_MAX_FRAMES:
                raise ValueError(f"link_block must be in [1, {ops.LINK_COUNTS_MAX_FRAMES}] (ops.LINK_COUNTS_MAX_FRAMES)")
            self.link_popped = torch.zeros((self.link_block, K, N), dtype=torch.uint8, device=dev)
            self.link_withdrawn = torch.zeros((self.link_block, K, N), dtype=torch.uint8, device=dev)
            self.link_acc = None        # (K, H, N) int32, sized by run() for its frames
        self.occupancy = bool(occupancy)
        if self.occupancy:
            self.link_bin_seconds = int(link_bin_seconds)
            if self.link_bin_seconds < 1:
                raise ValueError("link_bin_seconds must be >= 1")
            if occupancy_block is None:
                occupancy_block = max(1, min(self.poll_frames, OCCUPANCY_RING_BYTES // (4 * K * N)))
            self.occupancy_block = int(occupancy_block)
            if not 1 <= self.occupancy_block <= ops.OCCUPANCY_MAX_FRAMES:
                raise ValueError(f"occupancy_block must be in [1, {ops.OCCUPANCY_MAX_FRAMES}] (ops.OCCUPANCY_MAX_FRAMES)")
            self.occ_ring = torch.zeros((self.occupancy_block, N, K), dtype=torch.float32, device=dev)
            self.occ_max = engine.static_node_features[0, :, 0].detach().cpu().numpy().astype(np.float64)
            self.occ_thr_host = capacity_threshold(self.occ_max)
            self.occ_thr = torch.from_numpy(self.occ_thr_host).to(dev)
            self.occ_acc = None         # veh, full (K, H, N) and peak (K, 1, N) int32, sized by run() for its frames
        self.trips = bool(trips)
        if self.trips:
            self.link_bin_seconds = int(link_bin_seconds)
            if self.link_bin_seconds < 1:
                raise ValueError("link_bin_seconds must be >= 1")
            self.trip_ff = None if trip_free_flow is None else trip_free_flow_times(engine, trip_free_flow)
        elif trip_free_flow is not None:
            raise ValueError("trip_free_flow is the reference of the per-trip report: it needs trips=True")
        # scratch, allocated once
        self.log_prob = torch.zeros(K, dtype=torch.float32, device=dev)
        self.action8 = torch.zeros((K, N), dtype=torch.uint8, device=dev)          # the last frame's action bytes
        self.summary = {"counts": torch.zeros((K, 3), dtype=torch.int32, device=dev),
                        "sums": torch.zeros((K, 3), dtype=torch.float64, device=dev),
                        "episode_return": torch.zeros(K, dtype=torch.float64, device=dev),
                        "hist": torch.zeros((K, self.num_bins), dtype=torch.int32, device=dev)}
        self.reward = self.actions = self._flag_host = None
        if head == "embedding":
            self.mode8 = torch.zeros((1, N), dtype=torch.uint8, device=dev)
            self.mode_lp = torch.zeros(1, dtype=torch.float32, device=dev)
        elif head == "dijkstra":
            self._init_baseline(baseline_dests)
        else:
            self.logits = torch.empty((K, E), dtype=torch.float32, device=dev)
            need = int(_lib.load().tarl_graphdist_rollout_scratch_bytes(plan.handle, K))
            self.dist_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
            if head == "edge_mlp_bf16":
                self.obs = torch.empty((K, N, 16), dtype=torch.bfloat16, device=dev)
            elif head != "embedding_dijkstra":
                self.obs = torch.empty((K, N, 16), dtype=torch.float32, device=dev)
            if head == "graph_transformer":
                n = int(_lib.load().tarl_policy_gt_fwd_scratch_floats(plan.handle, K))
                self.gt_scratch = torch.empty(n, dtype=torch.float32, device=dev)

    def _init_baseline(self, baseline_dests):
        """The baseline's buffers, once per evaluator: travel times (K, E), the next-hop table (K, D, N) and the tree scratch
        (O(min(K D, 1024) N)). Refused beyond half the free device memory, like the graph-transformer critic's store."""
        eng = self.eng
        K, N, E, dev = eng.B, eng.N, eng.E, eng.device
        if baseline_dests is None:      # src.agents.base.destination_set's rule: every distinct DESTINATION, row 0 included
            d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
            d = d[(d >= 0) & (d < N)].contiguous()
            slot = torch.full((N,), -1, dtype=torch.int32, device=dev)
            slot[d] = torch.arange(d.numel(), dtype=torch.int32, device=dev)
            baseline_dests = (d, slot)
        self.dests, self.dest_slot = baseline_dests
        D = int(self.dests.numel())
        table_bytes, scratch_bytes = ops.destination_trees_batched_bytes(eng.plan, K, D)
        if scratch_bytes < 0:
            raise _lib.TarlError("tarl_dest_trees_batched_scratch_bytes refused the evaluator's sizes")
        free = int(torch.cuda.mem_get_info(dev)[0])
        if table_bytes + scratch_bytes > free // 2:
            raise _lib.TarlError(f"the shortest-path baseline's next-hop table ({table_bytes / 2**30:.2f} GiB for K = {K} "
                                 f"environments x D = {D} destinations x N = {N} nodes) and tree scratch "
                                 f"({scratch_bytes / 2**30:.2f} GiB) exceed half the free device memory "
                                 f"({free / 2**30:.2f} GiB free): evaluate fewer environments at a time")
        self.weights = torch.empty((K, E), dtype=torch.float32, device=dev)
        self.table = torch.full((K, D, N), -1, dtype=torch.int32, device=dev)
        self.tree_scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device=dev)

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

    # -- the action of one frame -----------------------------------------------------------------------------------------
    def _logits(self):
        eng, plan, fs = self.eng, self.eng.plan, self.eng.fs
        if self.head == "embedding_dijkstra":
            return ops.fused_prior_logits(plan, fs, eng._x, eng.Nmax, eng.agents, self.emb, self.prior_table,
                                          self.prior_weight, out=self.logits, dest_slot=self.dest_slot)
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
        if self.head != "embedding":
            return      # (the baseline builds its tables at frame 0: 0 % refresh_rate == 0)
        eng = self.eng
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
        if self.occupancy:          # and of the counts ring
            masks["counts"] = self.occ_ring[t % self.occupancy_block]
        if self.head == "dijkstra":     # choice -> core -> withdraw / insert -> reward: the environment's step order
            if eng._packed_stale:
                eng.resync()
            if t % self.refresh_rate == 0:
                ops.fused_edge_travel_time(eng.plan, eng.fs, out=self.weights)
                ops.destination_trees_batched(eng.plan, self.weights, self.dests, out=self.table, scratch=self.tree_scratch)
            ops.fused_select_next_hop_dest(eng.plan, eng.fs, self.dest_slot, self.table, choice8=rec)
            return eng.frame_fused(skip_choice=True, reward=self.reward[t], **masks)
        if self.head == "embedding":
            if rec is not None and deterministic:
                rec.copy_(self.action8)
            return eng.frame_fused(skip_choice=deterministic, reward=self.reward[t], **masks)
        logits = self._logits()
        if deterministic:
            ops.graphdist_mode_rollout(eng.plan, logits, self.temperature, choice8=rec, sel8=eng.fs.sel8,
                                       log_prob=self.log_prob)
        else:
            ops.graphdist_rollout(eng.plan, logits, self.temperature, seed=eng.seed ^ 0x5DEECE66D,
                                  counter=eng.sample_counter + 1, choice8=rec, sel8=eng.fs.sel8, log_prob=self.log_prob,
                                  scratch=self.dist_scratch)
        return eng.frame_fused(skip_choice=True, reward=self.reward[t], **masks)

    # -- the evaluation ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self, frames=None, deterministic=True, trip_pair=None):
        """Reset the engine, run ``frames`` frames (default: until the episode ends) and return an :class:`EvalResult`.
        ``trip_pair`` (``trips=True``): the agent tables (K, A, 9) that another run on the same environments left behind
        (its ``engine.agents``, still on the device); this run's per-agent launch then also pairs the two, trip by trip:
        ``trips`` gains n_both, d_sum, d_sumsq, n_faster, n_slower with d = this run - the other (``trip_report`` of the OTHER
        run takes this one as its ``baseline``)."""
        t_start = time.perf_counter()
        eng, fs = self.eng, self.eng.fs
        T = self.episode_frames if frames is None else int(frames)
        if T < 1:
            raise ValueError("frames must be >= 1")
        if self.head == "dijkstra" and not deterministic:
            raise ValueError("head 'dijkstra' has no sampled mode: the shortest-path router is deterministic given the state")
        if trip_pair is not None and not self.trips:
            raise ValueError("trip_pair pairs the trips of two runs: it needs trips=True")
        self._reserve(T)
        self._flag_host.zero_()
        fs.check_flags()            # whatever an earlier user of this engine left unread is theirs: raised, not averaged
        eng.reset()
        if self.trips:
            pop = eng.agents[:, :, :3]
            if not bool((pop == pop[:1]).all()):
                raise ValueError("trips=True needs the same population in every environment: ORIGIN, DESTINATION or "
                                 "DEPARTURE_TIME differ between the agent tables")
            if trip_pair is not None and (tuple(trip_pair.shape) != tuple(eng.agents.shape) or
                                          not bool((trip_pair[:, :, :3] == pop).all())):
                raise ValueError("trip_pair must hold the same population as this engine's agent tables")
        self._start(bool(deterministic))
        if self.link_counts or self.occupancy or self.trips:      # one binning for the per-road reports and the trips
            clock0, step, bins = int(eng.time), int(eng.timestep), self.link_bin_seconds
            first_bin = clock0 // bins
            H = (clock0 + (T - 1) * step) // bins - first_bin + 1
        if self.trips and H > ops.TRIP_MAX_BINS:
            raise ValueError(f"trips=True stores at most {ops.TRIP_MAX_BINS} time bins (ops.TRIP_MAX_BINS); {T} frames in bins "
                             f"of {bins} s reach {H}: widen link_bin_seconds")
        if self.link_counts:
            if self.link_acc is None or self.link_acc.size(1) != H:
                self.link_acc = torch.empty((eng.B, H, eng.N), dtype=torch.int32, device=eng.device)
            self.link_acc.zero_()
        if self.occupancy:
            if self.occ_acc is None or self.occ_acc["veh"].size(1) != H:
                self.occ_acc = {"veh": torch.empty((eng.B, H, eng.N), dtype=torch.int32, device=eng.device),
                                "full": torch.empty((eng.B, H, eng.N), dtype=torch.int32, device=eng.device),
                                "peak": torch.empty((eng.B, 1, eng.N), dtype=torch.int32, device=eng.device)}
            for v in self.occ_acc.values():
                v.zero_()
        polls = []                  # (frames queued when the status word was copied, event)
        seen = False
        done = 0
        for t in range(T):
            self._frame(t, bool(deterministic))
            done = t + 1
            if self.link_counts and (done % self.link_block == 0 or done == T):      # one launch per block of the rings
                f0 = t - t % self.link_block
                ops.link_counts_accumulate(self.link_popped, self.link_withdrawn, self.link_acc, t0=clock0 + f0 * step,
                                           timestep=step, bin_seconds=bins, first_bin=first_bin, frames=done - f0)
            if self.occupancy and (done % self.occupancy_block == 0 or done == T):   # one launch per block of the ring
                f0 = t - t % self.occupancy_block
                ops.occupancy_accumulate(self.occ_ring, self.occ_thr, self.occ_acc["veh"], self.occ_acc["full"],
                                         self.occ_acc["peak"], t0=clock0 + f0 * step, timestep=step, bin_seconds=bins,
                                         first_bin=first_bin, frames=done - f0)
            if done % self.poll_frames == 0 or done == T:
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
        if self.head == "dijkstra":
            settings.update(refresh_rate=self.refresh_rate, destinations=int(self.dests.numel()))
        res = EvalResult(envs=eng.B, head=self.head, deterministic=bool(deterministic), frames_run=done, settings=settings)
        first = 0
        for j, (upto, _) in enumerate(polls):
            v = int(self._flag_host[j])
            if v & _lib.FLAG_COUNT_AT_NMAX:
                res.domain_exit, res.domain_exit_frames = True, (first, upto)
                # frames queued behind the flagged block ran on a state outside the domain (memory-safe: csrc/fused.hip
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
        if self.link_counts:
            st = ops.link_count_stats(self.link_acc)
            res.link_counts, res.link_first_bin, res.link_bin_seconds = self.link_acc.cpu().numpy(), first_bin, bins
            res.link_stats = link_moments({k: v.cpu().numpy() for k, v in st.items()}, eng.B)
        if self.occupancy:
            res.occupancy, res.occupancy_stats = {}, {}
            for k, acc in self.occ_acc.items():
                st = ops.link_count_stats(acc)
                res.occupancy[k] = acc.cpu().numpy()
                res.occupancy_stats[k] = link_moments({j: v.cpu().numpy() for j, v in st.items()}, eng.B)
            bins_of = (clock0 + np.arange(done, dtype=np.int64) * step) // bins - first_bin
            res.occupancy_frames_per_bin = [int(x) for x in np.bincount(bins_of, minlength=H)]
            res.occupancy_meta = dict(first_bin=int(first_bin), bin_seconds=int(bins), timestep=int(step),
                                      max=self.occ_max.copy(), thr=self.occ_thr_host.copy())
        if self.trips:
            self._trip_reduce(res, trip_pair, first_bin, bins, H)
        res.computation_time_ms = (time.perf_counter() - t_start) * 1000.0
        return res

    def _trip_reduce(self, res, trip_pair, first_bin, bins, H):
        """The two trip reductions of a finished run into ``res``. Clock values outside the H bins of the frames (a
        departure before the first frame's bin) are clamped into the first / last bin by the kernel."""
        eng = self.eng
        # the agents sorted by departure bin: once per run, for all K environments (run() has checked that they agree)
        order = ops.trip_departure_order(eng.agents[0, :, 2], bin_seconds=bins, first_bin=first_bin, num_bins=H)
        per_agent = ops.trip_agent_stats(eng.agents, trip_pair, free_flow=self.trip_ff)
        per_bin = ops.trip_bin_stats(eng.agents, bin_seconds=bins, first_bin=first_bin, num_bins=H, free_flow=self.trip_ff,
                                     order=order)
        res.trips = {k: v.cpu().numpy() for k, v in per_agent.items()}
        res.trip_bins = {k: v.cpu().numpy() for k, v in per_bin.items()}
        pop = eng.agents[0, :, :3].cpu().numpy()
        res.trip_meta = dict(first_bin=int(first_bin), bin_seconds=int(bins), origin=pop[:, 0].astype(np.int64),
                             destination=pop[:, 1].astype(np.int64), departure=pop[:, 2].copy(),
                             free_flow=None if self.trip_ff is None else self.trip_ff.cpu().numpy(),
                             paired=trip_pair is not None)
