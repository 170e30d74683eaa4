"""Replanner — day-to-day replanning on the vectorised evaluation. NOT in the reference, which has no dynamic
traffic assignment loop; the scheme is MATSim's: every simulated day a share of the agents re-routes onto the path that would
have been quickest under the road times experienced so far, everybody else keeps their plan.

Day 0 follows the quickest routes of the EMPTY network (``veh = 0``: ``tau`` is the free-flow time in every bin), through the
same two calls as every other day. Day j:
  1. the ``"routes"`` head of :class:`VecEvaluator` runs the day (``occupancy=True, dynamic_gap=True``);
  2. the day's occupancy sums ``veh`` are added into an int32 accumulator, and ``ops.td_road_times`` gets the accumulator
     with ``frames_per_bin * (j + 1)``: the mean occupancy over the days so far (successive averaging, exact in integers);
  3. ``ops.td_routes`` plans every (environment, agent) on those road times;
  4. an agent adopts its new route with probability ``fraction`` (``"msa"``: 1 / (j + 2)), drawn on the host from
     ``torch.Generator().manual_seed(day_seed(seed, j))`` as a (P, A) mask of ``torch.rand(...) < p``; an agent whose current
     route has length <= 0 always adopts.
P = K plans with ``per_env=True`` (environment k plans on its own history); ``per_env=False`` plans once on the sum over the K
environments (one table, ``frames * K``) and every environment follows the one plan.

Every day runs on the engine's own seed AND from the same noise counters: the days share their noise streams, so the day table
shows what the plans change, not what the noise does. A day that leaves the domain ends the loop and is reported as such,
never averaged. The last day is planned (its ``differs`` share says how far the plans are from a fixed point) but not
swapped: ``ReplanResult.routes`` is the plan the last day — and ``ReplanResult.last`` — ran with. Everything stays on the
device except K numbers per day."""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .eval_reports import _sample_moments
from .evaluator import EvalResult, VecEvaluator

DAY_KEYS = ("arrived", "avg_travel_time", "relative_gap")


def day_seed(seed, day):
    """The seed of day ``day``'s switch mask: a fixed mix of (seed, day), below 2^63."""
    return (int(seed) * 1000003 + int(day) * 7919 + 12345) & ((1 << 63) - 1)


def switch_probability(fraction, day):
    return 1.0 / (day + 2) if fraction == "msa" else float(fraction)


def parse_fraction(text):
    """``--replan-fraction`` / ``Replanner(fraction=)``: ``"msa"`` or a share in (0, 1], as text or number."""
    if isinstance(text, str) and text == "msa":
        return text
    v = float(text)
    if not 0.0 < v <= 1.0:
        raise ValueError(f"the replanning fraction must be 'msa' or in (0, 1], got {text!r}")
    return v


@dataclass
class ReplanResult:
    days: list                                     # one record per simulated day (dicts: DAY_KEYS as aggregates, shares, times)
    last: EvalResult | None                        # the last completed day's evaluation (None: day 0 left the domain)
    routes: torch.Tensor | None = field(default=None, compare=False)        # (P, A, max_hops) int32: the last day's plan
    route_len: torch.Tensor | None = field(default=None, compare=False)     # (P, A) int32
    settings: dict = field(default_factory=dict)
    domain_exit_day: int | None = None


class Replanner:
    def __init__(self, engine, *, days, fraction=0.1, max_hops=None, link_bin_seconds=3600, seed=0, per_env=True, keep=False,
                 route_departures=False, trip_reward=False, **eval_kw):
        """``engine``: a fused :class:`SimEngine` with K environments that share one population. ``days`` >= 1 simulated
        days; ``fraction``: the share that may switch per day, in (0, 1], or ``"msa"``; ``max_hops``: the longest route
        stored (default min(N, 256)); ``link_bin_seconds``: the bins of the road times; ``seed``: of the switch masks.
        ``keep``: also keep, per day, clones of the plan the day ran with, of the agent tables it left and of the switch mask
        drawn after it in ``history`` (tests). ``eval_kw``: further report flags of :class:`VecEvaluator` (link_counts, trips, turns, ...) for every day's run.
        ``route_departures``: every day's ``routes`` evaluator runs with the first-hop rule, so that an agent
        follows its own plan on its first road too.
        ``trip_reward``: every day's evaluator also computes the trip reward; the day records gain
        ``trip_return`` (its moments over the environments), the report ``trip_return_mean`` / ``trip_return_se``.
        The routes take 4 K A max_hops bytes twice (current and new); with the search scratch that is refused beyond half
        the free device memory."""
        if int(days) < 1:
            raise ValueError("days must be >= 1")
        self.fraction = parse_fraction(fraction)
        self.eng, self.days, self.seed, self.per_env = engine, int(days), int(seed), bool(per_env)
        K, N, A, dev = engine.B, engine.N, engine.A, engine.device
        self.max_hops = min(N, 256) if max_hops is None else int(max_hops)
        if not 1 <= self.max_hops <= ops.TD_ROUTES_MAX_HOPS:
            raise ValueError(f"max_hops must be in [1, {ops.TD_ROUTES_MAX_HOPS}], got {max_hops!r}")
        self.link_bin_seconds = int(link_bin_seconds)
        P = self.P = K if self.per_env else 1
        scratch = ops.td_routes_bytes(engine.plan, P, A, self.max_hops)
        if scratch < 0:
            raise _lib.TarlError("tarl_td_routes_scratch_bytes refused the replanner's sizes")
        need = 2 * 4 * P * A * self.max_hops
        free = int(torch.cuda.mem_get_info(dev)[0])
        if need + scratch > free // 2:
            raise _lib.TarlError(f"the replanner's routes ({need / 2**30:.2f} GiB for {P} plans x A = {A} agents x max_hops = "
                                 f"{self.max_hops}, current and new) and search scratch ({scratch / 2**30:.2f} GiB) exceed half "
                                 f"the free device memory ({free / 2**30:.2f} GiB free): plan fewer environments at a time "
                                 f"(per_env=False plans once) or lower max_hops")
        i32 = dict(dtype=torch.int32, device=dev)
        self.cur = (torch.zeros((P, A, self.max_hops), **i32), torch.zeros((P, A), **i32))
        self.new = (torch.zeros((P, A, self.max_hops), **i32), torch.zeros((P, A), **i32))
        self.best = torch.empty((P, A), dtype=torch.float64, device=dev)
        self.scratch = torch.empty(max(scratch, 1), dtype=torch.uint8, device=dev)
        self.hops = torch.arange(self.max_hops, device=dev)
        for k in ("occupancy", "dynamic_gap", "dynamic_gap_envs", "link_bin_seconds", "routes"):
            if k in eval_kw:
                raise ValueError(f"{k} is the replanner's own: every day runs with occupancy and the dynamic gap over all K "
                                 f"environments, in bins of link_bin_seconds")
        self.ev = VecEvaluator(engine, "routes", routes=self._plan_of(self.cur), occupancy=True, dynamic_gap=True,
                               link_bin_seconds=self.link_bin_seconds,
                               **({"route_departures": True} if route_departures else {}),
                               **({"trip_reward": True} if trip_reward else {}), **eval_kw)
        st = engine.static_node_features[0]
        mx, ff = st[:, 0].contiguous(), st[:, 2].contiguous()
        cc = engine.cc if engine.cc is not None else ff * (mx + 10 - st[:, 4] * ff / 3600)      # as VecEvaluator._gap_reserve
        self.road = (mx, ff, cc.to(torch.float32).contiguous())
        self.keep, self.history = bool(keep), []

    def _plan_of(self, pair):
        return (pair[0], pair[1]) if self.per_env else (pair[0][0], pair[1][0])

    def _plan(self, acc, frames_per_bin, days_so_far, sched):
        """Road times from the accumulated occupancy and one search per (plan, agent) -> self.new, self.best."""
        eng = self.eng
        scale = days_so_far * (1 if self.per_env else eng.B)
        fpb = torch.from_numpy((frames_per_bin.astype(np.int64) * scale).astype(np.int32)).to(eng.device)
        kw = dict(bin_seconds=sched[0], first_bin=sched[1])
        tau, env = ops.td_road_times(acc, fpb, *self.road, **kw)
        ops.td_routes(eng.plan, tau, env, eng.agents[:self.P], max_hops=self.max_hops, out=(self.best, *self.new),
                      scratch=self.scratch, **kw)

    def _differs(self):
        """(P, A) bool: the new route is not the current one (lengths, and the roads up to the new length)."""
        (cr, cl), (nr, nl) = self.cur, self.new
        live = self.hops < nl.clamp(min=0).unsqueeze(-1)
        return (cl != nl) | ((cr != nr) & live).any(-1)

    def _adopt(self, mask):
        (cr, cl), (nr, nl) = self.cur, self.new
        cr.copy_(torch.where(mask.unsqueeze(-1), nr, cr))
        cl.copy_(torch.where(mask, nl, cl))

    @torch.no_grad()
    def run(self, frames=None):
        eng, ev = self.eng, self.ev
        K, N, A, P = eng.B, eng.N, eng.A, self.P
        T = ev.episode_frames if frames is None else int(frames)
        if T < 1:
            raise ValueError("frames must be >= 1")
        eng.reset()
        t0, step, bins = int(eng.time), int(eng.timestep), self.link_bin_seconds
        first_bin = t0 // bins
        H = (t0 + (T - 1) * step) // bins - first_bin + 1
        sched = (bins, first_bin)
        frames_per_bin = np.bincount((t0 + np.arange(T, dtype=np.int64) * step) // bins - first_bin, minlength=H)
        counters = (eng.noise_counter, eng.sample_counter)
        acc = torch.zeros((P, H, N), dtype=torch.int32, device=eng.device)
        # day 0's plan: the empty network, through the same two calls; everybody adopts (no current route)
        t_plan = time.perf_counter()
        self._plan(acc, frames_per_bin, 1, sched)
        self._adopt(torch.ones((P, A), dtype=torch.bool, device=eng.device))
        torch.cuda.synchronize(eng.device)
        plan0_ms = (time.perf_counter() - t_plan) * 1000.0
        self.history = []
        records, last, exit_day = [], None, None
        for day in range(self.days):
            eng.noise_counter, eng.sample_counter = counters      # the days share their noise streams
            ev.set_routes(*self._plan_of(self.cur))
            res = ev.run(T)
            rec = dict(day=day, domain_exit=res.domain_exit, sim_ms=res.computation_time_ms)
            if res.domain_exit:      # no statistics, nothing to plan on: the loop ends here
                rec["domain_exit_frames"] = res.domain_exit_frames
                records.append(rec)
                exit_day = day
                break
            last = res
            if self.keep:
                self.history.append(dict(routes=self.cur[0].clone(), route_len=self.cur[1].clone(), agents=eng.agents.clone(),
                                         mask=None))
            t_plan = time.perf_counter()
            veh = ev.occ_acc["veh"]
            acc += veh if self.per_env else veh.sum(0, keepdim=True, dtype=torch.int32)
            self._plan(acc, frames_per_bin, day + 1, sched)
            differs = self._differs()
            p = switch_probability(self.fraction, day)
            nl, cl = self.new[1], self.cur[1]
            rec.update(switch_probability=p, differs=int(differs[:, 1:].sum()), agents=P * (A - 1),
                       without_route=int((cl[:, 1:] <= 0).sum()), overflowing=int((nl[:, 1:] < 0).sum()), switched=None)
            if day + 1 < self.days:
                g = torch.Generator().manual_seed(day_seed(self.seed, day))
                mask = (torch.rand((P, A), generator=g) < p).to(eng.device) | (cl <= 0)
                if self.keep:
                    self.history[-1]["mask"] = mask.clone()
                rec["switched"] = int((mask & differs)[:, 1:].sum())
                self._adopt(mask)
            torch.cuda.synchronize(eng.device)
            rec["plan_ms"] = (time.perf_counter() - t_plan) * 1000.0
            pe = res.dynamic_gap["per_env"]
            rg = [float((pe["tt_sum"][k] - pe["ht_sum"][k]) / pe["tt_sum"][k]) if pe["n"][k] > 0 else None for k in range(K)]
            rec["per_env"] = dict(arrived=list(res.arrived), avg_travel_time=list(res.avg_travel_time), relative_gap=rg,
                                  episode_return=list(res.episode_return))
            for key in DAY_KEYS:
                v = np.asarray([x for x in rec["per_env"][key] if x is not None], dtype=np.float64)
                rec[key] = dict(n=int(v.size), **_sample_moments(v))
            if res.trip_return is not None:      # trip_reward=True: the frames owed by all travellers, DESIGN 4.24
                rec["per_env"]["trip_return"] = list(res.trip_return)
                v = np.asarray(res.trip_return, dtype=np.float64)
                rec["trip_return"] = dict(n=int(v.size), **_sample_moments(v))
            records.append(rec)
        settings = dict(days=self.days, fraction=self.fraction, max_hops=self.max_hops, per_env=self.per_env, plans=P,
                        seed=self.seed, engine_seed=eng.seed, envs=K, frames=T, link_bin_seconds=bins, bins=int(H),
                        first_plan_ms=plan0_ms, shared_noise=True)
        return ReplanResult(days=records, last=last, routes=self.cur[0], route_len=self.cur[1], settings=settings,
                            domain_exit_day=exit_day)


# ---- the report ------------------------------------------------------------------------------------------------------------------
REPLAN_NOTE = ("every day runs on the engine's own seed and noise counters: the days share their noise streams, so the table "
               "shows what the plans change; 'differs' is the share of agents whose new quickest route is not their current "
               "one, 'switched' the share that adopted it; the last day is planned but not swapped")
REPLAN_COLUMNS = ("day", "domain_exit", "arrived", "arrived_se", "avg_travel_time", "avg_travel_time_se", "relative_gap",
                  "relative_gap_se", "switch_probability", "differs_share", "switched_share", "without_route", "overflowing",
                  "sim_ms", "plan_ms")


def replan_report(result: ReplanResult) -> dict:
    """The day table of a :class:`ReplanResult`: ``rows`` (one dict per day, ``columns`` their keys; a day that left the
    domain has no statistics), ``env_rows`` (one per day and environment), ``settings`` and the note on the shared noise."""
    rows, env_rows = [], []
    trip = any("trip_return" in r for r in result.days)       # Replanner(trip_reward=True): two more columns
    columns = list(REPLAN_COLUMNS) + (["trip_return_mean", "trip_return_se"] if trip else [])
    for r in result.days:
        row = {c: None for c in columns}
        row.update(day=r["day"], domain_exit=bool(r["domain_exit"]), sim_ms=r["sim_ms"])
        if not r["domain_exit"]:
            for key in DAY_KEYS:
                row[key], row[key + "_se"] = r[key]["mean"], r[key]["se"]
            row.update(switch_probability=r["switch_probability"], differs_share=r["differs"] / max(r["agents"], 1),
                       switched_share=None if r["switched"] is None else r["switched"] / max(r["agents"], 1),
                       without_route=r["without_route"], overflowing=r["overflowing"], plan_ms=r["plan_ms"])
            if trip:
                row["trip_return_mean"], row["trip_return_se"] = r["trip_return"]["mean"], r["trip_return"]["se"]
            for k in range(len(r["per_env"]["arrived"])):
                env_rows.append(dict(day=r["day"], env=k, **{key: r["per_env"][key][k] for key in DAY_KEYS}))
        rows.append(row)
    return dict(available=True, columns=columns, rows=rows, env_columns=["day", "env"] + list(DAY_KEYS),
                env_rows=env_rows, settings=dict(result.settings), domain_exit_day=result.domain_exit_day, note=REPLAN_NOTE)


def _pm(mean, se, fmt):
    if mean is None:
        return "-"
    return format(mean, fmt) + ("" if se is None else " +- " + format(se, fmt))


def replan_lines(report: dict):
    """:func:`replan_report` as printable lines."""
    s = report["settings"]
    out = [f"{s['days']} days, {s['envs']} environments, {s['plans']} plan(s), fraction {s['fraction']}, max_hops {s['max_hops']}, "
           f"{s['frames']} frames per day, bins of {s['link_bin_seconds']} s",
           f"{'day':>4} {'arrived':>18} {'travel time [s]':>22} {'relative gap':>20} {'differs':>8} {'switched':>9} "
           f"{'no route':>9} {'overflow':>9} {'sim ms':>9} {'plan ms':>9}"]
    for r in report["rows"]:
        if r["domain_exit"]:
            out.append(f"{r['day']:>4} domain exit: a FIFO count reached Nmax; no statistics, the loop ends here")
            continue
        sw = "-" if r["switched_share"] is None else f"{r['switched_share']:.4f}"
        out.append(f"{r['day']:>4} {_pm(r['arrived'], r['arrived_se'], '.1f'):>18} "
                   f"{_pm(r['avg_travel_time'], r['avg_travel_time_se'], '.2f'):>22} "
                   f"{_pm(r['relative_gap'], r['relative_gap_se'], '.4f'):>20} {r['differs_share']:>8.4f} {sw:>9} "
                   f"{r['without_route']:>9d} {r['overflowing']:>9d} {r['sim_ms']:>9.1f} {r['plan_ms']:>9.1f}")
    if "trip_return_mean" in report["columns"]:
        out.append("trip return per day: " + ", ".join(
            "-" if r["domain_exit"] else _pm(r["trip_return_mean"], r["trip_return_se"], ".1f") for r in report["rows"])
            + "  (-(on the way + due and waiting) summed over the frames, DESIGN 4.24)")
    out.append("note: " + report["note"])
    return out
