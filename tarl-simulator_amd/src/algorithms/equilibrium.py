"""Equilibrium metrics of the static assignment model ``run_msa`` solves: relative gap ("Nash gap"), total system travel
time, the system optimum and the Price of Anarchy.

The model is ``run_msa``'s: nodes of the dual graph are roads; entering road node v costs
``t_v(f) = ff_v (1 + 0.15 (f_v / max(cap_v, 1e-8))^4)``, SRC / DEST pseudo-nodes cost 0; a path costs the sum over
``path[1:]``; the demand is the OD count matrix of the agent table (``build_demand``). All numbers are float64.

* ``TSTT(f) = sum_roads f_v t_v(f_v)``; ``SPTT_c(f) = sum_od vol * dist_c(o, d)`` over the reachable pairs at node costs c.
* user equilibrium: relative gap ``(sum f t - SPTT_t) / sum f t``.
* system optimum: the same problem on the marginal cost ``m_v(f) = d(f t_v)/df = ff_v (1 + 0.75 (f_v / cap_v)^4)``; its gap
  is the same expression with m in place of t, and by convexity ``TSTT(f) - (sum f m - SPTT_m)`` is a lower bound on the
  optimal system cost from ANY feasible flow f.
* Volume of OD pairs no path serves is reported apart (``unrouted_volume``) and enters no sum.

Every iteration is two launches: one all-or-nothing assignment at the costs of the current flows, which also yields the
shortest-path travel time of the demand and with it the gap of those flows (``tarl_msa_assign_sssp_gap`` per origin, or
``tarl_apsp_f64`` + ``tarl_msa_assign_gap`` below 4 096 nodes), and one ``tarl_bpr_step``: target, exact line search (or
the 1/k step), new flows and their costs, nothing read by the host. A gap is never formed from the SPTT of one flow and
the TSTT of another. The host reads one small record per checked iteration.

Solvers: ``"msa"`` (step 1/k), ``"fw"`` (Frank-Wolfe, exact line search), ``"cfw"`` (conjugate Frank-Wolfe, Mitradjieva and
Lindberg 2013).

Not covered: a gap of the SIMULATED, time-dependent trajectories (the simulator counts departures on the origin road,
which the static model skips, and a dynamic Nash gap needs time-dependent shortest paths); path- or bush-based solvers.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from .._compat import cached_plan, require_cuda
from ..feature_helpers import FeatureHelpers
from .user_equilibrium_msa import ALL_PAIRS_MAX_NODES, METHODS, build_demand

OBJECTIVES = ("ue", "so")
SOLVERS = ("cfw", "fw", "msa")


@dataclass
class AssignmentResult:
    """What is known about one flow vector. ``tstt``, ``sptt``, ``relative_gap`` all belong to ``flow``."""
    objective: str
    solver: Optional[str]
    method: str
    flow: torch.Tensor                      # float64 [N], on the device
    tstt: float                             # sum f t(f)
    objective_cost: float                   # sum f cost(f): = tstt for "ue", sum f m(f) for "so"
    sptt: float                             # at the objective's costs
    relative_gap: float
    average_excess_cost: float
    tstt_lower_bound: Optional[float]       # objective "so" only
    routed_volume: float
    unrouted_volume: float
    iterations: int = 0
    converged: bool = False
    trace: List[Tuple[float, float, float]] = field(default_factory=list)   # per iteration k: (gap of f_k, lambda_k, alpha_k)

    def scalars(self) -> dict:
        return {k: getattr(self, k) for k in ("objective", "solver", "method", "tstt", "objective_cost", "sptt",
                                              "relative_gap", "average_excess_cost", "tstt_lower_bound",
                                              "routed_volume", "unrouted_volume", "iterations", "converged")}


class _Problem:
    """Graph, demand and the device buffers one solve or one evaluation needs."""

    def __init__(self, graph, agents, method: str):
        from tarl_hip import ops
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        x = graph.x
        require_cuda(x, "graph.x")
        self.ops = ops
        self.N = N = int(x.size(0))
        self.method = ("all_pairs" if N <= ALL_PAIRS_MAX_NODES else "per_origin") if method == "auto" else method
        h = FeatureHelpers(Nmax=(int(x.size(1)) - 7) // 3)
        self.dev = dev = x.device
        self.num_roads = int(getattr(graph, "num_roads", None) or N)
        self.free_flow = x[:, h.FREE_FLOW_TIME_TRAVEL].to(torch.float64).contiguous()
        self.capacity = x[:, h.MAX_FLOW].to(torch.float64).contiguous()      # the kernel clamps at 1e-8 as run_msa does
        self.is_road = (x[:, h.ROAD_INDEX] >= 0).to(torch.uint8).contiguous()
        od_o, od_d, od_vol = build_demand(agents, N)
        self.od_o, self.od_d, self.od_vol = od_o.to(dev), od_d.to(dev), od_vol.to(dev)
        self.plan = cached_plan(graph.edge_index, N)
        self.enter = graph.edge_index[1]                  # an edge costs what its head node costs
        if self.method == "per_origin":                   # build_demand's pairs are sorted by origin
            self.origins, per = torch.unique_consecutive(self.od_o, return_counts=True)
            self.od_ptr = torch.zeros(self.origins.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(per, 0, out=self.od_ptr[1:])
            self.sptt_part = torch.zeros(self.origins.numel(), dtype=torch.float64, device=dev)
            self.unrouted_part = torch.zeros_like(self.sptt_part)
        self.aux = torch.zeros(N, dtype=torch.float64, device=dev)
        self.cost = torch.empty(N, dtype=torch.float64, device=dev)
        self.record = torch.zeros(ops.BPR_RECORD, dtype=torch.float64, device=dev)
        # [sptt, unrouted, sum f t, sum f cost, gap, -, -, total volume]: what the host reads, one small copy
        self.stats = torch.zeros(8, dtype=torch.float64, device=dev)
        self.stats[7] = self.od_vol.sum()

    def assign(self):
        """One all-or-nothing launch at ``self.cost``: fills ``self.aux`` and stats[0:2] (SPTT, unrouted volume)."""
        ops = self.ops
        self.aux.zero_()
        w = self.cost[self.enter].contiguous()
        if self.method == "per_origin":
            ops.msa_assign_trees_gap(self.plan, w, self.origins, self.od_ptr, self.od_d, self.od_vol, self.is_road,
                                     self.aux, self.sptt_part, self.unrouted_part)
            self.stats[0] = self.sptt_part.sum()
            self.stats[1] = self.unrouted_part.sum()
        else:
            next_hop = ops.all_pairs_shortest_paths(self.plan, w)[0][0]
            pc = ops.msa_assign_gap(next_hop, self.od_o, self.od_d, self.od_vol, self.is_road, self.cost, self.aux)
            ok = torch.isfinite(pc)
            zero = torch.zeros_like(pc)
            self.stats[0] = torch.where(ok, self.od_vol * pc, zero).sum()
            self.stats[1] = torch.where(ok, zero, self.od_vol).sum()

    def close_stats(self):
        """stats[2:5] from the record of the step (or evaluation) that produced the current flows and the SPTT just
        assigned: both belong to the same flow vector."""
        s = self.stats
        s[2:4] = self.record[2:4]
        s[4] = (s[3] - s[0]) / s[3]

    def result(self, flow, objective, solver, iterations, converged, trace) -> AssignmentResult:
        sptt, unrouted, tstt, fc, gap, _, _, total = self.stats.cpu().tolist()
        routed = total - unrouted
        excess = fc - sptt
        return AssignmentResult(
            objective=objective, solver=solver, method=self.method, flow=flow, tstt=tstt, objective_cost=fc, sptt=sptt,
            relative_gap=gap, average_excess_cost=excess / routed if routed > 0 else math.nan,
            # rounding can leave the excess a few ulps below zero at an exact optimum: the bound never exceeds TSTT(f)
            tstt_lower_bound=(tstt - max(excess, 0.0)) if objective == "so" else None,
            routed_volume=routed, unrouted_volume=unrouted, iterations=iterations, converged=converged, trace=trace)


def _check(objective, solver=None):
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, got {objective!r}")
    if solver is not None and solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")


def solve_assignment(graph, agents, objective: str = "ue", solver: str = "cfw", gap_tol: float = 1e-4,
                     max_iter: int = 500, method: str = "auto", check_every: int = 1,
                     flow_callback=None) -> AssignmentResult:
    """User-equilibrium (``"ue"``) or system-optimum (``"so"``) link flows.

    Iteration k assigns the demand at the costs of ``f_{k-1}`` (which gives the gap of ``f_{k-1}``), then steps. The
    first iteration is the all-or-nothing load at free flow. The loop stops when the gap of the current flows is
    ``<= gap_tol`` (looked at every ``check_every``-th iteration: the only host read of the loop) or after ``max_iter``
    steps, which are followed by one closing assignment, so the result's gap, TSTT and SPTT belong to ``flow``.
    ``flow_callback(k, flow)`` (optional, a test hook) sees the device flows after every step."""
    _check(objective, solver)
    if max_iter < 1 or check_every < 1:
        raise ValueError("max_iter and check_every must be >= 1")
    pb = _Problem(graph, agents, method)
    ops = pb.ops
    flow = torch.zeros(pb.N, dtype=torch.float64, device=pb.dev)
    target = torch.zeros_like(flow)
    trace_dev = torch.full((max_iter, 3), math.nan, dtype=torch.float64, device=pb.dev)
    # free-flow costs: the evaluation of the zero flow
    ops.bpr_step(flow, None, None, pb.free_flow, pb.capacity, pb.is_road, objective=objective, rule="eval",
                 cost_out=pb.cost, record=pb.record)
    done, converged = 0, False
    for k in range(1, max_iter + 1):
        pb.assign()
        if k > 1:
            pb.close_stats()                                   # the gap of f_{k-1}
            trace_dev[k - 2, 0] = pb.stats[4]
            if (k - 1) % check_every == 0 and float(pb.stats[4]) <= gap_tol:
                converged = True
                break
        ops.bpr_step(flow, pb.aux, target, pb.free_flow, pb.capacity, pb.is_road, objective=objective, rule=solver,
                     msa_step=1.0 / k, iteration=k, cost_out=pb.cost, record=pb.record)
        trace_dev[k - 1, 1] = pb.record[1]
        trace_dev[k - 1, 2] = pb.record[0]
        done = k
        if flow_callback is not None:
            flow_callback(k, flow)
    if not converged:                                          # the closing assignment: the gap of the returned flows
        pb.assign()
        pb.close_stats()
        trace_dev[done - 1, 0] = pb.stats[4]
    trace = [tuple(r) for r in trace_dev[:done].cpu().tolist()]
    # the closing assignment may find the target met after the last step as well
    return pb.result(flow, objective, solver, done, converged or float(pb.stats[4]) <= gap_tol, trace)


def assignment_gap(graph, agents, flow, objective: str = "ue", method: str = "auto") -> AssignmentResult:
    """The same numbers for a flow vector handed in (``run_msa``'s output, or any feasible flow): one evaluation and one
    assignment launch. ``flow``: float64 per node (or per road: shorter vectors are padded with zeros), a ``{road: flow}``
    map as ``run_msa`` returns it, on any device. With ``objective="so"`` the gap is the marginal-cost gap of that flow,
    which gives ``tstt_lower_bound`` from any feasible flow, user-equilibrium flows included."""
    _check(objective)
    pb = _Problem(graph, agents, method)
    if isinstance(flow, dict):
        vals = torch.zeros(pb.N, dtype=torch.float64)
        for r, v in flow.items():
            vals[int(r)] = float(v)
        flow = vals
    flow = torch.as_tensor(flow, dtype=torch.float64).to(pb.dev).reshape(-1)
    if flow.numel() > pb.N:
        raise ValueError(f"flow has {flow.numel()} entries for {pb.N} nodes")
    if flow.numel() < pb.N:
        flow = torch.cat([flow, torch.zeros(pb.N - flow.numel(), dtype=torch.float64, device=pb.dev)])
    flow = flow.contiguous().clone()
    pb.ops.bpr_step(flow, None, None, pb.free_flow, pb.capacity, pb.is_road, objective=objective, rule="eval",
                    cost_out=pb.cost, record=pb.record)
    pb.assign()
    pb.close_stats()
    return pb.result(flow, objective, None, 0, False, [])


def _road_map(res: AssignmentResult, num_roads: int) -> Dict[int, float]:
    return {i: float(v) for i, v in enumerate(res.flow[:num_roads].cpu().tolist())}


def equilibrium_report(graph, agents, **solver_options) -> dict:
    """Solve both problems and report them together: the UE and SO scalars, ``price_of_anarchy = TSTT(f_ue) / TSTT(f_so)``
    with the interval ``[TSTT(f_ue) / TSTT(f_so), TSTT(f_ue) / TSTT_lb]`` and both gaps (no PoA without them), and
    ``run_msa``-compatible ``{road: flow}`` maps. ``solver_options`` go to :func:`solve_assignment`."""
    solver_options.pop("objective", None)
    ue = solve_assignment(graph, agents, objective="ue", **solver_options)
    so = solve_assignment(graph, agents, objective="so", **solver_options)
    num_roads = int(getattr(graph, "num_roads", None) or graph.x.size(0))
    lb = so.tstt_lower_bound
    return {
        "ue": ue.scalars(), "so": so.scalars(),
        "price_of_anarchy": ue.tstt / so.tstt if so.tstt > 0 else math.nan,
        "price_of_anarchy_interval": [ue.tstt / so.tstt if so.tstt > 0 else math.nan,
                                      ue.tstt / lb if lb and lb > 0 else math.inf],
        "relative_gap_ue": ue.relative_gap, "relative_gap_so": so.relative_gap,
        "tstt_ue": ue.tstt, "tstt_so": so.tstt, "tstt_lower_bound": lb,
        "unrouted_volume": ue.unrouted_volume,
        "ue_flows": _road_map(ue, num_roads), "so_flows": _road_map(so, num_roads),
        "ue_result": ue, "so_result": so,
    }
