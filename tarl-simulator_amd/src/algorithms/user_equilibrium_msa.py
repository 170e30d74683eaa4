"""Method of Successive Averages on the device (reference: src/algorithms/user_equilibrium_msa.py:65-165).

``run_msa(graph, agents)`` post-processes a simulation snapshot into deterministic user-equilibrium link flows: build
the OD demand from the agents' trips, then iterate {all-or-nothing assignment on the current shortest paths, MSA
averaging of the flows, BPR update of the link costs} until the L1 change of the flows drops below ``tol``.

Where the reference walks ``nx.shortest_path`` per OD pair on the host, this build has two device methods, both on
float64 costs as the reference keeps them:

* ``"all_pairs"``: the all-pairs next-hop table once per iteration with ``tarl_apsp_f64`` and every OD pair walked
  along it with ``tarl_msa_assign`` (one thread per pair, fp64 atomics). O(N^2) memory per iteration.
* ``"per_origin"``: one shortest-path tree per distinct origin of the demand with ``tarl_msa_assign_sssp`` (one
  workgroup per origin; its OD pairs walk the tree inside the same launch). O(E) work per tree, O(workgroups x N)
  scratch, no N^2 table. Tie rule: among the exact shortest paths take the fewest hops, then at every node the
  smallest predecessor id.
* ``"auto"`` (default): all_pairs for N <= 4096, per_origin above.

Shortest-path COSTS are unique; when two paths tie exactly the reference's bidirectional Dijkstra and either tie rule may
pick different ones (regular grids at free flow) — the flows then differ by how the tied volume is routed, the
equilibrium cost does not.
"""
from __future__ import annotations

from typing import Dict

import torch

from .._compat import cached_plan, require_cuda
from ..feature_helpers import FeatureHelpers

ALPHA, BETA = 0.15, 4.0    # BPR parameters of the reference
ALL_PAIRS_MAX_NODES = 4096  # "auto" keeps the all-pairs table up to this size
METHODS = ("auto", "all_pairs", "per_origin")


def build_demand(agents, num_nodes: int):
    """Distinct (origin, destination) pairs of the trips (row 0 = dummy agent is skipped) and their volumes."""
    feats = agents.agent_features
    dev = feats.device if feats is not None else "cuda"
    if feats is None or feats.size(0) <= 1:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return e, e.clone(), torch.zeros(0, dtype=torch.float64, device=dev)
    flat = feats[1:, agents.ORIGIN].to(torch.int64) * num_nodes + feats[1:, agents.DESTINATION].to(torch.int64)
    pairs, counts = torch.unique(flat, return_counts=True)
    return (torch.div(pairs, num_nodes, rounding_mode="floor").contiguous(), (pairs % num_nodes).contiguous(),
            counts.to(torch.float64).contiguous())


def run_msa(graph, agents, tol: float = 1e-5, max_iter: int = 1000, method: str = "auto") -> Dict[int, float]:
    from tarl_hip import ops
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    x = graph.x
    require_cuda(x, "graph.x")
    N = int(x.size(0))
    if method == "auto":
        method = "all_pairs" if N <= ALL_PAIRS_MAX_NODES else "per_origin"
    h = FeatureHelpers(Nmax=(int(x.size(1)) - 7) // 3)
    num_roads = int(getattr(graph, "num_roads", N))
    free_flow = x[:, h.FREE_FLOW_TIME_TRAVEL].to(torch.float64)
    capacity = x[:, h.MAX_FLOW].to(torch.float64).clamp(min=1e-8)
    is_road = x[:, h.ROAD_INDEX] >= 0
    road_u8 = is_road.to(torch.uint8).contiguous()
    od_o, od_d, od_vol = build_demand(agents, N)
    od_o, od_d, od_vol = od_o.to(x.device), od_d.to(x.device), od_vol.to(x.device)
    flow = torch.zeros(N, dtype=torch.float64, device=x.device)
    cost = torch.where(is_road, free_flow, torch.zeros_like(free_flow))
    plan = cached_plan(graph.edge_index, N)
    enter = graph.edge_index[1]                       # an edge costs what its head node costs
    if method == "per_origin":                        # build_demand's pairs are sorted by origin
        origins, per = torch.unique_consecutive(od_o, return_counts=True)
        od_ptr = torch.zeros(origins.numel() + 1, dtype=torch.int64, device=x.device)
        torch.cumsum(per, 0, out=od_ptr[1:])
    for it in range(1, max_iter + 1):
        aux = torch.zeros_like(flow)
        if method == "per_origin":
            ops.msa_assign_trees(plan, cost[enter].contiguous(), origins, od_ptr, od_d, od_vol, road_u8, aux)
        else:
            next_hop = ops.all_pairs_shortest_paths(plan, cost[enter].contiguous())[0][0]
            ops.msa_assign(next_hop, od_o, od_d, od_vol, road_u8, aux)
        prev = flow.clone()
        flow += (1.0 / it) * (aux - flow)
        cost = torch.where(is_road, free_flow * (1.0 + ALPHA * (flow / capacity) ** BETA), cost)
        if float((flow - prev).abs().sum()) < tol:
            break
    out = flow[:num_roads].cpu().tolist()
    return {i: float(v) for i, v in enumerate(out)}
