"""Thin, validated wrappers over the C ABI (include/tarl_hip.h). Tensors in, tensors out; no compute happens in Python
and there is no fallback: every function enqueues hand-written HIP kernels on torch's current stream.

Batched state convention: ``x`` is fp32 ``(R, F)`` or ``(B, R, F)`` (last dim contiguous, arbitrary row / env
strides), mutated in place like the reference does.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref

import torch

from . import lib as _lib

EPS_GUMBEL = 1e-12   # src/direction_mpnn.py:136
# revision of the fused path's packed HBM layout / kernel set: a PMC traffic record (profiles/*_pmc_traffic.json) only
# applies to the revision it was measured on
FUSED_LAYOUT = "v11"


# the three frame kernels with their launch dispatch, and every csrc header they include: what a PMC traffic record measured.
# (Pack, export, the action draw and the host loops are not in it; the packed layout is, through fused_common.h.)
FRAME_KERNEL_SOURCES = ("fused_direction.hip", "fused_rows.hip", "fused_insert.hip",
                        "fused_common.h", "fused_frame.h", "fused_choice.h", "tarl_common.h")


def frame_kernel_source_hash(csrc: str | None = None) -> str:
    """sha256 (first 16 hex digits) of FRAME_KERNEL_SOURCES, in that order: a PMC traffic record (tools/pmc_bench.py ->
    profiles/*.json) is only paired with kernel times measured on the very code it was taken on. ``csrc``: another directory
    holding the sources (default: this tree's csrc/)."""
    import hashlib
    h = hashlib.sha256()
    if csrc is None:
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    for name in FRAME_KERNEL_SOURCES:
        with open(os.path.join(csrc, name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _check_dev(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.TarlError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")


def _contig(t: torch.Tensor, dtype, name: str):
    _check_dev(t, dtype, name)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _state(x: torch.Tensor, Nmax: int):
    """-> (B, rows, x_bstride, ldx)."""
    _check_dev(x, torch.float32, "x")
    if x.dim() not in (2, 3) or x.stride(-1) != 1 or x.size(-1) < 3 * Nmax + 7:
        raise ValueError(f"x must be (R,F) or (B,R,F) with F >= 3*Nmax+7 and a contiguous last dim, got {tuple(x.shape)}")
    if x.dim() == 2:
        return 1, x.size(0), x.size(0) * x.stride(0), x.stride(0)
    return x.size(0), x.size(1), x.stride(0), x.stride(1)


def _agents(a: torch.Tensor, B: int):
    """-> (A, a_bstride)."""
    _check_dev(a, torch.float32, "agent_features")
    if a.size(-1) != 9 or a.stride(-1) != 1 or a.stride(-2) != 9:
        raise ValueError("agent_features must be (A,9) or (B,A,9) with contiguous rows")
    if a.dim() == 2:
        if B != 1:
            raise ValueError("batched state needs batched agent_features (B,A,9)")
        return a.size(0), a.size(0) * 9
    if a.size(0) != B:
        raise ValueError("agent_features batch does not match x")
    return a.size(1), a.stride(0)


class Plan:
    """Static per-graph plan (``tarl_plan_create``): int32 CSC/CSR built once on the host and kept on the device."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, src_order: torch.Tensor | None = None):
        L = _lib.load()
        ei = edge_index.detach().to("cpu", torch.int64).contiguous()
        if ei.dim() != 2 or ei.size(0) != 2:
            raise ValueError("edge_index must be (2, E)")
        so = None if src_order is None else src_order.detach().to("cpu", torch.int64).contiguous()
        handle = C.c_void_p()
        _lib.check(L.tarl_plan_create(ei.data_ptr(), ei.size(1), int(num_nodes), _lib.ptr(so), C.byref(handle)))
        self._h = handle
        self._finalizer = weakref.finalize(self, L.tarl_plan_destroy, handle)
        info = (C.c_int64 * 6)()
        _lib.check(L.tarl_plan_info(handle, info))
        self.num_nodes, self.num_edges, self.num_groups, self.max_in, self.max_out, src_sorted = [int(v) for v in info]
        self.src_sorted = bool(src_sorted)
        geo = (C.c_int64 * 3)()
        _lib.check(L.tarl_plan_geometry(handle, geo))
        self.siblings4, self.row_siblings, self.num_row_chunks = bool(geo[0]), bool(geo[1]), int(geo[2])
        self.device = torch.device("cuda", torch.cuda.current_device())

    @property
    def handle(self):
        return self._h


_LOG_EPS = None


def log_eps() -> float:
    """fp32 ``log(0 + 1e-12)`` evaluated by torch on the CPU, as the reference does (src/direction_mpnn.py:138)."""
    global _LOG_EPS
    if _LOG_EPS is None:
        _LOG_EPS = float(torch.log(torch.zeros(1, dtype=torch.float32) + EPS_GUMBEL)[0])
    return _LOG_EPS


class EdgeConst:
    """Per-graph edge constants on the device: ``edge_attr`` (E,) and ``log(edge_attr + 1e-12)`` evaluated on the CPU
    with torch so that the Gumbel-max scores are bit-identical to the reference's."""

    def __init__(self, edge_attr: torch.Tensor, device):
        ea = edge_attr.detach().to("cpu", torch.float32).reshape(-1).contiguous()
        self.edge_attr = ea.to(device)
        self.log_edge_attr = torch.log(ea + EPS_GUMBEL).to(device)
        self.log_eps = log_eps()


def gumbel_from_uniform_cpu(u: torch.Tensor) -> torch.Tensor:
    """``-log(-log(u))`` evaluated on the CPU (parity runs feed the reference's own noise, src/direction_mpnn.py:137)."""
    u = u.detach().to("cpu", torch.float32)
    return -torch.log(-torch.log(u))


def direction_step(plan: Plan, x, Nmax, ec: EdgeConst, t, *, congestion_constant=None, gumbel=None, seed=0, counter=0,
                   want_dtt=True, chosen=None, status=None):
    """DirectionMPNN.forward on B environments. Returns (delta_travel_time (B,E) or None, chosen (B,R))."""
    L = _lib.load()
    B, R, bs, ldx = _state(x, Nmax)
    E = plan.num_edges
    if chosen is None:
        chosen = torch.empty((B, R), dtype=torch.float32, device=x.device)
    dtt = torch.empty((B, E), dtype=torch.float32, device=x.device) if want_dtt else None
    if gumbel is not None:
        _contig(gumbel, torch.float32, "gumbel")
        if gumbel.numel() != B * E:
            raise ValueError("gumbel must hold B*E values")
    if congestion_constant is not None:
        _contig(congestion_constant, torch.float32, "congestion_constant")
        if congestion_constant.numel() < R:
            raise ValueError("congestion_constant shorter than num_roads")
    _lib.check(L.tarl_direction_step(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, R, ec.edge_attr.data_ptr(),
                                     ec.log_edge_attr.data_ptr(), ec.log_eps, _lib.ptr(congestion_constant), float(t),
                                     _lib.ptr(gumbel), int(seed), int(counter), _lib.ptr(dtt), chosen.data_ptr(),
                                     _lib.ptr(status), _lib.current_stream()))
    return dtt, chosen


def response_step(plan: Plan, x, Nmax, *, popped=None, any_flag=None):
    """ResponseMPNN.forward on B environments. Returns popped (B,R) uint8; ``any_flag`` int32[1] set on device."""
    L = _lib.load()
    B, R, bs, ldx = _state(x, Nmax)
    if popped is None:
        popped = torch.empty((B, R), dtype=torch.uint8, device=x.device)
    _lib.check(L.tarl_response_step(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, R, popped.data_ptr(),
                                    _lib.ptr(any_flag), _lib.current_stream()))
    return popped


def core_step(plan: Plan, x, Nmax, ec: EdgeConst, t, *, congestion_constant=None, gumbel=None, seed=0, counter=0,
              want_dtt=True, chosen=None, popped=None, any_flag=None, status=None):
    """SimulationCoreModel.forward (both rounds). Returns (dtt or None, popped)."""
    L = _lib.load()
    B, R, bs, ldx = _state(x, Nmax)
    E = plan.num_edges
    if chosen is None:
        chosen = torch.empty((B, R), dtype=torch.float32, device=x.device)
    if popped is None:
        popped = torch.empty((B, R), dtype=torch.uint8, device=x.device)
    dtt = torch.empty((B, E), dtype=torch.float32, device=x.device) if want_dtt else None
    if gumbel is not None:
        _contig(gumbel, torch.float32, "gumbel")
    _lib.check(L.tarl_core_step(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, R, ec.edge_attr.data_ptr(),
                                ec.log_edge_attr.data_ptr(), ec.log_eps, _lib.ptr(congestion_constant), float(t),
                                _lib.ptr(gumbel), int(seed), int(counter), _lib.ptr(dtt), chosen.data_ptr(),
                                popped.data_ptr(), _lib.ptr(any_flag), _lib.ptr(status), _lib.current_stream()))
    return dtt, popped


def apply_action(plan: Plan, x, Nmax, *, action_onehot=None, choice=None):
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    if N != plan.num_nodes:
        raise ValueError("x rows must equal the plan's node count")
    if action_onehot is not None:
        _contig(action_onehot, torch.int64, "action")
    if choice is not None:
        _contig(choice, torch.int32, "choice")
    _lib.check(L.tarl_apply_action(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, _lib.ptr(action_onehot),
                                   _lib.ptr(choice), _lib.current_stream()))


def withdraw_step(plan: Plan, x, Nmax, agent_features, t, *, withdrawn=None, want_mask=True):
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    if withdrawn is None and want_mask:
        withdrawn = torch.empty((B, N), dtype=torch.uint8, device=x.device)
    _lib.check(L.tarl_withdraw_step(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, N, agent_features.data_ptr(), A, abs_,
                                    float(t), _lib.ptr(withdrawn), _lib.current_stream()))
    return withdrawn


def insert_step(x, Nmax, agent_features, t, *, congestion_constant=None, scratch=None, reward=None, counts=None):
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    if scratch is None:
        scratch = torch.empty((B, 2 * A), dtype=torch.int32, device=x.device)
    _lib.check(L.tarl_insert_step(x.data_ptr(), B, bs, ldx, Nmax, N, agent_features.data_ptr(), A, abs_,
                                  _lib.ptr(congestion_constant), float(t), scratch.data_ptr(), _lib.ptr(reward),
                                  _lib.ptr(counts), _lib.current_stream()))


# ---- shortest-path routing -------------------------------------------------------------------------------------------------
def edge_travel_time(plan: Plan, x, Nmax, congestion_constant):
    """(B, E) current travel time of every edge, original edge order (src/agents/base.py:541-550)."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    out = torch.empty((B, plan.num_edges), dtype=torch.float32, device=x.device)
    cc = congestion_constant.to(torch.float32).contiguous()
    _lib.check(L.tarl_edge_travel_time(plan.handle, x.data_ptr(), B, bs, ldx, Nmax, cc.data_ptr(), out.data_ptr(),
                                       _lib.current_stream()))
    return out


def all_pairs_shortest_paths(plan: Plan, weights, *, want_next_hop=True, want_dist=False):
    """``weights`` (E,) or (B, E) fp32 in original edge order -> (next_hop int64 (B, N, N) | None, dist fp32 (B, N, N) |
    None), networkx-compatible tie order (tarl_apsp)."""
    L = _lib.load()
    f64 = weights.dtype == torch.float64          # double weights stay double (tarl_apsp_f64)
    w = weights.contiguous() if f64 else weights.to(torch.float32).contiguous()
    w = w.view(1, -1) if w.dim() == 1 else w
    B, N = w.size(0), plan.num_nodes
    assert w.size(1) == plan.num_edges, "one weight per edge"
    nh = torch.empty((B, N, N), dtype=torch.int64, device=w.device) if want_next_hop else None
    d = torch.empty((B, N, N), dtype=torch.float32, device=w.device) if want_dist else None
    need = int(L.tarl_apsp_scratch_bytes(plan.handle, B))
    scratch = torch.empty(need, dtype=torch.uint8, device=w.device) if need > 0 else None
    fn = L.tarl_apsp_f64 if f64 else L.tarl_apsp
    _lib.check(fn(plan.handle, w.data_ptr(), B, plan.num_edges, _lib.ptr(scratch), need, _lib.ptr(nh), _lib.ptr(d),
                  _lib.current_stream()))
    return nh, d


def msa_assign(next_hop, od_origin, od_dest, od_volume, is_road, aux_flow):
    """All-or-nothing assignment: aux_flow (N,) float64 += volume of every OD pair on the road nodes of its path."""
    L = _lib.load()
    N = next_hop.size(-1)
    for t, dt, nm in ((next_hop, torch.int64, "next_hop"), (od_origin, torch.int64, "od_origin"),
                      (od_dest, torch.int64, "od_dest"), (od_volume, torch.float64, "od_volume"),
                      (is_road, torch.uint8, "is_road"), (aux_flow, torch.float64, "aux_flow")):
        _contig(t, dt, nm)
    _lib.check(L.tarl_msa_assign(next_hop.data_ptr(), N, od_origin.data_ptr(), od_dest.data_ptr(), od_volume.data_ptr(),
                                 od_origin.numel(), is_road.data_ptr(), aux_flow.data_ptr(), _lib.current_stream()))


def _tree_check(plan: Plan, weights, wdtype, roots, name, od=None):
    """The checks every shortest-path tree wrapper shares (csrc/sp_trees.h), all before the first library call:
    ``weights`` (E,) of ``wdtype`` and ``roots`` (R,) int64 (``name`` in the messages), both contiguous on the device;
    ``od`` = the (od_ptr, od_dest, od_volume, is_road, aux_flow) of an assignment. -> R."""
    _contig(weights, wdtype, "weights")
    _contig(roots, torch.int64, name)
    if weights.dim() != 1 or weights.numel() != plan.num_edges:
        raise ValueError(f"weights must be ({plan.num_edges},) {str(wdtype).split('.')[-1]} in original edge order, got "
                         f"{tuple(weights.shape)}")
    if roots.dim() != 1:
        raise ValueError(f"{name} must be 1-D")
    if od is not None:
        od_ptr, od_dest, od_volume, is_road, aux_flow = od
        for t, dt, nm in ((od_ptr, torch.int64, "od_ptr"), (od_dest, torch.int64, "od_dest"),
                          (od_volume, torch.float64, "od_volume"), (is_road, torch.uint8, "is_road"),
                          (aux_flow, torch.float64, "aux_flow")):
            _contig(t, dt, nm)
        if od_ptr.numel() != roots.numel() + 1 or od_volume.numel() != od_dest.numel():
            raise ValueError("od_ptr must have num_origins + 1 entries and od_volume one per od_dest")
        if is_road.numel() != plan.num_nodes or aux_flow.numel() != plan.num_nodes:
            raise ValueError("is_road and aux_flow need one entry per node")
    return roots.numel()


def _tree_scratch(plan: Plan, weights, R, scratch_query):
    """-> (L, the bytes ``scratch_query`` asks for R roots, a scratch buffer of that size or None)."""
    L = _lib.load()
    need = int(getattr(L, scratch_query)(plan.handle, R))
    scratch = torch.empty(need, dtype=torch.uint8, device=weights.device) if need > 0 else None
    return L, need, scratch


def shortest_path_trees(plan: Plan, weights, sources, *, want_dist=True, want_pred=True):
    """One shortest-path tree per source (tarl_sssp_f64): ``weights`` (E,) float64 in original edge order, ``sources``
    (S,) int64 -> (dist float64 (S, N) | None, pred int32 (S, N) | None). dist is Dijkstra's left-to-right fp64 sum (+inf:
    unreachable); pred[v] = the smallest-id tight in-neighbour among those fewest tight hops from the source (-1 for
    the source and unreachable nodes). Rows of out-of-range sources are left as allocated (uninitialised)."""
    if not (want_dist or want_pred):
        raise ValueError("no output requested")
    S = _tree_check(plan, weights, torch.float64, sources, "sources")
    L, need, scratch = _tree_scratch(plan, weights, S, "tarl_msa_scratch_bytes")
    N = plan.num_nodes
    d = torch.empty((S, N), dtype=torch.float64, device=weights.device) if want_dist else None
    p = torch.empty((S, N), dtype=torch.int32, device=weights.device) if want_pred else None
    _lib.check(L.tarl_sssp_f64(plan.handle, weights.data_ptr(), sources.data_ptr(), S, _lib.ptr(scratch), need,
                               _lib.ptr(d), _lib.ptr(p), _lib.current_stream()))
    return d, p


def msa_assign_trees(plan: Plan, weights, origins, od_ptr, od_dest, od_volume, is_road, aux_flow):
    """All-or-nothing assignment along per-origin trees (tarl_msa_assign_sssp): the OD pairs sorted by origin, those of
    ``origins[j]`` at ``[od_ptr[j], od_ptr[j+1])``; aux_flow (N,) float64 += volume of every pair on the road nodes of
    its path (origin excluded). Same semantics as :func:`msa_assign` on the all-pairs table."""
    S = _tree_check(plan, weights, torch.float64, origins, "origins", od=(od_ptr, od_dest, od_volume, is_road, aux_flow))
    L, need, scratch = _tree_scratch(plan, weights, S, "tarl_msa_scratch_bytes")
    _lib.check(L.tarl_msa_assign_sssp(plan.handle, weights.data_ptr(), origins.data_ptr(), S, od_ptr.data_ptr(),
                                      od_dest.data_ptr(), od_volume.data_ptr(), is_road.data_ptr(), _lib.ptr(scratch),
                                      need, aux_flow.data_ptr(), _lib.current_stream()))


# ---- equilibrium metrics (csrc/equilibrium.hip, csrc/msa.hip) -----------------------------------------------------------------
BPR_OBJECTIVES = {"ue": 0, "so": 1}                      # TARL_BPR_UE / TARL_BPR_SO
BPR_RULES = {"msa": 0, "fw": 1, "cfw": 2, "eval": 3}     # TARL_BPR_MSA / FW / CFW / EVAL
BPR_RECORD = 8                                            # {alpha, lambda, sum f t, sum f cost, g(0), g(1), halvings, iteration}


def _same_device(ref, *tensors):
    for t in tensors:
        if t.device != ref.device:
            raise ValueError("all tensors must live on the same device")


def msa_assign_trees_gap(plan: Plan, weights, origins, od_ptr, od_dest, od_volume, is_road, aux_flow, sptt_part=None,
                         unrouted_part=None):
    """:func:`msa_assign_trees` that also returns ``(sptt_part, unrouted_part)``, float64 ``(num_origins,)``: per origin
    the sum, in pair order, of ``volume * dist[dest]`` over its reachable pairs, and the volume of the unreachable ones
    (tarl_msa_assign_sssp_gap; no atomics on these two, so they repeat bit for bit)."""
    S = _tree_check(plan, weights, torch.float64, origins, "origins", od=(od_ptr, od_dest, od_volume, is_road, aux_flow))
    if sptt_part is None:
        sptt_part = torch.zeros(S, dtype=torch.float64, device=weights.device)
    if unrouted_part is None:
        unrouted_part = torch.zeros(S, dtype=torch.float64, device=weights.device)
    for t, nm in ((sptt_part, "sptt_part"), (unrouted_part, "unrouted_part")):
        _contig(t, torch.float64, nm)
        if t.numel() != S:
            raise ValueError(f"{nm} needs one entry per origin")
    _same_device(weights, origins, od_ptr, od_dest, od_volume, is_road, aux_flow, sptt_part, unrouted_part)
    L, need, scratch = _tree_scratch(plan, weights, S, "tarl_msa_scratch_bytes")
    _lib.check(L.tarl_msa_assign_sssp_gap(plan.handle, weights.data_ptr(), origins.data_ptr(), S, od_ptr.data_ptr(),
                                          od_dest.data_ptr(), od_volume.data_ptr(), is_road.data_ptr(),
                                          _lib.ptr(scratch), need, aux_flow.data_ptr(), sptt_part.data_ptr(),
                                          unrouted_part.data_ptr(), _lib.current_stream()))
    return sptt_part, unrouted_part


def msa_assign_gap(next_hop, od_origin, od_dest, od_volume, is_road, node_cost, aux_flow, pair_cost=None):
    """:func:`msa_assign` that also returns ``pair_cost`` float64 ``(num_pairs,)``: the left-to-right sum of ``node_cost``
    over the nodes each pair enters, +inf where there is no path (tarl_msa_assign_gap)."""
    for t, dt, nm in ((next_hop, torch.int64, "next_hop"), (od_origin, torch.int64, "od_origin"),
                      (od_dest, torch.int64, "od_dest"), (od_volume, torch.float64, "od_volume"),
                      (is_road, torch.uint8, "is_road"), (node_cost, torch.float64, "node_cost"),
                      (aux_flow, torch.float64, "aux_flow")):
        _contig(t, dt, nm)
    if next_hop.dim() != 2 or next_hop.size(0) != next_hop.size(1):
        raise ValueError(f"next_hop must be (N, N), got {tuple(next_hop.shape)}")
    N, P = next_hop.size(0), od_origin.numel()
    if od_dest.numel() != P or od_volume.numel() != P:
        raise ValueError("od_origin, od_dest and od_volume need one entry per pair")
    if is_road.numel() != N or node_cost.numel() != N or aux_flow.numel() != N:
        raise ValueError("is_road, node_cost and aux_flow need one entry per node")
    if pair_cost is None:
        pair_cost = torch.empty(P, dtype=torch.float64, device=next_hop.device)
    _contig(pair_cost, torch.float64, "pair_cost")
    if pair_cost.numel() != P:
        raise ValueError("pair_cost needs one entry per pair")
    _same_device(next_hop, od_origin, od_dest, od_volume, is_road, node_cost, aux_flow, pair_cost)
    L = _lib.load()
    _lib.check(L.tarl_msa_assign_gap(next_hop.data_ptr(), N, od_origin.data_ptr(), od_dest.data_ptr(),
                                     od_volume.data_ptr(), P, is_road.data_ptr(), node_cost.data_ptr(),
                                     aux_flow.data_ptr(), pair_cost.data_ptr(), _lib.current_stream()))
    return pair_cost


def bpr_step(flow, aon_flow, target_prev, free_flow, capacity, is_road, *, objective="ue", rule="fw", msa_step=0.0,
             iteration=2, cost_out=None, record=None):
    """The step between two all-or-nothing assignments in one launch (tarl_bpr_step): forms the target (``cfw``: the
    conjugate combination with ``target_prev``), finds the step (``msa``: ``msa_step``; else the exact line search),
    updates ``flow`` and ``target_prev`` IN PLACE and returns ``(cost_out, record)``: the objective's node costs at the
    new flow (0 off the roads) and the float64 record ``[alpha, lambda, sum f t, sum f cost, g(0), g(1), halvings,
    iteration]``. ``iteration <= 1`` is the first load (``lambda = 1``). ``rule="eval"`` changes nothing and evaluates
    ``flow`` (``aon_flow`` and ``target_prev`` may be None)."""
    if objective not in BPR_OBJECTIVES:
        raise ValueError(f"objective must be one of {tuple(BPR_OBJECTIVES)}, got {objective!r}")
    if rule not in BPR_RULES:
        raise ValueError(f"rule must be one of {tuple(BPR_RULES)}, got {rule!r}")
    msa_step = float(msa_step)
    if rule == "msa" and not 0.0 <= msa_step <= 1.0:
        raise ValueError("msa_step must lie in [0, 1]")
    N = flow.numel() if isinstance(flow, torch.Tensor) else 0
    need = [(flow, torch.float64, "flow"), (free_flow, torch.float64, "free_flow"),
            (capacity, torch.float64, "capacity"), (is_road, torch.uint8, "is_road")]
    if rule != "eval" or aon_flow is not None:
        need.append((aon_flow, torch.float64, "aon_flow"))
    if rule != "eval" or target_prev is not None:
        need.append((target_prev, torch.float64, "target_prev"))
    if cost_out is not None:
        need.append((cost_out, torch.float64, "cost_out"))
    for t, dt, nm in need:
        _contig(t, dt, nm)
        if t.dim() != 1 or t.numel() != N:
            raise ValueError(f"{nm} must be ({N},), got {tuple(t.shape)}")
    if record is not None:
        _contig(record, torch.float64, "record")
        if record.numel() != BPR_RECORD:
            raise ValueError(f"record must hold {BPR_RECORD} float64 values")
    if cost_out is None:
        cost_out = torch.empty(N, dtype=torch.float64, device=flow.device)
    if record is None:
        record = torch.zeros(BPR_RECORD, dtype=torch.float64, device=flow.device)
    _same_device(flow, *[t for t, _, _ in need], cost_out, record)
    L = _lib.load()
    _lib.check(L.tarl_bpr_step(flow.data_ptr(), _lib.ptr(aon_flow), _lib.ptr(target_prev), free_flow.data_ptr(),
                               capacity.data_ptr(), is_road.data_ptr(), N, BPR_OBJECTIVES[objective], BPR_RULES[rule],
                               msa_step, int(iteration), cost_out.data_ptr(), record.data_ptr(),
                               _lib.current_stream()))
    return cost_out, record


def select_next_hop(x, Nmax, agent_features, next_hop):
    """x[b, i, SELECTED_ROAD] = next_hop[b, i, DESTINATION[head agent of i]] (src/agents/base.py:572-580)."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    nh = next_hop.view(-1, N, N)
    assert nh.dtype == torch.int64 and nh.is_contiguous() and nh.size(0) in (1, B)
    _lib.check(L.tarl_select_next_hop(x.data_ptr(), B, bs, ldx, Nmax, N, agent_features.data_ptr(), A, abs_,
                                      nh.data_ptr(), 0 if nh.size(0) == 1 else N * N, _lib.current_stream()))


def destination_trees(plan: Plan, weights, dests, *, want_next_hop=True, want_dist=False):
    """One reverse shortest-path tree per destination (tarl_dest_trees): ``weights`` (E,) fp32 in original edge order
    (what :func:`edge_travel_time` writes), ``dests`` (D,) int64 -> (next_hop int32 (D, N) | None, dist float64 (D, N) |
    None). dist[j, u] is the fp64 sum w1 + (w2 + (...)) of the shortest path u -> dests[j] (+inf: unreachable);
    next_hop[j, u] = the successor of u on a tight out-edge, the fewest tight hops to the destination first, then the
    smallest id (the destination itself on its own column, -1: unreachable). Rows of out-of-range destinations are left
    as allocated (uninitialised)."""
    if not (want_next_hop or want_dist):
        raise ValueError("no output requested")
    D = _tree_check(plan, weights, torch.float32, dests, "dests")
    L, need, scratch = _tree_scratch(plan, weights, D, "tarl_dest_trees_scratch_bytes")
    N = plan.num_nodes
    nh = torch.empty((D, N), dtype=torch.int32, device=weights.device) if want_next_hop else None
    d = torch.empty((D, N), dtype=torch.float64, device=weights.device) if want_dist else None
    _lib.check(L.tarl_dest_trees(plan.handle, weights.data_ptr(), dests.data_ptr(), D, _lib.ptr(scratch), need,
                                 _lib.ptr(nh), _lib.ptr(d), _lib.current_stream()))
    return nh, d


def select_next_hop_dest(x, Nmax, agent_features, dest_slot, next_hop):
    """x[b, i, SELECTED_ROAD] = next_hop[dest_slot[DESTINATION[head agent of i]], i] (tarl_select_next_hop_dest): the
    (D, N) int32 table of :func:`destination_trees`, shared by the environments; ``dest_slot`` (N,) int32 is the table
    row of each destination, -1 = no tree (the row keeps its selection)."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    _contig(dest_slot, torch.int32, "dest_slot")
    _contig(next_hop, torch.int32, "next_hop")
    if dest_slot.dim() != 1 or dest_slot.numel() != N or next_hop.dim() != 2 or next_hop.size(1) != N:
        raise ValueError(f"dest_slot must be ({N},) and next_hop (D, {N}), got {tuple(dest_slot.shape)} and "
                         f"{tuple(next_hop.shape)}")
    _lib.check(L.tarl_select_next_hop_dest(x.data_ptr(), B, bs, ldx, Nmax, N, agent_features.data_ptr(), A, abs_,
                                           dest_slot.data_ptr(), next_hop.data_ptr(), next_hop.size(0),
                                           _lib.current_stream()))


# ---- the shortest-path baseline on the packed state (tarl_hip/evaluator.py, head "dijkstra") ---------------------------------
def fused_edge_travel_time(plan: Plan, fs, out=None):
    """:func:`edge_travel_time` on the packed state (tarl_fused_edge_travel_time): (B, E) fp32, original edge order,
    bit-identical to ``edge_travel_time`` on the exported ``x``."""
    L = _lib.load()
    E = plan.num_edges
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    if out is None:
        out = torch.empty((fs.B, E), dtype=torch.float32, device=fs.sel8.device)
    _contig(out, torch.float32, "out")
    if out.dim() != 2 or out.size(0) != fs.B or out.size(1) != E:
        raise ValueError(f"out must be (B, E) = ({fs.B}, {E}), got {tuple(out.shape)}")
    _lib.check(L.tarl_fused_edge_travel_time(plan.handle, fs.ref, fs.B, out.data_ptr(), _lib.current_stream()))
    return out


def destination_trees_batched_bytes(plan: Plan, B: int, num_dests: int):
    """-> (table bytes, scratch bytes) of :func:`destination_trees_batched` for ``B`` weight sets and ``num_dests``
    destinations; scratch is -1 for a bad argument."""
    return (4 * int(B) * int(num_dests) * plan.num_nodes,
            int(_lib.load().tarl_dest_trees_batched_scratch_bytes(plan.handle, int(B), int(num_dests))))


def destination_trees_batched(plan: Plan, weights, dests, *, B=None, out=None, scratch=None):
    """:func:`destination_trees` for B weight sets at once (tarl_dest_trees_batched): ``weights`` (B, E) fp32, or (E,)
    with ``B`` given (one set shared by B slices), ``dests`` (D,) int64 -> next_hop int32 (B, D, N); slice ``[b]`` equals
    ``destination_trees(plan, weights[b], dests)`` bit for bit. ``out`` / ``scratch`` (uint8): caller-owned buffers (rows of
    out-of-range destinations keep what ``out`` held)."""
    _contig(weights, torch.float32, "weights")
    _contig(dests, torch.int64, "dests")
    E, N = plan.num_edges, plan.num_nodes
    if weights.dim() == 1 and weights.numel() == E and B is not None:
        B, stride = int(B), 0
    elif weights.dim() == 2 and weights.size(1) == E and B in (None, weights.size(0)):
        B, stride = weights.size(0), E
    else:
        raise ValueError(f"weights must be (B, {E}) fp32 in original edge order, or ({E},) with B given, got "
                         f"{tuple(weights.shape)}")
    if B < 1 or dests.dim() != 1:
        raise ValueError("B must be >= 1 and dests 1-D")
    D = dests.numel()
    L = _lib.load()
    need = int(L.tarl_dest_trees_batched_scratch_bytes(plan.handle, B, D))
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=weights.device)
    _contig(scratch, torch.uint8, "scratch")
    if out is None:
        out = torch.empty((B, D, N), dtype=torch.int32, device=weights.device)
    _contig(out, torch.int32, "out")
    if tuple(out.shape) != (B, D, N):
        raise ValueError(f"out must be (B, D, N) = ({B}, {D}, {N}), got {tuple(out.shape)}")
    _lib.check(L.tarl_dest_trees_batched(plan.handle, weights.data_ptr(), B, stride, dests.data_ptr(), D,
                                         scratch.data_ptr(), scratch.numel(), out.data_ptr(), _lib.current_stream()))
    return out


def fused_select_next_hop_dest(plan: Plan, fs, dest_slot, next_hop, choice8=None, hold=False):
    """:func:`select_next_hop_dest` on the packed state (tarl_fused_select_next_hop_dest): the SELECTED_ROAD bytes of ``fs``
    <- the next hop towards the destination of every row's head agent. ``next_hop`` int32 (D, N) shared by the
    environments, or (B, D, N) with environment b's table; ``dest_slot`` (N,) int32. ``choice8`` (B, N) uint8 (optional):
    the rows' bytes after the call, env-major. ``hold`` (tarl_fused_select_next_hop_hold, not the reference's rule): a row
    whose next hop is its head agent's destination selects ITSELF instead, so that the environment's step order withdraws
    the agent there instead of stranding it on its destination road."""
    L = _lib.load()
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    _contig(dest_slot, torch.int32, "dest_slot")
    _contig(next_hop, torch.int32, "next_hop")
    if dest_slot.dim() != 1 or dest_slot.numel() != N or next_hop.dim() not in (2, 3) or next_hop.size(-1) != N or \
            (next_hop.dim() == 3 and next_hop.size(0) != fs.B):
        raise ValueError(f"dest_slot must be ({N},) and next_hop (D, {N}) or ({fs.B}, D, {N}), got "
                         f"{tuple(dest_slot.shape)} and {tuple(next_hop.shape)}")
    D = next_hop.size(-2)
    if choice8 is not None:
        _contig(choice8, torch.uint8, "choice8")
        if tuple(choice8.shape) != (fs.B, N):
            raise ValueError(f"choice8 must be (B, N) = ({fs.B}, {N})")
    entry = L.tarl_fused_select_next_hop_hold if hold else L.tarl_fused_select_next_hop_dest
    _lib.check(entry(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, dest_slot.data_ptr(), next_hop.data_ptr(),
                     D * N if next_hop.dim() == 3 else 0, D, _lib.ptr(choice8), _lib.current_stream()))
    return choice8


def reset_state(x, Nmax, agent_features=None):
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = (0, 0) if agent_features is None else _agents(agent_features, B)
    _lib.check(L.tarl_reset_state(x.data_ptr(), B, bs, ldx, Nmax, N, _lib.ptr(agent_features), A, abs_,
                                  _lib.current_stream()))


# ---- GraphDistribution ------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor, E: int, name: str):
    if t.size(-1) != E:
        raise ValueError(f"{name} last dim must be E={E}")
    return t.numel() // E


def graphdist_softmax(plan: Plan, logits, temperature=1.0):
    L = _lib.load()
    _contig(logits, torch.float32, "logits")
    B = _rows(logits, plan.num_edges, "logits")
    proba = torch.empty_like(logits)
    _lib.check(L.tarl_graphdist_softmax(plan.handle, logits.data_ptr(), B, float(temperature), proba.data_ptr(),
                                        _lib.current_stream()))
    return proba


def graphdist_sample(plan: Plan, proba, *, uniform=None, seed=0, counter=0, want_onehot=True, want_choice=False):
    L = _lib.load()
    _contig(proba, torch.float32, "proba")
    E, G, N = plan.num_edges, plan.num_groups, plan.num_nodes
    B = _rows(proba, E, "proba")
    if uniform is not None:
        _contig(uniform, torch.float32, "uniform")
        if uniform.numel() != B * G:
            raise ValueError("uniform must hold B*num_groups values")
    sums = torch.empty((B, G + 1), dtype=torch.float64, device=proba.device)
    onehot = torch.empty(proba.shape, dtype=torch.int64, device=proba.device) if want_onehot else None
    choice = torch.empty(proba.shape[:-1] + (N,), dtype=torch.int32, device=proba.device) if want_choice else None
    _lib.check(L.tarl_graphdist_sample(plan.handle, proba.data_ptr(), B, _lib.ptr(uniform), int(seed), int(counter),
                                       sums.data_ptr(), _lib.ptr(onehot), _lib.ptr(choice), _lib.current_stream()))
    return onehot, choice


def graphdist_rollout(plan: Plan, logits, temperature=1.0, *, uniform=None, seed=0, counter=0, choice=None, choice8=None,
                      sel8=None, log_prob=None, scratch=None):
    """sample() + log_prob() of GraphDistribution(logits / temperature) in one launch (bit-identical to softmax -> sample
    -> logprob). logits (B, E); outputs written in place where given: choice int32 (B, N), choice8 uint8 (B, N) rank
    bytes, sel8 uint8 (N, B) = the packed state's SELECTED_ROAD bytes; returns log_prob (B,)."""
    L = _lib.load()
    _contig(logits, torch.float32, "logits")
    E, G, N = plan.num_edges, plan.num_groups, plan.num_nodes
    B = _rows(logits, E, "logits")
    if uniform is not None:
        _contig(uniform, torch.float32, "uniform")
        if uniform.numel() != B * G:
            raise ValueError("uniform must hold B*num_groups values")
    for name, t, dt, n in (("choice", choice, torch.int32, B * N), ("choice8", choice8, torch.uint8, B * N),
                           ("sel8", sel8, torch.uint8, B * N)):
        if t is not None:
            _contig(t, dt, name)
            if t.numel() != n:
                raise ValueError(f"{name} must hold B * num_nodes values")
    need = int(L.tarl_graphdist_rollout_scratch_bytes(plan.handle, B))
    if scratch is None or scratch.numel() * scratch.element_size() < need:
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=logits.device)
    if log_prob is None:
        log_prob = torch.empty(B, dtype=torch.float32, device=logits.device)
    else:
        _contig(log_prob, torch.float32, "log_prob")
    _lib.check(L.tarl_graphdist_rollout(plan.handle, logits.data_ptr(), B, float(temperature), _lib.ptr(uniform), int(seed),
                                        int(counter), scratch.data_ptr(), _lib.ptr(choice), _lib.ptr(choice8),
                                        _lib.ptr(sel8), log_prob.data_ptr(), _lib.current_stream()))
    return log_prob


def graphdist_mode_rollout(plan: Plan, logits, temperature=1.0, *, choice=None, choice8=None, sel8=None, log_prob=None):
    """mode() + log_prob() of GraphDistribution(logits / temperature) in one launch (bit-identical to softmax -> mode ->
    logprob): the deterministic action of an evaluation. logits (B, E); outputs written in place where given, as
    :func:`graphdist_rollout`: choice int32 (B, N), choice8 uint8 (B, N) rank bytes, sel8 uint8 (N, B) = the packed state's
    SELECTED_ROAD bytes; returns log_prob (B,)."""
    L = _lib.load()
    _contig(logits, torch.float32, "logits")
    E, N = plan.num_edges, plan.num_nodes
    B = _rows(logits, E, "logits")
    for name, t, dt, n in (("choice", choice, torch.int32, B * N), ("choice8", choice8, torch.uint8, B * N),
                           ("sel8", sel8, torch.uint8, B * N)):
        if t is not None:
            _contig(t, dt, name)
            if t.numel() != n:
                raise ValueError(f"{name} must hold B * num_nodes values")
    if log_prob is None:
        log_prob = torch.empty(B, dtype=torch.float32, device=logits.device)
    else:
        _contig(log_prob, torch.float32, "log_prob")
        if log_prob.numel() != B:
            raise ValueError("log_prob must hold B values")
    _lib.check(L.tarl_graphdist_mode_rollout(plan.handle, logits.data_ptr(), B, float(temperature), _lib.ptr(choice),
                                             _lib.ptr(choice8), _lib.ptr(sel8), log_prob.data_ptr(),
                                             _lib.current_stream()))
    return log_prob


def episode_summary(agent_features, *, reward=None, frames=None, bin_width=10.0, num_bins=720, out=None):
    """Per-environment summary of an episode from the agent tables ``agent_features`` (B, A, 9) (row 0, the dummy, is
    skipped) and the per-frame rewards ``reward`` (T, B) (its first ``frames`` rows; None: no return). Returns the dict
    ``counts`` int32 (B, 3) {arrived, on the way, not departed}, ``sums`` fp64 (B, 3) {sum tt, sum tt^2, max tt} over the
    arrived agents, ``episode_return`` fp64 (B,), ``hist`` int32 (B, num_bins) travel-time histogram (bin ``min(floor(tt /
    bin_width), num_bins - 1)``); ``out``: such a dict to write into (allocated once by the caller)."""
    L = _lib.load()
    if agent_features.dim() != 3:
        raise ValueError("agent_features must be (B, A, 9)")
    B = agent_features.size(0)
    A, abs_ = _agents(agent_features, B)
    T = 0
    if reward is not None:
        _contig(reward, torch.float32, "reward")
        if reward.dim() != 2 or reward.size(1) != B:
            raise ValueError("reward must be (T, B)")
        T = reward.size(0) if frames is None else int(frames)
        if not 0 <= T <= reward.size(0):
            raise ValueError("frames must be in [0, reward.size(0)]")
    if int(num_bins) < 1 or not float(bin_width) > 0.0:
        raise ValueError("num_bins must be >= 1 and bin_width positive")
    dev = agent_features.device
    if out is None:
        out = {"counts": torch.empty((B, 3), dtype=torch.int32, device=dev),
               "sums": torch.empty((B, 3), dtype=torch.float64, device=dev),
               "episode_return": torch.empty(B, dtype=torch.float64, device=dev),
               "hist": torch.empty((B, int(num_bins)), dtype=torch.int32, device=dev)}
    for name, dt, shp in (("counts", torch.int32, (B, 3)), ("sums", torch.float64, (B, 3)),
                          ("episode_return", torch.float64, (B,)), ("hist", torch.int32, (B, int(num_bins)))):
        _contig(out[name], dt, name)
        if tuple(out[name].shape) != shp:
            raise ValueError(f"{name} must be {shp}")
    _lib.check(L.tarl_episode_summary(agent_features.data_ptr(), B, A, abs_, _lib.ptr(reward) if T else None, T,
                                      float(bin_width), int(num_bins), out["counts"].data_ptr(), out["sums"].data_ptr(),
                                      out["episode_return"].data_ptr(), out["hist"].data_ptr(), _lib.current_stream()))
    return out


LINK_COUNTS_MAX_FRAMES = 127      # = TARL_LINK_COUNTS_MAX_FRAMES of include/tarl_hip.h


def _meta(t, dtype, shape, name):
    """dtype, shape and layout of ``t`` (checked before its device, so that a wrong call is named for what is wrong)."""
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _bin_schedule(frames, Fcap, Fmax, t0, timestep, bin_seconds, first_bin, H, fmax_name=""):
    """The frame count, clock and bin arguments of an accumulate call, checked -> ``(F, t0, timestep, bin_seconds, first_bin)``:
    ``frames`` defaults to the ring's ``Fcap`` and is at most the kernel's ``Fmax``, ``first_bin`` to the bin of ``t0``."""
    F = Fcap if frames is None else int(frames)
    if not 1 <= F <= Fcap:
        raise ValueError(f"frames must be in [1, {Fcap}], got {F}")
    if F > Fmax:
        raise ValueError(f"one call takes at most {Fmax} frames{fmax_name}, got {F}")
    t0, timestep, bin_seconds = int(t0), int(timestep), int(bin_seconds)
    if t0 < 0 or timestep < 0 or bin_seconds < 1:
        raise ValueError("t0 and timestep must be >= 0 and bin_seconds >= 1")
    first_bin = t0 // bin_seconds if first_bin is None else int(first_bin)
    lo, hi = t0 // bin_seconds - first_bin, (t0 + (F - 1) * timestep) // bin_seconds - first_bin
    if first_bin < 0 or lo < 0 or hi >= H:
        raise ValueError(f"bin out of range: the frames fall in bins {lo} .. {hi} of the {H} stored (first_bin {first_bin})")
    return F, t0, timestep, bin_seconds, first_bin


def link_counts_accumulate(popped, withdrawn, counts, *, t0, timestep=1, bin_seconds=3600, first_bin=None, frames=None):
    """``counts`` int32 (B, H, N) += the per-bin sums of ``popped`` + ``withdrawn`` uint8 (F, B, N), the per-frame masks of
    ``SimEngine.frame_fused`` for ``frames`` (default: all F) consecutive frames whose first started at clock ``t0``
    (integers: frame f at ``t0 + f * timestep``, bin ``clock // bin_seconds - first_bin``; ``first_bin`` defaults to the
    bin of ``t0``). One launch; at most :data:`LINK_COUNTS_MAX_FRAMES` frames; a frame outside the H stored bins is refused
    before anything is launched. Returns ``counts``."""
    if popped.dim() != 3:
        raise ValueError(f"popped must be (F, B, N), got {tuple(popped.shape)}")
    _meta(popped, torch.uint8, popped.shape, "popped")
    _meta(withdrawn, torch.uint8, popped.shape, "withdrawn")
    Fcap, B, N = popped.shape
    if counts.dim() != 3:
        raise ValueError(f"counts must be (B, H, N), got {tuple(counts.shape)}")
    H = counts.size(1)
    _meta(counts, torch.int32, (B, H, N), "counts")
    F, t0, timestep, bin_seconds, first_bin = _bin_schedule(frames, Fcap, LINK_COUNTS_MAX_FRAMES, t0, timestep, bin_seconds,
                                                            first_bin, H, " (TARL_LINK_COUNTS_MAX_FRAMES)")
    for t, dt, name in ((popped, torch.uint8, "popped"), (withdrawn, torch.uint8, "withdrawn"), (counts, torch.int32, "counts")):
        _check_dev(t, dt, name)
    _lib.check(_lib.load().tarl_link_counts_accumulate(popped.data_ptr(), withdrawn.data_ptr(), F, B, N, t0, timestep,
                                                       bin_seconds, first_bin, H, counts.data_ptr(), _lib.current_stream()))
    return counts


def link_count_stats(counts_a, counts_b=None, *, out=None):
    """Integer moments over the K environments of ``counts_a`` int32 (K, H, N) — or, with ``counts_b`` of the same shape, of
    the per-environment difference a - b — per (row, road), the rows being the H bins and the episode total (row H): the
    dict ``sum`` and ``sumsq`` int64 (H + 1, N), ``min`` and ``max`` int32 (H + 1, N); ``out``: such a dict to write into."""
    if counts_a.dim() != 3:
        raise ValueError(f"counts_a must be (K, H, N), got {tuple(counts_a.shape)}")
    K, H, N = counts_a.shape
    if K < 1 or H < 1 or N < 1:
        raise ValueError("counts_a must not be empty")
    _meta(counts_a, torch.int32, (K, H, N), "counts_a")
    if counts_b is not None:
        _meta(counts_b, torch.int32, (K, H, N), "counts_b")
    spec = (("sum", torch.int64), ("sumsq", torch.int64), ("min", torch.int32), ("max", torch.int32))
    if out is not None:
        for name, dt in spec:
            _meta(out[name], dt, (H + 1, N), name)
    _check_dev(counts_a, torch.int32, "counts_a")
    if counts_b is not None:
        _check_dev(counts_b, torch.int32, "counts_b")
    if out is None:
        out = {name: torch.empty((H + 1, N), dtype=dt, device=counts_a.device) for name, dt in spec}
    for name, dt in spec:
        _check_dev(out[name], dt, name)
    _lib.check(_lib.load().tarl_link_count_stats(counts_a.data_ptr(), _lib.ptr(counts_b), K, H, N, out["sum"].data_ptr(),
                                                 out["sumsq"].data_ptr(), out["min"].data_ptr(), out["max"].data_ptr(),
                                                 _lib.current_stream()))
    return out


OCCUPANCY_MAX_FRAMES = 1 << 23      # 255 * 2^23 < 2^31: the int32 partial sums of one tarl_occupancy_accumulate call


def occupancy_accumulate(ring, thr, veh, full, peak, *, t0, timestep=1, bin_seconds=3600, first_bin=None, frames=None):
    """``ring`` fp32 (F, N, K): the ``counts`` slices of ``SimEngine.frame_fused`` (env-minor, the count after the frame) of
    ``frames`` (default: all F) consecutive frames whose first started at clock ``t0``; ``thr`` int32 (N,): the count from
    which a road is at capacity. ``veh`` int32 (K, H, N) += the per-bin sums of the counts, ``full`` int32 (K, H, N) += the
    per-bin number of frames with count >= thr, ``peak`` int32 (K, 1, N) = max(peak, the largest count): a second call
    continues the first. Bins as :func:`link_counts_accumulate` (frame f at ``t0 + f * timestep``, bin
    ``clock // bin_seconds - first_bin``; ``first_bin`` defaults to the bin of ``t0``). A value is converted by truncation,
    NaN and negatives count 0, anything above 255 counts 255. One launch; at most :data:`OCCUPANCY_MAX_FRAMES` frames; a
    frame outside the H stored bins is refused before anything is launched. Returns ``(veh, full, peak)``."""
    if ring.dim() != 3:
        raise ValueError(f"ring must be (F, N, K), got {tuple(ring.shape)}")
    _meta(ring, torch.float32, ring.shape, "ring")
    Fcap, N, K = ring.shape
    _meta(thr, torch.int32, (N,), "thr")
    if veh.dim() != 3:
        raise ValueError(f"veh must be (K, H, N), got {tuple(veh.shape)}")
    H = veh.size(1)
    _meta(veh, torch.int32, (K, H, N), "veh")
    _meta(full, torch.int32, (K, H, N), "full")
    _meta(peak, torch.int32, (K, 1, N), "peak")
    if K < 1 or N < 1 or H < 1:
        raise ValueError("ring and the accumulators must not be empty")
    F, t0, timestep, bin_seconds, first_bin = _bin_schedule(frames, Fcap, OCCUPANCY_MAX_FRAMES, t0, timestep, bin_seconds,
                                                            first_bin, H)
    for t, dt, name in ((ring, torch.float32, "ring"), (thr, torch.int32, "thr"), (veh, torch.int32, "veh"),
                        (full, torch.int32, "full"), (peak, torch.int32, "peak")):
        _check_dev(t, dt, name)
    _lib.check(_lib.load().tarl_occupancy_accumulate(ring.data_ptr(), thr.data_ptr(), F, K, N, t0, timestep, bin_seconds,
                                                     first_bin, H, veh.data_ptr(), full.data_ptr(), peak.data_ptr(),
                                                     _lib.current_stream()))
    return veh, full, peak


TURN_COUNTS_MAX_FRAMES = 1 << 23      # the limit of one tarl_turn_counts_accumulate call


def turn_counts_accumulate(plan, popped, sel8, counts, turns, lost, unresolved, *, prev_counts=None, t0, timestep=1,
                           bin_seconds=3600, first_bin=None, frames=None):
    """The rings of ``frames`` (default: all F) consecutive frames of ``SimEngine.frame_fused`` whose first started at clock
    ``t0``: ``popped`` uint8 (F, K, N) (env-major), ``sel8`` uint8 (F, N, K) (the engine's ``fs.sel8`` after each frame) and
    ``counts`` fp32 (F, N, K) (env-minor, the count after the frame); ``prev_counts`` fp32 (N, K): the ``counts`` slice of
    the frame before the first (``None``: every road was empty, as after a reset). ``turns`` int32 (K, H, E) += the vehicles
    that crossed each route edge per bin, in the ORIGINAL edge order of ``plan``; ``lost`` int32 (K, H, N) += the frames in
    which a road was popped although it was empty (the agent the U-turn double pop loses); ``unresolved`` int32 (K,) += the
    pops of a non-empty road whose SELECTED_ROAD byte names no out-edge. Bins as :func:`link_counts_accumulate`. One launch;
    a frame outside the H stored bins is refused before anything is launched. Returns ``(turns, lost, unresolved)``."""
    if popped.dim() != 3:
        raise ValueError(f"popped must be (F, K, N), got {tuple(popped.shape)}")
    _meta(popped, torch.uint8, popped.shape, "popped")
    Fcap, K, N = popped.shape
    E = plan.num_edges
    if N != plan.num_nodes:
        raise ValueError(f"popped must be (F, K, {plan.num_nodes}) for this plan, got {tuple(popped.shape)}")
    _meta(sel8, torch.uint8, (Fcap, N, K), "sel8")
    _meta(counts, torch.float32, (Fcap, N, K), "counts")
    if prev_counts is not None:
        _meta(prev_counts, torch.float32, (N, K), "prev_counts")
    if turns.dim() != 3:
        raise ValueError(f"turns must be (K, H, E), got {tuple(turns.shape)}")
    H = turns.size(1)
    _meta(turns, torch.int32, (K, H, E), "turns")
    _meta(lost, torch.int32, (K, H, N), "lost")
    _meta(unresolved, torch.int32, (K,), "unresolved")
    if K < 1 or N < 1 or H < 1 or E < 1:
        raise ValueError("the rings and the tables must not be empty")
    F, t0, timestep, bin_seconds, first_bin = _bin_schedule(frames, Fcap, TURN_COUNTS_MAX_FRAMES, t0, timestep, bin_seconds,
                                                            first_bin, H)
    for t, dt, name in ((popped, torch.uint8, "popped"), (sel8, torch.uint8, "sel8"), (counts, torch.float32, "counts"),
                        (turns, torch.int32, "turns"), (lost, torch.int32, "lost"), (unresolved, torch.int32, "unresolved")):
        _check_dev(t, dt, name)
    if prev_counts is not None:
        _check_dev(prev_counts, torch.float32, "prev_counts")
    _lib.check(_lib.load().tarl_turn_counts_accumulate(plan.handle, popped.data_ptr(), sel8.data_ptr(), counts.data_ptr(),
                                                       _lib.ptr(prev_counts), F, K, t0, timestep, bin_seconds, first_bin, H,
                                                       turns.data_ptr(), lost.data_ptr(), unresolved.data_ptr(),
                                                       _lib.current_stream()))
    return turns, lost, unresolved


TRIP_MAX_BINS = 4096      # = TARL_TRIP_MAX_BINS of include/tarl_hip.h: the arrivals histogram of one environment lives in LDS
_TRIP_AGENT_SPEC = (("n_done", torch.int32), ("n_way", torch.int32), ("tt_sum", torch.float64), ("tt_sumsq", torch.float64),
                    ("tt_min", torch.float32), ("tt_max", torch.float32))
_TRIP_PAIR_SPEC = (("n_both", torch.int32), ("d_sum", torch.float64), ("d_sumsq", torch.float64), ("n_faster", torch.int32),
                   ("n_slower", torch.int32))
_TRIP_BIN_SPEC = (("dep_done", torch.int32), ("dep_way", torch.int32), ("arr", torch.int32), ("dep_tt", torch.float64))
_TRIP_FF_SPEC = (("dep_ff", torch.float64), ("dep_ff_n", torch.int32))


def _trip_tables(agents, name):
    """(K, A, 9) fp32 agent tables -> (K, A, a_bstride), meta first and device last as :func:`_meta` does."""
    if agents.dim() != 3:
        raise ValueError(f"{name} must be (K, A, 9), got {tuple(agents.shape)}")
    if agents.dtype != torch.float32:
        raise TypeError(f"{name} must be {torch.float32}, got {agents.dtype}")
    K, A = agents.size(0), agents.size(1)
    if K < 1 or A < 1:
        raise ValueError(f"{name} must not be empty")
    if agents.size(2) != 9 or agents.stride(2) != 1 or agents.stride(1) != 9 or (K > 1 and agents.stride(0) < 9 * A):
        raise ValueError(f"{name} must be (K, A, 9) with contiguous rows and tables that do not overlap")
    return K, A, agents.stride(0) if K > 1 else 9 * A


def _trip_out(out, spec, shape, device):
    if out is None:
        out = {}
    for name, dt in spec:
        if name in out:
            _meta(out[name], dt, shape, name)
        else:
            out[name] = torch.empty(shape, dtype=dt, device=device)
    return out


def trip_agent_stats(agents, agents_b=None, *, free_flow=None, out=None):
    """Per agent over the K environments of the agent tables ``agents`` fp32 (K, A, 9) after an episode
    (tarl_trip_agent_stats; row 0, the dummy, is skipped and entry 0 of every output is zero). Returns the dict ``n_done``,
    ``n_way`` int32 (A,): the environments in which the agent arrived (DONE == 1) / was still on the way; ``tt_sum``,
    ``tt_sumsq`` fp64 (A,) of the travel time ARRIVAL_TIME - DEPARTURE_TIME (fp32, widened) over the environments in which it
    arrived; ``tt_min``, ``tt_max`` fp32 (A,), +inf / -inf for an agent that never arrived. ``agents_b``: the tables of a
    second run of the same shape (the baseline); the dict gains, over the environments in which the agent arrived in BOTH runs
    and with d = tt - tt_b in fp64, ``n_both`` int32, ``d_sum``, ``d_sumsq`` fp64, ``n_faster`` (d < 0) and ``n_slower``
    (d > 0) int32. ``free_flow`` fp64 (A,): a free-flow time per agent; the dict gains ``n_under`` int32, the environments in
    which the agent arrived with tt < free_flow. The fp64 sums follow a fixed order (csrc/trips.hip): bit-identical from run to run. ``out``: such a dict
    (or a part of it) to write into."""
    K, A, abs_ = _trip_tables(agents, "agents")
    bbs = 0
    if agents_b is not None:
        Kb, Ab, bbs = _trip_tables(agents_b, "agents_b")
        if (Kb, Ab) != (K, A):
            raise ValueError(f"agents_b must be {(K, A, 9)} like agents, got {tuple(agents_b.shape)}")
    if free_flow is not None:
        _meta(free_flow, torch.float64, (A,), "free_flow")
    under = (("n_under", torch.int32),) if free_flow is not None else ()
    spec = under + _TRIP_AGENT_SPEC + (_TRIP_PAIR_SPEC if agents_b is not None else ())
    dev = agents.device
    out = _trip_out(out, spec, (A,), dev)
    _check_dev(agents, torch.float32, "agents")
    if agents_b is not None:
        _check_dev(agents_b, torch.float32, "agents_b")
    if free_flow is not None:
        _check_dev(free_flow, torch.float64, "free_flow")
    for name, dt in spec:
        _check_dev(out[name], dt, name)
    pair = [out[n].data_ptr() for n, _ in _TRIP_PAIR_SPEC] if agents_b is not None else [None] * 5
    _lib.check(_lib.load().tarl_trip_agent_stats(agents.data_ptr(), _lib.ptr(agents_b), _lib.ptr(free_flow), K, A, abs_, bbs,
                                                 out["n_under"].data_ptr() if under else None,
                                                 *[out[n].data_ptr() for n, _ in _TRIP_AGENT_SPEC], *pair,
                                                 _lib.current_stream()))
    return out


def _trip_bins(bin_seconds, first_bin, num_bins):
    bin_seconds, first_bin, num_bins = int(bin_seconds), int(first_bin), int(num_bins)
    if bin_seconds < 1 or first_bin < 0:
        raise ValueError("bin_seconds must be >= 1 and first_bin >= 0")
    if not 1 <= num_bins <= TRIP_MAX_BINS:
        raise ValueError(f"num_bins must be in [1, {TRIP_MAX_BINS}] (ops.TRIP_MAX_BINS), got {num_bins}")
    return bin_seconds, first_bin, num_bins


def trip_clock_bin(clock, bin_seconds, first_bin, num_bins):
    """The stored bin of every clock value of ``clock`` (fp32 tensor) -> int64: ``clamp(floor(c) // bin_seconds - first_bin,
    0, num_bins - 1)``, a NaN or negative clock taken as 0 and one from 2^62 on as the last bin — the rule of
    tarl_trip_bin_stats, in torch."""
    c = torch.nan_to_num(clock.to(torch.float32), nan=0.0, posinf=float(2 ** 63), neginf=0.0).clamp(min=0.0)
    q = torch.div(torch.floor(c.clamp(max=float(2 ** 62))).to(torch.int64), int(bin_seconds), rounding_mode="trunc") - int(first_bin)
    q = torch.where(c >= float(2 ** 62), torch.full_like(q, int(num_bins) - 1), q)
    return q.clamp(0, int(num_bins) - 1)


def trip_departure_order(departure, *, bin_seconds, first_bin, num_bins):
    """The agents sorted by departure bin, once per population: ``departure`` fp32 (A,) (the DEPARTURE_TIME column of one
    agent table, row 0 the dummy) -> (perm int32 (max(A - 1, 1),): the agents 1 .. A - 1 bin by bin, ascending id within a
    bin; seg int32 (num_bins + 1,): where every bin's segment starts in perm, seg[num_bins] = A - 1). Torch plumbing on the
    tensor's device; what :func:`trip_bin_stats` takes as ``order``."""
    bin_seconds, first_bin, num_bins = _trip_bins(bin_seconds, first_bin, num_bins)
    if departure.dim() != 1 or departure.numel() < 1:
        raise ValueError(f"departure must be (A,), got {tuple(departure.shape)}")
    A, dev = departure.numel(), departure.device
    bins = trip_clock_bin(departure[1:], bin_seconds, first_bin, num_bins)
    srt, idx = torch.sort(bins, stable=True)
    perm = torch.zeros(max(A - 1, 1), dtype=torch.int32, device=dev)
    perm[:A - 1] = (idx + 1).to(torch.int32)
    seg = torch.searchsorted(srt, torch.arange(num_bins + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    return perm, seg


def trip_bin_stats(agents, *, bin_seconds, first_bin, num_bins, free_flow=None, order=None, out=None):
    """Per (environment, time bin) over the agents of the tables ``agents`` fp32 (K, A, 9) after an episode
    (tarl_trip_bin_stats; row 0 is skipped), bin h = absolute bin ``first_bin + h`` of ``bin_seconds`` seconds, clock values
    outside the ``num_bins`` stored bins clamped into the first / last one. Returns the dict, each (K, num_bins):
    ``dep_done``, ``dep_way`` int32: the agents whose DEPARTURE_TIME falls into the bin and that arrived / are on the way at the
    end; ``dep_tt`` fp64: the sum of the travel times of the former; ``arr`` int32: the agents that arrived, binned by
    ARRIVAL_TIME. ``free_flow`` fp64 (A,): a free-flow time per agent (+inf: none); the dict gains ``dep_ff`` fp64, the sum
    of the free-flow times of the arrived agents of the bin that have a finite one, and ``dep_ff_n`` int32, their number.
    The agents are binned by the DEPARTURE_TIME of environment 0, which the caller guarantees to be every environment's
    (``VecEvaluator`` checks it); ``order``: :func:`trip_departure_order` of that column and the same bins, built once per
    population (default: built here). At most :data:`TRIP_MAX_BINS` bins; a refused call leaves ``out`` untouched."""
    K, A, abs_ = _trip_tables(agents, "agents")
    bin_seconds, first_bin, H = _trip_bins(bin_seconds, first_bin, num_bins)
    if K * H >= 1 << 31:
        raise ValueError(f"K * num_bins must stay below 2^31, got {K} * {H}")
    dev = agents.device
    if free_flow is not None:
        _meta(free_flow, torch.float64, (A,), "free_flow")
    spec = _TRIP_BIN_SPEC + (_TRIP_FF_SPEC if free_flow is not None else ())
    if order is not None:
        _meta(order[0], torch.int32, (max(A - 1, 1),), "order[0] (perm)")
        _meta(order[1], torch.int32, (H + 1,), "order[1] (seg)")
    out = _trip_out(out, spec, (K, H), dev)
    _check_dev(agents, torch.float32, "agents")
    if free_flow is not None:
        _check_dev(free_flow, torch.float64, "free_flow")
    if order is None:
        order = trip_departure_order(agents[0, :, 2], bin_seconds=bin_seconds, first_bin=first_bin, num_bins=H)
    perm, seg = order
    for t, name in ((perm, "perm"), (seg, "seg")):
        _check_dev(t, torch.int32, name)
    for name, dt in spec:
        _check_dev(out[name], dt, name)
    ffo = [out[n].data_ptr() for n, _ in _TRIP_FF_SPEC] if free_flow is not None else [None, None]
    _lib.check(_lib.load().tarl_trip_bin_stats(agents.data_ptr(), K, A, abs_, perm.data_ptr(), seg.data_ptr(),
                                               _lib.ptr(free_flow), bin_seconds, first_bin, H,
                                               *[out[n].data_ptr() for n, _ in _TRIP_BIN_SPEC], *ffo, _lib.current_stream()))
    return out


# ---- dynamic relative gap (tarl_hip/evaluator.py, dynamic_gap=True) ----------------------------------------------------------
def td_road_times(veh, frames_per_bin, max_agents, free_flow, cong, *, bin_seconds, first_bin, out=None):
    """Time-dependent road times of an episode and their FIFO envelope (tarl_td_road_times). ``veh`` int32 (K, H, N): the
    occupancy sums of :func:`occupancy_accumulate`; ``frames_per_bin`` int32 (H,): the frames that fell into each bin;
    ``max_agents``, ``free_flow``, ``cong`` fp32 (N,): MAX_NUMBER_OF_AGENT, FREE_FLOW_TIME_TRAVEL and the congestion constant
    of every road. Returns ``(tau, env)``: ``tau`` fp32 (K, H, N) = (float) max(FF, cong / ((MAX + 10) - veh / frames)) in
    fp64 — FF for a bin without frames, +inf for a denominator <= 0 — and ``env`` fp64 (K, H + 1, N) with ``env[:, H] = +inf``
    and ``env[:, h] = min((first_bin + h) * bin_seconds + tau[:, h], env[:, h + 1])``. ``out``: such a pair to write into; a
    refused call leaves it untouched."""
    if veh.dim() != 3:
        raise ValueError(f"veh must be (K, H, N), got {tuple(veh.shape)}")
    K, H, N = veh.shape
    if K < 1 or H < 1 or N < 1:
        raise ValueError("veh must not be empty")
    _meta(veh, torch.int32, (K, H, N), "veh")
    _meta(frames_per_bin, torch.int32, (H,), "frames_per_bin")
    for t, name in ((max_agents, "max_agents"), (free_flow, "free_flow"), (cong, "cong")):
        _meta(t, torch.float32, (N,), name)
    bin_seconds, first_bin, H = _trip_bins(bin_seconds, first_bin, H)
    if K >= 65536:
        raise ValueError(f"one call takes fewer than 65536 environments, got {K}")
    if out is not None:
        _meta(out[0], torch.float32, (K, H, N), "out[0] (tau)")
        _meta(out[1], torch.float64, (K, H + 1, N), "out[1] (env)")
    for t, dt, name in ((veh, torch.int32, "veh"), (frames_per_bin, torch.int32, "frames_per_bin"),
                        (max_agents, torch.float32, "max_agents"), (free_flow, torch.float32, "free_flow"),
                        (cong, torch.float32, "cong")):
        _check_dev(t, dt, name)
    if out is None:
        out = (torch.empty((K, H, N), dtype=torch.float32, device=veh.device),
               torch.empty((K, H + 1, N), dtype=torch.float64, device=veh.device))
    tau, env = out
    _check_dev(tau, torch.float32, "out[0] (tau)")
    _check_dev(env, torch.float64, "out[1] (env)")
    _lib.check(_lib.load().tarl_td_road_times(veh.data_ptr(), frames_per_bin.data_ptr(), max_agents.data_ptr(),
                                              free_flow.data_ptr(), cong.data_ptr(), K, H, N, bin_seconds, first_bin,
                                              tau.data_ptr(), env.data_ptr(), _lib.current_stream()))
    return tau, env


def td_hindsight_bytes(plan: Plan, K: int, num_agents: int) -> int:
    """Scratch bytes of :func:`td_hindsight` for K x num_agents searches (one fp64 label row of N per resident workgroup);
    -1 for a bad argument."""
    return int(_lib.load().tarl_td_hindsight_scratch_bytes(plan.handle, int(K), int(num_agents)))


def td_hindsight(plan: Plan, tau, env, agents, *, bin_seconds, first_bin, out=None, scratch=None):
    """The hindsight arrival of every (environment, agent) under the road times of :func:`td_road_times`
    (tarl_td_hindsight): ``tau`` fp32 (K, H, N), ``env`` fp64 (K, H + 1, N), ``agents`` fp32 (K, A, 9) after the episode ->
    ``best`` fp64 (K, A), every entry written: the earliest clock at which the agent could have left its destination road
    (both end roads traversed, waiting for a later bin allowed), +inf for an unreachable destination, an id out of range,
    row 0 and an agent with DONE != 1. ``out`` fp64 (K, A) and ``scratch`` uint8 (:func:`td_hindsight_bytes`): caller-owned
    buffers; a refused call leaves ``out`` untouched. The graph-size limit is :func:`destination_trees`'s."""
    K, A, abs_ = _trip_tables(agents, "agents")
    N = plan.num_nodes
    if tau.dim() != 3:
        raise ValueError(f"tau must be (K, H, N), got {tuple(tau.shape)}")
    H = tau.size(1)
    _meta(tau, torch.float32, (K, H, N), "tau")
    _meta(env, torch.float64, (K, H + 1, N), "env")
    bin_seconds, first_bin, H = _trip_bins(bin_seconds, first_bin, H)
    if out is not None:
        _meta(out, torch.float64, (K, A), "out")
    if scratch is not None:
        if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous():
            raise TypeError("scratch must be a contiguous 1-D uint8 tensor")
    for t, dt, name in ((agents, torch.float32, "agents"), (tau, torch.float32, "tau"), (env, torch.float64, "env")):
        _check_dev(t, dt, name)
    need = td_hindsight_bytes(plan, K, A)
    if need < 0:
        raise _lib.TarlError("tarl_td_hindsight_scratch_bytes refused the sizes")
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=agents.device)
    _check_dev(scratch, torch.uint8, "scratch")
    if out is None:
        out = torch.empty((K, A), dtype=torch.float64, device=agents.device)
    _check_dev(out, torch.float64, "out")
    _lib.check(_lib.load().tarl_td_hindsight(plan.handle, tau.data_ptr(), env.data_ptr(), agents.data_ptr(), K, A, abs_,
                                             bin_seconds, first_bin, H, scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                             _lib.current_stream()))
    return out


# ---- day-to-day replanning (tarl_hip/replanning.py; NOT reference semantics) ----------------------------------
TD_ROUTES_MAX_HOPS = 1 << 20


def td_routes_bytes(plan: Plan, K: int, num_agents: int, max_hops: int) -> int:
    """Scratch bytes of :func:`td_routes` for K x num_agents searches (per resident workgroup one fp64 label row of N and
    the walk's stack of ``max_hops`` road ids); -1 for a bad argument (``max_hops`` outside [1, 2^20] among them)."""
    return int(_lib.load().tarl_td_routes_scratch_bytes(plan.handle, int(K), int(num_agents), int(max_hops)))


def td_routes(plan: Plan, tau, env, agents, *, bin_seconds, first_bin, max_hops, out=None, scratch=None):
    """The quickest time-dependent route of every (environment, agent) under the road times of :func:`td_road_times`
    (tarl_td_routes): :func:`td_hindsight`'s search for every agent a >= 1 with origin and destination in range, whatever its
    DONE flag, from its DEPARTURE_TIME -> ``(best, routes, route_len)``: ``best`` fp64 (K, A), ``routes`` int32
    (K, A, max_hops) stored forward (origin first, destination at ``route_len - 1``) and ``route_len`` int32 (K, A). Ties go
    to the in-neighbour with the smallest road id. ``route_len`` 0 with ``best`` +inf: unreachable, row 0, an id out of range;
    ``-(true length)``: longer than ``max_hops`` (the row is then left as it was). ``best`` and ``route_len`` are written
    everywhere, ``routes`` only up to the length. ``out``: such a triple to write into; ``scratch`` uint8
    (:func:`td_routes_bytes`); a refused call leaves ``out`` untouched."""
    K, A, abs_ = _trip_tables(agents, "agents")
    N = plan.num_nodes
    if tau.dim() != 3:
        raise ValueError(f"tau must be (K, H, N), got {tuple(tau.shape)}")
    H = tau.size(1)
    _meta(tau, torch.float32, (K, H, N), "tau")
    _meta(env, torch.float64, (K, H + 1, N), "env")
    bin_seconds, first_bin, H = _trip_bins(bin_seconds, first_bin, H)
    max_hops = int(max_hops)
    if not 1 <= max_hops <= TD_ROUTES_MAX_HOPS:
        raise ValueError(f"max_hops must be in [1, {TD_ROUTES_MAX_HOPS}], got {max_hops}")
    if out is not None:
        _meta(out[0], torch.float64, (K, A), "out[0] (best)")
        _meta(out[1], torch.int32, (K, A, max_hops), "out[1] (routes)")
        _meta(out[2], torch.int32, (K, A), "out[2] (route_len)")
    if scratch is not None:
        if scratch.dtype != torch.uint8 or scratch.dim() != 1 or not scratch.is_contiguous():
            raise TypeError("scratch must be a contiguous 1-D uint8 tensor")
    for t, dt, name in ((agents, torch.float32, "agents"), (tau, torch.float32, "tau"), (env, torch.float64, "env")):
        _check_dev(t, dt, name)
    need = td_routes_bytes(plan, K, A, max_hops)
    if need < 0:
        raise _lib.TarlError("tarl_td_routes_scratch_bytes refused the sizes")
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=agents.device)
    _check_dev(scratch, torch.uint8, "scratch")
    if out is None:
        out = (torch.empty((K, A), dtype=torch.float64, device=agents.device),
               torch.empty((K, A, max_hops), dtype=torch.int32, device=agents.device),
               torch.empty((K, A), dtype=torch.int32, device=agents.device))
    best, routes, route_len = out
    _check_dev(best, torch.float64, "out[0] (best)")
    _check_dev(routes, torch.int32, "out[1] (routes)")
    _check_dev(route_len, torch.int32, "out[2] (route_len)")
    _lib.check(_lib.load().tarl_td_routes(plan.handle, tau.data_ptr(), env.data_ptr(), agents.data_ptr(), K, A, abs_,
                                          bin_seconds, first_bin, H, max_hops, scratch.data_ptr(), scratch.numel(),
                                          best.data_ptr(), routes.data_ptr(), route_len.data_ptr(), _lib.current_stream()))
    return best, routes, route_len


def fused_select_route(plan: Plan, fs, routes, route_len, choice8=None):
    """The SELECTED_ROAD bytes of ``fs`` <- the road that follows every row on its head agent's route
    (tarl_fused_select_route; the hold rule of :func:`fused_select_next_hop_dest` one road short of the destination).
    ``routes`` int32 (A, L) with ``route_len`` (A,): one plan shared by the environments, or (B, A, L) with (B, A):
    environment b's. A row whose head has no route (length <= 0) or stands off its route is left untouched. ``choice8``
    (B, N) uint8 (optional): the rows' bytes after the call, env-major."""
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    _check_dev(routes, torch.int32, "routes")
    _check_dev(route_len, torch.int32, "route_len")
    _contig(routes, torch.int32, "routes")
    _contig(route_len, torch.int32, "route_len")
    if routes.dim() not in (2, 3) or tuple(route_len.shape) != tuple(routes.shape[:-1]) or routes.size(-2) != fs.A or \
            routes.size(-1) < 1 or (routes.dim() == 3 and routes.size(0) != fs.B):
        raise ValueError(f"routes must be ({fs.A}, L) or ({fs.B}, {fs.A}, L) int32 and route_len the same without L, got "
                         f"{tuple(routes.shape)} and {tuple(route_len.shape)}")
    L = routes.size(-1)
    if choice8 is not None:
        _contig(choice8, torch.uint8, "choice8")
        if tuple(choice8.shape) != (fs.B, N):
            raise ValueError(f"choice8 must be (B, N) = ({fs.B}, {N})")
    _lib.check(_lib.load().tarl_fused_select_route(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, routes.data_ptr(),
                                                   route_len.data_ptr(), fs.A * L if routes.dim() == 3 else 0, L,
                                                   _lib.ptr(choice8), _lib.current_stream()))
    return choice8


# ---- the per-agent path trace (csrc/path_trace.hip; NOT reference semantics) ----------------------------------
PATH_MAX_HOPS = 4096      # = TARL_PATH_MAX_HOPS of include/tarl_hip.h
PATH_MAX_AGENTS = 1 << 24
_PATH_STATE_SPEC = (("last_road", torch.int32), ("roads", torch.int32), ("revisits", torch.int32), ("off_tree", torch.int32),
                    ("path_cost", torch.float64), ("excess", torch.float64))
_PATH_I32 = ("n_done", "n_zero_excess", "n_loop", "n_trunc", "n_seen", "n_loop_all", "roads_max", "n_both")
_PATH_F64 = ("moves_sum", "moves_sumsq", "cost_sum", "cost_sumsq", "excess_sum", "excess_sumsq", "dmoves_sum", "dmoves_sumsq",
             "dexcess_sum", "dexcess_sumsq")


class PathTraceState:
    """The state of the per-agent path trace for B environments of A agents (row 0 the dummy) and at most L kept roads:
    ``last_road``, ``roads``, ``revisits``, ``off_tree`` int32 (B, A), ``path_cost``, ``excess`` fp64 (B, A), ``route`` int32
    (B, A, L) and ``bad`` int32 (B,). Allocated uninitialised: :func:`path_trace_reset` sets the initial values."""

    def __init__(self, B, A, L, device):
        B, A, L = int(B), int(A), int(L)
        if B < 1 or not 1 <= A <= PATH_MAX_AGENTS:
            raise ValueError(f"B must be >= 1 and A in [1, {PATH_MAX_AGENTS}], got B = {B}, A = {A}")
        if not 0 <= L <= PATH_MAX_HOPS:
            raise ValueError(f"L must be in [0, {PATH_MAX_HOPS}] (ops.PATH_MAX_HOPS), got {L}")
        self.B, self.A, self.L = B, A, L
        for name, dt in _PATH_STATE_SPEC:
            setattr(self, name, torch.empty((B, A), dtype=dt, device=device))
        self.route = torch.empty((B, A, L), dtype=torch.int32, device=device)
        self.bad = torch.empty(B, dtype=torch.int32, device=device)

    def tensors(self):
        """name -> tensor, in the order of the C ABI."""
        return {**{n: getattr(self, n) for n, _ in _PATH_STATE_SPEC}, "route": self.route, "bad": self.bad}

    def clone(self):
        """A copy of the state as it stands (the other run of a paired report, where this one is reset and run again)."""
        c = object.__new__(PathTraceState)
        c.B, c.A, c.L = self.B, self.A, self.L
        for name, t in self.tensors().items():
            setattr(c, name, t.clone())
        return c

    @property
    def route_len(self):
        """(B, A) int32: the kept roads of every trace, min(roads, L) — with ``route`` the pair the ``"routes"`` head takes."""
        return self.roads.clamp(max=self.L)

    def _ptrs(self):
        B, A, L = self.B, self.A, self.L
        for name, dt in _PATH_STATE_SPEC:
            t = getattr(self, name)
            _meta(t, dt, (B, A), f"state.{name}")
            _check_dev(t, dt, f"state.{name}")
        _meta(self.route, torch.int32, (B, A, L), "state.route")
        _check_dev(self.route, torch.int32, "state.route")
        _meta(self.bad, torch.int32, (B,), "state.bad")
        _check_dev(self.bad, torch.int32, "state.bad")
        return [getattr(self, n).data_ptr() for n, _ in _PATH_STATE_SPEC] + [self.route.data_ptr() if L else None,
                                                                             self.bad.data_ptr()]


def path_trace_state(B, A, L, device):
    """-> :class:`PathTraceState` for B environments, A agents (row 0 the dummy) and L kept roads per trace (0: none)."""
    return PathTraceState(B, A, L, device)


def path_trace_reset(state: PathTraceState):
    """The initial values of the trace (tarl_path_trace_reset): ``last_road`` and ``route`` -1, everything else 0."""
    _lib.check(_lib.load().tarl_path_trace_reset(state.B, state.A, state.L, *state._ptrs(), _lib.current_stream()))
    return state


def fused_path_trace(plan: Plan, fs, state: PathTraceState, weights=None, dist=None, dest_slot=None):
    """The sighting pass of the per-agent path trace on the packed state AFTER a frame (tarl_fused_path_trace):
    every agent that heads a non-empty road it was not seen on last gains that road — ``roads`` + 1, the road into ``route``
    while fewer than L are kept, ``revisits`` + 1 where the kept prefix already holds it — and, with ``weights`` fp32 (E,) in
    original edge order, ``dist`` fp64 (D, N) and ``dest_slot`` int32 (N,) of :func:`destination_trees` (all three or none),
    the hop's weight into ``path_cost`` and its reduced cost ``(w + dist[s][u]) - dist[s][p]`` towards the agent's own
    destination into ``excess`` (``off_tree`` + 1 where that is not finite). ``fs`` is read, never written. ``state.bad``
    counts what must not happen: a head id beyond the agent table, two sightings no edge connects."""
    N, E = plan.num_nodes, plan.num_edges
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    if (state.B, state.A) != (fs.B, fs.A):
        raise ValueError(f"state is for (B, A) = ({state.B}, {state.A}), the packed state for ({fs.B}, {fs.A})")
    given = [t is not None for t in (weights, dist, dest_slot)]
    if any(given) and not all(given):
        raise ValueError("weights, dist and dest_slot come together: all three or none")
    D = 0
    if weights is not None:
        _meta(weights, torch.float32, (E,), "weights")
        if dist.dim() != 2:
            raise ValueError(f"dist must be (D, {N}), got {tuple(dist.shape)}")
        D = dist.size(0)
        _meta(dist, torch.float64, (D, N), "dist")
        _meta(dest_slot, torch.int32, (N,), "dest_slot")
        for t, dt, name in ((weights, torch.float32, "weights"), (dist, torch.float64, "dist"),
                            (dest_slot, torch.int32, "dest_slot")):
            _check_dev(t, dt, name)
    _lib.check(_lib.load().tarl_fused_path_trace(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, state.L, *state._ptrs(),
                                                 _lib.ptr(weights), _lib.ptr(dist), _lib.ptr(dest_slot), D,
                                                 _lib.current_stream()))
    return state


def path_agent_stats(state: PathTraceState, agents, state_b=None, agents_b=None, out=None):
    """The trace reduced per agent over the K environments after an episode (tarl_path_agent_stats); ``agents`` fp32
    (K, A, 9), read for the DONE flag. Returns a dict of (A,) arrays, entry 0 (the dummy) zero. Over the environments in which
    the agent ARRIVED: ``n_done``, ``n_zero_excess`` (excess == 0 and no off-tree hop), ``n_loop`` (revisits > 0), ``n_trunc``
    (roads > L) int32 and the fp64 sums and sums of squares ``moves_sum``, ``moves_sumsq`` (moves = max(roads - 1, 0)),
    ``cost_sum``, ``cost_sumsq``, ``excess_sum``, ``excess_sumsq``; over all environments ``n_seen`` (roads > 0),
    ``n_loop_all`` and ``roads_max``. ``state_b`` with ``agents_b``: a second run on the same environments (the baseline); the
    dict gains, over the environments in which the agent arrived in BOTH, ``n_both`` and the sums ``dmoves_sum``,
    ``dmoves_sumsq``, ``dexcess_sum``, ``dexcess_sumsq`` of this run minus the other. Every sum adds the environments in
    ascending order: bit-identical from run to run. ``out`` = (int32 (8, A), fp64 (10, A)) to write into."""
    K, A, abs_ = _trip_tables(agents, "agents")
    if (state.B, state.A) != (K, A):
        raise ValueError(f"state is for (K, A) = ({state.B}, {state.A}), agents for ({K}, {A})")
    if (state_b is None) != (agents_b is None):
        raise ValueError("state_b and agents_b come together")
    pair = state_b is not None
    bbs = 0
    if pair:
        Kb, Ab, bbs = _trip_tables(agents_b, "agents_b")
        if (Kb, Ab) != (K, A) or (state_b.B, state_b.A) != (K, A):
            raise ValueError(f"state_b and agents_b must be for (K, A) = ({K}, {A}) like this run's")
        _check_dev(agents_b, torch.float32, "agents_b")
        state_b._ptrs()
    _check_dev(agents, torch.float32, "agents")
    ptrs = state._ptrs()
    if out is None:
        out = (torch.zeros((8, A), dtype=torch.int32, device=agents.device),
               torch.zeros((10, A), dtype=torch.float64, device=agents.device))
    oi, of = out
    _meta(oi, torch.int32, (8, A), "out[0]")
    _meta(of, torch.float64, (10, A), "out[1]")
    _check_dev(oi, torch.int32, "out[0]")
    _check_dev(of, torch.float64, "out[1]")
    _lib.check(_lib.load().tarl_path_agent_stats(ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], agents.data_ptr(), abs_,
                                                 state_b.roads.data_ptr() if pair else None,
                                                 state_b.excess.data_ptr() if pair else None, _lib.ptr(agents_b), bbs, K, A,
                                                 state.L, oi.data_ptr(), of.data_ptr(), _lib.current_stream()))
    ni, nf = (8, 10) if pair else (7, 6)
    return {**{n: oi[j] for j, n in enumerate(_PATH_I32[:ni])}, **{n: of[j] for j, n in enumerate(_PATH_F64[:nf])}}


def fused_hold_policy_actions(plan: Plan, fs, agent_features, choice8=None, held=None):
    """The hold rule of DESIGN 4.13a as a post-pass over the SELECTED_ROAD bytes a POLICY head has just written into ``fs``
    (tarl_fused_hold_policy_actions; an action shield, not the reference's rule): a row with a non-empty FIFO
    whose chosen out-edge leads to the DESTINATION of its head agent (``agent_features`` (B, A, 9), integers compared)
    selects ITSELF instead — the raw code with its own id — so that the environment's step order withdraws the agent there
    instead of stranding it on its destination road. Every other row keeps what the policy wrote; unlike the routers' rule
    an EMPTY row is never touched. ``choice8`` (B, N) uint8 (optional): the rows' bytes after the call, env-major.
    ``held`` (B,) int32 (optional): += the rows held by this call."""
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    A, abs_ = _agents(agent_features, fs.B)
    if choice8 is not None:
        _contig(choice8, torch.uint8, "choice8")
        if tuple(choice8.shape) != (fs.B, N):
            raise ValueError(f"choice8 must be (B, N) = ({fs.B}, {N})")
    if held is not None:
        _contig(held, torch.int32, "held")
        if tuple(held.shape) != (fs.B,):
            raise ValueError(f"held must be (B,) = ({fs.B},)")
    _lib.check(_lib.load().tarl_fused_hold_policy_actions(plan.handle, fs.ref, fs.B, fs.Nmax, agent_features.data_ptr(), A,
                                                          abs_, _lib.ptr(choice8), _lib.ptr(held), _lib.current_stream()))
    return choice8


def fused_set_policy_hold(fs, on, held=None):
    """The switch of the state-dependent T-frame rollouts (:func:`fused_rollout_policy`, :func:`fused_rollout_prior`,
    :func:`fused_rollout_gt`; tarl_fused_set_policy_hold): with ``on`` their loop queues :func:`fused_hold_policy_actions`
    in every frame between the draw and the Direction launch. The rollout's ``choice8`` keeps the policy's draw. ``held``
    (B,) int32 (optional, kept alive on ``fs``): += the rows held, per environment. Off (the default) the loop queues
    exactly the launches it always queued."""
    if held is not None:
        _contig(held, torch.int32, "held")
        if tuple(held.shape) != (fs.B,):
            raise ValueError(f"held must be (B,) = ({fs.B},)")
    _lib.check(_lib.load().tarl_fused_set_policy_hold(fs.ref, 1 if on else 0, _lib.ptr(held)))
    fs.policy_held = held


# ---- first-hop routing: empty origin roads select for their departing agent (NOT reference semantics) ----------
def _departure_args(plan: Plan, fs, pend, choice8, routed):
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    _contig(pend, torch.int32, "pend")
    if tuple(pend.shape) != (N, fs.B):
        raise ValueError(f"pend must be (N, B) = ({N}, {fs.B})")
    if choice8 is not None:
        _contig(choice8, torch.uint8, "choice8")
        if tuple(choice8.shape) != (fs.B, N):
            raise ValueError(f"choice8 must be (B, N) = ({fs.B}, {N})")
    if routed is not None:
        _contig(routed, torch.int32, "routed")
        if tuple(routed.shape) != (fs.B,):
            raise ValueError(f"routed must be (B,) = ({fs.B},)")


def _departure_table(plan: Plan, fs, dest_slot, table):
    N = plan.num_nodes
    _contig(dest_slot, torch.int32, "dest_slot")
    _contig(table, torch.int32, "table")
    if dest_slot.dim() != 1 or dest_slot.numel() != N or table.dim() not in (2, 3) or table.size(-1) != N or \
            (table.dim() == 3 and table.size(0) != fs.B):
        raise ValueError(f"dest_slot must be ({N},) and table (D, {N}) or ({fs.B}, D, {N}), got "
                         f"{tuple(dest_slot.shape)} and {tuple(table.shape)}")
    D = table.size(-2)
    return D * N if table.dim() == 3 else 0, D


def fused_pending_departures(plan: Plan, fs, t, out=None):
    """-> ``pend`` (N, B) int32: per road and environment the SMALLEST id among the agents that are ready to depart from it
    in the frame whose clock is ``t`` (waiting, DEPARTURE_TIME <= t: the insert rule's test; agent 0 counts), -1 where there
    is none (tarl_fused_pending_departures). With the departure window the scan starts at the insert cursor; neither the
    cursor nor any other word of ``fs`` is written. ``out``: such a tensor to write into (every entry is written)."""
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    t = float(t)
    if not math.isfinite(t):
        raise ValueError(f"t must be finite, got {t}")
    if out is None:
        out = torch.empty((N, fs.B), dtype=torch.int32, device=fs.hdp.device)
    _contig(out, torch.int32, "out")
    if tuple(out.shape) != (N, fs.B):
        raise ValueError(f"out must be (N, B) = ({N}, {fs.B})")
    _lib.check(_lib.load().tarl_fused_pending_departures(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, t, out.data_ptr(),
                                                         _lib.current_stream()))
    return out


def fused_route_departures(plan: Plan, fs, pend, dest_slot, table, choice8=None, routed=None):
    """First-hop routing by a next-hop table (tarl_fused_route_departures): every EMPTY road u of ``fs`` with
    ``pend[u][b] >= 0`` (:func:`fused_pending_departures`) selects the next hop towards that agent's destination —
    :func:`fused_select_next_hop_dest` with ``hold=True`` and the pending agent as the head, except that an unreachable
    destination (-1) leaves the row as it was. A non-empty road keeps its head's choice; every other row keeps its bytes.
    ``table`` int32 (D, N) or (B, D, N) with ``dest_slot`` (N,). ``choice8`` (B, N) uint8 (optional): the rows' bytes after
    the call, env-major. ``routed`` (B,) int32 (optional): += the rows written."""
    _departure_args(plan, fs, pend, choice8, routed)
    stride, D = _departure_table(plan, fs, dest_slot, table)
    _lib.check(_lib.load().tarl_fused_route_departures(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, pend.data_ptr(),
                                                       dest_slot.data_ptr(), table.data_ptr(), stride, D, _lib.ptr(choice8),
                                                       _lib.ptr(routed), _lib.current_stream()))
    return choice8


def fused_route_departures_plan(plan: Plan, fs, pend, routes, route_len, choice8=None, routed=None):
    """First-hop routing by a per-agent plan (tarl_fused_route_departures_plan): as :func:`fused_route_departures`, the
    lookup being :func:`fused_select_route`'s with the pending agent as the head. No route, or a road off the route: the
    row keeps its byte."""
    _departure_args(plan, fs, pend, choice8, routed)
    _check_dev(routes, torch.int32, "routes")
    _check_dev(route_len, torch.int32, "route_len")
    _contig(routes, torch.int32, "routes")
    _contig(route_len, torch.int32, "route_len")
    if routes.dim() not in (2, 3) or tuple(route_len.shape) != tuple(routes.shape[:-1]) or routes.size(-2) != fs.A or \
            routes.size(-1) < 1 or (routes.dim() == 3 and routes.size(0) != fs.B):
        raise ValueError(f"routes must be ({fs.A}, L) or ({fs.B}, {fs.A}, L) int32 and route_len the same without L, got "
                         f"{tuple(routes.shape)} and {tuple(route_len.shape)}")
    L = routes.size(-1)
    _lib.check(_lib.load().tarl_fused_route_departures_plan(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, pend.data_ptr(),
                                                            routes.data_ptr(), route_len.data_ptr(),
                                                            fs.A * L if routes.dim() == 3 else 0, L, _lib.ptr(choice8),
                                                            _lib.ptr(routed), _lib.current_stream()))
    return choice8


def fused_set_departure_router(fs, on, dest_slot=None, table=None, pend=None, routed=None, plan=None):
    """The switch of the state-dependent T-frame rollouts (tarl_fused_set_departure_router): with ``on`` their loop queues
    :func:`fused_pending_departures` into ``pend`` and :func:`fused_route_departures` with ``dest_slot`` / ``table`` in every
    frame, after the optional hold launch and before Direction. The rollout's ``choice8`` keeps the policy's draw.
    ``routed`` (B,) int32 (optional): += the rows written, per environment. The tensors are kept alive on ``fs``. Off (the
    default; no tensors) the loop queues exactly the launches it always queued."""
    if not on:
        if any(v is not None for v in (dest_slot, table, pend, routed)):
            raise ValueError("a table or a routed counter without the switch")
        _lib.check(_lib.load().tarl_fused_set_departure_router(fs.ref, 0, None, None, 0, 0, None, None))
        fs.departure_router = None
        return
    if dest_slot is None or table is None or pend is None or plan is None:
        raise ValueError("the switch needs plan, dest_slot, table and pend")
    _departure_args(plan, fs, pend, None, routed)
    stride, D = _departure_table(plan, fs, dest_slot, table)
    _lib.check(_lib.load().tarl_fused_set_departure_router(fs.ref, 1, dest_slot.data_ptr(), table.data_ptr(), stride, D,
                                                           pend.data_ptr(), _lib.ptr(routed)))
    fs.departure_router = (dest_slot, table, pend, routed)


# ---- the trip reward: travellers who should be under way and have not arrived (NOT reference semantics) --------
def fused_trip_reward(plan: Plan, fs, t, out=None, parts=None):
    """-> ``reward`` (B,) fp32 = -(on_way + ready) per environment, after the frame whose clock is ``t`` has run completely
    (tarl_fused_trip_reward): on_way = agents with status 1, ready = waiting agents with DEPARTURE_TIME <= t (the insert
    rule's test; every row of the agent table counts, agent 0 too). With the departure window ``ready`` is the walk from
    the insert cursor; neither the cursor nor any other word of ``fs`` is written. ``out``: such a tensor to write into;
    ``parts`` (B, 2) int32 (optional): {on_way, ready}. Every element of both is overwritten."""
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    t = float(t)
    if not math.isfinite(t):
        raise ValueError(f"t must be finite, got {t}")
    if out is None:
        out = torch.empty((fs.B,), dtype=torch.float32, device=fs.hdp.device)
    _contig(out, torch.float32, "out")
    if tuple(out.shape) != (fs.B,):
        raise ValueError(f"out must be (B,) = ({fs.B},)")
    if parts is not None:
        _contig(parts, torch.int32, "parts")
        if tuple(parts.shape) != (fs.B, 2):
            raise ValueError(f"parts must be (B, 2) = ({fs.B}, 2)")
    _lib.check(_lib.load().tarl_fused_trip_reward(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, t, out.data_ptr(), _lib.ptr(parts),
                                                  _lib.current_stream()))
    return out


def fused_set_trip_reward(fs, on, parts=None):
    """The switch of the state-dependent T-frame rollouts (tarl_fused_set_trip_reward): with ``on`` their loop queues
    :func:`fused_trip_reward` in every frame after the insert launch, into the rollout's ``reward[t]``: the reward buffer
    then holds the trip reward instead of the queue reward. ``parts`` (T_max, B, 2) int32 (optional, kept alive on ``fs``):
    {on_way, ready} of frame t at ``parts[t]``; the rollout must not run more than T_max frames. Action bytes, log-probs and
    count bytes are the same either way. Off (the default) the loop queues exactly the launches it always queued."""
    if parts is not None:
        if not on:
            raise ValueError("a parts buffer without the switch")
        _contig(parts, torch.int32, "parts")
        if parts.dim() != 3 or tuple(parts.shape[1:]) != (fs.B, 2):
            raise ValueError(f"parts must be (T_max, B, 2) = (T_max, {fs.B}, 2)")
    _lib.check(_lib.load().tarl_fused_set_trip_reward(fs.ref, 1 if on else 0, _lib.ptr(parts)))
    fs.trip_parts = parts


BC_IGNORE = 0xFF        # TARL_BC_IGNORE: the label byte of a row the expert says nothing about


def fused_expert_labels(plan: Plan, fs, dest_slot, table, out=None, n_labelled=None):
    """The shortest-path router's action of every row of ``fs`` as a LABEL in the policy's action space
    (tarl_fused_expert_labels): the rank byte :func:`fused_select_next_hop_dest` (hold off) would write, with the
    packed state left untouched. -> uint8 (B, N) env-major (``out``: written in place); ``BC_IGNORE`` on empty rows, on rows
    the select kernel leaves untouched and on rows where it writes the raw code. ``table`` int32 (D, N) shared by the
    environments or (B, D, N); ``dest_slot`` (N,) int32. ``n_labelled`` (B,) int32 (optional): += the labelled rows."""
    N = plan.num_nodes
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    _contig(dest_slot, torch.int32, "dest_slot")
    _contig(table, torch.int32, "table")
    if dest_slot.dim() != 1 or dest_slot.numel() != N or table.dim() not in (2, 3) or table.size(-1) != N or \
            (table.dim() == 3 and table.size(0) != fs.B):
        raise ValueError(f"dest_slot must be ({N},) and table (D, {N}) or ({fs.B}, D, {N}), got "
                         f"{tuple(dest_slot.shape)} and {tuple(table.shape)}")
    D = table.size(-2)
    if out is None:
        out = torch.empty((fs.B, N), dtype=torch.uint8, device=table.device)
    _contig(out, torch.uint8, "out")
    if tuple(out.shape) != (fs.B, N):
        raise ValueError(f"out must be (B, N) = ({fs.B}, {N})")
    if n_labelled is not None:
        _contig(n_labelled, torch.int32, "n_labelled")
        if tuple(n_labelled.shape) != (fs.B,):
            raise ValueError(f"n_labelled must be (B,) = ({fs.B},)")
    _lib.check(_lib.load().tarl_fused_expert_labels(plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, dest_slot.data_ptr(),
                                                    table.data_ptr(), D * N if table.dim() == 3 else 0, D, out.data_ptr(),
                                                    _lib.ptr(n_labelled), _lib.current_stream()))
    return out


def graphdist_bc(plan: Plan, logits, labels, temperature=1.0, grad_scale=None, want_grad=True, scratch=None):
    """Cross-entropy of GraphDistribution(logits / temperature) on the labelled nodes, forward and backward
    (tarl_graphdist_bc). ``logits`` fp32 (M, E), ``labels`` uint8 (M, N): node n is labelled when its byte is
    below min(out-degree, 0x7F). -> (nll fp64 (M,), n_labelled int32 (M,), n_hit int32 (M,), grad_logits fp32 (M, E) or
    None). ``grad_scale``: the factor on every gradient element, 1 / (labelled nodes of the minibatch) for the mean loss;
    None: taken from a forward-only call first. ``scratch`` (optional): a device tensor of any dtype to reuse across calls;
    only its size in bytes (at least ``tarl_graphdist_bc_scratch_bytes(plan, M)``) and an 8-byte aligned address matter. The C
    entry point takes no size, so a smaller one is refused HERE, from the shapes alone: before the tensors are looked at,
    before anything is allocated and before any HIP call."""
    L = _lib.load()
    E, N = plan.num_edges, plan.num_nodes
    if logits.dim() != 2 or logits.size(1) != E or labels.dim() != 2 or tuple(labels.shape) != (logits.size(0), N):
        raise ValueError(f"logits must be (M, {E}) and labels (M, {N}), got {tuple(logits.shape)} and {tuple(labels.shape)}")
    M = logits.size(0)
    if M < 1 or not float(temperature) > 0.0:
        raise ValueError("M must be >= 1 and temperature positive")
    need = int(L.tarl_graphdist_bc_scratch_bytes(plan.handle, M))
    if need < 0:
        raise _lib.TarlError("tarl_graphdist_bc_scratch_bytes refused the sizes")
    if scratch is not None and scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch holds {scratch.numel() * scratch.element_size()} bytes, tarl_graphdist_bc needs {need}")
    _contig(logits, torch.float32, "logits")
    _contig(labels, torch.uint8, "labels")
    if scratch is None:
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=logits.device)
    elif not scratch.is_cuda or not scratch.is_contiguous():
        raise _lib.TarlError("scratch must be a contiguous tensor on the GPU")
    dev = logits.device
    nll = torch.empty(M, dtype=torch.float64, device=dev)
    n_lab = torch.empty(M, dtype=torch.int32, device=dev)
    n_hit = torch.empty(M, dtype=torch.int32, device=dev)

    def call(scale, grad):
        _lib.check(L.tarl_graphdist_bc(plan.handle, logits.data_ptr(), M, float(temperature), labels.data_ptr(), float(scale),
                                       nll.data_ptr(), n_lab.data_ptr(), n_hit.data_ptr(), _lib.ptr(grad), scratch.data_ptr(),
                                       _lib.current_stream()))
    grad = torch.empty_like(logits) if want_grad else None
    if want_grad and grad_scale is None:
        call(0.0, None)
        grad_scale = 1.0 / max(int(n_lab.sum().item()), 1)
    call(0.0 if grad_scale is None else grad_scale, grad)
    return nll, n_lab, n_hit, grad


# ---- per-decision PPO credit (csrc/decision_credit.hip; NOT reference semantics) -----------------------------------
HEAD_CAPTURE = 8        # TARL_HEAD_CAPTURE: bit 3 of tarl_fused.policy_hold


def _rows_n(t, dtype, N, name, rows=None):
    """A contiguous device (rows, N) tensor of ``dtype``."""
    _contig(t, dtype, name)
    if t.dim() != 2 or t.size(1) != N or (rows is not None and t.size(0) != rows):
        raise ValueError(f"{name} must be ({'rows' if rows is None else rows}, {N}), got {tuple(t.shape)}")
    return t


def _row_list(t, n, name):
    _contig(t, torch.int32, name)
    if t.dim() != 1 or (n is not None and t.numel() != n):
        raise ValueError(f"{name} must be a 1-D int32 tensor{'' if n is None else f' of {n} entries'}, got {tuple(t.shape)}")
    return t.numel()


def _counts2(counts):
    """The {headed, due} counters of credit scope "due": int32 (2,) on the device, or None."""
    if counts is not None:
        _contig(counts, torch.int32, "counts")
        if counts.numel() != 2:
            raise ValueError(f"counts must hold two int32 {{headed, due}}, got {tuple(counts.shape)}")
    return counts


def fused_head_rows(plan: Plan, fs, env, slot, head_keep, t=None, counts=None):
    """``head_keep[slot[j]][u]`` (int32 (rows, N)) = the head agent id of road u in environment ``env[j]`` of ``fs`` where the
    road's FIFO is not empty, 0 otherwise (tarl_fused_head_rows): whom each road's decision of the next frame is taken for.
    ``env`` / ``slot``: int32 (n,) device tensors; the slots must be rows of ``head_keep`` (the kernel trusts them, as
    :func:`fused_obs16_rows` trusts its own). Reads ``fs.hdp`` alone.
    With ``t`` (credit scope "due"; tarl_fused_head_rows_due): the clock the next frame is stepped with; the id
    only where the head's departure is ``<= t`` as well (Direction's fp32 test), and ``counts`` (int32 (2,), optional) +=
    {roads with a head, roads with a due head}."""
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    n = _row_list(env, None, "env")
    _row_list(slot, n, "slot")
    _rows_n(head_keep, torch.int32, plan.num_nodes, "head_keep")
    if t is None:
        if counts is not None:
            raise ValueError("counts belongs to the due scope: it needs the clock t")
        _lib.check(_lib.load().tarl_fused_head_rows(plan.handle, fs.ref, fs.B, env.data_ptr(), slot.data_ptr(), n,
                                                    head_keep.data_ptr(), _lib.current_stream()))
        return head_keep
    if not math.isfinite(float(t)):
        raise ValueError(f"t must be a finite clock, got {t}")
    _lib.check(_lib.load().tarl_fused_head_rows_due(plan.handle, fs.ref, fs.B, float(t), env.data_ptr(), slot.data_ptr(), n,
                                                    head_keep.data_ptr(), _lib.ptr(_counts2(counts)), _lib.current_stream()))
    return head_keep


def fused_set_head_capture(fs, on, head_keep=None, plan=None, scope="headed", counts=None):
    """The switch of the state-dependent T-frame rollouts (tarl_fused_set_head_capture): with ``on`` their loop queues
    :func:`fused_head_rows` for the kept (environment, slot) pairs of every frame in front of that frame's head call, into
    ``head_keep`` (int32 (rows, N), kept alive on ``fs``; its rows are the rows of the rollout's ``obs_keep``). Off (the
    default, ``head_keep`` None) the loop queues exactly the launches it always queued.
    ``scope="due"`` (tarl_fused_set_head_capture_scope): the loop queues the due form with every frame's clock
    instead, ``counts`` (int32 (2,), optional, kept alive on ``fs``) += {headed, due}. ``"headed"`` makes no further call."""
    if scope not in ("headed", "due"):
        raise ValueError("scope must be 'headed' or 'due'")
    if (scope == "due" or counts is not None) and not on:
        raise ValueError("scope and counts belong to the switched-on capture")
    if scope != "due" and counts is not None:
        raise ValueError("counts belongs to scope 'due'")
    _counts2(counts)
    if on:
        if head_keep is None:
            raise ValueError("the switch needs its head_keep buffer")
        _contig(head_keep, torch.int32, "head_keep")
        if head_keep.dim() != 2 or (plan is not None and head_keep.size(1) != plan.num_nodes):
            raise ValueError(f"head_keep must be (rows, N), got {tuple(head_keep.shape)}")
    elif head_keep is not None:
        raise ValueError("a head_keep buffer without the switch")
    _lib.check(_lib.load().tarl_fused_set_head_capture(fs.ref, 1 if on else 0, _lib.ptr(head_keep)))
    fs.head_keep = head_keep
    fs.head_counts = None
    if scope == "due":
        _lib.check(_lib.load().tarl_fused_set_head_capture_scope(fs.ref, 1, _lib.ptr(counts)))
        fs.head_counts = counts


def fused_agent_roads(plan: Plan, fs, Nmax, out=None, bad=None):
    """-> int32 (B, A): the road every agent of ``fs`` is queued on, -1 where it is queued nowhere (waiting, arrived, or lost)
    (tarl_fused_agent_roads). Reads the packed FIFOs alone (count, ring offset, the slots below the count) and
    writes nothing of the state. ``bad`` (int32 (1,), optional) += the ids outside [1, A) it met, plus, off the defined domain,
    the whole count of a row whose ring offset is >= Nmax (nothing of it is read) and the part of a count above Nmax."""
    _check_dev(fs.hdp, torch.int32, "fs.hdp")
    if out is None:
        out = torch.empty((fs.B, fs.A), dtype=torch.int32, device=fs.hdp.device)
    _contig(out, torch.int32, "out")
    if tuple(out.shape) != (fs.B, fs.A):
        raise ValueError(f"out must be ({fs.B}, {fs.A}), got {tuple(out.shape)}")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=out.device)
    _contig(bad, torch.int32, "bad")
    if bad.numel() != 1:
        raise ValueError("bad must hold one int32")
    _lib.check(_lib.load().tarl_fused_agent_roads(plan.handle, fs.ref, fs.B, fs.A, int(Nmax), out.data_ptr(), bad.data_ptr(),
                                                  _lib.current_stream()))
    return out


def decision_advantage(plan: Plan, head_keep, frame, env, slot, agent_features, times, t_end, dist, dest_slot, *, B,
                       timestep, decision_gamma=1.0, adv_raw, truncated, bad, agent_road=None, bootstrap=False,
                       bootstrapped=None):
    """The raw per-decision advantage of the kept rows of ONE episode segment (tarl_decision_advantage), to be called
    before the engine is reset: row j is frame ``frame[j]``, environment ``env[j]``, row ``slot[j]`` of ``head_keep`` /
    ``adv_raw`` ((rows, N) int32 / fp32). ``times`` (T + 1,) fp32 device clocks, ``t_end``: the segment ends after frame
    t_end - 1; ``dist`` (D, N) float64 free-flow distances of :func:`destination_trees`, ``dest_slot`` (N,) int32.
    Writes ``adv_raw`` of every road of the listed rows (0 where not live), clears ``head_keep`` where the decision is not
    live, and adds to ``truncated`` / ``bad`` (int32 (1,)).
    With ``agent_road`` (int32 (B, A) of :func:`fused_agent_roads`, taken when the segment ended) and ``bootstrapped``
    (int32 (1,)) the call is tarl_decision_advantage_boot: ``bootstrap`` True continues a traveller still under
    way at the horizon in free flow from the road it is queued on and counts it in ``bootstrapped`` instead of
    ``truncated``; False gives the plain call's output bit for bit."""
    N = plan.num_nodes
    boot_call = agent_road is not None or bootstrapped is not None
    if bootstrap and not boot_call:
        raise ValueError("bootstrap needs agent_road and bootstrapped")
    n = _row_list(frame, None, "frame")
    _row_list(env, n, "env")
    _row_list(slot, n, "slot")
    _rows_n(head_keep, torch.int32, N, "head_keep")
    _rows_n(adv_raw, torch.float32, N, "adv_raw", head_keep.size(0))
    A, abs_ = _agents(agent_features, B)
    _contig(times, torch.float32, "times")
    _contig(dist, torch.float64, "dist")
    _contig(dest_slot, torch.int32, "dest_slot")
    if times.dim() != 1 or dist.dim() != 2 or dist.size(1) != N or tuple(dest_slot.shape) != (N,):
        raise ValueError(f"times must be 1-D, dist (D, {N}) and dest_slot ({N},), got {tuple(times.shape)}, "
                         f"{tuple(dist.shape)} and {tuple(dest_slot.shape)}")
    for nm, t_ in (("truncated", truncated), ("bad", bad)):
        _contig(t_, torch.int32, nm)
        if t_.numel() != 1:
            raise ValueError(f"{nm} must hold one int32")
    if not 1 <= int(t_end) <= times.numel():
        raise ValueError(f"t_end must be in [1, {times.numel()}], got {t_end}")
    if not (float(timestep) > 0.0 and 0.0 < float(decision_gamma) <= 1.0):
        raise ValueError("timestep must be positive and decision_gamma in (0, 1]")
    args = (plan.handle, head_keep.data_ptr(), frame.data_ptr(), env.data_ptr(), slot.data_ptr(), n, int(B),
            agent_features.data_ptr(), A, abs_, times.data_ptr(), times.numel(), int(t_end), dist.data_ptr(),
            dest_slot.data_ptr(), dist.size(0), float(timestep), float(decision_gamma), adv_raw.data_ptr(),
            truncated.data_ptr(), bad.data_ptr())
    if not boot_call:
        _lib.check(_lib.load().tarl_decision_advantage(*args, _lib.current_stream()))
        return adv_raw
    if agent_road is None or bootstrapped is None:
        raise ValueError("agent_road and bootstrapped go together")
    _contig(agent_road, torch.int32, "agent_road")
    if tuple(agent_road.shape) != (int(B), A):
        raise ValueError(f"agent_road must be ({int(B)}, {A}), got {tuple(agent_road.shape)}")
    _contig(bootstrapped, torch.int32, "bootstrapped")
    if bootstrapped.numel() != 1:
        raise ValueError("bootstrapped must hold one int32")
    _lib.check(_lib.load().tarl_decision_advantage_boot(*args, agent_road.data_ptr(), 1 if bootstrap else 0,
                                                        bootstrapped.data_ptr(), _lib.current_stream()))
    return adv_raw


def decision_stats(adv_raw, head_keep):
    """-> float64 (3,) = {sum, sum of squares, count} of ``adv_raw`` over the elements with ``head_keep > 0``
    (tarl_decision_stats): :func:`advantage_stats` with a mask, the layout :func:`advantage_normalize_` reads."""
    _contig(adv_raw, torch.float32, "adv_raw")
    _contig(head_keep, torch.int32, "head_keep")
    if adv_raw.shape != head_keep.shape or adv_raw.numel() < 1:
        raise ValueError(f"adv_raw and head_keep must have one non-empty shape, got {tuple(adv_raw.shape)} and "
                         f"{tuple(head_keep.shape)}")
    partial = torch.empty(768, dtype=torch.float64, device=adv_raw.device)
    stats = torch.empty(3, dtype=torch.float64, device=adv_raw.device)
    _lib.check(_lib.load().tarl_decision_stats(adv_raw.data_ptr(), head_keep.data_ptr(), adv_raw.numel(), partial.data_ptr(),
                                               stats.data_ptr(), _lib.current_stream()))
    return stats


def _decision_logits(plan: Plan, logits, temperature):
    _contig(logits, torch.float32, "logits")
    if logits.dim() != 2 or logits.size(1) != plan.num_edges or logits.size(0) < 1:
        raise ValueError(f"logits must be (M, {plan.num_edges}) with M >= 1, got {tuple(logits.shape)}")
    if not float(temperature) > 0.0:
        raise ValueError("temperature must be positive")
    return logits.size(0)


def graphdist_node_logprob(plan: Plan, logits, choice, temperature=1.0, out=None):
    """-> fp32 (M, N): log(p_choice + 1e-8) of every node's categorical over its out-edges, p = softmax(logits /
    temperature) (tarl_graphdist_node_logprob); 0 where ``choice`` (int32 (M, N), the edge ids :func:`rollout_gather`
    returns, -1: none) names no out-edge of the node. The sum over the nodes is GraphDistribution's joint log-prob."""
    M = _decision_logits(plan, logits, temperature)
    _rows_n(choice, torch.int32, plan.num_nodes, "choice", M)
    if out is None:
        out = torch.empty((M, plan.num_nodes), dtype=torch.float32, device=logits.device)
    _rows_n(out, torch.float32, plan.num_nodes, "out", M)
    _lib.check(_lib.load().tarl_graphdist_node_logprob(plan.handle, logits.data_ptr(), M, float(temperature),
                                                       choice.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return out


def graphdist_decision_ppo(plan: Plan, logits, choice, head, lp_old_node, adv_raw, stats3, n_live, *, clip_epsilon=0.2,
                           temperature=1.0, grad_scale=1.0, grad_logits=None, scratch=None):
    """The clipped PPO objective per live decision, forward and backward (tarl_graphdist_decision_ppo).
    ``logits`` fp32 (M, E); ``choice`` / ``head`` int32 (M, N) (``head > 0``: live), ``lp_old_node`` / ``adv_raw`` fp32
    (M, N); ``stats3`` float64 (3,) of :func:`decision_stats` (all-reduced where the statistic is global); ``n_live`` int32
    (1,) on the device: the live decisions of this minibatch, the L of the mean. -> float64 (M, 4) = per sample {sum of the
    clipped gains, live decisions, ratios outside the clip, sum of lp_old - lp}. ``grad_logits`` fp32 (M, E) (optional):
    the gradient of -(1 / L) * sum of the gains times ``grad_scale`` is ADDED on the out-edges of the live nodes."""
    L = _lib.load()
    N = plan.num_nodes
    M = _decision_logits(plan, logits, temperature)
    need = int(L.tarl_graphdist_decision_ppo_scratch_bytes(plan.handle, M))
    if need < 0:
        raise _lib.TarlError("tarl_graphdist_decision_ppo_scratch_bytes refused the sizes")
    if scratch is not None and scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch holds {scratch.numel() * scratch.element_size()} bytes, tarl_graphdist_decision_ppo needs "
                         f"{need}")
    _rows_n(choice, torch.int32, N, "choice", M)
    _rows_n(head, torch.int32, N, "head", M)
    _rows_n(lp_old_node, torch.float32, N, "lp_old_node", M)
    _rows_n(adv_raw, torch.float32, N, "adv_raw", M)
    _contig(stats3, torch.float64, "stats3")
    _contig(n_live, torch.int32, "n_live")
    if stats3.numel() != 3 or n_live.numel() != 1:
        raise ValueError("stats3 must hold three float64 and n_live one int32")
    if not 0.0 <= float(clip_epsilon) < 1.0:
        raise ValueError("clip_epsilon must be in [0, 1)")
    if grad_logits is not None:
        _contig(grad_logits, torch.float32, "grad_logits")
        if grad_logits.shape != logits.shape:
            raise ValueError(f"grad_logits must be {tuple(logits.shape)}, got {tuple(grad_logits.shape)}")
    if scratch is None:
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=logits.device)
    elif not scratch.is_cuda or not scratch.is_contiguous():
        raise _lib.TarlError("scratch must be a contiguous tensor on the GPU")
    out4 = torch.empty((M, 4), dtype=torch.float64, device=logits.device)
    _lib.check(L.tarl_graphdist_decision_ppo(plan.handle, logits.data_ptr(), M, float(temperature), choice.data_ptr(),
                                             head.data_ptr(), lp_old_node.data_ptr(), adv_raw.data_ptr(), stats3.data_ptr(),
                                             n_live.data_ptr(), float(clip_epsilon), float(grad_scale), out4.data_ptr(),
                                             _lib.ptr(grad_logits), scratch.data_ptr(), _lib.current_stream()))
    return out4


def graphdist_mode(plan: Plan, proba, *, want_choice=False):
    L = _lib.load()
    _contig(proba, torch.float32, "proba")
    B = _rows(proba, plan.num_edges, "proba")
    onehot = torch.zeros_like(proba)
    choice = (torch.empty(proba.shape[:-1] + (plan.num_nodes,), dtype=torch.int32, device=proba.device)
              if want_choice else None)
    _lib.check(L.tarl_graphdist_mode(plan.handle, proba.data_ptr(), B, onehot.data_ptr(), _lib.ptr(choice),
                                     _lib.current_stream()))
    return onehot, choice


def graphdist_logprob_entropy(plan: Plan, proba, *, action_onehot=None, choice=None, want_logprob=True,
                              want_entropy=True):
    L = _lib.load()
    _contig(proba, torch.float32, "proba")
    B = _rows(proba, plan.num_edges, "proba")
    shape = proba.shape[:-1]
    if action_onehot is not None:
        _contig(action_onehot, torch.int64, "action")
    if choice is not None:
        _contig(choice, torch.int32, "choice")
    lp = torch.empty(shape, dtype=torch.float32, device=proba.device) if want_logprob else None
    ent = torch.empty(shape, dtype=torch.float32, device=proba.device) if want_entropy else None
    _lib.check(L.tarl_graphdist_logprob_entropy_fwd(plan.handle, proba.data_ptr(), B, _lib.ptr(action_onehot),
                                                    _lib.ptr(choice), _lib.ptr(lp), _lib.ptr(ent),
                                                    _lib.current_stream()))
    return lp, ent


def graphdist_logprob_entropy_bwd(plan: Plan, proba, temperature, *, action_onehot=None, choice=None,
                                  grad_log_prob=None, grad_entropy=None, log_prob_fwd=None):
    L = _lib.load()
    _contig(proba, torch.float32, "proba")
    B = _rows(proba, plan.num_edges, "proba")
    for name, t in (("grad_log_prob", grad_log_prob), ("grad_entropy", grad_entropy), ("log_prob_fwd", log_prob_fwd)):
        if t is not None:
            _contig(t, torch.float32, name)
    grad = torch.zeros_like(proba)
    _lib.check(L.tarl_graphdist_logprob_entropy_bwd(plan.handle, proba.data_ptr(), B, float(temperature),
                                                    _lib.ptr(action_onehot), _lib.ptr(choice),
                                                    _lib.ptr(grad_log_prob), _lib.ptr(grad_entropy),
                                                    _lib.ptr(log_prob_fwd), grad.data_ptr(), _lib.current_stream()))
    return grad


# ---- policy -----------------------------------------------------------------------------------------------------------
def _road_index_view(node_features: torch.Tensor, plan: Plan):
    """node_features (..., N, C>=7): the ROAD_INDEX observation column (ObservationFeatureHelpers.ROAD_INDEX = 6)."""
    _check_dev(node_features, torch.float32, "node_features")
    if node_features.dim() == 2:
        nf = node_features.unsqueeze(0)
    else:
        nf = node_features.reshape(-1, node_features.size(-2), node_features.size(-1))
    if nf.size(1) != plan.num_nodes or nf.size(2) < 7:
        raise ValueError("node_features must be (..., N, >=7)")
    col = nf[:, :, 6]
    return col, nf.size(0), col.stride(0), col.stride(1)


def policy_edge_logits(plan: Plan, node_features, emb):
    L = _lib.load()
    _contig(emb, torch.float32, "emb")
    col, B, bs, ns = _road_index_view(node_features, plan)
    shape = (plan.num_edges,) if node_features.dim() == 2 else tuple(node_features.shape[:-2]) + (plan.num_edges,)
    logits = torch.empty(shape, dtype=torch.float32, device=emb.device)
    _lib.check(L.tarl_policy_edge_logits_fwd(plan.handle, col.data_ptr(), bs, ns, B, emb.data_ptr(), emb.numel(),
                                             logits.data_ptr(), _lib.current_stream()))
    return logits


def policy_edge_logits_bwd(plan: Plan, node_features, grad_logits, num_embeddings):
    L = _lib.load()
    _contig(grad_logits, torch.float32, "grad_logits")
    col, B, bs, ns = _road_index_view(node_features, plan)
    grad_emb = torch.zeros(num_embeddings, dtype=torch.float32, device=grad_logits.device)
    scratch = None
    if bs == 0 and B >= 256:      # one observation broadcast over many rows: the row sum in parallel chunks
        scratch = torch.empty(int(L.tarl_policy_edge_logits_bwd_scratch_floats(plan.handle, B)), dtype=torch.float32,
                              device=grad_logits.device)
    _lib.check(L.tarl_policy_edge_logits_bwd(plan.handle, col.data_ptr(), bs, ns, B, grad_logits.data_ptr(),
                                             grad_emb.data_ptr(), num_embeddings, _lib.ptr(scratch), _lib.current_stream()))
    return grad_emb


# ---- per-edge MLP policy head ----------------------------------------------------------------------------------------------
class EdgeMlpWeights:
    """Flat views of the reference's ``edge_mlp.{0,2,4}.{weight,bias}`` tensors (device, fp32, contiguous)."""

    def __init__(self, w1, b1, w2, b2, w3, b3):
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = (_contig(t.detach(), torch.float32, n) for t, n in
                                                               ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"),
                                                                (w3.reshape(-1), "w3"), (b3, "b3")))
        if self.w1.shape != (64, 33) or self.w2.shape != (32, 64) or self.w3.numel() != 32:
            raise ValueError("edge_mlp must be 33 -> 64 -> 32 -> 1")

    def ptrs(self):
        return [t.data_ptr() for t in (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)]


def policy_obs16(node_features, agent_index, agent_features):
    """x = cat(node_features[..., :7], agent_features[agent_index]) -> (M, N, 16) (src/agents/mpnn_agent.py:166-178).
    ``node_features`` (N, >=7) or (M, N, >=7) (last dim contiguous), ``agent_index`` int64 matching, ``agent_features``
    (A, 9) shared or (M, A, 9)."""
    L = _lib.load()
    _check_dev(node_features, torch.float32, "node_features")
    nf = node_features.unsqueeze(0) if node_features.dim() == 2 else node_features
    M, N = nf.shape[:2]
    if nf.stride(-1) != 1 or nf.stride(0) != N * nf.stride(1):     # rows may be strided (a view of x), samples may not
        nf = nf.contiguous()
    ai = _contig(agent_index.reshape(M, N).to(torch.int64), torch.int64, "agent_index")
    ag = _contig(agent_features, torch.float32, "agent_features")
    A = ag.size(-2)
    obs = torch.empty((M, N, 16), dtype=torch.float32, device=nf.device)
    _lib.check(L.tarl_policy_obs16(nf.data_ptr(), nf.stride(1), ai.data_ptr(), ag.data_ptr(), A,
                                   A * 9 if ag.dim() == 3 else 0, M, N, obs.data_ptr(), _lib.current_stream()))
    return obs


def fused_obs16(plan: Plan, fs, x, Nmax, agent_features, out=None):
    """The same observation from the packed state of the fused engine: (B, N, 16)."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    obs = out if out is not None else torch.empty((B, N, 16), dtype=torch.float32, device=x.device)
    _lib.check(L.tarl_fused_obs16(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, agent_features.data_ptr(), A, abs_,
                                  obs.data_ptr(), _lib.current_stream()))
    return obs


def fused_obs16_bf16(plan: Plan, fs, x, Nmax, agent_features, out=None):
    """The packed state's observation rounded to bf16 (RNE): (B, N, 16) torch.bfloat16."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    obs = out if out is not None else torch.empty((B, N, 16), dtype=torch.bfloat16, device=x.device)
    _lib.check(L.tarl_fused_obs16_bf16(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, agent_features.data_ptr(), A,
                                       abs_, obs.data_ptr(), _lib.current_stream()))
    return obs


def fused_obs16_rows(plan: Plan, fs, x, Nmax, agent_features, env, slot, out):
    """fp32 observation rows of a few environments: ``out[slot[j]] = obs[env[j]]`` (``out`` (K, N, 16), int32 lists)."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    _contig(env, torch.int32, "env")
    _contig(slot, torch.int32, "slot")
    _contig(out, torch.float32, "out")
    _lib.check(L.tarl_fused_obs16_rows(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, agent_features.data_ptr(), A,
                                       abs_, env.data_ptr(), slot.data_ptr(), env.numel(), out.data_ptr(),
                                       _lib.current_stream()))
    return out


def fused_set_actions(plan: Plan, fs, choice8):
    """Env-major action bytes ``choice8`` (B, N) uint8 -> the SELECTED_ROAD column of the packed state (env-minor). A byte
    with bit 7 set keeps the road's previous value; the completed code is written back into ``choice8``."""
    L = _lib.load()
    _contig(choice8, torch.uint8, "choice8")
    if choice8.dim() != 2 or choice8.size(0) != fs.B or choice8.size(1) != plan.num_nodes:
        raise ValueError(f"choice8 must be (B, N) = ({fs.B}, {plan.num_nodes})")
    _lib.check(L.tarl_fused_set_actions(plan.handle, fs.ref, fs.B, choice8.data_ptr(), _lib.current_stream()))
    return choice8


EDGE_MLP_PRECISIONS = ("fp32", "bf16", "x3")


def _edge_mlp_precision(bf16, precision):
    """``precision``: "fp32" = fp32 MFMA (exact fp32 products), "bf16" = bf16 MFMA, "x3" = fp32 accuracy on the bf16 pipe
    (operands split into three exact bf16 pieces). ``bf16=True`` is the older spelling of precision="bf16"."""
    if precision is None:
        precision = "bf16" if bf16 else "fp32"
    if precision not in EDGE_MLP_PRECISIONS:
        raise ValueError(f"precision must be one of {EDGE_MLP_PRECISIONS}")
    return precision


def policy_edge_mlp(plan: Plan, obs16, ec: EdgeConst, w: EdgeMlpWeights, *, bf16=False, precision=None, out=None):
    """obs16 (M, N, 16) -> logits (M, E) of the per-edge MLP head: fp32 MFMA (default), bf16 MFMA (``bf16=True`` /
    ``precision="bf16"``) or fp32-accurate on the bf16 pipe (``precision="x3"``); ``obs16`` in torch.bfloat16
    (fused_obs16_bf16) selects the bf16 MFMA kernel that reads bf16 observations."""
    L = _lib.load()
    if obs16.dtype == torch.bfloat16:
        _contig(obs16, torch.bfloat16, "obs16")
        if obs16.shape[1:] != (plan.num_nodes, 16):
            raise ValueError("obs16 must be (M, num_nodes, 16)")
        M = obs16.size(0)
        logits = out if out is not None else torch.empty((M, plan.num_edges), dtype=torch.float32, device=obs16.device)
        _lib.check(L.tarl_policy_edge_mlp_fwd(plan.handle, obs16.data_ptr(), M, ec.edge_attr.data_ptr(), *w.ptrs(), 2,
                                              logits.data_ptr(), _lib.current_stream()))
        return logits
    _contig(obs16, torch.float32, "obs16")
    M = obs16.size(0)
    if obs16.shape[1:] != (plan.num_nodes, 16):
        raise ValueError("obs16 must be (M, num_nodes, 16)")
    logits = out if out is not None else torch.empty((M, plan.num_edges), dtype=torch.float32, device=obs16.device)
    code = {"fp32": 0, "bf16": 1, "x3": 3}[_edge_mlp_precision(bf16, precision)]
    _lib.check(L.tarl_policy_edge_mlp_fwd(plan.handle, obs16.data_ptr(), M, ec.edge_attr.data_ptr(), *w.ptrs(),
                                          code, logits.data_ptr(), _lib.current_stream()))
    return logits


def edge_mlp_bwd_scratch_floats(plan: Plan, M: int) -> int:
    """fp32 elements of device scratch one tarl_policy_edge_mlp_bwd call over ``M`` samples needs (k-major activations and
    their gradients of every edge + the split partial sums)."""
    return int(_lib.load().tarl_policy_edge_mlp_bwd_scratch_floats(plan.handle, int(M)))


def policy_edge_mlp_bwd(plan: Plan, obs16, ec: EdgeConst, w: EdgeMlpWeights, grad_logits, grads, scratch=None):
    """Accumulates into ``grads`` = (gw1, gb1, gw2, gb2, gw3, gb3), tensors shaped like the weights (fp32, contiguous).
    ``scratch``: an fp32 contiguous device tensor of at least ``edge_mlp_bwd_scratch_floats(plan, M)`` elements to reuse
    across calls (ValueError otherwise; allocated per call when None). The kernels write every element they read."""
    L = _lib.load()
    _contig(obs16, torch.float32, "obs16")
    gl = _contig(grad_logits, torch.float32, "grad_logits")
    M = obs16.size(0)
    if gl.numel() != M * plan.num_edges:
        raise ValueError("grad_logits must be (M, E)")
    need = int(L.tarl_policy_edge_mlp_bwd_scratch_floats(plan.handle, M))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=obs16.device)
    elif (not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.float32 or not scratch.is_contiguous()
          or scratch.device != obs16.device or scratch.numel() < need):
        raise ValueError(f"scratch must be a contiguous fp32 tensor on {obs16.device} of at least {need} elements")
    gs = [_contig(g, torch.float32, "grad") for g in grads]
    _lib.check(L.tarl_policy_edge_mlp_bwd(plan.handle, obs16.data_ptr(), M, ec.edge_attr.data_ptr(), *w.ptrs(),
                                          gl.data_ptr(), scratch.data_ptr(), *(g.data_ptr() for g in gs),
                                          _lib.current_stream()))


# ---- critic -----------------------------------------------------------------------------------------------------------
class CriticWeights:
    """Flat views of the reference's ``final_mlp.{0,2,4}.{weight,bias}`` tensors (device, fp32, contiguous)."""

    def __init__(self, w1, b1, w2, b2, w3, b3):
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = (_contig(t, torch.float32, n) for t, n in
                                                               ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"),
                                                                (w3, "w3"), (b3, "b3")))
        if self.w1.size(0) != 64 or self.w2.shape != (64, 64) or self.w3.numel() != 64:
            raise ValueError("critic must be (N+1)->64->64->1")
        self.N = self.w1.size(1) - 1


def critic_forward(cw: CriticWeights, counts, time_rows, rows_per_time=1, *, keep_hidden=False, split_k=False):
    """counts (M, N) fp32 with contiguous last dim (row stride free); time_rows (ceil(M / rows_per_time),).
    split_k (fp32 rows only): spread the first layer of FEW rows over the input columns (tarl_critic_mlp_fwd_splitk)."""
    L = _lib.load()
    u8 = counts.dtype == torch.uint8           # the rollout buffers' count bytes (widened inside the kernel)
    _check_dev(counts, torch.uint8 if u8 else torch.float32, "counts")
    if counts.dim() != 2 or counts.stride(1) != 1 or counts.size(1) != cw.N:
        raise ValueError(f"counts must be (M, {cw.N}) with a contiguous last dim")
    _contig(time_rows, torch.float32, "time_rows")
    M = counts.size(0)
    if time_rows.numel() * rows_per_time < M:
        raise ValueError("time_rows too short")
    value = torch.empty(M, dtype=torch.float32, device=counts.device)
    h1 = torch.empty((M, 64), dtype=torch.float32, device=counts.device) if keep_hidden else None
    h2 = torch.empty((M, 64), dtype=torch.float32, device=counts.device) if keep_hidden else None
    if split_k and not u8:
        scratch = torch.empty(int(L.tarl_critic_splitk_scratch_floats(M, cw.N)), dtype=torch.float32,
                              device=counts.device)
        _lib.check(L.tarl_critic_mlp_fwd_splitk(counts.data_ptr(), counts.stride(0), M, cw.N, time_rows.data_ptr(),
                                                rows_per_time, cw.w1.data_ptr(), cw.b1.data_ptr(), cw.w2.data_ptr(),
                                                cw.b2.data_ptr(), cw.w3.data_ptr(), cw.b3.data_ptr(), scratch.data_ptr(),
                                                value.data_ptr(), _lib.ptr(h1), _lib.ptr(h2), _lib.current_stream()))
        return value, h1, h2
    fn = L.tarl_critic_mlp_fwd_u8 if u8 else L.tarl_critic_mlp_fwd
    _lib.check(fn(counts.data_ptr(), counts.stride(0), M, cw.N, time_rows.data_ptr(), rows_per_time,
                  cw.w1.data_ptr(), cw.b1.data_ptr(), cw.w2.data_ptr(), cw.b2.data_ptr(),
                  cw.w3.data_ptr(), cw.b3.data_ptr(), value.data_ptr(), _lib.ptr(h1), _lib.ptr(h2),
                  _lib.current_stream()))
    return value, h1, h2


def critic_backward(cw: CriticWeights, counts, time_rows, rows_per_time, h1, h2, grad_value, grads):
    """Accumulates into ``grads`` = (gw1, gb1, gw2, gb2, gw3, gb3), tensors shaped like the weights."""
    L = _lib.load()
    M = counts.size(0)
    _contig(grad_value, torch.float32, "grad_value")
    scratch = torch.empty(int(L.tarl_critic_mlp_bwd_scratch_floats(M, cw.N)), dtype=torch.float32, device=counts.device)
    gw1, gb1, gw2, gb2, gw3, gb3 = (_contig(g, torch.float32, "grad") for g in grads)
    _lib.check(L.tarl_critic_mlp_bwd(counts.data_ptr(), counts.stride(0), M, cw.N, time_rows.data_ptr(), rows_per_time,
                                     cw.w1.data_ptr(), cw.w2.data_ptr(), cw.w3.data_ptr(), h1.data_ptr(), h2.data_ptr(),
                                     grad_value.data_ptr(), scratch.data_ptr(), gw1.data_ptr(), gb1.data_ptr(),
                                     gw2.data_ptr(), gb2.data_ptr(), gw3.data_ptr(), gb3.data_ptr(),
                                     _lib.current_stream()))


# ---- PPO --------------------------------------------------------------------------------------------------------------
def gae(reward, value, next_value, *, done=None, terminated=None, gamma=0.99, lmbda=0.95):
    """Time-major (T, B) fp32 tensors -> (advantage, value_target), un-normalised."""
    L = _lib.load()
    for n, t in (("reward", reward), ("value", value), ("next_value", next_value)):
        _contig(t, torch.float32, n)
    T, B = reward.shape
    adv, tgt = torch.empty_like(reward), torch.empty_like(reward)
    _lib.check(L.tarl_gae(reward.data_ptr(), value.data_ptr(), next_value.data_ptr(), _lib.ptr(done),
                          _lib.ptr(terminated), T, B, float(gamma), float(lmbda), adv.data_ptr(), tgt.data_ptr(),
                          _lib.current_stream()))
    return adv, tgt


def advantage_stats(adv):
    L = _lib.load()
    _contig(adv, torch.float32, "advantage")
    partial = torch.empty(512, dtype=torch.float64, device=adv.device)
    stats = torch.empty(3, dtype=torch.float64, device=adv.device)
    _lib.check(L.tarl_advantage_stats(adv.data_ptr(), adv.numel(), partial.data_ptr(), stats.data_ptr(),
                                      _lib.current_stream()))
    return stats


def advantage_normalize_(adv, stats):
    L = _lib.load()
    _lib.check(L.tarl_advantage_normalize(adv.data_ptr(), adv.numel(), stats.data_ptr(), _lib.current_stream()))
    return adv


def ppo_loss(lp_new, lp_old, adv, value, target, entropy, *, clip_epsilon=0.2, entropy_coef=0.01, critic_coef=1.0,
             grad_scale=1.0, want_grads=True):
    """-> (out6, g_lp, g_ent, g_val); out6 = loss_objective, loss_critic, loss_entropy, clip_fraction, kl_approx, ESS."""
    L = _lib.load()
    ts = [_contig(t.reshape(-1), torch.float32, "ppo input") for t in (lp_new, lp_old, adv, value, target, entropy)]
    M = ts[0].numel()
    if any(t.numel() != M for t in ts):
        raise ValueError("ppo_loss inputs must have the same number of elements")
    out = torch.empty(6, dtype=torch.float32, device=ts[0].device)
    gs = [torch.empty(M, dtype=torch.float32, device=ts[0].device) if want_grads else None for _ in range(3)]
    _lib.check(L.tarl_ppo_loss(*(t.data_ptr() for t in ts), M, float(clip_epsilon), float(entropy_coef),
                               float(critic_coef), float(grad_scale), out.data_ptr(), *(_lib.ptr(g) for g in gs),
                               _lib.current_stream()))
    return out, gs[0], gs[1], gs[2]


def adam_step_(param, grad, exp_avg, exp_avg_sq, step, *, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    L = _lib.load()
    for n, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _contig(t, torch.float32, n)
    _lib.check(L.tarl_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                param.numel(), int(step), float(lr), float(beta1), float(beta2), float(eps),
                                float(grad_scale), _lib.current_stream()))
    return param


# ---- fused rollout frame ----------------------------------------------------------------------------------------------
# default number of accumulator banks of a FusedState (measured against 16, 8 and 4);
# TARL_ACC_SLOTS (developer knob, read once): another default for a same-box A/B through bench.py
ACC_SLOTS = int(os.environ.get("TARL_ACC_SLOTS") or 32)


class FusedState:
    """Side buffers of the fused path (``tarl_fused`` in include/tarl_hip.h), ENV-MINOR ([node][env]): the packed dense
    words (hdp, tl, post, sel8), the event-only byte gc8, static node records, the slot-interleaved FIFO store and the
    agent SoA. They hold the state between :func:`fused_pack` and :func:`fused_export`."""

    def __init__(self, plan: Plan, B: int, A: int, device, Nmax: int = 15, env_base: int = 0, acc_slots: int = ACC_SLOTS):
        """``env_base``: global id of environment 0 of this batch — the device noise streams are indexed by
        ``env_base + b`` (include/tarl_hip.h: tarl_fused.env_base), so a shard of a larger batch reproduces the larger
        batch's trajectories. ``acc_slots``: accumulator banks per environment (1 .. 4096); the banks hold exact sums, so
        the number changes the atomics' spread and the insert launch's traffic, never a result."""
        if isinstance(acc_slots, bool) or not isinstance(acc_slots, int) or not 1 <= acc_slots <= 4096:
            raise ValueError(f"acc_slots must be an integer in 1 .. 4096 (got {acc_slots!r})")
        L = _lib.load()
        N, E = plan.num_nodes, plan.num_edges
        if Nmax > 127 or plan.max_out > 126:
            raise _lib.TarlError(f"the fused path needs Nmax <= 127 and out-degree <= 126 (got Nmax={Nmax}, max out-degree="
                                 f"{plan.max_out}); construct SimEngine(..., fused=False) for this graph")
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        # Never zeroed after this: a CLEAN row's dead slots are zero by rule, whatever the store holds (csrc/fused_common.h)
        self.ld_slots = int(L.tarl_fused_slot_floats(Nmax))
        self.slots = torch.zeros((N, B, self.ld_slots), **f32)
        self.hdp = torch.zeros((N, B, 2), **i32)
        self.tl = torch.zeros((N, B), **i32)
        self.gc8 = torch.zeros((N, B), dtype=torch.uint8, device=device)     # pending-garbage code (event-only byte)
        self.post = torch.zeros((N, B), **i32)
        self.st0 = torch.zeros((N, 4), **f32)
        self.sel8 = torch.zeros((N, B), dtype=torch.uint8, device=device)
        self.sel = torch.zeros((N, B), **f32)
        self.node_rec = torch.zeros((N, 36), **i32)          # static records (fused_common.h: NodeRec / InRec)
        self.in_rec = torch.zeros((E + 4, 5), **i32)
        self.out_pad = torch.zeros(E + 4, **i32)
        self.acc_slots = acc_slots      # accumulator banks (spread the per-environment atomics of the N/chunk workgroups)
        self.acc_lp = torch.zeros((self.acc_slots, B), dtype=torch.int64, device=device)
        self.acc_n = torch.zeros((self.acc_slots, B), **f32)
        self.acc_w = torch.zeros((self.acc_slots, B), **f32)
        self.a_origin = torch.zeros((B, A), **i32)
        self.a_dest = torch.zeros((B, A), **i32)
        self.a_dep = torch.zeros((B, A), **f32)
        self.a_status = torch.zeros((B, A), dtype=torch.uint8, device=device)
        self.a_order = torch.zeros((B, A), **i32)
        self.a_dep_sorted = torch.zeros((B, A), **f32)
        self.cur_lo = torch.zeros(B, **i32)
        self.a_win = torch.zeros((B, A, 4), **i32)
        self.a_ins = torch.zeros((B, A), dtype=torch.uint8, device=device)
        self.a_rank = torch.zeros((B, A), **i32)
        self.flags = torch.zeros(1, **i32)
        # the library's device-resident copy of the pointer table below (include/tarl_hip.h: tarl_fused.bufs_dev)
        self.bufs_dev = torch.zeros(int(L.tarl_fused_bufs_bytes()), dtype=torch.uint8, device=device)
        self.order_valid = False
        self.struct = _lib.FusedStruct(self.hdp.data_ptr(), self.tl.data_ptr(), self.gc8.data_ptr(),
                                       self.post.data_ptr(), self.st0.data_ptr(), self.slots.data_ptr(), self.ld_slots,
                                       self.sel8.data_ptr(), self.sel.data_ptr(), self.node_rec.data_ptr(),
                                       self.in_rec.data_ptr(), self.out_pad.data_ptr(),
                                       self.acc_lp.data_ptr(), self.acc_n.data_ptr(), self.acc_w.data_ptr(),
                                       self.a_origin.data_ptr(), self.a_dest.data_ptr(), self.a_dep.data_ptr(),
                                       self.a_status.data_ptr(), None, self.cur_lo.data_ptr(), None, None, None, None,
                                       self.acc_slots, self.flags.data_ptr(), int(env_base), 0.0, 0, self.bufs_dev.data_ptr())
        self.B, self.N, self.A, self.Nmax, self.env_base = B, N, A, Nmax, int(env_base)

    # -- unpacked views of the dense words (tests / debugging; torch plumbing, never on a hot path) ----------------------
    @property
    def count(self):
        return (self.hdp[..., 0] & 127).to(torch.float32)      # (bit 7 of the count byte: HD_DIRTY, csrc/fused_common.h)

    @property
    def head_id(self):
        return ((self.hdp[..., 0] >> 8) & 0xFFFFFF).to(torch.float32)

    @property
    def head_dep(self):
        """Stored head departure; not maintained for an empty row that idled in the last frame (count 0, tl bit 0 clear)."""
        return self.hdp[..., 1].contiguous().view(torch.float32)

    @property
    def tail_id(self):
        return ((self.tl >> 8) & 0xFFFFFF).to(torch.float32)

    @property
    def head_slot_arrival(self):
        """Arrival field of the slot record at every row's ring offset: the head's arrival time where the row holds
        somebody (csrc/fused_common.h: head_arrival)."""
        hoff = ((self.tl >> 1) & 127).long().unsqueeze(-1)
        w = 8 if int(_lib.load().tarl_fused_slot_floats(1)) == 8 else 3    # (developer build -DTARL_SLW=8: 32-byte records)
        arr = self.slots[..., :w * self.Nmax].reshape(self.N, self.B, self.Nmax, w)[..., 1]
        return torch.gather(arr, 2, hoff).squeeze(-1)

    def sort_agents(self, agent_features):
        """Departure-time order of every environment's population (static while DEPARTURE_TIME is not edited): lets the
        insert kernel scan a small window per frame. Plain torch sort — set-up plumbing, not on the per-frame path."""
        dep = agent_features.reshape(self.B, self.A, 9)[:, :, 2]
        order = torch.argsort(dep, dim=1, stable=True)
        self.a_order.copy_(order.to(torch.int32))
        self.a_dep_sorted.copy_(torch.gather(dep, 1, order))
        self.a_rank.scatter_(1, order, torch.arange(self.A, dtype=torch.int32, device=order.device).expand(self.B, -1))
        self.struct.a_order = self.a_order.data_ptr()
        self.struct.a_dep_sorted = self.a_dep_sorted.data_ptr()
        self.struct.a_win = self.a_win.data_ptr()       # filled by tarl_fused_pack
        self.struct.a_ins = self.a_ins.data_ptr()
        self.struct.a_rank = self.a_rank.data_ptr()
        # hint for the insert kernel's geometry: departures per second and environment at the busiest second of the
        # schedule (the never-departing dummy, 48 h, is left out). One histogram over all environments: set-up plumbing.
        real = self.a_dep_sorted[self.a_dep_sorted < 86400.0 * 1.5]
        if real.numel() > 0:
            lo, hi = float(real.min()), float(real.max())
            bins = max(1, min(1 << 20, int(hi - lo) + 1))
            self.struct.due_rate = float(torch.histc(real, bins=bins, min=lo, max=lo + bins).max()) / self.B
        self.order_valid = True

    def check_flags(self):
        """Read the device status word (one host synchronisation) and raise on a domain exit."""
        raise_on_flags(int(self.flags.item()))

    @property
    def ref(self):
        return C.byref(self.struct)


def fused_path_supported(edge_index: torch.Tensor, Nmax: int) -> bool:
    """Can the packed path (FusedState) represent this graph? Nmax <= 127 (count byte + 7-bit ring offset), out-degree
    <= 126 (7-bit rank of the chosen out-edge) and no parallel dual edges (two out-edges of one node to the same target
    have no unique rank: FLAG_AMBIGUOUS_EDGES). Decided on the host from the topology alone, so every rank of a
    data-parallel job takes the same branch; graphs outside it run on the unfused entry points."""
    ei = edge_index.detach().to("cpu", torch.int64)
    if ei.numel() == 0:
        return Nmax <= 127
    n = int(ei.max()) + 1
    key = ei[0] * n + ei[1]
    return bool(Nmax <= 127 and int(torch.bincount(ei[0]).max()) <= 126 and key.unique().numel() == key.numel())


def raise_on_flags(v: int):
    """Turn the bits of a device status word (include/tarl_hip.h: TARL_FLAG_*) into a :class:`TarlError`."""
    if v & _lib.FLAG_COUNT_AT_NMAX:
        raise _lib.TarlError("a FIFO count reached Nmax: the state left the reference's defined domain (its "
                             "DirectionMPNN.update silently overwrites the neighbouring FIFO blocks there and raises "
                             "IndexError only a few steps later, src/direction_mpnn.py:172-191)")
    if v & _lib.FLAG_AMBIGUOUS_EDGES:
        raise _lib.TarlError("two out-edges of one node lead to the same ROAD_INDEX: SELECTED_ROAD has no unique rank "
                             "on this graph; construct SimEngine(..., fused=False)")
    if v & _lib.FLAG_PACK_RANGE:
        raise _lib.TarlError("pack: a FIFO count above 255 or an agent id at / above 2^24 does not fit the packed words")
    if v & _lib.FLAG_CHOICE_OVERFLOW:
        raise _lib.TarlError("more than 65536 nodes drew no action in one block of frames: degenerate policy tables")


def fused_pack(plan: Plan, fs: FusedState, x, Nmax, agent_features, congestion_constant=None, sort_agents=None, *,
               ec: EdgeConst):
    """``ec``: the graph's edge constants (the turn probabilities go into the static in-edge records);
    ``sort_agents``: True = (re)build the departure-time order, None = build it once, False = never."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    if sort_agents or (sort_agents is None and not fs.order_valid):
        fs.sort_agents(agent_features)
    _lib.check(L.tarl_fused_pack(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, _lib.ptr(congestion_constant),
                                 ec.edge_attr.data_ptr(), agent_features.data_ptr(), A, abs_, _lib.current_stream()))


def fused_reset(plan: Plan, fs: FusedState, agent_features):
    """SimulatorEnv._reset on the packed state (no round trip through x)."""
    L = _lib.load()
    A, abs_ = _agents(agent_features, fs.B)
    _lib.check(L.tarl_fused_reset(plan.handle, fs.ref, fs.B, fs.Nmax, agent_features.data_ptr(), A, abs_,
                                  _lib.current_stream()))


def fused_export(plan: Plan, fs: FusedState, x, Nmax, last_step_time):
    """Write the packed state (FIFO columns, NUMBER_OF_AGENT, SELECTED_ROAD) back into ``x`` (reference layout).
    ``last_step_time``: the clock passed to the most recent :func:`fused_frame`."""
    L = _lib.load()
    B, N, bs, ldx = _state(x, Nmax)
    _lib.check(L.tarl_fused_export(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, float(last_step_time),
                                   _lib.current_stream()))


class PolicyTables:
    """Per-edge tables of the live policy's GraphDistribution (plan order), valid until the embedding changes."""

    def __init__(self, plan: Plan, device):
        self.thresholds = torch.empty(plan.num_edges, dtype=torch.float32, device=device)
        self.log_probs = torch.empty(plan.num_edges, dtype=torch.int64, device=device)   # 2^-32 fixed point
        self.entropy = torch.empty(1, dtype=torch.float32, device=device)
        self.base = torch.empty(plan.num_groups + 1, dtype=torch.float64, device=device)


def fused_policy_prepare(plan: Plan, fs: FusedState, emb, temperature=1.0, tables: PolicyTables | None = None):
    L = _lib.load()
    _contig(emb, torch.float32, "emb")
    if tables is None:
        tables = PolicyTables(plan, emb.device)
    _lib.check(L.tarl_fused_policy_prepare(plan.handle, fs.ref, emb.data_ptr(), emb.numel(), float(temperature),
                                           tables.base.data_ptr(), tables.thresholds.data_ptr(),
                                           tables.log_probs.data_ptr(), tables.entropy.data_ptr(),
                                           _lib.current_stream()))
    return tables


def fused_apply_choice(plan: Plan, fs: FusedState, choice):
    """SELECTED_ROAD of the packed state <- an externally sampled action: ``choice`` (B, N) int32 edge ids (-1: none)."""
    L = _lib.load()
    _contig(choice, torch.int32, "choice")
    if tuple(choice.shape) != (fs.B, fs.N):
        raise ValueError("choice must be (B, N)")
    _lib.check(L.tarl_fused_apply_choice(plan.handle, fs.ref, fs.B, choice.data_ptr(), _lib.current_stream()))


def fused_frame(plan: Plan, fs: FusedState, tables: PolicyTables | None, agent_features, ec: EdgeConst, t, *,
                use_cong=True, prev_time=None, uniform=None, policy_seed=0, policy_counter=0, gumbel=None, seed=0,
                counter=0, dtt=None, popped=None, withdrawn=None, scratch=None, choice=None, log_prob=None, entropy=None,
                reward=None, counts=None):
    """One collector frame for all B environments: sample + log_prob + choice phase, core step, withdraw, insert, reward.
    ``tables=None`` skips the choice phase (the action was written by :func:`fused_apply_choice`).
    ``choice`` (N, B) int32 and ``counts`` (N, B) fp32 are ENV-MINOR; ``dtt`` (B, E), ``popped`` / ``withdrawn`` (B, N)
    uint8, ``log_prob`` / ``entropy`` / ``reward`` (B,). Outputs are written into the tensors passed in.
    ``prev_time``: the previous frame's clock (default ``t - 1``; only ``dtt`` reads it)."""
    L = _lib.load()
    B, Nmax = fs.B, fs.Nmax
    A, abs_ = _agents(agent_features, B)
    if scratch is None:
        scratch = torch.empty((B, 2 * A), dtype=torch.int32, device=agent_features.device)
    for n, tt, dt in (("gumbel", gumbel, torch.float32), ("uniform", uniform, torch.float32),
                      ("dtt", dtt, torch.float32), ("reward", reward, torch.float32), ("counts", counts, torch.float32),
                      ("popped", popped, torch.uint8), ("withdrawn", withdrawn, torch.uint8),
                      ("choice", choice, torch.int32), ("log_prob", log_prob, torch.float32),
                      ("entropy", entropy, torch.float32)):
        if tt is not None:
            _contig(tt, dt, n)
    th, lg, en = ((tables.thresholds.data_ptr(), tables.log_probs.data_ptr(), tables.entropy.data_ptr())
                  if tables is not None else (None, None, None))
    _lib.check(L.tarl_fused_frame(plan.handle, fs.ref, B, Nmax, th, lg, en, _lib.ptr(uniform),
                                  int(policy_seed), int(policy_counter), agent_features.data_ptr(), A, abs_,
                                  ec.edge_attr.data_ptr(), ec.log_edge_attr.data_ptr(), ec.log_eps,
                                  1 if use_cong else 0, float(t), float(t - 1 if prev_time is None else prev_time),
                                  _lib.ptr(gumbel), int(seed), int(counter),
                                  _lib.ptr(dtt), _lib.ptr(popped), _lib.ptr(withdrawn), scratch.data_ptr(),
                                  _lib.ptr(choice), _lib.ptr(log_prob), _lib.ptr(entropy), _lib.ptr(reward),
                                  _lib.ptr(counts), _lib.current_stream()))


def _check_rollout_outputs(T, B, N, env_minor, m_env, choice, counts, log_prob, entropy, reward, dtt_node, events, leg):
    nb = (lambda t_, k: (t_, N, k)) if env_minor else (lambda t_, k: (t_, k, N))
    for name, tns, dt, shp in (("choice", choice, torch.uint8, nb(T, B)), ("counts", counts, torch.uint8, nb(T, B)),
                               ("log_prob", log_prob, torch.float32, (T, B)), ("entropy", entropy, torch.float32, (T, B)),
                               ("reward", reward, torch.float32, (T, B)),
                               ("dtt_node", dtt_node, torch.float32, nb(T, m_env)),
                               ("events", events, torch.uint8, nb(T, m_env)), ("leg", leg, torch.int32, (T, B, 2))):
        if tns is not None and (tns.dtype != dt or tuple(tns.shape) != shp or not tns.is_contiguous() or not tns.is_cuda):
            raise ValueError(f"{name} must be a contiguous cuda {dt} tensor of shape {shp}")


def _rollout_args(fs: FusedState, agent_features, times, scratch, prev_time):
    """Common preamble of the multi-frame wrappers -> (library, T, A, a_bstride, prev_time), ``prev_time`` defaulting to
    ``times[0] - 1``."""
    A, abs_ = _agents(agent_features, fs.B)
    _contig(scratch, torch.int32, "scratch")
    return _lib.load(), len(times), A, abs_, float(times[0] - 1 if prev_time is None else prev_time)


def _keep_args(keep, obs_keep, T, N):
    """``keep`` = (ptr, env, slot) of the state-dependent rollouts (see :func:`fused_rollout_policy`) -> the C arguments
    (int64 pointer array, env, slot); Nones without ``keep``."""
    if keep is None:
        return None, None, None
    ptr, kenv, kslot = keep
    if len(ptr) != T + 1 or ptr[0] != 0 or any(b < a for a, b in zip(ptr, ptr[1:])):
        raise ValueError("keep pointer list must be T + 1 non-decreasing offsets starting at 0")
    _contig(kenv, torch.int32, "keep env")
    _contig(kslot, torch.int32, "keep slot")
    _contig(obs_keep, torch.float32, "obs_keep")
    if kenv.numel() < ptr[-1] or kslot.numel() < ptr[-1] or obs_keep.shape[1:] != (N, 16):
        raise ValueError("keep arrays shorter than the pointer list, or obs_keep not (K, N, 16)")
    return (C.c_int64 * (T + 1))(*[int(v) for v in ptr]), kenv, kslot


def _sampler_scratch(L, plan: Plan, fs: FusedState):
    """The per-frame sampler's (B, E) fp32 logits and tarl_graphdist_rollout scratch, one pair per FusedState shared by
    the state-dependent heads."""
    if getattr(fs, "logits_scratch", None) is None:
        fs.logits_scratch = torch.empty((fs.B, plan.num_edges), dtype=torch.float32, device=fs.sel8.device)
        fs.dist_scratch = torch.empty((int(L.tarl_graphdist_rollout_scratch_bytes(plan.handle, fs.B)) + 7) // 8,
                                      dtype=torch.float64, device=fs.sel8.device)
    return fs.logits_scratch.data_ptr(), fs.dist_scratch.data_ptr()


def fused_rollout(plan: Plan, fs: FusedState, tables: PolicyTables, agent_features, ec: EdgeConst, times, *, use_cong,
                  policy_seed, policy_counter0, seed, counter0, scratch, prev_time=None, choice=None, log_prob=None,
                  entropy=None, reward=None, counts=None, metrics_envs=0, dtt_node=None, events=None, leg=None):
    """``T = len(times)`` frames in one foreign call (tarl_fused_rollout). ``choice`` (T,N,B) uint8 (rank of the chosen
    out-edge, bit 7: none), ``counts`` (T,N,B) uint8 (counts[t] = per-node counts after frame t), ``log_prob`` / ``entropy``
    / ``reward`` (T,B) fp32, ``leg`` (T,B,2) int32, ``dtt_node`` (T,N,metrics_envs) fp32, ``events`` (T,N,metrics_envs)
    uint8 — all optional, contiguous device tensors. Frame t uses policy counter ``policy_counter0 + t`` and noise counter
    ``counter0 + t``."""
    L, T, A, abs_, prev = _rollout_args(fs, agent_features, times, scratch, prev_time)
    _check_rollout_outputs(T, fs.B, fs.N, True, metrics_envs, choice, counts, log_prob, entropy, reward, dtt_node, events, leg)
    if getattr(fs, "acc_scratch", None) is None:     # double buffers of the merged insert + choice launch
        fs.acc_scratch = torch.zeros_like(fs.acc_lp)
    if choice is None and getattr(fs, "sel_scratch", None) is None:
        fs.sel_scratch = torch.empty_like(fs.sel8)
    need = int(L.tarl_fused_rollout_scratch_ints(plan.handle, T, fs.B))
    if getattr(fs, "choice_scratch", None) is None or fs.choice_scratch.numel() < need:
        # unresolved-draw list + packed policy records + per-(frame, env) log-prob accumulators of the side stream
        fs.choice_scratch = torch.zeros(need, dtype=torch.int32, device=fs.sel8.device)
    tarr = (C.c_float * T)(*[float(t) for t in times])
    _lib.check(L.tarl_fused_rollout(plan.handle, fs.ref, fs.B, fs.Nmax, T, tarr, prev, tables.thresholds.data_ptr(),
                                    tables.log_probs.data_ptr(), tables.entropy.data_ptr(), int(policy_seed),
                                    int(policy_counter0), agent_features.data_ptr(), A, abs_, ec.edge_attr.data_ptr(),
                                    ec.log_edge_attr.data_ptr(), ec.log_eps, 1 if use_cong else 0, int(seed),
                                    int(counter0), scratch.data_ptr(),
                                    _lib.ptr(getattr(fs, "sel_scratch", None)) if choice is None else None,
                                    fs.acc_scratch.data_ptr(), fs.choice_scratch.data_ptr(), _lib.ptr(choice),
                                    _lib.ptr(log_prob), _lib.ptr(entropy),
                                    _lib.ptr(reward), _lib.ptr(counts), int(metrics_envs), _lib.ptr(dtt_node),
                                    _lib.ptr(events), _lib.ptr(leg), _lib.current_stream()))


def _head_rollout(entry, plan: Plan, fs: FusedState, x, agent_features, ec: EdgeConst, times, head, *, use_cong,
                  temperature, policy_seed, policy_counter0, seed, counter0, scratch, prev_time, keep, obs_keep, choice8,
                  log_prob, reward, counts, obs_scratch=False, head_scratch=(), logs=None):
    """The one body of the state-dependent rollouts (csrc/rollout_heads.h): checks what they share and calls ``entry``
    with the common head of the C argument list, the head's own arguments ``head``, the sampler arguments and keep list,
    the scratch buffers (``obs_scratch``: the lazily created (B, N, 16) observation buffer, then ``head_scratch``), the
    outputs and — for the entry point that has them — the per-step ``logs`` (metrics_envs, dtt_node, events, leg)."""
    L, T, A, abs_, prev = _rollout_args(fs, agent_features, times, scratch, prev_time)
    B, N = fs.B, fs.N
    _, _, bs, ldx = _state(x, fs.Nmax)
    m_env, dtt_node, events, leg = logs or (0, None, None, None)
    _check_rollout_outputs(T, B, N, True, m_env, None, counts, log_prob, None, reward, dtt_node, events, leg)
    _check_rollout_outputs(T, B, N, False, m_env, choice8, None, None, None, None, None, None, None)
    if obs_scratch and getattr(fs, "obs_scratch", None) is None:
        fs.obs_scratch = torch.empty((B, N, 16), dtype=torch.float32, device=fs.sel8.device)
    logits_scratch, dist_scratch = _sampler_scratch(L, plan, fs)
    kptr, kenv, kslot = _keep_args(keep, obs_keep, T, N)
    tarr = (C.c_float * T)(*[float(t) for t in times])
    _lib.check(getattr(L, entry)(
        plan.handle, fs.ref, B, fs.Nmax, T, tarr, prev, x.data_ptr(), bs, ldx, agent_features.data_ptr(), A, abs_,
        ec.edge_attr.data_ptr(), ec.log_edge_attr.data_ptr(), ec.log_eps, 1 if use_cong else 0, *head, float(temperature),
        int(policy_seed), int(policy_counter0), int(seed), int(counter0), kptr, _lib.ptr(kenv), _lib.ptr(kslot),
        _lib.ptr(obs_keep), *((fs.obs_scratch.data_ptr(),) if obs_scratch else ()), *head_scratch, logits_scratch,
        dist_scratch, scratch.data_ptr(), _lib.ptr(choice8), _lib.ptr(log_prob), _lib.ptr(reward), _lib.ptr(counts),
        *((int(m_env), _lib.ptr(dtt_node), _lib.ptr(events), _lib.ptr(leg)) if logs else ()), _lib.current_stream()))


def fused_rollout_policy(plan: Plan, fs: FusedState, x, agent_features, ec: EdgeConst, w: EdgeMlpWeights, times, *,
                         use_cong, bf16=False, temperature, policy_seed, policy_counter0, seed, counter0, scratch,
                         prev_time=None, keep=None, obs_keep=None, choice8=None, log_prob=None, reward=None, counts=None,
                         metrics_envs=0, dtt_node=None, events=None, leg=None, precision=None):
    """``T = len(times)`` frames under the per-edge MLP policy in one foreign call (tarl_fused_rollout_policy).
    ``keep`` = (ptr, env, slot): ``ptr`` a Python list of T + 1 offsets, ``env`` / ``slot`` int32 device tensors — the
    observations (frame t, environment env[j]) for ptr[t] <= j < ptr[t + 1] are copied to ``obs_keep[slot[j]]``
    ((K, N, 16) fp32). ``choice8`` (T, B, N) uint8 ENV-MAJOR rank bytes; ``counts`` (T, N, B) uint8 env-minor; the
    other outputs as :func:`fused_rollout`."""
    head = (*w.ptrs(), {"fp32": 0, "bf16": 1, "x3": 2}[_edge_mlp_precision(bf16, precision)])
    _head_rollout("tarl_fused_rollout_policy", plan, fs, x, agent_features, ec, times, head, use_cong=use_cong,
                  temperature=temperature, policy_seed=policy_seed, policy_counter0=policy_counter0, seed=seed,
                  counter0=counter0, scratch=scratch, prev_time=prev_time, keep=keep, obs_keep=obs_keep, choice8=choice8,
                  log_prob=log_prob, reward=reward, counts=counts, obs_scratch=True,
                  logs=(metrics_envs, dtt_node, events, leg))


# ---- shortest-path prior head (policy_head = "embedding_dijkstra", csrc/prior.hip) ------------------------------------------
def prior_dest_table_bytes(plan: Plan, num_dests: int):
    """-> (table bytes, scratch bytes) of :func:`prior_dest_table` for ``num_dests`` destinations."""
    L = _lib.load()
    return 4 * plan.num_nodes * int(num_dests), int(L.tarl_prior_dest_table_scratch_bytes(plan.handle, int(num_dests)))


def prior_dest_table(plan: Plan, weights, dests):
    """The per-destination distance table of the prior head (tarl_prior_dest_table): ``weights`` (E,) fp32 in original edge
    order, ``dests`` (D,) int64 -> fp32 (N, D), table[u, j] = the fp32 rounding of the fp64 shortest-path distance
    u -> dests[j] (+inf: unreachable, 0 at the destination). Column j equals the all-pairs ``dist[:, dests[j]]`` wherever
    :func:`destination_trees`' exactness condition holds."""
    D = _tree_check(plan, weights, torch.float32, dests, "dests")
    L, need, scratch = _tree_scratch(plan, weights, D, "tarl_prior_dest_table_scratch_bytes")
    N = plan.num_nodes
    table = torch.empty((N, D), dtype=torch.float32, device=weights.device)
    _lib.check(L.tarl_prior_dest_table(plan.handle, weights.data_ptr(), dests.data_ptr(), D, _lib.ptr(scratch), need,
                                       table.data_ptr(), _lib.current_stream()))
    return table


def _prior_args(plan: Plan, emb, table, prior_weight, dest_slot):
    """-> (weight, the table's trailing C arguments, the entry-point suffix). ``dest_slot`` None: ``table`` is the (N, N)
    all-pairs table; else ``table`` is the (N, D) per-destination table and ``dest_slot`` (N,) int32 its column map."""
    _contig(emb, torch.float32, "emb")
    _contig(table, torch.float32, "prior_table")
    N = plan.num_nodes
    w = float(prior_weight)
    if not (0.0 <= w < float("inf")):
        raise ValueError("prior_weight must be finite and >= 0")
    if dest_slot is None:
        if tuple(table.shape) != (N, N):
            raise ValueError(f"prior_table must be the ({N}, {N}) all-pairs distance table of the plan's graph")
        return w, (table.data_ptr(), table.size(0)), ""
    _contig(dest_slot, torch.int32, "dest_slot")
    if table.dim() != 2 or table.size(0) != N or table.size(1) < 1 or tuple(dest_slot.shape) != (N,):
        raise ValueError(f"a per-destination prior_table must be ({N}, D >= 1) with a ({N},) dest_slot, got "
                         f"{tuple(table.shape)} and {tuple(dest_slot.shape)}")
    return w, (table.data_ptr(), table.size(1), dest_slot.data_ptr()), "_dest"


def policy_prior_logits(plan: Plan, obs16, emb, table, prior_weight=1.0, dest_slot=None):
    """logit[m, e] = emb[ROAD_INDEX(dst)] + prior_weight * ((-table[dst, dest(src)]) - time_travel(dst)) from observations
    ``obs16`` (M, N, 16) (the :func:`policy_obs16` layout) -> (M, E). ``table``: (N, N) fp32 free-flow distances
    (MPNNPolicyNet.dist_matrix), or with ``dest_slot`` the (N, D) table of :func:`prior_dest_table`, read as
    table[dst, dest_slot[dest]] (tarl_policy_prior_logits_dest). Unreachable candidates, and destinations without a column,
    carry the finite sentinel -1e20 (see include/tarl_hip.h)."""
    L = _lib.load()
    w, targs, sfx = _prior_args(plan, emb, table, prior_weight, dest_slot)
    _contig(obs16, torch.float32, "obs16")
    if obs16.dim() != 3 or tuple(obs16.shape[1:]) != (plan.num_nodes, 16):
        raise ValueError(f"obs16 must be (M, {plan.num_nodes}, 16)")
    M = obs16.size(0)
    logits = torch.empty((M, plan.num_edges), dtype=torch.float32, device=obs16.device)
    fn = getattr(L, "tarl_policy_prior_logits" + sfx)
    _lib.check(fn(plan.handle, obs16.data_ptr(), M, emb.data_ptr(), emb.numel(), *targs, w, logits.data_ptr(),
                  _lib.current_stream()))
    return logits


def fused_prior_logits(plan: Plan, fs, x, Nmax, agent_features, emb, table, prior_weight=1.0, out=None, dest_slot=None):
    """The same logits from the packed state of the fused engine: (B, E), no observation materialised (``dest_slot``: as
    :func:`policy_prior_logits`)."""
    L = _lib.load()
    w, targs, sfx = _prior_args(plan, emb, table, prior_weight, dest_slot)
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    logits = out if out is not None else torch.empty((B, plan.num_edges), dtype=torch.float32, device=x.device)
    _contig(logits, torch.float32, "logits")
    if tuple(logits.shape) != (B, plan.num_edges):
        raise ValueError(f"logits must be ({B}, {plan.num_edges})")
    fn = getattr(L, "tarl_fused_prior_logits" + sfx)
    _lib.check(fn(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, agent_features.data_ptr(), A, abs_, emb.data_ptr(),
                  emb.numel(), *targs, w, logits.data_ptr(), _lib.current_stream()))
    return logits


def fused_rollout_prior(plan: Plan, fs: FusedState, x, agent_features, ec: EdgeConst, emb, table, times, *, prior_weight,
                        use_cong, temperature, policy_seed, policy_counter0, seed, counter0, scratch, prev_time=None,
                        keep=None, obs_keep=None, choice8=None, log_prob=None, reward=None, counts=None, dest_slot=None):
    """``T = len(times)`` frames under the prior head in one foreign call (tarl_fused_rollout_prior, or
    tarl_fused_rollout_prior_dest with ``dest_slot``: as :func:`policy_prior_logits`). ``keep`` / ``obs_keep`` /
    ``choice8`` / ``counts`` as :func:`fused_rollout_policy`; ``log_prob`` / ``reward`` (T, B)."""
    w, targs, sfx = _prior_args(plan, emb, table, prior_weight, dest_slot)
    _head_rollout("tarl_fused_rollout_prior" + sfx, plan, fs, x, agent_features, ec, times,
                  (emb.data_ptr(), emb.numel(), *targs, w), use_cong=use_cong, temperature=temperature,
                  policy_seed=policy_seed, policy_counter0=policy_counter0, seed=seed, counter0=counter0, scratch=scratch,
                  prev_time=prev_time, keep=keep, obs_keep=obs_keep, choice8=choice8, log_prob=log_prob, reward=reward,
                  counts=counts)


# ---- goal-conditioned MLP head (policy_head = "goal_mlp", csrc/goal_mlp.hip) -------------------------------------------------
GOAL_MLP_FEATURES, GOAL_MLP_HIDDEN, GOAL_MLP_PARAMS = 8, 16, 161
# state-dict keys of MPNNPolicyNet's ``goal_mlp`` submodule in the kernels' order (offsets 0, 128, 144, 160)
GOAL_MLP_KEYS = ("goal_mlp.0.weight", "goal_mlp.0.bias", "goal_mlp.2.weight", "goal_mlp.2.bias")


class GoalMlpWeights:
    """The 161 parameters of the goal-conditioned head as ONE flat fp32 device tensor in kernel order: ``goal_mlp.0.weight``
    (16, 8), ``goal_mlp.0.bias`` (16,), ``goal_mlp.2.weight`` (1, 16), ``goal_mlp.2.bias`` (1,). Built from the four tensors
    (copied into a flat buffer) or, with ``flat=``, around an existing (161,) tensor (a view of a flat parameter buffer: no
    copy, updates are seen)."""

    def __init__(self, w1=None, b1=None, w2=None, b2=None, *, flat=None):
        if flat is None:
            parts = [(w1, (GOAL_MLP_HIDDEN, GOAL_MLP_FEATURES), "w1"), (b1, (GOAL_MLP_HIDDEN,), "b1"),
                     (w2, (1, GOAL_MLP_HIDDEN), "w2"), (b2, (1,), "b2")]
            for t, shp, name in parts:
                ok = isinstance(t, torch.Tensor) and (tuple(t.shape) == shp or (name == "w2" and tuple(t.shape) == shp[1:]))
                if not ok:
                    raise ValueError(f"goal_mlp must be 8 -> 16 -> 1: {name} must be {shp}")
            flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for t, _, _ in parts])
        self.flat = _contig(flat.detach(), torch.float32, "goal_mlp weights")
        if tuple(self.flat.shape) != (GOAL_MLP_PARAMS,):
            raise ValueError(f"goal_mlp weights must be ({GOAL_MLP_PARAMS},) floats")

    @property
    def w1(self):
        return self.flat[:128].view(GOAL_MLP_HIDDEN, GOAL_MLP_FEATURES)

    @property
    def b1(self):
        return self.flat[128:144]

    @property
    def w2(self):
        return self.flat[144:160]

    @property
    def b2(self):
        return self.flat[160:161]


# ---- the learned per-decision critic (csrc/decision_critic.hip; NOT reference semantics) --------------------------
DECISION_CRITIC_FEATURES, DECISION_CRITIC_PARAMS = 8, 161


class DecisionCriticWeights(GoalMlpWeights):
    """The 161 parameters of the per-decision critic (8 -> 16 -> 1) as ONE flat fp32 device tensor, the layout of
    :class:`GoalMlpWeights`: built from the four tensors w1 (16, 8), b1 (16,), w2 (1, 16), b2 (1,), or with ``flat=``
    around a (161,) view of a flat parameter buffer."""


def decision_critic_init(device="cpu", seed=0):
    """-> [w1 (16, 8), b1 (16,), w2 (1, 16), b2 (1,)] fp32: W1 uniform in (-0.1, 0.1), everything else 0. With the last
    layer at zero the critic's value is 0, so the first update's advantages are those of the free-flow baseline."""
    g = torch.Generator().manual_seed(int(seed))
    w1 = (torch.rand((16, 8), generator=g, dtype=torch.float64) * 0.2 - 0.1).to(torch.float32)
    return [t.to(device) for t in (w1, torch.zeros(16), torch.zeros(1, 16), torch.zeros(1))]


def _critic_inputs(plan, obs16, head, frames_left, dist, dest_slot, timestep):
    N = plan.num_nodes
    _contig(obs16, torch.float32, "obs16")
    if obs16.dim() != 3 or obs16.size(1) != N or obs16.size(2) != 16 or obs16.size(0) < 1:
        raise ValueError(f"obs16 must be (M, {N}, 16) with M >= 1, got {tuple(obs16.shape)}")
    M = obs16.size(0)
    _rows_n(head, torch.int32, N, "head", M)
    _row_list(frames_left, M, "frames_left")
    _contig(dist, torch.float64, "dist")
    _contig(dest_slot, torch.int32, "dest_slot")
    if dist.dim() != 2 or dist.size(1) != N or dist.size(0) < 1 or tuple(dest_slot.shape) != (N,):
        raise ValueError(f"dist must be (D, {N}) with D >= 1 and dest_slot ({N},), got {tuple(dist.shape)} and "
                         f"{tuple(dest_slot.shape)}")
    if not float(timestep) > 0.0:
        raise ValueError("timestep must be positive")
    return M, (plan.handle, obs16.data_ptr(), M, head.data_ptr(), frames_left.data_ptr(), dist.data_ptr(),
               dest_slot.data_ptr(), dist.size(0), float(timestep))


def _critic_net(weights, delay_scale, adv_raw, N, M):
    if not isinstance(weights, GoalMlpWeights):
        raise ValueError("weights must be ops.DecisionCriticWeights")
    if not (math.isfinite(float(delay_scale)) and float(delay_scale) > 0.0):
        raise ValueError("delay_scale must be positive and finite")
    _rows_n(adv_raw, torch.float32, N, "adv_raw", M)


def decision_critic_features(plan: Plan, obs16, head, frames_left, dist, dest_slot, *, timestep, out=None):
    """-> fp32 (M, N, 8): the critic's features of every (kept row, road), zeros where ``head <= 0``
    (tarl_decision_critic_features; the test hook the restatement is anchored to). ``obs16`` fp32 (M, N, 16), ``head`` int32
    (M, N), ``frames_left`` int32 (M,), ``dist`` float64 (D, N) and ``dest_slot`` int32 (N,) of :func:`decision_advantage`."""
    M, args = _critic_inputs(plan, obs16, head, frames_left, dist, dest_slot, timestep)
    if out is None:
        out = torch.empty((M, plan.num_nodes, DECISION_CRITIC_FEATURES), dtype=torch.float32, device=obs16.device)
    _contig(out, torch.float32, "out")
    if tuple(out.shape) != (M, plan.num_nodes, DECISION_CRITIC_FEATURES):
        raise ValueError(f"out must be ({M}, {plan.num_nodes}, 8), got {tuple(out.shape)}")
    _lib.check(_lib.load().tarl_decision_critic_features(*args, out.data_ptr(), _lib.current_stream()))
    return out


def decision_critic_forward(plan: Plan, obs16, head, frames_left, dist, dest_slot, weights, adv_raw, *, timestep,
                            delay_scale=16.0, value=None, adv_out=None, want_adv=True):
    """-> (value, adv_dec), fp32 (M, N) each (tarl_decision_critic_fwd): ``value`` the critic's estimate of the delay beyond
    free flow in units of ``delay_scale`` frames, ``adv_dec = adv_raw + delay_scale * value``; zeros where ``head <= 0``.
    ``want_adv=False`` -> (value, None)."""
    M, args = _critic_inputs(plan, obs16, head, frames_left, dist, dest_slot, timestep)
    N = plan.num_nodes
    _critic_net(weights, delay_scale, adv_raw, N, M)
    if value is None:
        value = torch.empty((M, N), dtype=torch.float32, device=obs16.device)
    _rows_n(value, torch.float32, N, "value", M)
    if want_adv and adv_out is None:
        adv_out = torch.empty((M, N), dtype=torch.float32, device=obs16.device)
    if adv_out is not None:
        _rows_n(adv_out, torch.float32, N, "adv_out", M)
    ptrs = {adv_raw.data_ptr(), value.data_ptr()} | ({adv_out.data_ptr()} if adv_out is not None else set())
    if len(ptrs) != (3 if adv_out is not None else 2):
        raise ValueError("value and adv_out may alias neither adv_raw nor each other")
    _lib.check(_lib.load().tarl_decision_critic_fwd(*args, weights.flat.data_ptr(), float(delay_scale), adv_raw.data_ptr(),
                                                    value.data_ptr(), _lib.ptr(adv_out), _lib.current_stream()))
    return value, adv_out


def decision_critic_scratch_bytes(plan: Plan, M) -> int:
    """Bytes of scratch of :func:`decision_critic_loss` for M rows: 40 per (row, tile of 256 roads) pair and 161 floats per
    run of ceil(pairs / 1024) pairs — the rule of the library, which is asked and must agree."""
    pairs = int(M) * max(1, -(-plan.num_nodes // 256))
    per = -(-pairs // 1024)
    want = pairs * 40 + (-(-pairs // per)) * DECISION_CRITIC_PARAMS * 4
    need = int(_lib.load().tarl_decision_critic_loss_scratch_bytes(plan.handle, int(M)))
    if need < 0:
        raise _lib.TarlError("tarl_decision_critic_loss_scratch_bytes refused the sizes")
    if need != want:
        raise _lib.TarlError(f"the scratch of tarl_decision_critic_loss is {need} bytes, the shapes say {want}")
    return need


def decision_critic_loss(plan: Plan, obs16, head, frames_left, dist, dest_slot, weights, adv_raw, n_live, *, timestep,
                         delay_scale=16.0, coef=1.0, grad_scale=1.0, grads=None, scratch=None):
    """The critic's smooth-L1 loss over the live decisions of a minibatch, forward and backward (tarl_decision_critic_loss).
    -> float64 (M, 5) = per row {sum of the losses, live decisions, sum of y, sum of y^2, sum of (y - value)^2} with the
    target y = -adv_raw / delay_scale. ``grads`` fp32 (161,) (optional): the gradient of ``grad_scale * coef / L`` times the
    summed loss is ADDED, L = ``n_live`` (int32 (1,) on the device). ``scratch``: at least
    :func:`decision_critic_scratch_bytes` bytes; a shorter one is refused."""
    M, args = _critic_inputs(plan, obs16, head, frames_left, dist, dest_slot, timestep)
    _critic_net(weights, delay_scale, adv_raw, plan.num_nodes, M)
    need = decision_critic_scratch_bytes(plan, M)
    if scratch is not None and scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch holds {scratch.numel() * scratch.element_size()} bytes, tarl_decision_critic_loss needs "
                         f"{need}")
    _contig(n_live, torch.int32, "n_live")
    if n_live.numel() != 1:
        raise ValueError("n_live must hold one int32")
    if not (math.isfinite(float(coef)) and float(coef) >= 0.0):
        raise ValueError("coef must be finite and >= 0")
    if grads is not None:
        _contig(grads, torch.float32, "grads")
        if tuple(grads.shape) != (DECISION_CRITIC_PARAMS,):
            raise ValueError(f"grads must be ({DECISION_CRITIC_PARAMS},), got {tuple(grads.shape)}")
    if scratch is None:
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=obs16.device)
    elif not scratch.is_cuda or not scratch.is_contiguous():
        raise _lib.TarlError("scratch must be a contiguous tensor on the GPU")
    out5 = torch.empty((M, 5), dtype=torch.float64, device=obs16.device)
    _lib.check(_lib.load().tarl_decision_critic_loss(*args, weights.flat.data_ptr(), float(delay_scale), adv_raw.data_ptr(),
                                                     n_live.data_ptr(), float(coef), float(grad_scale), out5.data_ptr(),
                                                     _lib.ptr(grads), scratch.data_ptr(), _lib.current_stream()))
    return out5


def goal_time_scale(x_static) -> float:
    """``time_scale`` of the goal-conditioned head: the mean FREE_FLOW over the roads of ``x_static`` (the (N, 7) static
    columns, or any (..., N, >= 3) tensor whose column 2 is FREE_FLOW: the first environment speaks for all), computed in
    float64 and rounded to fp32. Must be finite and > 0."""
    t = x_static
    while t.dim() > 2:
        t = t[0]
    if t.dim() != 2 or t.size(1) < 3 or t.size(0) < 1:
        raise ValueError("x_static must be (N, >= 3) with FREE_FLOW in column 2")
    s = float(torch.tensor(float(t[:, 2].detach().to("cpu", torch.float64).mean()), dtype=torch.float32))
    if not (0.0 < s < float("inf")):
        raise ValueError(f"the mean FREE_FLOW must be finite and > 0, got {s}")
    return s


def _goal_args(plan: Plan, table, time_scale, dest_slot):
    """-> (the table's C arguments ``table, table_cols, dest_slot``, the fp32 ``time_scale``); the shapes as
    :func:`_prior_args`."""
    _contig(table, torch.float32, "prior_table")
    N = plan.num_nodes
    s = float(time_scale)
    if not (0.0 < s < float("inf")):
        raise ValueError("time_scale must be finite and > 0")
    if dest_slot is None:
        if tuple(table.shape) != (N, N):
            raise ValueError(f"prior_table must be the ({N}, {N}) all-pairs distance table of the plan's graph")
        return (table.data_ptr(), N, None), s
    _contig(dest_slot, torch.int32, "dest_slot")
    if table.dim() != 2 or table.size(0) != N or table.size(1) < 1 or tuple(dest_slot.shape) != (N,):
        raise ValueError(f"a per-destination prior_table must be ({N}, D >= 1) with a ({N},) dest_slot, got "
                         f"{tuple(table.shape)} and {tuple(dest_slot.shape)}")
    return (table.data_ptr(), table.size(1), dest_slot.data_ptr()), s


def _goal_obs(plan: Plan, obs16):
    _contig(obs16, torch.float32, "obs16")
    if obs16.dim() != 3 or tuple(obs16.shape[1:]) != (plan.num_nodes, 16) or obs16.size(0) < 1:
        raise ValueError(f"obs16 must be (M >= 1, {plan.num_nodes}, 16)")
    return obs16.size(0)


def _goal_weights(w):
    if not isinstance(w, GoalMlpWeights):
        raise ValueError("weights must be ops.GoalMlpWeights")
    return w.flat


def policy_goal_features(plan: Plan, obs16, table, time_scale, dest_slot=None, out=None):
    """The eight destination-relative features of every (sample, edge) from observations ``obs16`` (M, N, 16) -> (M, E, 8)
    fp32 in original edge order (tarl_policy_goal_features; the rule: include/tarl_hip.h). ``table`` / ``dest_slot`` as
    :func:`policy_prior_logits`."""
    L = _lib.load()
    targs, s = _goal_args(plan, table, time_scale, dest_slot)
    M = _goal_obs(plan, obs16)
    shp = (M, plan.num_edges, GOAL_MLP_FEATURES)
    feats = out if out is not None else torch.empty(shp, dtype=torch.float32, device=obs16.device)
    _contig(feats, torch.float32, "feats")
    if tuple(feats.shape) != shp:
        raise ValueError(f"feats must be {shp}")
    _lib.check(L.tarl_policy_goal_features(plan.handle, obs16.data_ptr(), M, *targs, s, feats.data_ptr(),
                                           _lib.current_stream()))
    return feats


def policy_goal_mlp(plan: Plan, obs16, w: GoalMlpWeights, table, time_scale, dest_slot=None, out=None):
    """obs16 (M, N, 16) -> logits (M, E) of the goal-conditioned head (tarl_policy_goal_mlp_fwd); an unreachable edge
    carries exactly -1e20."""
    L = _lib.load()
    targs, s = _goal_args(plan, table, time_scale, dest_slot)
    flat = _goal_weights(w)
    M = _goal_obs(plan, obs16)
    logits = out if out is not None else torch.empty((M, plan.num_edges), dtype=torch.float32, device=obs16.device)
    _contig(logits, torch.float32, "logits")
    if tuple(logits.shape) != (M, plan.num_edges):
        raise ValueError(f"logits must be ({M}, {plan.num_edges})")
    _lib.check(L.tarl_policy_goal_mlp_fwd(plan.handle, obs16.data_ptr(), M, *targs, s, flat.data_ptr(), logits.data_ptr(),
                                          _lib.current_stream()))
    return logits


GOAL_MLP_BWD_BLOCK, GOAL_MLP_BWD_MAX_PARTS = 256, 1024


def goal_mlp_bwd_scratch_floats(plan: Plan, M: int) -> int:
    """fp32 elements of device scratch one :func:`policy_goal_mlp_bwd` call over ``M`` samples needs, from the shapes alone
    (the rule of tarl_policy_goal_mlp_bwd_scratch_floats: 161 per partition of the (sample, edge) pairs)."""
    M, E = int(M), plan.num_edges
    if M < 1:
        raise ValueError("M must be >= 1")
    if E == 0:
        return 0
    tiles = -(-M * E // GOAL_MLP_BWD_BLOCK)
    per = -(-tiles // GOAL_MLP_BWD_MAX_PARTS)
    return -(-tiles // per) * GOAL_MLP_PARAMS


def policy_goal_mlp_bwd(plan: Plan, obs16, w: GoalMlpWeights, table, time_scale, grad_logits, grads, dest_slot=None,
                        scratch=None):
    """ACCUMULATES (+=) the gradient of sum(grad_logits * logits) into ``grads``, a (161,) fp32 contiguous tensor in the
    order of ``GoalMlpWeights.flat``. ``scratch``: an fp32 contiguous device tensor of at least
    ``goal_mlp_bwd_scratch_floats(plan, M)`` elements (ValueError otherwise, decided from the shapes before any call;
    allocated per call when None). Deterministic: two calls give the same bits."""
    L = _lib.load()
    targs, s = _goal_args(plan, table, time_scale, dest_slot)
    flat = _goal_weights(w)
    M = _goal_obs(plan, obs16)
    gl = _contig(grad_logits, torch.float32, "grad_logits")
    if gl.numel() != M * plan.num_edges:
        raise ValueError("grad_logits must be (M, E)")
    _contig(grads, torch.float32, "grads")
    if tuple(grads.shape) != (GOAL_MLP_PARAMS,):
        raise ValueError(f"grads must be ({GOAL_MLP_PARAMS},)")
    need = goal_mlp_bwd_scratch_floats(plan, M)
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.float32, device=obs16.device)
    elif (not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.float32 or not scratch.is_contiguous()
          or scratch.device != obs16.device or scratch.numel() < need):
        raise ValueError(f"scratch must be a contiguous fp32 tensor on {obs16.device} of at least {need} elements")
    if int(L.tarl_policy_goal_mlp_bwd_scratch_floats(plan.handle, M)) != need:
        raise _lib.TarlError("goal_mlp_bwd_scratch_floats disagrees with the library")
    _lib.check(L.tarl_policy_goal_mlp_bwd(plan.handle, obs16.data_ptr(), M, *targs, s, flat.data_ptr(), gl.data_ptr(),
                                          grads.data_ptr(), scratch.data_ptr(), _lib.current_stream()))
    return grads


def fused_goal_mlp_logits(plan: Plan, fs, x, Nmax, agent_features, w: GoalMlpWeights, table, time_scale, dest_slot=None,
                          out=None):
    """The same logits from the packed state of the fused engine: (B, E), no observation materialised
    (tarl_fused_goal_mlp_logits; bit-identical to :func:`policy_goal_mlp` on :func:`fused_obs16` of that state)."""
    L = _lib.load()
    targs, s = _goal_args(plan, table, time_scale, dest_slot)
    flat = _goal_weights(w)
    B, N, bs, ldx = _state(x, Nmax)
    A, abs_ = _agents(agent_features, B)
    logits = out if out is not None else torch.empty((B, plan.num_edges), dtype=torch.float32, device=x.device)
    _contig(logits, torch.float32, "logits")
    if tuple(logits.shape) != (B, plan.num_edges):
        raise ValueError(f"logits must be ({B}, {plan.num_edges})")
    _lib.check(L.tarl_fused_goal_mlp_logits(plan.handle, fs.ref, x.data_ptr(), B, bs, ldx, Nmax, agent_features.data_ptr(), A,
                                            abs_, *targs, s, flat.data_ptr(), logits.data_ptr(), _lib.current_stream()))
    return logits


def fused_rollout_goal(plan: Plan, fs: FusedState, x, agent_features, ec: EdgeConst, w: GoalMlpWeights, table, time_scale,
                       times, *, use_cong, temperature, policy_seed, policy_counter0, seed, counter0, scratch,
                       prev_time=None, keep=None, obs_keep=None, choice8=None, log_prob=None, reward=None, counts=None,
                       dest_slot=None):
    """``T = len(times)`` frames under the goal-conditioned head in one foreign call (tarl_fused_rollout_goal). Buffers as
    :func:`fused_rollout_prior`."""
    targs, s = _goal_args(plan, table, time_scale, dest_slot)
    flat = _goal_weights(w)
    _head_rollout("tarl_fused_rollout_goal", plan, fs, x, agent_features, ec, times, (*targs, s, flat.data_ptr()),
                  use_cong=use_cong, temperature=temperature, policy_seed=policy_seed, policy_counter0=policy_counter0,
                  seed=seed, counter0=counter0, scratch=scratch, prev_time=prev_time, keep=keep, obs_keep=obs_keep,
                  choice8=choice8, log_prob=log_prob, reward=reward, counts=counts)


# ---- graph-transformer head (policy_head = "graph_transformer", csrc/gt_policy.hip) ------------------------------------------
# state-dict keys of GraphTransformerNet in the kernels' order: the trainable tensors that reach the logits, then the
# BatchNorm running statistics (include/tarl_hip.h)
_GT_EDGE = ("WE.weight", "WE.bias", "WOe.weight", "WOe.bias", "norm1e.weight", "norm1e.bias", "ffn_e.mlp.0.weight",
            "ffn_e.mlp.0.bias", "ffn_e.mlp.3.weight", "ffn_e.mlp.3.bias", "norm2e.weight", "norm2e.bias")
GT_PARAM_KEYS = (("node_emb.weight", "pe_emb.weight", "edge_emb.weight")
                 + tuple("gt_layers.0." + k for k in ("WQ.weight", "WK.weight", "WV.weight", "n_gate.weight", "n_gate.bias",
                                                      "WO.weight", "WO.bias", "norm1.weight", "norm1.bias",
                                                      "ffn.mlp.0.weight", "ffn.mlp.0.bias", "ffn.mlp.3.weight",
                                                      "ffn.mlp.3.bias", "norm2.weight", "norm2.bias") + _GT_EDGE)
                 + tuple("gt_layers.1." + k for k in ("WQ.weight", "WK.weight") + _GT_EDGE)
                 + ("edge_linear.weight", "edge_linear.bias"))
GT_BUFFER_KEYS = tuple(f"gt_layers.{L}.{n}.{s}" for L, norms in ((0, ("norm1", "norm2", "norm1e", "norm2e")),
                                                                 (1, ("norm1e", "norm2e")))
                       for n in norms for s in ("running_mean", "running_var"))


class GtWeights:
    """The graph-transformer head's tensors in kernel order (``GT_PARAM_KEYS`` then ``GT_BUFFER_KEYS``), fp32 device tensors
    (contiguous views, no copies); ``tensors`` maps each key to its tensor, e.g. a ``GraphTransformerNet.state_dict()``."""
    PARAM_KEYS, BUFFER_KEYS = GT_PARAM_KEYS, GT_BUFFER_KEYS

    def __init__(self, tensors):
        self.params = [_contig(tensors[k].detach(), torch.float32, k) for k in self.PARAM_KEYS]
        self.buffers = [_contig(tensors[k].detach(), torch.float32, k) for k in self.BUFFER_KEYS]
        self.table = _ptr_array(self.params + self.buffers)


def _gt_args(plan: Plan, obs16, pe, least=0):
    """Checks the observations (M, N, 16) and the positional encoding (N, 16) of either graph-transformer network; -> M
    (``least`` = 1: the critic takes no empty batch and says so)."""
    _contig(obs16, torch.float32, "obs16")
    _contig(pe, torch.float32, "pe")
    N = plan.num_nodes
    if obs16.dim() != 3 or tuple(obs16.shape[1:]) != (N, 16) or obs16.size(0) < least:
        raise ValueError(f"obs16 must be (M, {N}, 16)" + (f" with M >= {least}" if least else ""))
    if tuple(pe.shape) != (N, 16):
        raise ValueError(f"pe must be ({N}, 16)")
    return obs16.size(0)


def policy_gt_logits(plan: Plan, obs16, ec: EdgeConst, pe, w: GtWeights, out=None, scratch=None):
    """The graph-transformer head's logits (M, E) from observations ``obs16`` (M, N, 16) (the :func:`policy_obs16` layout),
    the edge attribute of ``ec`` and the positional encoding ``pe`` (N, 16); evaluation-mode BatchNorm / dropout.
    ``scratch``: a caller-owned fp32 buffer of at least tarl_policy_gt_fwd_scratch_floats(plan, M) elements."""
    L = _lib.load()
    M = _gt_args(plan, obs16, pe)
    logits = out if out is not None else torch.empty((M, plan.num_edges), dtype=torch.float32, device=obs16.device)
    n = int(L.tarl_policy_gt_fwd_scratch_floats(plan.handle, M))
    if scratch is None or scratch.numel() < n:
        scratch = torch.empty(n, dtype=torch.float32, device=obs16.device)
    _contig(scratch, torch.float32, "scratch")
    _lib.check(L.tarl_policy_gt_fwd(plan.handle, obs16.data_ptr(), M, ec.edge_attr.data_ptr(), pe.data_ptr(), w.table,
                                    scratch.data_ptr(), n, logits.data_ptr(), _lib.current_stream()))
    return logits


GT_CHUNK_ITEMS = 1024          # items per stage-1 partial sum of the backward's weight gradients (csrc/gt_policy.hip)


def gt_bwd_max_samples(plan: Plan) -> int:
    """The largest sample count one tarl_policy_gt_bwd call takes: its weight-gradient grid has one row of blocks per
    1 024 (sample, edge) or (sample, node) items, at most 65 535 rows."""
    return 65535 * GT_CHUNK_ITEMS // max(plan.num_edges, plan.num_nodes, 1)


def gt_bwd_scratch_bytes(plan: Plan, M: int) -> int:
    """Device scratch of one tarl_policy_gt_bwd call over ``M`` samples (activation records of every node and edge)."""
    return 4 * int(_lib.load().tarl_policy_gt_bwd_scratch_floats(plan.handle, int(M)))


def policy_gt_bwd(plan: Plan, obs16, ec: EdgeConst, pe, w: GtWeights, grad_logits, grads, scratch=None):
    """Accumulates the gradients of sum(grad_logits * logits) into ``grads``: one fp32 contiguous tensor per
    ``GT_PARAM_KEYS`` entry, shaped like the parameter. Deterministic (no atomics). ``scratch``: an fp32 device tensor of
    at least ``gt_bwd_scratch_bytes(plan, M) / 4`` elements to reuse across calls (allocated per call when None)."""
    L = _lib.load()
    M = _gt_args(plan, obs16, pe)
    gl = _contig(grad_logits, torch.float32, "grad_logits")
    if gl.numel() != M * plan.num_edges:
        raise ValueError("grad_logits must be (M, E)")
    gs = [_contig(g, torch.float32, "grad") for g in grads]
    if len(gs) != len(GT_PARAM_KEYS) or any(g.shape != p.shape for g, p in zip(gs, w.params)):
        raise ValueError("grads must match GT_PARAM_KEYS in number and shapes")
    if M > gt_bwd_max_samples(plan):
        raise ValueError(f"the graph-transformer backward takes at most {gt_bwd_max_samples(plan)} samples on this graph")
    n = int(L.tarl_policy_gt_bwd_scratch_floats(plan.handle, M))
    if scratch is None:
        scratch = torch.empty(n, dtype=torch.float32, device=obs16.device)
    else:
        _contig(scratch, torch.float32, "scratch")
        n = scratch.numel()
    _lib.check(L.tarl_policy_gt_bwd(plan.handle, obs16.data_ptr(), M, ec.edge_attr.data_ptr(), pe.data_ptr(), w.table,
                                    gl.data_ptr(), scratch.data_ptr(), n, _ptr_array(gs), _lib.current_stream()))


def fused_rollout_gt(plan: Plan, fs: FusedState, x, agent_features, ec: EdgeConst, pe, w: GtWeights, times, *, use_cong,
                     temperature, policy_seed, policy_counter0, seed, counter0, scratch, prev_time=None, keep=None,
                     obs_keep=None, choice8=None, log_prob=None, reward=None, counts=None):
    """``T = len(times)`` frames under the graph-transformer head in one foreign call (tarl_fused_rollout_gt). ``keep`` /
    ``obs_keep`` / ``choice8`` / ``counts`` as :func:`fused_rollout_policy`; ``log_prob`` / ``reward`` (T, B)."""
    _contig(pe, torch.float32, "pe")
    if tuple(pe.shape) != (fs.N, 16):
        raise ValueError(f"pe must be ({fs.N}, 16)")
    n = int(_lib.load().tarl_policy_gt_fwd_scratch_floats(plan.handle, fs.B))
    if getattr(fs, "gt_scratch", None) is None or fs.gt_scratch.numel() < n:
        fs.gt_scratch = torch.empty(n, dtype=torch.float32, device=fs.sel8.device)
    _head_rollout("tarl_fused_rollout_gt", plan, fs, x, agent_features, ec, times, (pe.data_ptr(), w.table),
                  use_cong=use_cong, temperature=temperature, policy_seed=policy_seed, policy_counter0=policy_counter0,
                  seed=seed, counter0=counter0, scratch=scratch, prev_time=prev_time, keep=keep, obs_keep=obs_keep,
                  choice8=choice8, log_prob=log_prob, reward=reward, counts=counts, obs_scratch=True,
                  head_scratch=(fs.gt_scratch.data_ptr(), fs.gt_scratch.numel()))


# ---- graph-transformer critic (value_head = "graph_transformer", csrc/gt_value.hip) -------------------------------------------
# state-dict keys of the critic's GraphTransformerNet in the kernels' order: the trainable tensors that reach the value, then
# the BatchNorm running statistics (include/tarl_hip.h). The edge side (edge_emb, WE, WOe, ffn_e, norm1e / norm2e, e_gate,
# edge_linear, log_var_mlp) never reaches the node output.
_GTV_NODE = ("WQ.weight", "WK.weight", "WV.weight", "n_gate.weight", "n_gate.bias", "WO.weight", "WO.bias", "norm1.weight",
             "norm1.bias", "ffn.mlp.0.weight", "ffn.mlp.0.bias", "ffn.mlp.3.weight", "ffn.mlp.3.bias", "norm2.weight",
             "norm2.bias")
GT_VALUE_PARAM_KEYS = (("node_emb.weight", "pe_emb.weight")
                       + tuple(f"gt_layers.{L}.{k}" for L in (0, 1) for k in _GTV_NODE)
                       + ("mu_mlp.mlp.0.weight", "mu_mlp.mlp.0.bias", "mu_mlp.mlp.2.weight", "mu_mlp.mlp.2.bias"))
GT_VALUE_BUFFER_KEYS = tuple(f"gt_layers.{L}.{n}.{s}" for L in (0, 1) for n in ("norm1", "norm2")
                             for s in ("running_mean", "running_var"))


class GtValueWeights(GtWeights):
    """The graph-transformer critic's tensors in kernel order (``GT_VALUE_PARAM_KEYS`` then ``GT_VALUE_BUFFER_KEYS``), fp32
    device tensors (contiguous views, no copies); ``tensors`` maps each key to its tensor."""
    PARAM_KEYS, BUFFER_KEYS = GT_VALUE_PARAM_KEYS, GT_VALUE_BUFFER_KEYS


def value_gt_fwd_scratch_bytes(plan: Plan, M: int) -> int:
    """Device scratch of one tarl_value_gt_fwd call over ``M`` samples."""
    return 4 * int(_lib.load().tarl_value_gt_fwd_scratch_floats(plan.handle, int(M)))


def value_gt_bwd_max_samples(plan: Plan) -> int:
    """The largest sample count one tarl_value_gt_bwd call takes (its weight-gradient grid has one row of blocks per
    1 024 (sample, node) items, at most 65 535 rows)."""
    return int(_lib.load().tarl_value_gt_bwd_max_samples(plan.handle))


def value_gt_bwd_scratch_bytes(plan: Plan, M: int) -> int:
    """Device scratch of one tarl_value_gt_bwd call over ``M`` samples (activation records of every node and edge)."""
    return 4 * int(_lib.load().tarl_value_gt_bwd_scratch_floats(plan.handle, int(M)))


def _scratch(scratch, n, device):
    if scratch is None:
        return torch.empty(n, dtype=torch.float32, device=device)
    _contig(scratch, torch.float32, "scratch")
    if scratch.numel() < n:
        raise ValueError(f"scratch holds {scratch.numel()} floats, the call needs {n}")
    return scratch


def value_gt_forward(plan: Plan, obs16, pe, w: GtValueWeights, out=None, scratch=None):
    """The graph-transformer critic's value (M,) from observations ``obs16`` (M, N, 16) (the :func:`policy_obs16` layout)
    and the positional encoding ``pe`` (N, 16); evaluation-mode BatchNorm / dropout. ``scratch``: an fp32 device tensor of
    at least ``value_gt_fwd_scratch_bytes(plan, M) / 4`` elements to reuse (allocated per call when None)."""
    L = _lib.load()
    M = _gt_args(plan, obs16, pe, least=1)
    value = out if out is not None else torch.empty(M, dtype=torch.float32, device=obs16.device)
    _contig(value, torch.float32, "value")
    if value.numel() != M:
        raise ValueError("value must hold M elements")
    scratch = _scratch(scratch, int(L.tarl_value_gt_fwd_scratch_floats(plan.handle, M)), obs16.device)
    _lib.check(L.tarl_value_gt_fwd(plan.handle, obs16.data_ptr(), M, pe.data_ptr(), w.table, scratch.data_ptr(),
                                   scratch.numel(), value.data_ptr(), _lib.current_stream()))
    return value


def value_gt_backward(plan: Plan, obs16, pe, w: GtValueWeights, grad_value, grads, scratch=None):
    """Accumulates the gradients of sum(grad_value * value) into ``grads``: one fp32 contiguous tensor per
    ``GT_VALUE_PARAM_KEYS`` entry, shaped like the parameter. Deterministic (no atomics). ``scratch``: an fp32 device tensor
    of at least ``value_gt_bwd_scratch_bytes(plan, M) / 4`` elements to reuse (allocated per call when None)."""
    L = _lib.load()
    M = _gt_args(plan, obs16, pe, least=1)
    gv = _contig(grad_value, torch.float32, "grad_value")
    if gv.numel() != M:
        raise ValueError("grad_value must hold M elements")
    gs = [_contig(g, torch.float32, "grad") for g in grads]
    if len(gs) != len(GT_VALUE_PARAM_KEYS) or any(g.shape != p.shape for g, p in zip(gs, w.params)):
        raise ValueError("grads must match GT_VALUE_PARAM_KEYS in number and shapes")
    cap = value_gt_bwd_max_samples(plan)
    if M > cap:
        raise ValueError(f"the graph-transformer critic's backward takes at most {cap} samples on this graph")
    scratch = _scratch(scratch, int(L.tarl_value_gt_bwd_scratch_floats(plan.handle, M)), obs16.device)
    _lib.check(L.tarl_value_gt_bwd(plan.handle, obs16.data_ptr(), M, pe.data_ptr(), w.table, gv.data_ptr(),
                                   scratch.data_ptr(), scratch.numel(), _ptr_array(gs), _lib.current_stream()))


def rollout_gather(plan: Plan, T, B, env_minor, idx=None, *, choice=None, counts=None):
    """Rollout bytes -> (choice_eid int32 (rows, N) | None, counts_f fp32 (rows, N) | None) for the (frame, env) pairs
    ``idx`` (int64 flat indices t * B + b; None = all ``T * B`` in order). ``choice`` / ``counts``: the uint8 buffers
    ((T,N,B) when ``env_minor`` else (T,B,N)); ``T`` is the buffers' leading extent."""
    L = _lib.load()
    N = plan.num_nodes
    some = choice if choice is not None else counts
    rows = T * B if idx is None else idx.numel()
    for nm, t_ in (("choice", choice), ("counts", counts)):
        if t_ is not None:
            _contig(t_, torch.uint8, nm)
            if t_.numel() != T * B * N:
                raise ValueError(f"{nm} must hold T*B*N bytes")
    if idx is not None:
        _contig(idx, torch.int64, "idx")
    ce = torch.empty((rows, N), dtype=torch.int32, device=some.device) if choice is not None else None
    cf = torch.empty((rows, N), dtype=torch.float32, device=some.device) if counts is not None else None
    _lib.check(L.tarl_rollout_gather(plan.handle, _lib.ptr(choice), _lib.ptr(counts), T, B, 1 if env_minor else 0,
                                     _lib.ptr(idx), rows, _lib.ptr(ce), _lib.ptr(cf), _lib.current_stream()))
    return ce, cf


# ---- MPNNValueNet (dormant message-passing critic) ---------------------------------------------------------------------------
def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def value_mpnn_forward(plan: Plan, node_features, agent_rows, edge_features, time, params, *, keep=False):
    """``node_features`` (M, N, 7), ``agent_rows`` (M, N, 9) or None, ``edge_features`` (M, E) or (E,), ``time`` (M,),
    ``params`` = the 12 parameter tensors in tarl_value_mpnn_fwd's order -> value (M,) [+ node_act, agg (M, N)]."""
    L = _lib.load()
    M, N = node_features.size(0), node_features.size(1)
    if N != plan.num_nodes or node_features.size(2) != 7:
        raise ValueError("node_features must be (M, num_nodes, 7)")
    nf = _contig(node_features, torch.float32, "node_features")
    ar = None if agent_rows is None else _contig(agent_rows, torch.float32, "agent_rows")
    ef = _contig(edge_features, torch.float32, "edge_features")
    ef_stride = 0 if ef.dim() == 1 or ef.size(0) == 1 else plan.num_edges
    tm = _contig(time, torch.float32, "time")
    ps = [_contig(p.detach(), torch.float32, "param") for p in params]
    value = torch.empty(M, dtype=torch.float32, device=nf.device)
    act = torch.empty((M, N), dtype=torch.float32, device=nf.device) if keep else None
    agg = torch.empty((M, N), dtype=torch.float32, device=nf.device) if keep else None
    _lib.check(L.tarl_value_mpnn_fwd(plan.handle, nf.data_ptr(), M, _lib.ptr(ar), ef.data_ptr(), ef_stride, tm.data_ptr(),
                                     _ptr_array(ps), value.data_ptr(), _lib.ptr(act), _lib.ptr(agg),
                                     _lib.current_stream()))
    return value, act, agg


def value_mpnn_backward(plan: Plan, node_features, agent_rows, edge_features, time, params, grad_value, act, agg):
    """Parameter gradients (list of 12 tensors shaped like ``params``) of sum(grad_value * value)."""
    L = _lib.load()
    M = node_features.size(0)
    nf = _contig(node_features, torch.float32, "node_features")
    ar = None if agent_rows is None else _contig(agent_rows, torch.float32, "agent_rows")
    ef = _contig(edge_features, torch.float32, "edge_features")
    ef_stride = 0 if ef.dim() == 1 or ef.size(0) == 1 else plan.num_edges
    ps = [_contig(p.detach(), torch.float32, "param") for p in params]
    grads = [torch.zeros_like(p) for p in ps]
    gv = _contig(grad_value, torch.float32, "grad_value")
    _lib.check(L.tarl_value_mpnn_bwd(plan.handle, nf.data_ptr(), M, _lib.ptr(ar), ef.data_ptr(), ef_stride,
                                     _contig(time, torch.float32, "time").data_ptr(), _ptr_array(ps), gv.data_ptr(),
                                     act.data_ptr(), agg.data_ptr(), _ptr_array(grads), _lib.current_stream()))
    return grads


def noise_export(plan: Plan, kind: str, seed: int, counter: int, env_ids):
    """The device noise of the Philox path for the listed GLOBAL environment ids (tarl_noise_export; test hook):
    ``kind="gumbel"`` -> (n, E) fp32 Gumbel values of DirectionMPNN.aggregate's race in ORIGINAL edge order (seed = the
    engine's ``seed``, counter = the frame's noise counter); ``kind="uniform"`` -> (n, G) uniforms of the action draw."""
    L = _lib.load()
    env = torch.as_tensor(env_ids, dtype=torch.int64).to(plan.device).contiguous()
    n = env.numel()
    width = plan.num_edges if kind == "gumbel" else plan.num_groups
    out = torch.empty((n, width), dtype=torch.float32, device=plan.device)
    _lib.check(L.tarl_noise_export(plan.handle, {"gumbel": 0, "uniform": 1}[kind], int(seed), int(counter), env.data_ptr(),
                                   n, out.data_ptr(), _lib.current_stream()))
    return out


def rollout_env_supported(plan: Plan) -> bool:
    return bool(_lib.load().tarl_rollout_env_supported(plan.handle))


def rollout_env(plan: Plan, fs: FusedState, tables: PolicyTables, agent_features, ec: EdgeConst, times, *, use_cong,
                policy_seed, policy_counter0, seed, counter0, scratch, prev_time=None, choice=None, log_prob=None,
                entropy=None, reward=None, counts=None, metrics_envs=0, dtt_node=None, events=None, leg=None):
    """Same contract as :func:`fused_rollout` through ``tarl_rollout_env`` (one workgroup per environment, LDS-resident
    records, one launch for all frames); the per-node buffers are ENV-MAJOR: ``choice`` / ``counts`` (T, B, N),
    ``dtt_node`` / ``events`` (T, metrics_envs, N)."""
    L, T, A, abs_, prev = _rollout_args(fs, agent_features, times, scratch, prev_time)
    _check_rollout_outputs(T, fs.B, fs.N, False, metrics_envs, choice, counts, log_prob, entropy, reward, dtt_node, events, leg)
    tdev = torch.tensor([float(t) for t in times], dtype=torch.float32).to(fs.sel.device, non_blocking=True)
    if getattr(fs, "env_scratch", None) is None:
        fs.env_scratch = torch.empty(int(L.tarl_rollout_env_scratch_bytes(plan.handle)), dtype=torch.uint8,
                                     device=fs.sel.device)
    _lib.check(L.tarl_rollout_env(plan.handle, fs.ref, fs.B, fs.Nmax, T, tdev.data_ptr(), prev, tables.thresholds.data_ptr(),
                                  tables.log_probs.data_ptr(), tables.entropy.data_ptr(), int(policy_seed),
                                  int(policy_counter0), agent_features.data_ptr(), A, abs_, ec.edge_attr.data_ptr(),
                                  ec.log_edge_attr.data_ptr(), ec.log_eps, 1 if use_cong else 0, int(seed),
                                  int(counter0), scratch.data_ptr(), fs.env_scratch.data_ptr(), _lib.ptr(choice),
                                  _lib.ptr(log_prob), _lib.ptr(entropy), _lib.ptr(reward), _lib.ptr(counts),
                                  int(metrics_envs), _lib.ptr(dtt_node), _lib.ptr(events), _lib.ptr(leg),
                                  _lib.current_stream()))
    return tdev


_SPLIT_SCRATCH = {}


def critic_forward_slabs(cw: CriticWeights, counts, time_rows, *, exact_chain=False):
    """counts (S, N, R) fp32 or uint8 contiguous = [frame][node][env] with R % 128 == 0 -> value (S*R,) in (frame, env)
    order; ``time_rows`` (S,) is each frame's clock."""
    L = _lib.load()
    u8 = counts.dtype == torch.uint8
    _contig(counts, torch.uint8 if u8 else torch.float32, "counts")
    _contig(time_rows, torch.float32, "time_rows")
    S, N, R = counts.shape
    if N != cw.N or R % 128 or time_rows.numel() < S:
        raise ValueError("counts must be (S, N, R) with R a multiple of 128 and one time per slab")
    value = torch.empty(S * R, dtype=torch.float32, device=counts.device)
    args = (counts.data_ptr(), R, S * R, N, time_rows.data_ptr(), R, cw.w1.data_ptr(), cw.b1.data_ptr(), cw.w2.data_ptr(),
            cw.b2.data_ptr(), cw.w3.data_ptr(), cw.b3.data_ptr())
    if u8:
        # count bytes: first layer on the bf16 matrix cores at fp32 accuracy (W1 as three exact bf16 pieces);
        # exact_chain=True keeps the k-ordered fp32 MFMA chain (bit-identical to the row-major kernel)
        scratch = None
        if not exact_chain:
            key = (str(counts.device), N)
            scratch = _SPLIT_SCRATCH.get(key)
            if scratch is None:
                scratch = torch.empty(int(L.tarl_critic_split_scratch_bytes(N)), dtype=torch.uint8, device=counts.device)
                _SPLIT_SCRATCH[key] = scratch
        _lib.check(L.tarl_critic_mlp_fwd_slabs_u8(*args, _lib.ptr(scratch), value.data_ptr(), _lib.current_stream()))
    else:
        _lib.check(L.tarl_critic_mlp_fwd_slabs(*args, value.data_ptr(), _lib.current_stream()))
    return value
