"""The shortest-path cases on the irregular road graphs of tests/irregular_graphs.py, shared by test_sp_irregular_host.py
(CPU) and test_gpu_sp_irregular.py (GPU): the two weight sets, the CPU references (computed once per process), the checks
the GPU tests apply to a kernel's output, and the restatements with one deliberate restriction each — what a kernel would
compute that fetched its weights in CSR position instead of by edge id, stopped every list after four entries, or looked
a next hop up among the four embedded out-edges only. Plain module: no fixtures, nothing here needs a GPU.

Weights: ``ff`` = the free-flow time of the target road (untied but for the self-evident cases), ``r5`` = ``ff`` rounded
to multiples of 5 s (three distinct values: many ties, none of them from a lattice).

Lists: the plan's CSR out-list of a road holds its out-edges in ascending edge id, the CSC in-list its in-edges likewise;
``out_eid`` / ``in_eid`` map a list position back to the edge id. Trees towards a destination PULL over the out-lists and
MARK over the in-lists; trees from an origin the opposite (csrc/sp_trees.h)."""
from __future__ import annotations

import functools
import heapq
import os
import types
from itertools import count

import numpy as np
import torch

import irregular_graphs as ig
from oracle import routing
from tree_restatement import adjacency, cpu_dijkstra, cpu_tie_rule

NAMES = ("MIXED", "HUB126")
WEIGHTS = ("ff", "r5")
SEL_RAW = 0x7F
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routing_irregular.npz")
UNREACHABLE = {"MIXED": 312, "HUB126": 1112}        # ordered pairs (u, d) without a path, of N * N
MAX_DEGREE = {"MIXED": 9, "HUB126": 126}


# ---- graphs, lists, weights ------------------------------------------------------------------------------------------------
def lists(ei, N):
    """The plan's two adjacencies (csrc/plan.hip) restated: dict of int64 tensors out_ptr, out_dst, out_eid, in_ptr,
    in_src, in_eid."""
    E = ei.size(1)
    out = {}
    for tag, key, other in (("out", ei[0], ei[1]), ("in", ei[1], ei[0])):
        eid = torch.argsort(key, stable=True)
        ptr = torch.zeros(N + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.bincount(key, minlength=N), 0)
        out[tag + "_ptr"], out[tag + "_eid"] = ptr, eid
        out["out_dst" if tag == "out" else "in_src"] = other[eid]
    assert out["out_eid"].numel() == E
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace: net, N, E, ei, Nmax, w = {"ff", "r5"} fp32 (E,), the lists of :func:`lists`, in_rank / out_rank (E,)."""
    net = ig.graph(name)
    N, ei = net.num_roads, net.edge_index
    ff = net.x[:, 3 * net.Nmax + 2][ei[1]].contiguous()
    irank, orank = ig.edge_ranks(ei, N)
    return types.SimpleNamespace(name=name, net=net, N=N, E=ei.size(1), ei=ei, Nmax=net.Nmax,
                                 w={"ff": ff, "r5": (torch.round(ff / 5) * 5).contiguous()}, in_rank=irank, out_rank=orank,
                                 **lists(ei, N))


def torus_case():
    """A heterogeneous torus in the same shape as :func:`case` (weights ``ff`` only): the graph family every shortest-path
    test ran on before, where both edge-id maps are the identity."""
    from tarl_hip import synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    N, ei = net.num_roads, net.edge_index
    ff = net.x[:, 3 * net.Nmax + 2][ei[1]].contiguous()
    irank, orank = ig.edge_ranks(ei, N)
    return types.SimpleNamespace(name="torus", net=net, N=N, E=ei.size(1), ei=ei, Nmax=net.Nmax, w={"ff": ff}, in_rank=irank,
                                 out_rank=orank, **lists(ei, N))


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def random_weights(E, seed):
    """Untied fp32 weights in [1, 21)."""
    return (torch.rand(E, generator=torch.Generator().manual_seed(seed)) * 20 + 1).contiguous()


# ---- references, once per process ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_pairs(name, tag):
    """oracle.routing.all_pairs: (next_hop int64 [u][d], dist fp32 [u][d]); -1 / +inf where there is no path."""
    c = case(name)
    return routing.all_pairs(c.ei, c.w[tag], c.N)


def trees_of(ei, w, N, reverse):
    """Every root's tree by tree_restatement: (dist fp64 [root][node], link int32 [root][node]). ``reverse``: towards the
    root, link = the next hop and the root holds itself; else from the root, link = the predecessor, -1 at the root."""
    adj = adjacency(ei, w.to(torch.float64), N, reverse=reverse)
    dist = torch.empty((N, N), dtype=torch.float64)
    link = torch.empty((N, N), dtype=torch.int32)
    for r in range(N):
        d, _ = cpu_dijkstra(adj, N, r, reverse=reverse)
        l = cpu_tie_rule(adj, d, N, r, reverse=reverse)
        if reverse:
            l[r] = r
        dist[r], link[r] = torch.tensor(d, dtype=torch.float64), torch.tensor(l, dtype=torch.int32)
    return dist, link


@functools.lru_cache(maxsize=None)
def trees(name, tag, reverse):
    c = case(name)
    return trees_of(c.ei, c.w[tag], c.N, reverse)


# ---- the checks of the GPU tests (the host tests feed them the restricted restatements) -------------------------------------
def check_all_pairs(name, tag, next_hop, dist):
    """A kernel's all-pairs tables [u][d] against the oracle's and, where the golden holds the pair, real networkx's."""
    nh_o, dist_o = all_pairs(name, tag)
    assert torch.equal(next_hop.to(torch.int64), nh_o), f"{name}/{tag}: next hops against the oracle"
    key = f"{name}__next_hop_{tag}"
    if key in golden():
        assert torch.equal(next_hop.to(torch.int16), golden()[key]), f"{name}/{tag}: next hops against networkx"
    assert dist.dtype == torch.float32 and torch.equal(dist, dist_o), f"{name}/{tag}: distances"
    unreachable = next_hop < 0
    assert int(unreachable.sum()) == UNREACHABLE[name] and bool(torch.isinf(dist[unreachable]).all())
    assert bool(torch.isfinite(dist[~unreachable]).all())


def check_trees(name, tag, reverse, dist, link):
    """A kernel's trees for all N roots in order, [root][node], against tree_restatement's distances and tie rule."""
    d_ref, l_ref = trees(name, tag, reverse)
    assert dist.dtype == torch.float64 and torch.equal(dist, d_ref), f"{name}/{tag}: distances, reverse={reverse}"
    assert torch.equal(link.to(torch.int32), l_ref), f"{name}/{tag}: links, reverse={reverse}"
    assert int(torch.isinf(dist).sum()) == UNREACHABLE[name]


def out_table(c):
    """(N, max out-degree) int64: every road's out-list targets in list order, padded with -2 (no table value)."""
    deg = c.out_ptr[1:] - c.out_ptr[:-1]
    t = torch.full((c.N, int(deg.max())), -2, dtype=torch.int64)
    t[c.ei[0][c.out_eid], c.out_rank[c.out_eid]] = c.out_dst
    return t


def rank_codes(c, next_hop_du, first_four=False):
    """The rank byte k_fused_select_next_hop_dest stores for a per-destination table [d][u]: the position of the first
    out-edge of u whose target is the table's value, SEL_RAW (the value travels as a float instead) where there is none:
    -1 and the destination itself. ``first_four``: the lookup stops after the four out-edges embedded in the node record."""
    t = out_table(c)
    if first_four:
        t = t[:, :4]
    hit = t.unsqueeze(0) == next_hop_du.to(torch.int64).unsqueeze(-1)              # [d][u][rank]
    first = torch.argmax(hit.to(torch.int8), dim=-1)
    return torch.where(hit.any(-1), first, torch.full_like(first, SEL_RAW))


def check_ranks(c, next_hop_du, codes):
    """Rank bytes [d][u] of a per-destination table: each names the out-edge at that list position, and SEL_RAW appears
    exactly where the hop is -1 or the row is the destination itself (no self-loops: its value is no successor). -> the
    number of codes >= 4."""
    nh = next_hop_du.to(torch.int64)
    raw = codes == SEL_RAW
    assert torch.equal(raw, (nh < 0) | torch.eye(c.N, dtype=torch.bool)), "SEL_RAW exactly at -1 and on the destination itself"
    t = out_table(c)
    named = t[torch.arange(c.N).unsqueeze(0).expand(c.N, -1), codes.clamp(max=t.size(1) - 1)]
    assert torch.equal(named[~raw], nh[~raw]), "a rank byte names another out-edge"
    return int(((codes >= 4) & ~raw).sum())


# ---- restatements with one restriction --------------------------------------------------------------------------------------
def positional_weights(c, w, by):
    """What a kernel reads that takes ``w[k]`` for ``w[eid[k]]``: edge e gets the weight stored at e's POSITION in the
    out-lists (``by="out"``) or the in-lists (``by="in"``). With these weights the correct algorithm is that kernel."""
    eid = c.out_eid if by == "out" else c.in_eid
    seen = torch.empty_like(w)
    seen[eid] = w                      # position k holds edge eid[k], and reads w[k]
    return seen


def all_pairs_lists(c, w, cut=False):
    """oracle.routing.all_pairs restated over the CSR lists the way k_apsp walks them (networkx's heap replay: (distance,
    push counter) keys, successors in list order). ``cut``: the relaxation loop stops after four entries."""
    N = c.N
    ptr, dst, wl = c.out_ptr.tolist(), c.out_dst.tolist(), w[c.out_eid].tolist()
    next_hop = torch.full((N, N), -1, dtype=torch.int64)
    dist_m = torch.full((N, N), float("inf"), dtype=torch.float64)
    for s in range(N):
        dist, seen, hop = {}, {s: 0.0}, {s: s}
        cnt = count()
        fringe = [(0.0, next(cnt), s)]
        while fringe:
            d, _, v = heapq.heappop(fringe)
            if v in dist:
                continue
            dist[v] = d
            k1 = min(ptr[v + 1], ptr[v] + 4) if cut else ptr[v + 1]
            for k in range(ptr[v], k1):
                u, vu = dst[k], d + wl[k]
                if u in dist:
                    continue
                if u not in seen or vu < seen[u]:
                    seen[u] = vu
                    heapq.heappush(fringe, (vu, next(cnt), u))
                    hop[u] = u if v == s else hop[v]
        for t, d in dist.items():
            next_hop[s, t] = hop[t]
            dist_m[s, t] = d
    return next_hop, dist_m.to(torch.float32)


def tree_distances_rounds(c, w, reverse, cut_pull=False, cut_mark=False):
    """spt_distances (csrc/sp_trees.h) restated round by round for all N roots at once: the frontier marks its dependants
    over the mark lists, every marked node pulls min(dist[nbr] + w) over its pull list and joins the next frontier if that
    improved it. fp64 [root][node]. ``cut_pull`` / ``cut_mark``: the pull / mark loop stops after four entries."""
    N = c.N
    owner, nbr = (c.ei[0], c.ei[1]) if reverse else (c.ei[1], c.ei[0])       # the node that pulls, the node pulled from
    pull_rank, mark_rank = (c.out_rank, c.in_rank) if reverse else (c.in_rank, c.out_rank)
    pull = torch.nonzero(pull_rank < 4).view(-1) if cut_pull else torch.arange(c.E)
    mark = torch.nonzero(mark_rank < 4).view(-1) if cut_mark else torch.arange(c.E)
    w64 = w.to(torch.float64)
    inf = float("inf")
    dist = torch.full((N, N), inf, dtype=torch.float64)
    dist[torch.arange(N), torch.arange(N)] = 0.0
    front = torch.eye(N, dtype=torch.bool)
    for _ in range(N):
        cand = torch.zeros((N, N), dtype=torch.bool)
        cand.index_put_((torch.arange(N).unsqueeze(1).expand(-1, mark.numel()), owner[mark].unsqueeze(0).expand(N, -1)),
                        front[:, nbr[mark]], accumulate=True)
        offer = w64[pull] + dist[:, nbr[pull]] if reverse else dist[:, nbr[pull]] + w64[pull]
        best = torch.full((N, N), inf, dtype=torch.float64).scatter_reduce_(
            1, owner[pull].unsqueeze(0).expand(N, -1), offer, reduce="amin", include_self=True)
        front = cand & (best < dist)
        if not bool(front.any()):
            break
        dist = torch.where(front, best, dist)
    return dist


def subgraph(c, w, keep):
    """(edge_index, weights) of the edges ``keep`` (bool (E,)), order kept."""
    return c.ei[:, keep].contiguous(), w[keep].contiguous()
