"""Irregular road graphs for the simulation-step tests: dual graphs of link lists with hubs (in-degree and out-degree far
beyond the four of a torus), dead ends and feeder links, a degree-agnostic random state, a census of which branches a run
of the CPU oracle reaches, and oracle replays with one deliberate restriction each (what a kernel that mishandles long
in-lists / out-lists or the tie order would compute). Two further graphs keep the sibling structure of a torus — rows 4c ..
4c+3 leave one intersection and share their upstream rows, every road has out-edges — at in-degrees 0 .. 9 and out-degrees
1 .. 9: the sibling Direction gather and the quad action draw off the torus. LONG127 and LONGMIX are small tori whose roads
hold up to 126 agents in 127-slot FIFOs — the FIFO-length limit of the packed path — with counters of how far the queues,
the ring offsets and the inserts of a run get (:func:`long_fifo_counters`). Plain module: no fixtures, nothing here needs
a GPU.

Ranks: the in-rank of a dual edge is its position among the edges with the same destination in ascending edge id (the
plan's CSC order); the out-rank its position among the edges with the same source (the plan's CSR order). The fused
records embed ranks 0-3 (NodeRec::in4 / out4); ranks >= 4 are reached only through the tail loops."""
from __future__ import annotations

import functools

import torch

from oracle import sim
from tarl_hip import ops, synth


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def hub_links(hubs, ring, seed):
    """Directed links (tail intersection, head intersection): a ring of ``ring`` ordinary intersections linked both ways,
    plus one extra intersection per ``(k_in, k_out)`` of ``hubs`` with ``k_in`` links from random ring intersections and
    ``k_out`` links to random ring intersections (drawn with replacement: parallel links are distinct roads); the link
    order is shuffled. Roads leaving a hub have in-degree ``k_in`` in the dual graph, roads entering it out-degree
    ``k_out``."""
    g = torch.Generator().manual_seed(seed)
    links = []
    for v in range(ring):
        links += [(v, (v + 1) % ring), ((v + 1) % ring, v)]
    for h, (k_in, k_out) in enumerate(hubs):
        links += [(v, ring + h) for v in torch.randint(0, ring, (k_in,), generator=g).tolist()]
        links += [(ring + h, v) for v in torch.randint(0, ring, (k_out,), generator=g).tolist()]
    return [links[i] for i in torch.randperm(len(links), generator=g).tolist()]


def road_network(links, seed, shuffle=True) -> synth.SynthNetwork:
    """The dual graph of ``links``: road r is ``links[r]``, one dual edge r -> s whenever head(r) == tail(s). Per-link
    length / lanes / capacity as ``synth.torus_network(heterogeneous=True)`` draws them, ``edge_attr`` random and normalised
    per upstream road. ``shuffle``: the edges are spread over the edge list at random (neither source- nor destination-
    sorted) — every road's own out-edges stay in ascending target order, so the roads entering one intersection keep
    identical ordered out-lists (the row pass groups rows by that list), while the order inside the in-lists is arbitrary."""
    g = torch.Generator().manual_seed(seed)
    R = len(links)
    tail = torch.tensor([a for a, _ in links])
    head = torch.tensor([b for _, b in links])
    lengths = 60.0 + 90.0 * torch.rand(R, generator=g)
    caps = 5.0 + torch.randint(0, 4, (R,), generator=g).float() * 5.0
    lanes = 1.0 + torch.randint(0, 2, (R,), generator=g).float()
    maxn = torch.floor(lengths * lanes / 7.5) + 1
    nmax = int(maxn.max().item()) + 1
    x = torch.zeros((R, 3 * nmax + 7), dtype=torch.float32)
    x[:, 3 * nmax + 0] = maxn
    x[:, 3 * nmax + 2] = lengths / 10.0
    x[:, 3 * nmax + 3] = lengths
    x[:, 3 * nmax + 4] = caps
    x[:, 3 * nmax + 6] = torch.arange(R, dtype=torch.float32)
    src, dst = torch.nonzero(head.unsqueeze(1) == tail.unsqueeze(0), as_tuple=True)      # sorted by (source, target)
    E = src.numel()
    w = 0.5 + torch.rand(E, generator=g)
    attr = (w / torch.zeros(R).index_add_(0, src, w)[src]).to(torch.float32)
    if shuffle:
        perm = torch.randperm(E, generator=g)
        place = perm[torch.argsort(src * E + perm)]      # k-th edge in (source, target) order -> its slot in the edge list
        ei, ea = torch.empty((2, E), dtype=torch.int64), torch.empty(E)
        ei[:, place], ea[place] = torch.stack([src, dst]), attr
    else:
        ei, ea = torch.stack([src, dst]), attr
    critical = x[:, 3 * nmax + 4] * x[:, 3 * nmax + 2] / 3600
    cong = x[:, 3 * nmax + 2] * (x[:, 3 * nmax + 0] + 10 - critical)
    net = synth.SynthNetwork(x=x, edge_index=ei.contiguous(), edge_attr=ea.view(-1, 1).contiguous(), Nmax=nmax, num_roads=R,
                             critical_number=critical, congestion_constant=cong)
    assert ops.fused_path_supported(net.edge_index, nmax)
    return net


def sibling_links(out_degrees, in_degrees, gen):
    """Directed links numbered by tail intersection — the roads that leave one intersection are consecutive — with the
    heads dealt to them by a seeded shuffle of every intersection's in-degree worth of heads, redrawn until no link is a
    self-loop. With out-degrees that are multiples of four the four roads 4c .. 4c+3 of the dual graph leave the same
    intersection: siblings, which share their whole in-list."""
    assert sum(out_degrees) == sum(in_degrees) and all(d % 4 == 0 for d in out_degrees)
    tails = torch.tensor([v for v, k in enumerate(out_degrees) for _ in range(k)])
    heads = torch.tensor([v for v, k in enumerate(in_degrees) for _ in range(k)])
    while True:
        dealt = heads[torch.randperm(heads.numel(), generator=gen)]
        if not bool((dealt == tails).any()):
            return list(zip(tails.tolist(), dealt.tolist()))


def sibling_network(seed) -> synth.SynthNetwork:
    """SIBS: the dual graph of :func:`sibling_links`, its edge list reordered by (pi(source), target) for a seeded
    permutation pi of the roads: every in-list is ordered by pi(source) — the same order for all siblings — every out-list
    stays in ascending target order, and the list as a whole is neither source- nor destination-sorted."""
    gen = torch.Generator().manual_seed(seed)
    net = road_network(sibling_links(SIBS_OUT, SIBS_IN, gen), seed, shuffle=False)
    R = net.num_roads
    pi = torch.randperm(R, generator=gen)
    order = torch.argsort(pi[net.edge_index[0]] * R + net.edge_index[1])
    net.edge_index = net.edge_index[:, order].contiguous()
    net.edge_attr = net.edge_attr[order].contiguous()
    return net


def detach_sibling_tails(net, seed):
    """SIBS_TAILS from SIBS (``net``, edited in place): in every chunk of in-degree above four, each of the siblings 1 .. 3
    gives one in-edge of in-rank >= 4, drawn at random, another source — a road that is not in the row's in-list and is
    not the row itself. The edge keeps its id (so its in-rank), ``edge_attr`` is normalised per source road again. The
    siblings then share their first four sources and their in-degree, nothing more. Returns the number of edges moved."""
    gen = torch.Generator().manual_seed(seed)
    R, ei = net.num_roads, net.edge_index
    din, _ = degrees(net)
    moved = 0
    for row in range(R):
        if row % 4 == 0 or int(din[row]) <= 4:
            continue
        eids = torch.nonzero(ei[1] == row).view(-1)
        e = int(eids[4 + int(torch.randint(0, eids.numel() - 4, (1,), generator=gen))])
        taken = set(ei[0][eids].tolist()) | {row}
        free = [r for r in range(R) if r not in taken]
        ei[0, e] = free[int(torch.randint(0, len(free), (1,), generator=gen))]
        moved += 1
    w = net.edge_attr.view(-1)
    net.edge_attr = (w / torch.zeros(R).index_add_(0, ei[0], w)[ei[0]]).to(torch.float32).view(-1, 1).contiguous()
    assert ops.fused_path_supported(ei, net.Nmax)
    return moved


RING = 12
MIXED_HUBS = [(9, 9), (5, 8), (8, 5), (3, 1), (1, 3), (0, 2), (2, 0)]
HUB126_HUBS = [(126, 126), (0, 2), (2, 0)]
MIXED_SEED, HUB126_SEED = 9, 1
MIXED_DEGREES = {0, 1, 3, 4, 5, 8, 9}
# the sibling graphs: 12 intersections, 56 roads; a road's in-degree is the in-degree of the intersection it leaves, its
# out-degree the out-degree of the intersection it enters
SIBS_OUT = [4] * 10 + [8] * 2
SIBS_IN = [9, 4, 1, 5, 0, 8, 3, 4, 2, 8, 4, 8]
SIBS_SEED, SIBS_TAILS_SEED = 2, 2
SIBS_TAILS_MOVED = 18      # six chunks of in-degree above four, three siblings each
# agents per road, frames
CENSUS = {"MIXED": dict(per_road=40, T=80), "HUB126": dict(per_road=12, T=80),
          "SIBS": dict(per_road=40, T=80), "SIBS_TAILS": dict(per_road=40, T=80),
          "LONG127": dict(per_road=150, T=300), "LONGMIX": dict(per_road=150, T=300)}
LONG_GRAPHS = ("LONG127", "LONGMIX")      # 2 x 2 torus, 940 m links: MAX_NUMBER_OF_AGENT 126, Nmax 127 (the packed path's limit)
LONG_LENGTH, LONG_SPEED, LONGMIX_SHORT_MAX = 940.0, 94.0, 14.0
TIE_WHICH = {"SIBS": 1, "SIBS_TAILS": 1}      # which road of the wanted in-degree carries the crafted tie (tie_case)


def degrees(net):
    """(in-degree, out-degree) of every road."""
    R = net.num_roads
    return torch.bincount(net.edge_index[1], minlength=R), torch.bincount(net.edge_index[0], minlength=R)


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "MIXED":
        net = road_network(hub_links(MIXED_HUBS, RING, MIXED_SEED), MIXED_SEED)
        din, dout = degrees(net)
        assert MIXED_DEGREES <= set(din.tolist()) and MIXED_DEGREES <= set(dout.tolist()), (din.unique(), dout.unique())
    elif name == "HUB126":
        net = road_network(hub_links(HUB126_HUBS, RING, HUB126_SEED), HUB126_SEED)
        din, dout = degrees(net)
        assert int(din.max()) == 126 and int(dout.max()) == 126 and 256 < net.num_roads <= 512
    elif name in ("SIBS", "SIBS_TAILS"):
        net = sibling_network(SIBS_SEED)
        if name == "SIBS_TAILS":
            assert detach_sibling_tails(net, SIBS_TAILS_SEED) == SIBS_TAILS_MOVED
        din, dout = degrees(net)
        assert net.num_roads == 56 and set(din.tolist()) == set(SIBS_IN) and int(dout.min()) > 0      # G == N: the quad draw
    elif name in LONG_GRAPHS:
        net = synth.torus_network(2, 2, length=LONG_LENGTH, freespeed=LONG_SPEED)
        nmax = net.Nmax
        if name == "LONGMIX":      # every third road short (as the ``tiny`` case of test_gpu_fused.py), in the same 127-slot ring
            net.x[::3, 3 * nmax + 0] = LONGMIX_SHORT_MAX
            net.critical_number = net.x[:, 3 * nmax + 4] * net.x[:, 3 * nmax + 2] / 3600
            net.congestion_constant = net.x[:, 3 * nmax + 2] * (net.x[:, 3 * nmax + 0] + 10 - net.critical_number)
        assert net.num_roads == 16 and net.edge_index.size(1) == 64 and nmax == 127 and int(net.x[:, 3 * nmax].max()) == 126
        assert float(net.x[0, 3 * nmax + 2]) == 10.0 and ops.fused_path_supported(net.edge_index, nmax)
    else:
        raise KeyError(name)
    return net


def graph(name):
    """``"MIXED"`` (about 80 roads, in- and out-degrees {0, 1, 3, 4, 5, 8, 9} and more), ``"HUB126"`` (about 280 roads,
    one hub at the degree limit of the packed path: 126 in, 126 out), ``"SIBS"`` (56 roads, four siblings per chunk with
    in-degrees 0 .. 9 and out-degrees 4 and 8, every road with out-edges) or ``"SIBS_TAILS"`` (SIBS whose siblings share
    only their first four sources, out-degrees 1 .. 9), ``"LONG127"`` (16 roads of a 2 x 2 torus, 940 m each: up to 126
    agents in a FIFO of Nmax = 127 slots, free-flow 10 s) or ``"LONGMIX"`` (LONG127 with every third road holding at most 14)
    — a fresh copy, the caller may edit it."""
    n = _graph(name)
    return synth.SynthNetwork(x=n.x.clone(), edge_index=n.edge_index.clone(), edge_attr=n.edge_attr.clone(), Nmax=n.Nmax,
                              num_roads=n.num_roads, critical_number=n.critical_number.clone(),
                              congestion_constant=n.congestion_constant.clone())


def edge_ranks(edge_index, num_roads):
    """(in-rank, out-rank) of every edge: position among the edges of the same destination / source, ascending edge id."""
    E = edge_index.size(1)
    out = []
    for key in (edge_index[1], edge_index[0]):
        order = torch.argsort(key, stable=True)
        start = torch.zeros(num_roads + 1, dtype=torch.int64)
        start[1:] = torch.cumsum(torch.bincount(key, minlength=num_roads), 0)
        rank = torch.empty(E, dtype=torch.int64)
        rank[order] = torch.arange(E) - start[key[order]]
        out.append(rank)
    return out


def out_lists(net):
    """Every road's out-edge targets in ascending edge id (the plan's CSR order)."""
    lists = [[] for _ in range(net.num_roads)]
    for s, d in net.edge_index.t().tolist():
        lists[s].append(d)
    return lists


def plan_facts(net):
    """What ``tarl_plan_create`` derives from the topology (csrc/plan.hip), restated on the host: is the edge list source-
    sorted / destination-sorted, do rows 4c .. 4c+3 share their upstream rows (siblings4), the sizes of the row groups
    (rows with identical ordered out-lists), the length of the row-chunk table (four rows per chunk, a group's remainder
    makes a partial chunk) and whether the row pass walks it (row_siblings)."""
    N, ei = net.num_roads, net.edge_index
    ins = [[] for _ in range(N)]
    for s, d in ei.t().tolist():
        ins[d].append(s)
    sib = N >= 4 and N % 4 == 0 and all(len(ins[c + r]) == len(ins[c]) and ins[c + r][:4] == ins[c][:4]
                                        for c in range(0, N - N % 4, 4) for r in range(1, 4))
    groups = {}
    for n, lst in enumerate(out_lists(net)):
        groups.setdefault(tuple(lst), []).append(n)
    sizes = sorted(len(g) for g in groups.values())
    chunks = sum((s + 3) // 4 for s in sizes)
    return dict(src_sorted=bool((ei[0][1:] >= ei[0][:-1]).all()), dst_sorted=bool((ei[1][1:] >= ei[1][:-1]).all()),
                siblings4=sib, group_sizes=sizes, num_row_chunks=chunks, row_siblings=N >= 8 and chunks * 4 <= N + N // 4,
                max_in=max(len(l) for l in ins), max_out=max(len(key) for key in groups))


def random_state(net, seed, t):
    """``synth.random_state`` without its four-out-edges assumption: consistent FIFO prefixes of distinct agent ids,
    departures scattered around ``t`` (both admissibility branches fire), SELECTED_ROAD a random entry of the road's own
    out-list, or a non-neighbour 10 % of the time; roads without out-edges keep theirs."""
    g = torch.Generator().manual_seed(seed)
    x = net.x.clone()
    R, nmax = x.size(0), net.Nmax
    maxn = x[:, 3 * nmax].to(torch.int64)
    u = torch.rand(R, generator=g)
    n = torch.where(u < 0.15, torch.zeros_like(maxn),
                    torch.where(u > 0.85, maxn - torch.randint(0, 4, (R,), generator=g),
                                (torch.rand(R, generator=g) * maxn.float()).to(torch.int64)))
    n = torch.minimum(n.clamp(min=0), maxn - 1)      # a FIFO at MAX that receives a relief move leaves the reference's domain
    total = int(n.sum())
    ids = (torch.randperm(max(total, 1), generator=g)[:total] + 1).float()
    occ = torch.arange(nmax).unsqueeze(0) < n.unsqueeze(1)
    x[:, 0:nmax][occ] = ids
    arr = t - torch.randint(0, 40, (R, nmax), generator=g).float()
    dep = t + torch.randint(-30, 12, (R, nmax), generator=g).float()
    x[:, nmax:2 * nmax] = torch.where(occ, arr, torch.zeros_like(arr))
    x[:, 2 * nmax:3 * nmax] = torch.where(occ, dep, torch.zeros_like(dep))
    stale = (torch.rand(R, generator=g) < 0.25).unsqueeze(1) & ~occ      # the reference leaves such values behind
    x[:, 0:nmax] = torch.where(stale, torch.randint(1, 50, (R, nmax), generator=g).float(), x[:, 0:nmax])
    x[:, 3 * nmax + 1] = n.float()
    lists = out_lists(net)
    pick_u, far, bogus = torch.rand(R, generator=g), torch.randint(0, R, (R,), generator=g), torch.rand(R, generator=g) < 0.1
    for r, lst in enumerate(lists):
        if not lst:
            continue
        target = lst[int(pick_u[r] * len(lst))]
        if bool(bogus[r]):
            target = next(c for c in ((int(far[r]) + k) % R for k in range(R)) if c not in lst)
        x[r, 3 * nmax + 5] = float(target)
    return x


def population(net, per_road, seed, t0=100, t1=130):
    """``per_road`` agents per road on average, departing in ``[t0, t1]`` (synth.population: row 0 is the dummy)."""
    return synth.population(per_road * net.num_roads, net.num_roads, seed=seed, t0=t0, t1=t1)


def random_actions(net, gen, B=None):
    """One uniformly drawn out-edge per road that has any: (B, N) int32 edge ids, -1 for roads without out-edges (no
    batch dimension with ``B=None``)."""
    N, E = net.num_roads, net.edge_index.size(1)
    src = net.edge_index[0]
    _, orank = edge_ranks(net.edge_index, N)
    deg = torch.bincount(src, minlength=N)
    table = torch.full((N, int(deg.max())), -1, dtype=torch.int64)
    table[src, orank] = torch.arange(E)
    pick = (torch.rand((B or 1, N), generator=gen) * deg).long().clamp(max=(deg - 1).clamp(min=0))
    ch = torch.gather(table.unsqueeze(0).expand(B or 1, -1, -1), 2, pick.unsqueeze(-1)).squeeze(-1).to(torch.int32)
    return ch if B else ch[0]


def onehot_of(choice, E):
    a = torch.zeros(E, dtype=torch.int64)
    a[choice[choice >= 0].long()] = 1
    return a


# ---- the oracle's frame, with the branch counters and the deliberate restrictions -----------------------------------------------
def direction_masks(x, edge_index, t, Nmax):
    """The two admissibility conditions of ``sim.direction_message`` separately: (m1, m2), edge-wise."""
    c = sim.Cols(Nmax)
    x_j, x_i = x.index_select(0, edge_index[0]), x.index_select(0, edge_index[1])
    dep = x_j[:, c.HEAD_DEP]
    heads_here = x_j[:, c.SEL] == x_i[:, c.ROAD]
    m1 = (dep <= t) & (x_i[:, c.N] < x_i[:, c.MAXN] - sim.CONGESTION_FILE) & heads_here & (x_j[:, c.N] > 0)
    m2 = ((dep - t < -10) & (x_j[:, c.MAXN] - sim.CONGESTION_FILE <= x_j[:, c.N])
          & (x_j[:, c.MAXN] - x_j[:, c.N] <= x_i[:, c.MAXN] - x_i[:, c.N]) & heads_here)
    return m1, m2


def segment_argmax_last(scores, index, n):
    """``sim.segment_argmax_first`` with the tie order reversed: the HIGHEST edge id among the maxima."""
    E = scores.numel()
    mx = scores.new_full((n,), float("-inf")).scatter_reduce_(0, index, scores, reduce="amax", include_self=True)
    cand = torch.where(scores == mx[index], torch.arange(E), torch.full((E,), -1))
    arg = torch.full((n,), -1, dtype=torch.long).scatter_reduce_(0, index, cand, reduce="amax", include_self=True)
    return torch.where(arg < 0, torch.full_like(arg, E), arg)


COUNTERS = ("a_tail_admissible", "b_tail_in_race", "c_tail_wins", "d_tail_response", "e_relief_admissions")
SHORT_IN = "f_short_in_admissions"      # counted beside COUNTERS: admissions into a road of in-degree 1 to 3


def sibling0_tail_edges(edge_index, num_roads):
    """``edge_index`` with the source of every in-edge of in-rank >= 4 into a road 4c + r, r > 0, replaced by the source of
    road 4c's in-edge of the same in-rank (where road 4c has one): the in-lists a kernel would walk that shared the WHOLE
    in-list between siblings, not only its first four entries."""
    irank, _ = edge_ranks(edge_index, num_roads)
    dst = edge_index[1]
    slot = torch.full((num_roads, int(irank.max()) + 1), -1, dtype=torch.int64)
    slot[dst, irank] = edge_index[0]
    lead = slot[dst - dst % 4, irank]
    swap = (irank >= 4) & (dst % 4 != 0) & (lead >= 0)
    return torch.stack([torch.where(swap, lead, edge_index[0]), dst])


def core_step_counted(x, net, t, uniform, counters, *, drop_in_tail=False, drop_out_tail=False, last_max=False,
                      sibling0_tail=False, edge_attr=None):
    """``sim.core_step`` on ``x`` (in place), restated from the oracle's own pieces so that the branches it takes can be
    counted into ``counters`` (see :func:`census`) and ONE restriction applied: ``drop_in_tail`` removes every in-edge of
    in-rank >= 4 from the Direction message, ``drop_out_tail`` every out-edge of out-rank >= 4 from the Response message,
    ``last_max`` breaks ties of the Gumbel race by the last maximum, ``sibling0_tail`` evaluates the Direction message of
    every in-edge of in-rank >= 4 on the source sibling 0 has at that rank (:func:`sibling0_tail_edges`: the identity where
    siblings share their whole in-list). Without a restriction it IS ``sim.core_step`` (the host suite asserts that).
    Returns (delta_travel_time, popped)."""
    ei, Nmax, R = net.edge_index, net.Nmax, net.num_roads
    ea = (net.edge_attr if edge_attr is None else edge_attr).reshape(-1)
    irank, orank = edge_ranks(ei, R)
    in_tail, out_tail = irank >= 4, orank >= 4
    ei_dir = sibling0_tail_edges(ei, R) if sibling0_tail else ei
    agent_id, prob, dtt = sim.direction_message(x, ei_dir, ea, t, Nmax)
    m1, m2 = direction_masks(x, ei_dir, t, Nmax)
    assert torch.equal(prob, ea * (m1 | m2).float())
    if drop_in_tail:
        prob = torch.where(in_tail, torch.zeros_like(prob), prob)
    adm = prob > 0
    scores = torch.log(prob + sim.EPS) + sim.gumbel_from_uniform(uniform)
    P = torch.zeros(R).index_add_(0, ei[1], prob)
    arg = (segment_argmax_last if last_max else sim.segment_argmax_first)(scores, ei[1], R)
    chosen = torch.zeros(R)
    has = P > 0
    chosen[has] = agent_id[arg[has]]
    if not (drop_in_tail or last_max):
        assert torch.equal(chosen, sim.direction_aggregate(agent_id, prob, ei[1], R, uniform=uniform))
    racers = torch.zeros(R, dtype=torch.int64).index_add_(0, ei[1], adm.long())
    win = arg[has]
    counters["a_tail_admissible"] += int((adm & in_tail).sum())
    counters["b_tail_in_race"] += int((adm & in_tail & (racers[ei[1]] >= 2)).sum())
    counters["c_tail_wins"] += int(in_tail[win].sum())
    counters["e_relief_admissions"] += int((m2 & ~m1)[win].sum())
    din = torch.bincount(ei[1], minlength=R)
    counters[SHORT_IN] += int((has & (din >= 1) & (din <= 3)).sum())
    sim.direction_update(x, chosen, t, Nmax, net.congestion_constant)
    msg = sim.response_message(x, ei, Nmax)
    counters["d_tail_response"] += int(((msg > 0) & out_tail).sum())
    if drop_out_tail:
        keep = ~out_tail
        _, popped = sim.response_step(x, ei[:, keep], Nmax)
    else:
        _, popped = sim.response_step(x, ei, Nmax)
    return dtt, popped


def env_step_counted(x, agents, net, adj, action, t, uniform, counters, **restrict):
    """``sim.env_step`` with :func:`core_step_counted` as its core step. Returns the reward."""
    c = sim.Cols(net.Nmax)
    sim.apply_action(x, net.edge_index, action, net.Nmax)
    dtt, popped = core_step_counted(x, net, t, uniform, counters, **restrict)
    _, withdrawn = sim.withdraw(x, agents, adj, t, net.Nmax)
    sim.insert(x, agents, t, net.Nmax, net.congestion_constant)
    return (-torch.sum(x[:, c.N])).flatten()


def new_counters():
    return {k: 0 for k in COUNTERS + (SHORT_IN,)}


def census_inputs(net, T, seed):
    """The seeded inputs of a census run: per frame (action one-hot (E,), uniforms (E,))."""
    gen = torch.Generator().manual_seed(seed)
    E = net.edge_index.size(1)
    return [(onehot_of(random_actions(net, gen), E), torch.rand(E, generator=gen)) for _ in range(T)]


def census(net, pop, T, seed, t0=100):
    """``T`` frames of ``oracle.sim.env_step`` from the empty network with population ``pop``, uniform random valid actions
    (one out-edge per road that has any) and seeded uniforms. Returns (frames, counters): per frame the state, the agent
    table and the reward after it; the counters over all frames —
    a_tail_admissible: admissible in-edges of in-rank >= 4; b_tail_in_race: those of them in a race of >= 2 admissible
    edges; c_tail_wins: races won by such an edge; d_tail_response: Response messages that fire on an out-edge of out-rank
    >= 4; e_relief_admissions: agents admitted through the second (gridlock-relief) condition only; f_short_in_admissions:
    agents admitted into a road of in-degree 1 to 3 (whose NodeRec::in4 ends in padding); max_count: the largest FIFO count
    seen; done: agents that arrived. The counters come from a shadow copy of each frame run through
    :func:`core_step_counted`, which must leave the state ``sim.env_step`` leaves."""
    x, ag = net.x.clone(), pop.clone()
    xs, ags = x.clone(), pop.clone()
    adj = net.dense_adjacency()
    col_n = 3 * net.Nmax + 1
    counters, frames, max_count = new_counters(), [], 0
    for s, (action, u) in enumerate(census_inputs(net, T, seed)):
        out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, t0 + s, net.Nmax, uniform=u,
                           congestion_constant=net.congestion_constant)
        rw = env_step_counted(xs, ags, net, adj, action, t0 + s, u, counters)
        assert torch.equal(x, xs) and torch.equal(ag, ags) and torch.equal(rw, out["reward"])
        max_count = max(max_count, int(x[:, col_n].max()))
        frames.append((x.clone(), ag.clone(), out["reward"].clone()))
    counters["max_count"] = max_count
    counters["done"] = int(ag[:, sim.DONE].sum())
    return frames, counters


def replay_restricted(net, pop, T, seed, frames, t0=100, **restrict):
    """The census run again with one restriction of :func:`core_step_counted`: the first frame whose state or agent table
    differs from the true run's ``frames`` (None: the restriction was never noticed)."""
    x, ag = net.x.clone(), pop.clone()
    adj = net.dense_adjacency()
    scratch = new_counters()
    for s, (action, u) in enumerate(census_inputs(net, T, seed)):
        env_step_counted(x, ag, net, adj, action, t0 + s, u, scratch, **restrict)
        if not (torch.equal(x, frames[s][0]) and torch.equal(ag, frames[s][1])):
            return s
    return None


# ---- long FIFOs: counts, ring offsets and insert positions beyond 63 ---------------------------------------------------------------
INS_CAP = 192      # csrc/fused_common.h: ready agents per frame the insert kernel keeps in LDS; more go through global scratch
LONG_COUNTERS = ("count_ge64", "at_max", "at_last_slot", "offset_ge64", "rings_wrapped", "insert_pos_ge64", "insert_frames_ge64",
                 "withdraw_ge2",
                 "e_relief_admissions", "max_count", "done", "due_frame0", "max_inserted_frame0")


def masked_counts(x, Nmax, mask):
    """A copy of ``x`` whose NUMBER_OF_AGENT column is read through ``& mask``."""
    xm = x.clone()
    xm[:, 3 * Nmax + 1] = (x[:, 3 * Nmax + 1].to(torch.int64) & mask).float()
    return xm


def core_step_count_masked(x, net, t, uniform, mask):
    """``sim.core_step`` on ``x`` (in place) whose Direction and Response MESSAGES read every count through ``& mask``
    (:func:`masked_counts`); the update and the pop work on the true counts. With ``mask = -1`` it is ``sim.core_step``."""
    ei, Nmax, R = net.edge_index, net.Nmax, net.num_roads
    agent_id, prob, _ = sim.direction_message(masked_counts(x, Nmax, mask), ei, net.edge_attr.reshape(-1), t, Nmax)
    chosen = sim.direction_aggregate(agent_id, prob, ei[1], R, uniform=uniform)
    sim.direction_update(x, chosen, t, Nmax, net.congestion_constant)
    msg = sim.response_message(masked_counts(x, Nmax, mask), ei, Nmax)
    popped = torch.zeros(R).scatter_reduce_(0, ei[0], msg, reduce="amax", include_self=False) > 0
    for base in (0, Nmax, 2 * Nmax):      # the pop of sim.response_step
        x[popped, base:base + Nmax - 1] = x[popped, base + 1:base + Nmax]
    x[popped, 3 * Nmax + 1] -= 1
    return popped


def insert_capacity_masked(x, agents, t, net, mask):
    """``sim.insert`` whose CAPACITY is computed from ``count & mask`` (positions and travel times from the true count), by
    the oracle's own function on a state whose MAX_NUMBER_OF_AGENT is raised by what the mask hides — the congestion time is
    a function of MAX - count, so it is then put right from the true MAX; an agent that would land behind the last slot is
    not kept (a narrowed mask cannot index outside a row). With ``mask = -1`` it is ``sim.insert``."""
    Nmax = net.Nmax
    c = sim.Cols(Nmax)
    n0 = x[:, c.N].clone()
    hidden = n0 - (n0.to(torch.int64) & mask).float()
    room = torch.minimum(x[:, c.MAXN] - sim.CONGESTION_FILE - (n0 - hidden), Nmax - n0)      # capacity, clamped to the row
    true_max = x[:, c.MAXN].clone()
    x[:, c.MAXN] = n0 + room + sim.CONGESTION_FILE
    sim.insert(x, agents, t, Nmax, None)
    x[:, c.MAXN] = true_max
    n1 = x[:, c.N]
    for r in torch.nonzero(n1 > n0).view(-1).tolist():      # departure = t + max(free flow, congestion time at the true count)
        a, b = int(n0[r]), int(n1[r])
        t_cong = net.congestion_constant[r] / (x[r, c.MAXN] + 10 - n0[r])
        x[r, 2 * Nmax + a:2 * Nmax + b] = float(t) + torch.maximum(x[r, c.FF], t_cong)


def env_step_long(x, agents, net, adj, action, t, uniform, stats, hoff, *, message_mask=None, capacity_mask=None):
    """``sim.env_step`` from the oracle's own pieces, with what the long-FIFO tests count added into ``stats`` and the
    host-derived ring offsets ``hoff`` (R,) advanced: a road's offset is the number of agents that left its head since the
    start (pops and withdrawals) modulo Nmax — where a ring buffer packed at offset 0 keeps its head. ``message_mask`` /
    ``capacity_mask``: ONE restriction of :func:`core_step_count_masked` / :func:`insert_capacity_masked`. Returns the
    reward."""
    Nmax = net.Nmax
    c = sim.Cols(Nmax)
    sim.apply_action(x, net.edge_index, action, Nmax)
    if message_mask is None:
        _, popped = core_step_counted(x, net, t, uniform, stats["branches"])
    else:
        popped = core_step_count_masked(x, net, t, uniform, message_mask)
    n_core = x[:, c.N].clone()
    sim.withdraw(x, agents, adj, t, Nmax)
    gone = n_core - x[:, c.N]
    n_wd = x[:, c.N].clone()
    if capacity_mask is None:
        sim.insert(x, agents, t, Nmax, net.congestion_constant)
    else:
        insert_capacity_masked(x, agents, t, net, capacity_mask)
    n = x[:, c.N]
    left = popped.long() + gone.long()
    stats["rings_wrapped"] |= hoff + left >= Nmax
    hoff.copy_((hoff + left) % Nmax)
    stats["count_ge64"] += int((n >= 64).sum())
    stats["at_max"] += int((n >= x[:, c.MAXN]).sum())
    stats["at_last_slot"] += int((n == Nmax - 1).sum())
    stats["offset_ge64"] += int((hoff >= 64).sum())
    stats["insert_pos_ge64"] += int((n - torch.maximum(n_wd, torch.full_like(n, 64.0))).clamp(min=0).sum())
    stats["insert_frames_ge64"] += int(((n > n_wd) & (n > 64)).sum())
    stats["withdraw_ge2"] += int((gone >= 2).sum())
    stats["max_count"] = max(stats["max_count"], int(n.max()))
    stats["max_inserted"] = int((n - n_wd).max())
    return (-torch.sum(n)).flatten()


def new_long_stats(net):
    stats = {k: 0 for k in LONG_COUNTERS}
    stats["branches"] = new_counters()
    stats["rings_wrapped"] = torch.zeros(net.num_roads, dtype=torch.bool)
    return stats


def long_fifo_counters(net, pop, T, seed, t1, t0=100):
    """The census run (:func:`census`: ``T`` frames of ``sim.env_step`` from the empty network, population ``pop`` due in
    ``[t0, t1]``, the seeded actions and uniforms of :func:`census_inputs`) with the counters of the long-FIFO tests. Returns
    (frames, counters): per frame the state, the agent table and the reward; over all frames and roads —
    count_ge64: road-frames that end with a count >= 64; at_max: those with count >= MAX_NUMBER_OF_AGENT; at_last_slot: those
    with count == Nmax - 1 (the packed row turns DIRTY); offset_ge64: road-frames whose host-derived ring offset
    (:func:`env_step_long`) is >= 64; rings_wrapped: per road (bool), that offset passed Nmax; insert_pos_ge64: agents the
    insert put at FIFO position >= 64; insert_frames_ge64: road-frames in which it put one there; withdraw_ge2: road-frames in which two or more agents arrived; e_relief_admissions:
    as :func:`census`; max_count: the largest count a frame ends with; done: agents that arrived; due_frame0: agents due at
    ``t0``; max_inserted_frame0: the most agents one road received in frame 0. Every frame is asserted equal to
    ``sim.env_step``'s."""
    assert float(pop[1:, sim.DEPARTURE_TIME].min()) >= t0 and float(pop[1:, sim.DEPARTURE_TIME].max()) <= t1
    x, ag = net.x.clone(), pop.clone()
    xs, ags = x.clone(), pop.clone()
    adj = net.dense_adjacency()
    stats, hoff, frames = new_long_stats(net), torch.zeros(net.num_roads, dtype=torch.int64), []
    stats["due_frame0"] = int((pop[1:, sim.DEPARTURE_TIME] <= t0).sum())
    for s, (action, u) in enumerate(census_inputs(net, T, seed)):
        out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, t0 + s, net.Nmax, uniform=u,
                           congestion_constant=net.congestion_constant)
        rw = env_step_long(xs, ags, net, adj, action, t0 + s, u, stats, hoff)
        assert torch.equal(x, xs) and torch.equal(ag, ags) and torch.equal(rw, out["reward"])
        if s == 0:
            stats["max_inserted_frame0"] = stats["max_inserted"]
        frames.append((x.clone(), ag.clone(), out["reward"].clone()))
    stats["e_relief_admissions"] = stats["branches"]["e_relief_admissions"]
    stats["done"] = int(ag[:, sim.DONE].sum())
    return frames, {k: stats[k] for k in LONG_COUNTERS}


def replay_long_restricted(net, pop, T, seed, frames, t0=100, **restrict):
    """The run of :func:`long_fifo_counters` again with one restriction of :func:`env_step_long` (``message_mask=63``: the
    Direction and Response messages read the counts through ``& 63``; ``capacity_mask=63``: the insert computes its
    capacity from ``count & 63``; a mask of -1 hides nothing): the first frame whose state or agent table differs from ``frames`` (None: never)."""
    x, ag = net.x.clone(), pop.clone()
    adj = net.dense_adjacency()
    stats, hoff = new_long_stats(net), torch.zeros(net.num_roads, dtype=torch.int64)
    for s, (action, u) in enumerate(census_inputs(net, T, seed)):
        env_step_long(x, ag, net, adj, action, t0 + s, u, stats, hoff, **restrict)
        if not (torch.equal(x, frames[s][0]) and torch.equal(ag, frames[s][1])):
            return s
    return None


# ---- a crafted tie across the 4 / 5 boundary of a nine-edge race ----------------------------------------------------------------
def tie_case(net, x, t, in_degree=9, which=0, ranks=(3, 4)):
    """Edit ``x`` (in place) and return (edge_attr, e3, e4, road): a road with ``in_degree`` in-edges — the ``which``-th of
    them in ascending road id — whose in-edges of rank 3 and 4 — the last record embedded in NodeRec::in4 and the first of
    the tail loop — are both admissible at time ``t`` and carry the SAME turn probability; with equal Gumbel noise on the
    two (and less on the others) their scores are bit-equal maxima, and the reference's first-maximum rule admits the head
    of rank 3's road. ``ranks``: another pair of in-ranks (a graph without in-lists longer than four)."""
    ei, nmax = net.edge_index, net.Nmax
    c = sim.Cols(nmax)
    din, _ = degrees(net)
    road = int(torch.nonzero(din == in_degree)[which])
    eids = torch.nonzero(ei[1] == road).view(-1)
    e3, e4 = int(eids[ranks[0]]), int(eids[ranks[1]])
    ea = net.edge_attr.clone()
    ea[e4] = ea[e3]
    x[road, c.N] = torch.minimum(x[road, c.N], x[road, c.MAXN] - sim.CONGESTION_FILE - 1)      # room downstream
    fresh = float(x[:, :nmax].max()) + 1.0
    for k, e in enumerate((e3, e4)):
        j = int(ei[0, e])
        assert j != road
        if x[j, c.N] == 0:                # an empty upstream road gets somebody: an id nobody else carries
            x[j, c.N], x[j, 0], x[j, nmax] = 1.0, fresh + k, t - 20.0
        x[j, 2 * nmax] = t - 1.0          # head due
        x[j, c.SEL] = float(road)
    return ea, e3, e4, road


def tie_uniform(u, net, road, e3, e4):
    """``u`` with the uniforms of ``road``'s in-edges capped below 0.9 and 0.999 on both tied edges."""
    u = u.clone()
    mine = net.edge_index[1] == road
    u[..., mine] = u[..., mine] * 0.9
    u[..., e3] = 0.999
    u[..., e4] = 0.999
    return u
