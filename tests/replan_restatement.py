"""TEST INFRASTRUCTURE: numpy / torch restatement of the day-to-day replanning: the quickest time-dependent ROUTE
per (environment, agent) (``tarl_td_routes``), the route-following select rule (``tarl_fused_select_route``) on an exported ``x``
plus agent table, and the day loop of ``tarl_hip.replanning.Replanner`` on ``oracle.sim.env_step`` in the shape of
``router_hold_restatement.replay`` — each also with ONE deliberate defect at a time (:data:`DEFECTS`). ``leave``, the road times,
the crafted cases and the enumeration of paths are ``dynamic_gap_restatement``'s, imported, not restated; the labels are its
heap search kept whole (``labels``; the host suite checks ``labels(...)[d] == hindsight_one(...)`` on every case). Plain module:
no fixtures; nothing at import time needs a GPU.

The route: with L the labels of the search from road o entered at t0, walk back from d; at v != o take the in-neighbour u with
leave(v, L[u]) == L[v] (fp64 equality), among several the SMALLEST ROAD ID; stop at o; the route is stored forward. len 0: d
unreachable (or no tight in-edge); -(true length): longer than max_hops; -1: more than N roads.
The select rule, for row i with head agent h (x[i][0]), r = routes[h], len = route_len[h]: untouched where h is out of range,
len <= 0 or len > max_hops, or no j < len has r[j] == i; else with the smallest such j: i itself for j == len - 1, else r[j + 1],
and i itself where r[j + 1] == r[len - 1] (the hold rule)."""
from __future__ import annotations

import heapq

import numpy as np
import torch

import dynamic_gap_restatement as G
from dynamic_gap_restatement import INF, leave

DEFECTS = ("largest_id_tie", "first_in_list_tie", "stops_after_four_in_edges",            # the walk
           "no_hold", "holds_two_short", "first_match_from_the_end",                      # the select rule
           "shared_plan_for_every_env", "swap_mask_ignored")                              # the day loop
ORIGIN, DEST, DEP, DONE = G.ORIGIN, G.DEST, G.DEP, G.DONE


# ---- the route -------------------------------------------------------------------------------------------------------------------
def in_lists(edge_index, N):
    """The sources of every road's in-edges, in the order of the edge list."""
    lists = [[] for _ in range(N)]
    for s, d in np.asarray(edge_index).T.tolist():
        lists[int(d)].append(int(s))
    return lists


def labels(outs, tau_k, env_k, o, t0, bin_seconds, first_bin):
    """``dynamic_gap_restatement.hindsight_one`` without a defect, returning every label instead of L[d]."""
    L = [INF] * len(outs)
    L[o] = leave(tau_k, env_k, o, t0, bin_seconds, first_bin)
    heap = [(L[o], o)] if L[o] < INF else []
    while heap:
        lu, u = heapq.heappop(heap)
        if lu > L[u]:
            continue
        for v in outs[u]:
            lv = leave(tau_k, env_k, v, lu, bin_seconds, first_bin)
            if lv < L[v]:
                L[v] = lv
                heapq.heappush(heap, (lv, v))
    return L


def walk(ins, tau_k, env_k, L, o, d, bin_seconds, first_bin, max_hops, defect=None):
    """-> (route_len, the route o .. d as a list; empty where there is none)."""
    if not L[d] < INF:
        return 0, []
    path, v = [d], d
    while v != o:
        cands = ins[v][:4] if defect == "stops_after_four_in_edges" else ins[v]
        tight = [u for u in cands if leave(tau_k, env_k, v, L[u], bin_seconds, first_bin) == L[v]]
        if not tight:
            return 0, []
        v = max(tight) if defect == "largest_id_tie" else tight[0] if defect == "first_in_list_tie" else min(tight)
        path.append(v)
        if len(path) > len(ins):
            return -1, []
    if len(path) > max_hops:
        return -len(path), []
    return len(path), path[::-1]


def planned(row, a, N):
    """(origin, destination) of an agent row that gets a plan (whatever its DONE flag), else ``None``."""
    o, d = float(row[ORIGIN]), float(row[DEST])
    if a < 1 or not (0.0 <= o < N) or not (0.0 <= d < N):
        return None
    return int(o), int(d)


def routes(edge_index, N, tau, env, agents, bin_seconds, first_bin, max_hops, defect=None):
    """``tarl_td_routes`` -> (best fp64 (K, A), routes int32 (K, A, max_hops) with -1 from the length on, route_len int32 (K, A)).
    Equal searches (environment, origin, destination, departure) are computed once."""
    K, A, _ = agents.shape
    outs, ins = G.out_lists(edge_index, N), in_lists(edge_index, N)
    best = np.full((K, A), INF)
    rt = np.full((K, A, max_hops), -1, np.int32)
    ln = np.zeros((K, A), np.int32)
    for k in range(K):
        seen = {}
        for a in range(A):
            od = planned(agents[k, a], a, N)
            if od is None:
                continue
            key = (od, float(agents[k, a, DEP]))
            if key not in seen:
                L = labels(outs, tau[k], env[k], od[0], key[1], bin_seconds, first_bin)
                seen[key] = (L[od[1]],) + walk(ins, tau[k], env[k], L, od[0], od[1], bin_seconds, first_bin, max_hops, defect)
            best[k, a], n, path = seen[key]
            ln[k, a] = n
            rt[k, a, :len(path)] = path
    return best, rt, ln


def is_path(outs, path, o, d):
    return len(path) >= 1 and path[0] == o and path[-1] == d and all(v in outs[u] for u, v in zip(path, path[1:]))


# ---- the select rule ---------------------------------------------------------------------------------------------------------------
def select_rule(x, rt, ln, defect=None):
    """One environment: ``x`` (N, F) exported state, ``rt`` (A, L) and ``ln`` (A,) its plan -> (written (N,) bool, value (N,)
    float64: the SELECTED_ROAD the rule writes, 0 where it writes nothing)."""
    N, A, Lmax = x.shape[0], rt.shape[0], rt.shape[1]
    written, value = np.zeros(N, bool), np.zeros(N)
    heads = np.asarray(x[:, 0], dtype=np.float64)
    for i in range(N):
        h = int(heads[i])
        if not 0 <= h < A:
            continue
        n = int(ln[h])
        if n <= 0 or n > Lmax:
            continue
        r = [int(v) for v in rt[h, :n]]
        where = [j for j in range(n) if r[j] == i]
        if not where:
            continue
        j = where[-1] if defect == "first_match_from_the_end" else where[0]
        nh = i
        if j < n - 1:
            nh = r[j + 1]
            if nh == r[n - 1] and defect != "no_hold":
                nh = i
            elif defect == "holds_two_short" and j + 2 <= n - 1 and r[j + 2] == r[n - 1]:
                nh = i
        written[i], value[i] = True, float(nh)
    return written, value


# ---- the day loop ------------------------------------------------------------------------------------------------------------------
def day_seed(seed, day):
    return (int(seed) * 1000003 + int(day) * 7919 + 12345) & ((1 << 63) - 1)


def relative_gap(edges, N, veh, fpb, road, tables, bin_seconds, first_bin):
    """RG per environment of one day, fp64, from the day's own occupancy sums: the evaluator's dynamic gap restated."""
    tau, env = G.road_times(veh, fpb, *road, bin_seconds, first_bin)
    best = G.hindsight(edges, N, tau, env, tables, bin_seconds, first_bin)
    H = veh.shape[1]
    dep_bin = np.array([G.clock_bin(t, bin_seconds, first_bin, H) for t in tables[0, :, DEP]])
    _, per_env, _ = G.reductions(tables, best, dep_bin, H)
    return G.relative_gaps(per_env)


def day_loop(net, pop, K, T, days, fraction, max_hops, bin_seconds, seed, gumbel_of, t_start, per_env=True, defect=None,
             fallback=True):
    """``Replanner(engine, days=, fraction=, max_hops=, link_bin_seconds=bin_seconds, seed=, per_env=).run(T)`` on the CPU oracle.
    ``gumbel_of(b, t)``: the Gumbel values of environment b at frame t, the same on every day. Every frame, as the "routes" head
    of the evaluator: ``router_hold_restatement.hold_choice`` on the free-flow table of the empty network writes every row
    (``fallback``), then the select rule overrides the rows whose head is on its route. SELECTED_ROAD survives the reset
    between two days (the packed state keeps its bytes); ARRIVAL_TIME too. -> one dict per day: routes, route_len (the plan the
    day ran with, (P, A, L) and (P, A)), mask (the switch mask drawn after it, None on the last day), differs, agents (K, A, 9),
    returns (K,), travel_time (K,: mean over the arrived, None without one), arrived, rg, veh."""
    import router_hold_restatement as HR
    from baseline_restatement import destination_columns
    from oracle import routing, sim
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    adj = net.dense_adjacency()
    edges = ei.numpy()
    A = pop.size(0)
    empty = net.x.clone()
    empty[:, :3 * Nmax] = 0
    empty[:, c.N] = 0
    dests = sorted({int(d) for d in pop[:, 1].tolist() if 0 <= d < N})
    table = destination_columns(ei, routing.edge_travel_time(empty, ei, net.congestion_constant, Nmax), N, dests)
    P = K if per_env else 1
    first = int(t_start) // bin_seconds
    H = (int(t_start) + T - 1) // bin_seconds - first + 1
    fpb = np.bincount((int(t_start) + np.arange(T)) // bin_seconds - first, minlength=H).astype(np.int32)
    c3 = 3 * Nmax
    road = (net.x[:, c3].numpy(), net.x[:, c3 + 2].numpy(), net.congestion_constant.numpy())
    xs = [net.x.clone() for _ in range(K)]
    ags = [pop.clone() for _ in range(K)]
    no_action = torch.zeros(ei.size(1), dtype=torch.long)
    acc = np.zeros((P, H, N), np.int64)

    def plan(days_so_far):
        scale = days_so_far * (1 if per_env else K)
        tau, env = G.road_times(acc.astype(np.int32), (fpb.astype(np.int64) * scale).astype(np.int32), *road, bin_seconds, first)
        tables = np.stack([a.numpy() for a in ags[:P]])
        return routes(edges, N, tau, env, tables, bin_seconds, first, max_hops)

    _, cur_r, cur_l = plan(1)
    out = []
    for day in range(days):
        veh = np.zeros((K, H, N), np.int32)
        returns = []
        for b in range(K):
            x, ag = xs[b], ags[b]
            x[:, :3 * Nmax] = 0
            x[:, c.N] = 0
            ag[:, sim.ON_WAY] = 0
            ag[:, sim.DONE] = 0
            p = 0 if (not per_env or defect == "shared_plan_for_every_env") else b
            total = 0.0
            for t in range(T):
                if fallback:
                    x = HR.hold_choice(x, ag, table, Nmax)
                written, value = select_rule(x.numpy(), cur_r[p], cur_l[p])
                x[:, c.SEL] = torch.where(torch.from_numpy(written), torch.from_numpy(value).to(x.dtype), x[:, c.SEL])
                res = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, float(t_start + t), Nmax, gumbel=gumbel_of(b, t),
                                   congestion_constant=net.congestion_constant)
                total += float(res["reward"])
                veh[b, (int(t_start) + t) // bin_seconds - first] += x[:, c.N].numpy().astype(np.int32)
            returns.append(total)
            xs[b] = x
        tables = np.stack([a.numpy().copy() for a in ags])
        arrived = [int(tb[1:, DONE].sum()) for tb in tables]
        tt = [float((tb[1:, G.ARR] - tb[1:, DEP])[tb[1:, DONE] == 1].astype(np.float64).mean()) if n else None
              for tb, n in zip(tables, arrived)]
        rec = dict(routes=cur_r.copy(), route_len=cur_l.copy(), agents=tables, returns=returns, arrived=arrived, travel_time=tt,
                   veh=veh, rg=relative_gap(edges, N, veh, fpb, road, tables, bin_seconds, first), mask=None)
        acc += veh if per_env else veh.sum(axis=0, keepdims=True)
        _, new_r, new_l = plan(day + 1)
        live = np.arange(max_hops)[None, None, :] < np.maximum(new_l, 0)[..., None]
        rec["differs"] = (cur_l != new_l) | ((cur_r != new_r) & live).any(-1)
        if day + 1 < days:
            prob = 1.0 / (day + 2) if fraction == "msa" else float(fraction)
            g = torch.Generator().manual_seed(day_seed(seed, day))
            mask = (torch.rand((P, A), generator=g) < prob).numpy() | (cur_l <= 0)
            if defect == "swap_mask_ignored":
                mask = np.ones_like(mask)
            rec["mask"] = mask
            cur_r = np.where(mask[..., None], new_r, cur_r)
            cur_l = np.where(mask, new_l, cur_l)
        out.append(rec)
    return out


# ---- crafted cases -----------------------------------------------------------------------------------------------------------------
def tie_case():
    """Seven roads, uniform road times (tau = 10, one bin): 0 -> {3, 1, 2} -> 4 -> 5, listed in that order, and 6 -> 4 between
    them: road 4 has the in-list [3, 6, 1, 2], three of them tight, whose smallest source (1) is neither first (3) nor last (2);
    road 6 has no in-edge, so it is unreachable as a destination and its edge into 4 is never tight."""
    N = 7
    edges = np.array([[0, 0, 0, 3, 6, 1, 2, 4], [3, 1, 2, 4, 4, 4, 4, 5]], dtype=np.int64)
    rows = [(0, 5, 100, (1,)), (0, 5, 100, (1,)), (0, 4, 105, (0,)), (1, 5, 100, (1,)), (5, 5, 100, (0,)), (0, 6, 100, (1,)),
            (4, 0, 100, (1,))]
    return dict(name="tie", N=N, K=1, H=1, bin_seconds=1000, first_bin=0, edges=edges, veh=np.zeros((1, 1, N), np.int32),
                frames_per_bin=np.array([4], np.int32), max_agents=np.full(N, 10, np.float32),
                free_flow=np.full(N, 10, np.float32), cong=np.full(N, 190, np.float32), agents=G._agents(1, rows), want=None,
                must=())


def late_tie_case():
    """Eight roads: road 7 has SIX in-edges, from 1 .. 6 in that order, of which only those from 5 and 6 are tight (roads 1 .. 4
    are slower): a walk that looks at the first four in-edges alone finds no predecessor."""
    N = 8
    srcs = [1, 2, 3, 4, 5, 6]
    edges = np.array([[0] * 6 + srcs, srcs + [7] * 6], dtype=np.int64)
    ff = np.array([10, 30, 30, 30, 30, 10, 10, 10], np.float32)
    rows = [(0, 7, 50, (1,)), (0, 7, 50, (1,)), (0, 7, 61, (1,))]
    return dict(name="late-tie", N=N, K=1, H=1, bin_seconds=1000, first_bin=0, edges=edges, veh=np.zeros((1, 1, N), np.int32),
                frames_per_bin=np.array([4], np.int32), max_agents=np.full(N, 10, np.float32), free_flow=ff,
                cong=(ff * 19).astype(np.float32), agents=G._agents(1, rows), want=None, must=())


def route_cases():
    """The crafted cases of ``dynamic_gap_restatement`` (at most 6 roads each: the enumeration of paths checks them) and the two
    tie cases above."""
    return G.crafted_cases() + [tie_case(), late_tie_case()]


def run_routes(case, max_hops=8, defect=None):
    tau, env = G.road_times(case["veh"], case["frames_per_bin"], case["max_agents"], case["free_flow"], case["cong"],
                            case["bin_seconds"], case["first_bin"])
    return (tau, env) + routes(case["edges"], case["N"], tau, env, case["agents"], case["bin_seconds"], case["first_bin"],
                               max_hops, defect)


def select_case():
    """Six rows, agent i + 1 heads row i, hand-made plans: agent 1 follows 0 1 2 0 3 5 — row 0 appears twice, the first match
    is followed by 1, the match from the end by 3; agent 2 follows 1 2 3 (row 1 is TWO short of 3: next 2); agent 3 follows 2 3
    (row 2 is one short: it holds, 2); agent 4 stands on its destination 3 (3); agent 5 (row 4) has no route and agent 6
    (row 5) a route that does not hold row 5: both rows untouched. Agent 7 heads nothing."""
    N, Nmax = 6, 4
    F = 3 * Nmax + 7
    x = np.zeros((N, F), np.float32)
    for i in range(N):
        x[i, 0] = i + 1
        x[i, 3 * Nmax + 1] = 1
        x[i, 3 * Nmax + 5] = -9.0
    rt = np.full((8, 6), -1, np.int32)
    ln = np.zeros(8, np.int32)
    plans = {1: [0, 1, 2, 0, 3, 5], 2: [1, 2, 3], 3: [2, 3], 4: [3], 6: [0, 1, 2]}
    for a, p in plans.items():
        rt[a, :len(p)], ln[a] = p, len(p)
    want = {0: 1.0, 1: 2.0, 2: 2.0, 3: 3.0}        # rows 4 and 5 untouched
    return dict(x=x, routes=rt, route_len=ln, want=want, N=N, Nmax=Nmax)
