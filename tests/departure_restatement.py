"""TEST INFRASTRUCTURE: first-hop routing written out on the CPU: on the exported ``x`` (N, F) and agent table
(A, 9) of ONE environment, with a next-hop table ``table[row][destination]`` (N, N) — ``baseline_restatement``'s orientation —
or the route arrays of ``replan_restatement``. Nothing here calls the code under test. Each piece is also available with ONE
defect at a time (:data:`DEFECTS`), and :func:`replay` is ``router_hold_restatement.replay`` with the rule between the hold
router's choice and ``oracle.sim.env_step``.

The rule, in the frame whose clock is t: agent a is READY as ``oracle.sim.insert`` has it (DEPARTURE_TIME <= t, not on the way,
not done; every row counts, agent 0 too); pend(u) = the smallest ready id with ORIGIN == u, else -1; road u is ROUTED when its
count is 0 and pend(u) >= 0. Table lookup with p = pend(u): d = DESTINATION of p outside [0, N) -> untouched; d without a slot
-> untouched; nh = table[u][d] < 0 -> untouched; nh == d -> u; SELECTED_ROAD[u] = nh. Plan lookup: ``replan_restatement``'s
select rule with p as the head."""
import numpy as np
import torch

ORIGIN, DEST, DEP, ON_WAY, DONE = 0, 1, 2, 7, 8

DEFECTS = ("first_in_departure_order",   # pend = the ready agent that departs first (ties: the smaller id), not the smallest id
           "nonempty_rows_routed",       # the count is not looked at
           "status_ignored",             # on-the-way and done agents count as ready
           "strict_less",                # DEPARTURE_TIME < t
           "no_hold",                    # the next hop is written even where it is the destination
           "table_transposed",           # table[d][u]
           "minus_one_written",          # an unreachable destination writes -1
           "plan_no_hold")               # the plan lookup without its hold


def _cols():
    from oracle import sim
    assert (sim.ORIGIN, sim.DESTINATION, sim.DEPARTURE_TIME, sim.ON_WAY, sim.DONE) == (ORIGIN, DEST, DEP, ON_WAY, DONE)


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


def pending(agents, t, N, defect=None):
    """-> (N,) int64: the smallest ready agent id per origin road, -1 where nobody is ready. ``t`` is compared as fp32."""
    _check(defect)
    ag = np.asarray(agents, dtype=np.float32)
    t = np.float32(t)
    pend = np.full(N, -1, np.int64)
    first_dep = np.full(N, np.inf)
    for a in range(ag.shape[0]):
        due = ag[a, DEP] < t if defect == "strict_less" else ag[a, DEP] <= t
        waiting = defect == "status_ignored" or (ag[a, ON_WAY] == 0 and ag[a, DONE] == 0)
        if not (due and waiting):
            continue
        u = float(ag[a, ORIGIN])
        if not 0.0 <= u < N:
            continue
        u = int(u)
        if defect == "first_in_departure_order":
            if pend[u] < 0 or ag[a, DEP] < first_dep[u]:
                pend[u], first_dep[u] = a, ag[a, DEP]
        elif pend[u] < 0:
            pend[u] = a
    return pend


def _empty(x, Nmax, defect):
    n = np.asarray(x[:, 3 * Nmax + 1])
    return np.ones(n.shape, bool) if defect == "nonempty_rows_routed" else n == 0


def route_table(x, agents, table, t, Nmax, slot_of=None, defect=None, pend=None):
    """-> (written (N,) bool, value (N,) float64, 0 where nothing is written). ``table`` (N, N) [row][destination];
    ``slot_of`` (N,): the destinations' slots, < 0 = none (default: every destination has one)."""
    N = x.shape[0]
    ag = np.asarray(agents, dtype=np.float32)
    tb = np.asarray(table)
    if pend is None:
        pend = pending(ag, t, N, defect)
    _check(defect)
    empty = _empty(x, Nmax, defect)
    written, value = np.zeros(N, bool), np.zeros(N)
    for u in range(N):
        p = int(pend[u])
        if p < 0 or not empty[u]:
            continue
        d = float(ag[p, DEST])
        if not 0.0 <= d < N:
            continue
        d = int(d)
        if slot_of is not None and int(slot_of[d]) < 0:
            continue
        nh = int(tb[d][u]) if defect == "table_transposed" else int(tb[u][d])
        if nh < 0 and defect != "minus_one_written":
            continue
        if nh == d and defect != "no_hold":
            nh = u
        written[u], value[u] = True, float(nh)
    return written, value


def route_plan(x, agents, rt, ln, t, Nmax, defect=None, pend=None):
    """The plan lookup: ``rt`` (A, L) int32, ``ln`` (A,) -> (written, value) as :func:`route_table`."""
    N, A, Lmax = x.shape[0], rt.shape[0], rt.shape[1]
    if pend is None:
        pend = pending(agents, t, N, defect)
    _check(defect)
    empty = _empty(x, Nmax, defect)
    written, value = np.zeros(N, bool), np.zeros(N)
    for u in range(N):
        p = int(pend[u])
        if p < 0 or p >= A or not empty[u]:
            continue
        n = int(ln[p])
        if n <= 0 or n > Lmax:
            continue
        r = [int(v) for v in rt[p, :n]]
        if u not in r:
            continue
        j = r.index(u)
        nh = u
        if j < n - 1:
            nh = r[j + 1]
            if nh == r[n - 1] and defect != "plan_no_hold":
                nh = u
        written[u], value[u] = True, float(nh)
    return written, value


def apply(x, written, value, Nmax):
    """SELECTED_ROAD of ``x`` (torch, in place) <- ``value`` where ``written``; -> rows whose value changed."""
    col = 3 * Nmax + 5
    w = torch.from_numpy(written)
    new = torch.where(w, torch.from_numpy(value).to(x.dtype), x[:, col])
    changed = int((new != x[:, col]).sum())
    x[:, col] = new
    return changed


def lost(x, agents, Nmax):
    """ON_WAY - queued: the agents that are on the way and stand in no FIFO."""
    return int(agents[:, ON_WAY].sum()) - int(x[:, 3 * Nmax + 1].sum())


def replay(net, pop, frames, refresh_rate, gumbel_of, t_start, route=True, *, defect=None, head=None, plan=None):
    """``router_hold_restatement.replay(hold=True)`` with the rule after the hold router's choice. ``refresh_rate`` 0: the
    free-flow router. ``head(x, agents, t)`` -> x (optional): another writer of SELECTED_ROAD in the router's place, the rule
    still looking its first hops up in the free-flow table built at frame 0. ``plan`` = (rt, ln): the "routes" head — the
    free-flow hold router writes every row, ``replan_restatement.select_rule`` the rows on a route, then the plan lookup.
    -> dict: sel (frames, N), reward, x, agents, arrivals, lost, routed (rows written, summed), changed (of them, the rows
    whose value changed), per_frame_routed."""
    import replan_restatement as RR
    import router_hold_restatement as H
    from baseline_restatement import destination_columns
    from oracle import routing, sim
    _cols()
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    adj = net.dense_adjacency()
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    dests = sorted({int(d) for d in ag[:, 1].tolist() if 0 <= d < N})
    slot_of = torch.full((N,), -1, dtype=torch.int64)
    slot_of[dests] = torch.arange(len(dests))
    no_action = torch.zeros(ei.size(1), dtype=torch.long)
    sel, reward, per_frame = [], [], []
    routed = changed = 0
    table = None
    static = head is not None or plan is not None
    for t in range(frames):
        if t == 0 if (static or refresh_rate == 0) else t % refresh_rate == 0:
            w = routing.edge_travel_time(x, ei, net.congestion_constant, Nmax)
            table = destination_columns(ei, w, N, dests)
        clock = float(t_start + t)
        if head is not None:
            x = head(x, ag, t)
        else:
            x = H.hold_choice(x, ag, table, Nmax)
        if plan is not None:
            wr, val = RR.select_rule(x.numpy(), plan[0], plan[1])
            apply(x, wr, val, Nmax)
        if route:
            if plan is not None:
                wr, val = route_plan(x.numpy(), ag.numpy(), plan[0], plan[1], clock, Nmax, defect=defect)
            else:
                wr, val = route_table(x.numpy(), ag.numpy(), table.numpy(), clock, Nmax, slot_of=slot_of.numpy(), defect=defect)
            changed += apply(x, wr, val, Nmax)
            routed += int(wr.sum())
            per_frame.append(int(wr.sum()))
        sel.append(x[:, c.SEL].clone())
        out = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=gumbel_of(t),
                           congestion_constant=net.congestion_constant)
        reward.append(float(out["reward"]))
    return dict(sel=torch.stack(sel), reward=reward, x=x, agents=ag, arrivals=int(ag[1:, sim.DONE].sum()),
                lost=lost(x, ag, Nmax), routed=routed, changed=changed, per_frame_routed=per_frame, dests=dests)


# ---- crafted cases ---------------------------------------------------------------------------------------------------------------
def crafted(net, t=100.0, seed=0):
    """One state, agent table and next-hop table on ``net`` that holds every case the rule distinguishes; -> dict with x
    (torch (N, F)), agents (torch (A, 9)), table (N, N) int64 [row][destination], slot_of (N,), t, and ``rows``: name -> road.
    The table is the free-flow table of the empty network except for the entries the cases set by hand. Roads are taken in
    the order of a seeded permutation among those with an out-edge; the last-rank case uses the road of the largest
    out-degree."""
    from baseline_restatement import destination_columns
    from oracle import routing, sim
    _cols()
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    x[:, c.SEL] = -7.0                                  # what no rule writes: an untouched row shows
    outs = [[] for _ in range(N)]
    for s, d in ei.t().tolist():
        outs[s].append(d)
    t32 = float(np.float32(t))
    after = float(np.nextafter(np.float32(t), np.float32(np.inf)))
    hub = max(range(N), key=lambda r: len(outs[r]))
    g = torch.Generator().manual_seed(seed)
    order = [r for r in torch.randperm(N, generator=g).tolist() if len(outs[r]) >= 1 and r != hub]
    names = ("two_agents", "nonempty", "exactly_t", "just_after_t", "on_way_and_done", "no_slot", "unreachable", "next_is_dest",
             "origin_is_dest", "rank_ge_4", "waiting", "dirty_empty")
    rows = dict(zip(names, order))
    rows["last_rank"] = hub
    wide = max((r for r in order), key=lambda r: len(outs[r]))      # a road with more than 4 out-edges, where there is one
    if len(outs[wide]) > 4 and wide not in rows.values():
        rows["rank_ge_4"] = wide
    used = set(rows.values())
    pool = [r for r in reversed(order) if r not in used]

    def far(u):                                         # a destination of its own that is neither u nor a neighbour of u
        k = next(k for k, r in enumerate(pool) if r != u and r not in outs[u])
        return pool.pop(k)

    ag = [[0.0, 0.0, 1e9, 0, 0, 0, 0, 0, 0]]            # agent 0: the dummy, never ready here

    def add(o, d, dep, on_way=0, done=0):
        ag.append([float(o), float(d), float(dep), 0, 0, 0, 0, float(on_way), float(done)])
        return len(ag) - 1

    ids = {}
    u = rows["two_agents"]                              # the larger id departs earlier: the smaller id speaks
    ids["two_small"] = add(u, far(u), t32 - 1)
    ids["two_large"] = add(u, outs[u][0], t32 - 5)
    u = rows["nonempty"]                                # a ready agent on a non-empty row: the head keeps its choice
    ids["nonempty"] = add(u, far(u), t32 - 2)
    spare = pool.pop()                                  # the origin of the agent that stands there: no case's road
    ids["nonempty_head"] = add(spare, far(spare), t32 - 50, on_way=1)
    x[u, 0], x[u, Nmax], x[u, 2 * Nmax], x[u, c.N] = ids["nonempty_head"], t32 - 3, t32 + 30, 1
    ids["exactly_t"] = add(rows["exactly_t"], far(rows["exactly_t"]), t32)
    ids["just_after_t"] = add(rows["just_after_t"], far(rows["just_after_t"]), after)
    u = rows["on_way_and_done"]                         # neither is ready; a third, larger id is
    ids["on_way"] = add(u, u, t32 - 9, on_way=1)       # (bound for u itself: were it counted, the row would select itself)
    ids["done"] = add(u, far(u), t32 - 9, done=1)
    ids["after_them"] = add(u, far(u), t32 - 1)
    u = rows["no_slot"]
    no_slot_dest = far(u)
    ids["no_slot"] = add(u, no_slot_dest, t32 - 1)
    u = rows["unreachable"]
    ids["unreachable"] = add(u, far(u), t32 - 1)
    u = rows["next_is_dest"]
    ids["next_is_dest"] = add(u, outs[u][0], t32 - 1)
    ids["origin_is_dest"] = add(rows["origin_is_dest"], rows["origin_is_dest"], t32 - 1)
    u = rows["rank_ge_4"]
    ids["rank_ge_4"] = add(u, far(u), t32 - 1)
    u = rows["last_rank"]
    ids["last_rank"] = add(u, far(u), t32 - 1)
    u = rows["waiting"]                                 # its target road is full: the agent stays ready over several frames
    ids["waiting"] = add(u, far(u), t32 - 4)
    u = rows["dirty_empty"]                             # count 0, but slot 0 still holds an old record: empty all the same
    ids["dirty_empty"] = add(u, far(u), t32 - 1)
    x[u, 0], x[u, Nmax], x[u, 2 * Nmax] = ids["nonempty_head"], t32 - 60, t32 - 50
    agents = torch.tensor(ag, dtype=torch.float32)
    dests = sorted({int(d) for d in agents[:, 1].tolist()} - {no_slot_dest} | {0})
    slot_of = torch.full((N,), -1, dtype=torch.int64)
    slot_of[dests] = torch.arange(len(dests))
    table = destination_columns(ei, routing.edge_travel_time(x, ei, net.congestion_constant, Nmax), N,
                                sorted(set(dests) | {no_slot_dest}))
    table[rows["unreachable"], int(agents[ids["unreachable"], 1])] = -1
    for name in ("rank_ge_4", "last_rank"):             # the next hop set by hand: the road's LAST out-edge
        u = rows[name]
        table[u, int(agents[ids[name], 1])] = outs[u][-1]
    return dict(x=x, agents=agents, table=table, slot_of=slot_of, t=t32, rows=rows, ids=ids, outs=outs)


def crafted_plan(c, max_hops=6):
    """Route arrays for the agents of :func:`crafted` -> (rt (A, max_hops) int32, ln (A,) int32, want: name -> the value the
    plan lookup writes on that case's road, None = untouched). The routes need not be paths: the lookup does not ask."""
    rows, ids, outs = c["rows"], c["ids"], c["outs"]
    A = c["agents"].size(0)
    rt = np.full((A, max_hops), -1, np.int32)
    ln = np.zeros(A, np.int32)
    others = [r for r in range(len(outs)) if r not in rows.values()]
    o1, o2, o3 = others[:3]

    def put(a, route):
        rt[a, :len(route)], ln[a] = route, len(route)

    u = rows["two_agents"]
    put(ids["two_small"], [u, outs[u][0], o1, o2])                  # the origin first: the road after it
    put(ids["two_large"], [u, outs[u][-1], o2, o1])
    u = rows["exactly_t"]
    put(ids["exactly_t"], [o1, u, outs[u][-1], o2, o3])             # an origin that is not r[0]
    u = rows["origin_is_dest"]
    put(ids["origin_is_dest"], [u])                                 # len 1: the destination row selects itself
    u = rows["next_is_dest"]
    put(ids["next_is_dest"], [u, outs[u][0]])                       # two roads: held on the first
    u = rows["unreachable"]
    put(ids["unreachable"], [o1, o2])                               # off its route
    u = rows["last_rank"]
    put(ids["last_rank"], [u, outs[u][-1], o1, o2])
    u = rows["dirty_empty"]
    put(ids["dirty_empty"], [u, outs[u][0], o3])
    u = rows["nonempty"]
    put(ids["nonempty"], [u, outs[u][0], o3])                       # a route, but the row is not empty
    u = rows["rank_ge_4"]
    ln[ids["rank_ge_4"]] = max_hops + 1                             # a length beyond max_hops: no route
    want = {"two_agents": outs[rows["two_agents"]][0], "exactly_t": outs[rows["exactly_t"]][-1],
            "origin_is_dest": rows["origin_is_dest"], "next_is_dest": rows["next_is_dest"], "unreachable": None,
            "last_rank": outs[rows["last_rank"]][-1], "dirty_empty": outs[rows["dirty_empty"]][0], "nonempty": None,
            "rank_ge_4": None, "no_slot": None, "waiting": None, "on_way_and_done": None, "just_after_t": None}
    return rt, ln, want
