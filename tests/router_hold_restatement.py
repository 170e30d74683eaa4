"""TEST INFRASTRUCTURE: the shortest-path router that HOLDS one road short of the destination (``tarl_hip.evaluator`` head
"dijkstra_hold") replayed on the CPU with the oracle's own pieces, in the shape of ``baseline_restatement``:
``oracle.routing.dijkstra_choice`` followed by the rule

    SELECTED_ROAD[i] = i   where   next_hop[i][d] == d,   d the destination of row i's head agent (integers),

then ``oracle.sim.env_step`` (all-zero action) in the ENVIRONMENT's step order. The same replay is available with ONE defect
at a time (:data:`DEFECTS`): what a wrong kernel would compute, for the tests that show the right one matters."""
import torch

from baseline_restatement import destination_columns

DEFECTS = ("minus_one",      # the hold value is -1 instead of the row's own id
           "two_short",      # also holds two roads short: where next_hop of the next hop is the destination
           "due_only",       # holds only when the head's departure from the row is already due
           "slot_float")     # compares after the float conversion, against the destination's SLOT instead of the destination


def _head_dest(x, agents):
    head = x[:, 0].to(torch.int64)
    return agents[head, 1].to(torch.int64)


def holding_rows(x, agents, table, Nmax, *, defect=None, t=None, slot_of=None):
    """-> (N,) bool: the rows the rule rewrites (the destination row itself included, where it changes nothing)."""
    N = x.size(0)
    rows = torch.arange(N)
    dest = _head_dest(x, agents)
    nh = table[rows, dest]
    hold = nh == dest
    if defect == "two_short":
        hold = hold | ((nh >= 0) & (table[nh.clamp(min=0), dest] == dest))
    elif defect == "due_only":
        hold = hold & (x[:, 2 * Nmax] <= float(t))
    elif defect == "slot_float":
        hold = nh.to(torch.float32) == slot_of[dest].to(torch.float32)
    elif defect not in (None, "minus_one"):
        raise ValueError(f"unknown defect {defect!r}")
    return hold


def hold_choice(x, agents, table, Nmax, *, defect=None, t=None, slot_of=None):
    """``oracle.routing.dijkstra_choice`` with ``table`` (N, N) int64 [row][destination], followed by the rule -> x with
    SELECTED_ROAD rewritten (a copy)."""
    from oracle import routing
    x, _ = routing.dijkstra_choice(x, agents, None, None, Nmax, next_hop=table)
    hold = holding_rows(x, agents, table, Nmax, defect=defect, t=t, slot_of=slot_of)
    own = torch.arange(x.size(0), dtype=x.dtype) if defect != "minus_one" else torch.full((x.size(0),), -1.0, dtype=x.dtype)
    col = 3 * Nmax + 5
    x[:, col] = torch.where(hold, own, x[:, col])
    return x


def replay(net, pop, frames, refresh_rate, gumbel_of, t_start, hold=True, *, defect=None, table=None):
    """One environment, as ``baseline_restatement.replay`` (same returned keys); ``hold=False`` IS that replay.
    ``refresh_rate=0``: the table is built at frame 0 only; ``table`` (N, N): this table at every frame, none built.
    Also returned: ``acted`` — (frame, row) pairs whose SELECTED_ROAD the rule changed, ``acted_occupied`` — those with a
    non-empty FIFO; ``origin_self`` — agents inserted while SELECTED_ROAD of their origin row named the row itself,
    ``origin_hold`` — those of them whose origin row the rule had changed; ``core_onto_dest`` — agents the core moved onto
    their own destination road (on the way before the frame, at a FIFO of that road with this frame's arrival clock);
    ``error`` — ``None``, or (frame, message) where the oracle's frame raised (the -1 defect under an entering agent: the
    replay ends there, with one reward fewer than frames)."""
    from oracle import routing, sim
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
    rows = torch.arange(N)
    sel, reward, weights, tables, max_count = [], [], [], [], 0.0
    acted = acted_occupied = origin_self = origin_hold = core_onto_dest = 0
    fixed = table is not None
    error = None
    for t in range(frames):
        if not fixed and (t == 0 if refresh_rate == 0 else t % refresh_rate == 0):
            w = routing.edge_travel_time(x, ei, net.congestion_constant, Nmax)
            table = destination_columns(ei, w, N, dests)
            weights.append(w)
            tables.append(table[:, dests].clone())
        clock = float(t_start + t)
        before, _ = routing.dijkstra_choice(x, ag, ei, net.congestion_constant, Nmax, next_hop=table)
        x = hold_choice(x, ag, table, Nmax, defect=defect, t=clock, slot_of=slot_of) if hold else before
        changed = x[:, c.SEL] != before[:, c.SEL]
        acted += int(changed.sum())
        acted_occupied += int((changed & (x[:, c.N] > 0)).sum())
        sel.append(x[:, c.SEL].clone())
        on_way = ag[:, sim.ON_WAY].clone()
        try:
            out = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=gumbel_of(t),
                               congestion_constant=net.congestion_constant)
        except IndexError as e:      # a SELECTED_ROAD of -1 under an entering agent: outside the oracle's domain, the replay ends
            error = (t, str(e))
            break
        reward.append(float(out["reward"]))
        max_count = max(max_count, float(x[:, c.N].max()))
        # who entered the network in this frame, and through which kind of origin row
        new = torch.nonzero((on_way == 0) & (ag[:, sim.ON_WAY] == 1)).view(-1)
        origin = ag[new, sim.ORIGIN].to(torch.int64)
        own = sel[-1][origin] == origin.to(sel[-1].dtype)
        origin_self += int(own.sum())
        origin_hold += int((own & changed[origin]).sum())
        # who the core carried onto the road it is bound for
        ids = x[:, :Nmax].to(torch.int64)
        active = torch.arange(Nmax) < x[:, c.N].unsqueeze(1)
        here = active & (x[:, Nmax:2 * Nmax] == clock) & (on_way[ids] == 1) & (ag[ids, sim.DESTINATION].to(torch.int64) == rows.unsqueeze(1))
        core_onto_dest += int(here.sum())
    return dict(sel=torch.stack(sel), reward=reward, x=x, agents=ag, weights=weights, tables=tables, max_count=max_count,
                dests=dests, acted=acted, acted_occupied=acted_occupied, origin_self=origin_self, origin_hold=origin_hold,
                core_onto_dest=core_onto_dest, arrivals=int(ag[1:, sim.DONE].sum()), error=error)
