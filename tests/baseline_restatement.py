"""TEST INFRASTRUCTURE: the shortest-path baseline of ``tarl_hip.evaluator`` (head "dijkstra") replayed on the CPU with the
oracle's own pieces — ``oracle.routing.edge_travel_time`` and ``dijkstra_choice`` for the weights and the selection,
``tree_restatement`` for the per-destination reverse trees and their tie rule, ``oracle.sim.env_step`` (all-zero action) for
the frame — in the ENVIRONMENT's step order (choice, core, withdraw / insert, reward), and a small population whose
destinations come from a few roads so that the CPU trees stay cheap."""
import torch

from tree_restatement import adjacency, cpu_dijkstra, cpu_tie_rule


def few_destination_population(agents, num_roads, dests, *, seed, t0, t1):
    """synth.population with every DESTINATION (dummy row 0 included) drawn from ``dests``."""
    from tarl_hip import synth
    pop = synth.population(agents, num_roads, seed=seed, t0=t0, t1=t1)
    pick = torch.randint(0, len(dests), (agents + 1,), generator=torch.Generator().manual_seed(seed + 1))
    pop[:, 1] = torch.tensor(dests, dtype=torch.float32)[pick]
    return pop


def destination_columns(edge_index, weights, N, dests):
    """(N, N) int64 next-hop table with the columns of ``dests`` filled by the reverse trees' rule (the destination holds
    itself, -1 where it is not reached) and -1 elsewhere: what ``oracle.routing.dijkstra_choice(next_hop=...)`` indexes."""
    rev = adjacency(edge_index, weights, N, reverse=True)
    table = torch.full((N, N), -1, dtype=torch.int64)
    for d in dests:
        dist, _ = cpu_dijkstra(rev, N, d, reverse=True)
        col = cpu_tie_rule(rev, dist, N, d, reverse=True)
        col[d] = d
        table[:, d] = torch.tensor(col, dtype=torch.int64)
    return table


def replay(net, pop, frames, refresh_rate, gumbel_of, t_start):
    """One environment. ``gumbel_of(t)`` -> (E,) Gumbel values of frame t. Returns dict: ``sel`` (frames, N) the
    SELECTED_ROAD column every frame ran with, ``reward`` (frames,), final ``x`` and ``agents``, ``weights`` and ``tables``
    of every refresh (lists), ``max_count`` the largest FIFO count seen."""
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
    no_action = torch.zeros(ei.size(1), dtype=torch.long)
    sel, reward, weights, tables, max_count = [], [], [], [], 0.0
    table = None
    for t in range(frames):
        if t % refresh_rate == 0:
            w = routing.edge_travel_time(x, ei, net.congestion_constant, Nmax)
            table = destination_columns(ei, w, N, dests)
            weights.append(w)
            tables.append(table[:, dests].clone())
        x, _ = routing.dijkstra_choice(x, ag, ei, net.congestion_constant, Nmax, next_hop=table)
        sel.append(x[:, c.SEL].clone())
        out = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, float(t_start + t), Nmax, gumbel=gumbel_of(t),
                           congestion_constant=net.congestion_constant)
        reward.append(float(out["reward"]))
        max_count = max(max_count, float(x[:, c.N].max()))
    return dict(sel=torch.stack(sel), reward=reward, x=x, agents=ag, weights=weights, tables=tables, max_count=max_count,
                dests=dests)
