"""Credit scope "due" and the horizon bootstrap of the per-decision PPO credit restated in numpy float64 (TEST
INFRASTRUCTURE): which heads are due at a frame's clock, the road every agent is queued on, and the raw advantage with the
free-flow continuation past a segment cut by the batch. ``defect`` names one deliberate mistake (DEFECTS):
test_credit_scope_host shows that each of them moves a named case by at least ten times the tolerance the GPU tests use, or
flips an integer. :func:`premise_replay` is the measurement the scope rests on: on the CPU oracle, the draw of a road whose
head is not due changes nothing.

Plain loops: the cases are small, and the order of every sum is written out."""
import numpy as np

import decision_credit_restatement as DC

DEFECTS = ("strict_less",                 # dep < t for dep <= t
           "next_clock",                  # the clock of frame t + 1
           "empty_dep_believed",          # the dep word of an empty road believed: the count not tested
           "garbage_slot_read",           # the slot AT the count (the pending garbage triple) read as an agent
           "hoff_ignored",                # logical slot k read at physical slot k
           "bootstrap_from_u",            # the continuation from the deciding road u instead of the road r the agent stands on
           "lost_bootstrapped",           # an agent queued nowhere continued (from the deciding road) instead of charged
           "bootstrap_at_episode_end",    # a segment that ended with the episode bootstrapped
           "dist_transposed",             # dist[r][s] for dist[s][r]
           "bootstrapped_also_truncated")  # a bootstrapped decision counted in ``truncated`` too


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


def due_heads(x, Nmax, clock, next_clock=None, defect=None):
    """x (B, N, F) exported state, ``clock`` the fp32 clock the frame is stepped with -> (heads int64 (B, N): FIFO slot 0
    where NUMBER_OF_AGENT > 0 and HEAD_DEP <= clock in fp32, else 0; headed (B, N) bool; due (B, N) bool)."""
    _check(defect)
    x = np.asarray(x, dtype=np.float32)
    t = np.float32(next_clock if defect == "next_clock" else clock)
    headed = x[..., 3 * Nmax + 1] > 0
    dep = x[..., 2 * Nmax]
    with np.errstate(invalid="ignore"):
        late = dep < t if defect == "strict_less" else dep <= t
    due = late if defect == "empty_dep_believed" else (headed & late)
    return np.where(due, x[..., 0].astype(np.int64), 0), headed, headed & due


def ring(x, Nmax, hoff):
    """The id column of the exported x (B, N, F) laid out as the packed store keeps it: logical slot k of row (b, u) at
    physical slot (hoff[b, u] + k) mod Nmax -> int64 (B, N, Nmax)."""
    ids = np.asarray(x)[..., :Nmax].astype(np.int64)
    out = np.zeros_like(ids)
    k = np.arange(Nmax)
    for idx in np.ndindex(ids.shape[:2]):
        out[idx][(int(hoff[idx]) + k) % Nmax] = ids[idx]
    return out


def agent_roads(ids, count, A, hoff=None, defect=None):
    """ids (B, N, Nmax): the id of every PHYSICAL slot; count (B, N); hoff (B, N) the physical slot of logical slot 0 (None:
    0 everywhere, the exported x) -> (road int64 (B, A): the road whose logical slots 0 .. count - 1 hold the agent, -1:
    none; bad: ids outside [1, A); twice: agents met on more than one (road, slot))."""
    _check(defect)
    ids = np.asarray(ids)
    B, N, Nmax = ids.shape
    road = np.full((B, A), -1, dtype=np.int64)
    bad = twice = 0
    for b in range(B):
        for u in range(N):
            n = int(count[b, u]) + (1 if defect == "garbage_slot_read" else 0)
            h = 0 if hoff is None or defect == "hoff_ignored" else int(hoff[b, u])
            for k in range(min(n, Nmax)):
                a = int(ids[b, u, (h + k) % Nmax])
                if not 1 <= a < A:
                    bad += 1
                    continue
                twice += int(road[b, a] >= 0)
                road[b, a] = max(road[b, a], u)
    return road, bad, twice


def segment_bootstrap(clock_after, episode_end, defect=None):
    """Whether the segment whose last frame left the clock at ``clock_after`` is bootstrapped: it was cut by the batch, the
    episode goes on (the trainer's ``eng.time <= EPISODE_END``)."""
    _check(defect)
    return True if defect == "bootstrap_at_episode_end" else bool(clock_after <= episode_end)


def decision_advantage_boot(head_keep, frame, env, agents, times, t_end, dist, dest_slot, out_deg, agent_road, bootstrap,
                            timestep=1.0, gamma=1.0, defect=None):
    """decision_credit_restatement.decision_advantage with the horizon rule: a live decision whose traveller is not DONE,
    with r = agent_road[b][a] >= 0 and dist[s][r] finite, has n = (t_end - t) + dist[s][r] / timestep and counts in
    ``bootstrapped``; every other such decision keeps n = t_end - t and counts in ``truncated``.
    -> dict: adv, live, n (float64, -1 where not live), truncated, bootstrapped, bad."""
    _check(defect)
    if not bootstrap:
        r = DC.decision_advantage(head_keep, frame, env, agents, times, t_end, dist, dest_slot, out_deg, timestep, gamma)
        return dict(r, n=r["n"].astype(np.float64), bootstrapped=0)
    head_keep = np.asarray(head_keep, dtype=np.int64)
    agents = np.asarray(agents)
    dist = np.asarray(dist, dtype=np.float64)
    rows, N = head_keep.shape
    B, A = agents.shape[0], agents.shape[1]
    D = dist.shape[0]
    adv = np.zeros((rows, N))
    live = np.zeros((rows, N), dtype=bool)
    nn = np.full((rows, N), -1.0)
    truncated = bootstrapped = bad = 0
    for j in range(rows):
        t, b = int(frame[j]), int(env[j])
        if not (0 <= t < t_end and 0 <= b < B):
            continue
        for u in range(N):
            a = int(head_keep[j, u])
            if a <= 0:
                continue
            if a >= A:
                bad += 1
                continue
            if out_deg[u] == 0:
                continue
            d = float(agents[b, a, DC.DESTINATION])
            if not (0 <= d < N):
                continue
            s = int(dest_slot[int(d)])
            if not (0 <= s < D):
                continue
            du = dist[s, u]
            if not np.isfinite(du):
                continue
            n, trunc = DC.frames_to_go(times, t, t_end, float(agents[b, a, DC.DONE]), float(agents[b, a, DC.ARRIVAL_TIME]))
            n = np.float64(n)
            if trunc:
                r = int(agent_road[b, a])
                go = None
                if defect == "bootstrap_from_u":
                    r = u if r >= 0 else r
                if 0 <= r < N:
                    dr = dist.reshape(-1)[r * D + s] if defect == "dist_transposed" else dist[s, r]
                    go = dr / np.float64(timestep) if np.isfinite(dr) else None
                elif defect == "lost_bootstrapped":
                    go = du / np.float64(timestep)
                if go is not None:
                    n = n + go
                    bootstrapped += 1
                    truncated += int(defect == "bootstrapped_also_truncated")
                else:
                    truncated += 1
            adv[j, u] = DC.owed(du / np.float64(timestep), gamma) - DC.owed(n, gamma)
            live[j, u] = True
            nn[j, u] = n
    return dict(adv=adv, live=live, n=nn, truncated=truncated, bootstrapped=bootstrapped, bad=bad)


# ---- the premise, on the CPU oracle ---------------------------------------------------------------------------------------------
def premise_replay(net, pop, frames, refresh_rate, gumbel_of, t_start, seed=0):
    """The holding router's replay (router_hold_restatement.replay's loop) with a shadow frame: in every frame the selection of
    every road whose head is headed but NOT due is re-drawn (another out-neighbour, seeded), leaving out the roads that are
    the origin of a ready agent (their selection places the departing agent), and the shadow is stepped with the same noise.
    -> dict: headed / due: the (frame, road) counts; redrawn: selections changed; differing: the frames after which the
    FIFO contents below the count, the counts or the agent table of the shadow differ from the real frame's; twice: ids
    found queued on two (road, slot) places after any frame; lost_or_waiting: agents queued nowhere after the last frame."""
    import torch
    import router_hold_restatement as H
    from baseline_restatement import destination_columns
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
    outs = DC.out_lists(ei.numpy(), N)
    dst = ei[1].numpy()
    rng = np.random.default_rng(seed)
    headed = due = redrawn = twice = 0
    differing = []
    table = None
    for t in range(frames):
        if t % refresh_rate == 0:
            table = destination_columns(ei, routing.edge_travel_time(x, ei, net.congestion_constant, Nmax), N, dests)
        clock = float(t_start + t)
        x = H.hold_choice(x, ag, table, Nmax)
        _, hd, du = due_heads(x.numpy()[None], Nmax, clock)
        headed, due = headed + int(hd.sum()), due + int(du.sum())
        ready = (ag[:, sim.DEPARTURE_TIME] <= clock) & (ag[:, sim.ON_WAY] == 0) & (ag[:, sim.DONE] == 0)
        origin = np.zeros(N, dtype=bool)
        origin[ag[ready, sim.ORIGIN].to(torch.long).numpy()] = True
        shadow, shadow_ag = x.clone(), ag.clone()
        for u in np.nonzero(hd[0] & ~du[0] & ~origin)[0]:
            others = [int(dst[e]) for e in outs[u] if float(dst[e]) != float(x[u, c.SEL])]
            if others:
                shadow[u, c.SEL] = float(others[int(rng.integers(len(others)))])
                redrawn += 1
        g = gumbel_of(t)
        sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=g, congestion_constant=net.congestion_constant)
        sim.env_step(shadow, shadow_ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=g,
                     congestion_constant=net.congestion_constant)
        below = (torch.arange(Nmax) < x[:, c.N].unsqueeze(1)).repeat(1, 3)
        same = (torch.equal(x[:, c.N], shadow[:, c.N]) and torch.equal(x[:, :3 * Nmax][below], shadow[:, :3 * Nmax][below])
                and torch.equal(ag, shadow_ag))
        if not same:
            differing.append(t)
        _, _, tw = agent_roads(x.numpy()[None, :, :Nmax].astype(np.int64), x.numpy()[None, :, c.N], ag.size(0))
        twice += tw
    road, _, _ = agent_roads(x.numpy()[None, :, :Nmax].astype(np.int64), x.numpy()[None, :, c.N], ag.size(0))
    return dict(headed=headed, due=due, redrawn=redrawn, differing=differing, twice=twice, x=x, agents=ag, road=road[0])
