"""The goal-conditioned policy head (csrc/goal_mlp.hip, include/tarl_hip.h) restated in numpy: features, forward and backward
in fp32 with the kernels' operation order (features and logits bit for bit) and in float64 (the reference of the bounds),
each with ONE named defect switched on at a time (``defect=``: what a wrong kernel would compute), and the crafted cases
that tell them apart. Plain module: nothing here needs a GPU.

Inputs: ``obs`` (M, N, 16) fp32 in the tarl_policy_obs16 layout (0 MAXN, 1 NUMBER_OF_AGENT, 2 FF, 4 MAX_FLOW, 8 DESTINATION
of the head agent), ``ei`` (2, E) int64, ``table`` (N, N) fp32 all-pairs distances [candidate][destination] or (N, D) with
``slot`` (N,) int32, ``S`` the fp32 time scale, ``w`` (161,) = W1 (16, 8) | b1 (16) | w2 (16) | b2."""
from __future__ import annotations

import functools

import numpy as np

UNREACHABLE = np.float32(-1e20)
NF, NH, NW = 8, 16, 161
DEFECTS = ("cmin_first4", "cmin_tile64", "cmin_unreachable", "dest_of_v", "table_transposed", "slot_ignored", "g3_g4_swapped",
           "unreachable_mlp_minus_1e20", "unreachable_grad_counted", "relu_mask_no_bias", "dw1_per_sample_mean")


def csr(ei, N):
    """(order, out_ptr): the plan's CSR — edges by source, ascending edge id inside a source."""
    src = np.asarray(ei[0])
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(N + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=N))
    return order, ptr


def time_travel(ff, maxn, maxflow, na, dt):
    """prior_time_travel (csrc/prior_tables.h) in ``dt``."""
    with np.errstate(all="ignore"):
        crit = maxflow * ff / dt(3600.0)
        tc = ff * (maxn + dt(10.0) - crit) / (maxn + dt(10.0) - na)
        return np.where(np.isnan(ff) | np.isnan(tc), dt(np.nan), np.maximum(ff, tc)).astype(dt)


def lookup(table, slot, v, d, dt, defect=None):
    """D[m, e] = table[v[e], d[m, e]] through PriorAllPairs (``slot`` None) / PriorPerDest; +inf outside."""
    N = table.shape[0]
    ok = (d >= 0) & (d < N)
    dc = np.where(ok, d, 0)
    if slot is None:
        val = table[dc, v[None, :]] if defect == "table_transposed" else table[v[None, :], dc]
    else:
        s = dc % table.shape[1] if defect == "slot_ignored" else slot[dc].astype(np.int64)
        ok &= (s >= 0) & (s < table.shape[1])
        val = table[v[None, :], np.where(ok, s, 0)]
    return np.where(ok, val.astype(dt), dt(np.inf)).astype(dt)


def features(obs, ei, table, S, slot=None, dt=np.float32, defect=None):
    """-> (g (M, E, 8), reach (M, E) bool) in ``dt`` (np.float32: the kernels' bits; np.float64: the reference)."""
    obs = np.asarray(obs, dtype=np.float32)
    M, N = obs.shape[:2]
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    E = src.size
    o = obs.astype(dt)
    S = dt(np.float32(S))
    dest_f = obs[:, dst if defect == "dest_of_v" else src, 8]
    d = dest_f.astype(np.int64)                                        # (long) DESTINATION: truncation
    maxn_v, na_v, ff_v, mf_v = (o[:, dst, c] for c in (0, 1, 2, 4))
    maxn_u, na_u = o[:, src, 0], o[:, src, 1]
    D = lookup(np.asarray(table), None if slot is None else np.asarray(slot), dst, d, dt, defect)
    tt = time_travel(ff_v, maxn_v, mf_v, na_v, dt)
    with np.errstate(all="ignore"):
        c = D + tt
        reach = np.isfinite(c)
        order, ptr = csr(ei, N)
        pos = np.empty(E, dtype=np.int64)
        pos[order] = np.arange(E)                                      # CSR position of every edge
        rank = pos - ptr[src]
        group = src.copy()
        member = np.ones(E, dtype=bool)
        if defect == "cmin_first4":
            member = rank < 4
        elif defect == "cmin_tile64":
            group = src * (E // 64 + 2) + pos // 64                    # the minimum of the edge's own 64-position tile only
        gid, ginv = np.unique(group, return_inverse=True)
        cmin_g = np.full((M, gid.size), np.inf, dtype=dt)
        mrow = np.repeat(np.arange(M), E).reshape(M, E)
        if defect == "cmin_unreachable":
            cand = np.where(member[None, :], c, dt(np.inf))            # NaN costs enter and poison the minimum
            for e in range(E):
                cmin_g[:, ginv[e]] = np.minimum(cmin_g[:, ginv[e]], cand[:, e])
        else:
            cand = np.where(reach & member[None, :], c, dt(np.inf))
            np.minimum.at(cmin_g, (mrow, np.broadcast_to(ginv, (M, E))), cand)
        cmin = cmin_g[:, ginv]
        g = np.zeros((M, E, NF), dtype=dt)
        g[..., 0] = np.where(reach, np.fmin((c - cmin) / S, dt(8.0)), dt(8.0))
        g[..., 1] = (d == dst[None, :]).astype(dt)
        g[..., 2] = np.where(ff_v > 0, np.fmin(tt / ff_v - dt(1.0), dt(8.0)), dt(0.0))
        g3 = np.where(maxn_v > 0, na_v / maxn_v, dt(0.0))
        g4 = np.where(maxn_u > 0, na_u / maxn_u, dt(0.0))
        g[..., 3], g[..., 4] = (g4, g3) if defect == "g3_g4_swapped" else (g3, g4)
        g[..., 5] = np.fmin(D / S, dt(64.0)) / dt(8.0)
        g[..., 6] = (na_u == 0).astype(dt)
        g[..., 7] = np.fmin(ff_v / S, dt(8.0))
    return g, reach


def split(w, dt):
    w = np.asarray(w, dtype=np.float32).astype(dt)
    return w[:128].reshape(NH, NF), w[128:144], w[144:160], w[160]


def hidden(g, w, dt):
    """pre (…, 16) = b1 + sum_k W1[:, k] g_k, k ascending, multiply then add."""
    W1, b1, _, _ = split(w, dt)
    pre = np.broadcast_to(b1, g.shape[:-1] + (NH,)).astype(dt)
    for k in range(NF):
        pre = (pre + (W1[:, k] * g[..., k:k + 1]).astype(dt)).astype(dt)
    return pre


def forward(obs, ei, table, S, w, slot=None, dt=np.float32, defect=None, feats=None):
    """-> logits (M, E) in ``dt``; an unreachable edge carries exactly -1e20. ``feats``: :func:`features`' result in ``dt``,
    where the caller has it already."""
    g, reach = feats if feats is not None else features(obs, ei, table, S, slot, dt, defect)
    _, _, w2, b2 = split(w, dt)
    pre = hidden(g, w, dt)
    h = np.where(pre > 0, pre, dt(0.0))
    l = np.full(g.shape[:2], b2, dtype=dt)
    for j in range(NH):
        l = (l + (w2[j] * h[..., j]).astype(dt)).astype(dt)
    if defect == "unreachable_mlp_minus_1e20":
        return np.where(reach, l, (l + dt(UNREACHABLE)).astype(dt))
    return np.where(reach, l, dt(UNREACHABLE))


def backward(obs, ei, table, S, w, gl, slot=None, dt=np.float64, defect=None, feats=None):
    """-> grads (161,) of sum(gl * logits) over the reachable pairs (``dt`` float64: plain sums; the order of the device's
    sums is not restated — its result is compared within a bound). ``feats``: as :func:`forward`."""
    g, reach = feats if feats is not None else features(obs, ei, table, S, slot, dt, defect)
    W1, b1, w2, _ = split(w, dt)
    pre = hidden(g, w, dt)
    glr = np.asarray(gl).astype(dt).reshape(g.shape[:2])
    if defect != "unreachable_grad_counted":
        glr = np.where(reach, glr, dt(0.0))
    mask = ((pre - b1) >= 0) if defect == "relu_mask_no_bias" else (pre > 0)
    h = np.where(pre > 0, pre, dt(0.0))
    a = glr[..., None] * w2 * mask                                     # (M, E, 16)
    dW1 = np.einsum("mej,mek->jk", a, g)
    if defect == "dw1_per_sample_mean":
        dW1 = dW1 / dt(g.shape[0])
    return np.concatenate([dW1.reshape(-1), a.sum((0, 1)), (glr[..., None] * h).sum((0, 1)), [glr.sum()]]).astype(dt)


def torch_backward(obs, ei, table, S, w, gl, slot=None):
    """The float64 gradient by torch autograd on the float64 features (the check of :func:`backward`)."""
    import torch
    g, reach = features(obs, ei, table, S, slot, np.float64)
    wt = torch.tensor(np.asarray(w, dtype=np.float32).astype(np.float64), requires_grad=True)
    W1, b1, w2, b2 = wt[:128].view(NH, NF), wt[128:144], wt[144:160], wt[160]
    l = torch.relu(torch.tensor(g) @ W1.t() + b1) @ w2 + b2
    glr = torch.tensor(np.where(reach, np.asarray(gl, dtype=np.float64).reshape(reach.shape), 0.0))
    (l * glr).sum().backward()
    return wt.grad.numpy()


# ---- crafted cases ----------------------------------------------------------------------------------------------------------
def free_flow_table(net):
    """(N, N) fp32 all-pairs free-flow distances [candidate][destination] by float64 Dijkstra on the edge weights FF(dst)
    (+inf: unreachable, 0 on the diagonal), and the fp32 time scale."""
    import heapq
    N, nmax = net.num_roads, net.Nmax
    ff = net.x[:, 3 * nmax + 2].double().numpy()
    src, dst = net.edge_index[0].numpy(), net.edge_index[1].numpy()
    rev = [[] for _ in range(N)]
    for s, t in zip(src, dst):
        rev[t].append((s, ff[t]))
    table = np.full((N, N), np.inf)
    for d in range(N):
        dist = table[:, d]
        dist[d] = 0.0
        heap = [(0.0, d)]
        while heap:
            du, u = heapq.heappop(heap)
            if du > dist[u]:
                continue
            for p, wgt in rev[u]:
                if du + wgt < dist[p]:
                    dist[p] = du + wgt
                    heapq.heappush(heap, (du + wgt, p))
    return table.astype(np.float32), np.float32(ff.mean())


def random_obs(net, M, seed, empty=0.2):
    """Observations with real static columns, random counts (``empty``: the share of empty roads, whose head is the dummy
    agent with destination 0) and a random destination per head."""
    g = np.random.default_rng(seed)
    N, nmax = net.num_roads, net.Nmax
    obs = np.zeros((M, N, 16), dtype=np.float32)
    obs[:, :, :7] = net.x[:, 3 * nmax:3 * nmax + 7].numpy()[None]
    cnt = np.floor(g.random((M, N)) * (obs[..., 0])).astype(np.float32)
    cnt[g.random((M, N)) < empty] = 0
    obs[..., 1] = cnt
    obs[..., 7:] = (g.random((M, N, 9)) * 100).astype(np.float32)
    obs[..., 8] = np.where(cnt > 0, g.integers(0, N, (M, N)), 0).astype(np.float32)
    return obs


def craft(ei, obs, table):
    """(obs, table, u0, u1) edited copies: node ``u0`` — occupied, bound for road N - 1 — whose candidates are ALL
    unreachable (their entries of column N - 1 set to +inf), and node ``u1`` — occupied, bound for road N - 2 — with exactly
    ONE reachable candidate, its first in CSR order (finite; the others +inf). u0, u1: the first two roads with at least two
    out-edges."""
    obs, table = obs.copy(), table.copy()
    N = table.shape[0]
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    u0, u1 = (int(u) for u in np.nonzero(np.bincount(src, minlength=N) >= 2)[0][:2])
    table[dst[src == u0], N - 1] = np.inf
    c1 = dst[src == u1]
    table[c1, N - 2] = np.inf
    table[c1[0], N - 2] = np.float32(5.0)
    for u, d in ((u0, N - 1), (u1, N - 2)):
        obs[:, u, 1], obs[:, u, 8] = 1.0, float(d)
    return obs, table, u0, u1


def per_destination(table, obs, drop=()):
    """The (N, D) table and slot map over the destinations ``obs`` names, without the columns of ``drop``; the columns are
    stored in DESCENDING destination order so that a slot never equals its destination by accident."""
    N = table.shape[0]
    dests = [d for d in sorted(set(obs[..., 8].astype(np.int64).reshape(-1).tolist()), reverse=True)
             if 0 <= d < N and d not in drop]
    slot = np.full(N, -1, dtype=np.int32)
    slot[dests] = np.arange(len(dests), dtype=np.int32)
    return np.ascontiguousarray(table[:, dests]), slot


def weights(seed, sharp=False):
    """(161,) fp32: U(-0.5, 0.5) weights and biases (pre-activations on both sides of 0); ``sharp``: |w| up to 4."""
    g = np.random.default_rng(seed)
    return ((g.random(NW) - 0.5) * (8.0 if sharp else 1.0)).astype(np.float32)


# ---- behaviour cloning of the router into the head: the "bound anywhere" case ---------------------------------------------------
ANYWHERE = dict(agents=128, frames=60, envs=3, seed=11, steps=50, lr=0.05)


def anywhere_case():
    """8 x 8 torus, 128 agents with destinations drawn over ALL roads, departures within 40 s of the episode start (the case
    DESIGN 4.21 reports at chance for every trainable head) -> (net, population, t0)."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    pop = synth.population(ANYWHERE["agents"], net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    return net, pop, EPISODE_START


def observations(x, ag, Nmax):
    """obs16 (S, N, 16) of states ``x`` (S, N, F): the seven node columns and the row of the head agent (slot 0's id; agent
    0 where the FIFO is empty or the id is out of range)."""
    import torch
    head = torch.where(x[..., 3 * Nmax + 1] > 0, x[..., 0], torch.zeros_like(x[..., 0])).long()
    head = torch.where((head >= 0) & (head < ag.size(0)), head, torch.zeros_like(head))
    return torch.cat([x[..., 3 * Nmax:3 * Nmax + 7], ag[head]], dim=-1).numpy().astype(np.float32)


def initial_weights(seed):
    """(161,) fp32 as MPNNPolicyNet.use_goal_mlp initialises: U(-0.1, 0.1) weights, zero bias."""
    g = np.random.default_rng(seed)
    w = np.zeros(NW, dtype=np.float32)
    w[:128] = (g.random(128) * 0.2 - 0.1).astype(np.float32)
    w[144:160] = (g.random(16) * 0.2 - 0.1).astype(np.float32)
    return w


def bc_loop_goal(ei, N, obs, labels, table, S, w0, steps, lr, temperature=1.0):
    """Full-batch behaviour cloning of the goal-conditioned head in float64: ``steps`` times the mean cross-entropy over the
    labelled nodes of ``labels`` (S, N) of the segment softmax of the head's logits on ``obs`` (S, N, 16), its gradient by
    torch autograd, one ``adam64`` step. -> dict: nll (steps + 1,) before every step and after the last, acc likewise, w."""
    import torch

    import bc_restatement as BC
    import update_restatement as R
    ei_t = torch.as_tensor(np.asarray(ei))
    eid, deg, _ = BC.csr_edges(ei_t, N)
    valid = eid >= 0
    lab = torch.as_tensor(np.asarray(labels)).to(torch.int64)
    labelled = lab < torch.minimum(deg, torch.tensor(0x7F)).unsqueeze(0)
    W = int(labelled.sum())
    g, reach = features(obs, ei, table, S, None, np.float64)
    g, reach = torch.tensor(g), torch.tensor(reach)

    def evaluate(w):
        W1, b1, w2, b2 = w[:128].view(NH, NF), w[128:144], w[144:160], w[160]
        l = torch.relu(g @ W1.t() + b1) @ w2 + b2
        l = torch.where(reach, l, torch.full_like(l, float(UNREACHABLE))) / temperature
        z = torch.where(valid.unsqueeze(0), l[:, eid.clamp(min=0)], torch.full((1,) + tuple(eid.shape), float("-inf"),
                                                                               dtype=l.dtype))
        lse = torch.logsumexp(z, dim=2)
        z_lab = torch.gather(torch.where(valid.unsqueeze(0), z, torch.zeros_like(z)), 2,
                             lab.clamp(max=eid.size(1) - 1).unsqueeze(2)).squeeze(2)
        loss = torch.where(labelled, lse - z_lab, torch.zeros_like(z_lab)).sum() / W
        acc = float((labelled & (torch.argmax(z, dim=2) == lab)).sum()) / W
        return loss, acc

    w = torch.tensor(np.asarray(w0, dtype=np.float32).astype(np.float64))
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    nll, accs = [], []
    for k in range(steps):
        p = w.clone().requires_grad_(True)
        loss, acc = evaluate(p)
        loss.backward()
        nll.append(float(loss.detach()))
        accs.append(acc)
        w, m, v = R.adam64(w, p.grad, m, v, k + 1, lr=lr)
    with torch.no_grad():
        loss, acc = evaluate(w)
    nll.append(float(loss))
    accs.append(acc)
    return dict(nll=nll, acc=accs, w=w.numpy(), labelled=W)


@functools.lru_cache(maxsize=None)
def anywhere_run():
    """The restated run both suites read: ``envs`` collections of the ``expert`` driver (``free_flow`` expert) on the CPU
    oracle, then the goal head and — the control — the embedding head cloned full batch in float64. -> dict: goal, embedding
    (the loops' results), labels, arrivals."""
    import torch

    import bc_restatement as BC
    net, pop, t0 = anywhere_case()
    N, c = net.num_roads, ANYWHERE
    runs = [BC.collect_expert(net, pop, c["frames"], c["seed"] + k, t0) for k in range(c["envs"])]
    labels = torch.cat([r["labels"] for r in runs])
    obs = observations(torch.cat([r["x"] for r in runs]), pop, net.Nmax)
    table, S = free_flow_table(net)
    goal = bc_loop_goal(net.edge_index.numpy(), N, obs, labels, table, S, initial_weights(1), c["steps"], c["lr"])
    emb0 = torch.randn(N, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    emb = BC.bc_loop_embedding(net.edge_index, N, labels, emb0, c["steps"], c["lr"])
    return dict(goal=goal, embedding=emb, labels=labels, arrivals=[r["arrivals"] for r in runs])
