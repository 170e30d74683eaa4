"""The learned per-decision critic restated in numpy (TEST INFRASTRUCTURE): the eight features of a live
decision, the 8 -> 16 -> 1 network, the advantage with the learned baseline, the smooth-L1 loss and its gradient.
``dtype=np.float32`` follows the kernels' operation order (a multiply then an add, k and j ascending, the sums in CSR
order), so features and values are reproduced bit for bit; ``dtype=np.float64`` is the reference. ``defect`` names one
deliberate mistake (DEFECTS): test_decision_critic_host shows that each of them moves a named case by at least ten times
the tolerance the GPU tests use.

Plain loops over the live (row, road) pairs: the cases are small, and the order of every sum is written out."""
import numpy as np

from decision_credit_restatement import out_lists

NF, NH, NW, B1, W2, B2 = 8, 16, 161, 128, 144, 160
OBS_MAXN, OBS_N, OBS_FF, OBS_DEST = 0, 1, 2, 8

DEFECTS = ("vstar_first_four",        # v* over the first four out-edges only
           "vstar_inf_wins",          # an unreachable (inf) neighbour can be v*
           "tie_last",                # a tie in dist goes to the last neighbour instead of the first
           "mean_over_all",           # f4 over all neighbours instead of the reachable ones
           "dest_of_v",               # the destination read from the first out-neighbour's head instead of u's
           "dist_transposed",         # dist[x][s] for dist[s][x]
           "slot_ignored",            # s = d instead of dest_slot[d]
           "frames_left_next_row",    # frames_left of the neighbouring row
           "target_sign",             # y = +adv_raw / delay_scale
           "adv_no_delay_scale",      # adv_out = adv_raw + value
           "sl1_switch",              # the smooth-L1 switch at |e| < 0.5
           "relu_mask_no_bias",       # the backward's ReLU mask from the weighted sum without the bias
           "loss_over_mn",            # the loss divided by M * N instead of L
           "count_nonlive")           # every road with an out-edge counted, live or not


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


def init_weights(seed=0):
    """The initialisation of DESIGN 4.27 as float64 (161,): W1 uniform in (-0.1, 0.1), b1 = w2 = b2 = 0."""
    w = np.zeros(NW)
    w[:B1] = np.random.default_rng(seed).uniform(-0.1, 0.1, B1).astype(np.float32)      # values an fp32 buffer holds exactly
    return w


def weights(seed, sharp=False):
    """(161,) fp32: U(-0.5, 0.5) weights and biases (pre-activations on both sides of 0); ``sharp``: |w| up to 4."""
    g = np.random.default_rng(seed)
    return ((g.random(NW) - 0.5) * (8.0 if sharp else 1.0)).astype(np.float32)


def _fill(om, x, dt):
    mx, n = dt(om[x, OBS_MAXN]), dt(om[x, OBS_N])
    return n / mx if mx > 0 else dt(0.0)


def decision_features(edge_index, N, obs16, m, u, frames_left, dist, dest_slot, timestep, dtype=np.float32, lists=None,
                      defect=None):
    """The eight features of decision (row m, road u) -> (NF,) of ``dtype``."""
    dt = dtype
    lists = out_lists(edge_index, N) if lists is None else lists
    dst = np.asarray(edge_index[1])
    om = np.asarray(obs16[m], dtype=np.float32)
    dist = np.asarray(dist, dtype=np.float64)
    D = dist.shape[0]
    M = len(frames_left)
    nb = [int(dst[e]) for e in lists[u]]
    src_row = nb[0] if (defect == "dest_of_v" and nb) else u
    dest = float(om[src_row, OBS_DEST])
    d, row = -1, None
    if 0 <= dest < N:
        d = int(dest)
        s = d % D if defect == "slot_ignored" else int(dest_slot[d])
        if 0 <= s < D:
            row = dist.reshape(-1)[np.arange(N) * D + s] if defect == "dist_transposed" else dist[s]
    tau64 = np.float64(np.float32(timestep))
    h = int(frames_left[(m + 1) % M] if defect == "frames_left_next_row" else frames_left[m])
    nff = row[u] / tau64 if row is not None else np.inf
    f = np.zeros(NF, dtype=dt)
    f[0] = dt(min(nff, 512.0)) / dt(64.0)
    f[1] = dt(min(h, 512)) / dt(64.0)
    f[2] = _fill(om, u, dt)
    best, vstar, ssum, reach = np.inf, -1, dt(0.0), 0
    if row is not None:
        cand = nb[:4] if defect == "vstar_first_four" else nb
        for v in nb:
            if np.isfinite(row[v]) or defect == "mean_over_all":
                ssum = dt(ssum + _fill(om, v, dt))
                reach += 1
        if defect == "vstar_inf_wins" and cand:
            vstar, best = cand[0], row[cand[0]]
        for v in cand:
            if np.isfinite(row[v]) and (row[v] <= best if defect == "tie_last" else row[v] < best):
                best, vstar = row[v], v
    if vstar >= 0:
        f[3] = _fill(om, vstar, dt)
        f[5] = dt(1.0 if vstar == d else 0.0)
    if reach > 0:
        f[4] = ssum / dt(reach)
    f[6] = dt(1.0 if nff > h else 0.0)
    tau = dt(np.float32(timestep))
    f[7] = min(dt(om[u, OBS_FF]) / tau, dt(64.0)) / dt(8.0)
    return f


def features(edge_index, N, obs16, head, frames_left, dist, dest_slot, timestep, dtype=np.float32, mask=None, defect=None):
    """-> (M, N, 8) of ``dtype``: zeros where ``head <= 0`` (or outside ``mask``, which replaces the live mask)."""
    _check(defect)
    head = np.asarray(head)
    live = head > 0 if mask is None else np.asarray(mask, dtype=bool)
    lists = out_lists(edge_index, N)
    out = np.zeros(head.shape + (NF,), dtype=dtype)
    for m, u in zip(*np.nonzero(live)):
        out[m, u] = decision_features(edge_index, N, obs16, int(m), int(u), frames_left, dist, dest_slot, timestep, dtype,
                                      lists, defect)
    return out


def mlp(w, f, dtype=np.float32):
    """f (..., 8) -> (pre (..., 16), value (...)): pre_j = b1[j] + sum_k W1[j][k] f_k, value = b2 + sum_j w2[j] relu(pre_j),
    every step one multiply and one add of ``dtype``."""
    dt = dtype
    w = np.asarray(w, dtype=dt)
    f = np.asarray(f, dtype=dt)
    pre = np.empty(f.shape[:-1] + (NH,), dtype=dt)
    y = np.full(f.shape[:-1], w[B2], dtype=dt)
    for j in range(NH):
        q = np.full(f.shape[:-1], w[B1 + j], dtype=dt)
        for k in range(NF):
            q = (q + (w[j * NF + k] * f[..., k]).astype(dt)).astype(dt)
        pre[..., j] = q
        y = (y + (w[W2 + j] * np.maximum(q, dt(0.0))).astype(dt)).astype(dt)
    return pre, y


def forward(w, feats, live, adv_raw, delay_scale=16.0, dtype=np.float32, defect=None):
    """-> (value, adv_dec), zeros where not live: adv_dec = adv_raw + delay_scale * value."""
    _check(defect)
    dt = dtype
    _, y = mlp(w, feats, dt)
    live = np.asarray(live, dtype=bool)
    a = np.asarray(adv_raw, dtype=np.float32).astype(dt)
    sc = dt(1.0) if defect == "adv_no_delay_scale" else dt(np.float32(delay_scale))
    adv = (a + (sc * y).astype(dt)).astype(dt)
    return np.where(live, y, dt(0.0)), np.where(live, adv, dt(0.0))


def smooth_l1(e, dt, defect=None):
    cut = dt(0.5) if defect == "sl1_switch" else dt(1.0)
    ae = np.abs(e)
    loss = np.where(ae < cut, ((dt(0.5) * e).astype(dt) * e).astype(dt), (ae - dt(0.5)).astype(dt))
    de = np.where(ae < cut, e, np.sign(e).astype(dt))
    return loss, de


def critic_loss(w, feats, live, adv_raw, n_live, delay_scale=16.0, coef=1.0, grad_scale=1.0, dtype=np.float64,
                defect=None):
    """The loss of DESIGN 4.27 over the live decisions, forward and backward, from the features.
    -> dict: out5 (M, 5) float64 = per row {sum of l, live, sum of y, sum of y^2, sum of (y - value)^2}; grads (161,) of
    ``dtype``: the gradient of grad_scale * coef / L * sum of l (zeros while L <= 0); loss = coef / L * sum of l;
    value, y (M, N); explained_variance."""
    _check(defect)
    dt = dtype
    w = np.asarray(w, dtype=dt)
    feats = np.asarray(feats, dtype=dt)
    live = np.asarray(live, dtype=bool)
    M, N = live.shape
    pre, val = mlp(w, feats, dt)
    a = np.asarray(adv_raw, dtype=np.float32).astype(dt)
    ds = dt(np.float32(delay_scale))
    y = (a if defect == "target_sign" else -a) / ds
    e = (val - y).astype(dt)
    loss, de = smooth_l1(e, dt, defect)
    L = int(M * N) if defect == "loss_over_mn" else int(n_live)
    c = (dt(np.float32(coef)) * dt(np.float32(grad_scale))) / dt(L) if L > 0 else dt(0.0)
    r = np.where(live, (c * de).astype(dt), dt(0.0))
    lv = live.astype(np.float64)
    y64, e64 = y.astype(np.float64), e.astype(np.float64)
    out5 = np.stack([(loss.astype(np.float64) * lv).sum(1), lv.sum(1), (y64 * lv).sum(1), (y64 * y64 * lv).sum(1),
                     (e64 * e64 * lv).sum(1)], axis=1)
    on = (pre - w[B1:W2]) >= 0 if defect == "relu_mask_no_bias" else pre > 0
    aj = np.where(on, r[..., None] * w[W2:B2], dt(0.0))                     # (M, N, 16)
    grads = np.zeros(NW, dtype=dt)
    grads[:B1] = np.einsum("mnj,mnk->jk", aj, feats).reshape(-1)
    grads[B1:W2] = aj.sum((0, 1))
    grads[W2:B2] = np.where(on, r[..., None] * pre, dt(0.0)).sum((0, 1))
    grads[B2] = r.sum()
    tot = out5.sum(0)
    cnt = max(tot[1], 1.0)
    den = tot[3] - tot[2] * tot[2] / cnt
    ev = 1.0 - tot[4] / den if den > 0 else 0.0
    return dict(out5=out5, grads=grads, loss=float(np.float32(coef)) * tot[0] / cnt if L > 0 else 0.0, value=np.where(live, val, 0),
                y=np.where(live, y, 0), explained_variance=ev, value_mean=(val.astype(np.float64) * lv).sum() / cnt)


def adam_fit(w0, feats, live, adv_raw, steps=200, lr=0.01, delay_scale=16.0, coef=1.0, dtype=np.float64):
    """``steps`` full-batch Adam steps (torch.optim.Adam's update, beta = 0.9 / 0.999, eps 1e-8) of the critic loss.
    -> (weights, the dict of :func:`critic_loss` at the final weights)."""
    w = np.asarray(w0, dtype=dtype).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    L = int(np.asarray(live, dtype=bool).sum())
    for step in range(1, steps + 1):
        g = critic_loss(w, feats, live, adv_raw, L, delay_scale, coef, 1.0, dtype)["grads"]
        m = m + (1 - 0.9) * (g - m)
        v = v * 0.999 + (1 - 0.999) * g * g
        w = w - (lr / (1 - 0.9 ** step)) * (m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** step) + 1e-8))
    return w, critic_loss(w, feats, live, adv_raw, L, delay_scale, coef, 1.0, dtype)


# ---- the learning case -----------------------------------------------------------------------------------------------------------
LEARN_T_END, LEARN_FRAMES = 120, tuple(range(90, 120))      # the segment's last 30 frames: 27 % of the decisions truncated
LEARN_STEPS, LEARN_LR = 200, 0.01
_LEARN = {}


def free_flow_dist(net, dests):
    """(D, N) float64 free-flow distances to ``dests`` over the travel times of the empty network (inf: not reached) and the
    (N,) slot table."""
    import torch
    from oracle import routing
    from tree_restatement import adjacency, cpu_dijkstra
    N, Nmax = net.num_roads, net.Nmax
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, 3 * Nmax + 1] = 0
    w = routing.edge_travel_time(x, net.edge_index, net.congestion_constant, Nmax)
    rev = adjacency(net.edge_index, w, N, reverse=True)
    dist = np.array([cpu_dijkstra(rev, N, d, reverse=True)[0] for d in dests], dtype=np.float64)
    slot = np.full(N, -1, dtype=np.int32)
    slot[list(dests)] = np.arange(len(dests), dtype=np.int32)
    return dist, slot


def obs16_of(x, agents, Nmax):
    """The observation ops.fused_obs16 forms: the 7 node columns and the 9 columns of the agent in FIFO slot 0."""
    import torch
    head = x[:, 0].long().clamp(0, agents.size(0) - 1)
    return torch.cat((x[:, 3 * Nmax:], agents[head]), dim=-1).numpy().astype(np.float32)


def learning_case():
    """The "spread" case of test_departures_host (8 x 8 torus, 128 agents, the free-flow hold router with the first-hop rule)
    on oracle.sim.env_step, one segment that ends at frame LEARN_T_END, the rows LEARN_FRAMES kept: heads and raw advantages
    of decision_credit_restatement, the observations in front of every kept frame. -> dict (computed once)."""
    if _LEARN:
        return _LEARN
    import decision_credit_restatement as DC
    import departure_restatement as D
    import router_hold_restatement as H
    import test_router_hold_host as RH
    from baseline_restatement import destination_columns
    from oracle import routing
    from tarl_hip.engine import EPISODE_START
    net, pop, _ = RH._case("spread")
    N, Nmax, T = net.num_roads, net.Nmax, LEARN_T_END
    dests = sorted({int(d) for d in pop[:, 1].tolist() if 0 <= d < N})
    seen, table = {}, []

    def head(x, ag, t):
        if t == 0:
            table.append(destination_columns(net.edge_index, routing.edge_travel_time(x, net.edge_index,
                                                                                      net.congestion_constant, Nmax), N, dests))
        if t in LEARN_FRAMES:
            seen[t] = (DC.heads(x.numpy()[None], Nmax)[0], obs16_of(x, ag, Nmax))
        return H.hold_choice(x, ag, table[0], Nmax)

    out = D.replay(net, pop, T, 0, RH._gumbel(net.edge_index.size(1), T), EPISODE_START, route=True, head=head)
    frames = list(LEARN_FRAMES)
    hk = np.stack([seen[t][0] for t in frames])
    obs = np.stack([seen[t][1] for t in frames])
    times = np.asarray([EPISODE_START + t for t in range(T + 1)], dtype=np.float32)
    dist, slot = free_flow_dist(net, dests)
    deg = np.bincount(net.edge_index[0].numpy(), minlength=N)
    adv = DC.decision_advantage(hk, frames, [0] * len(frames), out["agents"].numpy()[None], times, T, dist, slot, deg, 1.0, 1.0)
    live = adv["live"]
    _LEARN.update(net=net, ei=net.edge_index.numpy(), N=N, obs=obs, head=np.where(live, hk, 0).astype(np.int32), live=live,
                  adv=adv["adv"].astype(np.float32), frames_left=(T - np.asarray(frames)).astype(np.int32), dist=dist, slot=slot,
                  truncated=adv["truncated"], timestep=1.0)
    return _LEARN


# ---- crafted cases -----------------------------------------------------------------------------------------------------------------
CRAFT_TAU, CRAFT_H = 0.25, 40      # row 0 has 40 frames left: n_ff = 40 at dist 10.0


def crafted_case(edge_index, N, seed=0, M=3, hub_ranks=()):
    """Random observations, heads, distances (a tenth of them inf) and destinations on any graph, with named decisions set
    by hand in row 0 (``named``: name -> (row, road)), each under a destination slot of its own:
    tie (the first and the last neighbour share the smallest distance), none (no reachable neighbour), one (exactly one, and
    it is the destination), maxn0 (MAXN = 0 on the road and on v*), nff_below / nff_equal / nff_above (n_ff against h = 40),
    big (row 1: n_ff = 800 and h = 600, both above 512) and hub_rank_<r> (row i: v* at CSR rank r of the road of the largest
    out-degree). timestep = CRAFT_TAU, so that FF / timestep passes 64."""
    rng = np.random.default_rng(1000 + seed)
    ei = np.asarray(edge_index)
    lists = out_lists(ei, N)
    nbrs = [[int(ei[1][e]) for e in ls] for ls in lists]
    deg = np.array([len(v) for v in nbrs])
    hub = int(np.argmax(deg))
    assert M >= max(2, len(hub_ranks))
    names = ["tie", "none", "one", "maxn0", "nff_below", "nff_equal", "nff_above", "big"]
    pool = [int(u) for u in rng.permutation(N) if deg[u] >= 2 and u != hub and len(set(nbrs[u])) == deg[u]]
    road = {nm: pool[i] for i, nm in enumerate(names)}
    D = len(names) + len(hub_ranks) + 4
    first = nbrs[road["one"]][1]                                   # the "one" case is bound for its only reachable neighbour
    dests = [int(d) for d in rng.permutation(N) if d != first][:D - 1]
    dests.insert(names.index("one"), first)
    slot = np.full(N, -1, dtype=np.int32)
    slot[dests] = np.arange(D, dtype=np.int32)
    dist = rng.uniform(1.0, 80.0, (D, N))
    dist[rng.random((D, N)) < 0.1] = np.inf
    obs = rng.normal(size=(M, N, 16)).astype(np.float32)
    obs[..., OBS_MAXN] = np.where(rng.random((M, N)) < 0.08, 0, rng.integers(3, 30, (M, N)))
    obs[..., OBS_N] = np.floor(rng.random((M, N)) * (obs[..., OBS_MAXN] + 1))
    obs[..., OBS_FF] = rng.uniform(2.0, 20.0, (M, N))
    obs[..., OBS_DEST] = np.asarray(dests)[rng.integers(0, D, (M, N))]
    head = np.where(rng.random((M, N)) < 0.3, rng.integers(1, 100, (M, N)), 0).astype(np.int32)
    frames_left = rng.integers(0, 500, M).astype(np.int32)
    frames_left[0], frames_left[1] = CRAFT_H, 600
    named = {}

    def put(name, m, u, s, fills=()):
        named[name] = (m, u)
        head[m, u] = 7
        obs[m, u, OBS_DEST] = dests[s]
        for v, (mx, n) in fills:
            obs[m, v, OBS_MAXN], obs[m, v, OBS_N] = mx, n

    for s, nm in enumerate(names):
        u = road[nm]
        nb = nbrs[u]
        dist[s, nb] = rng.uniform(10.0, 50.0, len(nb))
        dist[s, u] = 30.0
        m, fills = 0, [(nb[0], (10, 2)), (nb[-1], (10, 7))]
        if nm == "tie":
            dist[s, nb[0]] = dist[s, nb[-1]] = 5.0
        elif nm == "none":
            dist[s, nb] = np.inf
        elif nm == "one":
            dist[s, nb] = np.inf
            dist[s, nb[1]] = 12.0
            fills = [(nb[0], (10, 2)), (nb[1], (10, 7))] + [(v, (10, 1)) for v in nb[2:]]
        elif nm == "maxn0":
            dist[s, nb[0]] = 2.0
            fills = [(u, (0, 3)), (nb[0], (0, 5))]
        elif nm.startswith("nff_"):
            dist[s, u] = {"nff_below": 9.75, "nff_equal": 10.0, "nff_above": 10.25}[nm]
        elif nm == "big":
            m = 1
            dist[s, u] = 200.0
        put(nm, m, u, s, fills)
    for i, r in enumerate(hub_ranks):
        s = len(names) + i
        nb = nbrs[hub]
        assert r < len(nb)
        dist[s, nb] = rng.uniform(10.0, 50.0, len(nb))
        dist[s, nb[r]] = 1.0
        dist[s, hub] = 20.0
        put(f"hub_rank_{r}", i, hub, s, [(v, (10, 1 + k % 3)) for k, v in enumerate(nb)] + [(nb[r], (10, 9))])
    u = road["maxn0"]                                              # last, so that no other case's fills undo it
    obs[0, u, OBS_MAXN] = obs[0, nbrs[u][0], OBS_MAXN] = 0
    adv = np.where(head > 0, rng.normal(size=(M, N)) * 24.0 - 4.0, 0.0).astype(np.float32)      # |e| on both sides of 1
    return dict(ei=ei, N=N, obs=obs, head=head, live=head > 0, frames_left=frames_left, dist=dist, slot=slot, adv=adv,
                named=named, timestep=CRAFT_TAU, nbrs=nbrs, hub=hub)
