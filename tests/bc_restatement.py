"""TEST INFRASTRUCTURE: behaviour cloning of the shortest-path router restated on the CPU.

  * the LABEL rule of ``ops.fused_expert_labels`` on the exported state ``x``, the agent table and a next-hop table:
    label[i] = the rank, among row i's out-edges in the plan's CSR order, of next_hop[slot(d)][i], d the destination of the
    row's head agent — and IGNORE where the row is empty, where head, destination or slot is out of range (the select
    kernel leaves such a row untouched) and where the next hop matches no out-edge (it writes the raw code);
  * the LOSS of ``ops.graphdist_bc``: per labelled node (byte < min(out-degree, 0x7F)) the cross-entropy of the segment
    softmax of logits / T, the counts, the hits (first maximum in CSR order) and the gradient, in float64 or in fp32;
  * the update LOOP for the embedding head (float64, torch autograd, ``update_restatement.adam64``).

Each is available with ONE defect at a time (:data:`LABEL_DEFECTS`, :data:`LOSS_DEFECTS`): what a wrong kernel would compute,
for the tests that show the right one matters. Helpers of ``policy_hold_restatement`` are reused by import."""
import types

import torch

import policy_hold_restatement as PH
import update_restatement as R

IGNORE = 0xFF
SEL_RAW = PH.SEL_RAW

LABEL_DEFECTS = ("empty_rows",     # labels empty rows too, reading agent 0 (the routers' head decode)
                 "held_table",     # labels from the HELD value: next hop == destination -> own id -> raw -> ignored
                 "rank4",          # the rank search stops after four out-edges
                 "wrong_env")      # environment b reads environment b + 1's table
LOSS_DEFECTS = ("wrong_segment",   # reads logits at the position in source-sorted order instead of the edge id
                "no_temperature",  # the gradient lacks the division by the temperature
                "ignored_grad",    # an ignored node of non-zero out-degree gets the softmax as gradient
                "last_max",        # a hit is counted against the LAST maximum
                "per_sample")      # grad_scale is applied per sample: 1 / n_labelled[m] instead of the caller's global factor


# ---- labels ----------------------------------------------------------------------------------------------------------------
def expert_labels(x, agents, dest_slot, table, succ, Nmax, *, defect=None):
    """One environment. ``x`` (N, F) exported state, ``agents`` (A, 9), ``dest_slot`` (N,) int64 (-1: no column), ``table``
    (D, N) int64 next hops [slot][row], ``succ`` (N, max out-degree) of ``PH.out_table`` -> (N,) int64 label bytes."""
    N, A, D = x.size(0), agents.size(0), table.size(0)
    rows = torch.arange(N)
    occupied = x[:, 3 * Nmax + 1] > 0
    head = x[:, 0].to(torch.int64)
    if defect == "empty_rows":
        head = torch.where(occupied, head, torch.zeros_like(head))
        occupied = torch.ones_like(occupied)
    ok = occupied & (head >= 0) & (head < A)
    dest = agents[head.clamp(0, A - 1), 1].to(torch.int64)
    ok = ok & (dest >= 0) & (dest < N)
    slot = dest_slot[dest.clamp(0, N - 1)]
    ok = ok & (slot >= 0) & (slot < D)
    nh = table[slot.clamp(0, max(D - 1, 0)), rows]
    if defect == "held_table":
        nh = torch.where(nh == dest, rows, nh)
    code = PH.codes_of(nh.to(torch.float32), succ[:, :4] if defect == "rank4" else succ)
    return torch.where(ok & (code < SEL_RAW), code, torch.full_like(code, IGNORE))


def expert_labels_envs(x, agents, dest_slot, tables, succ, Nmax, *, defect=None):
    """K environments: ``x`` (K, N, F), ``agents`` (K, A, 9), ``tables`` (K, D, N) or (D, N) shared -> (K, N) uint8."""
    K = x.size(0)
    out = []
    for b in range(K):
        tb = tables if tables.dim() == 2 else tables[(b + 1) % K if defect == "wrong_env" else b]
        out.append(expert_labels(x[b], agents[b], dest_slot, tb, succ, Nmax, defect=None if defect == "wrong_env" else defect))
    return torch.stack(out).to(torch.uint8)


def crafted_labels(name, K, seed=0):
    """``PH.crafted``'s state with a crafted next-hop table per environment -> namespace (PH.crafted's fields plus
    dests, dest_slot (N,) int64, tables (K, D, N) int64, why: row name -> the label the rule must give there, one value
    or one per environment).
    Table entries: a random out-target of the row (any rank: ranks >= 4 on the hubs) three times out of four, else -1, the
    row itself or a road that is no successor. One destination (``no_slot``) has no column. Crafted rows, the same in every
    environment (heads as in PH.crafted):
      near        the next hop IS the head's destination (rank 0) in the even environments, the rank-1 target in the odd ones
                                                                                   -> 0 / 1    (held_table: ignored; wrong_env)
      far         the hub, next hop = its LAST out-target                          -> deg - 1  (rank4: ignored off the torus)
      rank4       a road with >= 5 out-edges, next hop = rank 4                    -> 4
      raw         next hop = -1                                                    -> ignored (raw)
      carried     next hop = the row itself                                        -> ignored (raw)
      other_road  next hop = a road that is no successor                           -> ignored (raw)
      own         the head's destination has no column                             -> ignored (untouched)
      head_hi     head id A + 3                                                    -> ignored (untouched)
      empty       count 0, agent 0's next hop is rank 0                            -> ignored (empty_rows: 0)
      stale       count 0, DIRTY                                                   -> ignored"""
    cr = PH.crafted(name, K, seed)
    N, succ, deg, rows = cr.N, cr.succ, cr.deg, cr.rows
    g = torch.Generator().manual_seed(7700 + seed)
    heads = dict(near=1, far=2, rank4=3, raw=4, carried=5, other_road=6, own=7)
    ag = cr.ag
    # `own`'s head is bound for a road that gets no column (nobody crafted is bound for it)
    fixed = {int(ag[0, h, 1]) for r, h in heads.items() if r != "own" and r in rows} | {int(ag[0, 0, 1]), int(ag[0, 11, 1])}
    no_slot = next(r for r in range(N) if r not in fixed)
    ag[:, heads["own"], 1] = float(no_slot)
    d_all = sorted({int(d) for d in ag[:, :, 1].flatten().tolist() if 0 <= d < N} - {no_slot})
    dests = torch.tensor(d_all, dtype=torch.int64)
    D = dests.numel()
    dest_slot = torch.full((N,), -1, dtype=torch.int64)
    dest_slot[dests] = torch.arange(D)
    pick = (torch.rand((K, D, N), generator=g) * deg.clamp(min=1)).long()
    tables = succ[torch.arange(N).view(1, 1, N), pick.clamp(max=succ.size(1) - 1)]
    kind = torch.rand((K, D, N), generator=g)
    foreign = torch.tensor([next(c for c in range(N) if c != r and c not in succ[r].tolist()) for r in range(N)])
    tables = torch.where(kind < 0.75, tables, torch.where(kind < 0.85, torch.full_like(tables, -1),
                                                          torch.where(kind < 0.92, torch.arange(N).expand(K, D, N),
                                                                      foreign.expand(K, D, N))))
    tables = torch.where(deg.view(1, 1, N) > 0, tables, torch.full_like(tables, -1))

    def put(r, value, agent=None):
        h = heads[r] if agent is None else agent
        tables[:, dest_slot[int(ag[0, h, 1])], rows[r]] = value

    hub = rows["far"]
    put("near", int(succ[rows["near"], 0]))
    tables[1::2, dest_slot[int(ag[0, heads["near"], 1])], rows["near"]] = int(succ[rows["near"], 1])
    put("far", int(succ[hub, int(deg[hub]) - 1]))
    if "rank4" in rows:
        put("rank4", int(succ[rows["rank4"], 4]))
    put("raw", -1)
    put("carried", rows["carried"])
    put("other_road", int(foreign[rows["other_road"]]))
    put("empty", int(succ[rows["empty"], 0]), agent=0)
    why = dict(near=[b % 2 for b in range(K)], far=int(deg[hub]) - 1, raw=IGNORE, carried=IGNORE, other_road=IGNORE, own=IGNORE, head_hi=IGNORE,
               empty=IGNORE, stale=IGNORE)
    if "rank4" in rows:
        why["rank4"] = 4
    return types.SimpleNamespace(**vars(cr), dests=dests, dest_slot=dest_slot, tables=tables, why=why, no_slot=no_slot)


# ---- the loss ----------------------------------------------------------------------------------------------------------------
def csr_edges(ei, N):
    """-> (eid (N, max out-degree) int64 padded with -1, deg (N,), pos (N, max out-degree)): every node's out-edge ids in the
    plan's CSR order (ascending edge id) and their positions in the source-sorted edge list."""
    _, orank = PH.ig.edge_ranks(ei, N)
    deg = torch.bincount(ei[0], minlength=N)
    width = max(1, int(deg.max()))
    eid = torch.full((N, width), -1, dtype=torch.int64)
    eid[ei[0], orank] = torch.arange(ei.size(1))
    start = torch.cumsum(deg, 0) - deg
    pos = torch.where(eid >= 0, start.unsqueeze(1) + torch.arange(width).unsqueeze(0), torch.full_like(eid, -1))
    return eid, deg, pos


def bc_loss(ei, N, logits, labels, temperature=1.0, grad_scale=1.0, dtype=torch.float64, *, defect=None):
    """``logits`` (M, E), ``labels`` (M, N) uint8 -> dict: nll (M,) float64, n_labelled, n_hit (M,) int64, grad (M, E) of
    ``dtype``, loss (M, N) per node (0 where ignored). Every operation in ``dtype``, in the kernel's order: z = l / T, the
    maximum, the sum of exp(z - mx) left to right, log s + mx - z_label; gradient (grad_scale (p - [j = label])) / T. The
    per-sample sum of the losses is taken in float64 either way."""
    eid, deg, pos = csr_edges(ei, N)
    M, E = logits.shape
    width = eid.size(1)
    valid = eid >= 0
    src = pos if defect == "wrong_segment" else eid
    T = torch.tensor(temperature, dtype=dtype)
    z = logits.to(dtype)[:, src.clamp(min=0)] / T                                     # (M, N, width)
    z = torch.where(valid.unsqueeze(0), z, torch.full_like(z, float("-inf")))
    lab = labels.to(torch.int64)
    labelled = lab < torch.minimum(deg, torch.tensor(0x7F)).unsqueeze(0)            # (M, N)
    mx = z.max(dim=2).values
    mx = torch.where(deg.unsqueeze(0) > 0, mx, torch.zeros_like(mx))
    ex = torch.where(valid.unsqueeze(0), torch.exp(z - mx.unsqueeze(2)), torch.zeros_like(z))
    s = torch.zeros_like(mx)
    for j in range(width):
        s = s + ex[:, :, j]
    safe = lab.clamp(max=width - 1)
    z_lab = torch.gather(torch.where(valid.unsqueeze(0), z, torch.zeros_like(z)), 2, safe.unsqueeze(2)).squeeze(2)
    s1 = torch.where(s > 0, s, torch.ones_like(s))
    loss = torch.where(labelled, torch.log(s1) + mx - z_lab, torch.zeros_like(mx))
    if defect == "last_max":
        arg = width - 1 - torch.argmax(torch.flip(z, dims=[2]), dim=2)
    else:
        arg = torch.argmax(z, dim=2)
    hit = labelled & (arg == lab)
    n_lab = labelled.sum(1)
    scale = torch.full((M, 1, 1), grad_scale, dtype=dtype)
    if defect == "per_sample":
        scale = (1.0 / n_lab.clamp(min=1).to(dtype)).view(M, 1, 1)
    onehot = (torch.arange(width).view(1, 1, width) == lab.unsqueeze(2)).to(dtype)
    g = scale * (ex / s1.unsqueeze(2) - onehot)
    if defect != "no_temperature":
        g = g / T
    keep = labelled
    if defect == "ignored_grad":
        g = torch.where(labelled.unsqueeze(2), g, scale * (ex / s1.unsqueeze(2)) / T)
        keep = torch.ones_like(labelled)
    g = torch.where(keep.unsqueeze(2) & valid.unsqueeze(0), g, torch.zeros_like(g))
    grad = torch.zeros((M, E), dtype=dtype)
    grad[:, src[valid]] = g[:, valid]
    return dict(nll=loss.double().sum(1), n_labelled=n_lab, n_hit=hit.sum(1), grad=grad, loss=loss, labelled=labelled)


def loss_logits(ei, N, M, kind, seed=0):
    """(M, E) fp32 logits: "random" N(0, 1); "sharp" N(0, 4) with one out-edge per node raised by 6 (neither uniform nor
    one-hot) and exact ties on every fifth node; "sentinel": random with the prior head's -1e20 on a fifth of the edges."""
    g = torch.Generator().manual_seed(8100 + seed)
    E = ei.size(1)
    lg = torch.randn((M, E), generator=g)
    if kind == "sharp":
        eid, deg, _ = csr_edges(ei, N)
        lg = 2.0 * lg
        pick = (torch.rand((M, N), generator=g) * deg.clamp(min=1)).long()
        e = torch.gather(eid.unsqueeze(0).expand(M, N, -1), 2, pick.unsqueeze(2)).squeeze(2)
        has = (deg > 0).unsqueeze(0).expand(M, N)
        lg[torch.arange(M).unsqueeze(1).expand(M, N)[has], e[has]] += 6.0
        for n in range(0, N, 5):                        # ties: all out-edges of the node carry one value
            if deg[n] > 1:
                lg[:, eid[n, :deg[n]]] = lg[:, eid[n, 0]].clone().unsqueeze(1)
    elif kind == "sentinel":
        lg = torch.where(torch.rand((M, E), generator=g) < 0.2, torch.full_like(lg, -1e20), lg)
    elif kind != "random":
        raise KeyError(kind)
    return lg.contiguous()


def loss_labels(ei, N, M, seed=0):
    """(M, N) uint8 labels of every kind: a random rank on about half of the nodes (the LAST rank on every hub), IGNORE,
    a byte >= the out-degree, 0x7F and carried-style bytes elsewhere; sample 0 all ignored (when M > 1), the last sample one
    labelled node only (when M > 2)."""
    g = torch.Generator().manual_seed(8200 + seed)
    deg = torch.bincount(ei[0], minlength=N)
    rank = (torch.rand((M, N), generator=g) * deg.clamp(min=1)).long()
    rank = torch.where((deg >= 9).unsqueeze(0), (deg - 1).clamp(min=0).unsqueeze(0).expand(M, N), rank)
    kind = torch.rand((M, N), generator=g)
    lab = torch.where(kind < 0.55, rank, torch.where(kind < 0.75, torch.full_like(rank, IGNORE),
                                                     torch.where(kind < 0.85, deg.unsqueeze(0).expand(M, N) + (rank % 3),
                                                                 torch.where(kind < 0.92, torch.full_like(rank, 0x7F),
                                                                             0x80 | rank.clamp(max=0x7E)))))
    lab = lab.clamp(max=0xFF)
    if M > 1:
        lab[0] = IGNORE
    if M > 2:
        n = int(torch.nonzero(deg > 1)[0])
        lab[M - 1] = IGNORE
        lab[M - 1, n] = 1
    return lab.to(torch.uint8).contiguous()


# ---- the update loop, embedding head ---------------------------------------------------------------------------------------------
def bc_loop_embedding(ei, N, labels, emb0, steps, lr, temperature=1.0, dtype=torch.float64):
    """Full-batch behaviour cloning of the embedding head (logit of an edge = embedding of its target road) in float64:
    ``steps`` times the mean cross-entropy over all labelled nodes of ``labels`` (S, N), its gradient by torch autograd, one
    ``adam64`` step (``dtype=torch.float32``: the same operations in fp32, for the tolerance rule's e32). -> dict: nll
    (steps + 1,) mean loss before every step and after the last, acc likewise, emb."""
    eid, deg, _ = csr_edges(ei, N)
    valid = eid >= 0
    lab = labels.to(torch.int64)
    labelled = lab < torch.minimum(deg, torch.tensor(0x7F)).unsqueeze(0)
    W = int(labelled.sum())
    dst = ei[1][eid.clamp(min=0)]                                                   # (N, width) target road of every out-edge

    def evaluate(emb):
        z = torch.where(valid, emb[dst] / temperature, torch.full(dst.shape, float("-inf"), dtype=emb.dtype))
        lse = torch.logsumexp(z, dim=1)
        z_lab = torch.gather(torch.where(valid, z, torch.zeros_like(z)).unsqueeze(0).expand(lab.size(0), -1, -1), 2,
                             lab.clamp(max=eid.size(1) - 1).unsqueeze(2)).squeeze(2)
        loss = torch.where(labelled, lse.unsqueeze(0) - z_lab, torch.zeros_like(z_lab)).sum() / W
        acc = float((labelled & (torch.argmax(z, dim=1).unsqueeze(0) == lab)).sum()) / W
        return loss, acc

    emb = emb0.to(dtype).clone()
    m, v = torch.zeros_like(emb), torch.zeros_like(emb)
    nll, accs = [], []
    for k in range(steps):
        p = emb.clone().requires_grad_(True)
        loss, acc = evaluate(p)
        loss.backward()
        nll.append(float(loss.detach()))
        accs.append(acc)
        emb, m, v = R.adam64(emb, p.grad, m, v, k + 1, lr=lr)
    with torch.no_grad():
        loss, acc = evaluate(emb)
    nll.append(float(loss))
    accs.append(acc)
    return dict(nll=nll, acc=accs, emb=emb, labelled=W)


def free_flow_table(net, dests):
    """The ``free_flow`` expert's table on an empty network: (D, N) int64 next hops [slot][row] by the reverse trees' rule."""
    import baseline_restatement as BR
    from oracle import routing
    N = net.num_roads
    x = net.x.clone()
    x[:, :3 * net.Nmax] = 0
    x[:, 3 * net.Nmax + 1] = 0
    w = routing.edge_travel_time(x, net.edge_index, net.congestion_constant, net.Nmax)
    full = BR.destination_columns(net.edge_index, w, N, list(dests))
    return full[:, list(dests)].t().contiguous()


def collect_expert(net, pop, frames, seed, t_start):
    """The ``expert`` driver with the ``free_flow`` expert on one environment, on the CPU: per frame the labels of the state
    (:func:`expert_labels`), then the holding router's choice (``router_hold_restatement.hold_choice``) and the oracle's
    frame with Gumbel noise from ``seed``. -> dict: labels (frames, N) uint8, x (frames, N, F) the labelled states,
    arrivals, dests, dest_slot, table (D, N)."""
    import router_hold_restatement as RH
    from oracle import sim
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    adj = net.dense_adjacency()
    succ, _, _ = PH.out_table(ei, N)
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    dests = sorted({int(d) for d in ag[:, 1].tolist() if 0 <= d < N})
    dest_slot = torch.full((N,), -1, dtype=torch.int64)
    dest_slot[dests] = torch.arange(len(dests))
    table = free_flow_table(net, dests)
    full = torch.full((N, N), -1, dtype=torch.int64)
    full[:, dests] = table.t()
    g = torch.Generator().manual_seed(seed)
    no_action = torch.zeros(ei.size(1), dtype=torch.long)
    labels, states = [], []
    for t in range(frames):
        labels.append(expert_labels(x, ag, dest_slot, table, succ, Nmax).to(torch.uint8))
        states.append(x.clone())
        x = RH.hold_choice(x, ag, full, Nmax)
        u = torch.rand(ei.size(1), generator=g).clamp(1e-7, 1 - 1e-7)
        sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, float(t_start + t), Nmax, gumbel=-torch.log(-torch.log(u)),
                     congestion_constant=net.congestion_constant)
    return dict(labels=torch.stack(labels), x=torch.stack(states), arrivals=int(ag[1:, sim.DONE].sum()), dests=dests,
                dest_slot=dest_slot, table=table)


# ---- the realisable single-destination case (host and device tests) -----------------------------------------------------------------
SINGLE = dict(agents=128, dest=77, frames=60, seed=11, steps=50, lr=0.05)


def single_destination_case():
    """8 x 8 torus, every agent bound for road 77, departures within 40 s of the episode start -> (net, population, t0)."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    pop = synth.population(SINGLE["agents"], net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    pop[:, 1] = float(SINGLE["dest"])
    return net, pop, EPISODE_START
