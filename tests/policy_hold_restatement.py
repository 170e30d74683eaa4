"""TEST INFRASTRUCTURE: the hold rule on a POLICY's action (``ops.fused_hold_policy_actions``) restated on the
CPU with the oracle's own pieces, in the manner of ``router_hold_restatement``: ``oracle.sim.apply_action`` on a recorded
action, then the rule on ``x[:, SEL]``

    SELECTED_ROAD[i] = i   where   row i holds somebody, its head agent h lies in [0, A), its SELECTED_ROAD is the target
                                   v of one of its out-edges (a rank, not a raw or carried code) and v == DESTINATION[h],
                                   integers compared

then the rest of ``oracle.sim.env_step`` (core, withdraw, insert, reward), in the ENVIRONMENT's step order. An EMPTY row is
never touched: the one difference from the routers' rule. The same restatement is available with ONE defect at a time
(:data:`DEFECTS`): what a wrong kernel would compute, for the tests that show the right one matters."""
import types

import torch

import irregular_graphs as ig

SEL_RAW, SEL_CARRIED = 0x7F, 0x80
PAD = -2                             # no road: pads the out-lists
SENTINEL = -7.0                      # what an untouched row's `sel` keeps in the kernel tests

DEFECTS = ("empty_rows",        # holds empty rows too, reading agent 0 (the routers' head decode)
           "minus_one",         # the hold value is -1 instead of the row's own id
           "any_target",        # holds when ANY out-target of the row is the destination, whatever the row chose
           "slot_float",        # compares after the float conversion, against the destination's SLOT instead of the destination
           "due_only",          # holds only when the head's departure from the row is already due
           "rewrite_action")    # the STORED action (what the update reads) is rewritten too

REASONS = ("hold", "empty", "raw", "carried", "head_range", "other_road")


def out_table(ei, N):
    """-> (succ (N, max out-degree) int64 padded with PAD, deg (N,) int64, out_rank (E,) int64): every road's out-list in
    the plan's CSR order (ascending edge id)."""
    _, orank = ig.edge_ranks(ei, N)
    deg = torch.bincount(ei[0], minlength=N)
    succ = torch.full((N, max(1, int(deg.max()))), PAD, dtype=torch.int64)
    succ[ei[0], orank] = ei[1]
    return succ, deg, orank


def codes_of(value, succ):
    """The rank byte of a SELECTED_ROAD value (k_pack_nodes' rule): the first out-edge whose target converts to it, else
    SEL_RAW. -> (N,) int64."""
    hit = succ.to(value.dtype) == value.unsqueeze(1)
    return torch.where(hit.any(1), torch.argmax(hit.to(torch.int8), dim=1), torch.full((succ.size(0),), SEL_RAW))


def classify(x, agents, succ, deg, Nmax, *, code=None, defect=None, t=None, slot_of=None):
    """-> (hold (N,) bool, reason: list of N names of :data:`REASONS`). ``x`` (N, F) after the action was applied; ``code``
    (N,) the rows' bytes where the caller has them (a carried or raw code cannot be told from a rank in ``x`` alone), else
    derived from ``x[:, SEL]`` by :func:`codes_of`."""
    N, A = x.size(0), agents.size(0)
    col_n, col_sel = 3 * Nmax + 1, 3 * Nmax + 5
    rows = torch.arange(N)
    code = codes_of(x[:, col_sel], succ) if code is None else code.to(torch.int64)
    occupied = x[:, col_n] > 0
    head = x[:, 0].to(torch.int64)
    if defect == "empty_rows":
        head = torch.where(occupied, head, torch.zeros_like(head))
        occupied = torch.ones_like(occupied)
    in_range = (head >= 0) & (head < A)
    d = agents[head.clamp(0, A - 1), 1].to(torch.int64)
    ranked = (code < SEL_RAW) & (code < deg)
    v = succ[rows, code.clamp(max=succ.size(1) - 1)]
    match = v == d
    if defect == "any_target":
        match = (succ == d.unsqueeze(1)).any(1)
    elif defect == "slot_float":
        match = v.to(torch.float32) == slot_of[d.clamp(0, N - 1)].to(torch.float32)
    elif defect == "due_only":
        match = match & (x[:, 2 * Nmax] <= float(t))
    elif defect not in (None, "empty_rows", "minus_one", "rewrite_action"):
        raise ValueError(f"unknown defect {defect!r}")
    hold = occupied & in_range & ranked & match
    reason = []
    for h, o, c, r, a in zip(hold.tolist(), occupied.tolist(), code.tolist(), ranked.tolist(), in_range.tolist()):
        reason.append("hold" if h else "empty" if not o else "carried" if c >= SEL_CARRIED else "raw" if not r else
                      "head_range" if not a else "other_road")
    return hold, reason


def apply_rule(x, agents, succ, deg, Nmax, *, code=None, defect=None, t=None, slot_of=None):
    """The rule on ``x[:, SEL]``, in place -> the holding rows (N,) bool."""
    hold, _ = classify(x, agents, succ, deg, Nmax, code=code, defect=defect, t=t, slot_of=slot_of)
    own = torch.arange(x.size(0), dtype=x.dtype) if defect != "minus_one" else torch.full((x.size(0),), -1.0, dtype=x.dtype)
    col = 3 * Nmax + 5
    x[:, col] = torch.where(hold, own, x[:, col])
    return hold


def expected_bytes(x, agents, succ, deg, Nmax, code, sel, **kw):
    """What the kernel must leave behind on one environment: ``x`` its exported state, ``code`` (N,) uint8 and ``sel`` (N,)
    fp32 the packed state's bytes and raw values before the call -> (sel8, sel, held): the holding rows carry SEL_RAW and
    their own id, every other entry is the input's."""
    hold, _ = classify(x, agents, succ, deg, Nmax, code=code, **kw)
    sel8 = torch.where(hold, torch.full_like(code, SEL_RAW), code)
    out = torch.where(hold, torch.arange(x.size(0), dtype=sel.dtype), sel)
    return sel8, out, int(hold.sum())


def onehot_of_bytes(code, ei, orank):
    """Rank bytes (N,) -> the action one-hot (E,) of ``oracle.sim.apply_action``: a carried or raw byte selects nothing."""
    c = code.to(torch.int64)[ei[0]]
    return ((c < SEL_RAW) & (c == orank)).to(torch.int64)


def slots_of(agents, N):
    dests = sorted({int(d) for d in agents[:, 1].tolist() if 0 <= d < N})
    slot_of = torch.full((N,), -1, dtype=torch.int64)
    slot_of[dests] = torch.arange(len(dests))
    return slot_of


def replay(net, pop, actions, gumbel_of, t_start, hold=True, *, defect=None):
    """One environment from the empty network: per frame t ``oracle.sim.apply_action`` on ``actions[t]`` ((N,) rank
    bytes, the policy's own choice), the rule, the rest of ``oracle.sim.env_step``. ``hold=False``: the environment as it
    is without the rule. -> dict: reward (list), x, agents, held (per frame), arrivals, stored (the action bytes an update
    would read: the input's, except under the rewrite defect), reasons (counts of :data:`REASONS` over all frames and rows),
    held_occupied, error (None, or (frame, message) where the oracle's frame raised: the -1 defect under an entering
    agent)."""
    from oracle import sim
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    adj = net.dense_adjacency()
    succ, deg, orank = out_table(ei, N)
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    slot_of = slots_of(ag, N)
    no_action = torch.zeros(ei.size(1), dtype=torch.long)
    reward, held, stored, error = [], [], [], None
    reasons = {k: 0 for k in REASONS}
    for t in range(len(actions)):
        clock = float(t_start + t)
        code = actions[t].to(torch.int64)
        sim.apply_action(x, ei, onehot_of_bytes(code, ei, orank), Nmax)
        kept = code.clone()
        n_held = 0
        if hold:
            _, why = classify(x, ag, succ, deg, Nmax)
            for w in why:
                reasons[w] += 1
            m = apply_rule(x, ag, succ, deg, Nmax, defect=defect, t=clock, slot_of=slot_of)
            n_held = int(m.sum())
            if defect == "rewrite_action":
                kept[m] = SEL_RAW
        held.append(n_held)
        stored.append(kept)
        try:
            out = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=gumbel_of(t),
                               congestion_constant=net.congestion_constant)
        except IndexError as e:
            error = (t, str(e))
            break
        reward.append(float(out["reward"]))
    return dict(reward=reward, x=x, agents=ag, held=held, arrivals=int(ag[1:, sim.DONE].sum()), stored=torch.stack(stored),
                reasons=reasons, error=error)


# ---- crafted packed states: the kernel's cases, on the host -------------------------------------------------------------------
def network(name):
    if name != "torus":
        return ig.graph(name)
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def crafted(name, K, seed=0):
    """-> namespace: net, N, Nmax, succ, deg, x (K, N, F), ag (K, A, 9), code (K, N) uint8, sel (K, N) fp32, rows (name ->
    road), t. Base: ``ig.random_state`` (consistent FIFOs with stale dead slots; four states, environment b takes b % 4), a
    random rank on every road with out-edges (a carried byte on the others), destinations uniform over the roads, and on
    every third occupied road the head agent bound for the road it chose: the rule's holds. Crafted, the same roads in every
    environment:
      near        occupied, rank 0 leads to the head's destination                                  -> holds
      far         the road with the most out-edges, its LAST rank leads to the head's destination   -> holds
      rank4       a road with five out-edges or more, rank 4 leads to the destination (off the torus) -> holds
      raw         occupied, raw code whose value IS the head's destination and a successor          -> left alone
      carried     occupied, carried code whose rank leads to the head's destination                 -> left alone
      head_hi     occupied, head id A + 3                                                           -> left alone
      other_road  occupied, rank 1 leads to the destination but the road chose rank 0               -> left alone
      empty       count 0, clean; agent 0 is bound for the road it chose                            -> left alone
      stale       count 0, slot 0 holds agent 11 (a DIRTY row), who is bound for the road it chose  -> left alone
      own         occupied, the head is bound for the road itself                                   -> left alone"""
    net = network(name)
    N, Nmax = net.num_roads, net.Nmax
    col_n = 3 * Nmax + 1
    succ, deg, _ = out_table(net.edge_index, N)
    g = torch.Generator().manual_seed(4200 + seed)
    base = [ig.random_state(net, seed=900 + b + 10 * seed, t=200.0) for b in range(min(K, 4))]
    x = torch.stack([base[b % len(base)] for b in range(K)]).clone()
    A = int(x[:, :, :Nmax].max()) + 5
    ag = torch.zeros((K, A, 9))
    ag[:, :, 1] = torch.randint(0, N, (K, A), generator=g).float()
    code = (torch.rand((K, N), generator=g) * deg.clamp(min=1)).long().clamp(max=126)
    code = torch.where(deg.unsqueeze(0) > 0, code, torch.full_like(code, SEL_CARRIED))
    sel = torch.full((K, N), SENTINEL)
    hub = int(torch.argmax(deg))
    cands = [r for r in range(N) if r != hub and deg[r] >= 2 and succ[r, 0] != succ[r, 1] and r not in succ[r].tolist()]
    names = ("near", "raw", "carried", "head_hi", "other_road", "empty", "stale", "own")
    assert len(cands) >= len(names) + 1
    rows = dict(zip(names, cands))
    rows["far"] = hub
    big = [r for r in cands[len(names):] if deg[r] >= 5]
    if big:
        rows["rank4"] = big[0]
    crafted_rows = set(rows.values())
    # every third occupied road: its head is bound for the road it chose
    for b in range(K):
        k = 0
        for i in range(N):
            if i in crafted_rows or deg[i] == 0 or x[b, i, col_n] == 0:
                continue
            k += 1
            h = int(x[b, i, 0])
            if k % 3 == 0 and 0 < h < A:
                ag[b, h, 1] = float(succ[i, code[b, i]])
    for r in ("near", "far", "rank4", "raw", "carried", "head_hi", "other_road", "own"):
        if r in rows:
            x[:, rows[r], col_n] = x[:, rows[r], col_n].clamp(min=1)
    heads = dict(near=1, far=2, rank4=3, raw=4, carried=5, other_road=6, own=7)
    for r, h in heads.items():
        if r in rows:
            x[:, rows[r], 0] = float(h)

    def bind(r, rank, byte=None):
        i = rows[r]
        code[:, i] = rank if byte is None else byte
        ag[:, heads[r], 1] = float(succ[i, rank])

    bind("near", 0)
    bind("far", int(deg[hub]) - 1)
    x[:, rows["near"], 2 * Nmax] = 250.0                # not yet due at t = 200: the rule holds all the same
    x[:, rows["far"], 2 * Nmax] = 195.0                 # due
    if "rank4" in rows:
        bind("rank4", 4)
    bind("raw", 0, SEL_RAW)
    sel[:, rows["raw"]] = float(succ[rows["raw"], 0])
    bind("carried", 1, SEL_CARRIED | 1)
    x[:, rows["head_hi"], 0] = float(A + 3)
    code[:, rows["head_hi"]] = 0
    code[:, rows["other_road"]] = 0
    ag[:, heads["other_road"], 1] = float(succ[rows["other_road"], 1])
    code[:, rows["own"]] = 0
    ag[:, heads["own"], 1] = float(rows["own"])
    i = rows["empty"]                                   # clean and empty: the routers' rule would read agent 0 here
    x[:, i, :3 * Nmax] = 0.0
    x[:, i, col_n] = 0.0
    code[:, i] = 0
    ag[:, 0, 1] = float(succ[i, 0])
    i = rows["stale"]                                   # empty, slot 0 holds agent 11 (DIRTY, no garbage pending)
    x[:, i, col_n] = 0.0
    x[:, i, 0], x[:, i, Nmax], x[:, i, 2 * Nmax] = 11.0, 150.0, 160.0
    code[:, i] = 1
    ag[:, 11, 1] = float(succ[i, 1])
    # one road is nobody's destination: from it on a destination's SLOT (its rank among the destinations) is not its id
    bound = {int(v) for v in ag[:, list(heads.values()) + [0, 11], 1].flatten().tolist()}
    skip = next(r for r in range(N) if r not in bound)
    ag[:, :, 1] = torch.where(ag[:, :, 1] == float(skip), torch.full_like(ag[:, :, 1], float((skip + 1) % N)), ag[:, :, 1])
    return types.SimpleNamespace(name=name, net=net, N=N, Nmax=Nmax, succ=succ, deg=deg, x=x, ag=ag, A=A,
                                 code=code.to(torch.uint8), sel=sel, rows=rows, t=200.0)


def with_selected_road(cr, b):
    """Environment b's crafted state with the bytes applied to ``x[:, SEL]``, as the packed state exports it: a rank names
    its target, a raw code its value, a carried code the target of its rank bits."""
    x = cr.x[b].clone()
    c = cr.code[b].to(torch.int64)
    rank = (c & 0x7F).clamp(max=cr.succ.size(1) - 1)
    target = cr.succ[torch.arange(cr.N), rank].to(x.dtype)
    is_rank = ((c & 0x7F) < SEL_RAW) & ((c & 0x7F) < cr.deg)
    col = 3 * cr.Nmax + 5
    x[:, col] = torch.where(is_rank, target, torch.where((c & 0x7F) == SEL_RAW, cr.sel[b], x[:, col]))
    return x
