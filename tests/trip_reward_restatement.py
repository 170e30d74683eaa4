"""TEST INFRASTRUCTURE: the trip reward written out on the CPU, on the exported agent table (A, 9) of ONE
environment — or (K, A, 9) of several — and a clock. Nothing here calls the code under test.

The rule, after the frame whose clock is t has run completely:

    on_way = #{ a : ON_WAY[a] == 1 and DONE[a] == 0 }             (the packed status byte 1)
    ready  = #{ a : ON_WAY[a] == 0 and DONE[a] == 0 and DEPARTURE_TIME[a] <= t }     (``oracle.sim.insert``'s test, fp32)
    owed   = on_way + ready,      reward = -float32(owed)

Every row of the table counts, agent 0 too. With queued = -(the queue reward of the same frame): owed = queued + lost + ready
and lost = on_way - queued. Each piece is also available with ONE defect at a time (:data:`DEFECTS`), :func:`byte_pass` is the
status pass of the kernel as an emulation on bytes (16-byte groups of a flat (K, A) array whose rows start wherever k * A falls,
head and tail bytes one by one), and :func:`replay` runs ``oracle.sim.env_step`` under a caller's writer of SELECTED_ROAD and
records the parts of every frame."""
import numpy as np
import torch

ORIGIN, DEST, DEP, ON_WAY, DONE = 0, 1, 2, 7, 8

DEFECTS = ("strict_less",        # ready is DEPARTURE_TIME < t
           "done_counted",       # done agents count as on the way
           "agent0_skipped",     # row 0 of the table is left out
           "wrong_row",          # the status is read from the next environment's row (the departure from the right one)
           "head_dropped",       # byte pass: the bytes of a row in front of its first aligned 16-byte group are not read
           "tail_dropped")       # byte pass: the bytes behind its last whole group are not read


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


def status_bytes(agents):
    """(..., A, 9) -> (..., A) uint8 as the pack writes them: 2 done, else 1 on the way, else 0 waiting."""
    ag = np.asarray(agents, dtype=np.float32)
    return np.where(ag[..., DONE] != 0, 2, np.where(ag[..., ON_WAY] != 0, 1, 0)).astype(np.uint8)


def parts(agents, t, defect=None):
    """One environment's table (A, 9) -> (on_way, ready) as ints; ``t`` is compared as fp32."""
    return tuple(int(v) for v in parts_batch(np.asarray(agents)[None], t, defect)[0])


def parts_batch(agents, t, defect=None):
    """(K, A, 9) -> (K, 2) int64 {on_way, ready}."""
    _check(defect)
    ag = np.asarray(agents, dtype=np.float32)
    t = np.float32(t)
    st = status_bytes(ag)
    if defect == "wrong_row":
        st = np.roll(st, -1, axis=0)
    due = ag[..., DEP] < t if defect == "strict_less" else ag[..., DEP] <= t
    on = st == 1
    if defect == "done_counted":
        on = on | (st == 2)
    ready = (st == 0) & due
    if defect == "agent0_skipped":
        on, ready = on[:, 1:], ready[:, 1:]
    return np.stack([on.sum(axis=1), ready.sum(axis=1)], axis=1).astype(np.int64)


def reward_batch(agents, t, defect=None):
    """(K, A, 9) -> (K,) float32: minus the travellers owed."""
    return -(parts_batch(agents, t, defect).sum(axis=1).astype(np.float32))


def byte_pass(status, base=0, defect=None):
    """The kernel's pass over the status bytes, emulated: ``status`` (K, A) uint8, laid out flat from byte address ``base``
    (only ``base % 16`` matters). Per row: the head bytes up to the first 16-byte boundary (at most 15, or the whole row where
    it is shorter), the whole aligned groups, the tail bytes (at most 15). -> (on_way (K,) int64, groups read per row, head and
    tail lengths per row)."""
    _check(defect)
    st = np.ascontiguousarray(status, dtype=np.uint8)
    K, A = st.shape
    flat = st.reshape(-1)
    on, shape = np.zeros(K, np.int64), []
    for k in range(K):
        row = k * A
        head = min((16 - (base + row) % 16) % 16, A)
        groups = (A - head) // 16
        tail0 = head + 16 * groups
        n = 0
        if defect != "head_dropped":
            n += int((flat[row:row + head] == 1).sum())
        for g in range(groups):
            lo = row + head + 16 * g
            assert (base + lo) % 16 == 0
            n += int((flat[lo:lo + 16] == 1).sum())
        if defect != "tail_dropped":
            n += int((flat[row + tail0:row + A] == 1).sum())
        on[k] = n
        shape.append((groups, head, A - tail0))
    return on, shape


def crafted(t=100.0, K=1):
    """An agent table that holds every case the rule distinguishes -> dict(agents (K, A, 9) float32 torch, t, ids: name -> row).
    Agent 0 is READY here (a defect that skips row 0 shows). With K > 1 the environments differ: in every odd one the agent
    that departs exactly at t is already on the way, in every third (from 2) the two waiting-and-due agents are done."""
    t32 = float(np.float32(t))
    after = float(np.nextafter(np.float32(t), np.float32(np.inf)))
    rows, ids = [], {}

    def add(name, dep, on_way=0, done=0):
        ids[name] = len(rows)
        rows.append([3.0, 5.0, float(dep), 0, 0, 0, 0, float(on_way), float(done)])

    add("agent0", t32 - 7)                       # row 0: waiting and due
    add("exactly_t", t32)                        # <= t, to the float
    add("just_after_t", after)                   # not yet
    add("not_due", t32 + 100)                    # waiting, not due
    add("on_way", t32 - 50, on_way=1)
    add("on_way_late_dep", t32 + 500, on_way=1)  # on the way counts whatever its departure says
    add("done", t32 - 60, done=1)                # arrived: owes nothing, although its departure is due
    add("done_2", t32 - 61, done=1)
    add("due_a", t32 - 1)
    add("due_b", t32 - 2)
    ag = torch.tensor(rows, dtype=torch.float32).unsqueeze(0).repeat(K, 1, 1).contiguous()
    ag[1::2, ids["exactly_t"], ON_WAY] = 1.0
    ag[2::3, ids["due_a"], DONE] = 1.0
    ag[2::3, ids["due_b"], DONE] = 1.0
    return dict(agents=ag, t=t32, ids=ids)


def padded(agents, A):
    """(K, A0, 9) -> (K, A, 9): the crafted rows repeated (cut) to A rows, so that every size holds every case in some row."""
    K, A0, _ = agents.shape
    reps = -(-A // A0)
    return agents.repeat(1, reps, 1)[:, :A].contiguous()


def empty_state(net):
    """The network's x with every FIFO empty, and the no-op action of ``oracle.sim.env_step``."""
    from oracle import sim
    c = sim.Cols(net.Nmax)
    x = net.x.clone()
    x[:, :3 * net.Nmax] = 0
    x[:, c.N] = 0
    return x, torch.zeros(net.edge_index.size(1), dtype=torch.long)


def replay(net, pop, frames, gumbel_of, t_start, choose):
    """``frames`` frames of ``oracle.sim.env_step`` from the empty network; in front of every frame ``choose(x, agents, t,
    clock)`` -> x writes SELECTED_ROAD. -> dict: queue (the oracle's reward per frame), trip (-owed per frame), on_way, ready,
    queued, lost (lists over frames), x, agents, arrivals."""
    from oracle import sim
    Nmax, ei = net.Nmax, net.edge_index
    adj = net.dense_adjacency()
    x, no_action = empty_state(net)
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    out = dict(queue=[], trip=[], on_way=[], ready=[], queued=[], lost=[])
    for t in range(frames):
        clock = float(t_start + t)
        x = choose(x, ag, t, clock)
        step = sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, clock, Nmax, gumbel=gumbel_of(t),
                            congestion_constant=net.congestion_constant)
        on, ready = parts(ag.numpy(), clock)
        queued = int(x[:, 3 * Nmax + 1].sum())
        assert float(step["reward"]) == -float(queued)
        out["queue"].append(float(step["reward"]))
        out["trip"].append(-float(on + ready))
        out["on_way"].append(on)
        out["ready"].append(ready)
        out["queued"].append(queued)
        out["lost"].append(on - queued)
    out.update(x=x, agents=ag, arrivals=int(ag[:, sim.DONE].sum()))
    return out


def hold_router(net, pop, route_departures):
    """-> choose(x, agents, t, clock) of :func:`replay`: the free-flow hold router (``router_hold_restatement.hold_choice`` on
    the table of the empty network, built at frame 0), then, with ``route_departures``, the first-hop rule of DESIGN 4.23."""
    import departure_restatement as D
    import router_hold_restatement as H
    from baseline_restatement import destination_columns
    from oracle import routing
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    dests = sorted({int(d) for d in pop[:, 1].tolist() if 0 <= d < N})
    slot_of = torch.full((N,), -1, dtype=torch.int64)
    slot_of[dests] = torch.arange(len(dests))
    state = {}

    def choose(x, ag, t, clock):
        if t == 0:
            state["table"] = destination_columns(ei, routing.edge_travel_time(x, ei, net.congestion_constant, Nmax), N, dests)
        x = H.hold_choice(x, ag, state["table"], Nmax)
        if route_departures:
            w, v = D.route_table(x.numpy(), ag.numpy(), state["table"].numpy(), clock, Nmax, slot_of=slot_of.numpy())
            D.apply(x, w, v, Nmax)
        return x
    return choose


def fixed_selection(sel, Nmax):
    """-> choose of :func:`replay`: SELECTED_ROAD is ``sel`` (N,) in every frame."""
    def choose(x, ag, t, clock):
        x[:, 3 * Nmax + 5] = sel.to(x.dtype)        # (no other column is touched)
        return x
    return choose


def one_agent_case(net, t_start, depart_after=2.0):
    """The case the feature exists for, on ``net`` (a torus: every road has its reverse edge): ONE traveller from road o to a
    road d that is no neighbour of o. -> dict(pop (2, 9), o, v, d, lost_sel (N,)): under ``lost_sel`` every road selects
    itself, except that o selects its first out-neighbour v and v selects o — the traveller is inserted onto v and turns back
    into its EMPTY origin road, where the reference's U-turn double pop loses it."""
    N, ei = net.num_roads, net.edge_index
    outs = [[] for _ in range(N)]
    for s, d in ei.t().tolist():
        outs[s].append(d)
    o = next(r for r in range(N) if any(r in outs[v] for v in outs[r] if v != r))
    v = next(v for v in outs[o] if v != o and o in outs[v])
    d = next(r for r in range(N) if r not in (o, v) and r not in outs[o] and r not in outs[v] and o not in outs[r])
    pop = torch.zeros((2, 9), dtype=torch.float32)
    pop[0, DEP] = 1e9                               # the dummy agent never departs
    pop[1, ORIGIN], pop[1, DEST], pop[1, DEP] = float(o), float(d), float(t_start + depart_after)
    sel = torch.arange(N, dtype=torch.float32)
    sel[o], sel[v] = float(v), float(o)
    return dict(pop=pop, o=o, v=v, d=d, lost_sel=sel)
