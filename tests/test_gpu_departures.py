"""GPU: first-hop routing — tarl_fused_pending_departures and both route launches against
``departure_restatement`` on crafted packed states (the 8 x 8 torus and both irregular graphs) and on live states,
``VecEvaluator(route_departures=True)`` replayed frame for frame by the CPU oracle under the exported device noise (the
free-flow router, the plan follower, a policy head under the hold rule), the test that fails without the feature, and the
one-call rollout with the switch set against its launches queued one by one. Every comparison is ``==``."""
import ctypes

import numpy as np
import pytest
import torch

import departure_restatement as D
import policy_hold_restatement as PH
import sp_cases as S

pytestmark = pytest.mark.gpu

SEL_RAW = 0x7F
BYTE, VALUE = 0x55, -7.0             # what an untouched row's sel8 / sel keep in the kernel tests
T0 = 200.0


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _net(name):
    return _torus8() if name == "torus" else S.case(name).net


def _spread_population(net):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    return synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)


def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


def _pend_want(agents, t, N):
    """(K, A, 9) host tensor -> (N, K) int32, the restatement environment by environment."""
    return torch.from_numpy(np.stack([D.pending(a.numpy(), t, N) for a in agents], axis=1).astype(np.int32))


def _between_guards(ops, plan, fs, t):
    """The launch into the middle of a buffer of garbage -> (pend (N, B) on the host); the bands on both sides must stay."""
    n = plan.num_nodes * fs.B
    buf = torch.full((n + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = buf[64:64 + n].view(plan.num_nodes, fs.B)
    ops.fused_pending_departures(plan, fs, t, out=out)
    assert bool((buf[:64] == 0x5A5A5A5A).all()) and bool((buf[64 + n:] == 0x5A5A5A5A).all())
    return out.cpu()


def _without_window(fs):
    """The handle as an engine packed without ``a_order`` has it: every agent is looked at. -> the pointer to put back."""
    saved = fs.struct.a_order
    fs.struct.a_order = None
    return saved


def _crafted_batch(net, K):
    """``departure_restatement.crafted`` in K environments whose statuses differ: in every odd one the agent that departs
    exactly at t is already on the way, in every third the two agents of one origin are done."""
    c = D.crafted(net, t=T0)
    x = c["x"].unsqueeze(0).repeat(K, 1, 1).contiguous()
    ag = c["agents"].unsqueeze(0).repeat(K, 1, 1).contiguous()
    ag[1::2, c["ids"]["exactly_t"], D.ON_WAY] = 1.0
    ag[2::3, c["ids"]["two_small"], D.DONE] = 1.0
    ag[2::3, c["ids"]["two_large"], D.DONE] = 1.0
    return c, x, ag


def _device_table(c, N):
    """[row][destination] (N, N) -> (dest_slot (N,) int32, next_hop (D, N) int32 [slot][row])."""
    slot = c["slot_of"].to(torch.int32)
    ds = torch.nonzero(slot >= 0).view(-1)
    table = torch.full((ds.numel(), N), -1, dtype=torch.int32)
    table[slot[ds].long()] = c["table"][:, ds].t().to(torch.int32)
    return slot, table.contiguous()


def _packed(ops, net, x, ag, sort_agents=None):
    K = x.size(0)
    plan = ops.Plan(net.edge_index, net.num_roads)
    fs = ops.FusedState(plan, K, ag.size(1), "cuda", net.Nmax)
    xd, agd = x.cuda(), ag.cuda()
    ops.fused_pack(plan, fs, xd, net.Nmax, agd, net.congestion_constant.cuda(), sort_agents=sort_agents,
                   ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    return plan, fs, xd, agd


def _export(ops, plan, fs, xd, Nmax):
    out = xd.clone()
    ops.fused_export(plan, fs, out, Nmax, T0)
    return out.cpu()


STATE = ("hdp", "tl", "gc8", "post", "slots", "a_origin", "a_dest", "a_dep", "a_status", "a_order", "a_dep_sorted", "cur_lo",
         "a_win", "a_ins", "a_rank", "acc_lp", "acc_n", "acc_w", "flags", "st0", "node_rec", "in_rec", "out_pad")


def _snapshot(fs):
    return {k: getattr(fs, k).clone() for k in STATE}


def _expected_bytes(written, value, succ):
    """(sel8, sel) the launch must leave from (BYTE, VALUE) everywhere."""
    w, v = torch.from_numpy(written), torch.from_numpy(value).float()
    code = PH.codes_of(v, succ)
    sel8 = torch.where(w, code, torch.full_like(code, BYTE)).to(torch.uint8)
    sel = torch.where(w & (code == SEL_RAW), v, torch.full_like(v, VALUE))
    return sel8, sel


# ---- 1. pend ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_pend_on_crafted_states(name, K):
    """The crafted agent table with statuses that differ between the environments: with the window, with the window's pointer
    withdrawn, and on a handle packed without ``a_order`` at all; from garbage, between guard bands; twice the same."""
    from tarl_hip import ops
    net = _net(name)
    N = net.num_roads
    c, x, ag = _crafted_batch(net, K)
    want = _pend_want(ag, T0, N)
    assert int((want >= 0).sum()) >= 10 * K
    r = c["rows"]
    assert want[r["two_agents"], 0] == c["ids"]["two_small"] and want[r["just_after_t"], 0] == -1
    assert want[r["on_way_and_done"], 0] == c["ids"]["after_them"]
    if K > 2:
        assert want[r["exactly_t"], 1] == -1 and want[r["two_agents"], 2] == -1 and not torch.equal(want[:, 0], want[:, 1])
    plan, fs, _, _ = _packed(ops, net, x, ag)
    assert fs.struct.a_order and fs.struct.a_win
    got = _between_guards(ops, plan, fs, T0)
    assert torch.equal(got, want)
    assert torch.equal(_between_guards(ops, plan, fs, T0), got)
    saved = _without_window(fs)
    assert torch.equal(_between_guards(ops, plan, fs, T0), want)
    fs.struct.a_order = saved
    plan2, fs2, _, _ = _packed(ops, net, x, ag, sort_agents=False)
    assert not fs2.struct.a_order
    assert torch.equal(_between_guards(ops, plan2, fs2, T0), want)
    # one float later the agent that departs just after t is ready too
    later = float(np.nextafter(np.float32(T0), np.float32(np.inf)))
    assert torch.equal(_between_guards(ops, plan, fs, later), _pend_want(ag, later, N))
    assert _pend_want(ag, later, N)[r["just_after_t"], 0] == c["ids"]["just_after_t"]


@pytest.mark.parametrize("K", [3, 65])
def test_pend_after_a_reset_and_on_a_live_state(K):
    """The spread case under the holding free-flow router: after the reset, and after 20 and 40 live frames (the cursor has
    advanced, the window holds inserted entries): ``pend ==`` the restatement on the exported agent
    tables, with and without the window; the launch writes nothing else."""
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    N = net.num_roads
    ev = VecEvaluator(_engine(net, _spread_population(net), K), "dijkstra_hold", refresh_rate=0)
    eng = ev.eng
    eng.reset()
    for t in (EPISODE_START, EPISODE_START + 17.0):
        assert torch.equal(_between_guards(ops, eng.plan, eng.fs, t), _pend_want(eng.agents.cpu(), t, N))
    for frames in (20, 40):         # half of the departures behind the cursor, then (nearly) all of them
        ev.run(frames)
        assert int(eng.fs.cur_lo.min()) > 0 and int(eng.fs.a_ins.sum()) > 0
        before = _snapshot(eng.fs)
        sel_before = (eng.fs.sel8.clone(), eng.fs.sel.clone())
        for t in (float(eng.time), float(eng.time) + 25.0):
            want = _pend_want(eng.agents.cpu(), t, N)
            assert torch.equal(_between_guards(ops, eng.plan, eng.fs, t), want)
            saved = _without_window(eng.fs)
            assert torch.equal(_between_guards(ops, eng.plan, eng.fs, t), want)
            eng.fs.struct.a_order = saved
        assert frames == 40 or int((want >= 0).sum()) > 0
        for k, v in before.items():
            assert torch.equal(getattr(eng.fs, k), v), k
        assert torch.equal(eng.fs.sel8, sel_before[0]) and torch.equal(eng.fs.sel, sel_before[1])


# ---- 2. the route launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_route_launches_on_crafted_states(name, K):
    """Both lookups on the crafted state (a DIRTY empty row among its roads): sel8 / sel / choice8 / routed ``==`` the
    restatement on the exported x, from sentinel bytes; every other array of the packed state and its export unchanged; one
    shared table == K copies of it; a refused call writes nothing."""
    from tarl_hip import lib, ops
    net = _net(name)
    N, Nmax = net.num_roads, net.Nmax
    c, x, ag = _crafted_batch(net, K)
    succ, deg, _ = PH.out_table(net.edge_index, N)
    slot, table = _device_table(c, N)
    plan, fs, xd, agd = _packed(ops, net, x, ag)
    exported = _export(ops, plan, fs, xd, Nmax)
    u = c["rows"]["dirty_empty"]
    assert bool(((fs.hdp[u, :, 0] & 0xFF) == 0x80).all()) and bool((exported[:, u, 0] == c["ids"]["nonempty_head"]).all())
    assert bool((exported[:, c["rows"]["nonempty"], 3 * Nmax + 1] == 1).all())
    pend = ops.fused_pending_departures(plan, fs, T0)
    rt, ln, want_plan = D.crafted_plan(c)
    before = _snapshot(fs)

    def launch(kind, tbl=None):
        fs.sel8.fill_(BYTE)
        fs.sel.fill_(VALUE)
        c8 = torch.full((K, N), 0xAA, dtype=torch.uint8, device="cuda")
        routed = torch.full((K,), 5, dtype=torch.int32, device="cuda")
        if kind == "table":
            ops.fused_route_departures(plan, fs, pend, slot.cuda(), tbl, choice8=c8, routed=routed)
        else:
            ops.fused_route_departures_plan(plan, fs, pend, torch.from_numpy(rt).cuda(), torch.from_numpy(ln).cuda(),
                                            choice8=c8, routed=routed)
        fs.check_flags()
        return fs.sel8.t().cpu(), fs.sel.t().cpu(), c8.cpu(), routed.cpu() - 5

    for kind in ("table", "plan"):
        s8, sv, c8, routed = launch(kind, table.cuda())
        for b in range(K):
            xb, ab = exported[b].numpy(), ag[b].numpy()
            if kind == "table":
                w, v = D.route_table(xb, ab, c["table"].numpy(), T0, Nmax, slot_of=c["slot_of"].numpy())
            else:
                w, v = D.route_plan(xb, ab, rt, ln, T0, Nmax)
            w8, wv = _expected_bytes(w, v, succ)
            assert torch.equal(s8[b], w8), (kind, b)
            assert torch.equal(sv[b], wv), (kind, b)
            assert int(routed[b]) == int(w.sum()) > 0, (kind, b)
            assert not w[c["rows"]["nonempty"]] and not w[c["rows"]["just_after_t"]] and w[u]
        assert torch.equal(c8, s8)
        for k, val in before.items():
            assert torch.equal(getattr(fs, k), val), (kind, k)
        again = _export(ops, plan, fs, xd, Nmax)
        sel_col = 3 * Nmax + 5
        keep = [j for j in range(exported.size(2)) if j != sel_col]
        assert torch.equal(again[:, :, keep], exported[:, :, keep]), kind
    # what the crafted roads show, environment 0
    s8, sv, _, _ = launch("table", table.cuda())
    r = c["rows"]
    hub_deg = len(c["outs"][r["last_rank"]])
    assert s8[0, r["last_rank"]] == hub_deg - 1 and s8[0, r["rank_ge_4"]] == len(c["outs"][r["rank_ge_4"]]) - 1
    if name != "torus":
        assert s8[0, r["rank_ge_4"]] >= 4
    if name == "HUB126":
        assert hub_deg == 126
    for row in ("next_is_dest", "origin_is_dest"):
        assert s8[0, r[row]] == SEL_RAW and sv[0, r[row]] == float(r[row])
    for row in ("no_slot", "unreachable", "nonempty", "just_after_t"):
        assert s8[0, r[row]] == BYTE and sv[0, r[row]] == VALUE
    p8, pv, _, _ = launch("plan")
    for row, val in want_plan.items():
        if val is None:
            assert p8[0, r[row]] == BYTE and pv[0, r[row]] == VALUE, row
        else:
            code = int(PH.codes_of(torch.tensor([float(val)]), succ[r[row]:r[row] + 1])[0])
            assert p8[0, r[row]] == code and (code != SEL_RAW or pv[0, r[row]] == float(val)), row
    # one table shared by all environments == K copies of it
    a = launch("table", table.cuda())
    b_ = launch("table", table.unsqueeze(0).repeat(K, 1, 1).contiguous().cuda())
    assert all(torch.equal(p, q) for p, q in zip(a, b_))
    # a refused call writes nothing
    L = lib.load()
    fs.sel8.fill_(BYTE)
    fs.sel.fill_(VALUE)
    routed = torch.zeros(K, dtype=torch.int32, device="cuda")
    tb = table.cuda()
    assert L.tarl_fused_route_departures(plan.handle, fs.ref, K, Nmax, fs.A, pend.data_ptr(), slot.cuda().data_ptr(),
                                         tb.data_ptr(), 0, 0, None, routed.data_ptr(), None) == -1
    assert L.tarl_fused_route_departures_plan(plan.handle, fs.ref, K, Nmax, fs.A, pend.data_ptr(), tb.data_ptr(),
                                              tb.data_ptr(), 0, 0, None, routed.data_ptr(), None) == -1
    keep_pend = pend.clone()
    assert L.tarl_fused_pending_departures(plan.handle, fs.ref, K, Nmax, fs.A, ctypes.c_float(float("inf")), pend.data_ptr(),
                                           None) == -1
    assert bool((fs.sel8 == BYTE).all()) and bool((fs.sel == VALUE).all()) and int(routed.sum()) == 0
    assert torch.equal(pend, keep_pend)


# ---- 3. frame for frame ------------------------------------------------------------------------------------------------------------------
def _gumbel_of(ops, eng, noise0, b):
    return lambda t: ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()


def _compare(ev, res, T, runs):
    eng = ev.eng
    rw = ev.reward[:T].cpu()
    for b, r in enumerate(runs):
        assert rw[:, b].tolist() == r["reward"], f"rewards of environment {b}"
        assert torch.equal(r["x"], eng.x[b].cpu()), f"final state of environment {b}"
        assert torch.equal(r["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        assert res.arrived[b] == r["arrivals"]
        if ev.route_departures:
            assert int(res.departures_routed[b]) == r["routed"], f"rows routed in environment {b}"


def _free_flow_run(net, pop, K, T, route):
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    kw = dict(route_departures=True) if route else {}
    ev = VecEvaluator(_engine(net, pop, K), "dijkstra_hold", refresh_rate=0, keep_actions=True, **kw)
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    runs = [D.replay(net, pop, T, 0, _gumbel_of(ops, eng, noise0, b), EPISODE_START, route=route) for b in range(K)]
    _compare(ev, res, T, runs)
    return ev, res, runs


@pytest.fixture(scope="module")
def spread_runs():
    """The spread case (8 x 8 torus, 128 agents, 300 frames, K = 3) under the free-flow hold router, with and without the
    rule, each replayed frame for frame by the restatement under the device's own noise."""
    net = _torus8()
    pop = _spread_population(net)
    return {route: _free_flow_run(net, pop, 3, 300, route) for route in (True, False)}


def test_free_flow_router_with_the_rule_is_replayed_by_the_oracle(spread_runs):
    ev, res, runs = spread_runs[True]
    assert res.settings["route_departures"] is True and res.departures_routed.shape == (3,)
    assert str(res.departures_routed.dtype) == "int64" and int(res.departures_routed.min()) > 0
    assert all(r["changed"] > 0 for r in runs)
    _, off, _ = spread_runs[False]
    assert off.departures_routed is None and "route_departures" not in off.settings
    print(f"[departures, free_flow] rows routed {res.departures_routed.tolist()}, of them changed {[r['changed'] for r in runs]}")


def test_first_hops_deliver_what_the_dummy_agent_strands(spread_runs):
    """THE TEST THAT FAILS WITHOUT THE FEATURE. On the run above the device's arrivals are the restatement's under the same
    noise; they exceed the same evaluator's arrivals without the flag in every environment, and fewer agents are lost
    (ON_WAY and queued nowhere). No arrival threshold is set: the bit-exact replay is the bar."""
    (ev_on, on, runs_on), (ev_off, off, runs_off) = spread_runs[True], spread_runs[False]
    a_on, a_off = [r["arrivals"] for r in runs_on], [r["arrivals"] for r in runs_off]
    l_on, l_off = [r["lost"] for r in runs_on], [r["lost"] for r in runs_off]
    print(f"[departures] arrivals without {a_off} with the rule {a_on}; ON_WAY - queued {l_off} -> {l_on}; return "
          f"{off.episode_return} -> {on.episode_return}")
    assert on.arrived == a_on and off.arrived == a_off
    assert all(w > wo for w, wo in zip(a_on, a_off))
    assert all(w < wo for w, wo in zip(l_on, l_off))
    for ev, lost in ((ev_on, l_on), (ev_off, l_off)):
        Nmax = ev.eng.Nmax
        assert [D.lost(ev.eng.x[b].cpu(), ev.eng.agents[b].cpu(), Nmax) for b in range(3)] == lost


def test_two_runs_with_the_rule_are_bit_identical():
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    pop = _spread_population(net)
    evs = [VecEvaluator(_engine(net, pop, 4), "dijkstra_hold", keep_actions=True, route_departures=True) for _ in range(2)]
    r1, r2 = evs[0].run(80), evs[1].run(80)
    assert r1 == r2 and np.array_equal(r1.departures_routed, r2.departures_routed)
    assert torch.equal(evs[0].eng.x, evs[1].eng.x) and torch.equal(evs[0].eng.agents, evs[1].eng.agents)
    assert torch.equal(evs[0].actions, evs[1].actions)


def test_a_policy_head_under_the_hold_rule_is_replayed_by_the_oracle():
    """``embedding_dijkstra`` in MODE with ``policy_hold`` and the rule, K = 2, 150 frames: the restatement is fed the
    device's recorded actions (the policy's own choice: the rule never shows in them), applies the hold rule and then looks
    the first hops up in the free-flow table of the empty network."""
    from oracle import sim
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    pop = _spread_population(net)
    K, T = 2, 150
    eng = _engine(net, pop, K)
    ff = net.x[:, 3 * Nmax + 2][ei[1]].contiguous().cuda()
    table = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    emb = (0.01 * torch.randn(N, generator=torch.Generator().manual_seed(5))).cuda()
    ev = VecEvaluator(eng, "embedding_dijkstra", emb=emb, prior_table=table, prior_weight=1.0, keep_actions=True,
                      policy_hold=True, route_departures=True)
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit
    actions = ev.actions[:T].cpu()
    succ, deg, orank = PH.out_table(ei, N)
    runs = []
    for b in range(K):
        def head(x, ag, t, b=b):
            sim.apply_action(x, ei, PH.onehot_of_bytes(actions[t, b], ei, orank), Nmax)
            PH.apply_rule(x, ag, succ, deg, Nmax)
            return x
        runs.append(D.replay(net, pop, T, 0, _gumbel_of(ops, eng, noise0, b), EPISODE_START, head=head))
    _compare(ev, res, T, runs)
    assert bool((actions < 4).all()) and int(res.departures_routed.min()) > 0 and int(res.held.min()) > 0
    print(f"[departures, embedding_dijkstra + hold] arrivals {res.arrived}, routed {res.departures_routed.tolist()}")


def test_the_plan_follower_with_the_rule_is_replayed_by_the_oracle():
    """Head ``routes`` with its free-flow fallback, K = 2, 120 frames, on a plan of free-flow routes in which every fourth
    agent has no route (the fallback's byte stays on its origin road) — the plan lookup writes the others' first hops."""
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    pop = _spread_population(net)
    K, T, L = 2, 120, 24
    rt, ln = _free_flow_routes(net, pop, L)
    ln[::4] = 0
    assert int((ln > 0).sum()) > 60
    eng = _engine(net, pop, K)
    ev = VecEvaluator(eng, "routes", routes=(torch.from_numpy(rt).cuda(), torch.from_numpy(ln).cuda()), keep_actions=True,
                      route_departures=True)
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit
    runs = [D.replay(net, pop, T, 0, _gumbel_of(ops, eng, noise0, b), EPISODE_START, plan=(rt, ln)) for b in range(K)]
    _compare(ev, res, T, runs)
    assert int(res.departures_routed.min()) > 0
    print(f"[departures, routes] arrivals {res.arrived}, routed {res.departures_routed.tolist()}")


def _free_flow_routes(net, pop, L):
    """-> (rt (A, L) int32, ln (A,) int32): every agent's walk along the free-flow next-hop table of the empty network, origin
    first; length 0 for agent 0, an unreachable destination or a walk longer than L."""
    from baseline_restatement import destination_columns
    from oracle import routing
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, 3 * Nmax + 1] = 0
    dests = sorted({int(d) for d in pop[:, 1].tolist()})
    table = destination_columns(ei, routing.edge_travel_time(x, ei, net.congestion_constant, Nmax), N, dests)
    A = pop.size(0)
    rt, ln = np.full((A, L), -1, np.int32), np.zeros(A, np.int32)
    for a in range(1, A):
        o, d = int(pop[a, 0]), int(pop[a, 1])
        path = [o]
        while path[-1] != d and len(path) <= L and int(table[path[-1], d]) >= 0:
            path.append(int(table[path[-1], d]))
        if path[-1] == d and len(path) <= L:
            rt[a, :len(path)], ln[a] = path, len(path)
    return rt, ln


def test_dijkstra_is_refused():
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    with pytest.raises(ValueError, match="dijkstra_hold"):
        VecEvaluator(_engine(net, _spread_population(net), 1), "dijkstra", route_departures=True)


# ---- 4. the one-call rollout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("B", [3, 65])
def test_rollout_prior_with_the_switch_equals_its_launches_one_by_one(B, hold):
    """tarl_fused_rollout_prior with tarl_fused_set_departure_router (and, ``hold``, tarl_fused_set_policy_hold) over T = 6
    frames == per frame: logits, draw, [hold,] pending, route, the frame — action bytes, log-probs, rewards, counts, routed
    and the final state bit for bit; switched off again the handle is as it was."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.evaluator import router_buffers
    net = synth.torus_network(6, 5, heterogeneous=True, seed=7)
    N, T, A = net.num_roads, 6, 200
    pops = torch.stack([synth.population(A, N, seed=b, t0=21540, t1=21546) for b in range(B)]).cuda()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    mk = lambda: SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,  # noqa: E731
                           pops.clone(), congestion_constant=net.congestion_constant, seed=11)
    e1, e2 = mk(), mk()
    e1.reset()
    e2.reset()
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()
    dist = ops.all_pairs_shortest_paths(e1.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    dests, slot, weights, table, scratch = router_buffers(e1, None, 1)
    ops.fused_edge_travel_time(e1.plan, e1.fs, out=weights)
    ops.destination_trees_batched(e1.plan, weights[:1], dests, out=table, scratch=scratch)
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    pend = torch.empty((N, B), dtype=torch.int32, device="cuda")
    routed, held = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    if hold:
        ops.fused_set_policy_hold(e1.fs, True, held)
    ops.fused_set_departure_router(e1.fs, True, slot, table[0], pend, routed, plan=e1.plan)
    assert e1.fs.struct.policy_hold == (3 if hold else 2)
    e1.rollout_prior(T, emb, dist, prior_weight=1.0, temperature=1.5, policy_seed=77, policy_counter0=5, choice8=ch,
                     log_prob=lp, reward=rw, counts=ct)
    ops.fused_set_departure_router(e1.fs, False)
    assert e1.fs.struct.policy_hold == (1 if hold else 0)
    if hold:
        ops.fused_set_policy_hold(e1.fs, False)
    assert e1.fs.struct.policy_hold == 0
    routed2, held2 = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    counts_f = torch.zeros((N, B), device="cuda")
    for t in range(T):
        logits = ops.fused_prior_logits(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents, emb, dist, 1.0)
        c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        lp2 = ops.graphdist_rollout(e2.plan, logits, 1.5, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
        if hold:
            ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
        p2 = ops.fused_pending_departures(e2.plan, e2.fs, float(e2.time))
        ops.fused_route_departures(e2.plan, e2.fs, p2, slot, table[0], routed=routed2)
        e2.frame_fused(skip_choice=True, counts=counts_f)
        assert torch.equal(c8, ch[t]) and torch.equal(lp2, lp[t]), t
        assert torch.equal(counts_f, ct[t + 1].float()) and torch.equal(e2.reward, rw[t]), t
    assert torch.equal(routed, routed2) and int(routed.sum()) > 0 and torch.equal(held, held2)
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert torch.equal(pend, p2)


# ---- 5. the trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer_case(hold):
    """A 5 x 4 torus, B = 96, 200 agents, T = 14, the per-edge MLP head -> (trainer on engine 1 with ``route_departures`` and
    ``policy_hold=hold``, twin engine 2, logits_of(engine, observation), TEMP)."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(5, 4, heterogeneous=True, seed=3)
    N = net.num_roads
    B, A, T, M, TEMP = 96, 200, 14, 20, 400.0
    pops = torch.stack([synth.population(A, N, seed=40 + b, t0=21540, t1=21552) for b in range(B)])

    def engine():
        return SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                         pops.clone().cuda(), congestion_constant=net.congestion_constant, seed=9)
    torch.manual_seed(1)
    pol = MPNNPolicyNet(net.edge_index, N, None, device="cuda")
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    mlp = [pol.edge_mlp[0].weight, pol.edge_mlp[0].bias, pol.edge_mlp[2].weight, pol.edge_mlp[2].bias,
           pol.edge_mlp[4].weight, pol.edge_mlp[4].bias]

    def logits_of(e, obs):
        return ops.policy_edge_mlp(e.plan, obs, e.ec, ops.EdgeMlpWeights(*(p.data for p in mlp)), precision="fp32")
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    e1, e2 = engine(), engine()
    tr = VecPPOTrainer(e1, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=extra, policy="edge_mlp", temperature=TEMP, policy_hold=hold, route_departures=True,
                       edge_mlp_params=mlp, policy_precision="fp32")
    tr.obs_idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(6))[:M]
    return tr, e2, logits_of, TEMP


@pytest.mark.parametrize("hold", [False, True])
def test_collect_with_the_rule_equals_its_launches_one_by_one(hold):
    """One ``collect()`` with ``route_departures=True`` against head, draw, [hold,] pending, route,
    ``frame_fused(skip_choice=True)`` queued one by one on a twin engine: action bytes, log-probs, rewards, count bytes and
    the routed (and held) counts bit for bit; the stored action is the draw's; the switch is off again afterwards."""
    from tarl_hip import ops
    from tarl_hip.evaluator import router_buffers
    tr, e2, logits_of, TEMP = _trainer_case(hold)
    e1 = tr.eng
    T, B, N = tr.T, e1.B, e1.N
    tr.collect()
    assert e1.fs.struct.policy_hold == 0
    e2.reset()
    dests, slot, weights, table, scratch = router_buffers(e2, None, 1)
    ops.fused_edge_travel_time(e2.plan, e2.fs, out=weights)
    ops.destination_trees_batched(e2.plan, weights[:1], dests, out=table, scratch=scratch)
    ch2 = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct2 = torch.zeros((T + 1, N, B), device="cuda")
    lp2, rw2 = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    routed2, held2 = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    pseed = tr.seed ^ 0x5DEECE66D
    for t in range(T):
        obs = ops.fused_obs16(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents)
        ops.graphdist_rollout(e2.plan, logits_of(e2, obs), TEMP, seed=pseed, counter=1 + t, choice8=ch2[t], sel8=e2.fs.sel8,
                              log_prob=lp2[t])
        if hold:
            ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
        pend = ops.fused_pending_departures(e2.plan, e2.fs, float(e2.time))
        ops.fused_route_departures(e2.plan, e2.fs, pend, slot, table[0], routed=routed2)
        e2.frame_fused(skip_choice=True, reward=rw2[t], counts=ct2[t + 1])
    assert torch.equal(tr.choice, ch2) and torch.equal(tr.logp, lp2) and torch.equal(tr.reward, rw2)
    assert torch.equal(tr.counts.float(), ct2) and torch.equal(tr.departures_routed, routed2)
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert int(routed2.sum()) > 0 and bool((tr.choice < 4).all())
    if hold:
        assert torch.equal(tr.held, held2)
    else:
        assert tr.held is None
    adv, tgt = tr.advantages()
    assert bool(torch.isfinite(tr.minibatch_step(adv, tgt)).all())
    print(f"[departures, collect] {int(routed2.sum())} rows routed in {T} frames x {B} environments")


def test_the_trainer_refuses_the_embedding_head():
    from tarl_hip.trainer import VecPPOTrainer
    net = _torus8()
    with pytest.raises(ValueError, match="not available for policy='embedding'"):
        VecPPOTrainer(_engine(net, _spread_population(net), 1), None, [], rollout_steps=4, policy="embedding",
                      route_departures=True)


# ---- 6. CLI end to end ------------------------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-300"


def _main(argv):
    import importlib
    importlib.import_module("main").main(argv)


def test_cli_eval_envs_end_to_end(tmp_path, capsys):
    import json
    out = tmp_path / "ev"
    _main(["--algo", "mpnn", "--mode", "eval", "--scenario", SCENARIO, "--steps", "60", "--eval-envs", "2", "--policy-hold",
           "--route-departures", "--eval-baseline", "free_flow", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert text.count("departures routed:") == 2 and "selected for their departing agent" in text
    doc = json.load(open(out / "eval_envs.json"))
    for key in ("mode", "baseline"):
        assert doc[key]["route_departures"] is True and len(doc[key]["departures_routed"]) == 2
        assert doc[key]["settings"]["route_departures"] is True
    assert "policy_hold" not in doc["baseline"]


def test_cli_dijkstra_envs_end_to_end(tmp_path, capsys):
    import json
    out = tmp_path / "dj"
    _main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
           "--dijkstra-envs", "2", "--dijkstra-router", "hold", "--route-departures", "--steps", "40", "--output-dir", str(out)])
    assert "departures routed:" in capsys.readouterr().out
    doc = json.load(open(out / "dijkstra_envs.json"))
    assert doc["mode"]["route_departures"] is True and len(doc["mode"]["departures_routed"]) == 2
    assert doc["mode"]["settings"]["route_departures"] is True and doc["mode"]["head"] == "dijkstra_hold"


def test_cli_replan_days_end_to_end(tmp_path, capsys):
    import json
    out = tmp_path / "rp"
    _main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
           "--replan-days", "2", "--replan-envs", "2", "--route-departures", "--steps", "40", "--output-dir", str(out)])
    assert "departures routed:" in capsys.readouterr().out
    doc = json.load(open(out / "replan_envs.json"))
    assert doc["routes"]["route_departures"] is True and len(doc["routes"]["departures_routed"]) == 2


def test_cli_train_end_to_end(tmp_path):
    import json
    run = tmp_path / "run"
    _main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", SCENARIO, "--policy-head", "edge_mlp", "--policy-hold",
           "--route-departures", "--rollout-steps", "32", "--iterations", "2", "--eval-envs", "2", "--steps", "5",
           "--output-dir", str(run)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert len(logs) == 2
    for rec in logs:
        assert rec["train/departures_routed"] >= 0 and rec["eval_vec/departures_routed"] >= 0 and rec["eval_vec/envs"] == 2


def test_cli_refusals():
    for argv, msg in ((["--algo", "mpnn", "--mode", "eval", "--route-departures"], "eval_envs > 0"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--eval-baseline", "dijkstra",
                        "--route-departures"], "dijkstra_hold or free_flow"),
                      (["--algo", "dijkstra", "--mode", "eval", "--dijkstra-envs", "2", "--route-departures"], "hold or free_flow"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--route-departures"], "state-dependent head")):
        with pytest.raises(ValueError, match=msg):
            _main(argv + ["--scenario", SCENARIO])
