"""GPU: the shortest-path router that holds one road short of its destination — tarl_fused_select_next_hop_hold
against ``router_hold_restatement.hold_choice`` on crafted packed states (the 8 x 8 torus and both irregular graphs),
``VecEvaluator(head="dijkstra_hold")`` replayed by the CPU oracle (refreshing and static tables), the finding it answers (the
reference rule delivers nobody on the torus, the hold rule does), the reports and the paired comparison on top of it, its
reproducibility, and the CLI. Every comparison is ``==``."""
import importlib
import json
import types

import numpy as np
import pytest
import torch

import irregular_graphs as ig
import sp_cases as S

pytestmark = pytest.mark.gpu

SEL_RAW = 0x7F
SENTINEL = -7.0                      # no table value: what an untouched row's `sel` keeps
FEW_DESTS = [3, 17, 40, 66, 90, 101, 120, 127]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _case(name):
    """sp_cases.case for the irregular graphs; the 8 x 8 torus in the same shape."""
    if name != "torus":
        return S.case(name)
    net = _torus8()
    N, ei = net.num_roads, net.edge_index
    irank, orank = ig.edge_ranks(ei, N)
    return types.SimpleNamespace(name=name, net=net, N=N, E=ei.size(1), ei=ei, Nmax=net.Nmax, in_rank=irank, out_rank=orank,
                                 **S.lists(ei, N))


def _few_population(net, agents=500, span=40):
    import baseline_restatement as BR
    from tarl_hip.engine import EPISODE_START
    return BR.few_destination_population(agents, net.num_roads, FEW_DESTS, seed=7, t0=EPISODE_START, t1=EPISODE_START + span)


def _engine(net, pop, K, seed=3, env_base=0):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed, env_base=env_base)


def _router(net, pop, K, head="dijkstra_hold", seed=3, **kw):
    from tarl_hip.evaluator import VecEvaluator
    return VecEvaluator(_engine(net, pop, K, seed), head, **kw)


# ---- 1. the select kernel, both forms, on crafted rows -----------------------------------------------------------------------------
def _crafted(c, K):
    """-> dict: x (K, N, F) and ag (K, A, 9) on the host, the crafted rows by name, the table edits. Base: ig.random_state
    (consistent FIFOs, stale dead slots; four different states, environment b takes state b % 4) and destinations uniform
    over the roads. Crafted, the same rows in every environment (heads 1 .. 12 are the agents whose destinations are set):
    own — bound for its own row; minus, beyond, frac — destinations -1, N + 3 and 2.5 (-> 2); id_a, id_b — head ids A and
    A + 40; no_slot — a destination without a tree; no_entry — table entry -1; foreign — an entry that is no successor;
    near — the next hop IS the destination, through the row's first out-edge (rank 0); far — the same through the LAST
    out-edge of the road with the most out-edges (rank >= 4 off the torus); detour — adjacent to its destination, but the
    tree goes elsewhere first; stale — an empty row whose slot 0 holds an old id (DIRTY, no garbage pending)."""
    net, N, Nmax = c.net, c.N, c.Nmax
    col_n = 3 * Nmax + 1
    base = [ig.random_state(net, seed=900 + b, t=200.0) for b in range(min(K, 4))]
    x = torch.stack([base[b % len(base)] for b in range(K)]).clone()
    A = int(x[:, :, :Nmax].max()) + 5
    ag = torch.zeros((K, A, 9))
    ag[:, :, 1] = torch.randint(0, N, (K, A), generator=torch.Generator().manual_seed(901)).float()
    outl = ig.out_lists(net)
    dout = torch.tensor([len(l) for l in outl])
    hub = int(torch.argmax(dout))
    cands = [r for r in range(N) if r != hub and len(outl[r]) >= 2 and outl[r][0] != outl[r][1]]
    assert len(cands) >= 13
    names = ("own", "minus", "beyond", "frac", "id_a", "id_b", "no_slot", "no_entry", "foreign", "near", "detour", "stale")
    rows = dict(zip(names, cands))
    rows["far"] = hub
    for r in rows.values():
        x[:, r, col_n] = x[:, r, col_n].clamp(min=1)
    heads = dict(own=(1, rows["own"]), minus=(2, -1.0), beyond=(3, N + 3.0), frac=(4, 2.5),
                 no_entry=(6, outl[rows["no_entry"]][0]), foreign=(7, outl[rows["foreign"]][0]),
                 near=(8, outl[rows["near"]][0]), far=(9, outl[hub][-1]), detour=(10, outl[rows["detour"]][1]))
    taken = {int(d) for _, d in heads.values()} | {2, outl[rows["stale"]][0]}
    no_tree = next(d for d in range(N) if d not in taken)      # a destination whose tree is withdrawn: nobody crafted needs it
    heads["no_slot"] = (5, no_tree)
    # agent 0, whom every clean empty row reads, keeps a destination with a tree (else a whole environment's empty rows go untouched)
    ag[:, 0, 1] = torch.where(ag[:, 0, 1] == float(no_tree), torch.full((K,), float(rows["own"])), ag[:, 0, 1])
    for name, (agent, dest) in heads.items():
        x[:, rows[name], 0] = float(agent)
        ag[:, agent, 1] = float(dest)
    x[:, rows["id_a"], 0], x[:, rows["id_b"], 0] = float(A), float(A + 40)
    r = rows["stale"]                                   # empty, slot 0 holds agent 11, bound for its first successor
    x[:, r, col_n] = 0.0
    x[:, r, 0], x[:, r, Nmax], x[:, r, 2 * Nmax] = 11.0, 150.0, 160.0
    ag[:, 11, 1] = float(outl[r][0])
    not_succ = next(v for v in range(N) if v != rows["foreign"] and v not in outl[rows["foreign"]])
    edits = [(int(heads["no_entry"][1]), rows["no_entry"], -1), (int(heads["foreign"][1]), rows["foreign"], not_succ),
             (int(heads["near"][1]), rows["near"], int(heads["near"][1])), (int(heads["far"][1]), hub, int(heads["far"][1])),
             (int(heads["detour"][1]), rows["detour"], outl[rows["detour"]][0]),
             (int(ag[0, 11, 1]), rows["stale"], int(ag[0, 11, 1]))]
    return dict(x=x, ag=ag, A=A, rows=rows, edits=edits, no_tree=no_tree, hub_degree=int(dout[hub]), outl=outl)


def _expected(c, x, ag, table_b, slot, hold):
    """One environment on the host: ``hold_choice`` (``dijkstra_choice`` with hold off) on the exported ``x`` -> (sel8, sel)
    as the kernel must leave them from (SEL_RAW, SENTINEL) everywhere. Rows the kernel leaves alone — a head, destination
    or slot out of range — read a stand-in agent here (the oracle indexes without guards) and keep the sentinels."""
    import router_hold_restatement as H
    from oracle import routing
    N, Nmax, A = c.N, c.Nmax, ag.size(0)
    head = x[:, 0].to(torch.int64)
    ok = (head >= 0) & (head < A)
    dest = ag[head.clamp(0, A - 1), 1].to(torch.int64)
    ok &= (dest >= 0) & (dest < N)
    ok &= slot[dest.clamp(0, N - 1)] >= 0
    full = torch.full((N, N), -1, dtype=torch.int64)                 # [row][destination], as the oracle indexes it
    ds = torch.nonzero(slot >= 0).view(-1)
    full[:, ds] = table_b[slot[ds].long()].t().to(torch.int64)
    xs = x.clone()
    xs[~ok, 0] = 1.0                                                 # agent 1: bound for a road with a tree
    out = H.hold_choice(xs, ag, full, Nmax) if hold else routing.dijkstra_choice(xs, ag, None, None, Nmax, next_hop=full)[0]
    value = out[:, 3 * Nmax + 5]
    hit = S.out_table(c).float() == value.unsqueeze(1)
    code = torch.where(hit.any(1), torch.argmax(hit.to(torch.int8), dim=1), torch.full((N,), SEL_RAW))
    sel8 = torch.where(ok, code, torch.full((N,), SEL_RAW)).to(torch.uint8)
    sel = torch.where(ok & (code == SEL_RAW), value, torch.full((N,), SENTINEL))
    return sel8, sel, ok


def _run_select(ops, plan, c, x, ag, slot, table, **kw):
    """Pack, export (the x the oracle reads), fill the outputs with sentinels, launch -> (exported x, sel8, sel, choice8)."""
    K = x.size(0)
    fs = ops.FusedState(plan, K, ag.size(1), "cuda", c.Nmax)
    ops.fused_pack(plan, fs, x.cuda(), c.Nmax, ag.cuda(), c.net.congestion_constant.cuda(),
                   ec=ops.EdgeConst(c.net.edge_attr, "cuda"))
    fs.check_flags()
    exported = x.clone().cuda()
    ops.fused_export(plan, fs, exported, c.Nmax, 200.0)
    fs.sel8.fill_(SEL_RAW)
    fs.sel.fill_(SENTINEL)
    c8 = torch.full((K, c.N), 0x55, dtype=torch.uint8, device="cuda")
    ops.fused_select_next_hop_dest(plan, fs, slot.cuda(), table, choice8=c8, **kw)
    fs.check_flags()
    return exported.cpu(), fs.sel8.t().cpu(), fs.sel.t().cpu(), c8.cpu(), fs


@pytest.mark.parametrize("K", [1, 3, 70])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_hold_select_on_crafted_rows(name, K):
    """Both forms of k_fused_select_next_hop_dest on a crafted packed state (:func:`_crafted`), a table per environment
    from random weights: sel8 / sel / choice8 against the oracle's choice plus the rule on the exported x, sentinel-filled
    outputs untouched on the rows the kernel must leave alone; one shared table (nh_bstride = 0) == K copies of it;
    hold=False == the call without the argument."""
    from tarl_hip import ops
    c = _case(name)
    N, Nmax = c.N, c.Nmax
    plan = ops.Plan(c.ei, N)
    cr = _crafted(c, K)
    x, ag, rows = cr["x"], cr["ag"], cr["rows"]
    w = torch.stack([S.random_weights(c.E, 40 + b) for b in range(K)]).cuda()
    table = ops.destination_trees_batched(plan, w, torch.arange(N, dtype=torch.int64, device="cuda"))      # (K, N, N) [b][d][u]
    slot = torch.arange(N, dtype=torch.int32)
    slot[cr["no_tree"]] = -1
    for d, row, value in cr["edits"]:
        table[:, d, row] = value
    table_h = table.cpu()
    results = {}
    for hold in (False, True):
        exported, sel8, sel, c8, fs = _run_select(ops, plan, c, x, ag, slot, table, hold=hold)
        dirty = ((fs.hdp[..., 0] & 0xFF) == 0x80).t().cpu()
        assert bool(dirty[:, rows["stale"]].all()) and bool((exported[:, rows["stale"], 0] == 11.0).all())
        for b in range(K):
            w8, wsel, ok = _expected(c, exported[b], ag[b], table_h[b], slot, hold)
            assert torch.equal(sel8[b], w8), f"sel8, environment {b}, hold={hold}"
            assert torch.equal(sel[b], wsel), f"sel, environment {b}, hold={hold}"
            for r in ("minus", "beyond", "id_a", "id_b", "no_slot"):
                assert not bool(ok[rows[r]]), r
            assert int(ok.sum()) >= N - 16                      # (the crafted five, and whoever else reads agents 2, 3, 5)
        assert torch.equal(c8, sel8)
        results[hold] = (sel8, sel)
    # what the crafted rows show: the rule acts on near, far and stale and nowhere else among them
    (r8, rs), (h8, hs) = results[False], results[True]
    for b in range(K):
        for r in ("near", "far", "stale"):
            i = rows[r]
            assert r8[b, i] < SEL_RAW and rs[b, i] == SENTINEL and h8[b, i] == SEL_RAW and hs[b, i] == float(i), (b, r)
        assert r8[b, rows["near"]] == 0 and r8[b, rows["far"]] == cr["hub_degree"] - 1
        for r in ("own", "no_entry", "foreign", "detour"):
            i = rows[r]
            assert r8[b, i] == h8[b, i] and rs[b, i] == hs[b, i], (b, r)
        assert h8[b, rows["own"]] == SEL_RAW and hs[b, rows["own"]] == float(rows["own"])
        assert hs[b, rows["no_entry"]] == -1.0 and h8[b, rows["foreign"]] == SEL_RAW
        assert h8[b, rows["detour"]] == 0
        for r in ("minus", "beyond", "id_a", "id_b", "no_slot"):
            assert h8[b, rows[r]] == SEL_RAW and hs[b, rows[r]] == SENTINEL, (b, r)
    if name != "torus":
        assert cr["hub_degree"] - 1 >= 4
    changed = (r8 != h8) | (rs != hs)
    assert int(changed.sum()) >= 3 * K                     # (and on whichever random rows sit next to their destinations)
    # one table shared by all environments == K copies of it, in both forms
    one = table[0].contiguous()
    copies = one.unsqueeze(0).repeat(K, 1, 1).contiguous()
    for hold in (False, True):
        _, a8, asel, ac8, _ = _run_select(ops, plan, c, x, ag, slot, one, hold=hold)
        _, b8, bsel, bc8, _ = _run_select(ops, plan, c, x, ag, slot, copies, hold=hold)
        assert torch.equal(a8, b8) and torch.equal(asel, bsel) and torch.equal(ac8, bc8), hold
        assert torch.equal(a8[0], results[hold][0][0]) and torch.equal(asel[0], results[hold][1][0])
    # hold=False is the op as it always was called
    _, d8, dsel, dc8, _ = _run_select(ops, plan, c, x, ag, slot, table)
    assert torch.equal(d8, r8) and torch.equal(dsel, rs) and torch.equal(dc8, r8)


# ---- 2. replay by the oracle -----------------------------------------------------------------------------------------------------
def _assert_replayed_by_the_oracle(net, pop, K, T, succ, refresh_rate=10):
    """``VecEvaluator(head="dijkstra_hold")`` on K environments for T frames against router_hold_restatement.replay under the
    Gumbel values the kernels consumed, environment by environment: SELECTED_ROAD on every node at every frame (``succ``
    (N, max out-degree): the out-lists, padded with a value no road has; a raw byte: the oracle's value is no successor of
    the node), every reward, the final state and agent table, and the EvalResult against eval_restatement."""
    import eval_restatement as R
    import router_hold_restatement as H
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    N, Nmax = net.num_roads, net.Nmax
    ev = _router(net, pop, K, keep_actions=True, refresh_rate=refresh_rate)
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T and res.head == "dijkstra_hold" and res.deterministic
    dests = {int(d) for d in pop[:, 1].tolist()}
    assert res.settings["refresh_rate"] == refresh_rate and res.settings["hold"] is True
    assert res.settings["destinations"] == len(dests)
    rw = ev.reward[:T].cpu()
    actions = ev.actions[:T].cpu().long()
    succ = succ.float()
    runs = []
    for b in range(K):
        r = H.replay(net, pop, T, refresh_rate,
                     lambda t: ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu(), EPISODE_START)
        assert r["error"] is None and r["max_count"] < Nmax
        for t in range(T):
            code = actions[t, b]
            ranked = code < SEL_RAW
            value = succ[torch.arange(N), code.clamp(max=succ.size(1) - 1)]
            assert torch.equal(value[ranked], r["sel"][t][ranked]), f"SELECTED_ROAD of environment {b}, frame {t}"
            assert not bool((succ[~ranked] == r["sel"][t][~ranked].unsqueeze(1)).any()), f"raw bytes, environment {b}, frame {t}"
            assert rw[t, b] == r["reward"][t], f"reward of environment {b}, frame {t}"
        assert torch.equal(r["x"], eng.x[b].cpu()), f"final state of environment {b}"
        assert torch.equal(r["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        print(f"[hold replay] environment {b}: largest count {r['max_count']:.0f} of {Nmax}, {r['arrivals']} arrivals, the rule "
              f"acted {r['acted']} times ({r['acted_occupied']} on occupied rows), {r['origin_hold']} agents entered through a "
              f"holding origin row, tables built {len(r['tables'])}")
        assert r["acted_occupied"] > 0 and r["core_onto_dest"] == 0
        runs.append(r)
    want = R.per_env(R.summary(torch.stack([r["agents"] for r in runs]).numpy(),
                               np.asarray([r["reward"] for r in runs], dtype=np.float32).T, 10.0, 720), 10.0)
    for b, w in enumerate(want):
        got = dict(arrived=res.arrived[b], on_way=res.on_way[b], not_departed=res.not_departed[b],
                   episode_return=res.episode_return[b], avg=res.avg_travel_time[b], std=res.std_travel_time[b],
                   max=res.max_travel_time[b], p50=res.p50_travel_time[b], p95=res.p95_travel_time[b])
        assert got == w, (b, got, w)
    return res, runs, actions


def test_hold_evaluation_replayed_by_the_oracle():
    """The few-destination case of DESIGN 4.13a (500 agents leaving within 40 s for eight roads), K = 2, T = 120, tables
    rebuilt every 10 frames from each environment's own state. Exact."""
    net = _torus8()
    N, ei = net.num_roads, net.edge_index
    res, runs, _ = _assert_replayed_by_the_oracle(net, _few_population(net), 2, 120, ei[1].view(N, 4))
    assert min(res.arrived) > 0 and all(r["origin_hold"] > 0 for r in runs)
    assert all(len(r["tables"]) == 12 for r in runs)


def test_hold_evaluation_replayed_by_the_oracle_on_an_irregular_graph():
    """MIXED under the load of test_gpu_eval_baseline.IRREGULAR_LOAD, K = 1: out-ranks >= 4, raw bytes from dead ends, from
    rows at their destination and from holding rows."""
    import baseline_restatement as BR
    from tarl_hip.engine import EPISODE_START
    from test_gpu_eval_baseline import IRREGULAR_LOAD as LOAD
    c = S.case("MIXED")
    _, dout = ig.degrees(c.net)
    leads_on = torch.nonzero(dout > 0).view(-1)
    pop = BR.few_destination_population(LOAD["agents"], c.N, LOAD["dests"], seed=7, t0=EPISODE_START,
                                        t1=EPISODE_START + LOAD["span"])
    pop[:, 0] = leads_on[pop[:, 0].long() % leads_on.numel()].float()
    res, runs, actions = _assert_replayed_by_the_oracle(c.net, pop, 1, LOAD["frames"], S.out_table(c))
    assert int(((actions >= 4) & (actions < SEL_RAW)).sum()) > 0 and bool((actions == SEL_RAW).any())
    assert res.arrived[0] > 0


def test_static_tables_replayed_by_the_oracle():
    """``refresh_rate=0``: the tables of frame 0 (the empty network) serve all 60 frames, K = 1."""
    net = _torus8()
    N, ei = net.num_roads, net.edge_index
    res, runs, _ = _assert_replayed_by_the_oracle(net, _few_population(net), 1, 60, ei[1].view(N, 4), refresh_rate=0)
    assert len(runs[0]["tables"]) == 1 and len(runs[0]["weights"]) == 1
    ff = net.x[:, 3 * net.Nmax + 2][ei[0]]
    assert torch.equal(runs[0]["weights"][0], ff)                   # every count 0: free-flow times


# ---- 3. the finding, and its remedy ------------------------------------------------------------------------------------------------
def test_the_reference_rule_strands_and_the_hold_rule_delivers_on_the_torus():
    """128 agents bound anywhere, 300 frames, K = 3: "dijkstra" delivers nobody in any environment (the finding
    must still hold), "dijkstra_hold" somebody in every one (CPU oracle under torch's noise: 0 and 105)."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    ref = _router(net, pop, 3, head="dijkstra").run(300)
    hold = _router(net, pop, 3).run(300)
    print(f"[hold] arrivals {ref.arrived} -> {hold.arrived}, return {ref.episode_return} -> {hold.episode_return}")
    assert not ref.domain_exit and not hold.domain_exit
    assert ref.arrived == [0, 0, 0] and ref.head == "dijkstra" and "hold" not in ref.settings
    assert min(hold.arrived) > 0 and hold.head == "dijkstra_hold"
    assert all(h > r for h, r in zip(hold.episode_return, ref.episode_return))


# ---- 4. the reports ----------------------------------------------------------------------------------------------------------------
def test_every_report_runs_on_the_hold_router_and_perturbs_nothing():
    """K = 2, 120 frames, link counts, occupancy, trips, dynamic gap and turns all on: nothing raises, every pop is
    attributed to an edge (unresolved == 0) and the lost agents are the ON_WAY agents queued nowhere; returns and arrivals
    equal the plain run's."""
    net = _torus8()
    pop = _few_population(net)
    plain_ev = _router(net, pop, 2)
    plain = plain_ev.run(120)
    ev = _router(net, pop, 2, link_counts=True, occupancy=True, trips=True, dynamic_gap=True, turns=True, link_bin_seconds=60)
    res = ev.run(120)
    assert not res.domain_exit and not plain.domain_exit
    from tarl_hip.evaluator import PER_ENV_KEYS
    assert res.episode_return == plain.episode_return and res.arrived == plain.arrived
    assert all(getattr(res, k) == getattr(plain, k) for k in PER_ENV_KEYS) and res.aggregate == plain.aggregate
    assert torch.equal(ev.eng.x, plain_ev.eng.x) and torch.equal(ev.eng.agents, plain_ev.eng.agents)
    assert not bool(ev.turn_acc["unresolved"].any())
    lost = res.turn_lost.sum(axis=(1, 2))
    on_way, queued = np.asarray(res.turn_meta["on_way"]), np.asarray(res.turn_meta["queued"])
    assert np.array_equal(lost, on_way - queued)
    assert res.link_counts is not None and res.occupancy is not None and res.dynamic_gap is not None
    assert int(res.trips["n_done"].sum()) == sum(res.arrived) > 0
    assert int(res.turn_counts.sum()) > 0 and plain.turn_counts is None and plain.trips is None


# ---- 5. the paired comparison has pairs ---------------------------------------------------------------------------------------------
def test_a_mode_run_paired_with_the_hold_baseline_has_usable_pairs():
    """The torus case of test_gpu_trips (embedding seed 32, every other agent bound three MODE steps from its origin), whose
    MODE runs deliver: against "dijkstra" that pairing has no usable pair, against "dijkstra_hold" it has."""
    import link_counts_restatement as O
    from tarl_hip.evaluator import VecEvaluator, paired_report, trip_report
    net = _torus8()
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(32))
    _, _, succ = O.oracle_mode(net, emb)
    pop = O.deliverable_population(net, succ)
    kw = dict(trips=True, link_bin_seconds=100)
    mode = VecEvaluator(O.engine_of(net, pop, 2), "embedding", emb=emb.cuda(), **kw)
    res = mode.run(300)
    base = VecEvaluator(O.engine_of(net, pop, 2), "dijkstra_hold", **kw).run(300, trip_pair=mode.eng.agents)
    assert not res.domain_exit and not base.domain_exit
    rep = paired_report(res, base)
    assert rep["available"] and rep["a"] == "embedding" and rep["b"] == "dijkstra_hold"
    assert rep["metrics"]["mean_travel_time"]["n"] >= 1 and rep["metrics"]["episode_return"]["n"] == 2
    trips = trip_report(res, baseline=base)
    p = trips["summary"]["paired"]
    n_both = int(base.trips["n_both"].sum())
    print(f"[hold, paired] arrivals policy {res.arrived} baseline {base.arrived}, trip pairs {n_both}, "
          f"travel-time pairs {rep['metrics']['mean_travel_time']['n']}")
    assert p["available"] and p["baseline_head"] == "dijkstra_hold" and p["pairs"] == n_both > 0


# ---- 6. reproducibility, refusals ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_sampled_mode_is_refused():
    net = _torus8()
    pop = _few_population(net)
    ev1, ev2 = (_router(net, pop, 4, keep_actions=True) for _ in range(2))
    r1, r2 = ev1.run(80), ev2.run(80)
    assert r1 == r2 and not r1.domain_exit and r1.settings == r2.settings
    assert torch.equal(ev1.eng.x, ev2.eng.x) and torch.equal(ev1.eng.agents, ev2.eng.agents)
    assert torch.equal(ev1.actions, ev2.actions) and torch.equal(ev1.reward[:80], ev2.reward[:80])
    static = _router(net, pop, 4, keep_actions=True, refresh_rate=0)
    r3 = static.run(80)
    assert r3.settings["refresh_rate"] == 0 and not torch.equal(static.actions, ev1.actions)
    with pytest.raises(ValueError, match="sampled"):
        ev1.run(8, deterministic=False)
    with pytest.raises(ValueError, match="refresh_rate"):
        _router(net, pop, 1, head="dijkstra", refresh_rate=0)


# ---- 7. CLI end to end --------------------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-1024"


@pytest.mark.parametrize("baseline,refresh", [("dijkstra_hold", 10), ("free_flow", 0)])
def test_cli_eval_baseline_end_to_end(tmp_path, capsys, baseline, refresh):
    main = importlib.import_module("main").main
    out = tmp_path / "ev"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", SCENARIO, "--eval-envs", "2", "--eval-baseline", baseline,
          "--steps", "40", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "=== Baseline (dijkstra_hold" in text and "(paired) ===" in text
    doc = json.load(open(out / "eval_envs.json"))
    assert doc["baseline"]["head"] == "dijkstra_hold" and doc["paired"]["b"] == "dijkstra_hold"
    assert doc["baseline"]["settings"]["refresh_rate"] == refresh and doc["baseline"]["settings"]["hold"] is True
    assert (out / "eval_envs.csv").exists()


def test_cli_dijkstra_router_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    out = tmp_path / "dj"
    main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
          "--dijkstra-envs", "2", "--dijkstra-router", "hold", "--steps", "40", "--start-end-time", "21540", "21660",
          "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "=== Vectorised evaluation (2 environments, dijkstra_hold) ===" in text
    doc = json.load(open(out / "dijkstra_envs.json"))
    assert doc["mode"]["head"] == "dijkstra_hold" and doc["mode"]["envs"] == 2
    assert (out / "dijkstra_envs.csv").exists()
