"""GPU: the vectorised shortest-path baseline on the packed path — tarl_fused_edge_travel_time and
tarl_fused_select_next_hop_dest against their unfused counterparts through tarl_fused_export, tarl_dest_trees_batched
against tarl_dest_trees slice by slice, ``VecEvaluator(head="dijkstra")`` replayed by the CPU oracle, its reproducibility,
the common random numbers the paired comparison rests on, the domain exit, and the CLI."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 3, 64)
SEL_RAW = 0x7F


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _pack(ops, plan, x, Nmax, ag, cc, edge_attr):
    fs = ops.FusedState(plan, x.size(0), ag.size(1), "cuda", Nmax)
    ops.fused_pack(plan, fs, x, Nmax, ag, cc, ec=ops.EdgeConst(edge_attr, "cuda"))
    fs.check_flags()
    return fs


def _export(ops, plan, fs, x, Nmax):
    """The packed state in the reference's layout: static columns from ``x``, dynamic ones from the export."""
    out = x.clone()
    out[:, :, :3 * Nmax] = -3.0
    out[:, :, 3 * Nmax + 1] = -3.0
    out[:, :, 3 * Nmax + 5] = -3.0
    ops.fused_export(plan, fs, out, Nmax, 100.0)
    return out


def _count_state(x0, K, Nmax, maxn):
    """(K, N, F): counts that cover 0 .. Nmax - 1 in every environment, shifted from one environment to the next, capped so
    that MAX + 10 - N stays positive; the FIFO columns hold ids for the occupied prefix."""
    N = x0.size(0)
    x = x0.unsqueeze(0).repeat(K, 1, 1).contiguous()
    for b in range(K):
        n = (torch.arange(N) * 7 + 3 * b) % Nmax
        n = torch.minimum(n, (maxn + 9).to(torch.int64)).clamp(min=0)
        x[b, :, 3 * Nmax + 1] = n.float()
        occ = torch.arange(Nmax).unsqueeze(0) < n.unsqueeze(1)
        x[b, :, :Nmax] = torch.where(occ, torch.ones(N, Nmax), torch.zeros(N, Nmax))
    return x


def _travel_time_case(ops, x0, ei, edge_attr, Nmax, cc, K):
    N = x0.size(0)
    plan = ops.Plan(ei, N)
    x = _count_state(x0, K, Nmax, x0[:, 3 * Nmax]).cuda()
    ag = torch.zeros((K, 2, 9), device="cuda")
    fs = _pack(ops, plan, x, Nmax, ag, cc.cuda(), edge_attr)
    got = ops.fused_edge_travel_time(plan, fs)
    want = ops.edge_travel_time(plan, _export(ops, plan, fs, x, Nmax), Nmax, cc.cuda())
    assert not bool(torch.isnan(want).any())
    assert torch.equal(got, want)
    return plan, x.cpu(), got


# ---- 1. travel times -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_fused_travel_times_equal_the_unfused_ones_on_the_export(K):
    """Crafted counts 0 .. Nmax - 1 in every environment, different from one environment to the next; a crafted congestion
    constant (a third of the nodes at 0.3 x) so that, among the occupied rows, the congested term sets the weight on some
    edges and the free-flow time on others."""
    from tarl_hip import ops
    net = _torus8()
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    cc = net.congestion_constant * torch.where(torch.arange(N) % 3 == 0, 0.3, 1.0)
    _, x, w = _travel_time_case(ops, net.x, ei, net.edge_attr, Nmax, cc, K)
    w = w.cpu()
    n = x[:, :, 3 * Nmax + 1]
    assert sorted(set(n[0].tolist())) == [float(v) for v in range(Nmax)]
    ff = x[0, ei[0], 3 * Nmax + 2]
    occupied = n[:, ei[0]] > 0
    assert bool(((w > ff) & occupied).any()) and bool(((w == ff) & occupied).any())
    if K > 1:
        assert not torch.equal(n[0], n[1]) and not torch.equal(w[0], w[1])


def test_fused_travel_times_on_a_matsim_grid_with_src_dest_nodes(tmp_path):
    from src.matsim_io import build_network
    from tarl_hip import ops, synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, Nmax = build_network(str(tmp_path / "network"))
    ei = graph.edge_index.cpu()
    assert ops.fused_path_supported(ei, Nmax)
    plan, _, w = _travel_time_case(ops, graph.x.cpu(), ei, graph.edge_attr.cpu(), Nmax, graph.congestion_constant.cpu(), 3)
    assert plan.num_groups < plan.num_nodes                      # DEST pseudo-nodes: no out-edges
    assert w.shape == (3, ei.size(1)) and not torch.equal(w[0], w[2])


# ---- 2. batched trees ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torus_weights():
    """(net, plan, weights (3, E) on the device) of the crafted state of test 1."""
    from tarl_hip import ops
    net = _torus8()
    cc = net.congestion_constant * torch.where(torch.arange(net.num_roads) % 3 == 0, 0.3, 1.0)
    plan, _, w = _travel_time_case(ops, net.x, net.edge_index, net.edge_attr, net.Nmax, cc, 3)
    return net, plan, w


@pytest.mark.parametrize("D", [1, 5, 256])
def test_batched_trees_equal_the_single_trees_slice_by_slice(torus_weights, D):
    from tarl_hip import ops
    from tree_restatement import check_table
    net, plan, w = torus_weights
    N = net.num_roads
    dests = (torch.arange(N) if D == N else torch.tensor([17, 0, 255, 101, 64][:D])).to(torch.int64).cuda()
    nh = ops.destination_trees_batched(plan, w, dests)
    assert nh.shape == (3, D, N) and nh.dtype == torch.int32
    for b in range(3):
        want, dist = ops.destination_trees(plan, w[b].contiguous(), dests, want_dist=True)
        assert torch.equal(nh[b], want), f"slice {b}"
        if b == 0:
            check_table(net.edge_index, w[0].cpu(), N, dests.cpu(), dist, nh[0], walks=2 if D < N else 0)
    assert not torch.equal(nh[0], nh[1]) or D == 1
    # one shared weight set: B equal slices
    shared = ops.destination_trees_batched(plan, w[1].contiguous(), dests, B=3)
    for b in range(3):
        assert torch.equal(shared[b], nh[1]), f"shared slice {b}"


def test_batched_trees_leave_the_rows_of_an_out_of_range_destination(torus_weights):
    from tarl_hip import ops
    net, plan, w = torus_weights
    N = net.num_roads
    dests = torch.tensor([3, -1, N, N + 1000, 17], dtype=torch.int64, device="cuda")
    out = torch.full((3, 5, N), -9, dtype=torch.int32, device="cuda")
    ops.destination_trees_batched(plan, w, dests, out=out)
    ok = ops.destination_trees_batched(plan, w, dests[[0, 4]].contiguous())
    assert bool((out[:, 1:4] == -9).all()) and torch.equal(out[:, [0, 4]], ok)


def test_batched_trees_on_the_25x25_torus():
    """N = 2 500: 79-word bitmaps; two weight sets, eight destinations."""
    from tarl_hip import ops, synth
    net = synth.torus_network(25, 25, heterogeneous=True, seed=1)
    N, ei = net.num_roads, net.edge_index
    plan = ops.Plan(ei, N)
    w = torch.stack([ops.edge_travel_time(plan, synth.random_state(net, seed=s, fill=0.9).cuda(), net.Nmax,
                                          net.congestion_constant.cuda())[0] for s in (7, 8)])
    dests = torch.tensor([0, 2499, 1250, 77, 1303, 640, 2048, 999], dtype=torch.int64, device="cuda")
    nh = ops.destination_trees_batched(plan, w, dests)
    for b in range(2):
        assert torch.equal(nh[b], ops.destination_trees(plan, w[b].contiguous(), dests)[0]), f"slice {b}"
    assert not torch.equal(nh[0], nh[1])


# ---- 3. the select kernel --------------------------------------------------------------------------------------------------
def _select_both_ways(ops, plan, fs, x, Nmax, ag, dest_slot, table):
    """-> (SELECTED_ROAD column the unfused kernel writes into the export with environment b's table, the exported column
    after the fused kernel, the choice8 bytes). Everything but that column must be left as it was."""
    K = x.size(0)
    before = _export(ops, plan, fs, x, Nmax)
    want = before.clone()
    for b in range(K):
        ops.select_next_hop_dest(want[b], Nmax, ag[b], dest_slot, table[b])
    c8 = torch.full((K, plan.num_nodes), 0x55, dtype=torch.uint8, device="cuda")
    ops.fused_select_next_hop_dest(plan, fs, dest_slot, table, choice8=c8)
    got = _export(ops, plan, fs, x, Nmax)
    col = 3 * Nmax + 5
    assert torch.equal(got[:, :, col], want[:, :, col])
    assert torch.equal(got, want)
    assert torch.equal(c8, fs.sel8.t().contiguous())
    return before[:, :, col], got[:, :, col], c8


@pytest.mark.parametrize("K", KS)
def test_fused_select_on_a_rollout_state(K):
    """40 frames into a sampled rollout of the embedding head (heads, empty rows, mixed destinations), a table per
    environment from that environment's own travel times, every node a destination except a few without a tree."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START, SimEngine
    net = _torus8()
    N, Nmax = net.num_roads, net.Nmax
    pops = synth.population_batch(400, N, K, seed=21, device="cuda", t1=EPISODE_START + 40)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(K, 1, 1).contiguous(), net.edge_index, net.edge_attr, Nmax, pops,
                    congestion_constant=net.congestion_constant, seed=11)
    eng.reset()
    eng.prepare_policy(torch.randn(N, generator=torch.Generator().manual_seed(0)).cuda(), 1.0)
    for _ in range(40):
        eng.frame_fused()
    eng.check_flags()
    plan, fs = eng.plan, eng.fs
    table = ops.destination_trees_batched(plan, ops.fused_edge_travel_time(plan, fs),
                                          torch.arange(N, dtype=torch.int64, device="cuda"))
    slot = torch.arange(N, dtype=torch.int32)
    slot[[9, 130, 200]] = -1
    x = eng.x.clone()
    n = x[:, :, 3 * Nmax + 1]
    assert bool((n == 0).any()) and bool((n > 0).any())
    before, after, c8 = _select_both_ways(ops, plan, fs, x, Nmax, eng.agents, slot.cuda(), table)
    assert not torch.equal(before, after)
    assert bool((c8 < 4).any())
    if K > 1:
        assert not torch.equal(table[0], table[1])


def test_fused_select_on_crafted_rows():
    """A packed random state (stale dead slots: DIRTY rows, empty rows whose slot 0 holds an old id) with, per environment:
    a head at its destination (the value is the row itself: raw), table entries of -1 and of a node that is no successor
    (raw), destinations without a tree and out of range, head ids at and above A (those rows keep their selection)."""
    from tarl_hip import ops, synth
    net = _torus8()
    N, Nmax, ei, K, A = net.num_roads, net.Nmax, net.edge_index, 3, 60
    plan = ops.Plan(ei, N)
    gen = torch.Generator().manual_seed(5)
    xs, ags = [], []
    for b in range(K):
        x = synth.random_state(net, seed=40 + b)
        x[:, 0] = torch.where(x[:, 3 * Nmax + 1] > 0, torch.randint(1, A, (N,), generator=gen).float(), x[:, 0])
        ag = synth.population(A - 1, N, seed=40 + b)
        ag[3, 1], ag[4, 1], ag[5, 1] = -1.0, float(N + 3), 2.5
        x[10:20, 3 * Nmax + 1] = x[10:20, 3 * Nmax + 1].clamp(min=1)
        x[10, 0], ag[7, 1] = 7.0, 10.0                               # the head of row 10 is bound for row 10
        x[11, 0], x[12, 0], x[13, 0] = 3.0, 4.0, 5.0                 # destinations -1, N + 3, 2.5 (-> 2)
        x[14, 0], x[15, 0] = float(A), float(A + 40)                 # head ids out of range
        x[16, 0], ag[8, 1] = 8.0, 77.0                               # destination 77: no tree (slot -1)
        x[17, 0], ag[9, 1] = 9.0, 78.0                               # destination 78: table entry -1 at row 17
        x[18, 0], ag[11, 1] = 11.0, 79.0                             # destination 79: a foreign entry at row 18
        xs.append(x)
        ags.append(ag)
    x, ag = torch.stack(xs).cuda(), torch.stack(ags).cuda()
    fs = _pack(ops, plan, x, Nmax, ag, net.congestion_constant.cuda(), net.edge_attr)
    dirty_empty = ((fs.hdp[..., 0] & 0xFF) == 0x80) & (x[:, :, 0].t() != 0)
    assert bool(dirty_empty.any()), "no empty row with a stale slot 0"
    table = ops.destination_trees_batched(plan, ops.fused_edge_travel_time(plan, fs),
                                          torch.arange(N, dtype=torch.int64, device="cuda"))
    slot = torch.arange(N, dtype=torch.int32)
    slot[77] = -1
    table[:, 78, 17] = -1
    foreign = int(next(v for v in range(N) if v != 18 and v not in ei[1][ei[0] == 18].tolist()))
    table[:, 79, 18] = foreign
    before, after, c8 = _select_both_ways(ops, plan, fs, x, Nmax, ag, slot.cuda(), table)
    before, after, c8 = before.cpu(), after.cpu(), c8.cpu()
    for b in range(K):
        assert after[b, 10] == 10.0 and c8[b, 10] == SEL_RAW
        assert after[b, 17] == -1.0 and c8[b, 17] == SEL_RAW
        assert after[b, 18] == float(foreign) and c8[b, 18] == SEL_RAW
        for row in (11, 12, 14, 15, 16):
            assert after[b, row] == before[b, row], (b, row)
        assert after[b, 13] == float(table[b, 2, 13])                # 2.5 truncates to destination 2


def test_fused_select_beyond_four_out_edges():
    """A node of out-degree 70 (ranks beyond NodeRec.out4, up to 69) and one of out-degree 9, edges in shuffled order."""
    from tarl_hip import ops
    gen = torch.Generator().manual_seed(3)
    N, Nmax, K, A = 96, 6, 3, 12
    deg = torch.randint(1, 5, (N,), generator=gen)
    deg[3], deg[40] = 70, 9
    src = torch.repeat_interleave(torch.arange(N), deg)
    dst = torch.cat([torch.randperm(N, generator=gen)[:int(d)] for d in deg])
    perm = torch.randperm(src.numel(), generator=gen)
    ei = torch.stack([src[perm], dst[perm]])
    assert ops.fused_path_supported(ei, Nmax)
    plan = ops.Plan(ei, N)
    assert plan.max_out == 70 and not plan.src_sorted
    F = 3 * Nmax + 7
    x = torch.zeros((K, N, F))
    x[:, :, 3 * Nmax + 0], x[:, :, 3 * Nmax + 2], x[:, :, 3 * Nmax + 3], x[:, :, 3 * Nmax + 4] = 5.0, 10.0, 100.0, 10.0
    x[:, :, 3 * Nmax + 6] = torch.arange(N).float()
    x[:, :, 3 * Nmax + 1] = torch.randint(0, 4, (K, N), generator=gen).float()
    x[:, [3, 40], 3 * Nmax + 1] = 2.0
    x[:, :, 0] = torch.where(x[:, :, 3 * Nmax + 1] > 0, torch.randint(1, A, (K, N), generator=gen).float(), torch.zeros(K, N))
    ag = torch.zeros((K, A, 9))
    ag[:, :, 1] = torch.randint(0, N, (K, A), generator=gen).float()
    x, ag = x.cuda(), ag.cuda()
    fs = _pack(ops, plan, x, Nmax, ag, None, torch.full((ei.size(1), 1), 0.25))
    w = (torch.rand((K, ei.size(1)), generator=gen) * 20 + 1).cuda()
    table = ops.destination_trees_batched(plan, w, torch.arange(N, dtype=torch.int64, device="cuda"))
    # the plan's CSR order of node 3's out-edges is the stable order of the edge list: force the ranks 65, 66, 67
    succ3 = ei[1][ei[0] == 3]
    for b in range(K):
        d = int(ag[b, int(x[b, 3, 0]), 1])
        table[b, d, 3] = int(succ3[65 + b])
    slot = torch.arange(N, dtype=torch.int32, device="cuda")
    _, after, c8 = _select_both_ways(ops, plan, fs, x, Nmax, ag, slot, table)
    c8 = c8.cpu()
    assert [int(c8[b, 3]) for b in range(K)] == [65, 66, 67]
    assert [float(after[b, 3]) for b in range(K)] == [float(succ3[65 + b]) for b in range(K)]
    assert bool((c8[:, 40] < 9).all())


# ---- 4. replay by the oracle -----------------------------------------------------------------------------------------------
LOAD = dict(agents=500, span=120, dests=[5, 77, 130, 201, 254, 31, 166, 98])


def _baseline_evaluator(net, pop, K, seed=3, env_base=0, **kw):
    from tarl_hip.engine import SimEngine
    from tarl_hip.evaluator import VecEvaluator
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                    congestion_constant=net.congestion_constant, num_envs=K, seed=seed, env_base=env_base)
    return VecEvaluator(eng, "dijkstra", **kw)


def _load_population(net):
    import baseline_restatement as BR
    from tarl_hip.engine import EPISODE_START
    return BR.few_destination_population(LOAD["agents"], net.num_roads, LOAD["dests"], seed=7, t0=EPISODE_START,
                                         t1=EPISODE_START + LOAD["span"])


def _assert_replayed_by_the_oracle(net, pop, K, T, succ):
    """``VecEvaluator(head="dijkstra")`` on K environments for T frames against baseline_restatement.replay, environment by
    environment: SELECTED_ROAD on every node at every frame (``succ`` (N, max out-degree): every node's successors in the
    plan's out-list order, padded with a value no road has; a raw byte: the oracle's value is no successor of the node),
    every reward, the final state and agent table, and the EvalResult against eval_restatement. -> (res, the replays)."""
    import baseline_restatement as BR
    import eval_restatement as R
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    ev = _baseline_evaluator(net, pop, K, keep_actions=True)
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T and res.head == "dijkstra" and res.deterministic
    dests = {int(d) for d in pop[:, 1].tolist()}
    assert res.settings["refresh_rate"] == 10 and res.settings["destinations"] == len(dests)
    rw = ev.reward[:T].cpu()
    actions = ev.actions[:T].cpu().long()
    ff = net.x[:, 3 * Nmax + 2][ei[0]]
    succ = succ.float()
    runs = []
    for b in range(K):
        r = BR.replay(net, pop, T, 10, lambda t: ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu(),
                      EPISODE_START)
        assert r["max_count"] < Nmax
        for t in range(T):
            code = actions[t, b]
            ranked = code < SEL_RAW
            value = succ[torch.arange(N), code.clamp(max=succ.size(1) - 1)]
            assert torch.equal(value[ranked], r["sel"][t][ranked]), f"SELECTED_ROAD of environment {b}, frame {t}"
            assert not bool((succ[~ranked] == r["sel"][t][~ranked].unsqueeze(1)).any()), f"raw bytes, environment {b}, frame {t}"
            assert rw[t, b] == r["reward"][t], f"reward of environment {b}, frame {t}"
        assert torch.equal(r["x"], eng.x[b].cpu()), f"final state of environment {b}"
        assert torch.equal(r["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        print(f"[baseline replay] environment {b}: largest count {r['max_count']:.0f} of {Nmax}, "
              f"{int(r['agents'][1:, 8].sum())} arrivals, edges off free flow per refresh "
              f"{[int((w != ff).sum()) for w in r['weights']]}")
        runs.append(r)
    want = R.per_env(R.summary(torch.stack([r["agents"] for r in runs]).numpy(),
                               np.asarray([r["reward"] for r in runs], dtype=np.float32).T, 10.0, 720), 10.0)
    for b, w in enumerate(want):
        got = dict(arrived=res.arrived[b], on_way=res.on_way[b], not_departed=res.not_departed[b],
                   episode_return=res.episode_return[b], avg=res.avg_travel_time[b], std=res.std_travel_time[b],
                   max=res.max_travel_time[b], p50=res.p50_travel_time[b], p95=res.p95_travel_time[b])
        assert got == w, (b, got, w)
    return res, runs, actions


def test_baseline_evaluation_replayed_by_the_oracle():
    """3 environments, 120 frames, 500 agents that leave within 120 s for one of eight roads (chosen on the CPU oracle under
    torch's own noise: largest count 11 of 15 in every environment, 100 - 500 edges off free flow at every refresh after the
    first, the tables of two environments apart from the sixth refresh on; on the device's noise streams, engine seed 3: largest
    count 11 in all three, 165 - 168 arrivals; the test prints them). Per environment the oracle rebuilds its table
    every 10 frames from ITS OWN state (oracle.routing.edge_travel_time, the reverse trees and tie rule of
    tree_restatement), selects with oracle.routing.dijkstra_choice and steps with oracle.sim.env_step under the Gumbel
    values the kernels consumed. Device SELECTED_ROAD == the oracle's on every node at every frame (a raw byte: the oracle's
    value is no successor of the node; the final export compares those values too), every reward, the final state and
    agent table, and the EvalResult against eval_restatement: exact."""
    net = _torus8()
    N, Nmax, ei, K, T = net.num_roads, net.Nmax, net.edge_index, 3, 120
    pop = _load_population(net)
    res, runs, _ = _assert_replayed_by_the_oracle(net, pop, K, T, ei[1].view(N, 4))      # source-sorted: the out-lists
    ff = net.x[:, 3 * Nmax + 2][ei[0]]
    # not vacuous: congestion moves the weights, and the environments route on different tables
    assert any(bool((w != ff).any()) for w in runs[0]["weights"][1:])
    assert any(not torch.equal(runs[0]["tables"][k], runs[b]["tables"][k]) for k in range(T // 10) for b in (1, 2))
    assert min(res.arrived) >= 5


IRREGULAR_LOAD = dict(agents=600, span=30, frames=40, dests=[5, 17, 33, 48, 61, 12, 13, 70])


def test_baseline_evaluation_replayed_by_the_oracle_on_an_irregular_graph():
    """The same replay on MIXED (tests/irregular_graphs.py: 80 roads, out-degrees 0 - 9, an edge list in no order, two dead
    ends, two roads nobody can enter), 3 environments, 40 frames, 600 agents that leave within 30 s for six ordinary roads,
    the road with nine out-edges or a dead end. Nobody starts on a dead end: the environment inserts an agent into the
    SELECTED_ROAD of its origin, and a road that leads nowhere selects -1 (outside the reference's domain). On the CPU
    oracle under torch's own noise: largest count 23 - 25 of 41, 37 - 40 arrivals, 190 - 250 edges off free flow at every
    refresh, the table rebuilt differently at every refresh, 640 - 680 selections of out-rank >= 4 and about 140 raw ones
    (the other dead end and the rows already at their destination); the test prints what the device's noise gives."""
    import baseline_restatement as BR
    import irregular_graphs as ig
    import sp_cases as S
    from tarl_hip.engine import EPISODE_START
    c = S.case("MIXED")
    net, N, K, T = c.net, c.N, 3, IRREGULAR_LOAD["frames"]
    _, dout = ig.degrees(net)
    leads_on = torch.nonzero(dout > 0).view(-1)
    dests = IRREGULAR_LOAD["dests"]
    assert int(dout[12]) == 9 and int(dout[13]) == 0 and all(int(dout[d]) > 0 for d in dests if d != 13)
    pop = BR.few_destination_population(IRREGULAR_LOAD["agents"], N, dests, seed=7, t0=EPISODE_START,
                                        t1=EPISODE_START + IRREGULAR_LOAD["span"])
    pop[:, 0] = leads_on[pop[:, 0].long() % leads_on.numel()].float()
    res, runs, actions = _assert_replayed_by_the_oracle(net, pop, K, T, S.out_table(c))
    ff = net.x[:, 3 * net.Nmax + 2][c.ei[0]]
    beyond = int(((actions >= 4) & (actions < SEL_RAW)).sum())
    print(f"[baseline replay] MIXED: {beyond} selections of out-rank >= 4, {int((actions == SEL_RAW).sum())} raw, "
          f"arrivals {res.arrived}")
    assert beyond > 0 and bool((actions == SEL_RAW).any())
    assert any(bool((w != ff).any()) for w in runs[0]["weights"][1:])
    assert any(not torch.equal(runs[0]["weights"][k], runs[b]["weights"][k]) for k in range(1, T // 10) for b in (1, 2))
    assert min(res.arrived) >= 5


# ---- 5. reproducibility and independence -----------------------------------------------------------------------------------
def test_baseline_is_reproducible_env_b_is_the_solo_engine_b_and_the_refresh_is_live():
    net = _torus8()
    pop = _load_population(net)
    T = 100
    ev1, ev2 = (_baseline_evaluator(net, pop, 8, keep_actions=True) for _ in range(2))
    r1, r2 = ev1.run(T), ev2.run(T)
    assert r1 == r2 and not r1.domain_exit
    assert torch.equal(ev1.eng.x, ev2.eng.x) and torch.equal(ev1.eng.agents, ev2.eng.agents)
    assert torch.equal(ev1.actions, ev2.actions)
    for b in (0, 5):
        solo = _baseline_evaluator(net, pop, 1, env_base=b)
        rs = solo.run(T)
        assert torch.equal(solo.eng.x[0], ev1.eng.x[b]) and torch.equal(solo.eng.agents[0], ev1.eng.agents[b]), b
        assert rs.episode_return[0] == r1.episode_return[b] and rs.arrived[0] == r1.arrived[b]
    # a table rebuilt every frame follows the congestion more closely: other actions on the loaded case
    ev3 = _baseline_evaluator(net, pop, 8, keep_actions=True, refresh_rate=1)
    r3 = ev3.run(T)
    assert not r3.domain_exit and r3.settings["refresh_rate"] == 1
    assert not torch.equal(ev3.actions, ev1.actions)
    with pytest.raises(ValueError, match="sampled"):
        ev1.run(8, deterministic=False)


# ---- 6. common random numbers ----------------------------------------------------------------------------------------------
def test_policy_and_baseline_share_their_noise_and_the_paired_report_equals_numpy():
    from tarl_hip import ops
    from tarl_hip.engine import SimEngine
    from tarl_hip.evaluator import PAIRED_METRICS, VecEvaluator, paired_report
    from oracle import dist, nets
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    N, K, T = net.num_roads, 8, 300
    # 128 agents, every other one bound for the road three MODE steps from its origin: the population under which the MODE of
    # this embedding stays inside the domain and delivers somebody (tests/test_gpu_eval.py)
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    action = dist.GraphDist(nets.policy_logits(net.x[:, 3 * net.Nmax:], net.edge_index, emb), net.edge_index).mode.long()
    chosen = action.nonzero().view(-1)
    succ = torch.empty(N, dtype=torch.long)
    succ[net.edge_index[0, chosen]] = net.edge_index[1, chosen]
    pop = synth.population(128, N, seed=7, t1=EPISODE_START + 200)
    pop[1::2, 1] = succ[succ[succ[pop[1::2, 0].long()]]].float()
    base = _baseline_evaluator(net, pop, K, seed=9)
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                    congestion_constant=net.congestion_constant, num_envs=K, seed=9)
    pol = VecEvaluator(eng, "embedding", emb=emb.cuda())
    c0 = (pol.eng.noise_counter, base.eng.noise_counter)
    assert c0[0] == c0[1] and pol.eng.seed == base.eng.seed and pol.eng.fs.env_base == base.eng.fs.env_base
    rp, rb = pol.run(T), base.run(T)
    assert not rp.domain_exit and not rb.domain_exit
    assert pol.eng.noise_counter == base.eng.noise_counter == c0[0] + T
    envs = list(range(K))
    for t in (0, 1, 57, T - 1):         # the same (seed, frame counter, environment) on both engines: the same values
        a = ops.noise_export(pol.eng.plan, "gumbel", pol.eng.seed, c0[0] + 1 + t, envs)
        b = ops.noise_export(base.eng.plan, "gumbel", base.eng.seed, c0[1] + 1 + t, envs)
        assert torch.equal(a, b) and not torch.equal(a[0], a[1])
    rep = paired_report(rp, rb)
    assert rep["available"] and rep["envs"] == K and rep["a"] == "embedding" and rep["b"] == "dijkstra"
    for name, key in PAIRED_METRICS:
        pairs = [(x, y) for x, y in zip(getattr(rp, key), getattr(rb, key)) if x is not None and y is not None]
        d = np.asarray([x - y for x, y in pairs], dtype=np.float64)
        m = rep["metrics"][name]
        assert m["n"] == d.size and m["dropped"] == K - d.size
        if d.size < 2:      # (under this population the router strands its agents on their destination roads: no arrival)
            assert m["std"] is None and m["se"] is None and m["ci95"] is None
            assert m["mean"] == (float(d[0]) if d.size else None)
        else:
            se = d.std(ddof=1) / math.sqrt(d.size)
            assert m["mean"] == d.mean() and m["std"] == d.std(ddof=1) and m["se"] == se
            assert m["ci95"] == (d.mean() - 1.96 * se, d.mean() + 1.96 * se)
    assert rep["metrics"]["episode_return"]["n"] == K and rep["frames_run"] == T
    print(f"[paired] arrivals policy {rp.arrived} baseline {rb.arrived}; return difference {rep['metrics']['episode_return']}")


# ---- 7. domain exit --------------------------------------------------------------------------------------------------------
def test_baseline_on_the_collapse_case():
    """1 024 agents leaving within 120 s (the load under which the MODE of the embedding head leaves the domain,
    tests/test_gpu_eval.py). Whichever way the router fares: a domain exit has no statistics and no paired report."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START, SimEngine
    from tarl_hip.evaluator import VecEvaluator, paired_report
    net = _torus8()
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    base = _baseline_evaluator(net, pop, 2)
    rb = base.run(256)
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                    congestion_constant=net.congestion_constant, num_envs=2, seed=3)
    rp = VecEvaluator(eng, "embedding", emb=torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0)).cuda()).run(256)
    print(f"[collapse] baseline domain_exit={rb.domain_exit} frames_run={rb.frames_run}; policy domain_exit={rp.domain_exit}")
    assert rp.domain_exit                    # (tests/test_gpu_eval.py: the MODE of this embedding leaves the domain here)
    if rb.domain_exit:
        assert rb.aggregate is None and rb.episode_return is None and rb.rows() == []
        assert "domain exit" in rb.summary_lines()[0]
    else:
        assert rb.frames_run == 256
    rep = paired_report(rp, rb)
    assert rep["available"] is False and "metrics" not in rep and "domain exit" in rep["reason"]


# ---- 8. CLI end to end -----------------------------------------------------------------------------------------------------
def test_cli_baseline_flags_end_to_end(tmp_path, capsys):
    import csv
    from tarl_hip.evaluator import PER_ENV_KEYS
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-1024"
    run = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", scenario, "--rollout-steps", "32", "--iterations", "2",
          "--eval-envs", "4", "--eval-baseline", "dijkstra", "--steps", "5", "--output-dir", str(run)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert len(logs) == 2
    for rec in logs:
        assert rec["eval_vec/envs"] == 4 and rec["eval_vec_baseline/envs"] == 4
        for k in ("avg_return", "avg_return_se", "arrived", "domain_exit", "computation_time_ms"):
            assert f"eval_vec_baseline/{k}" in rec, k
        assert rec["eval_vec_paired/available"] in (0, 1)
        if rec["eval_vec_paired/available"]:
            assert rec["eval_vec_paired/episode_return/n"] == 4
            assert math.isfinite(rec["eval_vec_paired/episode_return/mean"]) and math.isfinite(rec["eval_vec_paired/episode_return/se"])
        assert "eval/avg_return" in rec
    # the router is a function of the seed only: evaluated once, the same numbers in every record
    assert logs[0]["eval_vec_baseline/avg_return"] == logs[1]["eval_vec_baseline/avg_return"]
    assert logs[0]["eval_vec_baseline/computation_time_ms"] == logs[1]["eval_vec_baseline/computation_time_ms"]
    # (--mode train ends with the eval report: 5 frames here)
    doc = json.load(open(run / "eval_envs.json"))
    assert set(doc) == {"mode", "baseline", "paired"}
    capsys.readouterr()
    # evaluation from the checkpoint, with the same flags
    ev_dir = tmp_path / "ev"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--checkpoint", str(run / "policy.pt"), "--eval-envs", "4",
          "--eval-baseline", "dijkstra", "--steps", "120", "--output-dir", str(ev_dir)])
    text = capsys.readouterr().out
    i0 = text.index("=== Vectorised evaluation (4 environments, MODE) ===")
    i1 = text.index("=== Baseline (dijkstra) ===")
    i2 = text.index("=== Policy − baseline (paired) ===")
    assert i0 < i1 < i2
    doc = json.load(open(ev_dir / "eval_envs.json"))
    assert doc["baseline"]["head"] == "dijkstra" and doc["baseline"]["envs"] == 4 and doc["baseline"]["frames_run"] == 120
    assert doc["baseline"]["settings"]["seed"] == doc["mode"]["settings"]["seed"]
    assert doc["paired"]["a"] == doc["mode"]["head"] and doc["paired"]["b"] == "dijkstra"
    if doc["paired"]["available"]:
        assert doc["paired"]["metrics"]["episode_return"]["n"] == 4
    rows = list(csv.DictReader(open(ev_dir / "eval_envs.csv")))
    assert len(rows) == 4 and all(f"baseline_{k}" in rows[0] for k in PER_ENV_KEYS)
    if not doc["baseline"]["domain_exit"]:
        assert all(r["baseline_episode_return"] != "" for r in rows)
    # the router on its own: --dijkstra-envs
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", scenario,
          "--dijkstra-envs", "4", "--steps", "120", "--start-end-time", "21540", "21660", "--output-dir", str(dj)])
    text = capsys.readouterr().out
    assert "=== Vectorised evaluation (4 environments, dijkstra) ===" in text
    doc = json.load(open(dj / "dijkstra_envs.json"))
    assert doc["mode"]["head"] == "dijkstra" and doc["mode"]["envs"] == 4 and doc["mode"]["frames_run"] == 120
    rows = list(csv.DictReader(open(dj / "dijkstra_envs.csv")))
    assert len(rows) == (0 if doc["mode"]["domain_exit"] else 4)
    # without the new flags: exactly today's keys and columns
    plain = tmp_path / "plain"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--checkpoint", str(run / "policy.pt"), "--eval-envs", "4",
          "--steps", "40", "--output-dir", str(plain)])
    text = capsys.readouterr().out
    assert "Baseline" not in text and "paired" not in text
    assert set(json.load(open(plain / "eval_envs.json"))) == {"mode"}
    assert list(csv.DictReader(open(plain / "eval_envs.csv")).fieldnames) == ["kind", "env"] + list(PER_ENV_KEYS)
    assert not (plain / "dijkstra_envs.json").exists()
