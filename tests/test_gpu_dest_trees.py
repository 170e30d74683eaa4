"""GPU: per-destination shortest-path trees (csrc/dest_trees.hip: tarl_dest_trees, tarl_select_next_hop_dest) and
``DijkstraAgents(method="per_destination")``. The CPU side is tree_restatement.py's: a heapq Dijkstra on the REVERSE
graph that accumulates fp64 in the kernel's order (w(u,v) + dist[v]), and the documented tie rule of the next hops (fewest
hops to the destination over tight edges, then the smallest successor id)."""
import os
import sys

import pytest
import torch

from conftest import PKG
from tree_restatement import adjacency, check_table, cpu_dijkstra, cpu_tie_rule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def _check_vs_cpu(ops, plan, ei, w, N, dests, cpu_dests=None, walks=4):
    nh, dist = ops.destination_trees(plan, w.cuda(), dests.cuda(), want_dist=True)
    rev = adjacency(ei, w, N, reverse=True)
    for j, d in enumerate(dests.tolist()):
        if cpu_dests is not None and d not in cpu_dests:
            continue
        dc, _ = cpu_dijkstra(rev, N, d, reverse=True)
        assert torch.equal(dist[j].cpu(), torch.tensor(dc, dtype=torch.float64)), f"distances to {d}"
        want = cpu_tie_rule(rev, dc, N, d, reverse=True)
        want[d] = d                                            # the destination holds itself, unreached nodes -1
        assert torch.equal(nh[j].cpu(), torch.tensor(want, dtype=torch.int32)), f"tie rule towards {d}"
    check_table(ei, w, N, dests, dist, nh, walks=walks)
    for _ in range(2):                                         # launch after launch: bit for bit
        nh2, d2 = ops.destination_trees(plan, w.cuda(), dests.cuda(), want_dist=True)
        assert torch.equal(nh2, nh) and torch.equal(d2, dist)
    _, d3 = ops.destination_trees(plan, w.cuda(), dests.cuda(), want_next_hop=False, want_dist=True)
    nh3, _ = ops.destination_trees(plan, w.cuda(), dests.cuda())
    assert torch.equal(d3, dist) and torch.equal(nh3, nh)
    return nh, dist


def _travel_times(ops, plan, x, Nmax, cc):
    """The weights DijkstraAgents routes on: tarl_edge_travel_time of the state (fp32, original edge order)."""
    return ops.edge_travel_time(plan, x.cuda(), Nmax, cc.cuda())[0].cpu()


# ---- 1. trees against the CPU restatement ---------------------------------------------------------------------------------
def test_trees_heterogeneous_torus(ops):
    from tarl_hip import synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    x = synth.random_state(net, seed=2)
    w = _travel_times(ops, plan, x, net.Nmax, net.congestion_constant)
    _check_vs_cpu(ops, plan, ei, w, N, torch.arange(N, dtype=torch.int64))


def test_trees_homogeneous_torus_tie_rule(ops):
    """Nearly every pair is tied on a homogeneous torus at free flow: the next hops must follow the CPU tie rule."""
    from tarl_hip import synth
    net = synth.torus_network(12, 9)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    w = _travel_times(ops, plan, net.x, net.Nmax, net.congestion_constant)
    assert bool((w == w[0]).all())
    dests = torch.cat([torch.arange(0, N, 5), torch.tensor([N - 1])]).to(torch.int64)
    _check_vs_cpu(ops, plan, ei, w, N, dests)


def test_trees_matsim_grid_src_dest(ops, tmp_path):
    """SRC / DEST pseudo-nodes: destinations nothing reaches, nodes that reach nothing (+inf, -1)."""
    from src.matsim_io import build_network
    from tarl_hip import synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, Nmax = build_network(str(tmp_path / "network"))
    ei, N = graph.edge_index.cpu(), graph.x.size(0)
    plan = ops.Plan(ei, N)
    w = _travel_times(ops, plan, graph.x, Nmax, graph.congestion_constant)
    nh, dist = _check_vs_cpu(ops, plan, ei, w, N, torch.arange(N, dtype=torch.int64))
    assert bool(torch.isinf(dist).any()) and int((nh == -1).sum()) > N


def test_trees_config4_congested(ops):
    """BASELINE config 4's graph (25 x 25 torus, N = 2 500) under a congested state: every destination's tree checked
    for tightness and reachability, a sample against the CPU restatement."""
    from tarl_hip import synth
    net = synth.torus_network(25, 25, heterogeneous=True, seed=1)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    x = synth.random_state(net, seed=7, fill=0.9)
    w = _travel_times(ops, plan, x, net.Nmax, net.congestion_constant)
    ff = x[:, 3 * net.Nmax + 2][ei[0]]
    assert float((w > ff).float().mean()) > 0.05                         # the congestion term sets part of the weights
    sample = set(torch.randperm(N, generator=torch.Generator().manual_seed(5))[:24].tolist())
    _check_vs_cpu(ops, plan, ei, w, N, torch.arange(N, dtype=torch.int64), cpu_dests=sample, walks=1)


def test_out_of_range_destination_leaves_its_row(ops):
    from tarl_hip import lib, synth
    L = lib.load()
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    w = _travel_times(ops, plan, net.x, net.Nmax, net.congestion_constant).cuda()
    dests = torch.tensor([3, -1, N, N + 1000, 17], dtype=torch.int64, device="cuda")
    D = dests.numel()
    dist = torch.full((D, N), -7.5, dtype=torch.float64, device="cuda")
    nh = torch.full((D, N), -9, dtype=torch.int32, device="cuda")
    need = int(L.tarl_dest_trees_scratch_bytes(plan.handle, D))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    lib.check(L.tarl_dest_trees(plan.handle, w.data_ptr(), dests.data_ptr(), D, scratch.data_ptr(), need, nh.data_ptr(),
                                dist.data_ptr(), lib.current_stream()))
    torch.cuda.synchronize()
    for j in (1, 2, 3):
        assert bool((dist[j] == -7.5).all()) and bool((nh[j] == -9).all()), f"row {j} was written"
    nh_ok, d_ok = ops.destination_trees(plan, w, dests[[0, 4]].contiguous(), want_dist=True)
    assert torch.equal(dist[[0, 4]], d_ok) and torch.equal(nh[[0, 4]], nh_ok)


# ---- 2. agreement with the all-pairs table on tie-free weights -------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(6, 5), (25, 25)])
def test_matches_all_pairs_tie_free(ops, W, H):
    """Random fp32 weights in [1, 21): the exactness condition holds (exponent span + log2 hops << 28), so the columns of
    tarl_apsp's tables equal the per-destination rows: the distances everywhere, the next hops wherever the first hop
    is not tied."""
    from tarl_hip import synth
    net = synth.torus_network(W, H, heterogeneous=True, seed=9)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    w = (torch.rand(ei.size(1), generator=torch.Generator().manual_seed(W * H)) * 20 + 1).cuda()
    nh_ap, d_ap = ops.all_pairs_shortest_paths(plan, w, want_dist=True)
    nh, dist = ops.destination_trees(plan, w, torch.arange(N, dtype=torch.int64, device="cuda"), want_dist=True)
    assert bool((nh_ap >= 0).all())
    assert torch.equal(dist.t().to(torch.float32), d_ap[0]), "distances"
    # an exact tie of two first hops (two tight out-edges of u towards d) is left to either rule; with random 24-bit
    # significands it is rare, and it is counted rather than assumed away
    src, dst = ei[0].cuda(), ei[1].cuda()
    tight = (w.to(torch.float64)[None, :] + dist[:, dst]) == dist[:, src]             # [d][e]
    ntight = torch.zeros((N, N), dtype=torch.int32, device="cuda").index_add_(1, src, tight.to(torch.int32))
    untied = (ntight <= 1).t()                                                        # [u][d]
    assert int((~untied).sum()) <= N * N // 100_000
    assert torch.equal(nh.t().to(torch.int64)[untied], nh_ap[0][untied]), "next hops"


# ---- 3. the select kernel -------------------------------------------------------------------------------------------------
def _select_case(net, B, seed):
    from tarl_hip import synth
    N, A = net.num_roads, 60
    gen = torch.Generator().manual_seed(seed)
    xs, ags = [], []
    for b in range(B):
        x = synth.random_state(net, seed=seed + b)
        x[:, 0] = torch.randint(0, A, (N,), generator=gen).float()          # the head agent of every row
        ag = synth.population(A - 1, N, seed=seed + b)
        ag[3, 1], ag[4, 1], ag[5, 1] = -1.0, float(N + 3), 2.5             # destinations out of range / fractional
        rows = torch.randperm(N, generator=gen)
        x[rows[:4], 0] = 0.0                                               # empty FIFO: reads agent 0
        x[rows[4:7], 0] = torch.tensor([-2.0, float(A), float(A + 40)])   # heads out of range
        x[rows[7:10], 0] = torch.tensor([3.0, 4.0, 5.0])
        xs.append(x)
        ags.append(ag)
    return torch.stack(xs).cuda(), torch.stack(ags).cuda()


@pytest.mark.parametrize("B", [1, 3])
def test_select_matches_all_pairs_select(ops, B):
    from tarl_hip import synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    ei, N, Nmax = net.edge_index, net.num_roads, net.Nmax
    plan = ops.Plan(ei, N)
    w = _travel_times(ops, plan, net.x, Nmax, net.congestion_constant).cuda()
    nh_ap = ops.all_pairs_shortest_paths(plan, w)[0]                      # (1, N, N): shared by the environments
    x0, ag = _select_case(net, B, seed=11)
    if B == 1:
        x0, ag = x0[0], ag[0]
    want = x0.clone()
    ops.select_next_hop(want, Nmax, ag, nh_ap)
    assert not torch.equal(want, x0)
    # every destination has a tree (the all-pairs columns): the same state
    table = nh_ap[0].t().to(torch.int32).contiguous()
    slot = torch.arange(N, dtype=torch.int32, device="cuda")
    got = x0.clone()
    ops.select_next_hop_dest(got, Nmax, ag, slot, table)
    assert torch.equal(got, want)
    # a third of the destinations without a tree: their rows keep their selection, the others as above
    keep = torch.rand(N, generator=torch.Generator().manual_seed(1)) < 0.66
    kd = torch.nonzero(keep).view(-1)
    slot2 = torch.full((N,), -1, dtype=torch.int32)
    slot2[kd] = torch.arange(kd.numel(), dtype=torch.int32)
    got2 = x0.clone()
    ops.select_next_hop_dest(got2, Nmax, ag, slot2.cuda(), table[kd.cuda()].contiguous())
    xv, wv, gv, av = x0.view(-1, N, x0.size(-1)).cpu(), want.view(-1, N, x0.size(-1)).cpu(), \
        got2.view(-1, N, x0.size(-1)).cpu(), ag.view(-1, ag.size(-2), 9).cpu()
    untouched = 0
    for b in range(xv.size(0)):
        exp = wv[b].clone()
        for i in range(N):
            head = int(xv[b, i, 0])
            if 0 <= head < av.size(1):
                dest = int(av[b, head, 1])
                if 0 <= dest < N and not bool(keep[dest]):
                    exp[i] = xv[b, i]
                    untouched += 1
        assert torch.equal(gv[b], exp), f"environment {b}"
    assert untouched > 0


# ---- 4. DijkstraAgents: per-destination against all-pairs, step by step ------------------------------------------------------
def _simulator(net, agents, method, t0):
    from src._compat import Data
    from src.agents.base import DijkstraAgents
    from src.feature_helpers import FeatureHelpers
    from src.transportation_simulator import TransportationSimulator
    sim = TransportationSimulator("cuda")
    ei = net.edge_index.cuda()
    sim.graph = Data(x=net.x.clone().cuda(), edge_index=ei, edge_attr=net.edge_attr.cuda(), edge_index_routes=ei,
                     edge_attr_routes=net.edge_attr.cuda(), num_roads=net.num_roads,
                     critical_number=net.critical_number.cuda(), congestion_constant=net.congestion_constant.cuda())
    sim.Nmax, sim.h = net.Nmax, FeatureHelpers(Nmax=net.Nmax)
    ag = DijkstraAgents("cuda", method=method)
    ag.agent_features = agents.clone().cuda()
    sim.agent = ag
    sim.config_parameters(timestep_size=1, start_time=t0)
    ag.set_time(t0)
    return sim, ag


def test_agent_run_matches_all_pairs(ops, capsys):
    """A few hundred steps on a heterogeneous torus (untied shortest paths): the per-destination agent drives the
    simulation exactly as the all-pairs agent does — state and agent table bit for bit after every step, also across a
    replacement of the agent table (new destinations) between two refreshes."""
    from tarl_hip import synth
    net = synth.torus_network(8, 8, heterogeneous=True, seed=3)
    N = net.num_roads
    t0 = 21_600
    agents = synth.population(1_500, N, seed=8, t0=t0, t1=t0 + 240)
    sims = [_simulator(net, agents, m, t0) for m in ("all_pairs", "per_destination")]
    (sim_a, ag_a), (sim_d, ag_d) = sims
    assert "per-destination" not in capsys.readouterr().out
    for s in range(320):
        if s == 155:                                   # between two refreshes: a new agent table with new destinations
            new = ag_a.agent_features.clone()
            later = new[:, ag_a.DEPARTURE_TIME] > t0 + s + 5
            new[later, ag_a.DESTINATION] = torch.randint(0, N, (int(later.sum()),), device="cuda",
                                                         generator=torch.Generator("cuda").manual_seed(2)).float()
            ag_a.agent_features, ag_d.agent_features = new, new.clone()
        sim_a.run()
        sim_d.run()
        assert torch.equal(sim_d.graph.x, sim_a.graph.x), f"state after step {s}"
        assert torch.equal(ag_d.agent_features, ag_a.agent_features), f"agents after step {s}"
    assert "Dijkstra routing: per-destination trees" in capsys.readouterr().out
    assert ag_d.next_hop_tensor is None and ag_a.dest_next_hop is None
    D = ag_d.destinations.numel()
    assert ag_d.dest_next_hop.shape == (D, N) and ag_d.dest_next_hop.dtype == torch.int32
    assert torch.equal(ag_d.destinations,
                       torch.unique(ag_d.agent_features[:, ag_d.DESTINATION].to(torch.int64)))  # rebuilt at the swap
    assert int(ag_d.dest_slot[ag_d.destinations].min()) == 0 and int((ag_d.dest_slot >= 0).sum()) == D
    # the per-destination rows are the all-pairs columns of the last refresh
    assert torch.equal(ag_d.dest_next_hop.to(torch.int64), ag_a.next_hop_tensor[:, ag_d.destinations].t())
    done = float(ag_a.agent_features[:, ag_a.DONE].sum())
    assert done > 50, done


# ---- 5. the CLI above the all-pairs size limit --------------------------------------------------------------------------------
def test_main_cli_dijkstra_auto_on_large_graph(tmp_path, monkeypatch, capsys):
    """`main.py --algo dijkstra --dijkstra-method auto` on a 25 x 50 torus (R = 5 000 roads, 20 000 turn edges): auto picks
    the per-destination trees, agents arrive, the eval report is written."""
    import importlib
    sys.path.insert(0, PKG)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    main(["--algo", "dijkstra", "--dijkstra-method", "auto", "--mode", "eval", "--scenario", "synthetic-20000-4096",
          "--steps", "400", "--start-end-time", "21540", "21940", "--output-dir", str(tmp_path / "runs")])
    out = capsys.readouterr().out
    assert "Dijkstra routing: per-destination trees" in out and "5000 nodes" in out
    arrived = int([ln for ln in out.splitlines() if ln.startswith("Agents arrived:")][-1].split()[-1])
    assert arrived > 0, out
    assert os.path.exists(tmp_path / "runs" / "msa_expected_flows.csv")
