"""GPU: per-origin shortest-path trees (csrc/msa.hip: tarl_sssp_f64, tarl_msa_assign_sssp) and run_msa's
``method="per_origin"``. The CPU side is tree_restatement.py's: a heapq Dijkstra that accumulates fp64 left to right (the
reference's distances bit for bit) and the documented tie rule of the predecessors (fewest hops over tight edges, then
the smallest predecessor id)."""
import math
import os
import sys
import types

import pytest
import torch

from conftest import PKG, load_golden
from tree_restatement import adjacency, check_tree, cpu_dijkstra, cpu_tie_rule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def _torus(W, H, het, seed=1):
    from tarl_hip import synth
    net = synth.torus_network(W, H, heterogeneous=het, seed=seed)
    ff = net.x[:, 3 * net.Nmax + 2].to(torch.float64)
    return net, ff[net.edge_index[1]].contiguous()            # an edge costs what its head node costs (run_msa)


def _sources(N, k, seed):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:k].to(torch.int64)


# ---- 1. trees against the CPU Dijkstra ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,k", [(25, 25, 64), (25, 250, 16)])
def test_trees_heterogeneous_torus(ops, W, H, k):
    net, w = _torus(W, H, True)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    srcs = _sources(N, k, seed=W * H)
    dist, pred = ops.shortest_path_trees(plan, w.cuda(), srcs.cuda())
    out = adjacency(ei, w, N)
    for j, s in enumerate(srcs.tolist()):
        dc, _ = cpu_dijkstra(out, N, s)
        assert torch.equal(dist[j].cpu(), torch.tensor(dc, dtype=torch.float64)), f"distances from {s}"
    check_tree(ei, w, N, srcs, dist, pred)


def test_trees_homogeneous_torus_tie_rule(ops):
    """Nearly every pair is tied on a homogeneous torus: pred must equal the CPU tie rule, launch after launch."""
    net, w = _torus(12, 9, False)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    srcs = torch.arange(0, N, 7, dtype=torch.int64)
    dist, pred = ops.shortest_path_trees(plan, w.cuda(), srcs.cuda())
    out = adjacency(ei, w, N)
    for j, s in enumerate(srcs.tolist()):
        dc, _ = cpu_dijkstra(out, N, s)
        assert torch.equal(dist[j].cpu(), torch.tensor(dc, dtype=torch.float64))
        want = cpu_tie_rule(out, dc, N, s)
        assert torch.equal(pred[j].cpu(), torch.tensor(want, dtype=torch.int32)), f"tie rule from {s}"
    check_tree(ei, w, N, srcs, dist, pred)
    for _ in range(2):
        d2, p2 = ops.shortest_path_trees(plan, w.cuda(), srcs.cuda())
        assert torch.equal(p2, pred) and torch.equal(d2, dist)


def test_trees_matsim_grid_src_dest(ops, tmp_path):
    """SRC/DEST pseudo-nodes: zero-cost nodes and nodes no path reaches (+inf, pred -1); zero-weight edges in ties."""
    from src.matsim_io import build_network
    from tarl_hip import synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, _ = build_network(str(tmp_path / "network"))
    ei, N = graph.edge_index.cpu(), graph.x.size(0)
    Nmax = (graph.x.size(1) - 7) // 3
    x = graph.x.cpu()
    cost = torch.where(x[:, 3 * Nmax + 6] >= 0, x[:, 3 * Nmax + 2].to(torch.float64), torch.zeros(N, dtype=torch.float64))
    w = cost[ei[1]].contiguous()
    assert bool((w == 0).any())
    plan = ops.Plan(ei, N)
    srcs = torch.arange(N, dtype=torch.int64)
    dist, pred = ops.shortest_path_trees(plan, w.cuda(), srcs.cuda())
    out = adjacency(ei, w, N)
    for s in range(N):
        dc, _ = cpu_dijkstra(out, N, s)
        assert torch.equal(dist[s].cpu(), torch.tensor(dc, dtype=torch.float64)), f"distances from {s}"
        want = cpu_tie_rule(out, dc, N, s)
        assert torch.equal(pred[s].cpu(), torch.tensor(want, dtype=torch.int32)), f"tie rule from {s}"
    assert bool(torch.isinf(dist).any()) and bool((pred == -1).sum() > N)
    check_tree(ei, w, N, srcs, dist, pred)


def test_out_of_range_source_leaves_its_row(ops):
    from tarl_hip import lib
    L = lib.load()
    net, w = _torus(6, 5, True)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    srcs = torch.tensor([3, -1, N, N + 1000, 17], dtype=torch.int64, device="cuda")
    S = srcs.numel()
    dist = torch.full((S, N), -7.5, dtype=torch.float64, device="cuda")
    pred = torch.full((S, N), -9, dtype=torch.int32, device="cuda")
    need = int(L.tarl_msa_scratch_bytes(plan.handle, S))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    lib.check(L.tarl_sssp_f64(plan.handle, w.cuda().data_ptr(), srcs.data_ptr(), S, scratch.data_ptr(), need,
                              dist.data_ptr(), pred.data_ptr(), lib.current_stream()))
    torch.cuda.synchronize()
    for j in (1, 2, 3):
        assert bool((dist[j] == -7.5).all()) and bool((pred[j] == -9).all()), f"row {j} was written"
    d_ok, p_ok = ops.shortest_path_trees(plan, w.cuda(), srcs[[0, 4]].contiguous())
    assert torch.equal(dist[[0, 4]], d_ok) and torch.equal(pred[[0, 4]], p_ok)


# ---- helpers for run_msa on synthetic graphs ---------------------------------------------------------------------------------
def _graph_and_agents(W, H, agents, seed=5):
    from src._compat import Data
    from tarl_hip import synth
    net = synth.torus_network(W, H, heterogeneous=True, seed=1)
    graph = Data(x=net.x.cuda(), edge_index=net.edge_index.cuda(), num_roads=net.num_roads)
    ag = types.SimpleNamespace(agent_features=synth.population(agents, net.num_roads, seed=seed).cuda(), ORIGIN=0,
                               DESTINATION=1)
    return net, graph, ag


def _flows(fl, R):
    return torch.tensor([fl[i] for i in range(R)], dtype=torch.float64)


# ---- 2. reference goldens through the per-origin path ------------------------------------------------------------------------
@pytest.mark.parametrize("tag,het", [("grid", False), ("gridhet", True)])
def test_per_origin_msa_golden(ops, tmp_path, tag, het):
    """The end state of test_gpu_routing.py's classical run (same inputs), then run_msa(method="per_origin")."""
    from src.agents.base import DijkstraAgents
    from src.algorithms.user_equilibrium_msa import run_msa
    from src.transportation_simulator import TransportationSimulator
    from tarl_hip import synth
    g = load_golden("routing")
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 4, 6, seed=3, heterogeneous=het)
    synth.write_matsim_population_xml(str(tmp_path / "population.xml"), 4, 6, 260, seed=4, first_departure=21600,
                                      spread=60)
    sim = TransportationSimulator("cuda")
    sim.config_network(str(tmp_path / "network"))
    ag = DijkstraAgents("cuda")
    ag.config_agents_from_xml(str(tmp_path), verbose=False)
    ag.agent_features[0, ag.DEPARTURE_TIME] = 48 * 3600
    sim.agent = ag
    sim.config_parameters(timestep_size=1, start_time=21600)
    ag.set_time(21600)
    E_r = sim.graph.edge_index_routes.size(1)
    for s in range(int(g[f"{tag}__steps"])):
        u = torch.rand(E_r, generator=torch.Generator().manual_seed(900 + s))
        sim.model_core.direction_mpnn.inject_uniform(u)
        sim.run()
    assert torch.equal(sim.graph.x.cpu(), g[f"{tag}__x"][-1])          # the golden end state
    R = int(sim.graph.num_roads)
    for iters in (1, 3, 25):
        got = _flows(run_msa(sim.graph, ag, max_iter=iters, method="per_origin"), R)
        want = g[f"{tag}__msa_{iters}"]
        if het:
            assert torch.allclose(got, want, rtol=1e-9, atol=1e-9), f"MSA flows after {iters} iterations"
        elif iters == 1:      # tied paths: the same number of roads carries each pair, so the total volume agrees
            assert abs(float(got.sum()) - float(want.sum())) < 1e-9 and float(got.min()) >= 0.0


# ---- 3. per-origin against all-pairs at config-4 size ---------------------------------------------------------------------
def test_per_origin_matches_all_pairs_config4(ops):
    from src.algorithms.user_equilibrium_msa import run_msa
    net, graph, ag = _graph_and_agents(25, 25, 16_384)
    for iters in (1, 3, 25):
        a = _flows(run_msa(graph, ag, max_iter=iters, method="all_pairs"), net.num_roads)
        b = _flows(run_msa(graph, ag, max_iter=iters, method="per_origin"), net.num_roads)
        assert float(a.sum()) > 0
        assert torch.allclose(b, a, rtol=1e-9, atol=1e-9), f"{iters} iterations"
    # "auto" keeps the all-pairs path at this size
    c = _flows(run_msa(graph, ag, max_iter=3), net.num_roads)
    assert torch.equal(c, _flows(run_msa(graph, ag, max_iter=3, method="all_pairs"), net.num_roads))


# ---- 4. config-5 scale -------------------------------------------------------------------------------------------------
def test_per_origin_config5_scale(ops):
    from src.algorithms.user_equilibrium_msa import run_msa
    net, graph, ag = _graph_and_agents(25, 250, 262_144)
    R = net.num_roads
    a = _flows(run_msa(graph, ag, max_iter=3), R)                  # "auto" -> per_origin at N = 25 000
    b = _flows(run_msa(graph, ag, max_iter=3, method="per_origin"), R)
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.sum()) > 0
    assert torch.allclose(a, b, rtol=1e-12, atol=0.0)


def test_per_origin_config5_small_population_vs_cpu(ops):
    from src.algorithms.user_equilibrium_msa import run_msa
    net, graph, ag = _graph_and_agents(25, 250, 64, seed=11)
    R = net.num_roads
    got = _flows(run_msa(graph, ag, max_iter=1, method="per_origin"), R)
    ff = net.x[:, 3 * net.Nmax + 2].to(torch.float64)
    w = ff[net.edge_index[1]]
    out = adjacency(net.edge_index, w, R)
    feats = ag.agent_features[1:].cpu()
    want = torch.zeros(R, dtype=torch.float64)
    trips = {}
    for o, d in zip(feats[:, 0].long().tolist(), feats[:, 1].long().tolist()):
        trips.setdefault(o, []).append(d)
    for o, ds in trips.items():
        _, pred = cpu_dijkstra(out, R, o, targets=ds)
        for d in ds:                  # path[1:]: d included, o excluded (every node of a torus is a road)
            v = d
            while v != o:
                want[v] += 1.0
                v = pred[v]
    assert float(want.sum()) > 0
    assert torch.allclose(got, want, rtol=1e-9, atol=1e-9)


# ---- 5. the runner writes the MSA flows above the old size cap ------------------------------------------------------------
def test_runner_eval_writes_msa_flows_on_large_graph(tmp_path, monkeypatch, capsys):
    import importlib
    sys.path.insert(0, PKG)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    main(["--algo", "random", "--mode", "eval", "--scenario", "synthetic-20000-512", "--steps", "10",
          "--start-end-time", "21540", "21600", "--output-dir", str(tmp_path / "runs")])
    assert "Simulation Summary" in capsys.readouterr().out
    path = tmp_path / "runs" / "msa_expected_flows.csv"
    assert os.path.exists(path), "eval skipped the MSA step"
    rows = open(path).read().splitlines()
    assert rows[0] == "road,expected_hourly_flow" and len(rows) == 1 + 5000      # 25 x 50 torus: R = 5 000 > 4 096
    vals = [float(r.split(",")[1]) for r in rows[1:]]
    assert all(math.isfinite(v) and v >= 0.0 for v in vals) and sum(vals) > 0
