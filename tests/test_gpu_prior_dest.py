"""GPU: the shortest-path prior from per-destination trees (MPNNPolicyNet.prior_method = "per_destination",
tarl_prior_dest_table and the *_dest prior entry points). Every graph here satisfies the exactness condition of
tarl_dest_trees (exponent span of the weights + ceil(log2 hops) <= 28 bits), which each check asserts; there the table's
columns, the logits, the draws and the updates equal the all-pairs path bit for bit."""
import math
import os
import sys

import pytest
import torch

from conftest import PKG
from tree_restatement import adjacency, cpu_dijkstra

pytestmark = pytest.mark.gpu
UNREACHABLE = -1e20


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    sys.path.insert(0, PKG)
    from tarl_hip import ops as _ops
    return _ops


def assert_exact(w, N):
    """The 28-bit condition on every path: positive weights span at most ``span`` binary exponents, a path has < N hops."""
    pos = w[(w > 0) & torch.isfinite(w)].double()
    span = math.floor(math.log2(float(pos.max()))) - math.floor(math.log2(float(pos.min()))) + 1
    assert span + math.ceil(math.log2(max(N, 2))) <= 28, (span, N)


def _free_flow(net):
    return net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()


def _check_columns(ops, ei, w, N, dests):
    plan = ops.Plan(ei, N)
    assert_exact(w, N)
    d_ap = ops.all_pairs_shortest_paths(plan, w, want_next_hop=False, want_dist=True)[1][0]
    table = ops.prior_dest_table(plan, w, dests)
    assert table.shape == (N, dests.numel()) and table.dtype == torch.float32
    ok = (dests >= 0) & (dests < N)
    assert torch.equal(table[:, ok], d_ap[:, dests[ok]]), "columns == dist_matrix[:, d]"
    assert bool(torch.isinf(table[:, ~ok]).all())
    return table, d_ap


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_table_heterogeneous_torus_25x25(ops):
    from tarl_hip import synth
    net = synth.torus_network(25, 25, heterogeneous=True, seed=1)
    N = net.num_roads
    table, _ = _check_columns(ops, net.edge_index, _free_flow(net), N, torch.arange(N, dtype=torch.int64, device="cuda"))
    assert bool((table.diagonal() == 0).all())


def test_table_matsim_grid_src_dest(ops, tmp_path):
    """SRC / DEST pseudo-nodes: a DEST node has no out-edges, so most pairs are +inf."""
    from src.matsim_io import build_network
    from tarl_hip import synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, Nmax = build_network(str(tmp_path / "network"))
    ei, N = graph.edge_index.cpu(), graph.x.size(0)
    w = graph.x[:, 3 * Nmax + 2][graph.edge_index[1]].to("cuda", torch.float32).contiguous()
    dests = torch.randperm(N, generator=torch.Generator().manual_seed(3))[: N // 2].cuda()
    table, _ = _check_columns(ops, ei, w, N, dests)
    assert bool(torch.isinf(table).any()) and bool(torch.isfinite(table).any())


def test_table_unreachable_and_out_of_range_destinations(ops):
    """Two disjoint tori: destinations in one cannot be reached from the other; out-of-range ids get a column of +inf."""
    from tarl_hip import synth
    a = synth.torus_network(4, 3, heterogeneous=True, seed=5)
    b = synth.torus_network(3, 3, heterogeneous=True, seed=6)
    Na, Nb = a.num_roads, b.num_roads
    ei = torch.cat([a.edge_index, b.edge_index + Na], dim=1)
    w = torch.cat([_free_flow(a), _free_flow(b)])
    N = Na + Nb
    dests = torch.tensor([0, Na + 2, -3, N, 5, N - 1], dtype=torch.int64, device="cuda")
    table, _ = _check_columns(ops, ei, w, N, dests)
    assert bool(torch.isinf(table[Na:, 0]).all()) and bool(torch.isinf(table[:Na, 1]).all())
    assert bool(torch.isfinite(table[:Na, 0]).all()) and bool(torch.isinf(table[:, 2:4]).all())


# ---- the logits -----------------------------------------------------------------------------------------------------------
def _obs_case(net, M, seed):
    """Observations with real counts and head agents (column 8 = the head agent's DESTINATION)."""
    g = torch.Generator().manual_seed(seed)
    N, Nmax = net.num_roads, net.Nmax
    nf = net.x[:, 3 * Nmax:3 * Nmax + 7].clone().unsqueeze(0).repeat(M, 1, 1)
    nf[..., 1] = torch.floor(torch.rand((M, N), generator=g) * (nf[..., 0] + 1))
    ag = torch.rand((M, N, 9), generator=g) * 100
    ag[..., 1] = torch.randint(0, N, (M, N), generator=g).float()
    return torch.cat((nf, ag), dim=-1).contiguous()


@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("w", [1.0, 0.37, 0.0])
def test_observation_logits_equal_all_pairs(ops, M, w):
    """tarl_policy_prior_logits_dest == tarl_policy_prior_logits; a destination without a column gets the sentinel."""
    from tarl_hip import synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    N = net.num_roads
    plan = ops.Plan(net.edge_index, N)
    ff = _free_flow(net)
    assert_exact(ff, N)
    dist = ops.all_pairs_shortest_paths(plan, ff, want_next_hop=False, want_dist=True)[1][0]
    obs = _obs_case(net, M, seed=M + 7).cuda().contiguous()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(2)).cuda()
    dests = torch.unique(obs[..., 8].reshape(-1).long())
    slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    slot[dests] = torch.arange(dests.numel(), dtype=torch.int32, device="cuda")
    table = ops.prior_dest_table(plan, ff, dests)
    a = ops.policy_prior_logits(plan, obs, emb, dist, w)
    b = ops.policy_prior_logits(plan, obs, emb, table, w, dest_slot=slot)
    assert torch.equal(a, b)
    # drop one destination's column: its candidates now carry the sentinel
    gone = int(dests[0])
    slot2 = slot.clone()
    slot2[gone] = -1
    c = ops.policy_prior_logits(plan, obs, emb, table, w, dest_slot=slot2)
    src, dst = net.edge_index[0].cuda(), net.edge_index[1].cuda()
    hit = obs[:, src, 8].long() == gone                                      # (M, E)
    assert bool(hit.any())
    assert torch.equal(c[~hit], a[~hit])
    sentinel = (emb[obs[:, dst, 6].long()] + UNREACHABLE)[hit]
    assert torch.equal(c[hit], sentinel)


def _engine(net, B, A, seed, t0=21540, t1=21560):
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    pops = torch.stack([synth.population(A, net.num_roads, seed=seed + b, t0=t0, t1=t1) for b in range(B)]).cuda()
    return SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax, pops,
                     congestion_constant=net.congestion_constant, seed=5)


@pytest.mark.parametrize("w", [1.0, 0.37, 0.0])
def test_packed_state_logits_equal_all_pairs_with_empty_rows(ops, w):
    """tarl_fused_prior_logits_dest == tarl_fused_prior_logits after live frames (queues, empty rows reading agent 0)."""
    from src.agents.base import destination_set
    from tarl_hip import synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=4)
    N, B = net.num_roads, 70
    eng = _engine(net, B, 300, seed=0)
    eng.reset()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(1)).cuda()
    eng.prepare_policy(emb)
    for _ in range(12):
        eng.frame_fused()
    ff = _free_flow(net)
    dist = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    dests, slot = destination_set(eng.agents, N)
    table = ops.prior_dest_table(eng.plan, ff, dests)
    obs = ops.fused_obs16(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents)
    assert float((obs[..., 1] == 0).float().mean()) > 0.05                    # empty rows present
    a = ops.fused_prior_logits(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents, emb, dist, w)
    b = ops.fused_prior_logits(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents, emb, table, w, dest_slot=slot)
    assert torch.equal(a, b)
    assert torch.equal(b, ops.policy_prior_logits(eng.plan, obs, emb, table, w, dest_slot=slot))
    # agent 0's destination without a column: every empty row's candidates get the sentinel
    d0 = int(eng.agents[0, 0, 1])
    slot2 = slot.clone()
    slot2[d0] = -1
    c = ops.fused_prior_logits(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents, emb, table, w, dest_slot=slot2)
    hit = obs[:, net.edge_index[0].cuda(), 8].long() == d0
    assert bool(hit.any()) and bool((c[hit] <= -1e19).all()) and torch.equal(c[~hit], a[~hit])


# ---- the rollout ------------------------------------------------------------------------------------------------------------
def _rollout(net, pops, T, method, table_fn, chunks=None):
    from tarl_hip.engine import SimEngine
    B, N = pops.size(0), net.num_roads
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.clone(), congestion_constant=net.congestion_constant, seed=13)
    eng.reset()
    table, slot = table_fn(eng)
    emb = torch.randn(N, generator=torch.Generator().manual_seed(8)).cuda()
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    t0 = 0
    for n in (chunks or [T]):
        sl = slice(t0, t0 + n)
        eng.rollout_prior(n, emb, table, prior_weight=0.37, temperature=1.0, policy_seed=99, policy_counter0=1 + t0,
                          choice8=ch[sl], log_prob=lp[sl], reward=rw[sl], counts=ct[t0:t0 + n + 1], dest_slot=slot)
        t0 += n
    torch.cuda.synchronize()
    return ch, lp, rw, ct, eng.x.clone(), eng.agents.clone()


def test_rollout_config4_bit_identical_to_all_pairs(ops):
    """Config 4 (25 x 25 torus), B = 1 024 environments of population_batch, 32 frames: choice bytes, log-probs, rewards,
    counts, the final x and agent tables equal the all-pairs rollout's; the multi-frame call equals single frames."""
    from src.agents.base import destination_set
    from tarl_hip import synth
    net = synth.torus_network(25, 25, heterogeneous=True, seed=1)
    N, B, T = net.num_roads, 1024, 32
    ff = _free_flow(net)
    assert_exact(ff, N)
    pops = synth.population_batch(2048, N, B, seed=21, device="cuda", t0=21540, t1=21570)
    plan = ops.Plan(net.edge_index, N)
    dist = ops.all_pairs_shortest_paths(plan, ff, want_next_hop=False, want_dist=True)[1][0]

    def per_dest(eng):
        dests, slot = destination_set(eng.agents, N)
        return ops.prior_dest_table(eng.plan, ff, dests), slot
    ref = _rollout(net, pops, T, "all_pairs", lambda eng: (dist, None))
    got = _rollout(net, pops, T, "per_destination", per_dest)
    names = ("choice", "log_prob", "reward", "counts", "x", "agents")
    for n, a, b in zip(names, ref, got):
        assert torch.equal(a, b), n
    assert float(ref[2].abs().sum()) > 0 and float(ref[3][-1].float().sum()) > 0
    single = _rollout(net, pops, T, "per_destination", per_dest, chunks=[1] * T)
    for n, a, b in zip(names, got, single):
        assert torch.equal(a, b), f"single frames: {n}"


# ---- the PPO update --------------------------------------------------------------------------------------------------------
def _trainer(net, B, T, M, method, seed=0):
    from src.agents.base import destination_set
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    N = net.num_roads
    pops = synth.population_batch(300, N, B, seed=17, device="cuda", t0=21540, t1=21555)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops, congestion_constant=net.congestion_constant, seed=3)
    torch.manual_seed(seed)
    pol = MPNNPolicyNet(net.edge_index, N, _free_flow(net), device="cuda")
    pol.prior_method = method
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    kw = dict(prior_table=pol.dist_matrix) if method == "all_pairs" else \
        dict(prior_free_flow=pol.free_flow_weights(), prior_dests=destination_set(eng.agents, N))
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=2, sub_batch_size=M, seed=seed,
                       extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")],
                       policy="embedding_dijkstra", prior_weight=0.37, **kw)
    return tr, eng, pol


def test_train_iteration_bit_identical_to_all_pairs(ops):
    from tarl_hip import synth
    net = synth.torus_network(6, 6, heterogeneous=True, seed=2)
    assert_exact(_free_flow(net), net.num_roads)
    out = {}
    for method in ("all_pairs", "per_destination"):
        tr, eng, pol = _trainer(net, 96, 24, 32, method)
        assert tr.rollout == "frames+prior"
        assert (tr.prior_dest_slot is None) == (method == "all_pairs")
        assert (pol._dist_matrix is None) == (method == "per_destination")
        tr.train_iteration()
        torch.cuda.synchronize()
        out[method] = (tr.flat.flat.clone(), [tr.flat.exp_avg.clone(), tr.flat.exp_avg_sq.clone()], tr.reward.clone())
    a, b = out["all_pairs"], out["per_destination"]
    assert float(a[2].abs().sum()) > 0
    assert torch.equal(a[0], b[0]), "flat parameters"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"Adam moment {i}"
    assert torch.equal(a[2], b[2])


def test_trainer_refuses_a_table_larger_than_half_the_free_memory(ops, monkeypatch):
    from tarl_hip import synth
    net = synth.torus_network(4, 4, heterogeneous=True, seed=2)
    real = torch.cuda.mem_get_info
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (64 * 1024, real(*a, **k)[1]))
    with pytest.raises(ValueError, match=r"per-destination prior table \(64 x \d+ fp32.*MiB\).*scratch.*free"):
        _trainer(net, 8, 4, 4, "per_destination")


def test_trainer_refuses_a_destination_set_that_misses_an_environment(ops):
    from src.agents.base import destination_set
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(4, 4, heterogeneous=True, seed=2)
    N, B = net.num_roads, 4
    pops = synth.population_batch(50, N, B, seed=1, device="cuda")
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops, congestion_constant=net.congestion_constant, seed=3)
    emb = torch.nn.Parameter(torch.zeros(N, 1, device="cuda"))
    crit = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in ((64, N + 1), (64,), (64, 64), (64,), (1, 64), (1,))]
    with pytest.raises(ValueError, match="cover"):
        VecPPOTrainer(eng, emb, crit, rollout_steps=4, sub_batch_size=4, policy="embedding_dijkstra",
                      prior_free_flow=_free_flow(net), prior_dests=destination_set(eng.agents[:1], N))


# ---- the module -----------------------------------------------------------------------------------------------------------
def test_module_forward_and_dijkstra_logits_per_destination(ops):
    """Forward (_PriorLogits) and compute_dijkstra_logits under per_destination equal all_pairs; the table follows a
    replaced agent table."""
    from src.agents.mpnn_agent import MPNNPolicyNet
    from tarl_hip import synth
    net = synth.torus_network(5, 4, heterogeneous=True, seed=3)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    ff = _free_flow(net)
    pols = {}
    for method in ("all_pairs", "per_destination"):
        torch.manual_seed(0)
        p = MPNNPolicyNet(net.edge_index.cuda(), N, ff, device="cuda")
        p.policy_head, p.prior_weight, p.prior_method = "embedding_dijkstra", 0.37, method
        p.agent_features = synth.population(200, N, seed=4).cuda()
        pols[method] = p
    nf = net.x[:, 3 * Nmax:3 * Nmax + 7].cuda().unsqueeze(0).repeat(3, 1, 1).contiguous()
    nf[..., 1] = torch.randint(0, 3, (3, N), generator=torch.Generator().manual_seed(1)).float().cuda()
    idx = torch.randint(0, 201, (3, N), generator=torch.Generator().manual_seed(2)).cuda()
    ef = torch.zeros((3, E, 1), device="cuda")
    outs = {m: p(nf, ef, idx) for m, p in pols.items()}
    assert torch.equal(outs["all_pairs"], outs["per_destination"])
    outs["per_destination"].sum().backward()
    outs["all_pairs"].sum().backward()
    assert torch.equal(pols["all_pairs"].nodes_embedding.weight.grad, pols["per_destination"].nodes_embedding.weight.grad)
    assert pols["per_destination"]._dist_matrix is None
    dst_ag = pols["per_destination"].agent_features[idx[0], 1].long()[net.edge_index[0].cuda()]
    tt = torch.rand(E, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(pols["all_pairs"].compute_dijkstra_logits(dst_ag, tt),
                       pols["per_destination"].compute_dijkstra_logits(dst_ag, tt))
    # a replaced agent table rebuilds the destination set
    pd = pols["per_destination"]
    t1, s1 = pd.prior_tables()
    pd.agent_features = synth.population(30, N, seed=9).cuda()
    t2, s2 = pd.prior_tables()
    assert t2 is not t1 and int((s2 >= 0).sum()) == t2.size(1) <= 31
    assert pd._dist_matrix is None


# ---- a graph beyond the all-pairs limit ------------------------------------------------------------------------------------
def test_large_graph_auto_never_builds_all_pairs(ops):
    """25 x 50 torus (N = 5 000) with auto: per_destination, no dist_matrix, a (N, D) table whose sampled columns equal the
    fp32 rounding of a host fp64 Dijkstra, and a short rollout without flags."""
    from src.agents.base import destination_set
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(25, 50, heterogeneous=True, seed=1)
    N, B = net.num_roads, 64
    assert N == 5000
    ff = _free_flow(net)
    assert_exact(ff, N)
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.policy_head, pol.prior_method = "embedding_dijkstra", "auto"
    assert pol.resolve_prior_method() == "per_destination"
    pops = synth.population_batch(4096, N, B, seed=3, device="cuda", t0=21540, t1=21560)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops, congestion_constant=net.congestion_constant, seed=3)
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    dests, slot = destination_set(eng.agents, N)
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight,
                                                         l[4].bias], rollout_steps=8, sub_batch_size=16,
                       policy="embedding_dijkstra", prior_free_flow=pol.free_flow_weights(), prior_dests=(dests, slot))
    assert tr.prior_table.shape == (N, dests.numel()) and pol._dist_matrix is None
    rev = adjacency(net.edge_index, ff.cpu().double(), N, reverse=True)
    table = tr.prior_table.cpu()
    for j in torch.randperm(dests.numel(), generator=torch.Generator().manual_seed(7))[:16].tolist():
        dc, _ = cpu_dijkstra(rev, N, int(dests[j]), reverse=True)
        ref = torch.tensor(dc, dtype=torch.float64).to(torch.float32)
        assert torch.equal(table[:, j], ref), j
    tr.collect()
    tr.check_flags()
    assert pol._dist_matrix is None


# ---- the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_trains_and_evaluates_per_destination(tmp_path, monkeypatch, capsys):
    import importlib
    sys.path.insert(0, PKG)
    from src.runner import Runner
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    created = []
    orig_setup = Runner.setup

    def spy_setup(self):
        orig_setup(self)
        created.append(self)
    monkeypatch.setattr(Runner, "setup", spy_setup)
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-1024", "--rollout-steps", "24",
          "--epochs", "2", "--steps", "6", "--num-envs", "4", "--policy-head", "embedding_dijkstra",
          "--prior-method", "per_destination", "--output-dir", str(tmp_path / "run"), "--seed", "1"])
    assert "Simulation Summary" in capsys.readouterr().out
    r = created[-1]
    assert r.policy_net.prior_method == "per_destination" and r.policy_net._dist_matrix is None
    from src.rl.ppo_trainer import ppo_train
    tr = ppo_train.last_trainer
    assert tr.rollout == "frames+prior" and tr.prior_dest_slot is not None
    assert tr.prior_table.size(0) == r.policy_net.num_nodes
    assert os.path.exists(tmp_path / "run" / "policy.pt")
