"""GPU: the vectorised policy evaluation — tarl_graphdist_mode_rollout against the three-launch chain and the reference,
tarl_episode_summary against numpy, VecEvaluator against the CPU oracle, against hand-composed frames and through the CLI."""
import csv
import importlib
import json
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

POLICY_SALT = 0x5DEECE66D


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _graph(kind, tmp_path):
    """(edge_index, N) of the 8 x 8 / 25 x 25 torus or of a MATSim grid with SRC / DEST pseudo-nodes (DEST: no out-edges,
    uneven degrees), as tests/test_gpu_gt_head.py builds one."""
    from tarl_hip import synth
    if kind == "matsim":
        from src.matsim_io import build_network
        synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 4, 6, seed=3)
        g, _ = build_network(str(tmp_path / "network"))
        return g.edge_index.cpu(), g.x.size(0)
    if kind == "irregular":
        # out-degrees 0 ... 126 (the packed path's limit), edges in shuffled order: the plan is not source-sorted, nodes
        # above four out-edges take the kernel's generic loop, node 1 200 crosses into a second chunk of 1 024 nodes
        gen = torch.Generator().manual_seed(17)
        N = 1300
        deg = torch.randint(0, 7, (N,), generator=gen)
        deg[[3, 500, 1200]] = torch.tensor([126, 64, 33])
        deg[[0, 7, 1299]] = 0
        src = torch.repeat_interleave(torch.arange(N), deg)
        dst = torch.cat([torch.randperm(N, generator=gen)[:int(d)] for d in deg])       # distinct targets per node
        perm = torch.randperm(src.numel(), generator=gen)
        return torch.stack([src[perm], dst[perm]]), N
    W, H = {"torus8": (8, 8), "config4": (25, 25)}[kind]
    net = synth.torus_network(W, H)
    return net.edge_index, net.num_roads


def _chain(ops, plan, logits, temperature):
    p = ops.graphdist_softmax(plan, logits, temperature)
    _, choice = ops.graphdist_mode(plan, p, want_choice=True)
    lp, _ = ops.graphdist_logprob_entropy(plan, p, choice=choice, want_entropy=False)
    return p, choice, lp


def _check_against_chain(ops, plan, ei, N, logits, temperature, sel_seed=5):
    """choice, choice8, sel8 and log_prob of the one-launch kernel == the chain's, bit for bit; sel8 against
    tarl_fused_set_actions of the chain's bytes on the same previous SELECTED_ROAD bytes. Returns the chain's (p, choice)."""
    from eval_restatement import rank_bytes
    B = logits.size(0)
    p, choice, lp = _chain(ops, plan, logits, temperature)
    prev = torch.randint(0, 3, (N, B), dtype=torch.uint8, device="cuda",
                         generator=torch.Generator(device="cuda").manual_seed(sel_seed))
    fs = ops.FusedState(plan, B, 2, "cuda", Nmax=2)          # only its sel8 column is used
    fs.sel8.copy_(prev)
    bytes_chain = rank_bytes(choice, ei, N)
    ops.fused_set_actions(plan, fs, bytes_chain)             # completes the bytes of nodes without out-edges in place
    sel8 = prev.clone()
    ch = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    c8 = torch.full((B, N), 0x55, dtype=torch.uint8, device="cuda")
    lp_m = ops.graphdist_mode_rollout(plan, logits, temperature, choice=ch, choice8=c8, sel8=sel8)
    assert torch.equal(ch, choice), "choice"
    assert torch.equal(c8, bytes_chain), "choice8"
    assert torch.equal(sel8, fs.sel8), "sel8"
    assert torch.equal(lp_m, lp), "log_prob"
    # every output alone (the others NULL) gives the same values
    lp_only = ops.graphdist_mode_rollout(plan, logits, temperature)
    assert torch.equal(lp_only, lp)
    c8b = torch.zeros_like(c8)
    ops.graphdist_mode_rollout(plan, logits, temperature, choice8=c8b)
    no_prev = torch.where((bytes_chain & 0x80) != 0, torch.full_like(c8, 0x80), bytes_chain)   # without sel8: previous rank 0
    assert torch.equal(c8b, no_prev)
    return p, choice


# ---- 1. the MODE kernel == the chain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["torus8", "config4", "matsim", "irregular"])
def test_mode_rollout_equals_the_chain_bit_for_bit(kind, tmp_path):
    from tarl_hip import ops
    ei, N = _graph(kind, tmp_path)
    plan = ops.Plan(ei, N)
    E = ei.size(1)
    if kind == "matsim":
        assert plan.num_groups < N and plan.max_out > 1          # nodes without out-edges, uneven degrees
    if kind == "irregular":
        assert plan.max_out == 126 and not plan.src_sorted and plan.num_groups < N
    gen = torch.Generator(device="cuda").manual_seed(11)
    for B in (1, 3, 64, 4096):
        for temperature in (1.0, 0.37):
            logits = 3.0 * torch.randn((B, E), device="cuda", generator=gen)
            _check_against_chain(ops, plan, ei, N, logits, temperature, sel_seed=B)


def test_mode_rollout_tie_rules_on_crafted_rows():
    """The comparison is on the PROBABILITIES: (row 0) two logits one ulp apart whose p round to the same value — the
    chain and the kernel take the FIRST, although the second logit is the larger; (row 1) a node whose candidates all carry
    the prior head's -1e20 sentinel: equal p, first edge; (row 2) equal logits everywhere: every node takes its first edge."""
    from eval_restatement import csr
    from tarl_hip import ops, synth
    net = synth.torus_network(8, 8)
    ei, N, E = net.edge_index, net.num_roads, net.edge_index.size(1)
    plan = ops.Plan(ei, N)
    out_ptr, out_eid = csr(ei, N)
    first = out_eid[out_ptr[:-1]]                                # first out-edge (lowest edge id) of every node
    e0 = out_eid[out_ptr[0]:out_ptr[1]]
    assert e0.numel() == 4 and bool((e0[1:] > e0[:-1]).all())
    logits = torch.randn((3, E), generator=torch.Generator().manual_seed(2))
    a = torch.tensor(1e-3)
    logits[0, e0] = torch.tensor([float(a), float(torch.nextafter(a, torch.tensor(1.0))), -5.0, -5.0])
    assert logits[0, e0[1]] > logits[0, e0[0]]
    e5 = out_eid[out_ptr[5]:out_ptr[6]]
    logits[1, e5] = -1e20
    logits[2] = 0.25
    p, choice = _check_against_chain(ops, plan, ei, N, logits.cuda(), 1.0)
    p, choice = p.cpu(), choice.cpu()
    assert p[0, e0[0]] == p[0, e0[1]] and choice[0, 0] == e0[0]
    assert bool((p[1, e5] == 0.25).all()) and choice[1, 5] == e5[0]
    assert torch.equal(choice[2].long(), first)


# ---- 2. the MODE kernel == the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dist_small", "dist_mid"])
def test_mode_rollout_equals_the_reference_mode(name):
    from oracle import dist
    from tarl_hip import ops
    z = load_golden(name)
    ei = z["edge_index"]
    N, E = int(ei.max()) + 1, ei.size(1)
    plan = ops.Plan(ei, N)

    def onehot(logits):
        ch = torch.empty((logits.size(0), N), dtype=torch.int32, device="cuda")
        ops.graphdist_mode_rollout(plan, logits.cuda().contiguous(), 1.0, choice=ch)
        out = torch.zeros((logits.size(0), E))
        for b, row in enumerate(ch.cpu().long()):
            out[b, row[row >= 0]] = 1
        return out
    got = onehot(z["logits"].view(1, -1))[0]
    assert torch.equal(got, z["mode"]) and torch.equal(got, dist.GraphDist(z["logits"], ei).mode)
    got_b = onehot(z["logits_b"])
    for b in range(z["logits_b"].size(0)):
        assert torch.equal(got_b[b], dist.GraphDist(z["logits_b"][b], ei).mode), b


# ---- the evaluation the oracle can follow: embedding head, 8 x 8 torus, a population a MODE policy can deliver ----------------
def _oracle_mode(net, emb):
    """The oracle's MODE action of the embedding head (state-independent): one-hot (E,) long, and its successor map."""
    from oracle import dist, nets
    gd = dist.GraphDist(nets.policy_logits(net.x[:, 3 * net.Nmax:], net.edge_index, emb), net.edge_index)
    action = gd.mode.long()
    succ = torch.empty(net.num_roads, dtype=torch.long)
    chosen = action.nonzero().view(-1)
    succ[net.edge_index[0, chosen]] = net.edge_index[1, chosen]
    return gd, action, succ


def _deliverable_population(net, succ, agents=128):
    """synth.population(agents, N, seed=7, t1=EPISODE_START + 200) with the destination of rows 1, 3, 5, ... replaced by the
    road three steps along the MODE successor map from the row's origin, so that a deterministic policy delivers somebody."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    pop = synth.population(agents, net.num_roads, seed=7, t1=EPISODE_START + 200)
    o = pop[1::2, 0].long()
    pop[1::2, 1] = succ[succ[succ[o]]].float()
    return pop


def _embedding_evaluator(net, pop, K, seed=3, env_base=0, **kw):
    from tarl_hip.engine import SimEngine
    from tarl_hip.evaluator import VecEvaluator
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                    congestion_constant=net.congestion_constant, num_envs=K, seed=seed, env_base=env_base)
    return VecEvaluator(eng, "embedding", emb=emb.cuda(), **kw), emb


# ---- 3. the summary kernel ---------------------------------------------------------------------------------------------------
def _assert_summary_equal(got, want):
    for k in ("counts", "sums", "hist", "episode_return"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_episode_summary_on_a_real_rollout_and_on_a_crafted_table():
    """Times and rewards are integer-valued fp32, so every fp64 sum is exact whatever the order: == without a tolerance."""
    import eval_restatement as R
    from tarl_hip import ops, synth
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    ev, _ = _embedding_evaluator(net, _deliverable_population(net, _oracle_mode(net, emb)[2]), K=8)
    res = ev.run(300)
    assert not res.domain_exit and min(res.arrived) >= 1
    eng = ev.eng
    for bw, nb in ((10.0, 720), (1.0, 16), (7.0, 1)):
        got = ops.episode_summary(eng.agents, reward=ev.reward, frames=300, bin_width=bw, num_bins=nb)
        _assert_summary_equal(got, R.summary(eng.agents.cpu().numpy(), ev.reward[:300].cpu().numpy(), bw, nb))
    assert int(got["counts"].sum()) == 8 * 128
    # crafted: environment 0 without an arrival, environment 1 with a travel time past the last bin
    ag = torch.zeros((2, 7, 9))
    ag[:, :, 2] = 21600.0
    ag[0, 1:4, 7] = 1                       # three on the way, three waiting
    ag[1, 1, 7] = 1
    for row, tt in ((2, 5.0), (3, 15.0), (4, 7300.0), (5, 7190.0)):
        ag[1, row, 8] = 1
        ag[1, row, 3] = 21600.0 + tt
    ag[1, 0, 8] = 1                         # the dummy row is skipped even when it looks arrived
    rw = -torch.tensor([[3.0, 1.0], [3.0, 2.0], [3.0, 2.0], [2.0, 1.0]])
    got = ops.episode_summary(ag.cuda(), reward=rw.cuda(), bin_width=10.0, num_bins=720)
    _assert_summary_equal(got, R.summary(ag.numpy(), rw.numpy(), 10.0, 720))
    c, s, h = got["counts"].cpu(), got["sums"].cpu(), got["hist"].cpu()
    assert c.tolist() == [[0, 3, 3], [4, 1, 1]]
    assert s[0].tolist() == [0.0, 0.0, 0.0] and s[1].tolist() == [14510.0, 5.0 ** 2 + 15.0 ** 2 + 7300.0 ** 2 + 7190.0 ** 2, 7300.0]
    assert int(h[0].sum()) == 0 and h[1, 0] == 1 and h[1, 1] == 1 and h[1, 719] == 2 and int(h[1].sum()) == 4
    assert got["episode_return"].cpu().tolist() == [-11.0, -6.0]
    # no reward buffer: a zero return; frames=2: the first two frames only
    assert ops.episode_summary(ag.cuda())["episode_return"].cpu().tolist() == [0.0, 0.0]
    assert ops.episode_summary(ag.cuda(), reward=rw.cuda(), frames=2)["episode_return"].cpu().tolist() == [-6.0, -3.0]


# ---- 4. oracle replay of a MODE evaluation -------------------------------------------------------------------------------------
def test_mode_evaluation_replayed_by_the_oracle():
    """Embedding head, 8 x 8 torus, K = 4, 300 frames, 128 agents of which every other one is bound for the road three MODE
    steps from its origin. The oracle computes the MODE action once from its own logits; oracle.sim.env_step replays every
    frame of every environment with the Gumbel values the kernels consumed (ops.noise_export). Device action == oracle
    action on every node, every frame's reward equal, final x and agent table bit-exact, and the EvalResult equal to the
    statistics of the oracle's final agent tables. Guards against passing on nothing, per environment: no count reaches Nmax,
    >= 1 000 Response pops, >= 5 arrivals (the CPU oracle under torch's own noise gave counts <= 12 of 15, 1 527 - 1 542
    pops and 12 - 14 arrivals for these inputs; on the device's noise streams, engine seed 3: largest count 12 in all four
    environments, 1 526 - 1 539 pops, 11 - 14 arrivals; the test prints them)."""
    import eval_restatement as R
    from oracle import sim
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    N, Nmax, K, T = net.num_roads, net.Nmax, 4, 300
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    gd, action, succ = _oracle_mode(net, emb)
    ps = gd.proba_sort.view(N, 4).sort(dim=1, descending=True).values
    print(f"[mode replay] smallest relative gap between a node's two largest probabilities: "
          f"{float(((ps[:, 0] - ps[:, 1]) / ps[:, 0]).min()):.3e}")
    pop = _deliverable_population(net, succ)
    ev, _ = _embedding_evaluator(net, pop, K)
    eng = ev.eng
    noise0 = eng.noise_counter + 1                     # the reset inside run() leaves the noise counter alone
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    # the action: the same bytes in every environment, and the oracle's edge on every node
    want_edges = torch.full((N,), -1, dtype=torch.long)
    chosen = action.nonzero().view(-1)
    want_edges[net.edge_index[0, chosen]] = chosen
    for b in range(K):
        assert torch.equal(R.edges_of_bytes(ev.action8[b], net.edge_index, N), want_edges), f"MODE action of environment {b}"
    assert torch.equal(eng.fs.sel8.t().contiguous(), ev.action8)
    rw = ev.reward[:T].cpu()
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    finals, rewards = [], []
    for b in range(K):
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pop.clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        n_pops, max_count, r_b = 0, 0.0, []
        for t in range(T):
            g = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
            out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, float(EPISODE_START + t), Nmax, gumbel=g,
                               congestion_constant=net.congestion_constant)
            n_pops += int(out["popped"].sum())
            max_count = max(max_count, float(x[:, c.N].max()))
            assert float(out["reward"]) == float(rw[t, b]), f"reward of environment {b}, frame {t}"
            r_b.append(float(out["reward"]))
        assert torch.equal(x, eng.x[b].cpu()), f"final state of environment {b}"
        assert torch.equal(ag, eng.agents[b].cpu()), f"agent table of environment {b}"
        arrivals = int(ag[1:, sim.DONE].sum())
        print(f"[mode replay] environment {b}: largest count {max_count:.0f} of {Nmax}, {n_pops} pops, {arrivals} arrivals")
        assert max_count < Nmax and n_pops >= 1000 and arrivals >= 5, (max_count, n_pops, arrivals)
        finals.append(ag)
        rewards.append(r_b)
    want = R.per_env(R.summary(torch.stack(finals).numpy(), np.asarray(rewards, dtype=np.float32).T, 10.0, 720), 10.0)
    for b, w in enumerate(want):
        got = dict(arrived=res.arrived[b], on_way=res.on_way[b], not_departed=res.not_departed[b],
                   episode_return=res.episode_return[b], avg=res.avg_travel_time[b], std=res.std_travel_time[b],
                   max=res.max_travel_time[b], p50=res.p50_travel_time[b], p95=res.p95_travel_time[b])
        assert got == w, (b, got, w)
        assert res.frames[b] == T
    a = np.asarray(res.episode_return)
    g = res.aggregate["episode_return"]
    assert g["mean"] == a.mean() and g["se"] == a.std(ddof=1) / math.sqrt(K) and g["n"] == K
    assert res.aggregate["avg_travel_time"]["missing"] == 0 and res.envs_without_arrival == 0


# ---- 5. evaluator properties ---------------------------------------------------------------------------------------------------
def test_evaluator_is_reproducible_and_environment_b_is_the_solo_engine_b():
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    pop = _deliverable_population(net, _oracle_mode(net, emb)[2])
    ev1, _ = _embedding_evaluator(net, pop, 8)
    ev2, _ = _embedding_evaluator(net, pop, 8)
    r1, r2 = ev1.run(300), ev2.run(300)
    assert r1 == r2 and not r1.domain_exit
    assert torch.equal(ev1.eng.x, ev2.eng.x) and torch.equal(ev1.eng.agents, ev2.eng.agents)
    # MODE with a state-independent head: one action for all environments, yet the noise is per environment
    assert bool((ev1.action8 == ev1.action8[0]).all())
    tables = ev1.eng.agents
    assert any(not torch.equal(tables[0], tables[b]) for b in range(1, 8))
    for b in (0, 5):
        solo, _ = _embedding_evaluator(net, pop, 1, env_base=b)
        rs = solo.run(300)
        assert torch.equal(solo.eng.x[0], ev1.eng.x[b]) and torch.equal(solo.eng.agents[0], ev1.eng.agents[b]), b
        assert rs.episode_return[0] == r1.episode_return[b] and rs.arrived[0] == r1.arrived[b]
        assert rs.aggregate["episode_return"]["ci95"] is None          # K = 1: no interval
    # default length: to the end of the episode (the frame that pushes the clock past EPISODE_END is the last)
    assert ev1.episode_frames == 3661


def _free_flow_weights(net):
    return net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()


def _state_engine(net, K, seed=11):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START, SimEngine
    pops = synth.population_batch(400, net.num_roads, K, seed=21, device="cuda", t1=EPISODE_START + 40)
    return SimEngine(net.x.cuda().unsqueeze(0).repeat(K, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                     pops.clone(), congestion_constant=net.congestion_constant, seed=seed)


def test_sampled_evaluation_equals_frames_composed_by_hand():
    from tarl_hip import ops, synth
    from tarl_hip.evaluator import VecEvaluator
    net = synth.torus_network(8, 8)
    N, K, T = net.num_roads, 8, 48
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0)).cuda()
    e1, e2 = _state_engine(net, K), _state_engine(net, K)
    table = ops.all_pairs_shortest_paths(e1.plan, _free_flow_weights(net), want_next_hop=False, want_dist=True)[1][0]
    ev = VecEvaluator(e1, "embedding_dijkstra", emb=emb, prior_table=table, prior_weight=0.05, keep_actions=True)
    res = ev.run(T, deterministic=False)
    assert not res.domain_exit
    e2.reset()
    rw = torch.zeros((T, K), device="cuda")
    c8 = torch.zeros((K, N), dtype=torch.uint8, device="cuda")
    for t in range(T):
        logits = ops.fused_prior_logits(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents, emb, table, 0.05)
        ops.graphdist_rollout(e2.plan, logits, 1.0, seed=e2.seed ^ POLICY_SALT, counter=e2.sample_counter + 1, choice8=c8,
                              sel8=e2.fs.sel8)
        assert torch.equal(c8, ev.actions[t]), t
        e2.frame_fused(skip_choice=True, reward=rw[t])
    assert torch.equal(rw, ev.reward[:T]) and float(rw.abs().sum()) > 0
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert len({bytes(ev.actions[:, b].cpu().numpy().tobytes()) for b in range(K)}) > 1       # sampled: they differ
    # the embedding head, sampled, is the engine's own table draw
    e3, e4 = _state_engine(net, K), _state_engine(net, K)
    VecEvaluator(e3, "embedding", emb=emb).run(T, deterministic=False)
    e4.reset()
    e4.prepare_policy(emb, 1.0)
    for t in range(T):
        e4.frame_fused(reward=rw[t])
    assert torch.equal(e3.x, e4.x) and torch.equal(e3.agents, e4.agents)


# ---- 6. state-dependent heads --------------------------------------------------------------------------------------------------
def _gt_state(seed):
    """Scaled random graph-transformer weights (as tests/test_gpu_gt_head.py draws them)."""
    from src.transformer import GraphTransformerNet
    from tarl_hip import ops
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4,
                                                       dropout=0.1).state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    for k in ops.GT_PARAM_KEYS:
        if k.endswith("weight") and "norm" not in k:
            sd[k] = torch.randn(sd[k].shape, generator=gen) / sd[k].size(-1) * (1e-4 if k == "node_emb.weight" else 1.0)
        if k.endswith("bias") or "norm" in k:
            sd[k] = sd[k] + 0.4 * torch.randn(sd[k].shape, generator=gen)
    for k in ops.GT_BUFFER_KEYS:
        sd[k] = (torch.rand(16, generator=gen) + 0.5) if k.endswith("var") else 0.3 * torch.randn(16, generator=gen)
    return sd


@pytest.mark.parametrize("head", ["prior_all_pairs", "prior_per_destination", "edge_mlp", "graph_transformer"])
def test_state_dependent_heads_equal_a_loop_of_existing_ops(head):
    """32 frames of VecEvaluator (MODE, K = 16, 8 x 8 torus) == per frame: logits -> graphdist_softmax ->
    graphdist_mode(want_choice=True) -> frame_fused(action=...), all existing ops: action bytes, rewards, final x, agents."""
    from src.agents.base import destination_set
    from tarl_hip import ops, synth
    from tarl_hip.evaluator import VecEvaluator
    net = synth.torus_network(8, 8)
    N, Nmax, K, T = net.num_roads, net.Nmax, 16, 32
    gen = torch.Generator().manual_seed(4)
    emb = torch.randn(N, generator=gen).cuda()
    e1, e2 = _state_engine(net, K), _state_engine(net, K)
    plan = e2.plan
    if head.startswith("prior"):
        w = _free_flow_weights(net)
        slot = None
        if head == "prior_all_pairs":
            table = ops.all_pairs_shortest_paths(plan, w, want_next_hop=False, want_dist=True)[1][0]
        else:
            dests, slot = destination_set(e1.agents, N)
            table = ops.prior_dest_table(plan, w, dests)
        ev = VecEvaluator(e1, "embedding_dijkstra", emb=emb, prior_table=table, dest_slot=slot, prior_weight=0.05,
                          keep_actions=True)

        def logits_of():
            return ops.fused_prior_logits(plan, e2.fs, e2._x, Nmax, e2.agents, emb, table, 0.05, dest_slot=slot)
    elif head == "edge_mlp":
        shapes = ((64, 33), (64,), (32, 64), (32,), (1, 32), (1,))
        mlp = ops.EdgeMlpWeights(*((torch.rand(s, generator=gen) * 0.2 - 0.1).cuda() for s in shapes))
        ev = VecEvaluator(e1, "edge_mlp", emb=emb, edge_mlp=mlp, keep_actions=True)

        def logits_of():
            return ops.policy_edge_mlp(plan, ops.fused_obs16(plan, e2.fs, e2._x, Nmax, e2.agents), e2.ec, mlp, precision="x3")
    else:
        from src.transformer import laplacian_pe
        gw = ops.GtWeights({k: v.cuda().contiguous() for k, v in _gt_state(3).items()
                            if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS})
        pe = laplacian_pe(net.edge_index, N, N).cuda()
        ev = VecEvaluator(e1, "graph_transformer", emb=emb, gt_pe=pe, gt_weights=gw, keep_actions=True)

        def logits_of():
            return ops.policy_gt_logits(plan, ops.fused_obs16(plan, e2.fs, e2._x, Nmax, e2.agents), e2.ec, pe, gw)
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    e2.reset()
    rw = torch.zeros((T, K), device="cuda")
    for t in range(T):
        p = ops.graphdist_softmax(plan, logits_of(), 1.0)
        _, choice = ops.graphdist_mode(plan, p, want_choice=True)
        e2.frame_fused(action=choice, reward=rw[t])
        assert torch.equal(e2.fs.sel8.t().contiguous(), ev.actions[t]), f"action bytes of frame {t}"
    assert torch.equal(rw, ev.reward[:T]) and float(rw.abs().sum()) > 0
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert len({bytes(ev.actions[t].cpu().numpy().tobytes()) for t in range(T)}) > 1         # the action follows the state


# ---- 7. domain exit ------------------------------------------------------------------------------------------------------------
def test_domain_exit_is_reported_not_raised_and_never_averaged():
    """1 024 agents leaving within 120 s on the 8 x 8 torus under the MODE of a state-independent head: traffic collapses onto
    the cycles of one successor map and a FIFO count reaches Nmax (the CPU oracle: frame 68 for this embedding). The engine's
    status flag for a state the reference leaves too — not a fault; the kernels bound every slot index by Nmax."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    ev, _ = _embedding_evaluator(net, pop, 2)
    res = ev.run(256)
    assert res.domain_exit and res.aggregate is None and res.episode_return is None and res.avg_travel_time is None
    assert res.rows() == [] and res.envs_without_arrival is None
    a, b = res.domain_exit_frames
    assert 0 <= a < b <= 256 and b - a <= ev.poll_frames and res.frames_run == b
    print(f"[domain exit] flag seen in frames [{a}, {b})")
    assert "domain exit" in res.summary_lines()[0]
    # the engine is usable again
    ev.eng.reset()
    ev.eng.check_flags()
    again = ev.run(8, deterministic=False)
    assert not again.domain_exit and again.frames_run == 8 and again.aggregate is not None


# ---- 8. CLI end to end ---------------------------------------------------------------------------------------------------------
VEC_KEYS = ("avg_return", "avg_return_se", "avg_travel_time", "avg_travel_time_se", "arrived", "p95_travel_time", "envs",
            "domain_exit", "computation_time_ms")


def test_cli_train_with_eval_envs_then_eval_from_the_checkpoint(tmp_path, capsys):
    main = importlib.import_module("main").main
    run = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-1024", "--rollout-steps", "32",
          "--iterations", "2", "--eval-envs", "4", "--steps", "5", "--output-dir", str(run)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert len(logs) == 2 and [r["global_step"] for r in logs] == [32, 64]
    for rec in logs:
        assert all(f"eval_vec/{k}" in rec for k in VEC_KEYS)
        assert rec["eval_vec/envs"] == 4
        if not rec["eval_vec/domain_exit"]:
            for k in ("avg_return", "avg_return_se", "arrived", "computation_time_ms"):
                assert math.isfinite(rec[f"eval_vec/{k}"]), k
            for k in ("avg_travel_time", "avg_travel_time_se", "p95_travel_time"):      # None only where nobody arrived
                assert rec[f"eval_vec/{k}"] is None or math.isfinite(rec[f"eval_vec/{k}"]), k
        for k in ("eval/avg_return", "eval/episode_len", "eval/computation_time_ms"):   # the drop-in pass, as before
            assert k in rec
        assert not any(k.startswith("eval_vec_stochastic/") for k in rec)
    assert "Vectorised evaluation (4 environments, MODE)" in capsys.readouterr().out
    # evaluation from the checkpoint
    from src.runner import CHECKPOINT_PREFIX, Runner, RunnerArgs
    ev_dir = tmp_path / "ev"
    runner = Runner(RunnerArgs(algo="mpnn", scenario="synthetic-1024-1024", mode="eval", checkpoint=str(run / "policy.pt"),
                               eval_envs=8, eval_sampled=True, steps=200, output_dir=str(ev_dir)))
    try:
        runner.setup()
        file = torch.load(run / "policy.pt", map_location="cpu")
        own = runner.policy_net.state_dict()
        assert sorted(CHECKPOINT_PREFIX + k for k in own) == sorted(file)
        for k, v in own.items():
            assert torch.equal(v.cpu(), file[CHECKPOINT_PREFIX + k]), k
        out = runner.eval()
    finally:
        runner.close()
    text = capsys.readouterr().out
    assert "=== Vectorised evaluation (8 environments, MODE) ===" in text
    assert "=== Vectorised evaluation (8 environments, sampled) ===" in text
    doc = json.load(open(ev_dir / "eval_envs.json"))
    assert doc["mode"]["envs"] == 8 and doc["mode"]["deterministic"] and not doc["sampled"]["deterministic"]
    assert doc["mode"]["frames_run"] == 200 and doc["mode"]["settings"]["num_bins"] == 720
    rows = list(csv.DictReader(open(ev_dir / "eval_envs.csv")))
    mode_rows = [r for r in rows if r["kind"] == "mode"]
    assert not out["vectorised"]["mode"].domain_exit, "the synthetic scenario left the domain under MODE"
    assert len(mode_rows) == 8 and len(rows) == 16 and sorted(int(r["env"]) for r in mode_rows) == list(range(8))
    assert [float(r["episode_return"]) for r in mode_rows] == out["vectorised"]["mode"].episode_return
    # a checkpoint of another network is refused, naming the key
    bad = {k: (torch.zeros(3, 1) if k.endswith("nodes_embedding.weight") else v) for k, v in file.items()}
    torch.save(bad, tmp_path / "bad.pt")
    with pytest.raises(ValueError, match="nodes_embedding.weight"):
        runner.load_checkpoint(str(tmp_path / "bad.pt"))
    # defaults: no vectorised evaluation, no eval_vec/ key, one iteration
    plain = tmp_path / "plain"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-1024", "--rollout-steps", "32",
          "--steps", "5", "--output-dir", str(plain)])
    logs = [json.loads(l) for l in open(plain / "train_log.jsonl")]
    assert len(logs) == 1 and not any(k.startswith("eval_vec") for k in logs[0])
    assert not (plain / "eval_envs.json").exists()
    from src.rl.ppo_trainer import ppo_train
    assert ppo_train.last_vec_eval is None
