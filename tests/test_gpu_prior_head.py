"""GPU: the shortest-path prior head (policy_head = "embedding_dijkstra", csrc/prior.hip).

logit[e] = W_emb[ROAD_INDEX(dst(e))] + prior_weight * ((-dist[dst(e), DESTINATION of the head agent of src(e)]) - time_travel(dst(e)))

The reference computes every term of the prior in MPNNPolicyNet.forward (src/agents/mpnn_agent.py:180-187) and leaves the
sum commented out (:188). ``restated_logits`` below is those lines with the add uncommented (and the weight, and the
documented sentinel for unreachable pairs), on the CPU; the kernels must equal it bit for bit."""
import os

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
UNREACHABLE = -1e20


def restated_logits(obs16, edge_index, dist, emb, w=1.0):
    """src/agents/mpnn_agent.py:166-190 on observations x = cat(node_features, agent_features[agent_index]) (M, N, 16),
    with ``logits + w * logits_dijkstra`` returned. Differentiable in ``emb``."""
    M, N, _ = obs16.shape
    E = edge_index.size(1)
    x = obs16.reshape(-1, 16)
    inc = (torch.arange(M).repeat_interleave(E) * N).repeat(2, 1)
    ei = edge_index.repeat(1, M) + inc                                         # the batched graph (:160-164)
    road = x[:, 6][ei[1]].to(torch.long)
    ok = (road >= 0) & (road < emb.numel())
    logits = torch.where(ok, emb.reshape(-1)[road.clamp(0, emb.numel() - 1)], torch.zeros(()))   # update_edges (:215-217)
    x_j = x[ei[1]]
    critical_number = x_j[:, 4] * x_j[:, 2] / 3600                                               # :182
    time_congestion = x_j[:, 2] * (x_j[:, 0] + 10 - critical_number) / (x_j[:, 0] + 10 - x_j[:, 1])   # :183
    time_travel = torch.max(torch.stack((x_j[:, 2], time_congestion)), dim=0).values             # :184
    dest = x[:, 8].to(torch.long)[ei[0]]                                                          # :186-187
    valid = (dest >= 0) & (dest < N)
    d = dist[edge_index[1].repeat(M), dest.clamp(0, N - 1)]                                       # compute_dijkstra_logits
    d = torch.where(valid, d, torch.full_like(d, float("inf")))
    prior = -d - time_travel
    prior = torch.where(torch.isinf(d), torch.full_like(prior, UNREACHABLE), w * prior)
    return (logits + prior).view(M, E)


def _net(W=5, H=4, seed=2):
    from tarl_hip import synth
    return synth.torus_network(W, H, heterogeneous=True, seed=seed)


def _table(net):
    from tarl_hip import ops
    N = net.num_roads
    plan = ops.Plan(net.edge_index, N)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda()
    return plan, ops.all_pairs_shortest_paths(plan, ff, want_next_hop=False, want_dist=True)[1][0]


def _random_obs(net, M, seed):
    """Observations with real counts and head agents: static columns of the network, NUMBER_OF_AGENT in [0, MAXN],
    agent rows with destinations in [0, N)."""
    g = torch.Generator().manual_seed(seed)
    N, Nmax = net.num_roads, net.Nmax
    nf = net.x[:, 3 * Nmax:3 * Nmax + 7].clone().unsqueeze(0).repeat(M, 1, 1)
    nf[..., 1] = torch.floor(torch.rand((M, N), generator=g) * (nf[..., 0] + 1))
    ag = torch.rand((M, N, 9), generator=g) * 100
    ag[..., 1] = torch.randint(0, N, (M, N), generator=g).float()
    return torch.cat((nf, ag), dim=-1).contiguous()


def test_observation_kernel_reproduces_the_reference_prior_golden():
    """emb = 0, prior_weight = 1, zero counts (time_travel = FREE_FLOW of the target road = torus__ff_edges): the
    observation-side kernel reproduces routing.npz:torus__prior_logits exactly. The golden draws one destination per EDGE;
    the kernel reads one per source road, so observation row r carries, at every road, the destination of its r-th
    out-edge and edge e is read from the row of its rank."""
    from tarl_hip import ops, synth
    g = load_golden("routing")
    net = synth.torus_network(3, 3, heterogeneous=True, seed=21)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    plan = ops.Plan(net.edge_index, N)
    src = net.edge_index[0]
    order = torch.argsort(src, stable=True)
    rank = torch.empty(E, dtype=torch.long)
    ptr = torch.zeros(N + 1, dtype=torch.long)
    ptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    rank[order] = torch.arange(E) - ptr[src[order]]
    R = int(rank.max()) + 1
    obs = torch.zeros((R, N, 16))
    obs[:, :, :7] = net.x[:, 3 * Nmax:3 * Nmax + 7]
    obs[:, :, 1] = 0
    obs[rank, src, 8] = g["torus__prior_dest"].float()
    table = g["torus__dist_matrix"].cuda()
    emb = torch.zeros(N, device="cuda")
    out = ops.policy_prior_logits(plan, obs.cuda(), emb, table, 1.0).cpu()
    got = out[rank, torch.arange(E)]
    assert torch.equal(got, g["torus__prior_logits"])
    assert torch.equal(out, restated_logits(obs, net.edge_index, g["torus__dist_matrix"], emb.cpu()))


@pytest.mark.parametrize("M,w", [(1, 1.0), (1, 0.37), (64, 1.0), (64, 0.37)])
def test_observation_kernel_equals_the_restatement_with_real_counts(M, w):
    from tarl_hip import ops
    net = _net()
    plan, table = _table(net)
    N = net.num_roads
    obs = _random_obs(net, M, seed=M + int(100 * w))
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3))
    out = ops.policy_prior_logits(plan, obs.cuda(), emb.cuda(), table, w).cpu()
    ref = restated_logits(obs, net.edge_index, table.cpu(), emb, w)
    assert torch.equal(out, ref)
    assert float(obs[..., 1].max()) > 0                    # the congested branch of time_travel is exercised
    if w == 1.0:     # the reference's literal sum: embedding + compute_dijkstra_logits
        from src.agents.mpnn_agent import MPNNPolicyNet
        pol = MPNNPolicyNet(net.edge_index.cuda(), N, net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda(), device="cuda")
        x = obs.reshape(-1, 16)
        E = net.edge_index.size(1)
        inc = (torch.arange(M).repeat_interleave(E) * N).repeat(2, 1)
        ei = net.edge_index.repeat(1, M) + inc
        x_j = x[ei[1]]
        crit = x_j[:, 4] * x_j[:, 2] / 3600
        tc = x_j[:, 2] * (x_j[:, 0] + 10 - crit) / (x_j[:, 0] + 10 - x_j[:, 1])
        tt = torch.max(torch.stack((x_j[:, 2], tc)), dim=0).values
        dij = pol.compute_dijkstra_logits(x[:, 8].long()[ei[0]].cuda(), tt.cuda()).cpu().reshape(M, E)
        assert torch.equal(out, emb[x[:, 6].long()[ei[1]]].view(M, E) + dij)


@pytest.mark.parametrize("w", [1.0, 0.37])
def test_fused_state_kernel_equals_the_observation_kernel(w):
    """After a few frames of the live policy (queues, head agents, empty rows), the packed-state kernel produces the same
    logits as the observation kernel on the packed state's observation."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = _net(6, 5, seed=4)
    N, B = net.num_roads, 70
    plan, table = _table(net)
    pops = torch.stack([synth.population(300, N, seed=b, t0=21540, t1=21560) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=5)
    eng.reset()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(1)).cuda()
    eng.prepare_policy(emb)
    for _ in range(12):
        eng.frame_fused()
    obs = ops.fused_obs16(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents)
    assert float(obs[..., 1].sum()) > 0 and float((obs[..., 1] == 0).float().mean()) > 0.05
    a = ops.policy_prior_logits(eng.plan, obs, emb, table, w)
    b = ops.fused_prior_logits(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents, emb, table, w)
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), restated_logits(obs.cpu(), net.edge_index, table.cpu(), emb.cpu(), w))


def test_module_forward_and_embedding_gradient():
    from tarl_hip import synth
    from src.agents.mpnn_agent import MPNNPolicyNet
    net = _net()
    N, M, Nmax = net.num_roads, 6, net.Nmax
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]]
    torch.manual_seed(0)
    pol = MPNNPolicyNet(net.edge_index.cuda(), N, ff.cuda(), device="cuda")
    pol.policy_head = "embedding_dijkstra"
    pol.prior_weight = 0.37
    A = 50
    pop = synth.population(A, N, seed=3)
    pol.agent_features = pop.cuda()
    obs = _random_obs(net, M, seed=9)
    aidx = torch.randint(0, A + 5, (M, N), generator=torch.Generator().manual_seed(2))    # some ids out of range -> agent 0
    nf = obs[..., :7].contiguous()
    x16 = torch.cat((nf, pop[torch.where(aidx < pop.size(0), aidx, torch.zeros_like(aidx))]), dim=-1)
    logits = pol(nf.cuda(), torch.zeros((M, net.edge_index.size(1), 1), device="cuda"), aidx.cuda())
    emb = pol.nodes_embedding.weight.detach().cpu().clone().requires_grad_(True)
    ref = restated_logits(x16, net.edge_index, pol.dist_matrix.cpu(), emb, 0.37)
    assert torch.equal(logits.detach().cpu(), ref.detach())
    coef = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))
    (logits * coef.cuda()).sum().backward()
    (ref * coef).sum().backward()
    assert float((pol.nodes_embedding.weight.grad.cpu() - emb.grad).abs().max()) <= 1e-5 * max(1.0, float(emb.grad.abs().max()))
    l1 = pol(nf[0].cuda(), torch.zeros((net.edge_index.size(1), 1), device="cuda"), aidx[0].cuda())
    assert l1.shape == (net.edge_index.size(1),) and torch.equal(l1.detach(), logits[0].detach())
    assert set(pol.state_dict().keys()) == set(MPNNPolicyNet(net.edge_index.cuda(), N, ff.cuda(), "cuda").state_dict().keys())


def test_unreachable_candidates_and_all_unreachable_nodes():
    """Roads 0 -> 1 -> 2 -> 0 and two DEST pseudo-nodes 3, 4 without out-edges; node 5 leads to DEST nodes only.
    Node 0 (head agent bound for 4) chooses between road 1 (reaches 4) and DEST 3 (dead end): probability exactly 0 for
    DEST 3, as in the reference. Node 5 (head agent bound for road 1): both candidates unreachable — the reference's softmax
    is NaN there; here it draws uniformly. Nothing non-finite anywhere."""
    from tarl_hip import ops
    ei = torch.tensor([[0, 1, 2, 0, 1, 2, 5, 5], [1, 2, 0, 3, 4, 3, 3, 4]])
    N, E = 6, ei.size(1)
    plan = ops.Plan(ei, N)
    ff = torch.tensor([5.0, 7.0, 11.0, 0.0, 0.0, 2.0])
    table = ops.all_pairs_shortest_paths(plan, ff[ei[1]].cuda(), want_next_hop=False, want_dist=True)[1][0]
    assert torch.isinf(table[3, 4]) and torch.isinf(table[3, 1]) and torch.isfinite(table[1, 4])
    obs = torch.zeros((2, N, 16))
    obs[:, :, 0] = torch.tensor([10.0, 10, 10, 0, 0, 0])                    # MAX_NUMBER_OF_AGENT
    obs[:, :, 2] = ff
    obs[:, :, 4] = 1800.0
    obs[:, :, 6] = torch.tensor([0.0, 1, 2, -1, -1, -1])                    # ROAD_INDEX (-1 on pseudo-nodes)
    obs[1, :, 1] = torch.tensor([3.0, 9, 1, 0, 0, 0])
    obs[:, 0, 8] = 4.0
    obs[:, 1, 8] = 4.0
    obs[:, 2, 8] = 3.0
    obs[:, 5, 8] = 1.0
    emb = torch.tensor([0.5, -0.25, 2.0], device="cuda", requires_grad=False)
    for w in (1.0, 0.37, 0.0):
        logits = ops.policy_prior_logits(plan, obs.cuda(), emb, table, w)
        assert bool(torch.isfinite(logits).all())
        assert torch.equal(logits.cpu(), restated_logits(obs, ei, table.cpu(), emb.cpu(), w))
        p = ops.graphdist_softmax(plan, logits)
        assert bool(torch.isfinite(p).all())
        assert bool((p[:, 3] == 0).all()) and bool((p[:, 0] == 1).all())            # node 0: DEST 3 is a dead end
        assert bool((p[:, 6] == 0.5).all()) and bool((p[:, 7] == 0.5).all())        # node 5: uniform
        for u in (0.0, 0.49, 0.51, 0.999999):
            onehot, choice = ops.graphdist_sample(plan, p, uniform=torch.full((2, plan.num_groups), u, device="cuda"),
                                                  want_choice=True)
            assert bool((choice[:, 0] == 0).all())
            assert bool((choice[:, 5] == (6 if u < 0.5 else 7)).all())
            lp, ent = ops.graphdist_logprob_entropy(plan, p, choice=choice)
            assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(ent).all())
            g = ops.graphdist_logprob_entropy_bwd(plan, p, 1.0, choice=choice, grad_log_prob=torch.ones(2, device="cuda"),
                                                  grad_entropy=torch.ones(2, device="cuda"), log_prob_fwd=lp)
            ge = ops.policy_edge_logits_bwd(plan, obs.cuda(), g, 3)
            assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(ge).all())


@pytest.mark.parametrize("t1", [21560, 21740])
def test_rollout_prior_equals_the_frames_issued_one_at_a_time(t1):
    """tarl_fused_rollout_prior over T frames == per frame: packed-state logits, tarl_graphdist_rollout (sel8), the frame.
    Departures in 21540 .. t1: about 20 agents due per frame and environment (the rollout's insert runs one environment per
    wave, like the twin's frames), or about 2 (tarl_insert_envs_per_wave packs 4 environments per wave; the twin still 1)."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = _net(6, 5, seed=7)
    N, B, T, A = net.num_roads, 96, 20, 400
    _, table = _table(net)
    pops = torch.stack([synth.population(A, N, seed=b, t0=21540, t1=t1) for b in range(B)]).cuda()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    mk = lambda: SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                           pops.clone(), congestion_constant=net.congestion_constant, seed=11)
    e1, e2 = mk(), mk()
    e1.reset()
    e2.reset()
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    P = 3
    keep = (list(range(0, (T + 1) * P, P)), torch.tensor([0, 50, B - 1] * T, dtype=torch.int32, device="cuda"),
            torch.arange(T * P, dtype=torch.int32, device="cuda"))
    obs_keep = torch.full((T * P, N, 16), float("nan"), device="cuda")
    e1.rollout_prior(T, emb, table, prior_weight=0.37, temperature=1.5, policy_seed=77, policy_counter0=5, choice8=ch,
                     log_prob=lp, reward=rw, counts=ct, keep=keep, obs_keep=obs_keep)
    counts_f = torch.zeros((N, B), device="cuda")
    for t in range(T):
        o = ops.fused_obs16(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents)
        assert torch.equal(o[[0, 50, B - 1]], obs_keep[t * P:(t + 1) * P]), t
        logits = ops.fused_prior_logits(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents, emb, table, 0.37)
        c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        lp2 = ops.graphdist_rollout(e2.plan, logits, 1.5, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
        e2.frame_fused(skip_choice=True, counts=counts_f)
        assert torch.equal(c8, ch[t]) and torch.equal(lp2, lp[t]), t
        assert torch.equal(counts_f, ct[t + 1].float()) and torch.equal(e2.reward, rw[t]), t
    assert float(rw.abs().sum()) > 0 and float(ct[-1].float().sum()) > 0
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)


def test_rollout_prior_oracle_replay_config4():
    """Config 4 (25 x 25 torus, 16 384 agents), B = 1 024, 32 frames of tarl_fused_rollout_prior next to the ORACLE: for
    probe environments every frame's observation is rebuilt from the oracle's own state and must equal the device's;
    the prior logits are restated on the CPU from it (bit-exact against the device kernel on the same observation); the
    device's action bytes are checked against GraphDist.sample with the exported uniforms (a draw may differ only where
    the uniform lies within 2 fp32 ulps of a CDF boundary: the device and the oracle round the boundary separately); then
    oracle/sim.env_step advances with the device's action and Gumbel values: counts and rewards of every frame, final x and
    agents bit-exact."""
    from draw_check import CARRIED, fp32_ulp, ranks
    from oracle import dist, sim
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START, SimEngine
    A, T, B, TEMP, W = 16384, 32, 1024, 1.0, 1.0
    probe = [0, 333, 1023]
    P = len(probe)
    net = synth.torus_network(25, 25)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    pops = synth.population_batch(A, N, B, seed=21, device="cuda", t1=EPISODE_START + 40)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, Nmax,
                    pops.clone(), congestion_constant=net.congestion_constant, seed=29)
    eng.reset()
    plan, table = _table(net)
    emb = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(8))).cuda()
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    keep = (list(range(0, (T + 1) * P, P)), torch.tensor(probe * T, dtype=torch.int32, device="cuda"),
            torch.arange(T * P, dtype=torch.int32, device="cuda"))
    obs_keep = torch.full((T * P, N, 16), float("nan"), device="cuda")
    noise0 = eng.noise_counter + 1
    eng.rollout_prior(T, emb, table, prior_weight=W, temperature=TEMP, policy_seed=77, policy_counter0=5, choice8=ch,
                      log_prob=lp, reward=rw, counts=ct, keep=keep, obs_keep=obs_keep)
    eng.check_flags()
    assert float(-rw[-1].mean()) > 100
    dev_logits = ops.policy_prior_logits(plan, obs_keep, emb, table, W).cpu()
    pidx = torch.tensor(probe, device="cuda")
    ch_p, ct_p, lp_p, rw_p = ch[:, pidx].cpu(), ct[:, :, pidx].cpu(), lp[:, pidx].cpu(), rw[:, pidx].cpu()
    obs_p = obs_keep.cpu()
    x_fin = torch.stack([eng.x[b] for b in probe]).cpu()
    ag_fin = torch.stack([eng.agents[b] for b in probe]).cpu()
    table_c, emb_c = table.cpu(), emb.cpu()
    src = net.edge_index[0]
    out_eid = torch.argsort(src, stable=True)
    out_ptr = torch.zeros(N + 1, dtype=torch.long)
    out_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    deg = out_ptr[1:] - out_ptr[:-1]
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    flips = draws = 0
    for k, b in enumerate(probe):
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pops[b].cpu().clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        for t in range(T):
            clock = float(EPISODE_START + t)
            nf, head = sim.observe(x, Nmax)
            x16 = torch.cat((nf, ag[head.clamp(0, A)]), dim=-1)
            assert torch.equal(obs_p[t * P + k], x16), f"observation of environment {b}, frame {t}"
            logits = restated_logits(x16.unsqueeze(0), net.edge_index, table_c, emb_c, W)[0]
            assert torch.equal(logits, dev_logits[t * P + k]), f"logits of environment {b}, frame {t}"
            gd = dist.GraphDist(logits, net.edge_index, TEMP)
            u = ops.noise_export(eng.plan, "uniform", 77, 5 + t, [b])[0].cpu()
            code = ch_p[t, k].long()
            r_dev = torch.where((code & CARRIED) != 0, deg, code)
            cs = gd.cumsum.detach().to(torch.float32)
            r_or = ranks(u, cs, out_ptr)
            ulp = fp32_ulp(torch.cumsum(gd.proba_sort.detach(), dim=-1))
            for i in torch.nonzero(r_or != r_dev).flatten().tolist():
                lo, hi = sorted((int(r_or[i]), int(r_dev[i])))
                q = torch.arange(int(out_ptr[i]) + lo, int(out_ptr[i]) + hi)
                assert bool(((u[i].double() - cs[q].double()).abs() <= 2 * ulp[q]).all()), (b, t, i)
                flips += 1
            draws += N
            drew = (code & CARRIED) == 0
            action = torch.zeros(E, dtype=torch.long)
            action[out_eid[out_ptr[:-1][drew] + code[drew]]] = 1
            lp_o = float(gd.log_prob(action))
            if bool(drew.all()):
                assert abs(float(lp_p[t, k]) - lp_o) <= 1e-4 * max(1.0, abs(lp_o)), (b, t, float(lp_p[t, k]), lp_o)
            g = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
            out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, clock, Nmax, gumbel=g,
                               congestion_constant=net.congestion_constant)
            assert torch.equal(x[:, c.N], ct_p[t + 1, :, k].float()), f"counts of environment {b} after frame {t}"
            assert float(out["reward"]) == float(rw_p[t, k]), f"reward of environment {b}, frame {t}"
        assert torch.equal(x, x_fin[k]), f"final state of environment {b}"
        assert torch.equal(ag, ag_fin[k]), f"agent table of environment {b}"
    assert flips <= draws * 1e-3


def _trainer(net, B, T, M, w, seed=0):
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    N = net.num_roads
    pops = torch.stack([synth.population(300, N, seed=b, t0=21540, t1=21555) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=3)
    torch.manual_seed(seed)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")],
                       policy="embedding_dijkstra", prior_table=pol.dist_matrix, prior_weight=w)
    return tr, eng, pol, crit


def test_trainer_refuses_the_unfused_engine():
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = _net()
    N = net.num_roads
    from tarl_hip import synth
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(2, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    torch.stack([synth.population(20, N, seed=b) for b in range(2)]).cuda(), fused=False)
    emb = torch.nn.Parameter(torch.zeros(N, 1, device="cuda"))
    with pytest.raises(ValueError, match="embedding_dijkstra"):
        VecPPOTrainer(eng, emb, [], rollout_steps=4, policy="embedding_dijkstra", prior_table=torch.zeros(N, N, device="cuda"))


@pytest.mark.parametrize("w", [1.0, 0.37])
def test_ppo_update_matches_oracle_autograd(w):
    """mode frames+prior: the first minibatch's recomputed log-probs equal the rollout's bit for bit (same logits), and one
    update (losses, gradients, Adam) equals the oracle's CPU autograd over the restated prior within 1e-4."""
    from oracle import dist, nets, ppo
    from tarl_hip import ops
    net = _net(4, 4, seed=2)
    N, E, B, T, M = net.num_roads, net.edge_index.size(1), 128, 24, 16
    tr, eng, pol, crit = _trainer(net, B, T, M, w)
    assert tr.rollout == "frames+prior"
    tr.keep_grad = True
    idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(4))[:M]
    tr.obs_idx = idx
    tr.collect()
    emb0 = pol.nodes_embedding.weight.detach().cpu().clone()
    crit0 = [p.detach().cpu().clone() for p in crit]
    table = pol.dist_matrix
    choice = eng.decode_rollout(False, choice=tr.choice)[0].cpu()          # action bytes: env-major (T, B, N)
    counts = eng.decode_rollout(True, counts=tr.counts)[1].cpu()          # count bytes: env-minor (T + 1, N, B)
    reward, times = tr.reward.cpu(), tr.times.cpu()
    assert float(reward.abs().sum()) > 0
    obs_mb = tr.obs_mb.cpu()
    t_idx, b_idx = idx // B, idx % B
    assert torch.equal(obs_mb[:, :, 1], counts[t_idx, b_idx])                 # kept observations = the frames drawn
    # the update's recomputed behaviour log-prob == the rollout's, bit for bit
    lg = ops.policy_prior_logits(eng.plan, tr.obs_mb, emb0.reshape(-1).cuda(), table, w)
    ch_mb, _ = ops.rollout_gather(eng.plan, T, B, False, idx.cuda(), choice=tr.choice)
    lp_re, _ = ops.graphdist_logprob_entropy(eng.plan, ops.graphdist_softmax(eng.plan, lg, tr.temperature), choice=ch_mb)
    assert torch.equal(lp_re, tr.logp.view(-1)[idx.cuda()])
    adv_g, tgt_g = tr.advantages()
    out = tr.minibatch_step(adv_g, tgt_g)
    # oracle
    emb = emb0.clone().requires_grad_(True)
    cw = [p.clone().requires_grad_(True) for p in crit0]
    nf_all = torch.zeros((T + 1, B, N, 7))
    nf_all[..., 1] = counts
    with torch.no_grad():
        v_all = nets.critic_value(nf_all, times.view(T + 1, 1, 1).expand(T + 1, B, 1), *cw).squeeze(-1)
        dmask = tr.done_frames.view(T, 1).expand(T, B)
        adv, tgt = ppo.gae(reward, v_all[:T], v_all[1:], dmask, dmask, average_gae=True)
    onehot = torch.zeros((M, E), dtype=torch.int64)
    onehot.scatter_(1, choice[t_idx, b_idx].long(), 1)
    with torch.no_grad():
        lp_old = dist.GraphDist(restated_logits(obs_mb, net.edge_index, table.cpu(), emb0, w), net.edge_index).log_prob(onehot)
    tol = lambda a, b_: float((a - b_).abs().max()) <= 1e-4 * max(1.0, float(b_.abs().max()))
    assert tol(tr.logp.view(-1).cpu()[idx], lp_old)
    d = dist.GraphDist(restated_logits(obs_mb, net.edge_index, table.cpu(), emb, w), net.edge_index)
    lp_new, ent = d.log_prob(onehot), d.entropy()
    value = nets.critic_value(nf_all[t_idx, b_idx], times[t_idx].view(M, 1), *cw).squeeze(-1)
    losses = ppo.clip_ppo_loss(lp_new, lp_old, adv.view(-1)[idx], value, tgt.view(-1)[idx], ent)
    (losses["loss_objective"] + losses["loss_critic"] + losses["loss_entropy"]).backward()
    o = out.cpu()
    for i, k in enumerate(["loss_objective", "loss_critic", "loss_entropy"]):
        assert abs(o[i].item() - losses[k].item()) <= 1e-4 * max(1.0, abs(losses[k].item())), k
    g = tr.last_grad.cpu()
    off = 0
    for name, ref in [("emb", emb.grad)] + [(f"critic{i}", c_.grad) for i, c_ in enumerate(cw)]:
        n = ref.numel()
        assert tol(g[off:off + n], ref.reshape(-1)), f"grad {name}"
        off += n
    assert float(g[off:].abs().sum()) == 0.0
    assert float(emb.grad.abs().sum()) > 0
    for p_gpu, p0, gr, name in [(pol.nodes_embedding.weight, emb0, emb.grad, "emb")] + \
            [(crit[i], crit0[i], cw[i].grad, f"critic{i}") for i in range(6)]:
        q = p0.clone()
        ppo.adam_step(q, gr, torch.zeros_like(q), torch.zeros_like(q), 1)
        assert tol(p_gpu.detach().cpu(), q), f"param {name}"


def test_cli_trains_and_evaluates_the_prior_head(tmp_path, monkeypatch, capsys):
    """`main.py --algo mpnn+ppo --policy-head embedding_dijkstra` trains and writes a checkpoint with the reference's keys;
    `--algo mpnn --mode eval --policy-head embedding_dijkstra` runs on a MATSim grid with SRC/DEST pseudo-nodes."""
    import importlib
    import sys
    from conftest import PKG
    sys.path.insert(0, PKG)
    from tarl_hip import synth
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
          "--epochs", "2", "--steps", "6", "--num-envs", "4", "--policy-head", "embedding_dijkstra", "--prior-weight", "0.5",
          "--output-dir", str(tmp_path / "run"), "--seed", "1"])
    assert "Simulation Summary" in capsys.readouterr().out
    r = created[-1]
    assert r.policy_net.policy_head == "embedding_dijkstra" and r.policy_net.prior_weight == 0.5
    from src.rl.ppo_trainer import ppo_train
    assert ppo_train.last_trainer.rollout == "frames+prior"
    ckpt = torch.load(tmp_path / "run" / "policy.pt", map_location="cpu")       # the reference's keys, no prior table
    ref_keys = set(r.policy_net.state_dict().keys())
    assert "module.0.module.nodes_embedding.weight" in ckpt
    assert {k.split("module.")[-1] for k in ckpt} == ref_keys
    torch.manual_seed(1)
    from src.agents.mpnn_agent import MPNNPolicyNet
    fresh = MPNNPolicyNet(r.policy_net.edge_index, r.policy_net.num_nodes, None, device="cuda")
    assert not torch.equal(fresh.nodes_embedding.weight, r.policy_net.nodes_embedding.weight)     # the embedding trained
    # eval on a MATSim grid (SRC / DEST pseudo-nodes: DEST nodes have no out-edges, unreachable pairs are common)
    os.makedirs("data/grid")
    synth.write_matsim_grid_xml("data/grid/network.xml", 4, 6, seed=3)
    synth.write_matsim_population_xml("data/grid/population.xml", 4, 6, 120, seed=4, first_departure=21600, spread=30)
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "grid", "--start-end-time", "21600", "21660",
          "--policy-head", "embedding_dijkstra", "--output-dir", str(tmp_path / "runs")])
    assert "Simulation Summary" in capsys.readouterr().out
    pol = created[-1].policy_net
    assert pol.policy_head == "embedding_dijkstra" and bool(torch.isinf(pol.dist_matrix).any())
