"""GPU: the goal-conditioned policy head (policy_head = "goal_mlp", csrc/goal_mlp.hip) — the features and the logits from
observations bit for bit against the fp32 restatement (``goal_mlp_restatement``; the torus and both irregular graphs, after a
reset and after 40 live frames of the holding router, M in {1, 3, 64, 65}, both table kinds, outputs between guard bands),
the logits from the packed state against the logits from that state's observations (crafted DIRTY rows, the 126-hub's list
across tile boundaries), the backward against float64 within the project's tolerance rule (deterministic, accumulating,
scratch from NaN), the one-call rollout against its launches queued one by one, and the refusals."""
import functools

import numpy as np
import pytest
import torch

import bc_restatement as BC
import goal_mlp_restatement as G
from update_restatement import tensor_bound

pytestmark = pytest.mark.gpu
GRAPHS = ("torus", "MIXED", "HUB126")
SIZES = (1, 3, 64, 65)
KMAX = 65


def _net(name):
    import irregular_graphs as ig
    from tarl_hip import synth
    return synth.torus_network(8, 8) if name == "torus" else ig.graph(name)


def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


@functools.lru_cache(maxsize=None)
def _graph_case(name):
    """Per graph, computed once: the plan, the device's all-pairs free-flow table, the time scale, and the observations of
    KMAX environments after a reset and after 40 frames of the holding router (agents bound for roads all over the graph)."""
    import irregular_graphs as ig
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _net(name)
    N, Nmax = net.num_roads, net.Nmax
    _, dout = ig.degrees(net)
    leads_on = torch.nonzero(dout > 0).view(-1)
    pop = synth.population(300 if name == "HUB126" else 500, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 30)
    pop[:, 0] = leads_on[pop[:, 0].long() % leads_on.numel()].float()      # nobody starts on a dead end
    ev = VecEvaluator(_engine(net, pop, KMAX), "dijkstra_hold")
    eng = ev.eng
    eng.reset()
    obs_reset = ops.fused_obs16(eng.plan, eng.fs, eng._x, Nmax, eng.agents).clone()
    res = ev.run(40)
    assert not res.domain_exit
    obs_live = ops.fused_obs16(eng.plan, eng.fs, eng._x, Nmax, eng.agents).clone()
    assert float((obs_live[..., 1] > 0).float().mean()) > 0.02 and float((obs_live[..., 1] == 0).float().mean()) > 0.02
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]].cuda().contiguous()
    table = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0].contiguous()
    S = ops.goal_time_scale(net.x[:, 3 * Nmax:])
    assert S == float(G.free_flow_table(net)[1])
    return dict(net=net, ei=net.edge_index.numpy(), plan=eng.plan, eng=eng, table=table, table_np=table.cpu().numpy(), S=S,
                reset=obs_reset, live=obs_live)


def _tables(c, obs_np, kind, drop=()):
    """(device table, device slot or None, host table, host slot or None)"""
    if kind == "all_pairs":
        return c["table"], None, c["table_np"], None
    tab, slot = G.per_destination(c["table_np"], obs_np, drop)
    return torch.tensor(tab).cuda(), torch.tensor(slot).cuda(), tab, slot


def _guarded(shape, pad=64):
    big = torch.full((int(np.prod(shape)) + 2 * pad,), float("nan"), device="cuda")
    return big, big[pad:pad + int(np.prod(shape))].view(shape), pad


def _guards_intact(big, pad):
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all())


def _weights(seed, sharp=False):
    from tarl_hip import ops
    w = G.weights(seed, sharp)
    return w, ops.GoalMlpWeights(flat=torch.tensor(w).cuda())


# ---- 1. features and forward from observations ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all_pairs", "per_destination"])
@pytest.mark.parametrize("state", ["reset", "live"])
@pytest.mark.parametrize("name", GRAPHS)
def test_features_and_logits_equal_the_fp32_restatement(name, state, kind):
    from tarl_hip import ops
    c = _graph_case(name)
    E = c["ei"].shape[1]
    if name != "torus":
        assert E % 64 != 0
    for M in SIZES:
        obs = c[state][:M].contiguous()
        obs_np = obs.cpu().numpy()
        if state == "live":      # the crafted nodes: all candidates unreachable / exactly one reachable
            obs_np, tab_np, u0, u1 = G.craft(c["ei"], obs_np, c["table_np"])
            obs = torch.tensor(obs_np).cuda()
            cc = dict(c, table=torch.tensor(tab_np).cuda(), table_np=tab_np)
        else:
            cc = c
        N = c["net"].num_roads      # a destination without a column: one some head is bound for, not a crafted node's
        named = [d for d in np.unique(obs_np[..., 8].astype(np.int64)).tolist() if 0 <= d < N - 2]
        drop = tuple(named[-1:]) if kind == "per_destination" and len(named) > 1 else ()
        tab, slot, tab_np, slot_np = _tables(cc, obs_np, kind, drop)
        big, feats, pad = _guarded((M, E, 8))
        ops.policy_goal_features(c["plan"], obs, tab, c["S"], dest_slot=slot, out=feats)
        want, reach = f32 = G.features(obs_np, c["ei"], tab_np, c["S"], slot_np)
        f64 = G.features(obs_np, c["ei"], tab_np, c["S"], slot_np, np.float64)
        assert _guards_intact(big, pad)
        assert np.array_equal(feats.cpu().numpy(), want), (name, state, kind, M)
        for sharp in (False, True):
            w_np, w = _weights(5 + M, sharp)
            bigl, logits, pad = _guarded((M, E))
            ops.policy_goal_mlp(c["plan"], obs, w, tab, c["S"], dest_slot=slot, out=logits)
            l32 = G.forward(obs_np, c["ei"], tab_np, c["S"], w_np, slot_np, feats=f32)
            l64 = G.forward(obs_np, c["ei"], tab_np, c["S"], w_np, slot_np, dt=np.float64, feats=f64)
            got = logits.cpu().numpy()
            assert _guards_intact(bigl, pad) and np.isfinite(got).all()
            assert np.array_equal(got, l32), (name, state, kind, M, sharp)
            assert np.array_equal(got == G.UNREACHABLE, ~reach)                            # sentinels exactly where restated
            if reach.any():
                e32 = np.abs(l32[reach].astype(np.float64) - l64[reach]).max()
                assert np.abs(got[reach] - l64[reach]).max() <= tensor_bound(e32, torch.tensor(l64[reach]))
        if state == "live":
            assert (~reach[:, c["ei"][0] == u0]).all() and (reach[:, c["ei"][0] == u1].sum(1) == 1).all()
            p = ops.graphdist_softmax(c["plan"], logits.contiguous())
            sel = torch.tensor(c["ei"][0] == u1).cuda()
            assert bool((p[:, sel].sum(1) == 1).all()) and bool(((p[:, sel] == 0) | (p[:, sel] == 1)).all())
            deg0 = int((c["ei"][0] == u0).sum())
            assert bool((p[:, torch.tensor(c["ei"][0] == u0).cuda()] == 1.0 / deg0).all())  # uniform where all unreachable
        if drop:
            hit = obs_np[:, c["ei"][0], 8].astype(np.int64) == drop[0]
            assert hit.any() and (~reach[hit]).all()


# ---- 2. logits from the packed state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", GRAPHS)
def test_packed_state_logits_equal_the_observation_path(name, B):
    """``BC.crafted_labels``' packed state (queues, empty rows, a DIRTY empty row, the hubs' heads) and the live engine state:
    fused_goal_mlp_logits == policy_goal_mlp on fused_obs16 of the same state, random and sharp weights, both table kinds."""
    from tarl_hip import ops
    c = _graph_case(name)
    cr = BC.crafted_labels(name, B)
    N, Nmax, E = cr.N, cr.Nmax, c["ei"].shape[1]
    assert torch.equal(cr.net.edge_index, c["net"].edge_index) and Nmax == c["net"].Nmax
    plan = c["plan"]
    fs = ops.FusedState(plan, B, cr.ag.size(1), "cuda", Nmax)
    x, ag = cr.x.cuda(), cr.ag.cuda()
    ops.fused_pack(plan, fs, x, Nmax, ag, cr.net.congestion_constant.cuda(), ec=ops.EdgeConst(cr.net.edge_attr, "cuda"))
    fs.check_flags()
    assert bool(((fs.hdp[cr.rows["stale"], :, 0] & 0xFF) == 0x80).all())                    # DIRTY, empty
    eng = c["eng"]
    states = [(fs, x, ag)]
    if B == KMAX:
        states.append((eng.fs, eng._x, eng.agents))
    if name == "HUB126":      # the hub's 126 positions cross a tile boundary of 64 CSR positions
        order, ptr = G.csr(c["ei"], N)
        hub = int(np.argmax(np.diff(ptr)))
        assert ptr[hub] // 64 != (ptr[hub + 1] - 1) // 64 and ptr[hub + 1] - ptr[hub] == 126
    for fs_, x_, ag_ in states:
        obs = ops.fused_obs16(plan, fs_, x_, Nmax, ag_)
        obs_np = obs.cpu().numpy()
        for kind in ("all_pairs", "per_destination"):
            tab, slot, _, _ = _tables(c, obs_np, kind)
            for sharp in (False, True):
                _, w = _weights(11 + B, sharp)
                big, out, pad = _guarded((B, E))
                ops.fused_goal_mlp_logits(plan, fs_, x_, Nmax, ag_, w, tab, c["S"], dest_slot=slot, out=out)
                want = ops.policy_goal_mlp(plan, obs, w, tab, c["S"], dest_slot=slot)
                assert _guards_intact(big, pad)
                assert torch.equal(out, want), (name, B, kind, sharp)
                assert bool((out != G.UNREACHABLE).any())


# ---- 3. the backward -------------------------------------------------------------------------------------------------------------
def _bwd(ops, c, obs, w, tab, slot, gl, init=None, scratch=None):
    grads = torch.zeros(G.NW, device="cuda") if init is None else init.clone()
    ops.policy_goal_mlp_bwd(c["plan"], obs, w, tab, c["S"], gl, grads, dest_slot=slot, scratch=scratch)
    return grads


BWD_CASES = [(n, M) for n in ("torus", "MIXED") for M in SIZES] + [("HUB126", M) for M in (1, 3, 17)]


@pytest.mark.parametrize("name,M", BWD_CASES)
def test_backward_against_float64(name, M):
    """Random and one-hot ``grad_logits`` (first and last pair, both sides of the first partition's edge), live observations:
    within tensor_bound(relative_scale=True) of the float64 restatement; two runs bit-identical from a NaN-filled scratch; a
    call on non-zero buffers adds exactly what a call on zeros wrote; an unreachable pair's grad_logits (NaN here) is not
    read. Pairs with a pre-activation within 1e-5 of zero get grad_logits = 0: excluded from the case, not from the kernel.
    HUB126 (17 852 edges) takes M = 17 for the large case: more than 1 024 tiles of 256 pairs, so a partition owns two tiles
    (M = 64 and 65 there cost eight seconds of numpy each and take no other path)."""
    from tarl_hip import ops
    c = _graph_case(name)
    ei, E = c["ei"], c["ei"].shape[1]
    obs = c["live"][:M].contiguous()
    obs_np = obs.cpu().numpy()
    w_np, w = _weights(31 + M)
    need = ops.goal_mlp_bwd_scratch_floats(c["plan"], M)
    chunk = -(-(-(-M * E // 256)) // 1024) * 256                                           # pairs per partition
    assert need == -(-M * E // chunk) * G.NW
    kinds = ("all_pairs", "per_destination") if M * E < 300000 else (("all_pairs", "per_destination")[M % 2],)
    for kind in kinds:
        tab, slot, tab_np, slot_np = _tables(c, obs_np, kind)
        g64, reach = f64 = G.features(obs_np, ei, tab_np, c["S"], slot_np, np.float64)
        f32 = G.features(obs_np, ei, tab_np, c["S"], slot_np)
        near0 = (np.abs(G.hidden(g64, w_np, np.float64)) < 1e-5).any(-1)
        rng = np.random.default_rng(M)
        probes = [rng.standard_normal((M, E))]
        for pair in {0, M * E - 1, min(chunk, M * E) - 1, min(chunk, M * E - 1), 255 % (M * E), 256 % (M * E)}:
            one = np.zeros(M * E)
            one[pair] = 1.0
            probes.append(one.reshape(M, E))
        for i, gl in enumerate(probes):
            gl = np.where(near0, 0.0, gl).astype(np.float32)
            ref = G.backward(obs_np, ei, tab_np, c["S"], w_np, gl, slot_np, feats=f64)
            r32 = G.backward(obs_np, ei, tab_np, c["S"], w_np, gl, slot_np, dt=np.float32, feats=f32)
            gl_dev = torch.tensor(np.where(reach, gl, np.nan).astype(np.float32)).cuda()
            scratch = torch.full((need + 8,), float("nan"), device="cuda")
            a = _bwd(ops, c, obs, w, tab, slot, gl_dev, scratch=scratch)
            b = _bwd(ops, c, obs, w, tab, slot, gl_dev, scratch=torch.full((need,), float("nan"), device="cuda"))
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
            assert bool(torch.isnan(scratch[need:]).all()) and bool(torch.isfinite(scratch[:need]).all())
            bound = tensor_bound(np.abs(r32.astype(np.float64) - ref).max(), torch.tensor(ref), relative_scale=True)
            err = np.abs(a.cpu().numpy().astype(np.float64) - ref).max()
            print(f"[goal bwd {name} M={M} {kind} probe {i}] err {err:.3e} bound {bound:.3e} max|ref| {np.abs(ref).max():.3e}")
            assert err <= bound, (name, M, kind, i, err, bound)
            if i == 0:
                init = torch.tensor(rng.standard_normal(G.NW).astype(np.float32)).cuda()
                assert torch.equal(_bwd(ops, c, obs, w, tab, slot, gl_dev, init=init), init + a)     # accumulates (+=)


# ---- 4. the rollout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("B", [3, 65])
def test_rollout_goal_equals_its_launches_queued_one_by_one(B, hold):
    """tarl_fused_rollout_goal over T = 6 frames == per frame: packed-state logits, tarl_graphdist_rollout (sel8), [the hold
    rule], the frame — action bytes, log-probs, rewards, counts, kept observation rows, final state; both table kinds."""
    from src.agents.base import destination_set
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = synth.torus_network(6, 5, heterogeneous=True, seed=7)
    N, T, A, TEMP = net.num_roads, 6, 400, 1.5
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()
    pops = torch.stack([synth.population(A, N, seed=b, t0=21540, t1=21560) for b in range(B)]).cuda()
    mk = lambda: SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                           pops.clone(), congestion_constant=net.congestion_constant, seed=11)
    S = ops.goal_time_scale(net.x[:, 3 * net.Nmax:])
    _, w = _weights(3, sharp=True)
    outs = {}
    for kind in ("all_pairs", "per_destination"):
        e1, e2 = mk(), mk()
        e1.reset()
        e2.reset()
        if kind == "all_pairs":
            table, slot = ops.all_pairs_shortest_paths(e1.plan, ff, want_next_hop=False, want_dist=True)[1][0], None
        else:
            dests, slot = destination_set(e1.agents, N)
            table = ops.prior_dest_table(e1.plan, ff, dests)
        ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
        ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
        lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
        P = 2
        keep = (list(range(0, (T + 1) * P, P)), torch.tensor([0, B - 1] * T, dtype=torch.int32, device="cuda"),
                torch.arange(T * P, dtype=torch.int32, device="cuda"))
        obs_keep = torch.full((T * P, N, 16), float("nan"), device="cuda")
        held1, held2 = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        if hold:
            ops.fused_set_policy_hold(e1.fs, True, held1)
        e1.rollout_goal(T, w, table, S, slot, temperature=TEMP, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp,
                        reward=rw, counts=ct, keep=keep, obs_keep=obs_keep)
        if hold:
            ops.fused_set_policy_hold(e1.fs, False)
        counts_f = torch.zeros((N, B), device="cuda")
        for t in range(T):
            o = ops.fused_obs16(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents)
            assert torch.equal(o[[0, B - 1]], obs_keep[t * P:(t + 1) * P]), t
            logits = ops.fused_goal_mlp_logits(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents, w, table, S, dest_slot=slot)
            c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
            lp2 = ops.graphdist_rollout(e2.plan, logits, TEMP, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
            if hold:
                ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
            e2.frame_fused(skip_choice=True, counts=counts_f)
            assert torch.equal(c8, ch[t]) and torch.equal(lp2, lp[t]), t
            assert torch.equal(counts_f, ct[t + 1].float()) and torch.equal(e2.reward, rw[t]), t
        assert float(rw.abs().sum()) > 0 and float(ct[-1].float().sum()) > 0
        assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents) and torch.equal(held1, held2)
        outs[kind] = float(rw.sum())
    assert all(np.isfinite(v) for v in outs.values())


# ---- 5. refusals on the device ---------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from tarl_hip import lib, ops
    from tarl_hip.engine import SimEngine
    c = _graph_case("torus")
    net, plan, E = c["net"], c["plan"], c["ei"].shape[1]
    N = net.num_roads
    obs = c["live"][:3].contiguous()
    _, w = _weights(1)
    grads = torch.full((G.NW,), 7.0, device="cuda")
    gl = torch.ones((3, E), device="cuda")
    need = ops.goal_mlp_bwd_scratch_floats(plan, 3)
    short = torch.full((need - 1,), 3.0, device="cuda")
    with pytest.raises(ValueError, match=f"at least {need} elements"):
        ops.policy_goal_mlp_bwd(plan, obs, w, c["table"], c["S"], gl, grads, scratch=short)
    with pytest.raises(ValueError, match="all-pairs distance table"):
        ops.policy_goal_mlp_bwd(plan, obs, w, c["table"][:, :-1].contiguous(), c["S"], gl, grads)
    with pytest.raises(ValueError, match="per-destination"):
        ops.policy_goal_mlp(plan, obs, w, c["table"], c["S"], dest_slot=torch.zeros(N - 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="time_scale"):
        ops.policy_goal_features(plan, obs, c["table"], 0.0)
    with pytest.raises(ValueError, match="GoalMlpWeights"):
        ops.policy_goal_mlp(plan, obs, torch.zeros(G.NW, device="cuda"), c["table"], c["S"])
    out = torch.full((3, E), 5.0, device="cuda")
    rc = lib.load().tarl_policy_goal_mlp_fwd(plan.handle, obs.data_ptr(), 3, c["table"].data_ptr(), N - 1, None, c["S"],
                                             w.flat.data_ptr(), out.data_ptr(), None)
    assert rc == -1 and b"N x N" in lib.load().tarl_last_error()
    torch.cuda.synchronize()
    assert bool((grads == 7.0).all()) and bool((short == 3.0).all()) and bool((out == 5.0).all())
    # an engine on the per-op kernels has no packed state to roll out from
    plain = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, c["eng"].agents[0].clone(),
                      congestion_constant=net.congestion_constant, num_envs=2, seed=1, fused=False)
    with pytest.raises(ValueError, match="fused engine"):
        plain.rollout_goal(2, w, c["table"], c["S"], temperature=1.0, policy_seed=1, policy_counter0=1, choice8=None,
                           log_prob=None, reward=None, counts=None)


# ---- 6. the module and the trainer ------------------------------------------------------------------------------------------------
def _free_flow(net):
    return net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()


def _policy(net, method="all_pairs", seed=1):
    from src.agents.mpnn_agent import MPNNPolicyNet
    from tarl_hip import ops
    torch.manual_seed(seed)
    pol = MPNNPolicyNet(net.edge_index, net.num_roads, _free_flow(net), device="cuda")
    before = set(pol.state_dict())
    pol.prior_method = method
    pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * net.Nmax:]))
    assert set(pol.state_dict()) - before == set(ops.GOAL_MLP_KEYS) | {"goal_scale"}
    return pol


def test_module_forward_and_backward_are_the_ops():
    """MPNNPolicyNet.use_goal_mlp(): forward == ops.policy_goal_mlp on policy_obs16, autograd == ops.policy_goal_mlp_bwd
    cut into the four parameters; per_destination gives the same bits; U(-0.1, 0.1) weights and zero bias."""
    from tarl_hip import ops, synth
    net = synth.torus_network(5, 4, heterogeneous=True, seed=3)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    nf = net.x[:, 3 * Nmax:3 * Nmax + 7].cuda().unsqueeze(0).repeat(3, 1, 1).contiguous()
    nf[..., 1] = torch.randint(0, 3, (3, N), generator=torch.Generator().manual_seed(1)).float().cuda()
    idx = torch.randint(0, 201, (3, N), generator=torch.Generator().manual_seed(2)).cuda()
    ef = torch.zeros((3, E, 1), device="cuda")
    coef = torch.randn((3, E), generator=torch.Generator().manual_seed(3)).cuda()
    outs = {}
    for method in ("all_pairs", "per_destination"):
        pol = _policy(net, method)
        m = pol.goal_mlp
        assert float(m[0].weight.detach().abs().max()) <= 0.1 and not bool(m[0].bias.any()) and not bool(m[2].bias.any())
        with torch.no_grad():
            m[0].bias.uniform_(-0.3, 0.3)
        pol.agent_features = synth.population(200, N, seed=4).cuda()
        logits = pol(nf, ef, idx)
        (logits * coef).sum().backward()
        table, slot = pol.prior_tables()
        obs = ops.policy_obs16(nf, idx, pol.agent_features)
        w = ops.GoalMlpWeights(*(p.data for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)))
        assert torch.equal(logits.detach(), ops.policy_goal_mlp(pol_plan(pol), obs, w, table, float(pol.goal_scale), dest_slot=slot))
        flat = torch.zeros(ops.GOAL_MLP_PARAMS, device="cuda")
        ops.policy_goal_mlp_bwd(pol_plan(pol), obs, w, table, float(pol.goal_scale), coef, flat, dest_slot=slot)
        got = torch.cat([p.grad.reshape(-1) for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)])
        assert torch.equal(got, flat) and bool(flat.any())
        assert pol(nf[0], ef[0], idx[0]).shape == (E,)
        outs[method] = (logits.detach().clone(), got)
    assert torch.equal(outs["all_pairs"][0], outs["per_destination"][0])
    assert torch.equal(outs["all_pairs"][1], outs["per_destination"][1])


def pol_plan(pol):
    from src._compat import cached_plan
    return cached_plan(pol.edge_index, pol.num_nodes)


def _trainer_case(hold):
    """A 5 x 4 torus, B = 96, 200 agents, T = 14 -> (trainer on engine 1, twin engine 2, the policy, TEMP)."""
    from src.agents.mpnn_agent import MPNNValueNetSimple
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(5, 4, heterogeneous=True, seed=3)
    N = net.num_roads
    B, A, T, M, TEMP = 96, 200, 14, 20, 2.0
    pops = torch.stack([synth.population(A, N, seed=40 + b, t0=21540, t1=21552) for b in range(B)])

    def engine():
        return SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                         pops.clone().cuda(), congestion_constant=net.congestion_constant, seed=9)
    pol = _policy(net)
    with torch.no_grad():
        pol.goal_mlp[0].bias.uniform_(-0.3, 0.3)
        pol.goal_mlp[0].weight.uniform_(-1.0, 1.0)
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    gm = pol.goal_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    e1, e2 = engine(), engine()
    tr = VecPPOTrainer(e1, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=extra, policy="goal_mlp", temperature=TEMP, policy_hold=hold,
                       goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias], prior_table=pol.dist_matrix)
    tr.obs_idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(6))[:M]
    return tr, e2, pol, TEMP


@pytest.mark.parametrize("hold", [False, True])
def test_collect_and_minibatch_step_equal_their_launches_one_by_one(hold):
    """One ``collect()`` of ``policy="goal_mlp"`` against head, draw, [hold], ``frame_fused(skip_choice=True)`` queued one by
    one on a twin engine: action bytes, log-probs, rewards, count bytes, held counts, final state bit for bit. The update
    recomputes the stored log-probs (1e-5, the tolerance of the existing update tests); the head's gradient after one
    minibatch step equals softmax, log-prob, loss, their backward and tarl_policy_goal_mlp_bwd queued one by one; the step
    moves the head's 161 parameters, which are one run of the flat buffer."""
    from tarl_hip import ops
    tr, e2, pol, TEMP = _trainer_case(hold)
    e1 = tr.eng
    T, B, N = tr.T, e1.B, e1.N
    assert tr.rollout == "frames+goal" and tr.state_dep
    w = tr._goal()
    gm = pol.goal_mlp
    assert torch.equal(w.flat, torch.cat([p.data.reshape(-1) for p in (gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias)]))
    assert w.flat.data_ptr() == gm[0].weight.data_ptr()
    tr.collect()
    e2.reset()
    ch2 = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct2 = torch.zeros((T + 1, N, B), device="cuda")
    lp2, rw2 = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    held2 = torch.zeros(B, dtype=torch.int32, device="cuda")
    for t in range(T):
        logits = ops.fused_goal_mlp_logits(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents, w, tr.prior_table, tr.goal_scale)
        ops.graphdist_rollout(e2.plan, logits, TEMP, seed=tr.seed ^ 0x5DEECE66D, counter=1 + t, choice8=ch2[t],
                              sel8=e2.fs.sel8, log_prob=lp2[t])
        if hold:
            ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
        e2.frame_fused(skip_choice=True, reward=rw2[t], counts=ct2[t + 1])
    assert torch.equal(tr.choice, ch2) and torch.equal(tr.logp, lp2) and torch.equal(tr.reward, rw2)
    assert torch.equal(tr.counts.float(), ct2) and torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    if hold:
        assert torch.equal(tr.held, held2) and int(held2.sum()) > 0
    idx = tr.obs_idx.cuda()
    order = torch.argsort(tr.obs_idx, stable=True).cuda()      # the kept rows are stored in frame order
    choice_mb = ops.rollout_gather(e1.plan, T, B, False, idx, choice=tr.choice)[0]
    logits = ops.policy_goal_mlp(e1.plan, tr.obs_mb, w, tr.prior_table, tr.goal_scale)
    proba = ops.graphdist_softmax(e1.plan, logits, TEMP)
    lp_new, ent = ops.graphdist_logprob_entropy(e1.plan, proba, choice=choice_mb)
    lp_old = tr.logp.view(-1).index_select(0, idx)
    assert float((lp_new - lp_old).abs().max()) <= 1e-5
    adv, tgt = tr.advantages()
    adv_mb, tgt_mb = adv.view(-1).index_select(0, idx), tgt.view(-1).index_select(0, idx)
    _, g_lp, g_ent, _ = ops.ppo_loss(lp_new, lp_old, adv_mb, torch.zeros_like(lp_new), tgt_mb, ent,
                                     clip_epsilon=tr.clip_epsilon, entropy_coef=tr.entropy_coef, critic_coef=tr.critic_coef,
                                     grad_scale=1.0)
    g_logits = ops.graphdist_logprob_entropy_bwd(e1.plan, proba, TEMP, choice=choice_mb, grad_log_prob=g_lp,
                                                 grad_entropy=g_ent, log_prob_fwd=lp_new)
    want = torch.zeros(ops.GOAL_MLP_PARAMS, device="cuda")
    ops.policy_goal_mlp_bwd(e1.plan, tr.obs_mb, w, tr.prior_table, tr.goal_scale, g_logits, want)
    before = w.flat.clone()
    out = tr.minibatch_step(adv, tgt)
    assert bool(torch.isfinite(out).all())
    got = tr.flat.grad[tr._goal_off:tr._goal_off + ops.GOAL_MLP_PARAMS]
    assert torch.equal(got, want) and bool(want.any())
    assert not torch.equal(tr._goal().flat, before)
    assert not bool(tr.flat.grad_view(tr.emb_param).any())      # the embedding is off this head's path
    del order


def test_trainer_refusals():
    from tarl_hip.trainer import VecPPOTrainer
    tr, e2, pol, _ = _trainer_case(False)
    gm = pol.goal_mlp
    params = [gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias]
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    crit = tr.critic_params
    with pytest.raises(ValueError, match="goal_mlp_params"):
        VecPPOTrainer(e2, pol.nodes_embedding.weight, crit, rollout_steps=4, sub_batch_size=4, extra_params=extra,
                      policy="goal_mlp", prior_table=pol.dist_matrix)
    with pytest.raises(ValueError, match="part of extra_params"):
        VecPPOTrainer(e2, pol.nodes_embedding.weight, crit, rollout_steps=4, sub_batch_size=4, extra_params=extra[:-1],
                      policy="goal_mlp", goal_mlp_params=params, prior_table=pol.dist_matrix)
    with pytest.raises(ValueError, match="prior_table"):
        VecPPOTrainer(e2, pol.nodes_embedding.weight, crit, rollout_steps=4, sub_batch_size=4, extra_params=extra,
                      policy="goal_mlp", goal_mlp_params=params)


# ---- 7. behaviour cloning: the test that fails without the head ------------------------------------------------------------------------
def _bc_case(net, pop, K, **bc_kw):
    from src.agents.mpnn_agent import MPNNValueNetSimple
    from tarl_hip.imitation import BCTrainer
    from tarl_hip.trainer import VecPPOTrainer
    pol = _policy(net)
    val = MPNNValueNetSimple(net.edge_index, net.num_roads, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    gm = pol.goal_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    ppo = VecPPOTrainer(_engine(net, pop, 2, seed=5), pol.nodes_embedding.weight, crit, rollout_steps=4, sub_batch_size=4,
                        extra_params=extra, policy="goal_mlp", prior_table=pol.dist_matrix,
                        goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias])
    return BCTrainer(ppo, _engine(net, pop, K), **bc_kw), pol, ppo


def test_the_cloned_head_learns_the_router_where_agents_are_bound_anywhere():
    """THE TEST THAT FAILS WITHOUT THE HEAD. ``goal_mlp_restatement.anywhere_case`` on the device: 8 x 8 torus, 128 agents
    bound for roads all over the graph, ``free_flow`` expert, ``expert`` driver, 60 frames, K = 3, 50 full-batch steps at lr
    0.05. Bounds from the float64 restatement (``anywhere_run``: nll 1.4057 -> 0.3743, accuracy on the labelled rows 0.945;
    the ``embedding`` control under the same loop: 1.6697 -> 1.0275, accuracy 0.503): accuracy >= 0.9 x the restatement's,
    nll <= 1.5 x its. Then MODE with ``policy_hold``, K = 3, 300 frames: the cloned head delivers more agents in EVERY
    environment than the same head untrained, and at least half of what the ``free_flow`` router delivers on that seed.
    (MI355X: 8 851 labelled rows, nll 1.4027 -> 0.3716, accuracy 0.000 -> 0.945; arrivals of 128: untrained 0, 0, 0, cloned
    112, 112, 112, the free_flow router 99, 99, 99.)"""
    from tarl_hip import ops
    from tarl_hip.evaluator import VecEvaluator
    ref = G.anywhere_run()
    c = G.ANYWHERE
    acc_ref, nll_ref = ref["goal"]["acc"][-1], ref["goal"]["nll"][-1]
    assert acc_ref >= ref["embedding"]["acc"][-1] + 0.3
    net, pop, _ = G.anywhere_case()
    S = c["frames"] * c["envs"]
    bc, pol, ppo = _bc_case(net, pop, c["envs"], expert="free_flow", driver="expert", frames=c["frames"], samples=S, batch=S,
                            epochs=c["steps"], lr=c["lr"])
    w0 = ppo._goal().flat.clone()
    rec = bc.iterate()
    nll1, acc1, W = bc.evaluate()
    print(f"[goal bc anywhere] {rec['labelled']} labelled rows, loss {rec['loss_first']:.4f} -> {nll1:.4f} (float64 "
          f"{ref['goal']['nll'][0]:.4f} -> {nll_ref:.4f}), accuracy {rec['accuracy_before']:.3f} -> {acc1:.3f} (float64 {acc_ref:.3f}; "
          f"embedding control {ref['embedding']['acc'][-1]:.3f})")
    assert bc.step == c["steps"] and W == rec["labelled"]
    assert acc1 >= 0.9 * acc_ref
    assert nll1 <= 1.5 * nll_ref
    arrived = {}
    for tag, flat in (("untrained", w0), ("cloned", ppo._goal().flat.clone())):
        ev = VecEvaluator(_engine(net, pop, 3, seed=21), "goal_mlp", emb=ppo._emb(), goal_mlp=ops.GoalMlpWeights(flat=flat),
                          goal_scale=ppo.goal_scale, prior_table=ppo.prior_table, policy_hold=True)
        res = ev.run(300)
        assert not res.domain_exit
        arrived[tag] = res.arrived
    ff = VecEvaluator(_engine(net, pop, 3, seed=21), "dijkstra_hold", refresh_rate=0).run(300).arrived
    print(f"[goal bc anywhere] arrivals of {c['agents']}: untrained {arrived['untrained']}, cloned {arrived['cloned']}, "
          f"free_flow router {ff}")
    assert all(a > u for a, u in zip(arrived["cloned"], arrived["untrained"]))
    assert all(2 * a >= f for a, f in zip(arrived["cloned"], ff))


# ---- 8. CLI end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["all_pairs", "per_destination"])
def test_cli_pretrain_then_eval(tmp_path, capsys, method):
    import importlib
    import json
    main = importlib.import_module("main").main
    run = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-300", "--policy-head", "goal_mlp",
          "--prior-method", method, "--pretrain-bc", "1", "--bc-envs", "2", "--bc-samples", "16", "--rollout-steps", "8",
          "--iterations", "1", "--steps", "5", "--output-dir", str(run)])
    text = capsys.readouterr().out
    assert "[bc 0] driver expert" in text
    assert len(open(run / "bc_log.jsonl").readlines()) == 1 and len(open(run / "train_log.jsonl").readlines()) == 1
    sd = torch.load(run / "policy.pt", map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    assert any(k.endswith("goal_mlp.0.weight") for k in sd) and any(k.endswith("goal_scale") for k in sd)
    out = tmp_path / "ev"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--policy-head", "goal_mlp", "--prior-method",
          method, "--checkpoint", str(run / "policy.pt"), "--steps", "60", "--eval-envs", "2", "--policy-hold",
          "--eval-baseline", "dijkstra_hold", "--output-dir", str(out)])
    doc = json.load(open(out / "eval_envs.json"))
    assert doc["mode"]["policy_hold"] is True and doc["baseline"]["settings"]["hold"] is True
