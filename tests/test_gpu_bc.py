"""GPU: behaviour cloning of the shortest-path router — tarl_fused_expert_labels against ``bc_restatement`` on
the exported state and against a select launch (crafted rows on the torus and both irregular graphs, after reset and live,
shared and per-environment tables, B in {1, 3, 64, 65}, outputs between guard bands and from garbage, every word of the packed
state compared whole), tarl_graphdist_bc against float64 within the project's tolerance rule and against the pinned
log-prob chain, ``BCTrainer`` against the "dijkstra_hold" evaluator, against its launches queued one by one and against the
float64 loop, the single-destination case in which the cloned embedding must learn the router and deliver, and the CLI."""
import ctypes
import importlib
import json

import pytest
import torch

import bc_restatement as BC
import policy_hold_restatement as PH
import update_restatement as R

pytestmark = pytest.mark.gpu

GUARD = 0x55
PACKED = ("hdp", "tl", "gc8", "post", "st0", "slots", "sel8", "sel", "node_rec", "in_rec", "out_pad", "acc_lp", "acc_n", "acc_w",
          "a_origin", "a_dest", "a_dep", "a_status", "cur_lo", "flags")
FEW_DESTS = [3, 17, 40, 66, 90, 101, 120, 127]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


def _pack(ops, plan, net, x, ag, Nmax, t=200.0):
    K = x.size(0)
    fs = ops.FusedState(plan, K, ag.size(1), "cuda", Nmax)
    ops.fused_pack(plan, fs, x.cuda(), Nmax, ag.cuda(), net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    exported = x.clone().cuda()
    ops.fused_export(plan, fs, exported, Nmax, t)
    return fs, exported


def _label_launch(ops, plan, fs, dest_slot, table, N, K, *, counter=True, x=None, Nmax=None, t=200.0):
    """The op with its outputs between guard bands, the labels starting from garbage and the counter from a base value ->
    (labels (K, N) on the host, labelled rows per environment or None). Every array of the packed state, and its export,
    is compared whole before and after."""
    before = {k: getattr(fs, k).clone() for k in PACKED}
    pad = 64
    l_big = torch.full((K * N + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    h_big = torch.full((K + 2 * pad,), -77, dtype=torch.int32, device="cuda")
    lab = l_big[pad:pad + K * N].view(K, N)
    lab.copy_(torch.randint(0, 256, (K, N), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda())
    h = h_big[pad:pad + K] if counter else None
    base = torch.arange(1000, 1000 + K, dtype=torch.int32, device="cuda")
    if counter:
        h.copy_(base)
    ops.fused_expert_labels(plan, fs, dest_slot, table, out=lab, n_labelled=h)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(fs, k), v), f"the kernel touched fs.{k}"
    if x is not None:
        again = x.clone()
        ops.fused_export(plan, fs, again, Nmax, t)
        assert torch.equal(again, x), "the exported state changed"
    assert bool((l_big[:pad] == GUARD).all()) and bool((l_big[pad + K * N:] == GUARD).all())
    assert bool((h_big[:pad] == -77).all()) and bool((h_big[pad + K:] == -77).all())
    if not counter:
        assert bool((h_big == -77).all())
    return lab.cpu(), (h - base).cpu().long() if counter else None


def _against_select(ops, plan, fs, dest_slot, table, lab):
    """Wherever the label is not IGNORE it is the byte ``fused_select_next_hop_dest(hold=False)`` writes on that state."""
    K, N = lab.shape
    c8 = torch.empty((K, N), dtype=torch.uint8, device="cuda")
    ops.fused_select_next_hop_dest(plan, fs, dest_slot, table, choice8=c8)
    c8 = c8.cpu()
    on = lab != BC.IGNORE
    assert torch.equal(lab[on], c8[on])
    return c8


# ---- 1. the labels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_labels_on_crafted_rows(name, K):
    """:func:`bc_restatement.crafted_labels` (the cases test_bc_host checks on the CPU; a DIRTY empty row among them), with
    per-environment tables (nh_bstride N D) and with environment 0's table shared (0): labels and counter ``==`` the
    restatement on the exported state, the named rows as crafted, and ``==`` the select kernel's byte wherever labelled."""
    from tarl_hip import ops
    cr = BC.crafted_labels(name, K)
    N, Nmax = cr.N, cr.Nmax
    plan = ops.Plan(cr.net.edge_index, N)
    fs, exported = _pack(ops, plan, cr.net, cr.x, cr.ag, Nmax)
    stale = cr.rows["stale"]
    assert bool(((fs.hdp[stale, :, 0] & 0xFF) == 0x80).all())                                       # DIRTY, empty
    fs.sel8.copy_(cr.code.t().cuda())
    fs.sel.copy_(cr.sel.t().cuda())
    ops.fused_export(plan, fs, exported, Nmax, 200.0)          # with the crafted SELECTED_ROAD bytes
    slot = cr.dest_slot.to(torch.int32).cuda()
    x_host = exported.cpu()
    for tables in (cr.tables, cr.tables[0]):
        dev = tables.to(torch.int32).contiguous().cuda()
        lab, cnt = _label_launch(ops, plan, fs, slot, dev, N, K, x=exported, Nmax=Nmax)
        want = BC.expert_labels_envs(x_host, cr.ag, cr.dest_slot, tables, cr.succ, Nmax)
        assert torch.equal(lab, want)
        assert torch.equal(cnt, (want != BC.IGNORE).sum(1))
        lab2, none = _label_launch(ops, plan, fs, slot, dev, N, K, counter=False)
        assert none is None and torch.equal(lab2, lab)
        if tables.dim() == 3:
            for r, w in cr.why.items():
                assert lab[:, cr.rows[r]].tolist() == (w if isinstance(w, list) else [w] * K), r
    fs.check_flags()
    _against_select(ops, plan, fs, slot, cr.tables.to(torch.int32).contiguous().cuda(),
                    BC.expert_labels_envs(x_host, cr.ag, cr.dest_slot, cr.tables, cr.succ, Nmax))


def test_labels_after_reset_and_a_refused_call():
    """After a reset every FIFO is empty: nothing is labelled — also where agent 0, whom the select kernel reads on an empty
    row, has a next hop. A refused call (negative table stride) writes nothing."""
    from tarl_hip import lib, ops, synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    N, K = net.num_roads, 3
    pop = synth.population(128, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    eng = _engine(net, pop, K)
    eng.reset()
    dests = torch.unique(pop[:, 1].long())
    slot = torch.full((N,), -1, dtype=torch.int32)
    slot[dests] = torch.arange(dests.numel(), dtype=torch.int32)
    table = BC.free_flow_table(net, dests.tolist()).to(torch.int32).cuda()
    lab, cnt = _label_launch(ops, eng.plan, eng.fs, slot.cuda(), table, N, K)
    assert bool((lab == BC.IGNORE).all()) and int(cnt.sum()) == 0
    c8 = _against_select(ops, eng.plan, eng.fs, slot.cuda(), table, lab)
    assert bool((c8 < 4).any())                                               # the select kernel does write there
    out = torch.full((K, N), GUARD, dtype=torch.uint8, device="cuda")
    cnt = torch.full((K,), 5, dtype=torch.int32, device="cuda")
    rc = lib.load().tarl_fused_expert_labels(eng.plan.handle, eng.fs.ref, K, eng.fs.Nmax, eng.fs.A, slot.cuda().data_ptr(),
                                             table.data_ptr(), -1, dests.numel(), out.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == GUARD).all()) and bool((cnt == 5).all())


def test_labels_on_a_live_state():
    """The 8 x 8 torus after 60 frames of the holding router, 500 agents bound for eight roads, K = 3, the device's own
    per-environment tables: against the restatement on the exported state and against the select launch."""
    import baseline_restatement as BR
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = synth.torus_network(8, 8)
    N, Nmax, K = net.num_roads, net.Nmax, 3
    pop = BR.few_destination_population(500, N, FEW_DESTS, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    ev = VecEvaluator(_engine(net, pop, K), "dijkstra_hold")
    ev.run(60)
    eng = ev.eng
    x = eng.x.clone()
    lab, cnt = _label_launch(ops, eng.plan, eng.fs, ev.dest_slot, ev.table, N, K, x=x, Nmax=Nmax, t=eng._last_step_time)
    succ, _, _ = PH.out_table(net.edge_index, N)
    want = BC.expert_labels_envs(x.cpu(), eng.agents.cpu(), ev.dest_slot.cpu().long(), ev.table.cpu().long(), succ, Nmax)
    assert torch.equal(lab, want) and torch.equal(cnt, (want != BC.IGNORE).sum(1)) and int(cnt.min()) >= 20
    _against_select(ops, eng.plan, eng.fs, ev.dest_slot, ev.table, lab)
    print(f"[bc labels, live torus] {cnt.tolist()} labelled rows of {N}")


@pytest.mark.parametrize("name", ["MIXED", "HUB126"])
def test_labels_on_a_live_state_of_an_irregular_graph(name):
    """40 frames of the holding router on MIXED (the load of test_gpu_eval_baseline.IRREGULAR_LOAD) and on HUB126 (300 agents
    bound for the hub with 126 out-edges, one of its targets and six more roads), K = 3, nobody starting on a dead end: states
    the engine produced itself, with long out-lists, dead ends and an unsorted edge list, the device's own per-environment
    tables. Against the restatement on the exported state and against the select launch; ranks >= 4 are among the labels."""
    import baseline_restatement as BR
    import irregular_graphs as ig
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = ig.graph(name)
    N, Nmax, K = net.num_roads, net.Nmax, 3
    _, dout = ig.degrees(net)
    leads_on = torch.nonzero(dout > 0).view(-1)
    succ, _, _ = PH.out_table(net.edge_index, N)
    if name == "MIXED":
        agents, span, dests = 600, 30, [5, 17, 33, 48, 61, 12, 13, 70]
    else:
        hub = int(torch.argmax(dout))
        agents, span = 300, 30
        dests = [hub, int(succ[hub, int(dout[hub]) - 1])] + [int(leads_on[k]) for k in (3, 40, 77, 110, 150, 200)]
    pop = BR.few_destination_population(agents, N, dests, seed=7, t0=EPISODE_START, t1=EPISODE_START + span)
    pop[:, 0] = leads_on[pop[:, 0].long() % leads_on.numel()].float()
    ev = VecEvaluator(_engine(net, pop, K), "dijkstra_hold")
    res = ev.run(40)
    assert not res.domain_exit
    eng = ev.eng
    x = eng.x.clone()
    lab, cnt = _label_launch(ops, eng.plan, eng.fs, ev.dest_slot, ev.table, N, K, x=x, Nmax=Nmax, t=eng._last_step_time)
    want = BC.expert_labels_envs(x.cpu(), eng.agents.cpu(), ev.dest_slot.cpu().long(), ev.table.cpu().long(), succ, Nmax)
    assert torch.equal(lab, want) and torch.equal(cnt, (want != BC.IGNORE).sum(1)) and int(cnt.min()) >= 20
    _against_select(ops, eng.plan, eng.fs, ev.dest_slot, ev.table, lab)
    on = lab != BC.IGNORE
    occupied = x[:, :, 3 * Nmax + 1].cpu() > 0
    print(f"[bc labels, live {name}] {cnt.tolist()} labelled rows of {N} ({occupied.sum(1).tolist()} occupied), "
          f"{int((lab[on] >= 4).sum())} labels of rank >= 4, largest {int(lab[on].max())}")
    assert bool((lab[on] >= 4).any()) and bool((occupied & ~on).any())      # long out-lists, and occupied rows the expert leaves


# ---- 2. the loss -----------------------------------------------------------------------------------------------------------------
def _bc_call(plan, logits, labels, T, scale, grad=True):
    """tarl_graphdist_bc through the C ABI with NaN / garbage-filled outputs between guard bands -> (nll, n_lab, n_hit, grad)."""
    from tarl_hip import lib
    L = lib.load()
    M, E = logits.shape
    pad = 16
    nll = torch.full((M + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda")
    cnt = torch.full((2, M + 2 * pad), -77, dtype=torch.int32, device="cuda")
    g = torch.full((M * E + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda") if grad else None
    need = int(L.tarl_graphdist_bc_scratch_bytes(plan.handle, M))
    scratch = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    rc = L.tarl_graphdist_bc(plan.handle, logits.data_ptr(), M, float(T), labels.data_ptr(), float(scale),
                             nll[pad:].data_ptr(), cnt[0, pad:].data_ptr(), cnt[1, pad:].data_ptr(),
                             g[pad:].data_ptr() if grad else None, scratch.data_ptr(), lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(nll[:pad]).all()) and bool(torch.isnan(nll[pad + M:]).all())
    assert bool((cnt[:, :pad] == -77).all()) and bool((cnt[:, pad + M:] == -77).all())
    if grad:
        assert bool(torch.isnan(g[:pad]).all()) and bool(torch.isnan(g[pad + M * E:]).all())
    return (nll[pad:pad + M].cpu(), cnt[0, pad:pad + M].cpu().long(), cnt[1, pad:pad + M].cpu().long(),
            g[pad:pad + M * E].view(M, E).cpu() if grad else None)


@pytest.fixture(scope="module")
def loss_refs():
    return {}


@pytest.mark.parametrize("M", [1, 3, 64, 65])
@pytest.mark.parametrize("kind", ["random", "sharp", "sentinel"])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_loss_against_float64(name, kind, M):
    """Counts and hits ``==``; nll and grad_logits against the float64 restatement within ``R.tensor_bound(e32, ref)``, e32
    from the fp32 restatement (``relative_scale=True`` for the O(1 / W) gradients); every output element written (NaN-filled
    before), two runs bit-identical. The torus is one full tile of 256 nodes, MIXED (80) and HUB126 (280: two tiles) leave a
    ragged last tile; MIXED's edge list is unsorted."""
    from tarl_hip import ops
    net = PH.network(name)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    lg, lab = BC.loss_logits(ei, N, M, kind), BC.loss_labels(ei, N, M)
    T = 0.7
    r64 = BC.bc_loss(ei, N, lg, lab, T, 1.0)
    W = max(int(r64["n_labelled"].sum()), 1)
    r64 = BC.bc_loss(ei, N, lg, lab, T, 1.0 / W)
    r32 = BC.bc_loss(ei, N, lg, lab, T, 1.0 / W, torch.float32)
    dl, dlab = lg.cuda(), lab.cuda()
    nll, nl, nh, g = _bc_call(plan, dl, dlab, T, 1.0 / W)
    assert torch.equal(nl, r64["n_labelled"]) and torch.equal(nh, r64["n_hit"])
    assert not bool(torch.isnan(nll).any()) and not bool(torch.isnan(g).any())
    b_n = R.tensor_bound(R.max_err(r32["nll"], r64["nll"]), r64["nll"])
    b_g = R.tensor_bound(R.max_err(r32["grad"], r64["grad"]), r64["grad"], relative_scale=True)
    err_n, err_g = R.max_err(nll, r64["nll"]), R.max_err(g, r64["grad"])
    print(f"[bc loss {name} {kind} M={M}] W={W} nll err {err_n:.3e} (bound {b_n:.3e}), grad err {err_g:.3e} (bound {b_g:.3e})")
    assert err_n <= b_n and err_g <= b_g
    assert not bool(g[~r64["labelled"][:, ei[0]]].any())                       # exact zeros on the edges of ignored nodes
    nll2, nl2, nh2, g2 = _bc_call(plan, dl, dlab, T, 1.0 / W)
    assert torch.equal(nll, nll2) and torch.equal(g, g2) and torch.equal(nl, nl2) and torch.equal(nh, nh2)
    nll3, nl3, nh3, none = _bc_call(plan, dl, dlab, T, 0.0, grad=False)
    assert none is None and torch.equal(nll3, nll) and torch.equal(nl3, nl) and torch.equal(nh3, nh)
    # the wrapper: grad_scale None = 1 / the labelled nodes of the call
    if W > 1:
        w = ops.graphdist_bc(plan, dl, dlab, T)
        assert torch.equal(w[0].cpu(), nll) and torch.equal(w[3].cpu(), g)


@pytest.mark.parametrize("name", ["torus", "HUB126"])
def test_gradient_equals_the_pinned_log_prob_chain(name):
    """Every node with out-edges labelled with its most probable edge: grad_logits equals graphdist_softmax ->
    graphdist_logprob_entropy_bwd with grad_log_prob = -grad_scale (the chain PPO's update runs) within the same bound.
    (The chain adds 1e-8 to the probability inside the logarithm: relative 1e-8 / p, far inside the bound at p >= 1 / 126.)"""
    from tarl_hip import ops
    net = PH.network(name)
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    M, T = 3, 0.7
    lg = BC.loss_logits(ei, N, M, "random")
    eid, deg, _ = BC.csr_edges(ei, N)
    z = torch.where(eid >= 0, lg[:, eid.clamp(min=0)], torch.full((1,), float("-inf")))
    rank = torch.argmax(z, dim=2)
    lab = torch.where(deg.unsqueeze(0) > 0, rank, torch.full_like(rank, BC.IGNORE)).to(torch.uint8)
    W = int((deg > 0).sum()) * M
    r64 = BC.bc_loss(ei, N, lg, lab, T, 1.0 / W)
    r32 = BC.bc_loss(ei, N, lg, lab, T, 1.0 / W, torch.float32)
    _, nl, nh, g = _bc_call(plan, lg.cuda(), lab.cuda(), T, 1.0 / W)
    assert int(nl.sum()) == W == int(nh.sum())
    choice = torch.where(deg.unsqueeze(0) > 0, torch.gather(eid.unsqueeze(0).expand(M, -1, -1), 2, rank.unsqueeze(2)).squeeze(2),
                         torch.full_like(rank, -1)).to(torch.int32).cuda()
    proba = ops.graphdist_softmax(plan, lg.cuda(), T)
    chain = ops.graphdist_logprob_entropy_bwd(plan, proba, T, choice=choice,
                                              grad_log_prob=torch.full((M,), -1.0 / W, device="cuda")).cpu()
    bound = R.tensor_bound(R.max_err(r32["grad"], r64["grad"]), r64["grad"], relative_scale=True)
    err = R.max_err(g, chain)
    print(f"[bc loss vs chain, {name}] err {err:.3e} (bound {bound:.3e})")
    assert err <= bound and R.max_err(g, r64["grad"]) <= bound


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------
def _bc_case(policy, net, pop, K, *, emb0=None, **bc_kw):
    """-> (BCTrainer on an engine of K environments, the policy network). The PPO trainer behind it runs on a two-environment
    engine of its own: it lends its flat parameter buffer and the head's forward and backward."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip.imitation import BCTrainer
    from tarl_hip.trainer import VecPPOTrainer
    N = net.num_roads
    torch.manual_seed(1)
    pol = MPNNPolicyNet(net.edge_index, N, None, device="cuda")
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    if emb0 is not None:
        pol.nodes_embedding.weight.data.copy_(emb0.view(-1, 1).cuda())
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    kw = {}
    if policy == "graph_transformer":
        from src.transformer import laplacian_pe
        pol.use_graph_transformer(laplacian_pe(net.edge_index, N, N))
        kw = dict(gt_params=pol.transformer.kernel_tensors(), gt_pe=pol.gt_pe)
    elif policy == "edge_mlp":
        m = pol.edge_mlp
        kw = dict(edge_mlp_params=[m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias],
                  policy_precision="fp32")
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    ppo = VecPPOTrainer(_engine(net, pop, 2, seed=5), pol.nodes_embedding.weight, crit, rollout_steps=4, sub_batch_size=4,
                        extra_params=extra, policy=policy, **kw)
    return BCTrainer(ppo, _engine(net, pop, K), **bc_kw), pol


def test_expert_iteration_is_the_dijkstra_hold_evaluation_with_labels():
    """One collection with the ``expert`` driver (expert ``dijkstra``, refresh every 10 frames), K = 3, 45 frames, 500 agents
    bound for eight roads: frame by frame the labels ``==`` the restatement on the device's exported state and tables;
    rewards and agent tables ``==`` a ``VecEvaluator(head="dijkstra_hold")`` run with the same seed; the store holds the
    kept pairs' label rows."""
    import baseline_restatement as BR
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = synth.torus_network(8, 8)
    N, Nmax, K, T = net.num_roads, net.Nmax, 3, 45
    pop = BR.few_destination_population(500, N, FEW_DESTS, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    bc, _ = _bc_case("embedding", net, pop, K, expert="dijkstra", driver="expert", frames=T, samples=40, batch=16)
    eng = bc.eng
    succ, _, _ = PH.out_table(net.edge_index, N)
    seen, total = [], [0]

    def hook(t):
        want = BC.expert_labels_envs(eng.x.cpu(), eng.agents.cpu(), bc.dest_slot.cpu().long(), bc.table.cpu().long(), succ, Nmax)
        assert torch.equal(bc.labels.cpu(), want), f"labels of frame {t}"
        seen.append(want)
        total[0] += int((want != BC.IGNORE).sum())
    bc.frame_hook = hook
    bc.keep_idx = torch.randperm(T * K, generator=torch.Generator().manual_seed(6))[:40]
    labelled, arrivals = bc.collect("expert")
    assert labelled == total[0] > 0
    for j, flat in enumerate(bc.keep_idx.tolist()):
        assert torch.equal(bc.label_store[j].cpu(), seen[flat // K][flat % K]), j
    ev = VecEvaluator(_engine(net, pop, K), "dijkstra_hold", refresh_rate=10)
    res = ev.run(T)
    assert torch.equal(ev.reward[:T], bc.reward[:T]) and torch.equal(ev.eng.agents, eng.agents) and torch.equal(ev.eng.x, eng.x)
    assert abs(arrivals - sum(res.arrived) / K) < 1e-3 and arrivals > 0
    print(f"[bc expert iteration] {labelled} labelled rows in {T} frames x {K} environments, arrivals {res.arrived}")


@pytest.mark.parametrize("policy", ["edge_mlp", "graph_transformer"])
def test_policy_driver_and_minibatch_step_equal_their_launches_one_by_one(policy):
    """5 x 4 torus, K = 6, 12 frames. The ``policy`` driver's frames ``==`` observation, head, sampled draw, hold launch and
    ``frame_fused(skip_choice=True)`` queued one by one on a twin engine (rewards, state, agent tables, held rows); one
    minibatch step ``==`` head forward, ``graphdist_bc``, head backward and Adam (fresh moments, step 1) queued one by one
    on a copy of the parameters."""
    from tarl_hip import ops, synth
    net = synth.torus_network(5, 4, heterogeneous=True, seed=3)
    N, K, T = net.num_roads, 6, 12
    pop = synth.population(200, N, seed=40, t0=21540, t1=21546)
    bc, pol = _bc_case(policy, net, pop, K, expert="free_flow", driver="policy", frames=T, samples=24, batch=8, lr=1e-2)
    ppo, eng = bc.ppo, bc.eng

    def logits_of(e, obs):
        if policy == "graph_transformer":
            return ops.policy_gt_logits(e.plan, obs, e.ec, pol.gt_pe, ppo._gt())
        return ops.policy_edge_mlp(e.plan, obs, e.ec, ppo._edge_mlp(), precision="fp32")
    labelled, _ = bc.collect("policy")
    e2 = _engine(net, pop, K)
    e2.reset()
    rw2 = torch.zeros((T, K), device="cuda")
    held2 = torch.zeros(K, dtype=torch.int32, device="cuda")
    for t in range(T):
        obs = ops.fused_obs16(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents)
        ops.graphdist_rollout(e2.plan, logits_of(e2, obs), ppo.temperature, seed=e2.seed ^ 0x5DEECE66D, counter=1 + t,
                              sel8=e2.fs.sel8)
        ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
        e2.frame_fused(skip_choice=True, reward=rw2[t])
    assert torch.equal(bc.reward[:T], rw2) and torch.equal(eng.x, e2.x) and torch.equal(eng.agents, e2.agents)
    assert torch.equal(bc.held, held2) and labelled > 0
    # one minibatch step
    per = (bc.label_store != BC.IGNORE).sum(1).cpu()
    idx = torch.nonzero(per > 0).view(-1)[:8]
    W = int(per[idx].sum())
    assert W > 0
    flat0 = ppo.flat.flat.clone()
    nll, nl, nh = bc.minibatch_step(idx.cuda(), W)
    flat1 = ppo.flat.flat.clone()
    ppo.flat.flat.copy_(flat0)
    obs, labels = bc.obs_store.index_select(0, idx.cuda()), bc.label_store.index_select(0, idx.cuda())
    out = ops.graphdist_bc(e2.plan, logits_of(e2, obs), labels, ppo.temperature, grad_scale=1.0 / W)
    assert torch.equal(out[0], nll) and int(out[1].sum()) == W
    ppo.flat.zero_grad()
    if policy == "graph_transformer":
        ops.policy_gt_bwd(e2.plan, obs, e2.ec, pol.gt_pe, ppo._gt(), out[3],
                          [ppo.flat.grad_view(ppo.gt_params[k]) for k in ops.GT_PARAM_KEYS])
    else:
        gm = [ppo.flat.grad_view(p) for p in ppo.edge_mlp_params]
        ops.policy_edge_mlp_bwd(e2.plan, obs, e2.ec, ppo._edge_mlp(), out[3], (gm[0], gm[1], gm[2], gm[3], gm[4].view(-1), gm[5]))
    assert bool(ppo.flat.grad.any())
    ops.adam_step_(ppo.flat.flat, ppo.flat.grad, torch.zeros_like(flat0), torch.zeros_like(flat0), 1, lr=1e-2)
    assert torch.equal(ppo.flat.flat, flat1) and not torch.equal(flat1, flat0)
    assert ppo.flat.step == 0 and not bool(ppo.flat.exp_avg.any())           # PPO's own moments are untouched
    print(f"[bc {policy}] policy driver: {labelled} labelled rows, held {held2.tolist()}; step on {W} labelled nodes")


def _single_case(K=3):
    net, pop, t0 = BC.single_destination_case()
    emb0 = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(5), dtype=torch.float64).float()
    S = BC.SINGLE["frames"] * K
    bc, pol = _bc_case("embedding", net, pop, K, emb0=emb0, expert="free_flow", driver="expert", frames=BC.SINGLE["frames"],
                       samples=S, batch=S, epochs=BC.SINGLE["steps"], lr=BC.SINGLE["lr"])
    return net, pop, emb0, bc, pol


def test_embedding_step_equals_the_float64_loop():
    """The embedding head, one full-batch step on the single-destination store: the updated embedding against one step of
    ``bc_restatement.bc_loop_embedding`` in float64 within ``R.tensor_bound``, e32 from the same step in fp32."""
    net, pop, emb0, bc, pol = _single_case()
    bc.collect("expert")
    labels = bc.label_store.cpu()
    W = int((labels != BC.IGNORE).sum())
    nll, _, _ = bc.minibatch_step(torch.arange(bc.samples, device="cuda"), W)
    got = pol.nodes_embedding.weight.detach().view(-1).cpu()
    r64 = BC.bc_loop_embedding(net.edge_index, net.num_roads, labels, emb0, 1, BC.SINGLE["lr"])
    r32 = BC.bc_loop_embedding(net.edge_index, net.num_roads, labels, emb0, 1, BC.SINGLE["lr"], dtype=torch.float32)
    bound = R.tensor_bound(R.max_err(r32["emb"], r64["emb"]), r64["emb"])
    err = R.max_err(got, r64["emb"])
    print(f"[bc embedding step] W={W}, loss {float(nll.sum()) / W:.6f} (float64 {r64['nll'][0]:.6f}), err {err:.3e} (bound {bound:.3e})")
    assert abs(float(nll.sum()) / W - r64["nll"][0]) <= 1e-5 * max(1.0, r64["nll"][0])
    assert err <= bound and not torch.equal(got, emb0)


def test_the_cloned_embedding_learns_the_router_and_delivers():
    """THE TEST THAT FAILS WITHOUT THE FEATURE. The single-destination case of test_bc_host on the device: 8 x 8 torus, every
    agent bound for one road, ``embedding`` head from N(0, 1), ``free_flow`` expert, ``expert`` driver, 50 full-batch steps
    at lr 0.05: final nll <= 0.5 x the first and accuracy on the labelled rows >= 0.9 (the host test's bounds with a factor
    two of room for fp32). Then ``VecEvaluator`` in MODE with ``policy_hold=True``, K = 3, 300 frames: the cloned head
    delivers more agents in EVERY environment than the same head untrained. (MI355X: 5 810 labelled rows, nll 1.8183 ->
    0.1234, accuracy 0.107 -> 1.000; arrivals of 128: untrained 0, 0, 0, cloned 128, 128, 128, the free_flow router 128, 128, 128.)"""
    from tarl_hip.evaluator import VecEvaluator
    net, pop, emb0, bc, pol = _single_case()
    rec = bc.iterate()
    nll1, acc1, W = bc.evaluate()
    print(f"[bc single destination] {rec['labelled']} labelled rows, loss {rec['loss_first']:.4f} -> {nll1:.4f}, accuracy "
          f"{rec['accuracy_before']:.3f} -> {acc1:.3f}, expert arrivals {rec['arrivals']:.1f}")
    assert bc.step == BC.SINGLE["steps"] and W == rec["labelled"]
    assert nll1 <= 0.5 * rec["loss_first"]
    assert acc1 >= 0.9 and rec["accuracy_after"] == acc1
    arrived = {}
    for tag, emb in (("untrained", emb0.cuda()), ("cloned", pol.nodes_embedding.weight.detach().view(-1).clone())):
        ev = VecEvaluator(_engine(net, pop, 3, seed=21), "embedding", emb=emb.contiguous(), policy_hold=True)
        res = ev.run(300)
        assert not res.domain_exit
        arrived[tag] = res.arrived
    ff = VecEvaluator(_engine(net, pop, 3, seed=21), "dijkstra_hold", refresh_rate=0).run(300).arrived
    print(f"[bc single destination] arrivals of {BC.SINGLE['agents']}: untrained {arrived['untrained']}, cloned {arrived['cloned']}, "
          f"free_flow router {ff}")
    assert all(c > u for c, u in zip(arrived["cloned"], arrived["untrained"]))


def test_refusals_of_the_wrapper_and_the_trainer(monkeypatch):
    """On the device: a scratch one byte short of ``tarl_graphdist_bc_scratch_bytes`` is refused by ``ops.graphdist_bc`` and a
    caller-owned buffer of exactly that size is accepted and gives the same outputs; ``BCTrainer`` refuses an engine on the
    per-op kernels (``fused=False``) and a store beyond half the free device memory, with the numbers in the message."""
    from tarl_hip import lib, ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.imitation import BCTrainer
    net = PH.network("HUB126")
    ei, N = net.edge_index, net.num_roads
    plan = ops.Plan(ei, N)
    M = 3
    lg, lab = BC.loss_logits(ei, N, M, "random").cuda(), BC.loss_labels(ei, N, M).cuda()
    need = int(lib.load().tarl_graphdist_bc_scratch_bytes(plan.handle, M))
    assert need == M * 2 * 16
    short = torch.full((need - 1,), GUARD, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=f"scratch holds {need - 1} bytes, tarl_graphdist_bc needs {need}"):
        ops.graphdist_bc(plan, lg, lab, 0.7, grad_scale=0.01, scratch=short)
    torch.cuda.synchronize()
    assert bool((short == GUARD).all())
    own = ops.graphdist_bc(plan, lg, lab, 0.7, grad_scale=0.01, scratch=torch.empty(need, dtype=torch.uint8, device="cuda"))
    ref = ops.graphdist_bc(plan, lg, lab, 0.7, grad_scale=0.01)
    assert all(torch.equal(a, b) for a, b in zip(own, ref))
    # the trainer
    tnet = synth.torus_network(4, 4)
    pop = synth.population(60, tnet.num_roads, seed=2, t0=21540, t1=21550)
    bc, _ = _bc_case("embedding", tnet, pop, 2, frames=8, samples=8, batch=4)
    plain = SimEngine(tnet.x.cuda(), tnet.edge_index, tnet.edge_attr, tnet.Nmax, pop.cuda(),
                      congestion_constant=tnet.congestion_constant, num_envs=2, seed=3, fused=False)
    assert plain.fs is None
    with pytest.raises(lib.TarlError, match="BCTrainer needs the fused engine"):
        BCTrainer(bc.ppo, plain)
    free = 10 * tnet.num_roads * 65 * 2 + 1                        # room for ten samples, not eleven
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (free, 4 * free))
    with pytest.raises(ValueError, match=f"store of 11 samples x {tnet.num_roads} nodes x 65 bytes .* at most 10 samples fit"):
        BCTrainer(bc.ppo, bc.eng, frames=8, samples=11, batch=4)


# ---- 4. CLI end to end -----------------------------------------------------------------------------------------------------------------
def test_cli_pretrain_then_eval(tmp_path, capsys):
    from tarl_hip.imitation import RECORD_KEYS
    main = importlib.import_module("main").main
    run = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-300", "--policy-head", "edge_mlp",
          "--pretrain-bc", "2", "--bc-driver", "dagger", "--bc-envs", "4", "--bc-samples", "32", "--bc-epochs", "2",
          "--rollout-steps", "32", "--iterations", "1", "--steps", "5", "--output-dir", str(run)])
    text = capsys.readouterr().out
    assert "[bc 0] driver expert (dijkstra)" in text and "[bc 1] driver policy (dijkstra)" in text
    logs = [json.loads(l) for l in open(run / "bc_log.jsonl")]
    assert len(logs) == 2 and all(tuple(r) == RECORD_KEYS for r in logs)
    assert [r["driver"] for r in logs] == ["expert", "policy"] and all(r["frames"] == 32 and r["envs"] == 4 for r in logs)
    assert len([json.loads(l) for l in open(run / "train_log.jsonl")]) == 1
    out = tmp_path / "ev"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--policy-head", "edge_mlp", "--checkpoint",
          str(run / "policy.pt"), "--steps", "120", "--eval-envs", "2", "--policy-hold", "--eval-baseline", "dijkstra_hold",
          "--output-dir", str(out)])
    doc = json.load(open(out / "eval_envs.json"))
    assert doc["mode"]["policy_hold"] is True and doc["baseline"]["settings"]["hold"] is True
    # cloning alone: --algo mpnn writes the checkpoint without a PPO iteration
    solo = tmp_path / "solo"
    main(["--algo", "mpnn", "--mode", "train", "--scenario", "synthetic-1024-300", "--pretrain-bc", "1", "--bc-driver", "expert",
          "--bc-expert", "free_flow", "--bc-envs", "2", "--bc-samples", "16", "--rollout-steps", "16", "--steps", "5",
          "--output-dir", str(solo)])
    assert (solo / "policy.pt").exists() and len(open(solo / "bc_log.jsonl").readlines()) == 1
    assert not (solo / "train_log.jsonl").exists() or not open(solo / "train_log.jsonl").read().strip()


def test_cli_refuses_a_graph_the_packed_path_cannot_represent(tmp_path, monkeypatch):
    """``--pretrain-bc`` on a network whose links hold 127 vehicles (948 m: Nmax = 128, beyond the packed path): refused in
    ``Runner.setup`` with a message, before any training; without the flag the same scenario sets up."""
    from src.runner import Runner, RunnerArgs
    from tarl_hip import ops, synth
    torus = synth.torus_network
    monkeypatch.setattr(synth, "torus_network", lambda W, H, **kw: torus(W, H, length=948.0, freespeed=94.8, **kw))
    base = dict(algo="mpnn", scenario="synthetic-64-40", mode="train", output_dir=str(tmp_path))
    r = Runner(RunnerArgs(**base, pretrain_bc=1))
    with pytest.raises(ValueError, match="--pretrain-bc needs the packed \\(fused\\) path, which cannot represent this graph"):
        r.setup()
    r = Runner(RunnerArgs(**{**base, "mode": "eval"}))
    r.setup()
    sim = r.env.simulator
    assert sim.Nmax == 128 and not ops.fused_path_supported(sim.graph.edge_index, sim.Nmax)
