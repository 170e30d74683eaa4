"""GPU: the hold rule on a policy's action — tarl_fused_hold_policy_actions against
``policy_hold_restatement`` on the exported state (the 8 x 8 torus after reset and in a live state, crafted rows on the torus
and both irregular graphs, B in {1, 3, 64, 65}, outputs between guard bands and from garbage-filled buffers, every array the
kernel must not touch compared whole), ``VecEvaluator(policy_hold=True)`` replayed frame by frame by the CPU oracle from the
device's own actions and noise, the finding it answers (a shortest-path policy delivers with the rule and strands without),
``VecPPOTrainer(policy_hold=True).collect()`` against its launches queued one by one, and the CLI. Every comparison is ``==``
except the recomputed log-prob, which keeps the tolerance of the existing update tests."""
import importlib
import json

import pytest
import torch

import policy_hold_restatement as PH

pytestmark = pytest.mark.gpu

SEL_RAW = PH.SEL_RAW
GUARD = 0x55
FEW_DESTS = [3, 17, 40, 66, 90, 101, 120, 127]
UNTOUCHED = ("hdp", "tl", "gc8", "post", "st0", "slots", "node_rec", "in_rec", "out_pad", "acc_lp", "acc_n", "acc_w", "a_origin",
             "a_dest", "a_dep", "a_status", "cur_lo", "flags")


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


def _launch(ops, plan, fs, agents, N, K, *, choice=True, held=True):
    """The op on ``fs`` with its optional outputs between guard bands, the counter starting from garbage -> (sel8 (K, N),
    sel (K, N), choice8 or None, rows held per environment or None), on the host. Every array the kernel must not touch,
    the agent table included, is compared whole before and after."""
    before = {k: getattr(fs, k).clone() for k in UNTOUCHED}
    ag0 = agents.clone()
    pad = 64
    c_big = torch.full((K * N + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    h_big = torch.full((K + 2 * pad,), -77, dtype=torch.int32, device="cuda")
    c8 = c_big[pad:pad + K * N].view(K, N) if choice else None
    h = h_big[pad:pad + K] if held else None
    base = torch.arange(1000, 1000 + K, dtype=torch.int32, device="cuda")
    if held:
        h.copy_(base)
    ops.fused_hold_policy_actions(plan, fs, agents, choice8=c8, held=h)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(fs, k), v), f"the kernel touched fs.{k}"
    assert torch.equal(agents, ag0), "the kernel touched the agent table"
    assert bool((c_big[:pad] == GUARD).all()) and bool((c_big[pad + K * N:] == GUARD).all())
    assert bool((h_big[:pad] == -77).all()) and bool((h_big[pad + K:] == -77).all())
    if not choice:
        assert bool((c_big == GUARD).all())
    if not held:
        assert bool((h_big == -77).all())
    return (fs.sel8.t().cpu(), fs.sel.t().cpu(), c8.cpu() if choice else None, (h - base).cpu().long() if held else None)


def _pack(ops, plan, net, x, ag, Nmax, t=200.0):
    K = x.size(0)
    fs = ops.FusedState(plan, K, ag.size(1), "cuda", Nmax)
    ops.fused_pack(plan, fs, x.cuda(), Nmax, ag.cuda(), net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    exported = x.clone().cuda()
    ops.fused_export(plan, fs, exported, Nmax, t)
    return fs, exported.cpu()


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_kernel_on_crafted_rows(name, K):
    """:func:`policy_hold_restatement.crafted` (the cases test_policy_hold_host checks on the CPU: >= 20 holds on occupied
    rows, every "leave alone" reason, ranks >= 4 and the last rank of the hubs with 9 and 126 out-edges, a DIRTY empty row,
    raw and carried codes): sel8, sel, choice8 and held against the restatement on the exported state; the optional
    outputs left out one at a time change nothing else."""
    from tarl_hip import ops
    cr = PH.crafted(name, K)
    N, Nmax = cr.N, cr.Nmax
    plan = ops.Plan(cr.net.edge_index, N)
    agents = cr.ag.cuda()
    results = []
    for choice, held in ((True, True), (False, True), (True, False), (False, False)):
        fs, exported = _pack(ops, plan, cr.net, cr.x, cr.ag, Nmax)
        stale = cr.rows["stale"]
        assert bool(((fs.hdp[stale, :, 0] & 0xFF) == 0x80).all()) and bool((exported[:, stale, 0] == 11.0).all())      # DIRTY, empty
        fs.sel8.copy_(cr.code.t().cuda())
        fs.sel.copy_(cr.sel.t().cuda())
        s8, sel, c8, h = _launch(ops, plan, fs, agents, N, K, choice=choice, held=held)
        fs.check_flags()
        for b in range(K):
            w8, wsel, wheld = PH.expected_bytes(exported[b], cr.ag[b], cr.succ, cr.deg, Nmax, cr.code[b], cr.sel[b])
            assert torch.equal(s8[b], w8), f"sel8, environment {b}"
            assert torch.equal(sel[b], wsel), f"sel, environment {b}"
            if held:
                assert int(h[b]) == wheld, f"held, environment {b}"
        if choice:
            assert torch.equal(c8, s8)
        results.append((s8, sel))
    assert all(torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) for r in results[1:])
    s8, sel = results[0]
    rows = cr.rows
    for r in ("near", "far") + (("rank4",) if "rank4" in rows else ()):
        i = rows[r]
        assert bool((s8[:, i] == SEL_RAW).all()) and bool((sel[:, i] == float(i)).all()), r
    for r in ("raw", "carried", "head_hi", "other_road", "empty", "stale", "own"):
        i = rows[r]
        assert torch.equal(s8[:, i], cr.code[:, i]) and torch.equal(sel[:, i], cr.sel[:, i]), r


def test_kernel_is_idempotent_and_counts_add_up():
    """Two calls in a row on the torus case: the second changes nothing and adds nothing (a held row carries the raw code)."""
    from tarl_hip import ops
    cr = PH.crafted("torus", 3)
    plan = ops.Plan(cr.net.edge_index, cr.N)
    fs, _ = _pack(ops, plan, cr.net, cr.x, cr.ag, cr.Nmax)
    fs.sel8.copy_(cr.code.t().cuda())
    fs.sel.copy_(cr.sel.t().cuda())
    agents = cr.ag.cuda()
    held = torch.zeros(3, dtype=torch.int32, device="cuda")
    ops.fused_hold_policy_actions(plan, fs, agents, held=held)
    s8, sel, first = fs.sel8.clone(), fs.sel.clone(), held.clone()
    ops.fused_hold_policy_actions(plan, fs, agents, held=held)
    assert torch.equal(fs.sel8, s8) and torch.equal(fs.sel, sel) and torch.equal(held, first) and int(first.sum()) >= 20
    assert int((s8 == SEL_RAW).sum()) == int(first.sum()) + int((cr.code == SEL_RAW).sum())


def test_nothing_changes_after_reset():
    """The 8 x 8 torus after reset: every FIFO is empty, so whatever the policy wrote stays — also where agent 0, whom the
    routers' rule would read on an empty row, is bound for the road the row chose."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    N, K = net.num_roads, 3
    pop = synth.population(128, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    succ, deg, _ = PH.out_table(net.edge_index, N)
    pop[0, 1] = float(succ[5, 2])
    eng = _engine(net, pop, K)
    eng.reset()
    code = torch.randint(0, 4, (K, N), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    code[:, 5] = 2
    eng.fs.sel8.copy_(code.t().cuda())
    eng.fs.sel.fill_(PH.SENTINEL)
    s8, sel, c8, h = _launch(ops, eng.plan, eng.fs, eng.agents, N, K)
    assert torch.equal(s8, code) and bool((sel == PH.SENTINEL).all()) and torch.equal(c8, code) and int(h.sum()) == 0
    # the restatement agrees, and its defect would not
    x = eng.x[0].cpu()
    assert not bool(PH.classify(x, pop, succ, deg, net.Nmax, code=code[0])[0].any())
    assert bool(PH.classify(x, pop, succ, deg, net.Nmax, code=code[0], defect="empty_rows")[0][5])


def test_kernel_on_a_live_state():
    """The 8 x 8 torus after 60 frames of the sampled embedding policy, 500 agents bound for eight roads: every occupied road
    next to its head's destination picks that road, the others a random one; against the restatement on the exported state."""
    import baseline_restatement as BR
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    N, Nmax, K = net.num_roads, net.Nmax, 3
    pop = BR.few_destination_population(500, N, FEW_DESTS, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    eng = _engine(net, pop, K)
    eng.reset()
    eng.prepare_policy(torch.randn(N, generator=torch.Generator().manual_seed(0)).cuda(), 1.0)
    for _ in range(60):
        eng.frame_fused()
    eng.fs.check_flags()
    x, ag = eng.x.cpu(), eng.agents.cpu()
    succ, deg, _ = PH.out_table(net.edge_index, N)
    g = torch.Generator().manual_seed(2)
    code = torch.randint(0, 4, (K, N), generator=g)
    head = x[:, :, 0].long().clamp(0, ag.size(1) - 1)
    dest = torch.gather(ag[:, :, 1].long(), 1, head)
    hit = succ.unsqueeze(0) == dest.unsqueeze(2)
    code = torch.where(hit.any(2), torch.argmax(hit.to(torch.int8), dim=2), code).to(torch.uint8)
    eng.fs.sel8.copy_(code.t().cuda())
    eng.fs.sel.fill_(PH.SENTINEL)
    sel0 = torch.full((N,), PH.SENTINEL)
    s8, sel, c8, h = _launch(ops, eng.plan, eng.fs, eng.agents, N, K)
    total = 0
    for b in range(K):
        w8, wsel, wheld = PH.expected_bytes(x[b], ag[b], succ, deg, Nmax, code[b], sel0)
        assert torch.equal(s8[b], w8) and torch.equal(sel[b], wsel) and int(h[b]) == wheld, b
        total += wheld
    assert torch.equal(c8, s8) and total > 0
    print(f"[policy hold, live torus] {total} rows held in {K} environments, {int((x[:, :, 3 * Nmax + 1] > 0).sum())} occupied")


# ---- 2. the evaluator, replayed by the oracle ----------------------------------------------------------------------------------------
def _spread_population(net):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    return synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)


def _replayed(ev, net, pop, T, deterministic, hold=True):
    """``ev.run(T)`` and, per environment, policy_hold_restatement.replay fed the device's recorded actions and exported
    Gumbel values: every reward, the final state, the agent table and the held count must be equal. -> (EvalResult, replays)."""
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T, deterministic=deterministic)
    assert not res.domain_exit and res.frames_run == T
    rw = ev.reward[:T].cpu()
    actions = ev.actions[:T].cpu()
    runs = []
    for b in range(eng.B):
        r = PH.replay(net, pop, actions[:, b], lambda t: ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu(),
                      EPISODE_START, hold=hold)
        assert r["error"] is None
        assert rw[:, b].tolist() == r["reward"], f"rewards of environment {b}"
        assert torch.equal(r["x"], eng.x[b].cpu()), f"final state of environment {b}"
        assert torch.equal(r["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        assert res.arrived[b] == r["arrivals"]
        if hold:
            assert int(res.held[b]) == sum(r["held"]), f"held of environment {b}"
        runs.append(r)
    return res, runs


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("K", [1, 3])
def test_embedding_head_with_the_rule_is_replayed_by_the_oracle(K, deterministic):
    """``VecEvaluator(head="embedding", policy_hold=True)``, MODE and sampled, 8 x 8 torus, 128 agents, 150 frames: the
    per-frame path (logits once, a draw per frame, the hold launch, the frame). ``actions`` is the policy's own choice: no
    raw byte on a graph where every road has out-edges."""
    import link_counts_restatement as O
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(32))
    pop = O.deliverable_population(net, O.oracle_mode(net, emb)[2]) if deterministic else _spread_population(net)
    ev = VecEvaluator(_engine(net, pop, K), "embedding", emb=emb.cuda(), keep_actions=True, policy_hold=True)
    res, runs = _replayed(ev, net, pop, 150, deterministic)
    assert res.settings["policy_hold"] is True and res.held.shape == (K,) and str(res.held.dtype) == "int64"
    assert bool((ev.actions[:150] < 4).all())
    print(f"[policy hold, embedding {'MODE' if deterministic else 'sampled'}, K={K}] arrivals {res.arrived}, held {res.held.tolist()}")
    if deterministic:       # one action for every environment and frame: the draw does not see the state
        assert bool((ev.actions[:150] == ev.actions[0, 0]).all())
    assert int(res.held.sum()) > 0


def _prior_evaluator(net, pop, K, **kw):
    from tarl_hip import ops
    from tarl_hip.evaluator import VecEvaluator
    eng = _engine(net, pop, K)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()
    table = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    emb = (0.01 * torch.randn(net.num_roads, generator=torch.Generator().manual_seed(5))).cuda()
    return VecEvaluator(eng, "embedding_dijkstra", emb=emb, prior_table=table, prior_weight=1.0, keep_actions=True, **kw)


def test_a_shortest_path_policy_delivers_with_the_rule_and_strands_without():
    """THE TEST THAT FAILS WITHOUT THE FEATURE. The ``embedding_dijkstra`` head in MODE (a policy that heads for the
    destination) on the 8 x 8 torus, 128 agents, 300 frames, K = 3: with ``policy_hold=True`` the device run is the
    restatement's replay of its own actions, frame by frame (the logits' arithmetic does not enter), so it delivers exactly
    the restatement's arrivals — and those exceed, in every environment, the arrivals of the same run without the flag,
    which is replayed by the restatement without the rule. No number is chosen in advance."""
    net = _torus8()
    pop = _spread_population(net)
    on, runs_on = _replayed(_prior_evaluator(net, pop, 3, policy_hold=True), net, pop, 300, True)
    off, runs_off = _replayed(_prior_evaluator(net, pop, 3), net, pop, 300, True, hold=False)
    a_on, a_off = [r["arrivals"] for r in runs_on], [r["arrivals"] for r in runs_off]
    print(f"[policy hold, embedding_dijkstra MODE] arrivals without {a_off} (device {off.arrived}), with the rule {a_on} "
          f"(device {on.arrived}), held {on.held.tolist()}, return {off.episode_return} -> {on.episode_return}")
    assert on.arrived == a_on and off.arrived == a_off
    assert all(w > wo for w, wo in zip(a_on, a_off))
    assert off.held is None and "policy_hold" not in off.settings
    assert all(w > wo for w, wo in zip(on.episode_return, off.episode_return))


# ---- 3. the trainer --------------------------------------------------------------------------------------------------------------------
def _trainer_case(policy, hold=True):
    """The sizes of test_rollout_policy_call_equals_its_launches_one_by_one (a 5 x 4 torus, B = 96, 200 agents, T = 14) ->
    (trainer on engine 1 with ``policy_hold=hold``, twin engine 2, logits_of(engine, observation), TEMP)."""
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
    kw = {}
    if policy == "graph_transformer":
        from src.transformer import laplacian_pe
        pol.use_graph_transformer(laplacian_pe(net.edge_index, N, N))
        tt = pol.transformer.kernel_tensors()
        kw = dict(gt_params=tt, gt_pe=pol.gt_pe)

        def logits_of(e, obs):
            return ops.policy_gt_logits(e.plan, obs, e.ec, pol.gt_pe, ops.GtWeights(tt))
    else:
        mlp = [pol.edge_mlp[0].weight, pol.edge_mlp[0].bias, pol.edge_mlp[2].weight, pol.edge_mlp[2].bias,
               pol.edge_mlp[4].weight, pol.edge_mlp[4].bias]
        kw = dict(edge_mlp_params=mlp, policy_precision="fp32")

        def logits_of(e, obs):
            return ops.policy_edge_mlp(e.plan, obs, e.ec, ops.EdgeMlpWeights(*(p.data for p in mlp)), precision="fp32")
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    e1, e2 = engine(), engine()
    tr = VecPPOTrainer(e1, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=extra, policy=policy, temperature=TEMP, policy_hold=hold, **kw)
    tr.obs_idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(6))[:M]
    return tr, e2, logits_of, TEMP


@pytest.mark.parametrize("policy", ["edge_mlp", "graph_transformer"])
def test_collect_with_the_rule_equals_its_launches_one_by_one(policy):
    """One ``collect()`` with ``policy_hold=True`` against head, draw, hold, ``frame_fused(skip_choice=True)`` queued one by
    one from Python on a twin engine: action bytes, log-probs, rewards, count bytes and held counts bit for bit (so the shared
    loop's Direction launch reads the raw rows as ``frame_fused`` does); the stored action carries no raw byte (the draw
    writes none here) although the packed state does; the first minibatch's recomputed log-prob equals the stored one at the
    tolerance of the existing update tests (PPO ratio 1); the switch is off again afterwards."""
    from tarl_hip import ops
    tr, e2, logits_of, TEMP = _trainer_case(policy)
    e1 = tr.eng
    T, B, N = tr.T, e1.B, e1.N
    tr.collect()
    assert e1.fs.struct.policy_hold == 0 and not e1.fs.struct.policy_held
    e2.reset()
    ch2 = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct2 = torch.zeros((T + 1, N, B), device="cuda")
    lp2, rw2 = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    held2 = torch.zeros(B, dtype=torch.int32, device="cuda")
    pseed = tr.seed ^ 0x5DEECE66D
    raw_in_state = 0
    for t in range(T):
        obs = ops.fused_obs16(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents)
        ops.graphdist_rollout(e2.plan, logits_of(e2, obs), TEMP, seed=pseed, counter=1 + t, choice8=ch2[t], sel8=e2.fs.sel8,
                              log_prob=lp2[t])
        ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents, held=held2)
        raw_in_state += int((e2.fs.sel8 == SEL_RAW).sum())
        e2.frame_fused(skip_choice=True, reward=rw2[t], counts=ct2[t + 1])
    assert torch.equal(tr.choice, ch2) and torch.equal(tr.logp, lp2) and torch.equal(tr.reward, rw2)
    assert torch.equal(tr.counts.float(), ct2) and torch.equal(tr.held, held2)
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert int(held2.sum()) > 0 and raw_in_state == int(held2.sum())
    assert not bool((tr.choice == SEL_RAW).any()) and bool((tr.choice < 4).all())      # the draw's bytes, not the rule's
    # the update recomputes the behaviour log-prob from the stored action: ratio 1
    idx = tr.obs_idx
    lp_dev, _ = ops.graphdist_logprob_entropy(e1.plan, ops.graphdist_softmax(e1.plan, logits_of(e1, tr.obs_mb), TEMP),
                                              choice=ops.rollout_gather(e1.plan, T, B, False, idx.cuda(), choice=tr.choice)[0])
    assert float((lp_dev.cpu() - tr.logp.view(-1).cpu()[idx]).abs().max()) <= 1e-5
    adv, tgt = tr.advantages()
    out = tr.minibatch_step(adv, tgt)
    assert bool(torch.isfinite(out).all())
    print(f"[policy hold, collect {policy}] {int(held2.sum())} rows held in {T} frames x {B} environments")


def test_the_rule_off_queues_what_it_always_queued_and_embedding_is_refused():
    """``policy_hold=False`` (the default) equals the twin loop WITHOUT the hold launch; ``policy='embedding'`` is refused."""
    from tarl_hip import ops
    from tarl_hip.trainer import VecPPOTrainer
    tr, e2, logits_of, TEMP = _trainer_case("edge_mlp", hold=False)
    e1 = tr.eng
    T, B, N = tr.T, e1.B, e1.N
    tr.collect()
    e2.reset()
    ch2 = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    rw2 = torch.zeros((T, B), device="cuda")
    for t in range(T):
        obs = ops.fused_obs16(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents)
        ops.graphdist_rollout(e2.plan, logits_of(e2, obs), TEMP, seed=tr.seed ^ 0x5DEECE66D, counter=1 + t, choice8=ch2[t],
                              sel8=e2.fs.sel8)
        e2.frame_fused(skip_choice=True, reward=rw2[t])
    assert torch.equal(tr.choice, ch2) and torch.equal(tr.reward, rw2) and torch.equal(e1.x, e2.x)
    assert tr.held is None and not bool((e1.fs.sel8 == SEL_RAW).any())
    with pytest.raises(ValueError, match="not available for policy='embedding'"):
        VecPPOTrainer(e1, None, [], rollout_steps=4, policy="embedding", policy_hold=True)


# ---- 4. CLI end to end ------------------------------------------------------------------------------------------------------------------
def test_cli_eval_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    out = tmp_path / "ev"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--steps", "120", "--eval-envs", "2",
          "--policy-hold", "--eval-trips", "--eval-baseline", "dijkstra_hold", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "=== Vectorised evaluation (2 environments, MODE) ===" in text
    assert "policy hold:" in text and "ran with the hold rule" in text and "rows held per environment" in text
    doc = json.load(open(out / "eval_envs.json"))
    assert doc["mode"]["policy_hold"] is True and len(doc["mode"]["held"]) == 2 and doc["mode"]["settings"]["policy_hold"] is True
    assert "policy_hold" not in doc["baseline"] and "policy_hold" not in doc["baseline"]["settings"]
    assert doc["baseline"]["settings"]["hold"] is True


def test_cli_train_end_to_end(tmp_path):
    main = importlib.import_module("main").main
    run = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-300", "--policy-head", "edge_mlp",
          "--policy-hold", "--rollout-steps", "32", "--iterations", "2", "--eval-envs", "2", "--steps", "5",
          "--output-dir", str(run)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert len(logs) == 2
    for rec in logs:
        assert rec["train/held"] >= 0 and rec["eval_vec/held"] >= 0 and rec["eval_vec/envs"] == 2
