"""GPU: the graph-transformer head (csrc/gt_policy.hip) against the reference's golden and the CPU restatement — forward,
deterministic backward, the PPO update on a rollout under the head, and the CLI end to end."""
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

sys.path.insert(0, PKG)
import gt_restatement as R_  # noqa: E402
import gt_cases as H  # noqa: E402
from gt_cases import _close, _random_state, _reference_state, _span  # noqa: E402

pytestmark = pytest.mark.gpu


def _golden():
    z = np.load(f"{ROOT}/tests/golden/gt_policy.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _setup(sd, ei, ea, N):
    from tarl_hip import ops
    plan = ops.Plan(ei, N)
    ec = ops.EdgeConst(ea.reshape(-1, 1), "cuda")
    t = {k: v.cuda().float().contiguous() for k, v in sd.items() if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS}
    return plan, ec, t


def _grads(ops, plan, obs, ec, pe, w, coef):
    grads = [torch.zeros_like(p) for p in w.params]
    ops.policy_gt_bwd(plan, obs, ec, pe, w, coef, grads)
    return grads


def test_forward_and_backward_match_the_reference_golden():
    from tarl_hip import ops
    g = _golden()
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd/")}
    N = g["pe"].size(0)
    plan, ec, t = _setup(sd, g["edge_index"], g["edge_attr"], N)
    w = ops.GtWeights(t)
    pe = g["pe"].cuda().contiguous()
    ls = ops.policy_gt_logits(plan, g["x_single"].cuda().unsqueeze(0).contiguous(), ec, pe, w)
    _close(ls[0].cpu(), g["logits_single"], "logits (unbatched)")
    xb = g["x_batch"].cuda().contiguous()
    _close(ops.policy_gt_logits(plan, xb, ec, pe, w).cpu(), g["logits_batch"], "logits (batched)")
    coef = g["coef"].cuda().contiguous()
    g1 = _grads(ops, plan, xb, ec, pe, w, coef)
    g2 = _grads(ops, plan, xb, ec, pe, w, coef)
    for k, a, b in zip(ops.GT_PARAM_KEYS, g1, g2):
        assert torch.equal(a, b), f"{k}: not bit-reproducible"
        _close(a.cpu(), g["grad/" + k], f"grad {k}")
    # every parameter outside the kernel list gets exactly zero from the reference too
    for k, v in g.items():
        if k.startswith("grad/") and k[5:] not in ops.GT_PARAM_KEYS:
            assert float(v.abs().max()) == 0.0, k


CASES = [("torus8", 1, "random"), ("torus16", 7, "random"), ("config4", 1, "reference"), ("config4", 7, "reference"),
         ("config4", 64, "reference"), ("config4", 7, "random"), ("matsim", 1, "reference"), ("matsim", 7, "reference"),
         ("matsim", 64, "reference"), ("matsim", 64, "random")] + H.ATTENTION_CASES


def _check_case(c, ops, plan, ec, w):
    """The kernel's logits and gradients on case ``c`` against its two restatement references; returns (logits, grads, (g64, g32, S))."""
    sharp = c.weights == "sharp"
    if sharp:      # before a kernel is called: the attention of these inputs is neither uniform nor one-hot
        H.check_census(H.attention_census(c.sd, c.obs, c.ei, c.pe, False, edge_attr=c.ea), False)
    obs, pe = c.obs.cuda().contiguous(), c.pe.cuda()
    logits = ops.policy_gt_logits(plan, obs, ec, pe, w)
    # the restatement in float64 (the exact reference) and in float32 (what plain fp32 autograd of the same function
    # achieves: its distance from float64 measures how the inputs condition the function at fp32 precision — on raw
    # observations the attention scores reach ~1e8, so a rounding of the scores moves the small softmax weights), on the
    # device for speed; the sharp cases' on the CPU, where test_gt_attention_host.py proves what their tolerance can see
    ref64, ref32, g64, g32, S = H.references(c, "cpu" if sharp else "cuda")
    if sharp:
        err, tol = float((logits.cpu().double() - ref64).abs().max()), H.sharp_tolerance(ref64, ref32)
        print(f"{c.kind} M={c.M} logits: |kernel - f64| {err:.3e}, |fp32 - f64| {float((ref32 - ref64).abs().max()):.3e}, tol {tol:.3e}")
        assert err <= tol, f"logits: {err} > {tol}"
    else:
        _close(logits.cpu(), ref64, "logits")
    grads = _grads(ops, plan, obs, ec, pe, w, c.coef.cuda())
    for k, gk in zip(ops.GT_PARAM_KEYS, grads):
        # the kernel's error may exceed fp32 autograd's by at most a factor 16, plus the kernel's own summation bound,
        # elementwise (gt_cases.grad_allowance)
        err = (gk.cpu().double() - g64[k]).abs()
        allow = H.grad_allowance(k, g64, g32, S, c)
        assert bool((err <= allow).all()), f"grad {k}: worst err / allowance {float((err / allow.clamp(min=1e-300)).max())}"
    return logits, grads, (g64, g32, S)


@pytest.mark.parametrize("kind,M,weights", CASES)
def test_forward_and_backward_match_the_restatement(kind, M, weights, tmp_path):
    """Unscaled observations (raw clock-time and id columns), the reference's initialisation, scaled random or sharp weights,
    on tori, config 4 (25 x 25), a MATSim grid with SRC / DEST pseudo-nodes (empty in- / out-segments, zero PE rows) and the
    irregular road graphs MIXED (80 roads: less than one block and one chunk at M = 1) and HUB126 (280 roads, 17 852 edges in
    no order, in- and out-degree up to 126: 840 node items and 53 556 edge items at M = 3, a short last chunk each).
    Sharp cases: the logits within 16 x the fp32 restatement's own distance from float64 + 8 ulps of their scale, after
    the inputs passed the attention census; the others within 1e-4 of their scale. Measured on an MI355X: DESIGN.md §4.11a."""
    from tarl_hip import ops
    c = H.case_inputs(kind, M, weights, False, tmp_path)
    if kind == "matsim":
        indeg, outdeg = torch.bincount(c.ei[1], minlength=c.N), torch.bincount(c.ei[0], minlength=c.N)
        assert int((indeg == 0).sum()) > 0 and int((outdeg == 0).sum()) > 0 and int(indeg.max()) > int(indeg[indeg > 0].min())
    plan, ec, t = _setup(c.sd, c.ei, c.ea, c.N)
    if kind in H.IRREGULAR_MAX_DEGREE:
        mx_in, mx_out, in0, out0, _ = H.graph_facts(c.ei, c.N)
        assert not plan.src_sorted and mx_in == mx_out == H.IRREGULAR_MAX_DEGREE[kind] and in0 > 0 and out0 > 0
        assert (plan.max_in, plan.max_out) == (mx_in, mx_out)
    if c.R < c.N:
        assert float(c.pe[c.R:].abs().max()) == 0.0
    assert float(c.obs[..., 9].max()) > 21000                      # raw clock-time departure column
    _check_case(c, ops, plan, ec, ops.GtWeights(t))


def test_sharp_mixed_case_is_reproducible_and_independent_of_the_edge_order(tmp_path):
    """("MIXED", 3, "sharp"): two backward calls give the same bits; and the same graph with its edge list in another order
    that keeps every node's in- and out-edges in their relative order (the plan sorts both segments by edge id, so every
    attention and Q / K / V gradient walk adds the same terms in the same order) gives bit-identical logits (mapped back) and
    bit-identical gradients of every node-side parameter. The edge-side parameters' gradients are sums over the (sample,
    edge) records in edge-id order, which no non-trivial permutation of the edge list keeps: those stay within the
    allowance of the float64 gradient."""
    from tarl_hip import ops
    c = H.case_inputs("MIXED", 3, "sharp", False, tmp_path)
    plan, ec, t = _setup(c.sd, c.ei, c.ea, c.N)
    w = ops.GtWeights(t)
    logits, grads, (g64, g32, S) = _check_case(c, ops, plan, ec, w)
    obs, pe = c.obs.cuda().contiguous(), c.pe.cuda()
    for k, a, b in zip(ops.GT_PARAM_KEYS, grads, _grads(ops, plan, obs, ec, pe, w, c.coef.cuda())):
        assert torch.equal(a, b), f"{k}: not bit-reproducible"
    order = H.order_preserving_shuffle(c.ei, seed=1)
    assert int((order != torch.arange(c.E)).sum()) > c.E // 2
    plan2, ec2, _ = _setup(c.sd, c.ei[:, order].contiguous(), c.ea[order].contiguous(), c.N)
    assert torch.equal(ops.policy_gt_logits(plan2, obs, ec2, pe, w), logits[:, order.cuda()])
    grads2 = _grads(ops, plan2, obs, ec2, pe, w, c.coef[:, order].contiguous().cuda())
    edge_side = 0
    for k, a, b in zip(ops.GT_PARAM_KEYS, grads, grads2):
        if H.items_per_sample(k, False, c.N, c.E) == c.N:
            assert torch.equal(a, b), f"{k}: depends on the edge order"
        else:
            edge_side += 1
            err = (b.cpu().double() - g64[k]).abs()
            assert bool((err <= H.grad_allowance(k, g64, g32, S, c)).all()), k
    assert edge_side == 27                        # edge_emb, 2 x 12 edge-layer parameters, edge_linear.{weight, bias}


def test_ppo_update_with_the_graph_transformer_head():
    """Rollout under the head (tarl_fused_rollout_gt), then one minibatch step: the recomputed log-probs of the kept frames
    equal the rollout's (PPO ratio 1), and the gradients match the restatement's autograd of the same loss."""
    from oracle import dist, nets, ppo
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from src.transformer import laplacian_pe
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(8, 8, heterogeneous=True, seed=2)
    N, E = net.num_roads, net.edge_index.size(1)
    B, A, T, M = 256, 600, 16, 32
    TEMP = 500.0
    pops = torch.stack([synth.population(A, N, seed=b, t0=21540, t1=21550) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=3)
    torch.manual_seed(0)
    pol = MPNNPolicyNet(net.edge_index, N, None, device="cuda")
    pol.use_graph_transformer(laplacian_pe(net.edge_index, N, N))
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    tt = pol.transformer.kernel_tensors()
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=extra, policy="graph_transformer", gt_params=tt, gt_pe=pol.gt_pe, temperature=TEMP)
    assert tr.rollout == "frames+gt"
    tr.keep_grad = True
    idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(4))[:M]
    tr.obs_idx = idx
    tr.collect()
    sd0 = {k: v.detach().cpu().clone() for k, v in tt.items()}
    crit0 = [p.detach().cpu().clone() for p in crit]
    counts = tr.counts.permute(0, 2, 1).float().cpu()
    choice = eng.decode_rollout(False, choice=tr.choice)[0].cpu()
    reward, times = tr.reward.cpu(), tr.times.cpu()
    x16 = tr.obs_mb.cpu()
    assert float(reward.abs().sum()) > 0
    t_idx, b_idx = idx // B, idx % B
    onehot = torch.zeros((M, E), dtype=torch.int64)
    onehot.scatter_(1, choice[t_idx, b_idx].long(), 1)
    pe = pol.gt_pe.cpu()
    # the update's recomputed log-probs of the kept frames == the rollout's
    with torch.no_grad():
        lg = ops.policy_gt_logits(eng.plan, tr.obs_mb, eng.ec, pol.gt_pe, ops.GtWeights(tt))
        lp_dev, _ = ops.graphdist_logprob_entropy(eng.plan, ops.graphdist_softmax(eng.plan, lg, TEMP),
                                                  choice=ops.rollout_gather(eng.plan, T, B, False, idx.cuda(),
                                                                            choice=tr.choice)[0])
    lp_roll = tr.logp.view(-1).cpu()[idx]
    assert float((lp_dev.cpu() - lp_roll).abs().max()) <= 1e-5
    adv_g, tgt_g = tr.advantages()
    out = tr.minibatch_step(adv_g, tgt_g)
    # ---- restatement autograd of the same loss ----
    p = {k: (v.clone().requires_grad_(True) if k in ops.GT_PARAM_KEYS else v) for k, v in sd0.items()}
    cw = [q.clone().requires_grad_(True) for q in crit0]
    nf_all = torch.zeros((T + 1, B, N, 7))
    nf_all[..., 1] = counts
    with torch.no_grad():
        v_all = nets.critic_value(nf_all, times.view(T + 1, 1, 1).expand(T + 1, B, 1), *cw).squeeze(-1)
        nodone = torch.zeros((T, B), dtype=torch.bool)
        adv, tgt = ppo.gae(reward, v_all[:T], v_all[1:], nodone, nodone, average_gae=True)
    d = dist.GraphDist(R_.gt_logits(p, x16, net.edge_index, net.edge_attr, pe), net.edge_index, TEMP)
    lp_new, ent = d.log_prob(onehot), d.entropy()
    _close(lp_new.detach(), lp_roll, "log-prob (ratio 1 at the first epoch)", 1e-5)
    value = nets.critic_value(nf_all[t_idx, b_idx], times[t_idx].view(M, 1), *cw).squeeze(-1)
    losses = ppo.clip_ppo_loss(lp_new, lp_roll, adv.view(-1)[idx], value, tgt.view(-1)[idx], ent)
    (losses["loss_objective"] + losses["loss_critic"] + losses["loss_entropy"]).backward()
    o = out.cpu()
    for i, k in enumerate(["loss_objective", "loss_critic", "loss_entropy"]):
        assert abs(o[i].item() - losses[k].item()) <= 1e-4 * max(1.0, abs(losses[k].item())), k
    g = tr.last_grad
    for k in ops.GT_PARAM_KEYS:
        _close(g[slice(*_span(tr, tt[k]))].cpu().view_as(p[k]), p[k].grad, f"grad {k}")
    for n_, q in pol.transformer.named_parameters():             # what does not reach the logits gets exactly zero
        if n_ not in ops.GT_PARAM_KEYS:
            assert float(g[slice(*_span(tr, q))].abs().max()) == 0.0, n_


def test_cli_train_and_eval_with_the_graph_transformer_head(tmp_path, monkeypatch, capsys):
    import importlib
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    out = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-1025", "--rollout-steps", "8",
          "--epochs", "2", "--steps", "4", "--num-envs", "4", "--policy-head", "graph_transformer", "--output-dir",
          str(out), "--seed", "1"])
    assert "Simulation Summary" in capsys.readouterr().out
    sd = torch.load(out / "policy.pt", map_location="cpu")
    assert any(k.startswith("module.0.module.transformer.gt_layers.0.WQ") for k in sd)
    assert "module.0.module.gt_pe" in sd and sd["module.0.module.gt_pe"].shape[1] == 16
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-1025", "--steps", "3",
          "--policy-head", "graph_transformer", "--output-dir", str(tmp_path / "ev")])
    assert "Simulation Summary" in capsys.readouterr().out


def _gt_engine(net, B, A, seed=29, t1=21580):
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    pops = synth.population_batch(A, net.num_roads, B, seed=21, device="cuda", t1=t1)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.clone(), congestion_constant=net.congestion_constant, seed=seed)
    return eng, pops


@pytest.mark.parametrize("t1", [21580, 21740])
def test_rollout_gt_equals_the_frames_issued_one_at_a_time(t1):
    """tarl_fused_rollout_gt over T frames == per frame: observation, transformer logits, tarl_graphdist_rollout (sel8), the
    frame; kept observation rows, action bytes, log-probs, rewards and count bytes bit for bit. Departures in 21540 .. t1:
    about 10 agents due per frame and environment, or about 2 (tarl_insert_envs_per_wave then packs 4 environments per wave
    in the rollout; the twin's frames insert with one)."""
    from src.transformer import laplacian_pe
    from tarl_hip import ops, synth
    net = synth.torus_network(6, 5, heterogeneous=True, seed=7)
    N, B, T = net.num_roads, 96, 20
    w = ops.GtWeights({k: v.cuda().contiguous() for k, v in _random_state(3).items()
                       if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS})
    pe = laplacian_pe(net.edge_index, N, N).cuda()
    e1, _ = _gt_engine(net, B, 400, seed=11, t1=t1)
    e2, _ = _gt_engine(net, B, 400, seed=11, t1=t1)
    e1.reset()
    e2.reset()
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    P = 3
    keep = (list(range(0, (T + 1) * P, P)), torch.tensor([0, 50, B - 1] * T, dtype=torch.int32, device="cuda"),
            torch.arange(T * P, dtype=torch.int32, device="cuda"))
    obs_keep = torch.full((T * P, N, 16), float("nan"), device="cuda")
    TEMP = 50.0
    e1.rollout_gt(T, pe, w, temperature=TEMP, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp, reward=rw,
                  counts=ct, keep=keep, obs_keep=obs_keep)
    counts_f = torch.zeros((N, B), device="cuda")
    for t in range(T):
        o = ops.fused_obs16(e2.plan, e2.fs, e2._x, net.Nmax, e2.agents)
        assert torch.equal(o[[0, 50, B - 1]], obs_keep[t * P:(t + 1) * P]), t
        logits = ops.policy_gt_logits(e2.plan, o, e2.ec, pe, w)
        c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        lp2 = ops.graphdist_rollout(e2.plan, logits, TEMP, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
        e2.frame_fused(skip_choice=True, counts=counts_f)
        assert torch.equal(c8, ch[t]) and torch.equal(lp2, lp[t]), t
        assert torch.equal(counts_f, ct[t + 1].float()) and torch.equal(e2.reward, rw[t]), t
    assert float(rw.abs().sum()) > 0 and float(ct[-1].float().sum()) > 0
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)


def test_rollout_gt_oracle_replay_config4():
    """Config 4 (25 x 25 torus, 16 384 agents), B = 1 024, 32 frames of tarl_fused_rollout_gt next to the ORACLE: for probe
    environments every frame's observation is rebuilt from the oracle's own state and must equal the device's; the device's
    logits of it agree with the float64 restatement (1e-4 of their scale); the device's action bytes are checked against
    GraphDist.sample of those logits with the exported uniforms (a draw may differ only where the uniform lies within 2
    fp32 ulps of a CDF boundary); then oracle/sim.env_step advances with the device's action and Gumbel values: counts and
    rewards of every frame, final x and agents bit-exact."""
    from draw_check import CARRIED, fp32_ulp, ranks
    from oracle import dist, sim
    from src.transformer import laplacian_pe
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    A, T, B = 16384, 32, 1024
    probe = [0, 333, 1023]
    P = len(probe)
    net = synth.torus_network(25, 25)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    eng, pops = _gt_engine(net, B, A, seed=29, t1=EPISODE_START + 40)
    eng.reset()
    plan = eng.plan
    sd = _reference_state(5)
    w = ops.GtWeights({k: v.cuda().contiguous() for k, v in sd.items() if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS})
    pe = laplacian_pe(net.edge_index, N, N)
    pe_d = pe.cuda()
    # a temperature at the logits' own spread on the reset state, so that the draws are not all one-hot
    l0 = ops.policy_gt_logits(plan, ops.fused_obs16(plan, eng.fs, eng._x, Nmax, eng.agents)[:8].contiguous(), eng.ec, pe_d, w)
    TEMP = max(1.0, float(l0.std()))
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    keep = (list(range(0, (T + 1) * P, P)), torch.tensor(probe * T, dtype=torch.int32, device="cuda"),
            torch.arange(T * P, dtype=torch.int32, device="cuda"))
    obs_keep = torch.full((T * P, N, 16), float("nan"), device="cuda")
    noise0 = eng.noise_counter + 1
    eng.rollout_gt(T, pe_d, w, temperature=TEMP, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp, reward=rw,
                   counts=ct, keep=keep, obs_keep=obs_keep)
    eng.check_flags()
    dev_logits = ops.policy_gt_logits(plan, obs_keep, eng.ec, pe_d, w).cpu()
    with torch.no_grad():
        ref = R_.gt_logits({k: v.double().cuda() for k, v in sd.items()}, obs_keep.double(), net.edge_index.cuda(),
                           net.edge_attr.double().cuda(), pe.double().cuda()).cpu()
    _close(dev_logits, ref, "rollout logits against the restatement")
    pidx = torch.tensor(probe, device="cuda")
    ch_p, ct_p, lp_p, rw_p = ch[:, pidx].cpu(), ct[:, :, pidx].cpu(), lp[:, pidx].cpu(), rw[:, pidx].cpu()
    obs_p = obs_keep.cpu()
    x_fin = torch.stack([eng.x[b] for b in probe]).cpu()
    ag_fin = torch.stack([eng.agents[b] for b in probe]).cpu()
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
            gd = dist.GraphDist(dev_logits[t * P + k], net.edge_index, TEMP)
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
