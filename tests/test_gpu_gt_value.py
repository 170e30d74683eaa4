"""GPU: the graph-transformer critic (csrc/gt_value.hip) against the reference's golden and the CPU restatement — forward,
deterministic backward, the trainer's observation store and GAE values, PPO steps with the critic, the budget refusal and
the CLI end to end."""
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

sys.path.insert(0, PKG)
import gt_restatement as R_  # noqa: E402
import gt_value_restatement as RV  # noqa: E402
import gt_cases as H  # noqa: E402  (graphs, observations, summation bound shared with the policy head's tests)

pytestmark = pytest.mark.gpu

EDGE_SIDE = ("edge_emb.", ".WE.", ".WOe.", ".ffn_e.", ".norm1e.", ".norm2e.", ".e_gate.", "edge_linear.", "log_var_mlp.")


def _golden():
    z = np.load(f"{ROOT}/tests/golden/gt_value.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _weights(sd):
    from tarl_hip import ops
    t = {k: v.cuda().float().contiguous() for k, v in sd.items() if k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS}
    return t, ops.GtValueWeights(t)


def _grads(plan, obs, pe, w, coef):
    from tarl_hip import ops
    grads = [torch.zeros_like(p) for p in w.params]
    ops.value_gt_backward(plan, obs, pe, w, coef, grads)
    return grads


def test_forward_and_backward_match_the_reference_golden():
    from tarl_hip import ops
    g = _golden()
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd/")}
    N = g["pe"].size(0)
    plan = ops.Plan(g["edge_index"], N)
    _, w = _weights(sd)
    pe = g["pe"].cuda().contiguous()
    xb = g["x_batch"].cuda().contiguous()
    v1 = ops.value_gt_forward(plan, xb, pe, w)
    H._close(v1.cpu(), g["value_batch"], "value")
    assert torch.equal(v1, ops.value_gt_forward(plan, xb, pe, w)), "value not bit-reproducible"
    coef = g["coef"].cuda().contiguous()
    g1, g2 = _grads(plan, xb, pe, w, coef), _grads(plan, xb, pe, w, coef)
    for k, a, b in zip(ops.GT_VALUE_PARAM_KEYS, g1, g2):
        assert torch.equal(a, b), f"{k}: not bit-reproducible"
        H._close(a.cpu(), g["grad/" + k], f"grad {k}")
    for k, v in g.items():         # what the kernels do not take gets exactly zero from the reference too: the edge side
        if k.startswith("grad/") and k[5:] not in ops.GT_VALUE_PARAM_KEYS:
            assert any(s in "." + k[5:] for s in EDGE_SIDE) and float(v.abs().max()) == 0.0, k


CASES = [("torus8", 1, "random"), ("torus16", 7, "random"), ("config4", 1, "reference"), ("config4", 7, "random"),
         ("config4", 64, "reference"), ("matsim", 1, "reference"), ("matsim", 7, "random"), ("matsim", 64, "random")] + H.ATTENTION_CASES


def _check_case(c, ops, plan, w):
    """The kernel's values and gradients on case ``c`` against its two restatement references; returns (value, grads)."""
    sharp = c.weights == "sharp"
    if sharp:      # before a kernel is called: the attention of these inputs is neither uniform nor one-hot, and the layer-1
        H.check_census(H.attention_census(c.sd, c.obs, c.ei, c.pe, True), True)      # scores overflow expf without the max
    obs, pe = c.obs.cuda().contiguous(), c.pe.cuda()
    value = ops.value_gt_forward(plan, obs, pe, w)
    # (the sharp cases' references on the CPU, where test_gt_attention_host.py proves what their tolerance can see)
    ref64, ref32, g64, g32, S = H.references(c, "cpu" if sharp else "cuda")
    if sharp:
        err, tol = float((value.cpu().double() - ref64).abs().max()), H.sharp_tolerance(ref64, ref32)
        print(f"{c.kind} M={c.M} value: |kernel - f64| {err:.3e}, |fp32 - f64| {float((ref32 - ref64).abs().max()):.3e}, tol {tol:.3e}")
        assert err <= tol, f"value: {err} > {tol}"
    else:
        H._close(value.cpu(), ref64, "value")
    grads = _grads(plan, obs, pe, w, c.coef.cuda())
    for k, gk in zip(ops.GT_VALUE_PARAM_KEYS, grads):
        err = (gk.cpu().double() - g64[k]).abs()
        allow = H.grad_allowance(k, g64, g32, S, c)
        assert bool((err <= allow).all()), f"grad {k}: worst err / allowance {float((err / allow.clamp(min=1e-300)).max())}"
    return value, grads


@pytest.mark.parametrize("kind,M,weights", CASES)
def test_forward_and_backward_match_the_restatement(kind, M, weights, tmp_path):
    """Raw observations, the reference's initialisation, scaled random or sharp weights, on tori, config 4, a MATSim grid
    with SRC / DEST pseudo-nodes and the irregular road graphs MIXED and HUB126 (edge lists in no order, degrees 0 - 9 and up
    to 126). Values to 1e-4 of their scale against float64 — the sharp cases, after their inputs passed the attention census,
    within 16 x the fp32 restatement's own distance from float64 + 8 ulps of their scale (measured on an MI355X: DESIGN.md
    §4.11a); gradients within the policy tests' two-term bound (16 x plain fp32 autograd's error + the kernel's summation
    bound); the edge side is not in the kernel's list."""
    from tarl_hip import ops
    c = H.case_inputs(kind, M, weights, True, tmp_path)
    plan = ops.Plan(c.ei, c.N)
    if kind in H.IRREGULAR_MAX_DEGREE:
        mx_in, mx_out, in0, out0, _ = H.graph_facts(c.ei, c.N)
        assert not plan.src_sorted and mx_in == mx_out == H.IRREGULAR_MAX_DEGREE[kind] and in0 > 0 and out0 > 0
        assert (plan.max_in, plan.max_out) == (mx_in, mx_out)
    _check_case(c, ops, plan, _weights(c.sd)[1])


def test_sharp_mixed_case_is_reproducible_and_independent_of_the_edge_order(tmp_path):
    """("MIXED", 3, "sharp"): two backward calls give the same bits; and the same graph with its edge list in another order
    that keeps every node's in- and out-edges in their relative order gives bit-identical values and gradients: the plan
    sorts both segments by edge id, so every walk adds the same terms in the same order, and every weight gradient of the
    critic is a sum over node or sample records, which an edge order does not touch."""
    from tarl_hip import ops
    c = H.case_inputs("MIXED", 3, "sharp", True, tmp_path)
    plan = ops.Plan(c.ei, c.N)
    _, w = _weights(c.sd)
    value, grads = _check_case(c, ops, plan, w)
    obs, pe = c.obs.cuda().contiguous(), c.pe.cuda()
    for k, a, b in zip(ops.GT_VALUE_PARAM_KEYS, grads, _grads(plan, obs, pe, w, c.coef.cuda())):
        assert torch.equal(a, b), f"{k}: not bit-reproducible"
    order = H.order_preserving_shuffle(c.ei, seed=1)
    assert int((order != torch.arange(c.E)).sum()) > c.E // 2
    plan2 = ops.Plan(c.ei[:, order].contiguous(), c.N)
    assert torch.equal(ops.value_gt_forward(plan2, obs, pe, w), value)
    for k, a, b in zip(ops.GT_VALUE_PARAM_KEYS, grads, _grads(plan2, obs, pe, w, c.coef.cuda())):
        assert torch.equal(a, b), f"{k}: depends on the edge order"


def test_value_net_unbatched_call_is_the_batched_one_at_m1():
    from src.agents.transformer_agent import ValueNet
    from src.transformer import laplacian_pe
    from tarl_hip import synth
    net = synth.torus_network(8, 8, heterogeneous=True, seed=2)
    N = net.num_roads
    torch.manual_seed(5)
    v = ValueNet(net.edge_index, N, "cuda", laplacian_pe(net.edge_index, N, N))
    v.agent_features = synth.population(300, N, seed=1).cuda()
    nf = net.x[:, 3 * net.Nmax:3 * net.Nmax + 7].cuda().contiguous()
    ai = torch.randint(0, 300, (N,), generator=torch.Generator().manual_seed(2)).cuda()
    ef = net.edge_attr.cuda()
    single = v(nf, ef, ai, torch.zeros(1, device="cuda"))
    batched = v(nf.unsqueeze(0), ef.unsqueeze(0), ai.unsqueeze(0), torch.zeros(1, 1, device="cuda"))
    assert single.shape == (1, 1) and batched.shape == (1, 1)
    assert torch.equal(single, batched)
    v.train()
    with pytest.raises(RuntimeError, match="evaluation mode"):
        v(nf, ef, ai, torch.zeros(1, device="cuda"))


def _trainer(net, B, T, M, policy="graph_transformer", timestep=1, seed=3):
    """Trainer with the graph-transformer critic on a torus; returns (trainer, policy net, value net, engine)."""
    from src.agents.mpnn_agent import MPNNPolicyNet
    from src.agents.transformer_agent import ValueNet
    from src.transformer import laplacian_pe
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    N = net.num_roads
    pops = torch.stack([synth.population(600, N, seed=b, t0=21540, t1=21550) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=seed, timestep=timestep)
    torch.manual_seed(0)
    pe = laplacian_pe(net.edge_index, N, N)
    pol = MPNNPolicyNet(net.edge_index, N, None, device="cuda")
    if policy == "graph_transformer":
        pol.use_graph_transformer(pe)
    val = ValueNet(net.edge_index, N, "cuda", pe)
    m = pol.edge_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, list(val.transformer.parameters()), rollout_steps=T,
                       num_epochs=1, sub_batch_size=M, extra_params=extra, policy=policy, temperature=500.0,
                       edge_mlp_params=[m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias],
                       gt_params=pol.transformer.kernel_tensors() if policy == "graph_transformer" else None,
                       gt_pe=getattr(pol, "gt_pe", None), value="graph_transformer",
                       gt_value_params=val.kernel_tensors(), gt_value_pe=val.gt_pe)
    return tr, pol, val, eng


def test_store_rows_equal_the_observations_frame_by_frame_and_feed_gae():
    """Every stored row (frames 0..T, an episode end inside the batch) equals tarl_fused_obs16 issued frame by frame on a
    second engine; the values GAE uses equal the kernel forward on those rows."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_END
    net = synth.torus_network(8, 8, heterogeneous=True, seed=2)
    B, T = 64, 16
    tr, pol, val, eng = _trainer(net, B, T, 16, timestep=300)
    tr.collect()
    assert bool(tr.done_frames.any()) and not bool(tr.done_frames[-1]), "the batch must hold an episode end inside it"
    tr2, _, _, eng2 = _trainer(net, B, T, 16, timestep=300)
    w = ops.GtWeights(pol.transformer.kernel_tensors())
    N = eng.N
    eng2.reset()
    ch, lp, rw = (torch.zeros((1, B, N), dtype=torch.uint8, device="cuda"), torch.zeros((1, B), device="cuda"),
                  torch.zeros((1, B), device="cuda"))
    cnt = torch.zeros((2, N, B), dtype=torch.uint8, device="cuda")
    for t in range(T):
        assert torch.equal(eng2.obs16(), tr.obs_all[t]), f"frame {t}"
        eng2.rollout_gt(1, pol.gt_pe, w, temperature=500.0, policy_seed=tr.seed ^ 0x5DEECE66D, policy_counter0=t + 1,
                        choice8=ch, log_prob=lp, reward=rw, counts=cnt, check=False)
        assert torch.equal(lp[0], tr.logp[t]) and torch.equal(rw[0], tr.reward[t])
        if eng2.time > EPISODE_END and t + 1 < T:
            eng2.reset()
    assert torch.equal(eng2.obs16(), tr.obs_all[T]), "frame T"
    tr.advantages()
    v = ops.value_gt_forward(eng.plan, tr.obs_all.view(-1, N, 16), val.gt_pe, ops.GtValueWeights(val.kernel_tensors()))
    assert torch.equal(tr.values.reshape(-1), v)


def _value_loss_grads(tr, pol, val, net, policy, idx, dt):
    """Restatement autograd (in ``dt``) of the PPO loss of one minibatch step with the graph-transformer critic (the
    policy's logits from the restatement for the graph-transformer head, else the trainer's own fp32 logits as constants)."""
    from oracle import dist, ppo
    from tarl_hip import ops
    T, B, N, E = tr.T, tr.eng.B, net.num_roads, net.edge_index.size(1)
    M = idx.numel()
    obs = tr.obs_all.view(-1, N, 16).cpu().to(dt)
    pv = {k: (v.detach().cpu().to(dt).requires_grad_(True) if k in ops.GT_VALUE_PARAM_KEYS else v.detach().cpu().to(dt))
          for k, v in val.kernel_tensors().items()}
    pe = val.gt_pe.cpu().to(dt)
    with torch.no_grad():
        v_all = torch.cat([RV.gt_value(pv, obs[i:i + 512], net.edge_index, pe) for i in range(0, obs.size(0), 512)])
        v_all = v_all.view(T + 1, B)
        done = tr.done_frames.view(T, 1).expand(T, B)
        adv, tgt = ppo.gae(tr.reward.cpu().to(dt), v_all[:T], v_all[1:], done, done, average_gae=True)
    choice = tr.eng.decode_rollout(False, choice=tr.choice)[0].cpu()
    t_idx, b_idx = idx // B, idx % B
    onehot = torch.zeros((M, E), dtype=torch.int64)
    onehot.scatter_(1, choice[t_idx, b_idx].long(), 1)
    pp = None
    if policy == "graph_transformer":
        pp = {k: (v.detach().cpu().to(dt).requires_grad_(True) if k in ops.GT_PARAM_KEYS else v.detach().cpu().to(dt))
              for k, v in pol.transformer.kernel_tensors().items()}
        logits = R_.gt_logits(pp, obs[idx], net.edge_index, net.edge_attr.to(dt), pol.gt_pe.cpu().to(dt))
    else:
        with torch.no_grad():
            logits = ops.policy_edge_mlp(tr.eng.plan, tr.obs_all.view(-1, N, 16).index_select(0, idx.cuda()), tr.eng.ec,
                                         tr._edge_mlp()).cpu().to(dt)
    d = dist.GraphDist(logits, net.edge_index, tr.temperature)
    lp_new, ent = d.log_prob(onehot), d.entropy()
    value = RV.gt_value(pv, obs[idx], net.edge_index, pe)
    losses = ppo.clip_ppo_loss(lp_new, tr.logp.view(-1).cpu().to(dt)[idx], adv.view(-1)[idx], value, tgt.view(-1)[idx], ent)
    (losses["loss_objective"] + losses["loss_critic"] + losses["loss_entropy"]).backward()
    return losses, pv, pp


def _close2(a, g64, g32, what):
    """The step's gradient against float64 restatement autograd: within 1e-4 of its scale (the policy head's step
    tolerance) or, where the raw observations make the loss ill-conditioned at fp32, within 16 x plain fp32 autograd's own
    error (the two-term rule of the kernel tests)."""
    err = float((a.double() - g64.double()).abs().max())
    allow = max(1e-4 * max(float(g64.abs().max()), 1.0), 16 * float((g32.double() - g64.double()).abs().max()))
    assert err <= allow, f"{what}: {err} > {allow}"


@pytest.mark.parametrize("policy,T", [("graph_transformer", 16), ("edge_mlp", 4)])
def test_ppo_step_with_the_graph_transformer_critic(policy, T):
    """One minibatch step: losses and the gradients of both networks (the critic's for the edge-MLP head) match the
    restatement's autograd; the critic's edge side gets exactly zero."""
    from tarl_hip import ops, synth
    net = synth.torus_network(8, 8, heterogeneous=True, seed=2)
    B, M = 128, 32
    tr, pol, val, eng = _trainer(net, B, T, M, policy=policy)
    assert tr.rollout == ("frames+gt" if policy == "graph_transformer" else "frames+policy")
    tr.keep_grad = True
    idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(4))[:M]
    tr.obs_idx = idx
    tr.collect()
    # the parameters before the step
    losses, pv, pp = _value_loss_grads(tr, pol, val, net, policy, idx, torch.float64)
    _, pv32, pp32 = _value_loss_grads(tr, pol, val, net, policy, idx, torch.float32)
    adv, tgt = tr.advantages()
    out = tr.minibatch_step(adv, tgt).cpu()
    for i, k in enumerate(["loss_objective", "loss_critic", "loss_entropy"]):
        assert abs(out[i].item() - losses[k].item()) <= 1e-4 * max(1.0, abs(losses[k].item())), k
    g = tr.last_grad
    for k in ops.GT_VALUE_PARAM_KEYS:
        _close2(g[slice(*H._span(tr, val.kernel_tensors()[k]))].cpu().view_as(pv[k]), pv[k].grad, pv32[k].grad,
                f"critic grad {k}")
    for n_, q in val.transformer.named_parameters():
        if n_ not in ops.GT_VALUE_PARAM_KEYS:
            assert float(g[slice(*H._span(tr, q))].abs().max()) == 0.0, n_
    if pp is not None:
        for k in ops.GT_PARAM_KEYS:
            _close2(g[slice(*H._span(tr, pol.transformer.kernel_tensors()[k]))].cpu().view_as(pp[k]), pp[k].grad,
                    pp32[k].grad, f"policy grad {k}")


def test_refusals_name_their_limits():
    from tarl_hip import synth
    net = synth.torus_network(8, 8, heterogeneous=True, seed=2)
    with pytest.raises(ValueError, match=r"at most \(T \+ 1\) \* B = \d+ frames fit"):
        _trainer(net, 64, 10_000_000, 16)
    with pytest.raises(ValueError, match="state-dependent policy head"):
        _trainer(net, 8, 4, 8, policy="embedding")


def test_cli_train_and_eval_with_the_graph_transformer_critic(tmp_path, monkeypatch, capsys):
    import importlib
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    out = tmp_path / "run"
    main(["--algo", "mpnn+ppo", "--mode", "train", "--scenario", "synthetic-1024-1025", "--rollout-steps", "8",
          "--epochs", "2", "--steps", "4", "--num-envs", "4", "--policy-head", "graph_transformer", "--value-head",
          "graph_transformer", "--output-dir", str(out), "--seed", "1"])
    assert "Simulation Summary" in capsys.readouterr().out
    sd = torch.load(out / "policy.pt", map_location="cpu")
    assert any(k.startswith("module.0.module.transformer.gt_layers.0.WQ") for k in sd)
    rec = (out / "train_log.jsonl").read_text().strip().splitlines()
    assert rec and all(np.isfinite(float(__import__("json").loads(r)["loss/value"])) for r in rec)
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-1025", "--steps", "3", "--policy-head",
          "graph_transformer", "--value-head", "graph_transformer", "--output-dir", str(tmp_path / "ev")])
    assert "Simulation Summary" in capsys.readouterr().out
