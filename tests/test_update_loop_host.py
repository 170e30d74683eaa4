"""CPU: pins tests/update_loop_restatement.py (the float64 replay test_gpu_update_loop.py holds VecPPOTrainer.update() to) to
what the project already trusts, and shows without a GPU what the GPU cases can see:

* one clean replayed epoch equals oracle/ppo.py, oracle/dist.py and oracle/nets.py under torch autograd in float64 (1e-12, the
  pin of test_update_host.py), and the torch forms of the head restatements equal the restatements they stand for;
* the minibatch draws of the two draw shapes have the properties the cases exist for (numpy's Philox alone);
* on the shape, draws and head of every GPU case, each defect of ``update_loop_restatement.DEFECTS`` that restates a bug of
  code the case runs moves at least one compared quantity by more than 10x that quantity's GPU tolerance."""
import numpy as np
import pytest
import torch

import update_loop_restatement as L
import update_restatement as R

D = torch.float64


# ---- synthetic inputs of a case ------------------------------------------------------------------------------------------
def _linear(gen, n_out, n_in):
    k = 1.0 / np.sqrt(n_in)
    return [(torch.rand((n_out, n_in), generator=gen) * 2 - 1) * k, (torch.rand(n_out, generator=gen) * 2 - 1) * k]


def host_case(name):
    """The case's shape, draws, head and critic on synthetic bytes: random counts (0 after a reset), a random valid action per
    road, the queue reward of those counts, observations with the network's static columns, those counts and random head
    agents; parameters initialised like the modules' (a run of dormant floats between the critic and the head); the stored
    behaviour log-prob is the head's own at those parameters. -> (spec, rollout, draws, theta0, obs_of)."""
    import goal_mlp_restatement as G
    from tarl_hip import synth
    c = L.CASES[name]
    T, B, M = c["T"], c["B"], c["M"]
    net = synth.torus_network(*c["torus"], heterogeneous=True, seed=2)
    N, ei = net.num_roads, net.edge_index
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    done = L.done_frames(T, c["timestep"])
    counts = torch.randint(0, 4, (T + 1, B, N), generator=gen).double()
    times = [21540.0]
    for t in range(T):
        if bool(done[t]) and t + 1 < T:
            counts[t + 1] = 0
            times.append(21540.0)
        else:
            times.append(times[-1] + c["timestep"])
    po = R.PlanOrder(ei, N)
    q = (torch.rand((T, B, N), generator=gen) * po.deg).long().clamp(max=po.deg - 1)
    choice = po.order[po.start + q]
    obs_of = torch.from_numpy(G.random_obs(net, T * B, seed=5)).view(T, B, N, 16)
    obs_of[..., 1] = counts[:T].float()
    obs_all = torch.cat([obs_of.view(T * B, N, 16), torch.from_numpy(G.random_obs(net, B, seed=6))])
    # the flat buffer: embedding, critic, 37 dormant floats, the head's own parameters
    params, layout, off = [], {}, 0

    def add(nm, t):
        nonlocal off
        if nm is not None:
            layout[nm] = (off, tuple(t.shape))
        params.append(t.reshape(-1).double())
        off += t.numel()
    consts = {}
    add("emb" if c["head"] in ("embedding", "embedding_dijkstra") else None, torch.randn((N, 1), generator=gen))
    if c["critic"] == "simple":
        for i, t in enumerate(_linear(gen, 64, N + 1) + _linear(gen, 64, 64) + _linear(gen, 1, 64)):
            add(f"critic.{i}", t)
    else:
        import gt_cases
        from src.transformer import laplacian_pe
        from tarl_hip import ops
        sd = gt_cases._random_state(11, critic=True)
        for k in ops.GT_VALUE_PARAM_KEYS:
            add("gtv." + k, sd[k])
        consts["gtv_buffers"] = {k: sd[k].double() for k in ops.GT_VALUE_BUFFER_KEYS}
        consts["gtv_pe"] = laplacian_pe(ei, N, N).double()
    add(None, torch.randn(37, generator=gen))
    if c["head"] == "edge_mlp":
        for i, t in enumerate(_linear(gen, 64, 33) + _linear(gen, 32, 64) + _linear(gen, 1, 32)):
            add(f"edge_mlp.{i}", t)
    elif c["head"] in ("embedding_dijkstra", "goal_mlp"):
        table, S = G.free_flow_table(net)
        if c["head"] == "goal_mlp":
            add("goal", torch.from_numpy(G.weights(3)))
            consts.update(table=table, S=S)
        else:
            consts.update(table=torch.from_numpy(table).double(), w=1.0)
    elif c["head"] == "graph_transformer":
        import gt_cases
        from src.transformer import laplacian_pe
        from tarl_hip import ops
        sd = gt_cases._random_state(7)
        for k in ops.GT_PARAM_KEYS:
            add("gt." + k, sd[k])
        consts["gt_buffers"] = {k: sd[k].double() for k in ops.GT_BUFFER_KEYS}
        consts["pe"] = laplacian_pe(ei, N, N).double()
    theta0 = torch.cat(params).float().double()           # fp32 values, as the trainer's snapshot holds them
    sp = L.spec(ei=ei, ea=net.edge_attr, N=N, T=T, B=B, head=c["head"], critic=c["critic"], layout=layout, numel=off,
                temperature=c.get("temperature", 1.0), consts=consts)
    reward = -counts[1:].sum(-1)
    with torch.no_grad():
        rows = obs_of.view(T * B, N, 16)
        lg = torch.cat([L.head_logits(sp, L.views(sp, theta0), rows[i:i + 64], 64) for i in range(0, T * B, 64)])[:T * B]
        logp = R.segment_dist(lg, ei, sp.temperature, N).log_prob(choice=choice.view(T * B, N)).view(T, B)
    ro = dict(counts=counts, choice=choice, logp=logp, reward=reward, times=torch.tensor(times, dtype=D), done=done,
              obs_all=obs_all if c["critic"] != "simple" else None)
    draws = L.replay_draws(c["seed"], T * B, M, c["epochs"])
    return sp, ro, draws, theta0, obs_of


_CACHE = {}


def _clean(name):
    if name not in _CACHE:
        sp, ro, draws, theta0, obs_of = host_case(name)
        _CACHE[name] = (sp, ro, draws, theta0, obs_of, L.replay_loop(sp, ro, draws, theta0, obs_of))
    return _CACHE[name]


# ---- agreement ------------------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=D).detach(), torch.as_tensor(b, dtype=D).detach()
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("name", ["emb_frames", "emb_env_odd"])
def test_a_clean_epoch_equals_the_oracle_under_autograd(name):
    """Embedding head, simple critic, 4 x 4 torus (the second case with an episode end inside the batch): advantages,
    targets, the three losses and every gradient of a replayed epoch against oracle/ppo.py + dist.py + nets.py."""
    from oracle import dist, nets, ppo
    sp, ro, draws, theta0, _ = host_case(name)
    T, B, N, E = sp.T, sp.B, sp.N, sp.E
    idx = draws[1]
    theta = (theta0 + 0.01 * torch.randn(sp.numel, generator=torch.Generator().manual_seed(1), dtype=D))   # ratio != 1
    got = L.replay_epoch(sp, ro, theta, idx, None)
    th = theta.clone().requires_grad_(True)
    P = L.views(sp, th)
    cw = [P[f"critic.{i}"] for i in range(6)]
    nf_all = torch.zeros((T + 1, B, N, 7), dtype=D)
    nf_all[..., 1] = ro["counts"]
    nf_all[..., 6] = torch.arange(N, dtype=D)
    with torch.no_grad():
        v = nets.critic_value(nf_all, ro["times"].view(T + 1, 1, 1).expand(T + 1, B, 1), *cw).squeeze(-1)
        dm = ro["done"].view(T, 1).expand(T, B)
        adv, tgt = ppo.gae(ro["reward"], v[:T], v[1:], dm, dm, average_gae=True)
    _close(got["adv"], adv)
    _close(got["target"], tgt)
    t_idx, b_idx = idx // B, idx % B
    onehot = torch.zeros((idx.numel(), E), dtype=torch.int64).scatter_(1, ro["choice"][t_idx, b_idx], 1)
    d = dist.GraphDist(nets.policy_logits(nf_all[t_idx, b_idx], sp.ei, P["emb"]), sp.ei)
    value = nets.critic_value(nf_all[t_idx, b_idx], ro["times"][t_idx].view(-1, 1), *cw).squeeze(-1)
    ls = ppo.clip_ppo_loss(d.log_prob(onehot), ro["logp"].view(-1)[idx], adv.view(-1)[idx], value, tgt.view(-1)[idx], d.entropy())
    (ls["loss_objective"] + ls["loss_critic"] + ls["loss_entropy"]).backward()
    _close(got["losses"], torch.stack([ls["loss_objective"], ls["loss_critic"], ls["loss_entropy"]]))
    _close(got["grad"], th.grad)
    assert float(th.grad[~L.live_mask(sp)].abs().max()) == 0.0 and float(got["grad"][L.live_mask(sp)].abs().max()) > 0
    assert got["ratio_max"] > 1e-3
    # Adam on the flat buffer is adam64, which test_update_host.py pins to the oracle
    m, v2 = torch.rand(sp.numel, dtype=D), torch.rand(sp.numel, dtype=D)
    q, mm, vv = theta.clone(), m.clone(), v2.clone()
    ppo.adam_step(q, th.grad, mm, vv, 3)
    for a, b in zip(L.apply_adam(theta, m, v2, 3, th.grad), (q, mm, vv)):
        _close(a, b)


def test_the_torch_forms_of_the_heads_equal_their_restatements():
    """goal_logits == goal_mlp_restatement.forward (float64) with torch_backward's gradient; the edge-MLP head through
    oracle/nets.py == edge_mlp_restatement.logits64."""
    import edge_mlp_restatement as EM
    import goal_mlp_restatement as G
    sp, ro, draws, theta0, obs_of = host_case("goal_B")
    obs = obs_of.view(-1, sp.N, 16)[:5]
    w = L.views(sp, theta0)["goal"].clone().requires_grad_(True)
    lg = L.goal_logits(obs.numpy(), sp.ei, sp.consts["table"], sp.consts["S"], w)
    want = G.forward(obs.numpy(), sp.ei.numpy(), sp.consts["table"], sp.consts["S"], w.detach().float().numpy(), dt=np.float64)
    _close(lg, torch.from_numpy(want))
    gl = torch.randn(lg.shape, generator=torch.Generator().manual_seed(2), dtype=D)
    (lg * gl).sum().backward()
    _close(w.grad, torch.from_numpy(G.torch_backward(obs.numpy(), sp.ei.numpy(), sp.consts["table"], sp.consts["S"],
                                                     w.detach().float().numpy(), gl.numpy())))
    sp, ro, draws, theta0, obs_of = host_case("edge_mlp_B")
    obs = obs_of.view(-1, sp.N, 16)[:5]
    P = L.views(sp, theta0)
    _close(L.head_logits(sp, P, obs), EM.logits64(obs, sp.ei, sp.ea, [P[f"edge_mlp.{i}"] for i in range(6)]))


# ---- the draws ------------------------------------------------------------------------------------------------------------
def _numpy_draws(shape):
    rng = np.random.Generator(np.random.Philox(key=shape["seed"]))
    n = shape["T"] * shape["B"]
    return [rng.choice(n, size=shape["M"], replace=False, shuffle=True).astype(np.int64) for _ in range(shape["epochs"])]


def test_draw_shape_a_leaves_a_segment_without_a_kept_row_and_keeps_rows_on_both_sides_of_a_reset():
    s = L.SHAPE_A
    draws = _numpy_draws(s)
    assert all(np.array_equal(a, b.numpy()) for a, b in zip(draws, L.replay_draws(s["seed"], s["T"] * s["B"], s["M"], s["epochs"])))
    done = L.done_frames(s["T"], s["timestep"])
    assert done.nonzero().flatten().tolist() == [12, 25]              # 13 + 13 + 2 frames at 300-s steps
    segs = L.segments(done)
    assert segs == [(0, 13), (13, 26), (26, 28)]
    frames = np.concatenate(draws) // s["B"]
    per = [int(((frames >= lo) & (frames < hi)).sum()) for lo, hi in segs]
    assert per[0] > 0 and per[1] > 0 and per[2] == 0, per
    assert sum(per) == s["M"] * s["epochs"]
    rows, got = L.kept_rows([torch.from_numpy(d) for d in draws], s["B"], done,
                            torch.zeros((s["T"], s["B"], 1, 1)))
    assert got == per


def test_draw_shape_b_repeats_pairs_across_epochs_and_keeps_the_first_and_the_last_frame():
    s = L.SHAPE_B
    draws = _numpy_draws(s)
    flat = np.concatenate(draws)
    assert flat.size > s["T"] * s["B"]                                   # more draws than (frame, environment) pairs
    uniq, cnt = np.unique(flat, return_counts=True)
    assert int((cnt == 2).sum()) > 0 and int((cnt == s["epochs"]).sum()) > 0 and s["epochs"] == 3
    assert all(np.unique(d).size == d.size for d in draws)               # (never twice within an epoch)
    frames = flat // s["B"]
    assert 0 in frames and s["T"] - 1 in frames
    assert not bool(L.done_frames(s["T"], s["timestep"]).any())
    # a repeated pair sits at two slots of the concatenated draws: the stable sort keeps both, in draw order
    order = np.argsort(flat, kind="stable")
    rep = uniq[cnt >= 2][0]
    slots = order[flat[order] == rep]
    assert slots.size >= 2 and list(slots) == sorted(slots)


# ---- the defects ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CASES))
def test_every_case_notices_every_defect_of_the_code_it_runs(name):
    """Teacher-forced like the GPU test: the defective epoch starts from the clean chain's state. A defect must move a
    quantity that is compared within a tolerance (advantages, targets, losses, a gradient slice, a parameter or a moment) by
    more than 10x it; the defects of the kept buffer itself must change a kept row as well (those are compared bit for bit)."""
    sp, ro, draws, theta0, obs_of, clean = _clean(name)
    assert len(clean) == L.CASES[name]["epochs"] >= 2
    for c in clean:         # the clean chain itself: live gradients, a ratio that leaves 1 after the first step
        assert float(c["grad"][~L.live_mask(sp)].abs().max()) == 0.0 and float(c["grad"].abs().max()) > 0
    assert clean[1]["ratio_max"] > 0 and bool(torch.isfinite(clean[-1]["theta"]).all())
    seen = []
    for defect in L.DEFECTS:
        if not L.applicable(name, defect):
            continue
        bad = L.replay_loop(sp, ro, draws, theta0, obs_of, defect=defect)
        ratio = L.moved(clean, bad, sp)
        rows = ratio.pop("rows", None)
        worst = max(ratio, key=ratio.get)
        assert ratio[worst] > 10.0, (name, defect, worst, ratio[worst])
        if defect in ("obs_unsorted", "segment_shift"):      # (a wrong offset reads right rows of the wrong epoch: the
            assert rows == 1.0, (name, defect)                # buffer itself is intact, only the replay can see it)
        seen.append(defect)
    assert {"stale_advantages", "adam_step_stuck"} <= set(seen)


def test_every_defect_is_shown_on_some_case():
    for defect in L.DEFECTS:
        assert any(L.applicable(n, defect) for n in L.CASES), defect
    with pytest.raises(ValueError):
        L.replay_epoch(None, None, None, None, None, defect="nonsense")
