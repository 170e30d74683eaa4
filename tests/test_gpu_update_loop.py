"""GPU: the multi-epoch PPO update of VecPPOTrainer — ``update()``: per epoch ``advantages()`` with the current critic, then
``minibatch_step()`` — for every policy head and critic, WITHOUT test hooks (``obs_idx`` stays None: the real minibatch draw,
the concatenation of all epochs' draws, the stable sort into the kept rows, the per-epoch offset, the split over episode
segments, Adam steps 2 and 3), against tests/update_loop_restatement.py.

Per case two identical trainers on twin engines: A runs ``collect()`` + ``update()``; B runs ``collect()`` and the loop written
out here, with a snapshot of the flat buffer, both moments and the step number in front of every epoch. Four checks:

1. A's final parameters, moments and step equal B's bit for bit (pins ``update()`` to the loop the replay follows);
2. every kept observation row equals the observation of its (frame, environment) pair, rebuilt on a third engine that is
   stepped frame by frame under the stored action bytes (bit for bit; ``obs_all`` for the graph-transformer critic);
3. every epoch, TEACHER-FORCED from B's snapshot: advantages, value targets, the three losses and every gradient slice
   against the float64 replay, within the tolerance of that head's one-epoch update test; dormant parameters exactly 0;
4. every epoch's Adam step: ``adam64`` on the GPU's own gradient and snapshot moments with step k + 1 against the next
   snapshot, within ``tensor_bound(e32, ref)`` and within the 1e-7 + 1e-6 |x| of the kernel's own test.

test_update_loop_host.py shows without a GPU that each case notices every defect of ``update_loop_restatement.DEFECTS``
that the code it runs could have. Measured figures: DESIGN.md §5."""
import types

import numpy as np
import pytest
import torch

import update_loop_restatement as L
import update_restatement as R

pytestmark = pytest.mark.gpu
CASES = list(L.CASES)


# ---- the trainers -------------------------------------------------------------------------------------------------------
def _engine(net, pops, c):
    from tarl_hip.engine import SimEngine
    B = c["B"]
    return SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                     pops.clone().cuda(), congestion_constant=net.congestion_constant, seed=3, timestep=c["timestep"])


def _trainer_case(name):
    """-> (net, populations, make) with make() a NEW trainer on a NEW engine, identical every time: namespace(tr, eng, layout, consts)."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import ops, synth
    from tarl_hip.trainer import VecPPOTrainer
    c = L.CASES[name]
    net = synth.torus_network(*c["torus"], heterogeneous=True, seed=2)
    N, B, T = net.num_roads, c["B"], c["T"]
    A = 300 if B > 6 else 200
    t1 = 23000 if c["timestep"] == 300 else 21552           # 300-s steps: departures over the first 5 frames of an episode
    pops = torch.stack([synth.population(A, N, seed=40 + b, t0=21540, t1=t1) for b in range(B)])
    head = c["head"]

    def make():
        eng = _engine(net, pops, c)
        torch.manual_seed(1)
        ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()
        pol = MPNNPolicyNet(net.edge_index, N, ff if head in ("embedding_dijkstra", "goal_mlp") else None, device="cuda")
        kw, consts, named = {}, {}, {}
        if head == "edge_mlp":
            m = pol.edge_mlp
            mlp = [m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]
            kw.update(policy="edge_mlp", edge_mlp_params=mlp, policy_precision="fp32")
            named.update({f"edge_mlp.{i}": p for i, p in enumerate(mlp)})
        elif head == "embedding_dijkstra":
            kw.update(policy="embedding_dijkstra")
            if c.get("per_dest"):
                from src.agents.base import destination_set
                pol.prior_method = "per_destination"
                kw.update(prior_free_flow=pol.free_flow_weights(), prior_dests=destination_set(eng.agents, N))
            else:
                kw.update(prior_table=pol.dist_matrix)
            named["emb"] = pol.nodes_embedding.weight
        elif head == "goal_mlp":
            pol.prior_method = "all_pairs"
            pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * net.Nmax:]))
            gm = pol.goal_mlp
            with torch.no_grad():       # pre-activations on both sides of 0 (test_gpu_goal_mlp.py's trainer case)
                gm[0].bias.uniform_(-0.3, 0.3)
                gm[0].weight.uniform_(-1.0, 1.0)
            kw.update(policy="goal_mlp", goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias],
                      prior_table=pol.dist_matrix)
            if c.get("rules"):
                kw.update(policy_hold=True, route_departures=True, reward="trip")
        elif head == "graph_transformer":
            import gt_cases
            from src.transformer import laplacian_pe
            pol.use_graph_transformer(laplacian_pe(net.edge_index, N, N))
            # scaled random weights (gt_cases): the reference's initialisation on raw observations leaves the ratio of the
            # second epoch beyond exp(60)
            pol.transformer.load_state_dict({k: v.cuda() for k, v in gt_cases._random_state(7).items()})
            tt = pol.transformer.kernel_tensors()
            kw.update(policy="graph_transformer", gt_params=tt, gt_pe=pol.gt_pe)
            named.update({"gt." + k: tt[k] for k in ops.GT_PARAM_KEYS})
            consts.update(gt_buffers={k: tt[k].detach().cpu().double() for k in ops.GT_BUFFER_KEYS}, pe=pol.gt_pe.cpu().double())
        else:
            kw.update(rollout=c["rollout"], lazy_log_prob=bool(c.get("lazy")))
            named["emb"] = pol.nodes_embedding.weight
        if c["critic"] == "simple":
            l = MPNNValueNetSimple(net.edge_index, N, device="cuda").final_mlp
            crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
            named.update({f"critic.{i}": p for i, p in enumerate(crit)})
        else:
            import gt_cases
            from src.agents.transformer_agent import ValueNet
            val = ValueNet(net.edge_index, N, "cuda", pol.gt_pe)
            val.transformer.load_state_dict({k: v.cuda() for k, v in gt_cases._random_state(11, critic=True).items()})
            crit = list(val.transformer.parameters())
            vt = val.kernel_tensors()
            kw.update(value="graph_transformer", gt_value_params=vt, gt_value_pe=val.gt_pe)
            named.update({"gtv." + k: vt[k] for k in ops.GT_VALUE_PARAM_KEYS})
            consts.update(gtv_buffers={k: vt[k].detach().cpu().double() for k in ops.GT_VALUE_BUFFER_KEYS},
                          gtv_pe=val.gt_pe.cpu().double())
        extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
        tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=c["epochs"], sub_batch_size=c["M"],
                           extra_params=extra, temperature=c.get("temperature", 1.0), seed=c["seed"], **kw)
        assert tr.obs_idx is None and tr.rank == 0
        layout = {k: (tr.flat.offsets[id(p)][0], tuple(p.shape)) for k, p in named.items()}
        if head == "goal_mlp":
            layout["goal"] = (tr._goal_off, (ops.GOAL_MLP_PARAMS,))
            consts.update(table=pol.dist_matrix.cpu().numpy(), S=np.float32(tr.goal_scale))
        if head == "embedding_dijkstra":
            table = tr.prior_table.cpu().double()
            if tr.prior_dest_slot is not None:          # (N, D) per-destination columns -> [candidate][destination], +inf elsewhere
                slot = tr.prior_dest_slot.cpu().long()
                full = torch.full((N, N), float("inf"), dtype=torch.float64)
                full[:, slot >= 0] = table[:, slot[slot >= 0]]
                table = full
            consts.update(table=table, w=tr.prior_weight)
        return types.SimpleNamespace(tr=tr, eng=eng, layout=layout, consts=consts)
    return net, pops, make


def _snapshot(tr):
    f = tr.flat
    return types.SimpleNamespace(flat=f.flat.detach().cpu().clone(), m=f.exp_avg.cpu().clone(), v=f.exp_avg_sq.cpu().clone(),
                                 step=int(f.step))


def _rebuild(net, pops, c, tr):
    """The observation of every (frame, environment) pair, rebuilt on a third engine stepped frame by frame under the stored
    action bytes (with the environment's rules launched one by one where the case has them), a reset where ``done_frames``
    says so. -> (obs_of (T, B, N, 16) and the final observation (B, N, 16) on the CPU, rewards (T, B) as that engine gave
    them, restated rewards (T, B) from the exported agent tables for the trip reward, else None)."""
    import goal_mlp_restatement as G
    import trip_reward_restatement as TR
    from tarl_hip import ops
    e = _engine(net, pops, c)
    T, B, N = c["T"], c["B"], e.N
    e.reset()
    rules = bool(c.get("rules"))
    if rules:
        from tarl_hip.evaluator import router_buffers
        dests, slot, weights, table, scratch = router_buffers(e, None, 1)
        ops.fused_edge_travel_time(e.plan, e.fs, out=weights)
        ops.destination_trees_batched(e.plan, weights[:1], dests, out=table, scratch=scratch)
    obs_of = torch.empty((T, B, N, 16))
    rw = torch.zeros((T, B), device="cuda")
    restated = torch.zeros((T, B)) if rules else None
    done = tr.done_frames.tolist()
    kept = set(torch.cat([i.cpu() for i in tr._mb_idx]).tolist()) if tr.state_dep else set()
    for t in range(T):
        o = e.obs16()
        obs_of[t] = o.cpu()
        envs = [b for b in range(B) if t * B + b in kept]
        if envs:        # the same rows from the exported state: node columns + the head agent's row
            x, ag = e.x.cpu(), e.agents.cpu()
            for b in envs:
                assert np.array_equal(G.observations(x[b:b + 1], ag[b], net.Nmax)[0], obs_of[t, b].numpy()), (t, b)
        ops.fused_set_actions(e.plan, e.fs, tr.choice[t].clone())
        clock = float(e.time)
        if rules:
            ops.fused_hold_policy_actions(e.plan, e.fs, e.agents)
            pend = ops.fused_pending_departures(e.plan, e.fs, clock)
            ops.fused_route_departures(e.plan, e.fs, pend, slot, table[0])
        is_done = e.frame_fused(skip_choice=True, reward=rw[t])
        if rules:
            ops.fused_trip_reward(e.plan, e.fs, clock, out=rw[t])
            restated[t] = torch.from_numpy(TR.reward_batch(e.agents.cpu().numpy(), clock))
        assert bool(is_done) == done[t], t
        if is_done and t + 1 < T:
            e.reset()
    return obs_of, e.obs16().cpu(), rw.cpu(), restated


_RUNS = {}


def _run(name):
    """Both trainers, the written-out loop, the rebuilt observations and the rollout in the replay's terms, once per case."""
    if name in _RUNS:
        if isinstance(_RUNS[name], BaseException):
            raise RuntimeError(f"case {name} failed earlier") from _RUNS[name]
        return _RUNS[name]
    try:
        _RUNS[name] = _run_once(name)
    except BaseException as exc:
        _RUNS[name] = exc
        raise
    return _RUNS[name]


def _run_once(name):
    c = L.CASES[name]
    T, B, M, K = c["T"], c["B"], c["M"], c["epochs"]
    net, pops, make = _trainer_case(name)
    a, b = make(), make()
    N = a.eng.N
    assert torch.equal(a.tr.flat.flat, b.tr.flat.flat)
    a.tr.collect()
    a.tr.update()
    tr = b.tr
    tr.keep_grad = True
    tr.collect()
    assert torch.equal(a.tr.choice, tr.choice) and torch.equal(a.tr.reward, tr.reward) and torch.equal(a.tr.counts, tr.counts)
    draws = L.replay_draws(c["seed"], T * B, M, K)
    if tr.state_dep:
        assert len(tr._mb_idx) == K and all(torch.equal(i.cpu(), d) for i, d in zip(tr._mb_idx, draws))
    r = types.SimpleNamespace(name=name, c=c, snaps=[], adv=[], target=[], losses=[], grads=[], draws=draws)
    # the rollout, before any step changes the parameters
    eng = tr.eng
    choice = eng.decode_rollout(False if tr.state_dep else tr.env_minor, choice=tr.choice)[0].cpu().long()
    counts = eng.decode_rollout(tr.env_minor, counts=tr.counts)[1].cpu().double()
    r.ro = dict(counts=counts, choice=choice, logp=tr.logp.cpu().double(), reward=tr.reward.cpu().double(),
                times=tr.times.cpu().double(), done=tr.done_frames.clone(), obs_all=None)
    r.reward32 = tr.reward.cpu().clone()
    r.obs_mb = tr.obs_mb.cpu().clone() if (tr.state_dep and tr.obs_all is None) else None
    if tr.obs_all is not None:
        r.ro["obs_all"] = tr.obs_all.view(-1, N, 16).cpu().clone()
    # ---- the loop of update(), written out, with a snapshot in front of every epoch ----
    for k in range(K):
        r.snaps.append(_snapshot(tr))
        adv, tgt = tr.advantages()
        r.adv.append(adv.cpu().clone())
        r.target.append(tgt.cpu().clone())
        out = tr.minibatch_step(adv, tgt)
        r.losses.append(out.cpu().clone())
        r.grads.append(tr.last_grad.cpu())
    r.snaps.append(_snapshot(tr))
    r.final_a = _snapshot(a.tr)
    tr.check_flags()
    a.tr.check_flags()
    r.sp = L.spec(ei=net.edge_index, ea=net.edge_attr, N=N, T=T, B=B, head=c["head"], critic=c["critic"], layout=b.layout,
                  numel=tr.flat.numel, temperature=tr.temperature, consts=b.consts, gamma=tr.gamma, lmbda=tr.lmbda,
                  clip_epsilon=tr.clip_epsilon, entropy_coef=tr.entropy_coef, critic_coef=tr.critic_coef, lr=tr.lr)
    if c.get("lazy"):       # the behaviour log-prob is recomputed from the rollout-time embedding: the exact one
        with torch.no_grad():
            lg = L.head_logits(r.sp, L.views(r.sp, r.snaps[0].flat.double()), None, 1)
            r.ro["logp"] = R.segment_dist(lg, net.edge_index, tr.temperature, N).log_prob(choice=choice.view(T * B, N)).view(T, B)
    r.obs_of = r.obs_last = r.twin_reward = r.restated_reward = None
    if tr.state_dep:
        r.obs_of, r.obs_last, r.twin_reward, r.restated_reward = _rebuild(net, pops, c, tr)
    del a, b, tr
    return r


def _epoch_obs(r, k):
    """Epoch k's observations for the replay: the REBUILT ones of its pairs (nothing the trainer kept)."""
    if r.obs_of is None:
        return None
    idx = r.draws[k]
    return r.obs_of[idx // r.c["B"], idx % r.c["B"]]


def _report(name, k, what, err, bound):
    print(f"LOOP {name} epoch {k} {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else float('inf'):.3f}")


# ---- 1. update() is the loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_update_equals_the_loop_written_out_bit_for_bit(name):
    r = _run(name)
    last = r.snaps[-1]
    assert r.final_a.step == last.step == r.c["epochs"]
    assert [s.step for s in r.snaps] == list(range(r.c["epochs"] + 1))
    assert torch.equal(r.final_a.flat, last.flat), "parameters"
    assert torch.equal(r.final_a.m, last.m) and torch.equal(r.final_a.v, last.v), "moments"
    assert not torch.equal(r.snaps[0].flat, last.flat)
    assert r.ro["done"].tolist() == L.done_frames(r.c["T"], r.c["timestep"]).tolist()
    assert float(r.ro["reward"].abs().sum()) > 0


# ---- 2. the kept observations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if L.CASES[n]["head"] != "embedding"])
def test_kept_rows_are_the_observations_of_their_pairs(name):
    r = _run(name)
    c, B = r.c, r.c["B"]
    assert torch.equal(r.twin_reward, r.reward32), "the third engine did not follow the rollout"
    if c.get("rules"):      # the trip reward, restated from the exported agent tables: the float64 GAE reads a checked reward
        assert torch.equal(r.restated_reward, r.reward32) and float(r.reward32.abs().sum()) > 0
    if r.obs_mb is None:    # the graph-transformer critic's store: row t * B + b, and frame T from the final state
        store = r.ro["obs_all"].view(c["T"] + 1, B, *r.obs_of.shape[2:])
        assert torch.equal(store[:c["T"]], r.obs_of) and torch.equal(store[c["T"]], r.obs_last)
        return
    flat = torch.cat(r.draws)
    order = torch.argsort(flat, stable=True)            # as _draw_minibatch_frames sorts: row order[p] holds sorted pair p
    assert r.obs_mb.size(0) == flat.numel()
    for p in range(flat.numel()):
        pair = int(flat[order[p]])
        assert torch.equal(r.obs_mb[order[p]], r.obs_of[pair // B, pair % B]), (p, pair)
    off = 0
    for k, idx in enumerate(r.draws):
        assert torch.equal(r.obs_mb[off:off + idx.numel()], _epoch_obs(r, k)), f"epoch {k}"
        off += idx.numel()
    uniq, cnt = torch.unique(flat, return_counts=True)
    for pair in uniq[cnt > 1].tolist():                  # a pair drawn in several epochs holds the same row at every slot
        slots = (flat == pair).nonzero().flatten().tolist()
        assert all(torch.equal(r.obs_mb[slots[0]], r.obs_mb[s]) for s in slots[1:]), pair
    # the draw properties the case exists for, on the draws the trainer actually made
    frames = flat // B
    per = L.kept_rows(r.draws, B, r.ro["done"], torch.zeros((c["T"], B, 1, 1)))[1]
    if c["timestep"] == 300:
        assert len(per) == 3 and per[0] > 0 and per[1] > 0 and per[2] == 0, per
    else:
        assert int((cnt == c["epochs"]).sum()) > 0 and 0 in frames and c["T"] - 1 in frames
    assert float(r.obs_mb[:, :, 1].sum()) > 0 and len({float(x) for x in r.obs_mb[:, :, 1].sum(1)}) > 2      # live, distinct


# ---- 3. every epoch against the float64 replay ---------------------------------------------------------------------------
def _grad_bound(ref64, ref32):
    """1e-4 of the slice's scale (``close`` of the one-epoch tests); with the graph-transformer critic the two-term rule of
    test_gpu_gt_value.py: or 16 x plain fp32 autograd's own distance from float64."""
    b = L.TOL * max(1.0, float(ref64.abs().max()))
    return b if ref32 is None else max(b, 16.0 * R.max_err(ref32, ref64))


@pytest.mark.parametrize("name", CASES)
def test_every_epoch_equals_the_float64_replay(name):
    r = _run(name)
    sp, live = r.sp, L.live_mask(r.sp)
    for k in range(r.c["epochs"]):
        theta = r.snaps[k].flat.double()
        ref = L.replay_epoch(sp, r.ro, theta, r.draws[k], _epoch_obs(r, k))
        ref32 = L.replay_epoch(sp, r.ro, theta, r.draws[k], _epoch_obs(r, k), dtype=torch.float32) \
            if sp.critic != "simple" else None
        checks = []
        for what, got, want in (("adv", r.adv[k], ref["adv"]), ("target", r.target[k], ref["target"])):
            checks.append((what, R.max_err(got, want), L.TOL * max(1.0, float(want.abs().max()))))
        for i, what in enumerate(("loss_objective", "loss_critic", "loss_entropy")):
            checks.append((what, abs(float(r.losses[k][i]) - float(ref["losses"][i])),
                           L.TOL * max(1.0, abs(float(ref["losses"][i])))))
        g = r.grads[k]
        for nm, (off, shape) in sp.layout.items():
            sl = slice(off, off + int(np.prod(shape)))
            checks.append((f"grad {nm}", R.max_err(g[sl], ref["grad"][sl]),
                           _grad_bound(ref["grad"][sl], None if ref32 is None else ref32["grad"][sl])))
        for what, err, bound in checks:
            _report(name, k, what, err, bound)
        for what, err, bound in checks:
            assert err <= bound, (name, k, what, err, bound)
        assert float(g[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, "dormant parameters receive no gradient"
        assert float(g[live].abs().max()) > 0 and float(ref["grad"][~live].abs().max() if bool((~live).any()) else 0.0) == 0.0
        if k > 0:       # the later epochs are off-policy: the ratio has left 1
            assert ref["ratio_max"] > 1e-6, (k, ref["ratio_max"])


# ---- 4. Adam, on the GPU's own gradient -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_every_adam_step_continues_the_moments_with_its_step_number(name):
    r = _run(name)
    for k in range(r.c["epochs"]):
        s0, s1 = r.snaps[k], r.snaps[k + 1]
        assert s0.step == k and s1.step == k + 1
        for (what, ref, bound), got in zip(L.adam_bounds(s0.flat, s0.m, s0.v, k + 1, r.grads[k], r.sp.lr), (s1.flat, s1.m, s1.v)):
            err = R.max_err(got, ref)
            _report(name, k, f"adam {what}", err, bound)
            assert err <= bound, (name, k, what, err, bound)
            # and never above what the kernel's own test allows (test_gpu_update_fp64.py: 1e-7 + 1e-6 |x| per element)
            assert torch.allclose(got.double(), ref, rtol=1e-6, atol=1e-7), (name, k, what, "1e-7 + 1e-6 |x|")
        assert not torch.equal(s0.flat, s1.flat)
