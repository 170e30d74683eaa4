"""GPU: per-decision PPO credit — tarl_fused_head_rows against the exported state (packed random states of the
torus at, below and above one tile of 256 roads and of both irregular graphs, after a reset and live, B in {1, 3, 64, 65},
outputs between guard bands), the one-call rollouts with the capture switch against the same calls without it and against
the launches made one by one, tarl_decision_advantage / tarl_decision_stats / tarl_graphdist_node_logprob /
tarl_graphdist_decision_ppo against ``decision_credit_restatement`` (integers and masks ``==``, floating point within
``update_restatement.tensor_bound``), one ``train_iteration`` of ``VecPPOTrainer(credit="decision")``, the default bit for bit,
the locality case that fails without the feature, and the CLI."""
import json

import numpy as np
import pytest
import torch

import decision_credit_restatement as DC
import irregular_graphs as ig
import update_restatement as R

pytestmark = pytest.mark.gpu

GUARD = 0x7F7F7F7F
PACKED = ("hdp", "tl", "gc8", "post", "st0", "slots", "sel8", "sel", "node_rec", "in_rec", "out_pad", "a_origin", "a_dest",
          "a_dep", "a_status", "cur_lo", "flags")
GRAPHS = ["torus8x8", "torus6x5", "torus9x8", "MIXED", "HUB126"]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _net(name):
    from tarl_hip import synth
    if name.startswith("torus"):
        w, h = (int(v) for v in name[5:].split("x"))
        return synth.torus_network(w, h)
    return ig.graph(name)


def _packed_random(ops, net, B, t=200.0):
    """B random mid-simulation states (stale ids on empty roads among them) packed -> (plan, fs, exported x on the host)."""
    from tarl_hip import synth
    Nmax, N = net.Nmax, net.num_roads
    x = torch.stack([ig.random_state(net, seed=100 + b, t=t) for b in range(B)])
    A = int(x[:, :, :Nmax].max()) + 2
    ag = torch.stack([synth.population(A - 1, N, seed=b, t0=100, t1=130) for b in range(B)])
    plan = ops.Plan(net.edge_index, N)
    fs = ops.FusedState(plan, B, A, "cuda", Nmax)
    ops.fused_pack(plan, fs, x.cuda(), Nmax, ag.cuda(), net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    out = x.clone().cuda()
    ops.fused_export(plan, fs, out, Nmax, t)
    return plan, fs, out.cpu()


def _head_launch(ops, plan, fs, env, slot, rows):
    """The op into a 0x7F-filled buffer between guard bands, twice -> head_keep (rows, N) on the host; the packed state is
    compared whole before and after."""
    N, pad = plan.num_nodes, 64
    before = {k: getattr(fs, k).clone() for k in PACKED}
    outs = []
    for _ in range(2):
        big = torch.full((rows * N + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
        hk = big[pad:pad + rows * N].view(rows, N)
        ops.fused_head_rows(plan, fs, torch.tensor(env, dtype=torch.int32).cuda(), torch.tensor(slot, dtype=torch.int32).cuda(),
                            hk)
        torch.cuda.synchronize()
        assert bool((big[:pad] == GUARD).all()) and bool((big[pad + rows * N:] == GUARD).all())
        outs.append(hk.cpu())
    assert torch.equal(outs[0], outs[1])
    for k, v in before.items():
        assert torch.equal(getattr(fs, k), v), f"the kernel touched fs.{k}"
    return outs[0]


def _check_heads(hk, x_host, Nmax, env, slot, rows):
    want = torch.from_numpy(DC.heads(x_host.numpy(), Nmax)).to(torch.int32)
    written = set(slot)
    for e, s in zip(env, slot):
        assert torch.equal(hk[s], want[e]), (e, s)
    for s in range(rows):
        if s not in written:
            assert bool((hk[s] == GUARD).all()), s


# ---- 1. tarl_fused_head_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_head_rows_on_packed_states(name, B):
    """Result ``==`` the exported x: FIFO slot 0 where NUMBER_OF_AGENT > 0, 0 elsewhere (an empty road whose slot still holds
    an id among them); n in {0, 1, several}; rows nobody names keep their fill."""
    from tarl_hip import ops
    net = _net(name)
    plan, fs, x = _packed_random(ops, net, B)
    stale = (x[:, :, 3 * net.Nmax + 1] == 0) & (x[:, :, 0] != 0)
    assert bool(stale.any()) and bool((x[:, :, 3 * net.Nmax + 1] > 0).any())
    rows = 7
    for env, slot in (([], []), ([B - 1], [3]), ([b % B for b in (0, 2, 64, 1, 33)], [6, 0, 2, 5, 1])):
        hk = _head_launch(ops, plan, fs, env, slot, rows)
        _check_heads(hk, x, net.Nmax, env, slot, rows)
    again = x.clone().cuda()
    ops.fused_export(plan, fs, again, net.Nmax, 200.0)
    assert torch.equal(again.cpu(), x), "the exported state changed"


def _live_case(B, name="torus8x8", agents=128, seed=11):
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = _net(name)
    N = net.num_roads
    pops = torch.stack([synth.population(agents, N, seed=b, t0=21540, t1=21560) for b in range(B)]).cuda()
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax, pops,
                    congestion_constant=net.congestion_constant, seed=seed)
    eng.reset()
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()
    dist = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    return net, eng, dist


def _run_prior(eng, T, emb, dist, **kw):
    B, N = eng.B, eng.N
    out = dict(choice8=torch.zeros((T, B, N), dtype=torch.uint8, device="cuda"),
               counts=torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda"),
               log_prob=torch.zeros((T, B), device="cuda"), reward=torch.zeros((T, B), device="cuda"))
    eng.rollout_prior(T, emb, dist, prior_weight=1.0, temperature=1.5, policy_seed=77, policy_counter0=5, **out, **kw)
    return out


@pytest.mark.parametrize("B", [3, 65])
def test_head_rows_after_a_reset_and_on_live_states(B):
    """After a reset every entry is 0; after 20 and 40 frames of the prior head the rows ``==`` the exported state."""
    from tarl_hip import ops
    net, eng, dist = _live_case(B)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(3)).cuda()
    env, slot = [0, B - 1, 1], [2, 0, 1]
    hk = _head_launch(ops, eng.plan, eng.fs, env, slot, 3)
    assert not bool(hk.any())
    for frames in (20, 20):
        _run_prior(eng, frames, emb, dist)
        hk = _head_launch(ops, eng.plan, eng.fs, env, slot, 3)
        _check_heads(hk, eng.x.cpu(), net.Nmax, env, slot, 3)
        assert int((hk > 0).sum()) >= 10
    eng.check_flags()


# ---- 2. the rollouts with the capture switch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", [(), ("hold", "router", "trip")])
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("head", ["prior", "goal"])
def test_rollouts_with_the_capture_switch(head, B, rules):
    """tarl_fused_rollout_prior / _goal over T = 6 frames with tarl_fused_set_head_capture: action bytes, log-probs, count
    bytes, rewards, kept observations and the final state ``==`` the same call without the switch; ``head_keep ==`` the
    launches made one by one in front of every frame of a twin engine stepped frame by frame."""
    import goal_mlp_restatement as G
    from tarl_hip import ops
    from tarl_hip.evaluator import router_buffers
    T = 6
    net, e1, dist = _live_case(B, "torus6x5", agents=200)
    _, e2, _ = _live_case(B, "torus6x5", agents=200)
    _, e3, _ = _live_case(B, "torus6x5", agents=200)
    N, Nmax = net.num_roads, net.Nmax
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    w = ops.GoalMlpWeights(flat=torch.tensor(G.weights(3, True)).cuda())
    scale = ops.goal_time_scale(net.x[:, 3 * Nmax:])
    dests, slot_t, weights, table, scratch = router_buffers(e1, None, 1)
    ops.fused_edge_travel_time(e1.plan, e1.fs, out=weights)
    ops.destination_trees_batched(e1.plan, weights[:1], dests, out=table, scratch=scratch)
    # the kept pairs: none in frame 1, one in frame 0, several elsewhere; the slots are a permutation
    gen = torch.Generator().manual_seed(5)
    per_frame = [1, 0, 3, 2, 4, 2]
    ptr = [0] + list(np.cumsum(per_frame))
    K = ptr[-1]
    kenv = torch.randint(0, B, (K,), generator=gen).to(torch.int32)
    kslot = torch.randperm(K, generator=gen).to(torch.int32)
    keep = (ptr, kenv.cuda(), kslot.cuda())

    def rollout(eng, capture):
        pend = torch.empty((N, B), dtype=torch.int32, device="cuda")
        obs = torch.zeros((K, N, 16), device="cuda")
        hk = torch.full((K, N), GUARD, dtype=torch.int32, device="cuda")
        word = 0
        if "hold" in rules:
            ops.fused_set_policy_hold(eng.fs, True)
            ops.fused_set_departure_router(eng.fs, True, slot_t, table[0], pend, plan=eng.plan)
            ops.fused_set_trip_reward(eng.fs, True)
            word = 7
        if capture:
            ops.fused_set_head_capture(eng.fs, True, hk, plan=eng.plan)
        assert eng.fs.struct.policy_hold == word | (8 if capture else 0)
        out = dict(choice8=torch.zeros((T, B, N), dtype=torch.uint8, device="cuda"),
                   counts=torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda"),
                   log_prob=torch.zeros((T, B), device="cuda"), reward=torch.zeros((T, B), device="cuda"))
        kw = dict(temperature=1.5, policy_seed=77, policy_counter0=5, keep=keep, obs_keep=obs, **out)
        if head == "prior":
            eng.rollout_prior(T, emb, dist, prior_weight=1.0, **kw)
        else:
            eng.rollout_goal(T, w, dist, scale, None, **kw)
        if capture:
            ops.fused_set_head_capture(eng.fs, False)
            assert eng.fs.struct.policy_hold == word            # the other three bits stay
        if "hold" in rules:
            ops.fused_set_trip_reward(eng.fs, False)
            ops.fused_set_departure_router(eng.fs, False)
            ops.fused_set_policy_hold(eng.fs, False)
        assert eng.fs.struct.policy_hold == 0
        return out, obs, hk

    out1, obs1, hk1 = rollout(e1, True)
    out0, obs0, hk0 = rollout(e3, False)
    for k in out1:
        assert torch.equal(out1[k], out0[k]), k
    assert torch.equal(obs1, obs0) and torch.equal(e1.x, e3.x) and torch.equal(e1.agents, e3.agents)
    assert bool((hk0 == GUARD).all())                           # with the bit clear nothing is written
    # the launches one by one, in front of every frame
    hk2 = torch.full((K, N), GUARD, dtype=torch.int32, device="cuda")
    counts_f = torch.zeros((N, B), device="cuda")
    for t in range(T):
        lo, hi = ptr[t], ptr[t + 1]
        if hi > lo:
            ops.fused_head_rows(e2.plan, e2.fs, keep[1][lo:hi], keep[2][lo:hi], hk2)
        if head == "prior":
            logits = ops.fused_prior_logits(e2.plan, e2.fs, e2._x, Nmax, e2.agents, emb, dist, 1.0)
        else:
            logits = ops.fused_goal_mlp_logits(e2.plan, e2.fs, e2._x, Nmax, e2.agents, w, dist, scale)
        c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        lp2 = ops.graphdist_rollout(e2.plan, logits, 1.5, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
        clock = float(e2.time)
        if "hold" in rules:
            ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents)
            p2 = ops.fused_pending_departures(e2.plan, e2.fs, clock)
            ops.fused_route_departures(e2.plan, e2.fs, p2, slot_t, table[0])
        e2.frame_fused(skip_choice=True, counts=counts_f)
        assert torch.equal(c8, out1["choice8"][t]) and torch.equal(lp2, out1["log_prob"][t]), t
        assert torch.equal(counts_f, out1["counts"][t + 1].float()), t
    assert torch.equal(hk1, hk2) and not bool((hk1 == GUARD).any())
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert int((hk1 > 0).sum()) > 0
    e1.check_flags()


# ---- 3. tarl_decision_advantage and tarl_decision_stats ----------------------------------------------------------------------------
def _advantage_inputs(name, B=3, rows=9, T=12, seed=0):
    """Crafted buffers on the graph's own out-degrees: head ids that are 0, valid, the dummy's neighbours and beyond the table
    (bad); two agent tables per environment set (one per segment) whose arrivals lie exactly on frame clocks, some never
    done; destinations out of range, without a table slot and unreachable (inf) among them."""
    net = _net(name)
    N = net.num_roads
    rng = np.random.default_rng(seed)
    A, D = 40, 7
    deg = np.bincount(net.edge_index[0].numpy(), minlength=N)
    times = (21540 + np.arange(T + 1)).astype(np.float32)
    t_mid = 7                                                    # the first segment ends after frame 6
    frame = np.sort(rng.integers(0, T, rows)).astype(np.int32)
    frame[0], frame[-1] = 0, T - 1
    env = rng.integers(0, B, rows).astype(np.int32)
    slot = rng.permutation(rows).astype(np.int32)
    head = rng.integers(0, A + 3, (rows, N)).astype(np.int32)    # ids A .. A + 2: beyond the table
    head[rng.random((rows, N)) < 0.4] = 0
    dests = rng.choice(N, D, replace=False)
    dest_slot = np.full(N, -1, dtype=np.int32)
    dest_slot[dests] = np.arange(D)
    tables = []
    for seg_end in (t_mid, T):
        ag = np.zeros((B, A, 9), dtype=np.float32)
        ag[:, :, DC.DESTINATION] = rng.choice(np.concatenate([dests, dests, [-1.0, N, (dests[0] + 1) % N]]), (B, A))
        done = rng.random((B, A)) < 0.6
        ag[:, :, DC.DONE] = done
        ag[:, :, DC.ON_WAY] = ~done
        ag[:, :, DC.ARRIVAL_TIME] = np.where(done, times[rng.integers(0, seg_end, (B, A))], 0.0)
        tables.append(ag)
    dist = rng.random((D, N)) * 40.0
    dist[rng.random((D, N)) < 0.1] = np.inf
    return dict(net=net, N=N, A=A, D=D, B=B, T=T, t_mid=t_mid, deg=deg, times=times, frame=frame, env=env, slot=slot,
                head=head, dest_slot=dest_slot, tables=tables, dist=dist, rows=rows)


def _restated_advantage(c, dist, gamma):
    """Both segments through the restatement -> (adv (rows, N) in slot order, live, truncated, bad)."""
    adv = np.zeros((c["rows"], c["N"]))
    live = np.zeros((c["rows"], c["N"]), dtype=bool)
    trunc = bad = 0
    for ag, lo_t, hi_t in ((c["tables"][0], 0, c["t_mid"]), (c["tables"][1], c["t_mid"], c["T"])):
        sel = np.nonzero((c["frame"] >= lo_t) & (c["frame"] < hi_t))[0]
        r = DC.decision_advantage(c["head"][c["slot"][sel]], c["frame"][sel], c["env"][sel], ag, c["times"], hi_t, dist,
                                  c["dest_slot"], c["deg"], 1.0, gamma)
        adv[c["slot"][sel]], live[c["slot"][sel]] = r["adv"], r["live"]
        trunc, bad = trunc + r["truncated"], bad + r["bad"]
    return adv, live, trunc, bad


def _device_advantage(ops, plan, c, dist, gamma):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()      # noqa: E731
    hk = dev(c["head"], torch.int32)
    adv = torch.full((c["rows"], c["N"]), float("nan"), device="cuda")
    trunc, bad = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    frame, env, slot = (dev(c[k], torch.int32) for k in ("frame", "env", "slot"))
    for ag, lo_t, hi_t in ((c["tables"][0], 0, c["t_mid"]), (c["tables"][1], c["t_mid"], c["T"])):
        sel = np.nonzero((c["frame"] >= lo_t) & (c["frame"] < hi_t))[0]
        lo, hi = int(sel[0]), int(sel[-1]) + 1                   # the rows are sorted by frame: a segment is a run
        ops.decision_advantage(plan, hk, frame[lo:hi], env[lo:hi], slot[lo:hi], dev(ag, torch.float32), dev(c["times"], torch.float32),
                               hi_t, dev(dist, torch.float64), dev(c["dest_slot"], torch.int32), B=c["B"], timestep=1,
                               decision_gamma=gamma, adv_raw=adv, truncated=trunc, bad=bad)
    torch.cuda.synchronize()
    return hk, adv, int(trunc), int(bad)


@pytest.mark.parametrize("name", GRAPHS)
def test_advantage_and_statistics_against_the_restatement(name):
    """With a zero distance table and gamma 1 ``adv_raw == -n`` exactly; the live mask, ``truncated``, ``bad`` and the count
    ``==``; with real distances and gamma in {1, 0.99} ``adv_raw``, its sum and its sum of squares within ``tensor_bound``
    (e32: the rounding of the float64 value to fp32). A segment ends inside the batch: two calls, two agent tables."""
    from tarl_hip import ops
    c = _advantage_inputs(name)
    plan = ops.Plan(c["net"].edge_index, c["N"])
    finite = np.where(np.isfinite(c["dist"]), 0.0, np.inf)
    want, live, trunc, bad = _restated_advantage(c, finite, 1.0)
    hk, adv, trunc_d, bad_d = _device_advantage(ops, plan, c, finite, 1.0)
    assert np.array_equal(adv.cpu().numpy().astype(np.float64), want)                   # -n, integers: exact
    assert np.array_equal((hk > 0).cpu().numpy(), live) and (trunc_d, bad_d) == (trunc, bad)
    assert bad > 0 and trunc > 0 and live.sum() > 20 and (want[live] == 0).any()
    assert np.array_equal(hk.cpu().numpy()[live], c["head"][live])                      # live heads keep their id
    if name in ("MIXED", "HUB126"):
        assert (c["deg"] == 0).any() and not live[:, c["deg"] == 0].any()
    for gamma in (1.0, 0.99):
        want, live2, _, _ = _restated_advantage(c, c["dist"], gamma)
        hk, adv, _, _ = _device_advantage(ops, plan, c, c["dist"], gamma)
        assert np.array_equal(live2, live) and np.array_equal((hk > 0).cpu().numpy(), live)
        w64 = torch.from_numpy(want)
        b = R.tensor_bound(R.max_err(w64.float(), w64), w64)
        err = R.max_err(adv.cpu(), w64)
        st = ops.decision_stats(adv, hk).cpu()
        ref = torch.from_numpy(DC.decision_stats(adv.cpu().numpy(), live))
        assert st[2] == ref[2] == live.sum()
        b_s = R.tensor_bound(0.0, ref[:2])
        err_s = R.max_err(st[:2], ref[:2])
        print(f"[decision advantage {name} gamma={gamma}] {int(live.sum())} live, err {err:.3e} (bound {b:.3e}), sums err "
              f"{err_s:.3e} (bound {b_s:.3e})")
        assert err <= b and err_s <= b_s
        assert torch.equal(st, ops.decision_stats(adv, hk).cpu())                        # a fixed order: bit-identical


# ---- 4. tarl_graphdist_node_logprob and tarl_graphdist_decision_ppo ---------------------------------------------------------------
def _loss_inputs(name, M, T=0.7, seed=0):
    net = _net(name)
    N, ei = net.num_roads, net.edge_index.numpy()
    E = ei.shape[1]
    rng = np.random.default_rng(seed + M)
    g = torch.Generator().manual_seed(seed + M)
    logits = (rng.normal(size=(M, E)) * 2.0).astype(np.float32)
    choice = ig.random_actions(net, g, M).numpy().astype(np.int32)
    deg = np.bincount(ei[0], minlength=N)
    live = (rng.random((M, N)) < 0.5) & (deg > 0)
    long_nodes = np.nonzero(deg > 4)[0]
    if long_nodes.size:                         # the last entry of a long out-list, chosen and live
        u = long_nodes[-1]
        live[:, u] = True
        choice[:, u] = DC.out_lists(ei, N)[u][-1]
    adv = np.where(live, rng.normal(size=(M, N)) * 6.0 - 2.0, 0.0).astype(np.float32)
    lp0 = DC.node_logprob(ei, N, logits, choice, T)
    lp_old = (lp0 + rng.choice([-0.5, -0.05, 0.0, 0.05, 0.5], size=(M, N))).astype(np.float32)      # below, inside, above the clip
    return dict(net=net, N=N, E=E, ei=ei, logits=logits, choice=choice, live=live, adv=adv, lp_old=lp_old, lp0=lp0, T=T, deg=deg)


@pytest.mark.parametrize("M", [1, 3, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_node_logprob_and_decision_ppo_against_float64(name, M):
    """lp_node against the restatement and its sum over the nodes against the joint log-prob of the pinned chain; loss parts
    (counts ``==``) and gradient against the float64 restatement within ``tensor_bound`` (e32 from its fp32 run), temperature
    0.7, ``grad_logits`` pre-filled so that ``+=`` shows and untouched off the live nodes, a NaN-filled scratch, two runs
    bit-identical."""
    from tarl_hip import ops
    c = _loss_inputs(name, M)
    N, E, ei, T = c["N"], c["E"], c["ei"], c["T"]
    plan = ops.Plan(c["net"].edge_index, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    lg, ch = dev(c["logits"]), dev(c["choice"])
    lp = ops.graphdist_node_logprob(plan, lg, ch, T, out=torch.full((M, N), float("nan"), device="cuda")).cpu()
    lp64, lp32 = torch.from_numpy(c["lp0"]), torch.from_numpy(DC.node_logprob(ei, N, c["logits"], c["choice"], T, np.float32))
    b = R.tensor_bound(R.max_err(lp32, lp64), lp64)
    assert R.max_err(lp, lp64) <= b and not bool(torch.isnan(lp).any())
    assert not bool(lp[:, torch.from_numpy(c["deg"] == 0)].any())
    joint, _ = ops.graphdist_logprob_entropy(plan, ops.graphdist_softmax(plan, lg, T), choice=ch, want_entropy=False)
    s64 = lp64.sum(1)
    b_j = R.tensor_bound(R.max_err(lp32.double().sum(1), s64), s64)
    assert R.max_err(lp.double().sum(1), s64) <= b_j
    # the chain adds its N fp32 terms in a tree: the depth bound of update_restatement.scalar_bound on top
    assert R.max_err(joint.cpu(), s64) <= b_j + R.scalar_bound(N, float(lp64.abs().sum(1).max()))
    # the loss
    st = DC.decision_stats(c["adv"], c["live"])
    L = int(c["live"].sum())
    kw = dict(clip_epsilon=0.2, temperature=T, grad_scale=0.5)
    r64 = DC.decision_ppo(ei, N, c["logits"], c["choice"], c["live"], c["lp_old"], c["adv"], st, L, **kw)
    r32 = DC.decision_ppo(ei, N, c["logits"], c["choice"], c["live"], c["lp_old"], c["adv"], st, L, dtype=np.float32, **kw)
    head = dev(np.where(c["live"], 5, 0).astype(np.int32))
    n_live = torch.tensor([L], dtype=torch.int32).cuda()
    fill = torch.from_numpy(np.random.default_rng(1).integers(-8, 9, size=(M, E)).astype(np.float32)) * 2.0 ** -12
    fill[fill == 0] = 2.0 ** -12
    runs = []
    for k in range(3):          # from zeros (the bound), then twice into the pre-filled buffer (+= and bit-identity)
        g = (torch.zeros_like(fill) if k == 0 else fill.clone()).cuda()
        need = ops._lib.load().tarl_graphdist_decision_ppo_scratch_bytes(plan.handle, M)
        scratch = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
        out4 = ops.graphdist_decision_ppo(plan, lg, ch, head, dev(c["lp_old"]), dev(c["adv"]), dev(st), n_live, grad_logits=g,
                                          scratch=scratch, **kw)
        runs.append((out4.cpu(), g.cpu()))
    assert torch.equal(runs[1][0], runs[2][0]) and torch.equal(runs[1][1], runs[2][1]) and torch.equal(runs[0][0], runs[1][0])
    out4, g_zero = runs[0]
    g = runs[1][1]
    o64, g64 = torch.from_numpy(r64["out4"]), torch.from_numpy(r64["grad"])
    assert torch.equal(out4[:, 1:3], o64[:, 1:3]) and int(out4[:, 1].sum()) == L
    if M > 1:
        assert 0 < int(out4[:, 2].sum()) < L
    b_o = R.tensor_bound(R.max_err(torch.from_numpy(r32["out4"]), o64), o64)
    b_g = R.tensor_bound(R.max_err(torch.from_numpy(r32["grad"]).double(), g64), g64, relative_scale=True)
    err_o, err_g = R.max_err(out4, o64), R.max_err(g_zero, g64)
    # += : the same values on top of the fill, within one fp32 ulp of the larger operand
    assert R.max_err(g.double() - fill.double(), g_zero) <= 2.0 ** -23 * float((fill.abs() + g_zero.abs()).max())
    print(f"[decision ppo {name} M={M}] L={L}, out4 err {err_o:.3e} (bound {b_o:.3e}), grad err {err_g:.3e} (bound {b_g:.3e})")
    assert err_o <= b_o and err_g <= b_g
    off = ~torch.from_numpy(c["live"])[:, torch.from_numpy(ei[0])]
    assert torch.equal(g[off], fill[off])                       # every edge of a node without a live decision: untouched
    assert bool((g[~off] != fill[~off]).any())
    # L = 0 on the device: nothing is added
    g0 = fill.clone().cuda()
    ops.graphdist_decision_ppo(plan, lg, ch, head, dev(c["lp_old"]), dev(c["adv"]), dev(st),
                               torch.zeros(1, dtype=torch.int32, device="cuda"), grad_logits=g0, **kw)
    assert torch.equal(g0.cpu(), fill)


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------------
def _trainer(credit=None, entropy_coef=0.01, epochs=2, B=3, T=24, M=8, seed=0):
    """The 8 x 8 torus, B = 3, 128 agents leaving at once, the goal-conditioned head, T = 24 frames, minibatches of 8."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(8, 8)
    N = net.num_roads
    pops = torch.stack([synth.population(128, N, seed=40 + b, t0=21540, t1=21545) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=9)
    torch.manual_seed(1)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.prior_method = "all_pairs"
    pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * net.Nmax:]))
    with torch.no_grad():
        pol.goal_mlp[0].bias.uniform_(-0.3, 0.3)
        pol.goal_mlp[0].weight.uniform_(-1.0, 1.0)
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    gm = pol.goal_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    kw = {} if credit is None else {"credit": credit}
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=epochs, sub_batch_size=M,
                       extra_params=extra, policy="goal_mlp", temperature=2.0, entropy_coef=entropy_coef, seed=seed,
                       goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias], prior_table=pol.dist_matrix, **kw)
    tr.keep_grad = True
    return tr, net


def _record_steps(tr):
    """Snapshots (parameters, gradient) in front of every Adam step and the logits' gradient handed to the head's backward."""
    snaps, g_logits = [], []
    adam, bwd = tr.flat.adam_step, tr._actor_logits_bwd

    def step(**kw):
        snaps.append((tr.flat.flat.clone(), tr.flat.grad.clone()))
        return adam(**kw)

    def backward(obs, g):
        g_logits.append(g.clone())
        return bwd(obs, g)
    tr.flat.adam_step, tr._actor_logits_bwd = step, backward
    return snaps, g_logits


def test_train_iteration_against_the_restatement():
    """One ``train_iteration`` of ``credit="decision"``, two epochs: per epoch the gradient of the logits ``==`` entropy term +
    decision term, the decision term against the restatement driven by the exported buffers within ``tensor_bound``, and the
    actor parameters' gradient ``==`` the head's backward of exactly that; ``lp_old_node`` sums to the rollout's stored joint
    log-prob; the report's numbers are those of the buffers."""
    from tarl_hip import ops
    tr, net = _trainer("decision")
    snaps, g_seen = _record_steps(tr)
    tr.train_iteration()
    tr.check_flags()
    eng, N, M, T = tr.eng, tr.eng.N, tr.M, tr.temperature
    ei = net.edge_index.numpy()
    assert len(snaps) == 2 and eng.fs.struct.policy_hold == 0
    hk, adv, lpo = tr.head_keep.cpu().numpy(), tr.adv_raw.cpu().numpy(), tr.lp_old_node.cpu().numpy()
    live = hk > 0
    assert live.sum() > 50 and int(tr.decision_bad) == 0
    # the captured heads and raw advantages: the restatement on the final agent table (one segment, no reset inside)
    frames = np.asarray(tr._keep[0])
    env, slot = tr._keep[1].cpu().numpy(), tr._keep[2].cpu().numpy()
    dist, dslot = tr._decision_dist
    r = DC.decision_advantage(hk[slot], frames, env, eng.agents.cpu().numpy(), tr.times.cpu().numpy(), tr.T, dist.cpu().numpy(),
                              dslot.cpu().numpy(), np.full(N, 4), eng.timestep, 1.0)
    a64 = torch.from_numpy(r["adv"])
    assert np.array_equal(r["live"], live[slot]) and r["bad"] == 0 and r["truncated"] == int(tr.decision_truncated)
    assert R.max_err(torch.from_numpy(adv[slot]), a64) <= R.tensor_bound(R.max_err(a64.float(), a64), a64)
    st = DC.decision_stats(adv, live)
    assert R.max_err(tr._decision_stats.cpu(), torch.from_numpy(st)) <= R.tensor_bound(0.0, torch.from_numpy(st))
    rep = {k: float(v) for k, v in tr.last["decision"].items()}
    mean = float(adv[live].astype(np.float64).mean())
    assert rep["decisions"] == live.sum() and abs(rep["delay_frames"] + mean) <= 1e-9 * max(1.0, abs(mean))
    assert rep["truncated"] == r["truncated"] / live.sum()
    assert 0.0 <= rep["truncated"] <= 1.0 and 0.0 <= rep["clip_fraction"] <= 1.0 and np.isfinite(rep["kl"])
    off = 0
    for e, idx in enumerate(tr._mb_idx):
        params, grad = snaps[e]
        w = ops.GoalMlpWeights(flat=params[tr._goal_off:tr._goal_off + ops.GOAL_MLP_PARAMS].clone())
        obs = tr.obs_mb[off:off + M]
        logits = ops.policy_goal_mlp(eng.plan, obs, w, tr.prior_table, tr.goal_scale, dest_slot=tr.prior_dest_slot)
        choice, _ = ops.rollout_gather(eng.plan, tr.T, eng.B, False, idx, choice=tr.choice)
        if e == 0:          # the parameters of the rollout: lp_old is this forward's, and sums to the stored joint log-prob
            lp_dev = ops.graphdist_node_logprob(eng.plan, logits, choice, T)
            assert torch.equal(lp_dev.cpu(), torch.from_numpy(lpo[off:off + M]))
            stored = tr.logp.view(-1).index_select(0, idx).cpu().double()
            s64 = torch.from_numpy(DC.node_logprob(ei, N, logits.cpu().numpy(), choice.cpu().numpy(), T).sum(1))
            assert R.max_err(stored, s64) <= R.tensor_bound(0.0, s64) + R.scalar_bound(N, float(s64.abs().max()))
        sl = slice(off, off + M)
        L = int(live[sl].sum())
        kw = dict(clip_epsilon=tr.clip_epsilon, temperature=T, grad_scale=1.0)
        args = (ei, N, logits.cpu().numpy(), choice.cpu().numpy(), live[sl], lpo[sl], adv[sl], st, L)
        r64, r32 = DC.decision_ppo(*args, **kw), DC.decision_ppo(*args, dtype=np.float32, **kw)
        # the entropy term alone: the existing backward with a zero log-prob seed
        proba = ops.graphdist_softmax(eng.plan, logits, T)
        g_ent = torch.full((M,), -tr.entropy_coef / M, device="cuda")
        base = ops.graphdist_logprob_entropy_bwd(eng.plan, proba, T, choice=choice, grad_log_prob=torch.zeros(M, device="cuda"),
                                                 grad_entropy=g_ent)
        dec = (g_seen[e].double() - base.double()).cpu()
        g64 = torch.from_numpy(r64["grad"])
        b = R.tensor_bound(R.max_err(torch.from_numpy(r32["grad"]).double(), g64), g64, relative_scale=True) + \
            2.0 ** -23 * float(base.abs().max())
        err = R.max_err(dec, g64)
        print(f"[decision trainer epoch {e}] L={L}, decision gradient err {err:.3e} (bound {b:.3e})")
        assert err <= b and L > 0 and float(g64.abs().max()) > 0
        edge_live = torch.from_numpy(live[sl])[:, net.edge_index[0]]
        assert torch.equal(g_seen[e].cpu()[~edge_live], base.cpu()[~edge_live])        # off the live roads: entropy alone
        # the actor parameters' gradient: the head's backward of exactly that, nothing else
        gp = torch.zeros(ops.GOAL_MLP_PARAMS, device="cuda")
        ops.policy_goal_mlp_bwd(eng.plan, obs, w, tr.prior_table, tr.goal_scale, g_seen[e], gp, dest_slot=tr.prior_dest_slot)
        assert torch.equal(grad[tr._goal_off:tr._goal_off + ops.GOAL_MLP_PARAMS], gp)
        assert not bool(grad[:N].any())                                                 # the embedding is not this head's
        off += M
    assert torch.equal(tr.last_grad, snaps[1][1])


def test_the_default_is_bit_identical():
    """``credit="joint"``: gradient and updated parameters ``==`` those of a trainer constructed without the argument."""
    a, _ = _trainer("joint")
    b, _ = _trainer(None)
    a.train_iteration()
    b.train_iteration()
    assert a.credit == b.credit == "joint" and "decision" not in a.last
    assert torch.equal(a.last_grad, b.last_grad) and torch.equal(a.flat.flat, b.flat.flat)
    assert torch.equal(a.choice, b.choice) and torch.equal(a.logp, b.logp) and torch.equal(a.last["losses"], b.last["losses"])


def test_locality_fails_without_the_feature():
    """THE TEST THAT FAILS WITHOUT THE FEATURE. Entropy coefficient 0: under ``credit="decision"`` the gradient of the logits
    is exactly 0 on every out-edge of every road that headed nobody; under ``"joint"`` the same frames spread one advantage
    over all roads, and such edges do receive gradient."""
    seen = {}
    for credit in ("decision", "joint"):
        tr, net = _trainer(credit, entropy_coef=0.0, epochs=1)
        _, g_seen = _record_steps(tr)
        tr.collect()
        if credit == "decision":    # who headed whom: the joint run below is the same rollout and the same minibatch draw
            seen["heads"] = tr.head_keep.cpu() > 0
        heads = seen["heads"]
        tr.update()
        g = g_seen[0].cpu()
        nobody = ~heads[:tr.M][:, net.edge_index[0]]
        seen[credit] = (g, nobody, tr.choice.clone())
    assert torch.equal(seen["decision"][2], seen["joint"][2])              # the same rollout, the same minibatch draw
    g, nobody, _ = seen["decision"]
    assert int(nobody.sum()) > 0 and not bool(g[nobody].any()) and bool(g[~nobody].any())
    g, nobody, _ = seen["joint"]
    assert bool(g[nobody].any())


def test_the_trainer_refusals():
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    pop = synth.population(16, net.num_roads, seed=1)
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(), congestion_constant=net.congestion_constant,
                    num_envs=1, seed=3)
    with pytest.raises(ValueError, match="credit='decision' is not available for policy='embedding'"):
        VecPPOTrainer(eng, None, [], rollout_steps=4, policy="embedding", credit="decision")
    with pytest.raises(ValueError, match="credit must be"):
        VecPPOTrainer(eng, None, [], rollout_steps=4, policy="embedding", credit="other")


# ---- 6. CLI end to end ---------------------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-300"
NEW_KEYS = {"train/credit", "train/decisions", "train/decision_delay_frames", "train/decision_truncated",
            "train/decision_clip_fraction", "train/decision_kl"}


def _main(argv):
    import importlib
    importlib.import_module("main").main(argv)


def test_cli_train_end_to_end(tmp_path):
    run, ref = tmp_path / "run", tmp_path / "ref"
    base = ["--algo", "mpnn+ppo", "--mode", "train", "--scenario", SCENARIO, "--policy-head", "goal_mlp", "--policy-hold",
            "--route-departures", "--rollout-steps", "256", "--iterations", "2", "--steps", "5"]      # 20 agents leave in time
    _main(base + ["--credit", "decision", "--credit-gamma", "0.99", "--output-dir", str(run)])
    _main(base + ["--output-dir", str(ref)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    old = [json.loads(l) for l in open(ref / "train_log.jsonl")]
    assert len(logs) == 2 and len(old) == 2
    assert set(logs[0]) - set(old[0]) == NEW_KEYS and set(old[0]) <= set(logs[0])      # the same frames: the same old keys
    for rec, o in zip(logs, old):
        assert NEW_KEYS <= set(rec) and not NEW_KEYS & set(o)
        assert rec["train/credit"] == "decision" and rec["train/decisions"] > 0
        assert 0.0 <= rec["train/decision_truncated"] <= 1.0 and 0.0 <= rec["train/decision_clip_fraction"] <= 1.0
        assert np.isfinite(rec["train/decision_kl"]) and np.isfinite(rec["train/decision_delay_frames"])
    # iteration 0 collects with the same parameters: the same frames
    assert logs[0]["PPO/avg_episode_return"] == old[0]["PPO/avg_episode_return"]
    assert logs[0]["train/held"] == old[0]["train/held"]


def test_cli_refusals():
    for argv, msg in ((["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--credit", "decision"], "mode 'train'"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--credit", "decision"], "state-dependent head"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit-gamma", "0.9"],
                       "needs credit decision"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "graph_transformer", "--value-head",
                        "graph_transformer", "--credit", "decision"], "graph_transformer")):
        with pytest.raises(ValueError, match=msg):
            _main(argv + ["--scenario", SCENARIO])
