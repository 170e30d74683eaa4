"""GPU: the trip reward — tarl_fused_trip_reward against ``trip_reward_restatement`` on packed agent tables of
every size at which the status pass takes another path (the 8 x 8 torus and both irregular graphs) and on live states, the
one-call rollouts with the switch set against their launches queued one by one, one ``collect()`` of
``VecPPOTrainer(reward="trip")``, ``VecEvaluator(trip_reward=True)`` replayed frame for frame by the CPU oracle under the
exported device noise, the test that fails without the feature, the one-agent ranking case, the CLI end to end and the
refusals. Every comparison of the reward and its parts is ``==``."""
import ctypes

import numpy as np
import pytest
import torch

import departure_restatement as D
import sp_cases as S
import trip_reward_restatement as R

pytestmark = pytest.mark.gpu

T0 = 200.0
# The status pass gives one wave a segment of 256 16-byte groups (4 096 bytes) of one environment's row and one workgroup four
# consecutive (environment, segment) tasks: S = max(1, ceil((A // 16) / 256)) segments per environment. Up to A = 8 207 an
# environment is at most two tasks, which never straddle a workgroup; A = 8 208 is the smallest A with S = 3 (513 whole groups
# in an aligned row), where environment 1 (tasks 3, 4, 5) spans workgroups 0 and 1 and its counts meet in the atomic word.
A_SPLIT = 8208
SIZES = (1, 15, 16, 17, 63, 64, 65, 128, 129)


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _net(name):
    return _torus8() if name == "torus" else S.case(name).net


def _spread_population(net):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    return synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)


def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


def _packed(ops, net, ag, sort_agents=None):
    """The empty network in K environments with the agent tables ``ag`` (K, A, 9)."""
    K = ag.size(0)
    x, _ = R.empty_state(net)
    plan = ops.Plan(net.edge_index, net.num_roads)
    fs = ops.FusedState(plan, K, ag.size(1), "cuda", net.Nmax)
    xd, agd = x.unsqueeze(0).repeat(K, 1, 1).contiguous().cuda(), ag.cuda()
    ops.fused_pack(plan, fs, xd, net.Nmax, agd, net.congestion_constant.cuda(), sort_agents=sort_agents,
                   ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    return plan, fs, xd, agd


def _between_guards(ops, plan, fs, t, with_parts=True):
    """The launch into the middle of NaN / 0x7F-filled buffers -> (reward (B,), parts (B, 2) or None) on the host; the bands on
    both sides must stay, and every element between them must have been written."""
    B = fs.B
    rbuf = torch.full((B + 128,), float("nan"), device="cuda")
    pbuf = torch.full((2 * B + 128,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    out, parts = rbuf[64:64 + B], pbuf[64:64 + 2 * B].view(B, 2)
    got = ops.fused_trip_reward(plan, fs, t, out=out, parts=parts if with_parts else None)
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(rbuf[:64]).all()) and bool(torch.isnan(rbuf[64 + B:]).all())
    assert bool((pbuf[:64] == 0x7F7F7F7F).all()) and bool((pbuf[64 + 2 * B:] == 0x7F7F7F7F).all())
    assert not bool(torch.isnan(out).any())
    if not with_parts:
        assert bool((pbuf == 0x7F7F7F7F).all())
        return out.cpu(), None
    assert not bool((parts == 0x7F7F7F7F).any())
    return out.cpu(), parts.cpu()


def _without_window(fs):
    """The handle as an engine packed without ``a_order`` has it: every agent's departure is tested beside its status."""
    saved = fs.struct.a_order
    fs.struct.a_order = None
    return saved


def _check(ops, plan, fs, agents, t):
    """reward and parts ``==`` the restatement on ``agents`` (K, A, 9, host): with the window and without it, with parts and
    without them, twice the same. -> parts."""
    want_p = torch.from_numpy(R.parts_batch(agents.numpy(), t).astype(np.int32))
    want_r = torch.from_numpy(R.reward_batch(agents.numpy(), t))
    results = []
    for window in (True, False):
        saved = None if window else _without_window(fs)
        for with_parts in (True, False, True):
            r, p = _between_guards(ops, plan, fs, t, with_parts)
            assert torch.equal(r, want_r), (window, with_parts, r.tolist(), want_r.tolist())
            assert p is None or torch.equal(p, want_p), (window, p.tolist(), want_p.tolist())
            results.append(r)
        if not window:
            fs.struct.a_order = saved
    assert all(torch.equal(results[0], r) for r in results)
    return want_p


STATE = ("hdp", "tl", "gc8", "post", "slots", "a_origin", "a_dest", "a_dep", "a_status", "a_order", "a_dep_sorted", "cur_lo",
         "a_win", "a_ins", "a_rank", "acc_lp", "acc_n", "acc_w", "flags", "st0", "node_rec", "in_rec", "out_pad", "sel8", "sel")


def _snapshot(fs):
    return {k: getattr(fs, k).clone() for k in STATE}


# ---- 1. the launch against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED", "HUB126"])
def test_trip_reward_on_packed_tables_of_every_size(name, K):
    """The crafted agent table, repeated to A rows, with statuses that differ between the environments: A = 1 (agent 0 alone),
    rows shorter than one 16-byte group, exactly one, one and a byte, ... — with K > 1 every row but the first starts at an
    unaligned byte whenever A is no multiple of 16. With the window, with its pointer withdrawn and on a handle packed without
    ``a_order``; from NaN / 0x7F-filled buffers between guard bands; the packed state and its export unchanged."""
    from tarl_hip import ops
    net = _net(name)
    c = R.crafted(t=T0, K=K)
    later = float(np.nextafter(np.float32(T0), np.float32(np.inf)))
    for A in SIZES:
        ag = R.padded(c["agents"], A)
        plan, fs, xd, agd = _packed(ops, net, ag)
        assert fs.A == A and fs.struct.a_order and fs.struct.a_win
        before = _snapshot(fs)
        exported = xd.clone()
        ops.fused_export(plan, fs, exported, net.Nmax, T0)
        p = _check(ops, plan, fs, ag, T0)
        assert int(p[:, 1].min()) >= 1                      # agent 0 is ready in every environment: a skipped row 0 shows
        if A >= 10:
            assert int(p[0, 0]) >= 2 and int(p[0, 1]) >= 4
            if K > 2:
                assert not torch.equal(p[0], p[1]) and not torch.equal(p[0], p[2])
            assert int(_check(ops, plan, fs, ag, later)[0, 1]) == int(p[0, 1]) + (A + 7) // 10     # one float later: every just_after_t
        _check(ops, plan, fs, ag, T0 - 1000.0)              # nobody is due
        for k, v in before.items():
            assert torch.equal(getattr(fs, k), v), (A, k)
        again = xd.clone()
        ops.fused_export(plan, fs, again, net.Nmax, T0)
        assert torch.equal(again, exported) and torch.equal(agd.cpu(), ag)
        plan2, fs2, _, _ = _packed(ops, net, ag, sort_agents=False)
        assert not fs2.struct.a_order
        r2, p2 = _between_guards(ops, plan2, fs2, T0)
        assert torch.equal(p2, p) and torch.equal(r2, -(p.sum(dim=1).float()))


@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("A", [A_SPLIT - 1, A_SPLIT, A_SPLIT + 1])
def test_trip_reward_where_one_environment_spans_two_workgroups(A, K):
    """A = 8 208 is the smallest A at which the status pass gives one environment three wave tasks, so that environment 1 is
    served by two workgroups (see A_SPLIT above); 8 207 is two tasks in one workgroup with unaligned rows, 8 209 three tasks
    with unaligned rows. Random statuses, so that every segment holds agents on the way; environment 1's second segment and
    its last sixteen agents — the one group of its third segment at A = 8 208 — are all on the way."""
    from tarl_hip import ops
    net = _torus8()
    g = torch.Generator().manual_seed(A + K)
    ag = torch.zeros((K, A, 9))
    ag[:, :, R.ORIGIN], ag[:, :, R.DEST] = 3.0, 5.0
    ag[:, :, R.DEP] = T0 + torch.randint(-50, 50, (K, A), generator=g).float()
    ag[:, A // 2, R.DEP] = T0
    status = torch.randint(0, 3, (K, A), generator=g)
    ag[:, :, R.ON_WAY], ag[:, :, R.DONE] = (status == 1).float(), (status == 2).float()
    for lo, hi in ((4096, 8192), (A - 16, A)):
        ag[1, lo:hi, R.ON_WAY], ag[1, lo:hi, R.DONE] = 1.0, 0.0
    plan, fs, xd, agd = _packed(ops, net, ag)
    before = _snapshot(fs)
    p = _check(ops, plan, fs, ag, T0)
    assert int(p[1, 0]) > 4096 + 1000 and int(p[:, 1].min()) > 500
    for k, v in before.items():
        assert torch.equal(getattr(fs, k), v), k
    on, shape = R.byte_pass(R.status_bytes(ag.numpy()), fs.a_status.data_ptr() % 16)
    assert on.tolist() == p[:, 0].tolist()
    assert (max(g_ for g_, _, _ in shape) > 512) == (A >= A_SPLIT)          # more groups than two segments hold, from 8 208 on


@pytest.mark.parametrize("K", [3, 65])
def test_trip_reward_after_a_reset_and_on_a_live_state(K):
    """The spread case under the holding free-flow router: after the reset, and after 20 and 40 live frames (the cursor has
    advanced, agents are on the way, some have arrived): ``==`` the restatement on the exported agent tables, with and without
    the window; the queue reward of the last frame is ``on_way - lost``; the launch writes nothing else."""
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    ev = VecEvaluator(_engine(net, _spread_population(net), K), "dijkstra_hold", refresh_rate=0)
    eng = ev.eng
    eng.reset()
    for t in (EPISODE_START, EPISODE_START + 17.0):
        p = _check(ops, eng.plan, eng.fs, eng.agents.cpu(), t)
        assert int(p[:, 0].max()) == 0
    for frames in (20, 40):
        ev.run(frames)
        assert int(eng.fs.cur_lo.min()) > 0 and int(eng.fs.a_ins.sum()) > 0
        before = _snapshot(eng.fs)
        last = float(eng.time) - float(eng.timestep)           # the clock of the frame that ran last
        for t in (last, float(eng.time) + 25.0):
            p = _check(ops, eng.plan, eng.fs, eng.agents.cpu(), t)
        assert int(p[:, 0].min()) > 0
        p = _check(ops, eng.plan, eng.fs, eng.agents.cpu(), last)
        for k, v in before.items():
            assert torch.equal(getattr(eng.fs, k), v), k
        queued = -ev.reward[frames - 1].cpu()                   # (reading eng.x exports the state: after the comparison above)
        lost = torch.tensor([D.lost(eng.x[b].cpu(), eng.agents[b].cpu(), net.Nmax) for b in range(K)], dtype=torch.float32)
        assert torch.equal(p[:, 0].float(), queued + lost)      # owed = queued + lost + ready


def test_a_refused_call_writes_nothing():
    from tarl_hip import lib, ops
    net = _torus8()
    ag = R.padded(R.crafted(t=T0, K=3)["agents"], 17)
    plan, fs, _, _ = _packed(ops, net, ag)
    L = lib.load()
    r = torch.full((3,), float("nan"), device="cuda")
    p = torch.full((3, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    for t in (float("inf"), float("nan")):
        assert L.tarl_fused_trip_reward(plan.handle, fs.ref, 3, net.Nmax, fs.A, ctypes.c_float(t), r.data_ptr(), p.data_ptr(),
                                        None) == -1
    assert L.tarl_fused_trip_reward(plan.handle, fs.ref, 3, net.Nmax, 0, ctypes.c_float(T0), r.data_ptr(), p.data_ptr(),
                                    None) == -1
    assert L.tarl_fused_trip_reward(plan.handle, fs.ref, 3, net.Nmax, fs.A, ctypes.c_float(T0), None, p.data_ptr(), None) == -1
    assert bool(torch.isnan(r).all()) and bool((p == 0x7F7F7F7F).all())
    with pytest.raises(ValueError, match="finite"):
        ops.fused_trip_reward(plan, fs, float("inf"))
    with pytest.raises(ValueError, match=r"\(B,\)"):
        ops.fused_trip_reward(plan, fs, T0, out=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match=r"\(B, 2\)"):
        ops.fused_trip_reward(plan, fs, T0, parts=torch.zeros((3, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="T_max"):
        ops.fused_set_trip_reward(fs, True, torch.zeros((3, 2), dtype=torch.int32, device="cuda"))
    assert fs.struct.policy_hold == 0


# ---- 2. the one-call rollouts ----------------------------------------------------------------------------------------------------
def _rollout_case(B):
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = synth.torus_network(6, 5, heterogeneous=True, seed=7)
    N, A = net.num_roads, 200
    pops = torch.stack([synth.population(A, N, seed=b, t0=21540, t1=21546) for b in range(B)]).cuda()
    mk = lambda: SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,  # noqa: E731
                           pops.clone(), congestion_constant=net.congestion_constant, seed=11)
    e1, e2 = mk(), mk()
    e1.reset()
    e2.reset()
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()
    dist = ops.all_pairs_shortest_paths(e1.plan, ff, want_next_hop=False, want_dist=True)[1][0]
    return net, e1, e2, dist


@pytest.mark.parametrize("rules", [(), ("hold",), ("router",), ("hold", "router")])
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("head", ["prior", "goal"])
def test_rollouts_with_the_switch_equal_their_launches_one_by_one(head, B, rules):
    """tarl_fused_rollout_prior / tarl_fused_rollout_goal with tarl_fused_set_trip_reward (and, ``rules``, the hold rule and the
    departure router) over T = 6 frames == per frame: logits, draw, [hold,] [pending, route,] the frame, then the trip launch
    with that frame's clock — the reward buffer holds the trip reward, the parts buffer its parts; action bytes, log-probs,
    count bytes and the final state are those of the same rollout with the switch clear, whose reward buffer ``==`` the queue
    reward of the frames queued one by one."""
    import goal_mlp_restatement as G
    from tarl_hip import ops
    from tarl_hip.evaluator import router_buffers
    net, e1, e2, dist = _rollout_case(B)
    N, T, Nmax = net.num_roads, 6, net.Nmax
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    w = ops.GoalMlpWeights(flat=torch.tensor(G.weights(3, True)).cuda())
    scale = ops.goal_time_scale(net.x[:, 3 * Nmax:])
    dests, slot, weights, table, scratch = router_buffers(e1, None, 1)
    ops.fused_edge_travel_time(e1.plan, e1.fs, out=weights)
    ops.destination_trees_batched(e1.plan, weights[:1], dests, out=table, scratch=scratch)
    pend = torch.empty((N, B), dtype=torch.int32, device="cuda")

    def rollout(eng, trip):
        ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
        ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
        lp, rw = torch.zeros((T, B), device="cuda"), torch.full((T, B), float("nan"), device="cuda")
        parts = torch.full((T, B, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        want_word = (1 if "hold" in rules else 0) | (2 if "router" in rules else 0) | (4 if trip else 0)
        if "hold" in rules:
            ops.fused_set_policy_hold(eng.fs, True)
        if "router" in rules:
            ops.fused_set_departure_router(eng.fs, True, slot, table[0], pend, plan=eng.plan)
        if trip:
            ops.fused_set_trip_reward(eng.fs, True, parts)
        assert eng.fs.struct.policy_hold == want_word
        kw = dict(temperature=1.5, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp, reward=rw, counts=ct)
        if head == "prior":
            eng.rollout_prior(T, emb, dist, prior_weight=1.0, **kw)
        else:
            eng.rollout_goal(T, w, dist, scale, None, **kw)
        if trip:
            ops.fused_set_trip_reward(eng.fs, False)
            assert eng.fs.struct.policy_hold == want_word & 3       # the other two bits stay
        if "router" in rules:
            ops.fused_set_departure_router(eng.fs, False)
        if "hold" in rules:
            ops.fused_set_policy_hold(eng.fs, False)
        assert eng.fs.struct.policy_hold == 0
        return ch, ct, lp, rw, parts

    e3 = _rollout_case(B)[1]
    ch, ct, lp, rw, parts = rollout(e1, True)
    ch0, ct0, lp0, rw0, parts0 = rollout(e3, False)
    assert torch.equal(ch, ch0) and torch.equal(ct, ct0) and torch.equal(lp, lp0)
    assert torch.equal(e1.x, e3.x) and torch.equal(e1.agents, e3.agents)
    assert bool((parts0 == 0x7F7F7F7F).all())
    trip2 = torch.empty((T, B), device="cuda")
    parts2 = torch.empty((T, B, 2), dtype=torch.int32, device="cuda")
    counts_f = torch.zeros((N, B), device="cuda")
    for t in range(T):
        if head == "prior":
            logits = ops.fused_prior_logits(e2.plan, e2.fs, e2._x, Nmax, e2.agents, emb, dist, 1.0)
        else:
            logits = ops.fused_goal_mlp_logits(e2.plan, e2.fs, e2._x, Nmax, e2.agents, w, dist, scale)
        c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        lp2 = ops.graphdist_rollout(e2.plan, logits, 1.5, seed=77, counter=5 + t, choice8=c8, sel8=e2.fs.sel8)
        if "hold" in rules:
            ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents)
        clock = float(e2.time)
        if "router" in rules:
            p2 = ops.fused_pending_departures(e2.plan, e2.fs, clock)
            ops.fused_route_departures(e2.plan, e2.fs, p2, slot, table[0])
        e2.frame_fused(skip_choice=True, counts=counts_f)
        ops.fused_trip_reward(e2.plan, e2.fs, clock, out=trip2[t], parts=parts2[t])
        assert torch.equal(c8, ch[t]) and torch.equal(lp2, lp[t]), t
        assert torch.equal(counts_f, ct[t + 1].float()), t
        assert torch.equal(e2.reward, rw0[t]), t               # the switch clear: today's queue reward
        assert torch.equal(trip2[t], rw[t]) and torch.equal(parts2[t], parts[t]), t
        want = R.parts_batch(e2.agents.cpu().numpy(), clock)
        assert np.array_equal(parts2[t].cpu().numpy(), want), t
        # owed = queued + lost + ready with lost >= 0: never fewer on the way than queued
        assert bool((parts2[t][:, 0].float() >= -e2.reward).all())
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert int(parts[-1][:, 0].min()) > 0 and not torch.equal(rw, rw0)


def test_the_switch_without_a_reward_buffer_queues_nothing():
    """``reward=None``: nothing is queued, the parts buffer stays as it was, and the rollout is the one without the switch."""
    from tarl_hip import ops
    net, e1, e2, dist = _rollout_case(3)
    N, T, B = net.num_roads, 6, 3
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    outs = []
    for eng, trip in ((e1, True), (e2, False)):
        ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
        lp = torch.zeros((T, B), device="cuda")
        parts = torch.full((T, B, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        if trip:
            ops.fused_set_trip_reward(eng.fs, True, parts)
        eng.rollout_prior(T, emb, dist, prior_weight=1.0, temperature=1.5, policy_seed=77, policy_counter0=5, choice8=ch,
                          log_prob=lp, reward=None, counts=torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda"))
        ops.fused_set_trip_reward(eng.fs, False)
        assert bool((parts == 0x7F7F7F7F).all())
        outs.append((ch, lp, eng.x.clone(), eng.agents.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------------------
def _trainer_case(reward, hold=True, route=True):
    """A 5 x 4 torus, B = 96, 200 agents, T = 14, the per-edge MLP head -> (trainer on engine 1, twin engine 2,
    logits_of(engine, observation), TEMP)."""
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
    mlp = [pol.edge_mlp[0].weight, pol.edge_mlp[0].bias, pol.edge_mlp[2].weight, pol.edge_mlp[2].bias,
           pol.edge_mlp[4].weight, pol.edge_mlp[4].bias]

    def logits_of(e, obs):
        return ops.policy_edge_mlp(e.plan, obs, e.ec, ops.EdgeMlpWeights(*(p.data for p in mlp)), precision="fp32")
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    e1, e2 = engine(), engine()
    kw = {} if reward is None else {"reward": reward}
    tr = VecPPOTrainer(e1, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=1, sub_batch_size=M,
                       extra_params=extra, policy="edge_mlp", temperature=TEMP, policy_hold=hold, route_departures=route,
                       edge_mlp_params=mlp, policy_precision="fp32", **kw)
    tr.obs_idx = torch.randperm(T * B, generator=torch.Generator().manual_seed(6))[:M]
    return tr, e2, logits_of, TEMP


@pytest.mark.parametrize("reward", ["trip", None])
def test_collect_with_the_trip_reward_equals_its_launches_one_by_one(reward):
    """One ``collect()`` of ``VecPPOTrainer(reward="trip")`` under the hold rule and the departure router against head, draw,
    hold, pending, route, ``frame_fused(skip_choice=True)`` and the trip launch queued one by one on a twin engine: action
    bytes, log-probs, count bytes and the final state bit for bit, ``tr.reward ==`` the trip reward; constructed WITHOUT the
    argument the same trainer stores today's queue reward. The switch is off again afterwards; the update recomputes the
    stored log-probs within the 1e-5 of the existing update tests and one minibatch step runs."""
    from tarl_hip import ops
    from tarl_hip.evaluator import router_buffers
    tr, e2, logits_of, TEMP = _trainer_case(reward)
    e1 = tr.eng
    T, B, N = tr.T, e1.B, e1.N
    assert tr.reward_kind == ("trip" if reward else "queue")
    tr.collect()
    assert e1.fs.struct.policy_hold == 0
    e2.reset()
    dests, slot, weights, table, scratch = router_buffers(e2, None, 1)
    ops.fused_edge_travel_time(e2.plan, e2.fs, out=weights)
    ops.destination_trees_batched(e2.plan, weights[:1], dests, out=table, scratch=scratch)
    ch2 = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct2 = torch.zeros((T + 1, N, B), device="cuda")
    lp2, rw2, trip2 = (torch.zeros((T, B), device="cuda") for _ in range(3))
    pseed = tr.seed ^ 0x5DEECE66D
    for t in range(T):
        obs = ops.fused_obs16(e2.plan, e2.fs, e2._x, e2.Nmax, e2.agents)
        ops.graphdist_rollout(e2.plan, logits_of(e2, obs), TEMP, seed=pseed, counter=1 + t, choice8=ch2[t], sel8=e2.fs.sel8,
                              log_prob=lp2[t])
        ops.fused_hold_policy_actions(e2.plan, e2.fs, e2.agents)
        clock = float(e2.time)
        pend = ops.fused_pending_departures(e2.plan, e2.fs, clock)
        ops.fused_route_departures(e2.plan, e2.fs, pend, slot, table[0])
        e2.frame_fused(skip_choice=True, reward=rw2[t], counts=ct2[t + 1])
        ops.fused_trip_reward(e2.plan, e2.fs, clock, out=trip2[t])
    assert torch.equal(tr.choice, ch2) and torch.equal(tr.logp, lp2) and torch.equal(tr.counts.float(), ct2)
    assert torch.equal(e1.x, e2.x) and torch.equal(e1.agents, e2.agents)
    assert torch.equal(tr.reward, trip2 if reward else rw2)
    assert not torch.equal(trip2, rw2) and bool((trip2 <= rw2).all())          # lost and waiting travellers cost on top
    idx = tr.obs_idx
    lp_dev, _ = ops.graphdist_logprob_entropy(e1.plan, ops.graphdist_softmax(e1.plan, logits_of(e1, tr.obs_mb), TEMP),
                                              choice=ops.rollout_gather(e1.plan, T, B, False, idx.cuda(), choice=tr.choice)[0])
    assert float((lp_dev.cpu() - tr.logp.view(-1).cpu()[idx]).abs().max()) <= 1e-5
    adv, tgt = tr.advantages()
    assert bool(torch.isfinite(tr.minibatch_step(adv, tgt)).all())


def test_the_trainer_refusals():
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = _torus8()
    with pytest.raises(ValueError, match="reward='trip' is not available for policy='embedding'"):
        VecPPOTrainer(_engine(net, _spread_population(net), 1), None, [], rollout_steps=4, policy="embedding", reward="trip")
    with pytest.raises(ValueError, match="'queue' or 'trip'"):
        VecPPOTrainer(_engine(net, _spread_population(net), 1), None, [], rollout_steps=4, policy="embedding", reward="other")


# ---- 4. the evaluator, frame for frame --------------------------------------------------------------------------------------------
def _gumbel_of(ops, eng, noise0, b):
    return lambda t: ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()


@pytest.fixture(scope="module")
def spread_runs():
    """The spread case (8 x 8 torus, 128 agents, 300 frames, K = 3) under the free-flow hold router, with and without the
    first-hop rule: ``VecEvaluator(trip_reward=True)``, the same evaluator without the argument, and the restatement's replay
    of every environment under the device's own noise. -> {route: (evaluator, result, result without, replays)}."""
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    pop = _spread_population(net)
    K, T = 3, 300
    out = {}
    for route in (True, False):
        kw = dict(route_departures=True) if route else {}
        ev = VecEvaluator(_engine(net, pop, K), "dijkstra_hold", refresh_rate=0, trip_reward=True, **kw)
        noise0 = ev.eng.noise_counter + 1
        res = ev.run(T)
        plain = VecEvaluator(_engine(net, pop, K), "dijkstra_hold", refresh_rate=0, **kw)
        off = plain.run(T)
        lost_off = [D.lost(plain.eng.x[b].cpu(), plain.eng.agents[b].cpu(), net.Nmax) for b in range(K)]
        runs = [R.replay(net, pop, T, _gumbel_of(ops, ev.eng, noise0, b), EPISODE_START, R.hold_router(net, pop, route))
                for b in range(K)]
        out[route] = (ev, res, off, lost_off, runs)
    return out


@pytest.mark.parametrize("route", [False, True])
def test_the_evaluator_is_replayed_frame_for_frame(spread_runs, route):
    """Per frame and environment the trip reward and its parts ``==`` the restatement's; ``trip_return`` equal per environment;
    the queue reward, ``episode_return``, every other number of the result and the agents lost ``==`` the same evaluator
    without the argument."""
    ev, res, off, lost_off, runs = spread_runs[route]
    T, K, Nmax = 300, 3, ev.eng.Nmax
    assert not res.domain_exit and res.frames_run == T and res.settings["trip_reward"] is True
    trip, parts, queue = ev.trip_rw[:T].cpu(), ev.trip_parts[:T].cpu(), ev.reward[:T].cpu()
    for b, r in enumerate(runs):
        assert trip[:, b].tolist() == r["trip"], f"trip reward of environment {b}"
        assert parts[:, b, 0].tolist() == r["on_way"] and parts[:, b, 1].tolist() == r["ready"], b
        assert queue[:, b].tolist() == r["queue"], b
        assert torch.equal(r["agents"], ev.eng.agents[b].cpu()) and torch.equal(r["x"], ev.eng.x[b].cpu())
        assert res.trip_return[b] == sum(r["trip"]) and res.episode_return[b] == sum(r["queue"])
        assert res.trip_parts_last[b].tolist() == [r["on_way"][-1], r["ready"][-1]]
        assert D.lost(ev.eng.x[b].cpu(), ev.eng.agents[b].cpu(), Nmax) == r["lost"][-1] == lost_off[b]
        # the identities, per frame
        assert all(-r["trip"][t] == r["queued"][t] + r["lost"][t] + r["ready"][t] for t in range(T))
    assert str(res.trip_parts_last.dtype) == "int64" and res.trip_parts_last.shape == (K, 2)
    g = res.aggregate["trip_return"]
    assert g["mean"] == pytest.approx(np.mean(res.trip_return)) and g["n"] == K
    # without the argument: the same numbers, and none of the new ones
    assert off.trip_return is None and off.trip_parts_last is None and "trip_reward" not in off.settings
    assert "trip_return" not in off.aggregate
    assert off.episode_return == res.episode_return and off.arrived == res.arrived
    assert {k: v for k, v in res.aggregate.items() if k != "trip_return"} == off.aggregate
    assert {k: v for k, v in res.settings.items() if k != "trip_reward"} == off.settings


def test_a_delivered_traveller_is_cheaper_than_a_lost_one(spread_runs):
    """THE TEST THAT FAILS WITHOUT THE FEATURE. With the first-hop rule the free-flow router delivers everybody and loses
    nobody; without it 29 travellers never arrive, 20 of them lost to the U-turn double pop. ``trip_return`` is the higher with
    the rule in every environment, and what is owed after the last frame is exactly the travellers that have not arrived."""
    (_, on, _, lost_on, runs_on), (_, off, _, lost_off, runs_off) = spread_runs[True], spread_runs[False]
    print(f"[trip reward] free_flow on the torus, without -> with the first-hop rule: arrivals {off.arrived} -> {on.arrived}, "
          f"lost {lost_off} -> {lost_on}, return {off.episode_return} -> {on.episode_return}, trip return {off.trip_return} -> "
          f"{on.trip_return}")
    for b in range(3):
        assert on.trip_return[b] > off.trip_return[b]
        for res in (on, off):
            assert int(res.trip_parts_last[b].sum()) == 128 - res.arrived[b]
        assert lost_on[b] < lost_off[b]
        assert off.trip_return[b] < off.episode_return[b]       # the lost travellers cost on top of the queues
    from tarl_hip.evaluator import paired_report
    rep = paired_report(on, off)
    assert rep["metrics"]["trip_return"]["n"] == 3 and rep["metrics"]["trip_return"]["mean"] > 0


def test_the_one_agent_ranking_case_on_the_device():
    """One traveller on the torus, 120 frames, K = 2. Under an ``embedding`` policy whose MODE action sends the origin road to
    its neighbour and the neighbour back, the traveller is lost to the U-turn double pop; the free-flow hold router delivers
    it. The queue return ranks the lost run strictly higher, the trip return the delivered run."""
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    net = _torus8()
    c = R.one_agent_case(net, EPISODE_START)
    T, K = 120, 2
    emb = torch.zeros(net.num_roads)
    emb[c["o"]] = emb[c["v"]] = 5.0
    lost = VecEvaluator(_engine(net, c["pop"], K), "embedding", emb=emb.cuda(), trip_reward=True).run(T)
    delivered = VecEvaluator(_engine(net, c["pop"], K), "dijkstra_hold", refresh_rate=0, trip_reward=True).run(T)
    assert lost.arrived == [0] * K and delivered.arrived == [1] * K
    assert lost.trip_parts_last.tolist() == [[1, 0]] * K and delivered.trip_parts_last.tolist() == [[0, 0]] * K
    print(f"[trip reward, one agent, device] queue return lost {lost.episode_return} / delivered {delivered.episode_return}; "
          f"trip return lost {lost.trip_return} / delivered {delivered.trip_return}")
    for b in range(K):
        assert lost.episode_return[b] > delivered.episode_return[b]
        assert delivered.trip_return[b] > lost.trip_return[b]
        assert delivered.trip_return[b] == delivered.episode_return[b]
        assert lost.trip_return[b] == -float(T - 2)             # departs in frame 2, owed in every frame until the horizon
        assert T >= 2 * -delivered.trip_return[b]


# ---- 5. CLI end to end -----------------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-300"


def _main(argv):
    import importlib
    importlib.import_module("main").main(argv)


def test_cli_eval_envs_end_to_end(tmp_path, capsys):
    import csv
    import json
    out, ref = tmp_path / "ev", tmp_path / "ref"
    base = ["--algo", "mpnn", "--mode", "eval", "--scenario", SCENARIO, "--steps", "60", "--eval-envs", "2", "--eval-baseline",
            "free_flow"]
    _main(base + ["--reward", "trip", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert text.count("trip reward:") == 2 and text.count("trip_return:") == 3          # two blocks and the paired one
    _main(base + ["--output-dir", str(ref)])
    assert "trip" not in capsys.readouterr().out
    doc, old = json.load(open(out / "eval_envs.json")), json.load(open(ref / "eval_envs.json"))
    for key in ("mode", "baseline"):
        assert len(doc[key]["trip_return"]) == 2 and len(doc[key]["trip_parts_last"]) == 2
        assert doc[key]["settings"]["trip_reward"] is True and doc[key]["aggregate"]["trip_return"]["n"] == 2
        assert "trip_return" not in old[key] and "trip_return" not in old[key]["aggregate"]
        for k, v in old[key]["aggregate"].items():      # the old keys: unchanged
            assert doc[key]["aggregate"][k] == v, (key, k)
        assert doc[key]["trip_return"][0] <= doc[key]["aggregate"]["episode_return"]["max"]
    assert doc["paired"]["metrics"]["trip_return"]["n"] == 2 and "trip_return" not in old["paired"]["metrics"]
    assert {k: v for k, v in doc["paired"]["metrics"].items() if k != "trip_return"} == old["paired"]["metrics"]
    rows, old_rows = list(csv.DictReader(open(out / "eval_envs.csv"))), list(csv.DictReader(open(ref / "eval_envs.csv")))
    assert set(rows[0]) - set(old_rows[0]) == {"trip_return", "baseline_trip_return"}
    assert [{k: r[k] for k in o} for r, o in zip(rows, old_rows)] == old_rows
    assert [float(r["trip_return"]) for r in rows] == doc["mode"]["trip_return"]


def test_cli_dijkstra_envs_end_to_end(tmp_path, capsys):
    import json
    out = tmp_path / "dj"
    _main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
           "--dijkstra-envs", "2", "--dijkstra-router", "hold", "--reward", "trip", "--steps", "40", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "trip reward:" in text and "trip_return:" in text
    doc = json.load(open(out / "dijkstra_envs.json"))
    assert len(doc["mode"]["trip_return"]) == 2 and doc["mode"]["settings"]["trip_reward"] is True
    assert "trip_return" in open(out / "dijkstra_envs.csv").readline()


def test_cli_replan_days_end_to_end(tmp_path, capsys):
    import json
    out = tmp_path / "rp"
    _main(["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
           "--replan-days", "2", "--replan-envs", "2", "--reward", "trip", "--steps", "40", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "trip return per day:" in text and "trip reward:" in text
    doc = json.load(open(out / "replan_envs.json"))
    assert len(doc["routes"]["trip_return"]) == 2
    assert [set(d) >= {"trip_return_mean", "trip_return_se"} for d in doc["days"]] == [True, True]
    assert all(d["trip_return_mean"] <= 0 for d in doc["days"])
    assert doc["days"][-1]["trip_return_mean"] == pytest.approx(np.mean(doc["routes"]["trip_return"]))     # the last day IS that run
    head = open(out / "replan_days.csv").readline().strip().split(",")
    assert head[-2:] == ["trip_return_mean", "trip_return_se"]


def test_cli_train_end_to_end(tmp_path):
    import json
    run, ref = tmp_path / "run", tmp_path / "ref"
    base = ["--algo", "mpnn+ppo", "--mode", "train", "--scenario", SCENARIO, "--policy-head", "goal_mlp", "--policy-hold",
            "--route-departures", "--rollout-steps", "32", "--iterations", "2", "--eval-envs", "2", "--steps", "5"]
    _main(base + ["--reward", "trip", "--output-dir", str(run)])
    _main(base + ["--output-dir", str(ref)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    old = [json.loads(l) for l in open(ref / "train_log.jsonl")]
    assert len(logs) == 2 and len(old) == 2
    for rec, o in zip(logs, old):
        assert rec["train/reward_kind"] == "trip" and rec["eval_vec/trip_return"] <= rec["eval_vec/avg_return"] <= 0
        assert "eval_vec/trip_return_se" in rec
        assert set(rec) - set(o) == {"train/reward_kind", "eval_vec/trip_return", "eval_vec/trip_return_se"}
    # iteration 0 collects with the same parameters: the same frames, another reward
    assert logs[0]["PPO/avg_episode_return"] <= old[0]["PPO/avg_episode_return"]
    assert logs[0]["eval_vec/avg_return"] == old[0]["eval_vec/avg_return"]


def test_cli_refusals():
    for argv, msg in ((["--algo", "mpnn", "--mode", "eval", "--reward", "trip"], "eval_envs > 0"),
                      (["--algo", "dijkstra", "--mode", "eval", "--reward", "trip"], "replan_days > 0"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--reward", "trip"], "state-dependent head"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "embedding", "--reward", "trip"],
                       "reward trip cannot train")):
        with pytest.raises(ValueError, match=msg):
            _main(argv + ["--scenario", SCENARIO])
