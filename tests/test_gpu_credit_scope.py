"""GPU: credit scope "due" and the horizon bootstrap of the per-decision PPO credit — tarl_fused_head_rows_due
and tarl_fused_agent_roads against ``credit_scope_restatement`` on the exported state (packed random states of the torus at,
below and above one tile of 256 roads and of both irregular graphs, live states after 20 and 40 frames, B in {1, 3, 65},
outputs between guard bands, the packed state compared whole), tarl_decision_advantage_boot against the plain entry point bit
for bit and against float64 within ``update_restatement.tensor_bound``, the one-call rollouts with the scope against the same
calls without it and against the launches made one by one, ``VecPPOTrainer(credit_scope=, credit_horizon=)``, the default bit
for bit, the case that fails without the feature, and the CLI."""
import json

import numpy as np
import pytest
import torch

import credit_scope_restatement as CS
import decision_credit_restatement as DC
import irregular_graphs as ig
import test_gpu_decision_credit as TD
import test_gpu_decision_critic as TC
import update_restatement as R

pytestmark = pytest.mark.gpu

GUARD = TD.GUARD
GRAPHS = TD.GRAPHS
PAIRS = lambda B: (([], []), ([B - 1], [3]), ([b % B for b in (0, 2, 64, 1, 33)], [6, 0, 2, 5, 1]))      # noqa: E731  n = 0, 1, 5
ROWS = 7


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _packed_random(ops, net, B, t=200.0):
    """test_gpu_decision_credit's packed random states, with two additions: every empty road that kept a stale id also gets a
    stale, early dep word (the pack stores slot 0 verbatim), and road 1 of environment 0 is filled to Nmax - 1 with fresh ids:
    its last slot is in use, the row is DIRTY. -> (plan, fs, exported x on the host, A)."""
    from tarl_hip import synth
    Nmax, N = net.Nmax, net.num_roads
    x = torch.stack([ig.random_state(net, seed=100 + b, t=t) for b in range(B)])
    empty = x[:, :, 3 * Nmax + 1] == 0
    x[:, :, 2 * Nmax] = torch.where(empty & (x[:, :, 0] != 0), torch.full_like(x[:, :, 0], t - 50.0), x[:, :, 2 * Nmax])
    top = int(x[:, :, :Nmax].max())
    x[0, 1, :Nmax - 1] = top + 1 + torch.arange(Nmax - 1, dtype=torch.float32)
    x[0, 1, Nmax:2 * Nmax - 1] = t - 5.0
    x[0, 1, 2 * Nmax:3 * Nmax - 1] = t + 3.0
    x[0, 1, 3 * Nmax + 1] = float(Nmax - 1)
    A = top + Nmax + 1
    ag = torch.stack([synth.population(A - 1, N, seed=b, t0=100, t1=130) for b in range(B)])
    plan = ops.Plan(net.edge_index, N)
    fs = ops.FusedState(plan, B, A, "cuda", Nmax)
    ops.fused_pack(plan, fs, x.cuda(), Nmax, ag.cuda(), net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    out = x.clone().cuda()
    ops.fused_export(plan, fs, out, Nmax, t)
    return plan, fs, out.cpu(), A


def _snapshot(fs):
    return {k: getattr(fs, k).clone() for k in TD.PACKED}


def _unchanged(fs, before):
    for k, v in before.items():
        assert torch.equal(getattr(fs, k), v), f"the kernel touched fs.{k}"


def _due_launch(ops, plan, fs, env, slot, clock):
    """The op into a 0x7F-filled buffer between guard bands, twice -> (head_keep (ROWS, N), counts (2,)) on the host; the
    packed state is compared whole before and after."""
    N, pad = plan.num_nodes, 64
    before = _snapshot(fs)
    outs = []
    for _ in range(2):
        big = torch.full((ROWS * N + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
        hk = big[pad:pad + ROWS * N].view(ROWS, N)
        cbig = torch.full((2 + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
        counts = cbig[pad:pad + 2]
        counts.zero_()
        ops.fused_head_rows(plan, fs, torch.tensor(env, dtype=torch.int32).cuda(), torch.tensor(slot, dtype=torch.int32).cuda(),
                            hk, t=clock, counts=counts)
        torch.cuda.synchronize()
        assert bool((big[:pad] == GUARD).all()) and bool((big[pad + ROWS * N:] == GUARD).all())
        assert bool((cbig[:pad] == GUARD).all()) and bool((cbig[pad + 2:] == GUARD).all())
        outs.append((hk.cpu(), counts.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _unchanged(fs, before)
    return outs[0]


def _check_due(ops, plan, fs, x_host, Nmax, B, clock):
    """Every pair list of PAIRS at ``clock`` against the restatement on the exported x -> the due decisions seen."""
    want, headed, due = CS.due_heads(x_host.numpy(), Nmax, clock)
    want = torch.from_numpy(want).to(torch.int32)
    seen = 0
    for env, slot in PAIRS(B):
        hk, counts = _due_launch(ops, plan, fs, env, slot, clock)
        for e, s in zip(env, slot):
            assert torch.equal(hk[s], want[e]), (e, s, clock)
        for s in range(ROWS):
            if s not in slot:
                assert bool((hk[s] == GUARD).all()), s
        assert counts.tolist() == [int(sum(headed[e].sum() for e in env)), int(sum(due[e].sum() for e in env))], (env, clock)
        seen += counts[1].item()
    return seen


def _clocks_around(x_host, Nmax, B):
    """The dep of a head of one of the listed environments exactly, one ulp below and one ulp above (fp32)."""
    envs = sorted({e for env, _ in PAIRS(B) for e in env})
    xs = x_host[envs]
    headed = xs[:, :, 3 * Nmax + 1] > 0
    d0 = np.float32(xs[:, :, 2 * Nmax][headed].median().item())         # (the lower median: an element)
    assert bool((xs[:, :, 2 * Nmax][headed] == float(d0)).any())
    return [float(d0), float(np.nextafter(d0, np.float32(-np.inf))), float(np.nextafter(d0, np.float32(np.inf)))]


# ---- 1. tarl_fused_head_rows_due -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_head_rows_due_on_packed_states(name, B):
    """Result and ``counts2`` ``==`` the restatement on the exported x with the clock exactly at, one ulp below and one ulp
    above a head's dep; empty roads with a stale id and a stale early dep word stay 0 (the count test protects them)."""
    from tarl_hip import ops
    net = TD._net(name)
    plan, fs, x, _ = _packed_random(ops, net, B)
    cnt = fs.hdp[..., 0] & 0x7F
    dep_word = fs.hdp[..., 1].contiguous().view(torch.float32)
    clocks = _clocks_around(x, net.Nmax, B)
    assert bool(((cnt == 0) & (dep_word <= min(clocks)) & ((fs.hdp[..., 0] >> 8) != 0)).any()), "no stale empty road to protect"
    got = [_check_due(ops, plan, fs, x, net.Nmax, B, c) for c in clocks]
    assert got[1] < got[0] <= got[2] and got[1] > 0                 # at the dep: due; one ulp below: not
    assert not np.array_equal(CS.due_heads(x.numpy(), net.Nmax, clocks[0], defect="strict_less")[0],
                              CS.due_heads(x.numpy(), net.Nmax, clocks[0])[0])      # what the clock at the dep would catch
    again = x.clone().cuda()
    ops.fused_export(plan, fs, again, net.Nmax, 200.0)
    assert torch.equal(again.cpu(), x), "the exported state changed"


def _hold_frames(eng, frames, emb, dist):
    """``frames`` frames of the prior head under the hold rule (agents are delivered: FIFOs pop and their rings turn)."""
    from tarl_hip import ops
    ops.fused_set_policy_hold(eng.fs, True)
    TD._run_prior(eng, frames, emb, dist)
    ops.fused_set_policy_hold(eng.fs, False)


@pytest.mark.parametrize("B", [3, 65])
def test_head_rows_due_and_agent_roads_on_live_states(B):
    """After a reset nothing is due and nobody is queued; after 20 and 40 frames of the prior head under the hold rule both
    kernels ``==`` the restatement on the exported state: the clock the next frame is stepped with, and the clocks around a
    head's dep; rings with ``hoff != 0`` among the rows."""
    from tarl_hip import ops
    net, eng, dist = TD._live_case(B)
    Nmax, A = net.Nmax, eng.A
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(3)).cuda()
    hk, counts = _due_launch(ops, eng.plan, eng.fs, [0, B - 1, 1], [2, 0, 1], float(eng.time))
    assert not bool(hk[:3].any()) and counts.tolist() == [0, 0]
    assert bool((_agent_roads(ops, eng.plan, eng.fs, Nmax, B, A) == -1).all())
    for _ in range(2):
        _hold_frames(eng, 20, emb, dist)
        x = eng.x.cpu()
        seen = _check_due(ops, eng.plan, eng.fs, x, Nmax, B, float(eng.time))
        for c in _clocks_around(x, Nmax, B):
            _check_due(ops, eng.plan, eng.fs, x, Nmax, B, c)
        assert seen > 0
        road = _agent_roads(ops, eng.plan, eng.fs, Nmax, B, A)
        want, bad, twice = CS.agent_roads(x[:, :, :Nmax].numpy().astype(np.int64), x[:, :, 3 * Nmax + 1].numpy(), A)
        assert np.array_equal(road.numpy(), want) and bad == 0 and twice == 0
        hoff = (eng.fs.tl >> 1) & 127
        assert bool(((hoff != 0) & ((eng.fs.hdp[..., 0] & 0x7F) > 0)).any()), "no turned ring among the occupied rows"
        assert int((road >= 0).sum()) >= 10
        assert torch.equal(eng.x.cpu(), x), "the exported state changed"
    done = eng.agents[:, :, 8].cpu() == 1
    assert bool((road[done] == -1).all())                           # who has arrived stands nowhere
    eng.check_flags()


# ---- 2. tarl_fused_agent_roads -----------------------------------------------------------------------------------------------------
def _agent_roads(ops, plan, fs, Nmax, B, A):
    """The op into a garbage-filled buffer between guard bands, twice -> (B, A) on the host; ``bad == 0``; the packed state is
    compared whole before and after."""
    pad = 64
    before = _snapshot(fs)
    outs = []
    for fill in (GUARD, 5):
        big = torch.full((B * A + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
        out = big[pad:pad + B * A].view(B, A)
        out.fill_(fill)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.fused_agent_roads(plan, fs, Nmax, out=out, bad=bad)
        torch.cuda.synchronize()
        assert bool((big[:pad] == GUARD).all()) and bool((big[pad + B * A:] == GUARD).all())
        assert int(bad) == 0
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    _unchanged(fs, before)
    return outs[0]


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_agent_roads_on_packed_states(name, B):
    """``==`` the restatement on the exported x: stale ids above the count (the slot AT the count among them) map nowhere, a
    row PRE-FILLED to Nmax - 1 by the pack is DIRTY and maps all its agents (filled, not driven there by frames: the insert stops
    at MAX - 3 and only three gridlock-relief admissions in a row reach Nmax - 1, one more leaves the defined domain, so no live
    run of a few frames lands there on demand; the kernel reads the same words either way); an agent table too short for the ids
    adds to ``bad``."""
    from tarl_hip import ops
    net = TD._net(name)
    Nmax = net.Nmax
    plan, fs, x, A = _packed_random(ops, net, B)
    assert int(fs.hdp[1, 0, 0]) & 0x80 and (int(fs.hdp[1, 0, 0]) & 0x7F) == Nmax - 1      # the filled row: dirty
    road = _agent_roads(ops, plan, fs, Nmax, B, A)
    ids, count = x[:, :, :Nmax].numpy().astype(np.int64), x[:, :, 3 * Nmax + 1].numpy()
    want, bad, twice = CS.agent_roads(ids, count, A)
    assert np.array_equal(road.numpy(), want) and bad == 0 and twice == 0
    assert int((road[0] == 1).sum()) == Nmax - 1 and bool((road == -1).any())
    garbage = CS.agent_roads(ids, count, A, defect="garbage_slot_read")[0]
    assert not np.array_equal(garbage, want), "no stale id at a count: the case would not catch the garbage slot"
    again = x.clone().cuda()
    ops.fused_export(plan, fs, again, Nmax, 200.0)
    assert torch.equal(again.cpu(), x), "the exported state changed"
    # ids at or beyond a shorter table are counted, not followed
    short = A - (Nmax - 1)
    fs.A = short
    try:
        out = torch.full((B, short), 7, dtype=torch.int32, device="cuda")
        bad_d = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.fused_agent_roads(plan, fs, Nmax, out=out, bad=bad_d)
        want_s, bad_s, _ = CS.agent_roads(ids, count, short)
        assert np.array_equal(out.cpu().numpy(), want_s) and int(bad_d) == bad_s and bad_s > 0
    finally:
        fs.A = A


# ---- 3. tarl_decision_advantage_boot -------------------------------------------------------------------------------------------------
def _boot_inputs(name):
    """test_gpu_decision_credit's crafted advantage buffers plus where every agent stands at the end of either segment:
    a third of the agents nowhere, the others on a random road (some with an unreachable destination from there)."""
    c = TD._advantage_inputs(name)
    rng = np.random.default_rng(11)
    c["roads"] = [np.where(rng.random((c["B"], c["A"])) < 0.33, -1, rng.integers(0, c["N"], (c["B"], c["A"]))).astype(np.int32)
                  for _ in range(2)]
    return c


def _segments(c):
    return ((c["tables"][0], c["roads"][0], 0, c["t_mid"]), (c["tables"][1], c["roads"][1], c["t_mid"], c["T"]))


def _restated_boot(c, dist, gamma, flags):
    adv, live = np.zeros((c["rows"], c["N"])), np.zeros((c["rows"], c["N"]), dtype=bool)
    trunc = boot = bad = 0
    for (ag, road, lo_t, hi_t), flag in zip(_segments(c), flags):
        sel = np.nonzero((c["frame"] >= lo_t) & (c["frame"] < hi_t))[0]
        r = CS.decision_advantage_boot(c["head"][c["slot"][sel]], c["frame"][sel], c["env"][sel], ag, c["times"], hi_t, dist,
                                       c["dest_slot"], c["deg"], road, flag, 1.0, gamma)
        adv[c["slot"][sel]], live[c["slot"][sel]] = r["adv"], r["live"]
        trunc, boot, bad = trunc + r["truncated"], boot + r["bootstrapped"], bad + r["bad"]
    return adv, live, trunc, boot, bad


def _device_boot(ops, plan, c, dist, gamma, flags):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()      # noqa: E731
    hk = dev(c["head"], torch.int32)
    adv = torch.full((c["rows"], c["N"]), float("nan"), device="cuda")
    trunc, bad, boot = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    frame, env, slot = (dev(c[k], torch.int32) for k in ("frame", "env", "slot"))
    for (ag, road, lo_t, hi_t), flag in zip(_segments(c), flags):
        sel = np.nonzero((c["frame"] >= lo_t) & (c["frame"] < hi_t))[0]
        lo, hi = int(sel[0]), int(sel[-1]) + 1                   # the rows are sorted by frame: a segment is a run
        ops.decision_advantage(plan, hk, frame[lo:hi], env[lo:hi], slot[lo:hi], dev(ag, torch.float32),
                               dev(c["times"], torch.float32), hi_t, dev(dist, torch.float64), dev(c["dest_slot"], torch.int32),
                               B=c["B"], timestep=1, decision_gamma=gamma, adv_raw=adv, truncated=trunc, bad=bad,
                               agent_road=dev(road, torch.int32), bootstrap=flag, bootstrapped=boot)
    torch.cuda.synchronize()
    return hk, adv, int(trunc), int(boot), int(bad)


@pytest.mark.parametrize("name", GRAPHS)
def test_advantage_boot_against_the_plain_call_and_float64(name):
    """``bootstrap = 0``: every output ``==`` tarl_decision_advantage's, bit for bit. ``bootstrap = 1``: the live mask,
    ``truncated``, ``bootstrapped`` and ``bad`` ``==`` the restatement, ``adv_raw`` within ``tensor_bound`` (e32: the rounding
    of the float64 value to fp32) for gamma in {1, 0.99}; a segment ends inside the batch (two calls, two agent tables, two
    tables of roads), once as an episode end that keeps the charge and once cut twice."""
    from tarl_hip import ops
    c = _boot_inputs(name)
    plan = ops.Plan(c["net"].edge_index, c["N"])
    for gamma in (1.0, 0.99):
        hk0, adv0, trunc0, bad0 = TD._device_advantage(ops, plan, c, c["dist"], gamma)
        hk, adv, trunc, boot, bad = _device_boot(ops, plan, c, c["dist"], gamma, (False, False))
        assert torch.equal(hk, hk0) and torch.equal(adv.view(torch.int32), adv0.view(torch.int32))
        assert (trunc, boot, bad) == (trunc0, 0, bad0)
        for flags in ((False, True), (True, True)):
            want, live, w_trunc, w_boot, w_bad = _restated_boot(c, c["dist"], gamma, flags)
            hk, adv, trunc, boot, bad = _device_boot(ops, plan, c, c["dist"], gamma, flags)
            assert np.array_equal((hk > 0).cpu().numpy(), live) and np.array_equal((hk0 > 0).cpu().numpy(), live)
            assert (trunc, boot, bad) == (w_trunc, w_boot, w_bad) and boot > 0 and trunc > 0 and trunc + boot == trunc0
            w64 = torch.from_numpy(want)
            b = R.tensor_bound(R.max_err(w64.float(), w64), w64)
            err = R.max_err(adv.cpu(), w64)
            moved = int((adv.cpu() != adv0.cpu()).sum())
            print(f"[decision advantage boot {name} gamma={gamma} flags={flags}] {int(live.sum())} live, {boot} bootstrapped, "
                  f"{trunc} truncated, {moved} elements moved, err {err:.3e} (bound {b:.3e})")
            assert err <= b and moved > 0
            again = _device_boot(ops, plan, c, c["dist"], gamma, flags)
            assert torch.equal(again[1].view(torch.int32), adv.view(torch.int32)) and again[2:] == (trunc, boot, bad)


# ---- 4. the rollouts with scope due --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("head", ["prior", "goal"])
def test_rollouts_with_scope_due(head, B):
    """tarl_fused_rollout_prior / _goal over T = 6 frames with the capture's scope set to due: action bytes, log-probs, count
    bytes, rewards, kept observations and the final state ``==`` the same call without the capture; ``head_keep`` and the
    counters ``==`` the launches made one by one in front of every frame of a twin engine run one frame per call, and its
    non-zero entries are entries of the headed capture."""
    import goal_mlp_restatement as G
    from tarl_hip import ops
    T = 6
    net, e1, dist = TD._live_case(B, "torus6x5", agents=200)
    engines = [e1] + [TD._live_case(B, "torus6x5", agents=200)[1] for _ in range(3)]
    N, Nmax = net.num_roads, net.Nmax
    emb = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    w = ops.GoalMlpWeights(flat=torch.tensor(G.weights(3, True)).cuda())
    scale = ops.goal_time_scale(net.x[:, 3 * Nmax:])
    gen = torch.Generator().manual_seed(5)
    per_frame = [1, 0, 3, 2, 4, 2]
    ptr = [0] + [int(v) for v in np.cumsum(per_frame)]
    K = ptr[-1]
    kenv = torch.randint(0, B, (K,), generator=gen).to(torch.int32).cuda()
    kslot = torch.randperm(K, generator=gen).to(torch.int32).cuda()

    def buffers(frames):
        return dict(choice8=torch.zeros((frames, B, N), dtype=torch.uint8, device="cuda"),
                    counts=torch.zeros((frames + 1, N, B), dtype=torch.uint8, device="cuda"),
                    log_prob=torch.zeros((frames, B), device="cuda"), reward=torch.zeros((frames, B), device="cuda"))

    def run(eng, frames, counter0, keep, obs, out):
        kw = dict(temperature=1.5, policy_seed=77, policy_counter0=counter0, keep=keep, obs_keep=obs, **out)
        if head == "prior":
            eng.rollout_prior(frames, emb, dist, prior_weight=1.0, **kw)
        else:
            eng.rollout_goal(frames, w, dist, scale, None, **kw)

    def rollout(eng, scope):
        obs = torch.zeros((K, N, 16), device="cuda")
        hk = torch.full((K, N), GUARD, dtype=torch.int32, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        if scope is not None:
            ops.fused_set_head_capture(eng.fs, True, hk, plan=eng.plan, scope=scope, counts=counts if scope == "due" else None)
            assert eng.fs.struct.policy_hold == 8
        out = buffers(T)
        run(eng, T, 5, (ptr, kenv, kslot), obs, out)
        if scope is not None:
            ops.fused_set_head_capture(eng.fs, False)
        assert eng.fs.struct.policy_hold == 0
        return out, obs, hk, counts

    for e in engines:                                           # 20 frames in: heads that travel and heads that are due
        TD._run_prior(e, 20, emb, dist)
    assert all(torch.equal(e.x, e1.x) for e in engines[1:])
    e_due, e_plain, e_headed, e_twin = engines
    out1, obs1, hk1, c1 = rollout(e_due, "due")
    out0, obs0, hk0, _ = rollout(e_plain, None)
    _, _, hkh, _ = rollout(e_headed, "headed")
    for k in out1:
        assert torch.equal(out1[k], out0[k]), k
    assert torch.equal(obs1, obs0) and torch.equal(e_due.x, e_plain.x) and torch.equal(e_due.agents, e_plain.agents)
    assert bool((hk0 == GUARD).all()) and not bool((hk1 == GUARD).any()) and not bool((hkh == GUARD).any())
    # the launches one by one, in front of every frame of the twin, one frame per call
    hk2 = torch.full((K, N), GUARD, dtype=torch.int32, device="cuda")
    c2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    obs2 = torch.zeros((K, N, 16), device="cuda")
    for t in range(T):
        lo, hi = ptr[t], ptr[t + 1]
        if hi > lo:
            ops.fused_head_rows(e_twin.plan, e_twin.fs, kenv[lo:hi], kslot[lo:hi], hk2, t=float(e_twin.time), counts=c2)
        out = buffers(1)
        run(e_twin, 1, 5 + t, ([0, hi - lo], kenv[lo:hi], kslot[lo:hi]) if hi > lo else None, obs2, out)
        assert torch.equal(out["choice8"][0], out1["choice8"][t]) and torch.equal(out["log_prob"][0], out1["log_prob"][t]), t
        assert torch.equal(out["counts"][1], out1["counts"][t + 1]) and torch.equal(out["reward"][0], out1["reward"][t]), t
    assert torch.equal(hk1, hk2) and torch.equal(c1, c2)
    assert torch.equal(e_due.x, e_twin.x) and torch.equal(e_due.agents, e_twin.agents) and torch.equal(obs1, obs2)
    due, headed = hk1 > 0, hkh > 0
    assert bool((~due | headed).all()) and torch.equal(hk1[due], hkh[due])
    assert c1.tolist() == [int(headed.sum()), int(due.sum())] and 0 < int(due.sum()) < int(headed.sum())
    e_due.check_flags()


# ---- 5. the trainer ----------------------------------------------------------------------------------------------------------------
def _split_rollouts(tr, states):
    """Make the trainer's engine queue its segment one frame per call and record, in front of every frame, the exported state
    and the clock (what the scope's restatement reads)."""
    eng = tr.eng
    whole = eng.rollout_goal

    def frame_by_frame(n, *a, policy_counter0, choice8, log_prob, reward, counts, keep, **kw):
        times = []
        for i in range(n):
            states.append((eng.x.cpu(), float(eng.time)))
            sub = None
            if keep is not None and keep[0][i + 1] > keep[0][i]:
                lo, hi = keep[0][i], keep[0][i + 1]
                sub = ([0, hi - lo], keep[1][lo:hi], keep[2][lo:hi])
            got = whole(1, *a, policy_counter0=policy_counter0 + i, choice8=choice8[i:i + 1], log_prob=log_prob[i:i + 1],
                        reward=reward[i:i + 1], counts=counts[i:i + 2], keep=sub, **kw)
            times += got[:-1]
        return times + [got[-1]]
    eng.rollout_goal = frame_by_frame


def test_the_defaults_are_bit_identical():
    """``credit_scope="headed", credit_horizon="charge"``: buffers, gradient, parameters and report ``==`` those of a trainer
    built without the arguments."""
    a, _ = TC._trainer(credit="decision", credit_scope="headed", credit_horizon="charge")
    b, _ = TC._trainer(credit="decision")
    a.train_iteration()
    b.train_iteration()
    assert torch.equal(a.last_grad, b.last_grad) and torch.equal(a.flat.flat, b.flat.flat)
    assert torch.equal(a.choice, b.choice) and torch.equal(a.logp, b.logp) and torch.equal(a.last["losses"], b.last["losses"])
    assert torch.equal(a.head_keep, b.head_keep) and torch.equal(a.adv_raw.view(torch.int32), b.adv_raw.view(torch.int32))
    assert set(a.last["decision"]) == set(b.last["decision"]) == {"decisions", "delay_frames", "truncated", "objective",
                                                                  "clip_fraction", "kl"}
    for k, v in a.last["decision"].items():
        assert torch.equal(v, b.last["decision"][k]), k
    assert not hasattr(a, "agent_road") and not hasattr(a, "decision_counts")


def test_due_and_bootstrap_buffers_against_the_restatement():
    """``credit_scope="due", credit_horizon="bootstrap"`` (goal_mlp, torus, B = 3, two epochs): ``head_keep``, the counters
    and ``adv_raw`` against the restatement driven by the state in front of every kept frame and by the final state (one
    segment, cut by the batch: bootstrapped); a trainer whose rollout is one call gives the same buffers bit for bit."""
    kw = dict(credit="decision", credit_scope="due", credit_horizon="bootstrap")
    tr, net = TC._trainer(**kw)
    whole, _ = TC._trainer(**kw)
    states = []
    _split_rollouts(tr, states)
    tr.train_iteration()
    whole.train_iteration()
    tr.check_flags()
    assert torch.equal(tr.head_keep, whole.head_keep) and torch.equal(tr.adv_raw.view(torch.int32), whole.adv_raw.view(torch.int32))
    assert torch.equal(tr.choice, whole.choice) and torch.equal(tr.flat.flat, whole.flat.flat)
    assert torch.equal(tr.decision_counts, whole.decision_counts) and torch.equal(tr.agent_road, whole.agent_road)
    eng, N, Nmax = tr.eng, tr.eng.N, net.Nmax
    assert len(states) == tr.T and eng.fs.struct.policy_hold == 0
    frames = np.asarray(tr._keep[0])
    env, slot = tr._keep[1].cpu().numpy(), tr._keep[2].cpu().numpy()
    captured = np.zeros((len(frames), N), dtype=np.int64)
    headed = due = 0
    for j, (t, b) in enumerate(zip(frames, env)):
        x, clock = states[t]
        h, hd, du = CS.due_heads(x[b:b + 1].numpy(), Nmax, clock)
        captured[j], headed, due = h[0], headed + int(hd.sum()), due + int(du.sum())
    assert tr.decision_counts.tolist() == [headed, due] and 0 < due < headed
    x_end = eng.x.cpu().numpy()
    road, bad, twice = CS.agent_roads(x_end[:, :, :Nmax].astype(np.int64), x_end[:, :, 3 * Nmax + 1], eng.A)
    assert np.array_equal(tr.agent_road.cpu().numpy(), road) and bad == 0 and twice == 0
    dist, dslot = tr._decision_dist
    from tarl_hip.engine import EPISODE_END
    assert CS.segment_bootstrap(float(eng.time), EPISODE_END)
    r = CS.decision_advantage_boot(captured, frames, env, eng.agents.cpu().numpy(), tr.times.cpu().numpy(), tr.T,
                                   dist.cpu().numpy(), dslot.cpu().numpy(), np.full(N, 4), road, True, eng.timestep, 1.0)
    hk, adv = tr.head_keep.cpu().numpy(), tr.adv_raw.cpu().numpy()
    assert np.array_equal(hk[slot], np.where(r["live"], captured, 0)) and r["bad"] == 0
    assert (int(tr.decision_truncated), int(tr.decision_bootstrapped)) == (r["truncated"], r["bootstrapped"])
    assert r["bootstrapped"] > 0 and r["live"].sum() > 10
    a64 = torch.from_numpy(r["adv"])
    err, b = R.max_err(torch.from_numpy(adv[slot]), a64), R.tensor_bound(R.max_err(a64.float(), a64), a64)
    print(f"[credit scope trainer] headed {headed}, due {due}, live {int(r['live'].sum())}, bootstrapped {r['bootstrapped']}, "
          f"truncated {r['truncated']}, adv err {err:.3e} (bound {b:.3e})")
    assert err <= b
    rep = tr.last["decision"]
    live = int(r["live"].sum())
    assert rep["credit_scope"] == "due" and rep["credit_horizon"] == "bootstrap"
    assert float(rep["decisions"]) == live and float(rep["decisions_headed"]) == headed
    assert float(rep["bootstrapped"]) == r["bootstrapped"] / live and float(rep["truncated"]) == r["truncated"] / live


@pytest.mark.parametrize("kw", [dict(credit_scope="due"), dict(credit_horizon="bootstrap"),
                                dict(credit_scope="due", credit_horizon="bootstrap")], ids=["due", "bootstrap", "both"])
def test_they_run_with_the_learned_baseline(kw):
    tr, _ = TC._trainer("learned", **kw)
    before = tr.flat.flat.clone()
    tr.train_iteration()
    tr.check_flags()
    rep = tr.last["decision"]
    nums = {k: float(v) for k, v in rep.items() if not isinstance(v, str)}
    assert all(np.isfinite(v) for v in nums.values()) and nums["decisions"] > 0
    assert ("decisions_headed" in rep) == ("credit_scope" in kw) and ("bootstrapped" in rep) == ("credit_horizon" in kw)
    assert {"critic_loss", "explained_variance", "value_mean"} <= set(rep)
    assert bool(torch.isfinite(tr.flat.flat).all()) and not torch.equal(tr.flat.flat, before)
    assert tr.eng.fs.struct.policy_hold == 0


def test_a_head_that_is_not_due_gets_no_gradient():
    """THE TEST THAT FAILS WITHOUT THE FEATURE. Entropy coefficient 0: under ``credit_scope="due"`` the gradient of the logits
    is exactly 0 on every out-edge of every road whose head was not due; under ``"headed"`` the same frames do put gradient
    on such edges (roads whose head was still travelling).
    "Not due" is read from the trainer's own ``head_keep`` here, so this test alone is not independent of the kernel under
    test: ``test_due_and_bootstrap_buffers_against_the_restatement`` pins that buffer to the float64 restatement."""
    seen = {}
    for scope in ("due", "headed"):
        tr, net = TC._trainer(credit="decision", epochs=1, entropy_coef=0.0, credit_scope=scope)
        _, g_seen = TD._record_steps(tr)
        tr.collect()
        live = tr.head_keep.cpu() > 0
        tr.update()
        seen[scope] = (g_seen[0].cpu(), live[:tr.M][:, net.edge_index[0]], tr.choice.clone())
    assert torch.equal(seen["due"][2], seen["headed"][2])                  # the same rollout, the same minibatch draw
    g, due, _ = seen["due"]
    assert int((~due).sum()) > 0 and not bool(g[~due].any()) and bool(g[due].any())
    g, headed, _ = seen["headed"]
    travelling = headed & ~due
    assert bool(headed[due].all())
    assert int(travelling.sum()) > 0 and bool(g[travelling].any())


# ---- 6. CLI end to end ---------------------------------------------------------------------------------------------------------------
NEW_KEYS = {"train/credit_scope", "train/credit_horizon", "train/decisions_headed", "train/decision_bootstrapped"}


def test_cli_train_end_to_end(tmp_path):
    run, ref = tmp_path / "run", tmp_path / "ref"
    base = ["--algo", "mpnn+ppo", "--mode", "train", "--scenario", TD.SCENARIO, "--policy-head", "goal_mlp", "--policy-hold",
            "--route-departures", "--rollout-steps", "256", "--iterations", "2", "--steps", "5", "--credit", "decision"]
    TD._main(base + ["--credit-scope", "due", "--credit-horizon", "bootstrap", "--output-dir", str(run)])
    TD._main(base + ["--output-dir", str(ref)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    old = [json.loads(l) for l in open(ref / "train_log.jsonl")]
    assert len(logs) == 2 and len(old) == 2
    assert set(logs[0]) - set(old[0]) == NEW_KEYS and set(old[0]) <= set(logs[0])
    for rec, o in zip(logs, old):
        assert NEW_KEYS <= set(rec) and not NEW_KEYS & set(o) and TD.NEW_KEYS <= set(o)
        assert rec["train/credit_scope"] == "due" and rec["train/credit_horizon"] == "bootstrap"
        assert rec["train/decisions_headed"] >= rec["train/decisions"] > 0
        assert 0.0 <= rec["train/decision_bootstrapped"] <= 1.0 and 0.0 <= rec["train/decision_truncated"] <= 1.0
        assert rec["train/decision_bootstrapped"] + rec["train/decision_truncated"] <= 1.0
    # iteration 0 collects with the same parameters: the same frames, fewer decisions in scope
    assert logs[0]["PPO/avg_episode_return"] == old[0]["PPO/avg_episode_return"]
    assert logs[0]["train/held"] == old[0]["train/held"]
    assert logs[0]["train/decisions"] <= old[0]["train/decisions"]


def test_cli_refusals():
    base = ["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--scenario", TD.SCENARIO]
    for extra in (["--credit-scope", "due"], ["--credit-horizon", "bootstrap"]):
        with pytest.raises(ValueError, match="needs credit decision"):
            TD._main(base + extra)
    with pytest.raises(ValueError, match="mode 'train'"):
        TD._main(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--credit", "decision", "--credit-scope", "due",
                  "--scenario", TD.SCENARIO])
