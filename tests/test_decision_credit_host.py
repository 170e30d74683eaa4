"""CPU: per-decision PPO credit on the restatement and the CPU oracle — the frame count of a decision against
the oracle's agent table frame by frame (the "spread" case, with and without the first-hop rule, a lost agent and an agent
withdrawn in the frame after it became a head among them), the sign of the gradient, every named defect against ten times the
tolerance the GPU tests use, the host checks of the entry points, the four switches of one word, and the argument rules."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import decision_credit_restatement as DC
import update_restatement as R
from fake_plan import fake_plan as _plan


# ---- 1. the frame count against the oracle -------------------------------------------------------------------------------------
def _spread_record(route):
    """The "spread" case (8 x 8 torus, 128 agents, 300 frames, free-flow hold router), with the state in front of every
    frame and the agent table after every frame kept. -> dict: heads (T, N), on_way (T, A) AFTER frame k, agents, times."""
    import departure_restatement as D
    import router_hold_restatement as H
    import test_router_hold_host as RH
    from baseline_restatement import destination_columns
    from oracle import routing, sim
    from tarl_hip.engine import EPISODE_START
    net, pop, T = RH._case("spread")
    N, Nmax = net.num_roads, net.Nmax
    dests = sorted({int(d) for d in pop[:, 1].tolist() if 0 <= d < N})
    seen, before, table = [], [], []

    def head(x, ag, t):
        if t == 0:
            table.append(destination_columns(net.edge_index, routing.edge_travel_time(x, net.edge_index, net.congestion_constant,
                                                                                      Nmax), N, dests))
        seen.append(DC.heads(x.numpy()[None], Nmax)[0])
        before.append(ag[:, sim.ON_WAY].clone().numpy())
        return H.hold_choice(x, ag, table[0], Nmax)

    out = D.replay(net, pop, T, 0, RH._gumbel(net.edge_index.size(1), T), EPISODE_START, route=route, head=head)
    on_way = np.stack(before[1:] + [out["agents"][:, sim.ON_WAY].numpy()])
    times = np.asarray([EPISODE_START + t for t in range(T + 1)], dtype=np.float32)
    return dict(net=net, heads=np.stack(seen), on_way=on_way, agents=out["agents"].numpy(), times=times, T=T, lost=out["lost"],
                dests=dests)


@pytest.mark.parametrize("route", [False, True])
def test_frame_count_equals_the_oracles_frames_on_the_way(route):
    """For every road with a head, at a spread of frames: n of the restatement (from DONE, ARRIVAL_TIME and the clocks alone)
    ``==`` the number of frames k >= t after which the oracle's agent table has that agent ON_WAY. A lost agent pays until
    the horizon, an agent withdrawn by the frame right after it became a head pays nothing."""
    rec = _spread_record(route)
    net, T, ag = rec["net"], rec["T"], rec["agents"]
    N = net.num_roads
    frames = list(range(0, T, 7)) + [T - 1]
    hk = rec["heads"][frames]
    D_ = len(rec["dests"])
    slot = np.full(N, -1, dtype=np.int64)
    slot[rec["dests"]] = np.arange(D_)
    out = DC.decision_advantage(hk, frames, [0] * len(frames), ag[None], rec["times"], T, np.zeros((D_, N)), slot,
                                np.full(N, 4), 1.0, 1.0)
    assert out["bad"] == 0 and int(out["live"].sum()) > 200
    lost_seen = zero_seen = 0
    for j, t in enumerate(frames):
        for u in np.nonzero(out["live"][j])[0]:
            a = int(hk[j, u])
            want = int(rec["on_way"][t:, a].sum())
            assert out["n"][j, u] == want, (t, u, a)
            assert out["adv"][j, u] == -want                                    # gamma 1, zero distances: -n exactly
            lost_seen += int(ag[a, DC.DONE] != 1 and want == T - t)
            zero_seen += int(want == 0)
    assert zero_seen > 0
    if not route:       # 20 agents are lost to the U-turn double pop without the rule; with it nobody is
        assert rec["lost"] == 20
    assert out["truncated"] == sum(int(ag[int(a), DC.DONE] != 1) for a in hk[out["live"]])
    print(f"[decision credit, spread, route={route}] {int(out['live'].sum())} live decisions, {out['truncated']} truncated, "
          f"{zero_seen} withdrawn by the next frame, {lost_seen} of never-arriving agents")


def test_a_lost_agent_pays_until_the_horizon():
    """Without the first-hop rule the spread case loses 20 agents to the U-turn double pop: ON_WAY and in no FIFO. Such an
    agent's last decision as a head gets n = t_end - t, and the oracle agrees."""
    rec = _spread_record(False)
    ag, T = rec["agents"], rec["T"]
    lost = [a for a in range(1, ag.shape[0]) if ag[a, DC.ON_WAY] == 1 and not (rec["heads"][T - 1] == a).any()]
    found = 0
    for a in lost:
        where = np.argwhere(rec["heads"] == a)
        if where.size == 0:
            continue
        t, u = (int(v) for v in where[-1])
        n, trunc = DC.frames_to_go(rec["times"], t, T, float(ag[a, DC.DONE]), float(ag[a, DC.ARRIVAL_TIME]))
        assert trunc and n == T - t == int(rec["on_way"][t:, a].sum())
        found += 1
    assert found >= 5


# ---- 2. the sign case ------------------------------------------------------------------------------------------------------------
def _two_sample_case(T=1.0):
    """Four nodes in a ring with two out-edges each; node 1 heads a traveller in both samples: sample 0 chose its first edge
    and needed 5 frames, sample 1 its second and needed 9. Every other node heads nobody."""
    ei = np.array([[0, 0, 1, 1, 2, 2, 3, 3], [1, 2, 2, 3, 3, 0, 0, 1]])
    N, E = 4, 8
    rng = np.random.default_rng(0)
    logits = rng.normal(size=(2, E))
    choice = np.array([[0, 2, 4, 6], [1, 3, 5, 7]])
    live = np.zeros((2, N), dtype=bool)
    live[:, 1] = True
    adv = np.zeros((2, N), dtype=np.float32)
    adv[0, 1], adv[1, 1] = -5.0, -9.0
    lp_old = DC.node_logprob(ei, N, logits, choice, T)
    return ei, N, logits, choice, live, adv, lp_old


def test_sign_case():
    ei, N, logits, choice, live, adv, lp_old = _two_sample_case()
    st = DC.decision_stats(adv, live)
    assert st.tolist() == [-14.0, 106.0, 2.0]
    r = DC.decision_ppo(ei, N, logits, choice, live, lp_old, adv, st, 2)
    g = r["grad"]
    assert g[0, 2] < 0 and g[1, 3] > 0         # descent raises the logit of the quick turn and lowers that of the slow one
    off = np.ones_like(g, dtype=bool)
    off[:, 2:4] = False
    assert not g[off].any()                    # exactly 0 on every edge of every node without a live decision
    assert r["out4"][:, 1].tolist() == [1.0, 1.0] and abs(r["out4"][:, 3]).max() == 0.0


# ---- 3. the named defects --------------------------------------------------------------------------------------------------------
def _advantage_case():
    """Three rows on a 6-road ring in two environments, clocks 100 .. 110, the segment ends after frame 9: heads that arrived,
    one that never did (ARRIVAL_TIME 0, its initial value), an empty road with a stale id, and two different agent tables."""
    N, A, B = 6, 5, 2
    times = np.arange(100, 111, dtype=np.float32)
    ag = np.zeros((B, A, 9), dtype=np.float32)
    ag[:, :, DC.DESTINATION] = [0, 3, 4, 5, 2]
    ag[0, 1, [DC.ARRIVAL_TIME, DC.DONE]] = [104.0, 1.0]         # withdrawn by frame 4
    ag[0, 2, DC.ON_WAY] = 1.0                                   # never arrived
    ag[0, 3, [DC.ARRIVAL_TIME, DC.DONE]] = [107.0, 1.0]
    ag[1, 1, [DC.ARRIVAL_TIME, DC.DONE]] = [108.0, 1.0]
    ag[1, 2, [DC.ARRIVAL_TIME, DC.DONE]] = [103.0, 1.0]
    ag[1, 3, DC.ON_WAY] = 1.0
    dests = [0, 2, 3, 4, 5]
    slot = np.full(N, -1, dtype=np.int64)
    slot[dests] = np.arange(len(dests))
    dist = np.array([[(d - u) % N * 1.5 for u in range(N)] for d in dests])     # a one-way ring, 1.5 s per road
    head = np.array([[1, 0, 2, 0, 0, 3], [0, 1, 0, 2, 3, 0], [3, 2, 1, 0, 0, 0]])
    frame, env = [1, 2, 6], [0, 1, 0]
    return dict(N=N, times=times, ag=ag, slot=slot, dist=dist, head=head, frame=frame, env=env, t_end=10, deg=np.full(N, 2))


def _adv(c, defect=None, gamma=1.0):
    return DC.decision_advantage(c["head"], c["frame"], c["env"], c["ag"], c["times"], c["t_end"], c["dist"], c["slot"],
                                 c["deg"], 1.0, gamma, defect)


def test_advantage_case_by_hand():
    c = _advantage_case()
    out = _adv(c)
    # row 0 (frame 1, env 0): agent 1 on road 0 arrives at clock 104 -> frames 1, 2, 3 owed; free flow 3 roads * 1.5
    assert out["n"][0].tolist() == [3, -1, 9, -1, -1, 6]
    assert out["adv"][0, 0] == 4.5 - 3 and out["adv"][0, 2] == 3.0 - 9 and out["adv"][0, 5] == 0.0 - 6
    assert out["truncated"] == 3 and out["bad"] == 0          # agent 2 of env 0 twice, agent 3 of env 1 once
    g = _adv(c, gamma=0.9)
    assert abs(g["adv"][0, 0] - ((1 - 0.9 ** 4.5) / 0.1 - (1 - 0.9 ** 3) / 0.1)) < 1e-12


def _loss_case(long_list=False, T=0.7):
    """Three samples on a graph with out-degrees 2 .. 6 (one node without out-edges), ratios below, inside and above the clip
    and advantages of both signs."""
    rng = np.random.default_rng(5)
    degs = [2, 3, 6, 0, 5, 4, 2, 6]
    N = len(degs)
    src = np.concatenate([np.full(d, u) for u, d in enumerate(degs)])
    dst = np.concatenate([rng.permutation(N)[:d] for d in degs])
    ei = np.stack([src, dst])
    E, M = ei.shape[1], 3
    lists = DC.out_lists(ei, N)
    logits = rng.normal(size=(M, E)) * 2.0
    choice = np.array([[(ls[-1] if long_list and len(ls) > 4 else ls[rng.integers(len(ls))]) if len(ls) else -1
                        for ls in lists] for _ in range(M)])
    live = rng.random((M, N)) < 0.7
    live[:, 3] = False
    live[:, 2] = True
    adv = np.where(live, rng.normal(size=(M, N)) * 6.0 - 2.0, 0.0).astype(np.float32)
    lp_old = DC.node_logprob(ei, N, logits, choice, T) + rng.choice([-0.5, -0.05, 0.05, 0.5], size=(M, N))
    return dict(ei=ei, N=N, logits=logits, choice=choice, live=live, adv=adv, lp_old=lp_old, T=T)


def _loss(c, defect=None, dtype=np.float64, stats_defect=None):
    st = DC.decision_stats(c["adv"], c["live"], stats_defect)
    return DC.decision_ppo(c["ei"], c["N"], c["logits"], c["choice"], c["live"], c["lp_old"], c["adv"], st,
                           int(c["live"].sum()), 0.2, c["T"], 0.5, dtype, defect)


def _bound(r32, r64, key, relative):
    return R.tensor_bound(R.max_err(torch.from_numpy(np.asarray(r32[key], dtype=np.float64)), torch.from_numpy(r64[key])),
                          torch.from_numpy(r64[key]), relative_scale=relative)


ADVANTAGE_DEFECTS = ("arrival_frame_owed", "never_arrived_as_arrived", "wrong_env", "dist_transposed")
LOSS_DEFECTS = ("clip_wrong_side", "no_p_factor", "no_temperature", "skip_last_of_long")


@pytest.mark.parametrize("defect", ADVANTAGE_DEFECTS + ("stale_head",))
def test_each_advantage_defect_changes_its_case(defect):
    """The raw advantage is compared on the GPU within ``tensor_bound`` of its fp32 rounding: each defect moves an element
    of the crafted case by whole frames, at least ten times that."""
    c = _advantage_case()
    ref = _adv(c)
    if defect == "stale_head":
        x = np.zeros((1, c["N"], 3 * 4 + 7))
        x[0, :, 0] = [1, 2, 0, 3, 4, 0]
        x[0, :, 3 * 4 + 1] = [1, 0, 0, 2, 0, 0]
        good, bad = DC.heads(x, 4), DC.heads(x, 4, defect)
        assert good.tolist() == [[1, 0, 0, 3, 0, 0]] and bad.tolist() == [[1, 2, 0, 3, 4, 0]]
        c2 = dict(c, head=np.concatenate([bad, bad, bad]), frame=[1, 1, 1], env=[0, 0, 0])
        c1 = dict(c2, head=np.concatenate([good, good, good]))
        ref, got = _adv(c1), _adv(c2)
    else:
        got = _adv(c, defect)
    a64 = torch.from_numpy(ref["adv"])
    bound = R.tensor_bound(R.max_err(a64.float(), a64), a64)
    moved = float(np.abs(got["adv"] - ref["adv"]).max())
    print(f"[decision credit defect {defect}] moved {moved:.3g}, bound {bound:.3g}")
    assert moved >= 10 * bound and moved >= 1.0


def test_statistics_over_all_elements_change_the_normalised_advantage():
    c = _loss_case()
    good, bad = _loss(c), _loss(c, stats_defect="stats_over_all")
    b = _bound(_loss(c, dtype=np.float32), good, "grad", True)
    moved = float(np.abs(good["grad"] - bad["grad"]).max())
    assert DC.decision_stats(c["adv"], c["live"])[2] == c["live"].sum() < c["live"].size
    assert moved >= 10 * b


@pytest.mark.parametrize("defect", LOSS_DEFECTS)
def test_each_loss_defect_changes_its_case(defect):
    """Gradient (``relative_scale``) and loss parts against ten times the bound of the GPU comparison, e32 from the fp32 run
    of the restatement. The factor p / (p + 1e-8) differs from 1 by 1e-8 / p: its case is a chosen edge of probability
    below 1e-6, where dropping it is visible."""
    c = _loss_case(long_list=defect == "skip_last_of_long")
    if defect == "no_p_factor":         # a node whose chosen edge is all but excluded: p ~ 1e-9
        c["logits"][:, DC.out_lists(c["ei"], c["N"])[2]] = 0.0
        c["logits"][np.arange(3), c["choice"][:, 2]] = -14.5
        c["lp_old"] = DC.node_logprob(c["ei"], c["N"], c["logits"], c["choice"], c["T"])
    good, bad, r32 = _loss(c), _loss(c, defect), _loss(c, dtype=np.float32)
    b_g = _bound(r32, good, "grad", True)
    b_o = _bound(r32, good, "out4", False)
    moved_g = float(np.abs(good["grad"] - bad["grad"]).max())
    moved_o = float(np.abs(good["out4"] - bad["out4"]).max())
    print(f"[decision credit defect {defect}] grad moved {moved_g:.3g} (bound {b_g:.3g}), out4 moved {moved_o:.3g} "
          f"(bound {b_o:.3g})")
    assert moved_g >= 10 * b_g
    if defect in ("clip_wrong_side", "skip_last_of_long"):
        assert moved_o >= 10 * b_o


def test_every_defect_is_covered_and_unknown_ones_are_refused():
    assert set(ADVANTAGE_DEFECTS) | set(LOSS_DEFECTS) | {"stale_head", "stats_over_all"} == set(DC.DEFECTS)
    with pytest.raises(ValueError, match="unknown defect"):
        DC.heads(np.zeros((1, 2, 19)), 4, "other")


def test_fp32_restatement_is_within_its_own_rule():
    c = _loss_case()
    r64, r32 = _loss(c), _loss(c, dtype=np.float32)
    assert np.abs(r32["grad"] - r64["grad"]).max() < 1e-5 and (r32["out4"][:, 1:3] == r64["out4"][:, 1:3]).all()


# ---- 4. the host side --------------------------------------------------------------------------------------------------------------
NEW = ("tarl_fused_head_rows", "tarl_fused_set_head_capture", "tarl_decision_advantage", "tarl_decision_stats",
       "tarl_graphdist_node_logprob", "tarl_graphdist_decision_ppo_scratch_bytes", "tarl_graphdist_decision_ppo")


def _fake_fused(lib):
    f = lib.FusedStruct()
    for name, typ in lib.FusedStruct._fields_:
        if typ is ctypes.c_void_p and name != "policy_held":
            setattr(f, name, 0x1000)                                        # never dereferenced: validation fails first
    f.ld_slots, f.acc_slots = 48, 1
    return f


def test_entry_points_are_bound_and_nothing_moved():
    from tarl_hip import lib
    L = lib.load()
    assert all(n in lib.SIGNATURES and hasattr(L, n) for n in NEW)
    assert L.tarl_abi_version() == 5
    assert lib.FusedStruct._fields_[-1][0] == "policy_held"                  # tarl_fused did not grow


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    pp = ctypes.byref(_plan(100, 400))
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    # plan, f, B, env, slot, n, head_keep, stream
    entry, ok = L.tarl_fused_head_rows, [pp, fp, 2, fake, fake, 3, fake, null]
    for i in (0, 1, 3, 4, 6):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad in ((2, 0), (2, 1 << 31), (5, -1), (5, 1 << 24)):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1, (i, bad)
    assert entry(pp, fp, 2, null, null, 0, null, null) == 0                  # nothing to do: no launch, no pointer needed
    # plan, head_keep, frame, env, slot, rows, B, agents, A, a_bstride, times, num_times, t_end, dist, dest_slot, D, timestep,
    # gamma, adv_raw, truncated, bad, stream
    entry = L.tarl_decision_advantage
    ok = [pp, fake, fake, fake, fake, 3, 2, fake, 5, 45, fake, 11, 10, fake, fake, 4, 1.0, 1.0, fake, fake, fake, null]
    for i in (0, 1, 2, 3, 4, 7, 10, 13, 14, 18, 19, 20):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((5, -1, b"bad sizes"), (6, 0, b"bad sizes"), (8, 0, b"bad sizes"), (8, (1 << 24) + 1, b"bad sizes"),
                        (9, 44, b"a_bstride"), (12, 0, b"t_end"), (12, 12, b"t_end"), (15, 0, b"bad sizes"),
                        (16, 0.0, b"timestep"), (16, float("inf"), b"timestep"), (17, 0.0, b"decision_gamma"),
                        (17, 1.5, b"decision_gamma"), (5, 1 << 24, b"too many")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    # adv_raw, head_keep, elems, partial, stats3, stream
    assert L.tarl_decision_stats(fake, fake, 0, fake, fake, null) == -1
    for i in (0, 1, 3, 4):
        args = [fake, fake, 8, fake, fake, null]
        args[i] = null
        assert L.tarl_decision_stats(*args) == -1, i
    # plan, logits, M, temperature, choice, lp_node, stream
    entry, ok = L.tarl_graphdist_node_logprob, [pp, fake, 2, 1.0, fake, fake, null]
    for i in (0, 1, 4, 5):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    assert entry(pp, fake, 0, 1.0, fake, fake, null) == -1 and entry(pp, fake, 2, 0.0, fake, fake, null) == -1
    assert entry(pp, fake, 1 << 24, 1.0, fake, fake, null) == -1 and b"too many" in L.tarl_last_error()
    # plan, logits, M, temperature, choice, head, lp_old, adv_raw, stats3, n_live, clip, grad_scale, out4, grad, scratch, stream
    entry = L.tarl_graphdist_decision_ppo
    ok = [pp, fake, 2, 1.0, fake, fake, fake, fake, fake, fake, 0.2, 1.0, fake, fake, fake, null]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 12, 14):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((2, 0, b"M must"), (3, 0.0, b"temperature"), (10, 1.0, b"clip_epsilon"), (10, -0.1, b"clip_epsilon"),
                        (14, ctypes.c_void_p(0x1004), b"aligned"), (2, 1 << 24, b"too many")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    assert L.tarl_graphdist_decision_ppo_scratch_bytes(null, 2) == -1
    assert L.tarl_graphdist_decision_ppo_scratch_bytes(pp, 0) == -1
    assert L.tarl_graphdist_decision_ppo_scratch_bytes(pp, 3) == 3 * 1 * 32      # one tile of 256 nodes, 32 bytes each
    assert L.tarl_graphdist_decision_ppo_scratch_bytes(ctypes.byref(_plan(257, 400)), 3) == 3 * 2 * 32


def test_the_four_switches_share_one_word_in_every_combination():
    """policy hold (1), departure router (2), trip reward (4), head capture (8): every setter changes its own bit alone,
    from every one of the sixteen states, and a refused call changes nothing."""
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    cap = L.tarl_fused_set_head_capture
    assert cap(null, 1, fake) == -1 and b"null" in L.tarl_last_error()
    assert cap(fp, 2, fake) == -1 and cap(fp, -1, fake) == -1
    assert cap(fp, 1, null) == -1 and b"go together" in L.tarl_last_error()
    assert cap(fp, 0, fake) == -1 and b"go together" in L.tarl_last_error()
    assert f.policy_hold == 0
    setters = {1: lambda on: L.tarl_fused_set_policy_hold(fp, on, null),
               2: lambda on: (L.tarl_fused_set_departure_router(fp, 1, fake, fake, 0, 3, fake, null) if on else
                              L.tarl_fused_set_departure_router(fp, 0, null, null, 0, 0, null, null)),
               4: lambda on: L.tarl_fused_set_trip_reward(fp, on, null),
               8: lambda on: cap(fp, on, fake if on else null)}
    for state in range(16):
        for bit, setter in setters.items():
            for b in (1, 2, 4, 8):                      # reach `state` from whatever the word holds
                assert setters[b](1 if state & b else 0) == 0
            assert f.policy_hold == state
            for on in (1, 0, 1 if state & bit else 0):
                assert setter(on) == 0
                assert f.policy_hold == (state & ~bit) | (bit if on else 0), (state, bit, on)
    for b in (1, 2, 4, 8):
        assert setters[b](0) == 0
    assert f.policy_hold == 0 and lib.FusedStruct().policy_hold == 0            # off by default
    from tarl_hip import ops
    assert ops.HEAD_CAPTURE == 8


class _P:
    num_nodes, num_edges, handle = 4, 8, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)


def test_the_ops_refuse_host_tensors_and_bad_arguments():
    from tarl_hip import lib, ops
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_head_rows(_P(), _FS(), i32(2), i32(2), i32(2, 4))
    with pytest.raises(ValueError, match="needs its head_keep"):
        ops.fused_set_head_capture(_FS(), True)
    with pytest.raises(ValueError, match="without the switch"):
        ops.fused_set_head_capture(_FS(), False, i32(2, 4))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.decision_stats(torch.zeros(2, 4), i32(2, 4))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.graphdist_node_logprob(_P(), torch.zeros(2, 8), i32(2, 4))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.decision_advantage(_P(), i32(2, 4), i32(2), i32(2), i32(2), torch.zeros(2, 3, 9), torch.zeros(5), 4,
                               torch.zeros(2, 4, dtype=torch.float64), i32(4), B=2, timestep=1, adv_raw=torch.zeros(2, 4),
                               truncated=i32(1), bad=i32(1))


# ---- 5. argument rules -----------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="goal_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules():
    assert _args().credit == "joint" and _args().credit_gamma is None
    for head in ("edge_mlp", "embedding_dijkstra", "graph_transformer", "goal_mlp"):
        assert _args(credit="decision", policy_head=head).credit == "decision"
    assert _args(credit="decision", algo="mpnn").credit == "decision"
    assert _args(credit="decision", credit_gamma=0.99).credit_gamma == 0.99
    # independent of the other switches, and combined with each of them
    assert _args(credit="decision", reward="trip", policy_hold=True, route_departures=True, pretrain_bc=2).credit == "decision"
    with pytest.raises(ValueError, match="state-dependent head"):
        _args(credit="decision", policy_head="embedding")
    with pytest.raises(ValueError, match="graph_transformer"):
        _args(credit="decision", value_head="graph_transformer", policy_head="graph_transformer")
    with pytest.raises(ValueError, match="mode 'train'"):
        _args(credit="decision", mode="eval", algo="mpnn", eval_envs=2)
    with pytest.raises(ValueError, match="algo mpnn"):
        _args(credit="decision", algo="dijkstra")
    with pytest.raises(ValueError, match="needs credit decision"):
        _args(credit_gamma=0.9)
    for g in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="credit_gamma must be"):
            _args(credit="decision", credit_gamma=g)
    with pytest.raises(ValueError, match="credit must be"):
        _args(credit="other")


def test_parser_flags():
    import importlib
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.credit == "joint" and ns.credit_gamma is None
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit",
                                         "decision", "--credit-gamma", "0.95"])
    assert ns.credit == "decision" and RunnerArgs(**vars(ns)).credit_gamma == 0.95
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--credit", "decision"])
    with pytest.raises(ValueError, match="credit decision"):
        RunnerArgs(**vars(ns))
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--credit-gamma", "0.9"])
    with pytest.raises(ValueError, match="credit_gamma"):
        RunnerArgs(**vars(ns))
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--credit", "other"])


def test_the_layers_take_the_arguments():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.trainer import VecPPOTrainer
    for fn in (ppo_train, VecPPOTrainer.__init__):
        p = inspect.signature(fn).parameters
        assert p["credit"].default == "joint" and p["decision_gamma"].default == 1.0


def test_trainer_refusals_without_a_device():
    """The three refusals of credit="decision", in the wording of policy_hold's; they come before anything touches a GPU."""
    from tarl_hip import lib
    from tarl_hip.trainer import VecPPOTrainer

    class _Eng:
        fs, B, N, device = None, 2, 4, "cpu"

    t = VecPPOTrainer.__new__(VecPPOTrainer)
    t.state_dep, t.decision_gamma = False, 1.0
    with pytest.raises(ValueError, match="not available for policy='embedding'"):
        t._check_decision_credit(_Eng(), "simple")
    t.state_dep = True
    with pytest.raises(lib.TarlError, match="needs the fused engine"):
        t._check_decision_credit(_Eng(), "simple")
    _Eng.fs = object()
    with pytest.raises(ValueError, match="value='graph_transformer'"):
        t._check_decision_credit(_Eng(), "graph_transformer")
    t.decision_gamma = 0.0
    with pytest.raises(ValueError, match="decision_gamma"):
        t._check_decision_credit(_Eng(), "simple")
