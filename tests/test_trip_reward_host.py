"""CPU: the trip reward — the rule written out (``trip_reward_restatement``) on crafted agent tables, an agent
kept waiting by a full road, an agent lost to the U-turn double pop, the identities owed = queued + lost + ready on the oracle
with and without the first-hop rule, THE CASE THE FEATURE EXISTS FOR (one traveller, lost in one run and delivered in the other:
the queue return prefers the lost run, the trip return the delivered one), what each of six defects would do instead, and the
host side: the new C-ABI entry points (bound, validated before any HIP call, ABI number unchanged, the handle's struct
unchanged), the three switches sharing one word, the ops' argument rules, the parser and argument rules, and the reports of
a run without the new arguments pinned to a snapshot recorded before the feature existed."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import trip_reward_restatement as R
from conftest import ROOT
from fake_plan import fake_plan as _plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trip_reward_off_snapshot.json")


def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


# ---- 1. the rule on crafted tables ---------------------------------------------------------------------------------------------
def test_crafted_cases():
    c = R.crafted()
    ag, t, ids = c["agents"][0].numpy(), c["t"], c["ids"]
    on, ready = R.parts(ag, t)
    # on the way: the two flagged agents, whatever their departure says; done agents owe nothing
    assert on == 2 and ag[ids["on_way_late_dep"], R.DEP] > t
    # ready: agent 0, the one that departs exactly at t and the two that are due; not the one a float later, not the late one
    assert ready == 4
    assert ag[ids["just_after_t"], R.DEP] > t and float(ag[ids["just_after_t"], R.DEP]) - t < 1e-4
    assert R.reward_batch(c["agents"].numpy(), t).tolist() == [-6.0]
    assert R.reward_batch(c["agents"].numpy(), t).dtype == np.float32
    # one float later the next agent is due too; long before, nobody is
    later = float(np.nextafter(np.float32(t), np.float32(np.inf)))
    assert R.parts(ag, later) == (2, 5) and R.parts(ag, t - 1000.0) == (2, 0)
    # leaving one agent out at a time changes exactly what it contributes
    for name, (d_on, d_ready) in {"agent0": (0, 1), "exactly_t": (0, 1), "just_after_t": (0, 0), "not_due": (0, 0),
                                  "on_way": (1, 0), "on_way_late_dep": (1, 0), "done": (0, 0), "due_a": (0, 1)}.items():
        rest = np.delete(ag, ids[name], axis=0)
        assert R.parts(rest, t) == (on - d_on, ready - d_ready), name
    # environments that differ
    b = R.crafted(K=4)
    assert R.parts_batch(b["agents"].numpy(), t).tolist() == [[2, 4], [3, 3], [2, 2], [3, 3]]
    # the status bytes are the pack's
    assert R.status_bytes(ag).tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 0, 0]


def test_an_agent_kept_waiting_by_a_full_road_stays_ready():
    """The road its origin row selects has no room (MAX - 3 - count <= 0): the insert leaves the agent where it is and it
    costs one ready traveller in every frame — under the queue reward it costs nothing — until there is room."""
    from oracle import sim
    net = _torus8()
    Nmax = net.Nmax
    cols = sim.Cols(Nmax)
    x, _ = R.empty_state(net)
    u, target = 3, int(net.edge_index[1][net.edge_index[0] == 3][0])
    ag = torch.zeros((2, 9))
    ag[0, R.DEP] = 1e9
    ag[1, R.ORIGIN], ag[1, R.DEST], ag[1, R.DEP] = float(u), 40.0, 100.0
    x[:, cols.SEL] = torch.arange(net.num_roads, dtype=x.dtype)
    x[u, cols.SEL] = float(target)
    x[target, cols.N] = x[target, cols.MAXN] - sim.CONGESTION_FILE
    assert R.parts(ag.numpy(), 99.0) == (0, 0)
    for k in range(3):
        sim.insert(x, ag, 100.0 + k, Nmax, net.congestion_constant)
        assert ag[1, R.ON_WAY] == 0 and R.parts(ag.numpy(), 100.0 + k) == (0, 1)
    x[target, cols.N] -= 1
    sim.insert(x, ag, 103.0, Nmax, net.congestion_constant)
    assert ag[1, R.ON_WAY] == 1 and R.parts(ag.numpy(), 103.0) == (1, 0)


# ---- 2. the case the feature exists for ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_agent():
    """One traveller on the 8 x 8 torus, 120 frames, the torch noise of test_router_hold_host: lost to the U-turn double pop
    under a fixed selection, delivered by the free-flow hold router."""
    import test_router_hold_host as RH
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    c = R.one_agent_case(net, EPISODE_START)
    T = 120
    g = RH._gumbel(net.edge_index.size(1), T)
    lost = R.replay(net, c["pop"], T, g, EPISODE_START, R.fixed_selection(c["lost_sel"], net.Nmax))
    delivered = R.replay(net, c["pop"], T, g, EPISODE_START, R.hold_router(net, c["pop"], False))
    return c, T, lost, delivered


def test_an_agent_lost_to_the_u_turn_double_pop_keeps_costing(one_agent):
    """Inserted onto its origin's neighbour, the traveller turns back into its empty origin road and both roads are popped:
    from that frame on it is on the way and queued nowhere. ``on_way`` stays 1 while ``queued`` drops to 0."""
    c, T, lost, _ = one_agent
    assert lost["arrivals"] == 0
    departed = lost["on_way"].index(1)
    vanished = next(t for t in range(departed, T) if lost["queued"][t] == 0)
    assert 2 <= departed < vanished <= departed + 20          # a few frames after departure
    assert all(q == 1 for q in lost["queued"][departed:vanished]) and all(q == 0 for q in lost["queued"][vanished:])
    assert all(o == 1 for o in lost["on_way"][departed:]) and all(r == 0 for r in lost["ready"])
    assert lost["lost"][vanished:] == [1] * (T - vanished) and lost["lost"][:vanished] == [0] * vanished
    assert lost["trip"][vanished:] == [-1.0] * (T - vanished) and lost["queue"][vanished:] == [0.0] * (T - vanished)


def test_the_queue_return_prefers_the_lost_run_and_the_trip_return_the_delivered_one(one_agent):
    """THE CASE THE FEATURE EXISTS FOR. The horizon is at least twice the delivered trip's length. The lost agent stops
    costing queue reward when it vanishes and costs trip reward until the horizon; the delivered one stops paying on arrival."""
    c, T, lost, delivered = one_agent
    assert delivered["arrivals"] == 1 and lost["arrivals"] == 0
    departed = delivered["on_way"].index(1)
    arrived = next(t for t in range(departed, T) if delivered["on_way"][t] == 0)
    assert T >= 2 * (arrived - departed)
    q_lost, q_del = sum(lost["queue"]), sum(delivered["queue"])
    t_lost, t_del = sum(lost["trip"]), sum(delivered["trip"])
    print(f"[trip reward, one agent] queue return lost {q_lost:.0f} / delivered {q_del:.0f}; trip return lost {t_lost:.0f} / "
          f"delivered {t_del:.0f}; trip of {arrived - departed} frames, horizon {T}")
    assert q_lost > q_del              # the reference's reward pays for losing the traveller
    assert t_del > t_lost              # the trip reward does not
    assert t_del == q_del              # nobody lost, nobody kept waiting: the two rewards agree
    assert t_lost == -float(T - lost["on_way"].index(1))


# ---- 3. the identities on the oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread_runs():
    """The "spread" case of test_router_hold_host (seed 7, 300 frames, its torch noise) under the free-flow hold router,
    without and with the first-hop rule of DESIGN 4.23 -> {route: (net, pop, T, noise, replay)}."""
    import test_router_hold_host as RH
    from tarl_hip.engine import EPISODE_START
    net, pop, T = RH._case("spread")
    g = RH._gumbel(net.edge_index.size(1), T)
    return {route: (net, pop, T, g, R.replay(net, pop, T, g, EPISODE_START, R.hold_router(net, pop, route)))
            for route in (False, True)}


@pytest.mark.parametrize("route,lost_want,arrivals_want", [(False, 20, 99), (True, 0, 128)])
def test_owed_is_queued_plus_lost_plus_ready_in_every_frame(spread_runs, route, lost_want, arrivals_want):
    """owed == queued + lost + ready and queued == -(queue reward) in every frame; the agents lost are those
    tests/test_departures_host.py asserts, 20 without the rule and 0 with it; the replay is departure_restatement's."""
    import departure_restatement as D
    from tarl_hip.engine import EPISODE_START
    net, pop, T, g, run = spread_runs[route]
    for t in range(T):
        owed = -run["trip"][t]
        assert owed == run["on_way"][t] + run["ready"][t]
        assert run["queued"][t] == -run["queue"][t]
        assert run["lost"][t] == run["on_way"][t] - run["queued"][t] >= 0
        assert owed == run["queued"][t] + run["lost"][t] + run["ready"][t]
    assert run["lost"][-1] == lost_want == D.lost(run["x"], run["agents"], net.Nmax)
    assert int(run["agents"][1:, 8].sum()) == arrivals_want
    assert -run["trip"][-1] == 128 - arrivals_want                 # what is still owed after the last frame
    want = D.replay(net, pop, T, 0, g, EPISODE_START, route=route)
    assert run["queue"] == want["reward"] and torch.equal(run["agents"], want["agents"])


def test_the_trip_return_rises_with_the_first_hop_rule(spread_runs):
    """29 more arrivals and no agent lost: the trip return is the higher with the rule. (On this case the queue return rises
    too; at config 4 it falls)"""
    (q0, t0), (q1, t1) = ((sum(spread_runs[k][4]["queue"]), sum(spread_runs[k][4]["trip"])) for k in (False, True))
    print(f"[trip reward, free_flow on the torus] without / with the first-hop rule: queue return {q0:.0f} / {q1:.0f}, "
          f"trip return {t0:.0f} / {t1:.0f}")
    assert round(q0) == -7863 and round(q1) == -5539              # the figures of DESIGN 4.23
    assert t1 > t0 and t0 < q0 and t1 <= q1                       # lost and waiting travellers cost on top of the queues


# ---- 4. one defect at a time ---------------------------------------------------------------------------------------------------
def test_each_rule_defect_changes_its_case():
    c = R.crafted(K=4)
    ag, t, ids = c["agents"].numpy(), c["t"], c["ids"]
    want = R.parts_batch(ag, t)
    # "<" loses the agent that departs exactly at t (environments 0 and 2, where it still waits)
    got = R.parts_batch(ag, t, "strict_less")
    assert (want - got).tolist() == [[0, 1], [0, 0], [0, 1], [0, 0]]
    # done agents counted: the two done agents everywhere, the two more of environment 2
    got = R.parts_batch(ag, t, "done_counted")
    assert (got - want).tolist() == [[2, 0], [2, 0], [4, 0], [2, 0]]
    # agent 0 skipped: one ready traveller fewer everywhere
    got = R.parts_batch(ag, t, "agent0_skipped")
    assert (want - got).tolist() == [[0, 1]] * 4 and ids["agent0"] == 0
    # the wrong environment's row: environment 0 reads environment 1's statuses
    got = R.parts_batch(ag, t, "wrong_row")
    assert got[0].tolist() == [3, 3] != want[0].tolist() and not np.array_equal(got, want)
    with pytest.raises(ValueError, match="defect"):
        R.parts_batch(ag, t, "other")


def test_the_byte_pass_and_its_two_defects():
    """The status pass as the kernel makes it, on bytes: rows of A = 17 bytes start at 0, 17, 34, ...: every row but the first
    has head bytes, every row has a tail or head. Dropping either changes the count; the pass itself equals the plain count
    for every A of the device test and every alignment of the array."""
    rng = np.random.default_rng(5)
    for A in (1, 15, 16, 17, 63, 64, 65, 128, 129, 8207, 8208, 8209):
        K = 5 if A < 1000 else 3
        st = rng.integers(0, 3, size=(K, A)).astype(np.uint8)
        for base in (0, 1, 9, 15):
            on, shape = R.byte_pass(st, base)
            assert on.tolist() == (st == 1).sum(axis=1).tolist(), (A, base)
            assert all(h <= 15 and tl <= 15 and h + 16 * g + tl == A for g, h, tl in shape)
    st = np.ones((4, 17), np.uint8)
    on, shape = R.byte_pass(st)
    assert on.tolist() == [17] * 4 and shape == [(1, 0, 1), (0, 15, 2), (0, 14, 3), (0, 13, 4)]
    assert R.byte_pass(st, defect="head_dropped")[0].tolist() == [17, 2, 3, 4]
    assert R.byte_pass(st, defect="tail_dropped")[0].tolist() == [16, 15, 14, 13]
    st = np.ones((2, 40), np.uint8)                     # the last partial 16-byte group of row 0: bytes 32..39; row 1 starts
    assert R.byte_pass(st, defect="tail_dropped")[0].tolist() == [32, 40]       # at byte 40 and ends on a boundary: no tail
    assert R.byte_pass(st, defect="head_dropped")[0].tolist() == [40, 32]       # but 8 head bytes
    assert set(R.DEFECTS) == {"strict_less", "done_counted", "agent0_skipped", "wrong_row", "head_dropped", "tail_dropped"}


# ---- 5. the host side ----------------------------------------------------------------------------------------------------------
NEW = ("tarl_fused_trip_reward", "tarl_fused_set_trip_reward")


def test_entry_points_are_bound_and_nothing_moved():
    from tarl_hip import lib, ops
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    for n in NEW:
        assert n in lib.SIGNATURES and getattr(L, n) is not None and n + "(" in header
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert "#define TARL_TRIP_REWARD 4" in header and "#define TARL_DEPARTURE_ROUTER 2" in header
    assert [f[0] for f in lib.FusedStruct._fields_][-3:] == ["policy_hold", "bufs_dev", "policy_held"]      # the handle did not grow
    kernel = open(os.path.join(ROOT, "tarl-simulator_amd", "csrc", "trip_reward.hip")).read()
    assert kernel.count("__global__") == 3 and "asm" not in kernel and "uint4" in kernel and "__shared__" in kernel
    assert "atomicAdd(acc" in kernel and "float atomic" not in kernel
    assert list(inspect.signature(ops.fused_trip_reward).parameters) == ["plan", "fs", "t", "out", "parts"]
    assert list(inspect.signature(ops.fused_set_trip_reward).parameters) == ["fs", "on", "parts"]


def _fake_fused(lib):
    f = lib.FusedStruct()
    for name, typ in lib.FusedStruct._fields_:
        if typ is ctypes.c_void_p and name != "policy_held":
            setattr(f, name, 0x1000)                                        # never dereferenced: validation fails first
    f.ld_slots, f.acc_slots = 48, 1
    return f


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    pp = ctypes.byref(_plan(100, 400))
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    t = ctypes.c_float(5.0)
    # plan, f, B, Nmax, num_agents, t, reward, parts, stream
    entry, ok = L.tarl_fused_trip_reward, [pp, fp, 2, 15, 4, t, fake, null, null]
    for i in (0, 1, 6):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((2, 0, b"bad sizes"), (3, 128, b"Nmax"), (2, 1 << 31, b"bad sizes"), (4, 0, b"bad sizes"),
                        (4, (1 << 24) + 1, b"bad sizes"), (5, ctypes.c_float(float("inf")), b"non-finite"),
                        (5, ctypes.c_float(float("-inf")), b"non-finite"), (5, ctypes.c_float(float("nan")), b"non-finite")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    empty = lib.FusedStruct()
    assert entry(pp, ctypes.byref(empty), 2, 15, 4, t, fake, null, null) == -1 and b"buffers missing" in L.tarl_last_error()
    # the switch: f, on, parts
    setter = L.tarl_fused_set_trip_reward
    assert setter(null, 1, null) == -1 and b"null" in L.tarl_last_error()
    assert setter(fp, 2, null) == -1 and setter(fp, -1, null) == -1
    assert setter(fp, 0, fake) == -1 and b"without the switch" in L.tarl_last_error()
    assert f.policy_hold == 0                                               # a refused call changes nothing
    assert lib.FusedStruct().policy_hold == 0                               # off by default


def test_the_three_switches_share_one_word_and_leave_each_other_alone():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    hold = lambda on: L.tarl_fused_set_policy_hold(fp, on, null)                                        # noqa: E731
    router = lambda on: (L.tarl_fused_set_departure_router(fp, 1, fake, fake, 0, 3, fake, null) if on   # noqa: E731
                         else L.tarl_fused_set_departure_router(fp, 0, null, null, 0, 0, null, null))
    trip = lambda on, parts=null: L.tarl_fused_set_trip_reward(fp, on, parts)                           # noqa: E731
    setters = {1: hold, 2: router, 4: trip}
    assert trip(1, fake) == 0 and f.policy_hold == 4 and trip(0) == 0 and f.policy_hold == 0
    for mask in range(8):                   # every combination of the other two: setting and clearing one leaves them
        for bit, setter in setters.items():
            for b2, s2 in setters.items():
                assert s2(1 if mask & b2 and b2 != bit else 0) == 0
            others = mask & ~bit
            assert f.policy_hold == others
            assert setter(1) == 0 and f.policy_hold == others | bit
            assert setter(1) == 0 and f.policy_hold == others | bit
            assert setter(0) == 0 and f.policy_hold == others
    for s in setters.values():
        assert s(0) == 0
    assert f.policy_hold == 0 and not f.policy_held


class _P:
    num_nodes, num_edges, handle = 4, 4, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)


def test_the_ops_refuse_host_tensors_and_bad_arguments():
    from tarl_hip import lib, ops
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_trip_reward(_P(), _FS(), 5.0)
    with pytest.raises(ValueError, match="without the switch"):
        ops.fused_set_trip_reward(_FS(), False, torch.zeros((3, 2, 2), dtype=torch.int32))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_set_trip_reward(_FS(), True, torch.zeros((3, 2, 2), dtype=torch.int32))


def test_evaluator_and_trainer_rules_without_a_device():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.evaluator import EvalResult, VecEvaluator
    from tarl_hip.replanning import Replanner
    from tarl_hip.trainer import VecPPOTrainer
    assert inspect.signature(VecEvaluator.__init__).parameters["trip_reward"].default is False
    assert inspect.signature(Replanner.__init__).parameters["trip_reward"].default is False
    assert inspect.signature(VecPPOTrainer.__init__).parameters["reward"].default == "queue"
    assert inspect.signature(ppo_train).parameters["reward"].default == "queue"
    res = EvalResult(envs=1, head="embedding", deterministic=True, frames_run=0)
    assert res.trip_return is None and res.trip_parts_last is None


# ---- 6. argument rules ---------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="edge_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules():
    assert _args().reward == "queue"
    for head in ("edge_mlp", "embedding_dijkstra", "graph_transformer", "goal_mlp"):
        assert _args(reward="trip", policy_head=head).reward == "trip"
    assert _args(reward="trip", policy_head="goal_mlp", pretrain_bc=2, policy_hold=True, route_departures=True).reward == "trip"
    with pytest.raises(ValueError, match="reward trip cannot train policy_head 'embedding'"):
        _args(reward="trip", policy_head="embedding")
    assert _args(reward="queue", policy_head="embedding").reward == "queue"
    with pytest.raises(ValueError, match="'queue' or 'trip'"):
        _args(reward="other")
    ev = dict(mode="eval", algo="mpnn", policy_head="embedding")
    with pytest.raises(ValueError, match="eval_envs > 0, dijkstra_envs > 0 or replan_days > 0"):
        _args(reward="trip", **ev)
    assert _args(reward="trip", eval_envs=2, **ev).reward == "trip"
    assert _args(reward="trip", eval_envs=2, eval_baseline="free_flow", **ev).reward == "trip"
    dj = dict(mode="eval", algo="dijkstra")
    assert _args(reward="trip", dijkstra_envs=2, **dj).reward == "trip"       # every router, the reference-order one too
    assert _args(reward="trip", replan_days=2, **dj).reward == "trip"
    with pytest.raises(ValueError, match="replan_days > 0"):
        _args(reward="trip", **dj)
    with pytest.raises(ValueError, match="algo mpnn or mpnn\\+ppo"):
        _args(reward="trip", algo="dijkstra", mode="train")


def test_parser_flag():
    import importlib
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    assert main.build_parser().parse_args([]).reward == "queue"
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "4", "--reward", "trip"])
    assert ns.reward == "trip" and RunnerArgs(**vars(ns)).reward == "trip"
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--reward", "trip"])
    with pytest.raises(ValueError, match="reward trip"):
        RunnerArgs(**vars(ns))
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "embedding", "--reward", "trip"])
    with pytest.raises(ValueError, match="reward trip"):
        RunnerArgs(**vars(ns))
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--reward", "other"])


# ---- 7. without the new arguments nothing changes --------------------------------------------------------------------------------
def _seeded_result(K, seed, head):
    """An EvalResult as a run WITHOUT trip_reward leaves it, from seeded per-environment numbers."""
    from tarl_hip.evaluator import EvalResult, summarise
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 30, size=(K, 3))
    counts[-1, 0] = 0                                   # an environment without an arrival
    sums = np.stack([counts[:, 0] * rng.uniform(40, 90, K), counts[:, 0] * rng.uniform(2000, 9000, K),
                     rng.uniform(90, 300, K)], axis=1)
    hist = rng.integers(0, 4, size=(K, 720))
    hist[-1] = 0
    ret = -rng.integers(100, 9000, K).astype(np.float64)
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=100,
                     settings=dict(seed=3, env_base=0, bin_width=10.0, num_bins=720))
    per, res.aggregate, res.envs_without_arrival = summarise(counts, sums, ret, hist, 100, 10.0)
    for k, v in per.items():
        setattr(res, k, v)
    return res


def _seeded_replan(K):
    from tarl_hip.eval_reports import _sample_moments
    from tarl_hip.replanning import DAY_KEYS, ReplanResult
    rng = np.random.default_rng(11)
    days = []
    for day in range(3):
        per = dict(arrived=[int(v) for v in rng.integers(50, 128, K)], avg_travel_time=[float(v) for v in rng.uniform(40, 60, K)],
                   relative_gap=[float(v) for v in rng.uniform(0, 0.2, K)], episode_return=[-float(v) for v in rng.integers(1, 9, K)])
        rec = dict(day=day, domain_exit=False, sim_ms=1.5, switch_probability=0.1, differs=7, agents=K * 127, without_route=0,
                   overflowing=0, switched=3 if day < 2 else None, plan_ms=2.5, per_env=per)
        for key in DAY_KEYS:
            v = np.asarray(per[key], dtype=np.float64)
            rec[key] = dict(n=int(v.size), **_sample_moments(v))
        days.append(rec)
    return ReplanResult(days=days, last=None, settings=dict(days=3, envs=K, plans=K, fraction=0.1, max_hops=24, frames=100,
                                                           link_bin_seconds=3600))


def build_snapshot():
    """Everything a run without the new arguments reports, as JSON-ready values."""
    from tarl_hip.evaluator import paired_lines, paired_report, paired_scalars
    from tarl_hip.replanning import replan_lines, replan_report
    a, b = _seeded_result(4, 1, "goal_mlp"), _seeded_result(4, 2, "dijkstra_hold")
    rep = paired_report(a, b)
    rr = replan_report(_seeded_replan(3))
    return dict(to_dict=a.to_dict(per_env=True), rows=a.rows(), summary_lines=a.summary_lines(), paired=rep,
                paired_lines=paired_lines(rep), paired_scalars=paired_scalars(rep), replan=rr, replan_lines=replan_lines(rr))


def test_reports_without_the_new_arguments_are_the_recorded_ones():
    """tests/golden/trip_reward_off_snapshot.json was recorded by :func:`build_snapshot` from the code as it was before the trip
    reward existed: compared as JSON text, which keeps every float64 bit and the order of the keys (the CSV columns)."""
    want = open(GOLDEN).read()
    assert json.dumps(build_snapshot(), indent=1) + "\n" == want


def test_reports_with_trip_return_gain_exactly_their_keys():
    from tarl_hip.evaluator import aggregate, paired_report
    from tarl_hip.replanning import REPLAN_COLUMNS, replan_lines, replan_report
    a, b = _seeded_result(4, 1, "goal_mlp"), _seeded_result(4, 2, "dijkstra_hold")
    off = dict(to_dict=a.to_dict(per_env=True), rows=a.rows(), lines=a.summary_lines(), paired=paired_report(a, b))
    a.trip_return = [-10.0, -20.0, -30.0, -45.0]
    a.aggregate["trip_return"] = aggregate(a.trip_return)
    assert paired_report(a, b) == off["paired"]                   # only one run has it: no row
    b.trip_return = [-11.0, -19.0, -33.0, -40.0]
    b.aggregate["trip_return"] = aggregate(b.trip_return)
    on = a.to_dict(per_env=True)
    assert set(on["per_env"]) - set(off["to_dict"]["per_env"]) == {"trip_return"}
    assert set(on["aggregate"]) - {"trip_return"} == set(off["to_dict"]["aggregate"]) - {"trip_return"}
    assert [set(r) - set(o) for r, o in zip(a.rows(), off["rows"])] == [{"trip_return"}] * 4
    assert a.summary_lines()[:-1] == off["lines"] and a.summary_lines()[-1].startswith("trip_return:")
    rep = paired_report(a, b)
    assert list(rep["metrics"])[:-1] == list(off["paired"]["metrics"]) and list(rep["metrics"])[-1] == "trip_return"
    m = rep["metrics"]["trip_return"]
    assert m["n"] == 4 and m["mean"] == pytest.approx(np.mean([1.0, -1.0, 3.0, -5.0]))
    assert {k: v for k, v in rep["metrics"].items() if k != "trip_return"} == off["paired"]["metrics"]
    # the replanning days
    rp = _seeded_replan(3)
    off_rep = replan_report(rp)
    for r in rp.days:
        r["trip_return"] = dict(n=3, mean=-100.0 - r["day"], std=1.0, se=0.5)
    on_rep = replan_report(rp)
    assert on_rep["columns"] == list(REPLAN_COLUMNS) + ["trip_return_mean", "trip_return_se"] and off_rep["columns"] == list(REPLAN_COLUMNS)
    assert [r["trip_return_mean"] for r in on_rep["rows"]] == [-100.0, -101.0, -102.0]
    lines = replan_lines(on_rep)
    assert len(lines) == len(replan_lines(off_rep)) + 1 and lines[-2].startswith("trip return per day:")
