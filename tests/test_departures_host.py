"""CPU: first-hop routing — the rule written out (``departure_restatement``) on a hand-made ring and on the
crafted cases of the 8 x 8 torus and both irregular graphs, what each of eight defects would do instead, an agent kept
waiting by a full road, the figures of the design note replayed on the oracle, and the host side: the new C-ABI entry points
(bound, validated before any HIP call, ABI number unchanged, the handle's struct unchanged), the ops' argument rules and the
evaluator's refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import departure_restatement as D
from conftest import ROOT
from fake_plan import fake_plan as _plan

GRAPHS = ["torus", "MIXED", "HUB126"]


def _net(name):
    import sp_cases as S
    from tarl_hip import synth
    return synth.torus_network(8, 8) if name == "torus" else S.case(name).net


@pytest.fixture(scope="module")
def crafted():
    return {name: (_net(name), D.crafted(_net(name))) for name in GRAPHS}


def _table_rule(net, c, defect=None):
    return D.route_table(c["x"].numpy(), c["agents"].numpy(), c["table"].numpy(), c["t"], net.Nmax,
                         slot_of=c["slot_of"].numpy(), defect=defect)


# ---- 1. the rule on a ring ---------------------------------------------------------------------------------------------------
def test_the_rule_on_a_three_road_ring():
    """0 -> 1 -> 2 -> 0, every road empty but road 2. Agent 1 leaves road 0 for road 2 (next hop 1), agent 2 leaves road 1 for
    road 2 (next hop IS the destination: road 1 selects itself), agent 3 would leave road 2, where agent 4 stands."""
    Nmax = 2
    col_n, col_sel = 3 * Nmax + 1, 3 * Nmax + 5
    x = torch.zeros((3, 3 * Nmax + 7))
    x[:, col_sel] = -9.0
    x[2, 0], x[2, col_n] = 4.0, 1.0
    ag = torch.zeros((5, 9))
    ag[0, D.DEP] = 1e9
    ag[1:, D.ORIGIN] = torch.tensor([0.0, 1.0, 2.0, 0.0])
    ag[1:, D.DEST] = torch.tensor([2.0, 2.0, 1.0, 1.0])
    ag[1:, D.DEP] = torch.tensor([5.0, 5.0, 5.0, 1.0])
    ag[4, D.ON_WAY] = 1.0
    table = torch.tensor([[0, 1, 1], [2, 1, 2], [0, 0, 2]])      # [row][destination]
    assert D.pending(ag.numpy(), 5.0, 3).tolist() == [1, 2, 3]
    assert D.pending(ag.numpy(), 4.0, 3).tolist() == [-1, -1, -1]
    w, v = D.route_table(x.numpy(), ag.numpy(), table.numpy(), 5.0, Nmax)
    assert w.tolist() == [True, True, False] and v.tolist() == [1.0, 1.0, 0.0]
    assert D.apply(x, w, v, Nmax) == 2
    assert x[:, col_sel].tolist() == [1.0, 1.0, -9.0]
    assert D.lost(x, ag, Nmax) == 0


# ---- 2. the crafted cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_crafted_cases(crafted, name):
    net, c = crafted[name]
    N, r, ids, outs, ag = net.num_roads, c["rows"], c["ids"], c["outs"], c["agents"]
    pend = D.pending(ag.numpy(), c["t"], N)
    w, v = _table_rule(net, c)
    dest = lambda a: int(ag[ids[a], D.DEST])                                    # noqa: E731
    nh = lambda row, a: int(c["table"][r[row], dest(a)])                         # noqa: E731
    # the smaller id speaks for both, although the larger one departs earlier
    assert ag[ids["two_large"], D.DEP] < ag[ids["two_small"], D.DEP] and ids["two_small"] < ids["two_large"]
    assert pend[r["two_agents"]] == ids["two_small"] and v[r["two_agents"]] == nh("two_agents", "two_small")
    assert nh("two_agents", "two_small") != nh("two_agents", "two_large")
    # a non-empty row keeps its head's choice
    assert pend[r["nonempty"]] == ids["nonempty"] and not w[r["nonempty"]]
    # <= t, to the float
    assert pend[r["exactly_t"]] == ids["exactly_t"] and w[r["exactly_t"]]
    assert pend[r["just_after_t"]] == -1 and not w[r["just_after_t"]]
    assert ag[ids["just_after_t"], D.DEP] > c["t"] and float(ag[ids["just_after_t"], D.DEP]) - c["t"] < 1e-4
    # on-the-way and done agents are not ready
    assert pend[r["on_way_and_done"]] == ids["after_them"] > ids["done"] > ids["on_way"]
    assert v[r["on_way_and_done"]] == nh("on_way_and_done", "after_them") != r["on_way_and_done"]
    # no slot, no path: untouched
    assert pend[r["no_slot"]] == ids["no_slot"] and not w[r["no_slot"]] and c["slot_of"][dest("no_slot")] < 0
    assert pend[r["unreachable"]] == ids["unreachable"] and not w[r["unreachable"]] and nh("unreachable", "unreachable") == -1
    # the hold rule, and the destination row itself
    assert nh("next_is_dest", "next_is_dest") == dest("next_is_dest") and v[r["next_is_dest"]] == r["next_is_dest"]
    assert dest("origin_is_dest") == r["origin_is_dest"] and w[r["origin_is_dest"]] and v[r["origin_is_dest"]] == r["origin_is_dest"]
    # late ranks
    u = r["rank_ge_4"]
    assert v[u] == outs[u][-1] and (name == "torus" or len(outs[u]) > 4)
    u = r["last_rank"]
    assert v[u] == outs[u][-1] and len(outs[u]) == max(len(o) for o in outs) and (name != "HUB126" or len(outs[u]) == 126)
    # a DIRTY empty row is empty
    assert c["x"][r["dirty_empty"], 0] != 0 and w[r["dirty_empty"]]
    # nobody else is touched
    assert int(w.sum()) == len(r) - 4 and set(np.nonzero(w)[0].tolist()) <= set(r.values())
    # the plan lookup
    rt, ln, want = D.crafted_plan(c)
    pw, pv = D.route_plan(c["x"].numpy(), ag.numpy(), rt, ln, c["t"], net.Nmax)
    for row, val in want.items():
        assert (not pw[r[row]]) if val is None else (pw[r[row]] and pv[r[row]] == val), row
    assert rt[ids["exactly_t"], 0] != r["exactly_t"] and ln[ids["origin_is_dest"]] == 1 and ln[ids["next_is_dest"]] == 2


def test_an_agent_kept_waiting_by_a_full_road_is_routed_in_every_frame(crafted):
    """The road the waiting agent is sent to has no room (MAX - 3 - count <= 0): the insert leaves the agent where it is, it
    stays ready, and the rule writes its origin road again in every frame until there is room."""
    from oracle import sim
    net, c = crafted["torus"]
    Nmax, N = net.Nmax, net.num_roads
    cols = sim.Cols(Nmax)
    x, ag = c["x"].clone(), c["agents"].clone()
    u, a = c["rows"]["waiting"], c["ids"]["waiting"]
    target = int(c["table"][u, int(ag[a, D.DEST])])
    x[target, cols.N] = x[target, cols.MAXN] - sim.CONGESTION_FILE
    for k in range(3):
        t = c["t"] + k
        x[:, cols.SEL] = -7.0
        w, v = D.route_table(x.numpy(), ag.numpy(), c["table"].numpy(), t, Nmax, slot_of=c["slot_of"].numpy())
        assert w[u] and v[u] == target and D.pending(ag.numpy(), t, N)[u] == a
        D.apply(x, w, v, Nmax)
        keep = x[:, cols.SEL].clone()
        x[:, cols.SEL] = torch.where(torch.from_numpy(w), keep, torch.arange(N, dtype=x.dtype))      # the others stay at home
        sim.insert(x, ag, t, Nmax, net.congestion_constant)
        assert ag[a, D.ON_WAY] == 0
    x[target, cols.N] -= 1
    x[:, cols.SEL] = torch.arange(N, dtype=x.dtype)
    w, v = D.route_table(x.numpy(), ag.numpy(), c["table"].numpy(), c["t"] + 3, Nmax, slot_of=c["slot_of"].numpy())
    D.apply(x, w, v, Nmax)
    sim.insert(x, ag, c["t"] + 3, Nmax, net.congestion_constant)
    assert ag[a, D.ON_WAY] == 1


# ---- 3. one defect at a time ------------------------------------------------------------------------------------------------------
CHANGES = {"first_in_departure_order": "two_agents", "nonempty_rows_routed": "nonempty", "status_ignored": "on_way_and_done",
           "strict_less": "exactly_t", "no_hold": "next_is_dest", "table_transposed": "last_rank",
           "minus_one_written": "unreachable"}


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("defect", sorted(CHANGES))
def test_each_defect_changes_its_case(crafted, name, defect):
    net, c = crafted[name]
    w, v = _table_rule(net, c)
    bw, bv = _table_rule(net, c, defect)
    u = c["rows"][CHANGES[defect]]
    assert (bw[u], bv[u]) != (w[u], v[u]), (defect, CHANGES[defect])
    if defect != "table_transposed":        # and nothing but its own case (the transposed table is wrong nearly everywhere)
        others = [r for k, r in c["rows"].items() if k != CHANGES[defect]]
        assert all((bw[r], bv[r]) == (w[r], v[r]) for r in others)
    if defect == "minus_one_written":
        assert bv[u] == -1.0


@pytest.mark.parametrize("name", GRAPHS)
def test_the_plan_lookup_without_its_hold(crafted, name):
    net, c = crafted[name]
    rt, ln, _ = D.crafted_plan(c)
    args = (c["x"].numpy(), c["agents"].numpy(), rt, ln, c["t"], net.Nmax)
    w, v = D.route_plan(*args)
    bw, bv = D.route_plan(*args, defect="plan_no_hold")
    u = c["rows"]["next_is_dest"]
    assert v[u] == u and bv[u] == c["outs"][u][0]
    assert np.array_equal(np.delete(v, u), np.delete(bv, u)) and np.array_equal(w, bw)


def test_unknown_defect_is_refused(crafted):
    net, c = crafted["torus"]
    with pytest.raises(ValueError, match="defect"):
        _table_rule(net, c, "other")
    assert set(CHANGES) | {"plan_no_hold"} == set(D.DEFECTS)


# ---- 4. the figures of the design note ------------------------------------------------------------------------------------------------
def _spread_replay(refresh_rate, route):
    import test_router_hold_host as RH
    from tarl_hip.engine import EPISODE_START
    net, pop, T = RH._case("spread")
    return D.replay(net, pop, T, refresh_rate, RH._gumbel(net.edge_index.size(1), T), EPISODE_START, route=route)


def test_the_free_flow_router_delivers_everybody_with_the_rule():
    """The "spread" case of test_router_hold_host (seed 7, 300 frames, its torch noise), free-flow hold router: 99 arrivals
    and 20 agents lost without the rule, 128 and 0 with it."""
    import router_hold_restatement as H
    import test_router_hold_host as RH
    off, on = _spread_replay(0, False), _spread_replay(0, True)
    print(f"[departures] free_flow: arrivals {off['arrivals']} -> {on['arrivals']}, ON_WAY - queued {off['lost']} -> {on['lost']}, "
          f"return {sum(off['reward']):.0f} -> {sum(on['reward']):.0f}, rows routed {on['routed']} ({on['changed']} changed)")
    assert off["arrivals"] == 99 and on["arrivals"] == 128
    assert off["lost"] == 20 and on["lost"] == 0
    assert round(sum(off["reward"])) == -7863 and round(sum(on["reward"])) == -5539
    assert 104 <= on["routed"] <= 111 and 65 <= on["changed"] <= 74
    # without the rule the replay IS the hold router's
    ref = RH._replay("spread", hold=True, refresh_rate=0)
    assert off["reward"] == ref["reward"] and torch.equal(off["x"], ref["x"]) and torch.equal(off["agents"], ref["agents"])
    assert torch.equal(off["sel"], ref["sel"]) and H.DEFECTS


def test_the_refreshing_router_with_the_rule():
    """``dijkstra_hold`` (refresh 10) on the same case: 105 arrivals and 18 lost without, 125 and 3 with the rule."""
    off, on = _spread_replay(10, False), _spread_replay(10, True)
    assert (off["arrivals"], off["lost"], round(sum(off["reward"]))) == (105, 18, -6770)
    assert (on["arrivals"], on["lost"], round(sum(on["reward"]))) == (125, 3, -5318)


# ---- 5. the host side ----------------------------------------------------------------------------------------------------------------
NEW = ("tarl_fused_pending_departures", "tarl_fused_route_departures", "tarl_fused_route_departures_plan",
       "tarl_fused_set_departure_router")


def test_entry_points_are_bound_and_nothing_moved():
    from tarl_hip import lib, ops
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    for n in NEW:
        assert n in lib.SIGNATURES and getattr(L, n) is not None and n + "(" in header
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert "src/agents/base.py:247-331" in header
    assert [f[0] for f in lib.FusedStruct._fields_][-3:] == ["policy_hold", "bufs_dev", "policy_held"]      # the handle did not grow
    assert lib.SIGNATURES[NEW[1]] == lib.SIGNATURES[NEW[2]]
    kernel = open(os.path.join(ROOT, "tarl-simulator_amd", "csrc", "departures.hip")).read()
    assert "template <class Lookup>" in kernel and kernel.count("__global__") == 3       # one route kernel, two scans
    assert "asm" not in kernel
    for name in ("fused_pending_departures", "fused_route_departures", "fused_route_departures_plan",
                 "fused_set_departure_router"):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(ops.fused_pending_departures).parameters) == ["plan", "fs", "t", "out"]
    assert list(inspect.signature(ops.fused_route_departures).parameters) == ["plan", "fs", "pend", "dest_slot", "table",
                                                                              "choice8", "routed"]
    assert list(inspect.signature(ops.fused_route_departures_plan).parameters) == ["plan", "fs", "pend", "routes", "route_len",
                                                                                   "choice8", "routed"]


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
    # plan, f, B, Nmax, num_agents, t, pend, stream
    entry, ok = L.tarl_fused_pending_departures, [pp, fp, 2, 15, 4, t, fake, null]
    for i in (0, 1, 6):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((2, 0, b"bad sizes"), (3, 128, b"Nmax"), (2, 1 << 31, b"bad sizes"), (4, 0, b"bad sizes"),
                        (4, (1 << 24) + 1, b"bad sizes"), (5, ctypes.c_float(float("inf")), b"non-finite"),
                        (5, ctypes.c_float(float("nan")), b"non-finite")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    empty = lib.FusedStruct()
    assert entry(pp, ctypes.byref(empty), 2, 15, 4, t, fake, null) == -1 and b"buffers missing" in L.tarl_last_error()
    # plan, f, B, Nmax, num_agents, pend, dest_slot, next_hop, nh_bstride, num_dests, choice8, routed, stream
    entry, ok = L.tarl_fused_route_departures, [pp, fp, 2, 15, 4, fake, fake, fake, 0, 3, null, null, null]
    for i in (0, 1, 5, 6, 7):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((2, 0, b"bad sizes"), (3, 128, b"Nmax"), (4, 0, b"bad sizes"), (9, 0, b"num_dests"), (9, -1, b"num_dests"),
                        (8, 299, b"overlap"), (8, -1, b"overlap")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    # plan, f, B, Nmax, num_agents, pend, routes, route_len, r_bstride, max_hops, choice8, routed, stream
    entry, ok = L.tarl_fused_route_departures_plan, [pp, fp, 2, 15, 4, fake, fake, fake, 0, 8, null, null, null]
    for i in (0, 1, 5, 6, 7):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((9, 0, b"max_hops"), (9, (1 << 20) + 1, b"max_hops"), (8, 31, b"overlap"), (4, 0, b"bad sizes")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    # the switch: f, on, dest_slot, next_hop, nh_bstride, num_dests, pend, routed
    setter = L.tarl_fused_set_departure_router
    assert setter(null, 1, fake, fake, 0, 3, fake, null) == -1 and b"null" in L.tarl_last_error()
    assert setter(fp, 2, fake, fake, 0, 3, fake, null) == -1 and setter(fp, -1, fake, fake, 0, 3, fake, null) == -1
    for i in (2, 3, 6):
        args = [fp, 1, fake, fake, 0, 3, fake, null]
        args[i] = null
        assert setter(*args) == -1 and b"without a table" in L.tarl_last_error(), i
    assert setter(fp, 1, fake, fake, 0, 0, fake, null) == -1 and b"num_dests" in L.tarl_last_error()
    assert setter(fp, 0, null, null, 0, 0, null, fake) == -1 and b"without the switch" in L.tarl_last_error()
    assert setter(fp, 0, fake, fake, 0, 3, fake, null) == -1 and b"without the switch" in L.tarl_last_error()
    assert f.policy_hold == 0                                               # a refused call changes nothing
    # the two switches share a word and leave each other's bit alone
    hold = L.tarl_fused_set_policy_hold
    assert setter(fp, 1, fake, fake, 0, 3, fake, fake) == 0 and f.policy_hold == 2
    assert hold(fp, 1, null) == 0 and f.policy_hold == 3
    assert setter(fp, 0, null, null, 0, 0, null, null) == 0 and f.policy_hold == 1
    assert setter(fp, 1, fake, fake, 0, 3, fake, null) == 0 and hold(fp, 0, null) == 0 and f.policy_hold == 2
    assert setter(fp, 0, null, null, 0, 0, null, null) == 0 and f.policy_hold == 0 and not f.policy_held
    assert lib.FusedStruct().policy_hold == 0                               # off by default


class _P:
    num_nodes, num_edges, handle = 4, 4, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)
    sel8 = torch.zeros((4, 2), dtype=torch.uint8)


def test_the_ops_refuse_host_tensors_and_bad_arguments():
    from tarl_hip import lib, ops
    pend = torch.zeros((4, 2), dtype=torch.int32)
    slot = torch.zeros(4, dtype=torch.int32)
    table = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_pending_departures(_P(), _FS(), 5.0)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_route_departures(_P(), _FS(), pend, slot, table)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_route_departures_plan(_P(), _FS(), pend, torch.zeros((3, 5), dtype=torch.int32),
                                        torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="without the switch"):
        ops.fused_set_departure_router(_FS(), False, slot, table)
    with pytest.raises(ValueError, match="needs"):
        ops.fused_set_departure_router(_FS(), True, slot, table)


def test_evaluator_rules_without_a_device():
    from tarl_hip.evaluator import EvalResult, VecEvaluator

    class _Fused:
        fs = object()
    assert inspect.signature(VecEvaluator.__init__).parameters["route_departures"].default is False
    with pytest.raises(ValueError, match="dijkstra_hold"):
        VecEvaluator(_Fused(), "dijkstra", route_departures=True)
    assert EvalResult(envs=1, head="embedding", deterministic=True, frames_run=0).departures_routed is None


# ---- 6. argument rules ------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="edge_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules():
    assert _args().route_departures is False
    # train: the state-dependent heads; behaviour cloning next to it is accepted
    for head in ("edge_mlp", "embedding_dijkstra", "graph_transformer", "goal_mlp"):
        assert _args(route_departures=True, policy_head=head).route_departures
    assert _args(route_departures=True, pretrain_bc=1).pretrain_bc == 1
    assert _args(route_departures=True, policy_hold=True, eval_envs=2, eval_baseline="free_flow").route_departures
    with pytest.raises(ValueError, match="state-dependent head"):
        _args(route_departures=True, policy_head="embedding")
    # eval: one of the three vectorised forms
    ev = dict(mode="eval", algo="mpnn", policy_head="embedding")
    with pytest.raises(ValueError, match="eval_envs > 0, dijkstra_envs > 0"):
        _args(route_departures=True, **ev)
    assert _args(route_departures=True, eval_envs=2, **ev).route_departures
    for name in ("dijkstra_hold", "free_flow"):
        assert _args(route_departures=True, eval_envs=2, eval_baseline=name, **ev).route_departures
    with pytest.raises(ValueError, match="dijkstra_hold or free_flow"):
        _args(route_departures=True, eval_envs=2, eval_baseline="dijkstra", **ev)
    dj = dict(mode="eval", algo="dijkstra")
    for name in ("hold", "free_flow"):
        assert _args(route_departures=True, dijkstra_envs=2, dijkstra_router=name, **dj).route_departures
    with pytest.raises(ValueError, match="hold or free_flow"):
        _args(route_departures=True, dijkstra_envs=2, **dj)
    assert _args(route_departures=True, replan_days=2, **dj).route_departures
    with pytest.raises(ValueError, match="replan_days > 0"):
        _args(route_departures=True, **dj)


def test_parser_flag():
    import importlib
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    assert main.build_parser().parse_args([]).route_departures is False
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "4", "--route-departures"])
    assert ns.route_departures is True and RunnerArgs(**vars(ns)).route_departures
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--route-departures"])
    with pytest.raises(ValueError, match="route_departures"):
        RunnerArgs(**vars(ns))


def test_the_layers_take_the_flag():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.replanning import Replanner
    from tarl_hip.trainer import VecPPOTrainer
    for fn in (ppo_train, Replanner.__init__, VecPPOTrainer.__init__):
        assert inspect.signature(fn).parameters["route_departures"].default is False
