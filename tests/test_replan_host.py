"""CPU: the day-to-day replanning without a device — the restatement's routes are paths that reproduce ``best``
bit for bit and equal the enumeration of paths on the small cases; every defect of ``replan_restatement.DEFECTS`` changes a
route, a selection or a day of the loop on a named case (the cases bite); the three entry points are bound and refuse bad
arguments before any HIP call; the pinned names are unchanged; the CLI and the evaluator's head rules."""
import os
import re

import numpy as np
import pytest
import torch

import dynamic_gap_restatement as G
import replan_restatement as R
from conftest import ROOT

CASES = {c["name"]: c for c in R.route_cases()}
MAX_HOPS = 8


# ---- 1. the routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_are_paths_that_reproduce_best(name):
    c = CASES[name]
    N, K, bs, fb, ag = c["N"], c["K"], c["bin_seconds"], c["first_bin"], c["agents"]
    tau, env, best, rt, ln = R.run_routes(c, MAX_HOPS)
    outs = G.out_lists(c["edges"], N)
    planned = routed = 0
    for k in range(K):
        for a in range(ag.shape[1]):
            od = R.planned(ag[k, a], a, N)
            if od is None:
                assert ln[k, a] == 0 and best[k, a] == G.INF
                continue
            planned += 1
            o, d = od
            t0 = float(ag[k, a, G.DEP])
            assert best[k, a] == G.hindsight_one(outs, tau[k], env[k], o, d, t0, bs, fb)         # the imported search
            if N <= 6:
                vals = [v for v, _, _ in G.brute_paths(outs, tau[k], env[k], o, d, t0, bs, fb)]
                assert best[k, a] == (min(vals) if vals else G.INF)
            if not best[k, a] < G.INF:
                assert ln[k, a] == 0
                continue
            routed += 1
            n = int(ln[k, a])
            assert 1 <= n <= N and (n == 1) == (o == d)
            path = rt[k, a, :n].tolist()
            assert R.is_path(outs, path, o, d) and len(set(path)) == n and (rt[k, a, n:] == -1).all()
            assert G.along(path, tau[k], env[k], t0, bs, fb) == best[k, a]                      # bit for bit
    assert planned > 0 and routed > 0


def test_a_route_longer_than_max_hops_has_a_negative_length():
    c = CASES["tie"]
    _, _, best, rt, ln = R.run_routes(c, 4)
    _, _, best3, rt3, ln3 = R.run_routes(c, 3)
    assert ln[0, 1] == 4 and rt[0, 1].tolist() == [0, 1, 4, 5]
    assert ln3[0, 1] == -4 and (rt3[0, 1] == -1).all() and best3[0, 1] == best[0, 1]
    assert ln3[0, 2] == 3 and rt3[0, 2].tolist() == [0, 1, 4]


def test_the_tie_goes_to_the_smallest_road_id_whatever_the_list_order():
    c = CASES["tie"]
    assert R.in_lists(c["edges"], c["N"])[4] == [3, 6, 1, 2]
    _, _, _, rt, ln = R.run_routes(c)
    assert rt[0, 1, :4].tolist() == [0, 1, 4, 5] and ln[0].tolist() == [0, 4, 3, 3, 1, 0, 0]


# ---- 2. the defects bite ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,case", [("largest_id_tie", "tie"), ("first_in_list_tie", "tie"),
                                         ("stops_after_four_in_edges", "late-tie")])
def test_walk_defects_change_a_route(defect, case):
    c = CASES[case]
    _, _, best, rt, ln = R.run_routes(c)
    _, _, dbest, drt, dln = R.run_routes(c, defect=defect)
    assert np.array_equal(best, dbest)                          # the labels are not the walk's
    assert not (np.array_equal(rt, drt) and np.array_equal(ln, dln)), defect
    if case == "late-tie":
        assert ln[0, 1] == 3 and rt[0, 1, :3].tolist() == [0, 5, 7] and dln[0, 1] == 0


def test_the_select_rule_by_hand_and_its_defects():
    s = R.select_case()
    written, value = R.select_rule(s["x"], s["routes"], s["route_len"])
    assert {i: value[i] for i in range(s["N"]) if written[i]} == s["want"]
    changed = {}
    for defect in ("no_hold", "holds_two_short", "first_match_from_the_end"):
        w, v = R.select_rule(s["x"], s["routes"], s["route_len"], defect=defect)
        assert np.array_equal(w, written)
        changed[defect] = [i for i in range(s["N"]) if v[i] != value[i]]
    assert changed == {"no_hold": [2], "holds_two_short": [1], "first_match_from_the_end": [0]}
    # a head id out of range and a length beyond the row leave the row untouched
    x = s["x"].copy()
    x[0, 0], x[1, 0] = 99.0, -1.0
    ln = s["route_len"].copy()
    ln[3] = 7
    w, _ = R.select_rule(x, s["routes"], ln)
    assert w.tolist() == [False, False, False, True, False, False]


def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _gumbel(E, K, frames):
    g = torch.Generator().manual_seed(1)
    vals = [[-torch.log(-torch.log(torch.rand(E, generator=g).clamp_min(1e-12))) for _ in range(frames)] for _ in range(K)]
    return lambda b, t: vals[b][t]


def _loop(defect=None, days=3, K=2, T=60):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    return R.day_loop(net, pop, K, T, days, 0.5, 16, 20, 0, _gumbel(net.edge_index.size(1), K, T), EPISODE_START, defect=defect)


@pytest.fixture(scope="module")
def loop():
    return _loop()


def test_the_day_loop_on_the_oracle(loop):
    """8 x 8 torus, 128 agents, 60 frames, K = 2, three days, fraction 0.5, bins of 20 s (torch's noise): day 0 follows the
    free-flow routes in both environments; later days differ between the environments and from day 0; only masked agents
    change their route; the last day draws no mask."""
    d0, d1, d2 = loop
    assert np.array_equal(d0["routes"][0], d0["routes"][1]) and (d0["route_len"][:, 1:] > 0).all()
    assert d0["mask"].shape == (2, 129) and d2["mask"] is None
    for a, b in ((d0, d1), (d1, d2)):
        moved = (a["route_len"] != b["route_len"]) | (a["routes"] != b["routes"]).any(-1)
        assert moved.any() and not (moved & ~a["mask"]).any() and np.array_equal(moved, a["mask"] & a["differs"])
    assert not np.array_equal(d2["routes"][0], d2["routes"][1])
    print("[replan host] arrivals", [d["arrived"] for d in loop], "travel time", [d["travel_time"] for d in loop], "RG",
          [d["rg"] for d in loop], "differs", [int(d["differs"][:, 1:].sum()) for d in loop])
    assert all(min(d["arrived"]) > 0 for d in loop)


@pytest.mark.parametrize("defect", ["shared_plan_for_every_env", "swap_mask_ignored"])
def test_loop_defects_change_a_day(loop, defect):
    bad = _loop(defect)
    assert np.array_equal(bad[0]["agents"], loop[0]["agents"])          # day 0: one plan, no mask yet
    assert any(not np.array_equal(b["agents"], g["agents"]) for b, g in zip(bad[1:], loop[1:])), defect


# ---- 3. ABI, names, CLI ------------------------------------------------------------------------------------------------------------
NEW = ("tarl_td_routes_scratch_bytes", "tarl_td_routes", "tarl_fused_select_route")


def test_entry_points_are_bound_and_the_abi_number_stays():
    from tarl_hip import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    for n in NEW:
        assert n in lib.SIGNATURES and getattr(L, n) is not None and n + "(" in header
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert "NOT reference semantics" in header[header.index("day-to-day replanning"):]


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null = None
    assert L.tarl_td_routes_scratch_bytes(null, 1, 1, 8) == -1
    assert L.tarl_td_routes(null, null, null, null, 1, 1, 9, 60, 0, 1, 8, null, 0, null, null, null, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_fused_select_route(null, null, 1, 15, 1, null, null, 0, 8, null, null) == -1
    assert b"null" in L.tarl_last_error()
    # what is refused before the plan is looked at, with a stand-in for it that is never dereferenced
    buf = torch.zeros(64, dtype=torch.float64)
    p = buf.data_ptr()
    for K, A, hops in ((0, 5, 8), (2, 0, 8), (2, 5, 0), (2, 5, (1 << 20) + 1), (1 << 31, 5, 8)):
        assert L.tarl_td_routes_scratch_bytes(p, K, A, hops) == -1
    for hops in (0, (1 << 20) + 1):
        assert L.tarl_td_routes(p, p, p, p, 1, 2, 18, 60, 0, 1, hops, p, 1 << 20, p, p, p, null) == -1
        assert b"max_hops" in L.tarl_last_error()
    assert L.tarl_td_routes(p, p, p, p, 0, 2, 18, 60, 0, 1, 8, p, 1 << 20, p, p, p, null) == -1 and b"sizes" in L.tarl_last_error()
    assert L.tarl_td_routes(p, p, p, p, 1, 2, 17, 60, 0, 1, 8, p, 1 << 20, p, p, p, null) == -1 and b"overlap" in L.tarl_last_error()
    assert L.tarl_td_routes(p, p, p, p, 1, 2, 18, 0, 0, 1, 8, p, 1 << 20, p, p, p, null) == -1 and b"bin_seconds" in L.tarl_last_error()
    assert L.tarl_td_routes(p, p, p, p, 1, 2, 18, 60, 0, 0, 8, p, 1 << 20, p, p, p, null) == -1 and b"H must" in L.tarl_last_error()


def test_ops_refuse_host_tensors_and_bad_shapes():
    from tarl_hip import lib, ops

    class _P:
        handle, num_nodes, num_edges = None, 3, 2
    plan = _P()
    tau, env, ag = torch.zeros((1, 1, 3)), torch.zeros((1, 2, 3), dtype=torch.float64), torch.zeros((1, 2, 9))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.td_routes(plan, tau, env, ag, bin_seconds=60, first_bin=0, max_hops=4)
    with pytest.raises(ValueError, match="max_hops"):
        ops.td_routes(plan, tau, env, ag, bin_seconds=60, first_bin=0, max_hops=0)

    class _FS:
        hdp = torch.zeros((3, 1, 2), dtype=torch.int32)
        B, A, Nmax = 1, 2, 15
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_select_route(plan, _FS(), torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def test_the_names_are_as_pinned():
    from src import runner
    from tarl_hip import evaluator as E
    assert "routes" in E.HEADS and E.PLAN_HEADS == ("routes",)
    assert E.ROUTER_HEADS == ("dijkstra", "dijkstra_hold")
    assert E.EVAL_BASELINES == {"dijkstra": ("dijkstra", {}), "dijkstra_hold": ("dijkstra_hold", {}),
                                "free_flow": ("dijkstra_hold", {"refresh_rate": 0})}
    assert E.DIJKSTRA_ROUTERS == {"reference": ("dijkstra", None), "hold": ("dijkstra_hold", None),
                                  "free_flow": ("dijkstra_hold", 0)}
    assert runner.EVAL_BASELINE_NAMES == ("none", "dijkstra", "dijkstra_hold", "free_flow")
    assert runner.DIJKSTRA_ROUTER_NAMES == ("reference", "hold", "free_flow")


def test_the_parser_takes_the_flags():
    import importlib
    main = importlib.import_module("main")
    p = main.build_parser()
    ns = p.parse_args([])
    assert (ns.replan_days, ns.replan_envs, ns.replan_fraction, ns.replan_max_hops) == (0, 1, 0.1, None)
    ns = p.parse_args(["--replan-days", "3", "--replan-envs", "2", "--replan-fraction", "msa", "--replan-max-hops", "40"])
    assert (ns.replan_days, ns.replan_envs, ns.replan_fraction, ns.replan_max_hops) == (3, 2, "msa", 40)
    assert p.parse_args(["--replan-fraction", "0.25"]).replan_fraction == 0.25
    assert p.parse_args(["--replan-fraction", "1"]).replan_fraction == 1.0
    for bad in ("0", "1.5", "-0.1", "often"):
        with pytest.raises(SystemExit):
            p.parse_args(["--replan-fraction", bad])


def test_runner_args_refuse_what_the_loop_cannot_do():
    from src.runner import RunnerArgs
    RunnerArgs(algo="dijkstra", scenario="synthetic-64-16", mode="eval", replan_days=2, replan_envs=2)
    RunnerArgs(algo="mpnn", scenario="synthetic-64-16", mode="eval", replan_days=1, replan_fraction="msa")
    for kw, msg in ((dict(replan_days=-1), "replan_days"), (dict(replan_days=1, mode="train", algo="mpnn+ppo"), "eval"),
                    (dict(replan_envs=0), "replan_envs"), (dict(replan_fraction=0.0), "replan_fraction"),
                    (dict(replan_fraction=1.5), "replan_fraction"), (dict(replan_max_hops=0), "replan_max_hops")):
        args = dict(algo="dijkstra", scenario="synthetic-64-16", mode="eval")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            RunnerArgs(**args)


def test_evaluator_head_rules_without_a_device():
    from tarl_hip.evaluator import VecEvaluator

    class _Fused:
        fs = object()
    with pytest.raises(ValueError, match="routes"):
        VecEvaluator(_Fused(), "routes")
    with pytest.raises(ValueError, match="routes"):             # a plan handed to a head that does not read it
        VecEvaluator(_Fused(), "dijkstra_hold", routes=(None, None))
    ev = object.__new__(VecEvaluator)
    ev.head, ev.eng = "routes", _Fused()
    with pytest.raises(ValueError, match="sampled"):
        ev.run(8, deterministic=False)
    ev.head = "dijkstra_hold"
    with pytest.raises(ValueError, match="set_routes"):
        ev.set_routes(None, None)


def test_replanner_pieces_without_a_device():
    from tarl_hip import replanning as P
    assert P.day_seed(0, 0) == R.day_seed(0, 0) and P.day_seed(5, 7) == R.day_seed(5, 7) != P.day_seed(5, 8)
    assert P.switch_probability("msa", 0) == 0.5 and P.switch_probability("msa", 2) == 0.25 and P.switch_probability(0.3, 9) == 0.3
    assert P.parse_fraction("msa") == "msa" and P.parse_fraction("0.5") == 0.5 and P.parse_fraction(1) == 1.0
    for bad in (0, 1.5, "0"):
        with pytest.raises(ValueError):
            P.parse_fraction(bad)
