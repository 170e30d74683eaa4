"""CPU: the per-agent path trace. First the two facts about the simulator that the trace rests on, checked on the
oracle in every frame of the 8 x 8 torus "spread" case under three choosers and of 120 frames on both irregular graphs; then
the rule written out (``path_trace_restatement``) on crafted cases, what each of six defects would do instead, and the host
side: the new C-ABI entry points (bound, validated before any HIP call, ABI number unchanged) and the refusals of the ops,
the evaluator and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import path_trace_restatement as P
from conftest import ROOT


# ---- 1. the two facts, on the oracle --------------------------------------------------------------------------------------------
def _snapshot(x, Nmax):
    """-> (road_of {agent: road} over every FIFO slot in use, head id per road, count per road)."""
    x = x.numpy()
    n = x[:, 3 * Nmax + 1].astype(np.int64)
    ids = x[:, :Nmax].astype(np.int64)
    road_of = {}
    for u in np.nonzero(n)[0]:
        for a in ids[u, :n[u]]:
            assert a != 0, "the dummy is queued nowhere"
            assert a not in road_of, f"agent {a} stands in two FIFOs"
            road_of[int(a)] = int(u)
    return road_of, ids[:, 0].copy(), n


def check_facts(states, edge_index, Nmax):
    """``states``: the oracle's x before the first frame and after every frame. Fact 1: an agent id other than 0 heads at most
    one non-empty road. Fact 2: an agent whose road changes from p to u was p's head in the snapshot before, the edge p -> u
    exists, and if u was empty before it is u's head now. -> (moves seen, moves into an empty road)."""
    edges = set(map(tuple, edge_index.t().tolist()))
    prev = _snapshot(states[0], Nmax)
    moves = into_empty = 0
    for x in states[1:]:
        cur = _snapshot(x, Nmax)
        road_of, head, n = cur
        live = head[(n > 0) & (head != 0)]
        assert len(set(live.tolist())) == live.size, "fact 1: an agent heads two non-empty roads"
        p_road, p_head, p_n = prev
        for a, u in road_of.items():
            p = p_road.get(a)
            if p is None or p == u:
                continue
            moves += 1
            assert p_n[p] > 0 and p_head[p] == a, f"fact 2: agent {a} left road {p} without being its head"
            assert (p, u) in edges, f"fact 2: agent {a} went {p} -> {u} over no edge"
            if p_n[u] == 0:
                into_empty += 1
                assert head[u] == a, f"fact 2: agent {a} entered the empty road {u} and is not its head"
        prev = cur
    return moves, into_empty


def _torus_states(chooser):
    """The "spread" case of test_router_hold_host (128 agents, 300 frames, its torch noise) under ``chooser``: "hold" (the
    free-flow hold router), "hold_first_hop" (with the first-hop rule of DESIGN 4.23) or "random" (a uniformly drawn
    out-edge per road and frame)."""
    import departure_restatement as D
    import irregular_graphs as G
    import router_hold_restatement as H
    import test_router_hold_host as RH
    from baseline_restatement import destination_columns
    from oracle import routing, sim
    from tarl_hip.engine import EPISODE_START
    net, pop, T = RH._case("spread")
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    c = sim.Cols(Nmax)
    gumbel = RH._gumbel(ei.size(1), T)
    adj = net.dense_adjacency()
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    dests = sorted({int(d) for d in ag[:, 1].tolist() if 0 <= d < N})
    slot_of = torch.full((N,), -1, dtype=torch.int64)
    slot_of[dests] = torch.arange(len(dests))
    table = destination_columns(ei, routing.edge_travel_time(x, ei, net.congestion_constant, Nmax), N, dests)
    gen = torch.Generator().manual_seed(3)
    none = torch.zeros(ei.size(1), dtype=torch.long)
    states = [x.clone()]
    for t in range(T):
        clock = float(EPISODE_START + t)
        action = none
        if chooser == "random":
            action = G.onehot_of(G.random_actions(net, gen), ei.size(1))
        else:
            x = H.hold_choice(x, ag, table, Nmax)
            if chooser == "hold_first_hop":
                wr, val = D.route_table(x.numpy(), ag.numpy(), table.numpy(), clock, Nmax, slot_of=slot_of.numpy())
                D.apply(x, wr, val, Nmax)
        sim.env_step(x, ag, ei, net.edge_attr, adj, action, clock, Nmax, gumbel=gumbel(t),
                     congestion_constant=net.congestion_constant)
        states.append(x.clone())
    return net, states, ag


@pytest.mark.parametrize("chooser", ["hold", "hold_first_hop", "random"])
def test_the_two_facts_on_the_torus(chooser):
    from oracle import sim
    net, states, ag = _torus_states(chooser)
    moves, into_empty = check_facts(states, net.edge_index, net.Nmax)
    print(f"[path trace] torus, {chooser}: {moves} moves, {into_empty} into an empty road, {int(ag[1:, sim.DONE].sum())} arrivals")
    assert moves > 100 and into_empty > 0


@pytest.mark.parametrize("name", ["MIXED", "HUB126"])
def test_the_two_facts_on_the_irregular_graphs(name):
    import irregular_graphs as G
    from oracle import sim
    net = G.graph(name)
    pop = G.population(net, G.CENSUS[name]["per_road"], seed=5)
    x, ag, adj = net.x.clone(), pop.clone(), net.dense_adjacency()
    states = [x.clone()]
    for s, (action, u) in enumerate(G.census_inputs(net, 120, 5)):
        sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, 100 + s, net.Nmax, uniform=u,
                     congestion_constant=net.congestion_constant)
        states.append(x.clone())
    moves, into_empty = check_facts(states, net.edge_index, net.Nmax)
    print(f"[path trace] {name}: {moves} moves, {into_empty} into an empty road")
    assert moves > 100      # (these networks are crowded: a move into an empty road is rare here, the torus cases have them)


def test_the_trace_of_an_oracle_run_is_a_walk():
    """The restatement fed the oracle's heads after every frame of the first-hop hold router: nothing is ``bad``, every kept
    route is a walk on the graph, and with the router's own free-flow weights every trip follows its tree — excess exactly 0."""
    from baseline_restatement import destination_columns  # noqa: F401  (the router's table: built in _torus_states)
    from oracle import routing, sim
    net, states, ag = _torus_states("hold_first_hop")
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    A = ag.size(0)
    graph = P.csr(ei.numpy(), N)
    x0 = states[0]
    w = routing.edge_travel_time(x0, ei, net.congestion_constant, Nmax).numpy().astype(np.float32)
    dist = _dist(ei.numpy(), w, N)
    slot = np.arange(N, dtype=np.int32)
    st = P.new_state(1, A, 64)
    a_dest = ag[:, 1].numpy().astype(np.int64)[None]
    for x in states[1:]:
        P.sighting_pass(st, P.heads_of(x, Nmax)[:, None], graph, a_dest, w, dist, slot)
    assert st["bad"].tolist() == [0]
    done = ag[:, sim.DONE].numpy() == 1
    assert done[1:].sum() == 128
    edges = set(map(tuple, ei.t().tolist()))
    for a in range(1, A):
        r = st["route"][0, a, :st["roads"][0, a]].tolist()
        assert all((p, u) in edges for p, u in zip(r, r[1:]))
        # (the insert places a departing agent on the road its origin row SELECTS: the origin itself or one of its successors)
        assert r and (r[0] == int(ag[a, 0]) or (int(ag[a, 0]), r[0]) in edges), "first seen on, or one road behind, the origin"
        nxt = {u for p, u in edges if p == r[-1]}
        assert r[-1] == int(ag[a, 1]) or int(ag[a, 1]) in nxt, "a delivered trip ends on, or one road short of, its destination"
    assert (st["excess"][0][done] == 0.0).all() and (st["off_tree"][0][done] == 0).all()
    assert (st["path_cost"][0, 1:] > 0).any()


def _dist(edge_index, w, N):
    """dist[d][u]: the fp64 shortest-path cost u -> d formed as sp_trees.h forms it, w + dist[next] from the destination out
    (Bellman-Ford on the reverse graph; exact ties resolve to the same value)."""
    src, dst = edge_index
    dist = np.full((N, N), np.inf)
    for d in range(N):
        dv = dist[d]
        dv[d] = 0.0
        for _ in range(N):
            cand = w.astype(np.float64) + dv[dst]
            new = dv.copy()
            np.minimum.at(new, src, cand)
            if np.array_equal(new, dv):
                break
            dv[:] = new
    return dist


# ---- 2. crafted cases ---------------------------------------------------------------------------------------------------------------
# roads 0 .. 5; 0 -> 1 twice (an ambiguous edge: ids 0 and 5, different weights), 1 -> 0, 1 -> 2, 2 -> 0, 2 -> 3, 3 -> 4
EI = np.array([[0, 1, 1, 2, 2, 0, 3], [1, 0, 2, 0, 3, 1, 4]])
W = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], np.float32)
N6 = 6
BIG = float(2 ** 60)


def _hd(cells, B=1):
    """{(road, env): (agent, count byte)} -> the packed word 0 of every (road, environment)."""
    hd = np.zeros((N6, B), np.int64)
    for (u, b), (a, cnt) in cells.items():
        hd[u, b] = (a << 8) | cnt
    return hd


def _walk(roads, L, *, agent=1, A=3, defect=None, **kw):
    st = P.new_state(1, A, L)
    for u in roads:
        P.sighting_pass(st, _hd({(u, 0): (agent, 1)}), P.csr(EI, N6), defect=defect, **kw)
    return st


def _tables():
    """Destination 4 (slot 0) is reachable from 0 .. 3; destination 5 (slot 1) from nowhere; road 1 has no slot."""
    dist = np.full((2, N6), np.inf)
    dist[0, [4, 3, 2, 1, 0]] = [0.0, 64.0, 80.0, 84.0, 85.0]
    dist[1, 5] = 0.0
    slot = np.array([-1, -1, -1, -1, 0, 1], np.int32)
    return dist, slot


def test_an_agent_seen_on_one_road_only():
    st = _walk([2, 2, 2], 4)
    assert st["roads"][0, 1] == 1 and st["revisits"][0, 1] == 0 and st["path_cost"][0, 1] == 0.0
    assert st["route"][0, 1].tolist() == [2, -1, -1, -1] and st["last_road"][0, 1] == 2
    assert max(st["roads"][0, 1] - 1, 0) == 0
    assert st["roads"][0, 2] == 0 and st["last_road"][0, 2] == -1 and st["bad"].tolist() == [0]


def test_a_three_road_loop():
    st = _walk([0, 1, 2, 0], 8)
    assert st["roads"][0, 1] == 4 and st["revisits"][0, 1] == 1 and st["route"][0, 1, :4].tolist() == [0, 1, 2, 0]
    assert st["bad"].tolist() == [0]


@pytest.mark.parametrize("L,kept,revisits", [(0, [], 0), (1, [0], 1), (2, [0, 1], 2)])
def test_truncation_and_revisits_against_the_kept_prefix(L, kept, revisits):
    st = _walk([0, 1, 0, 1, 2], L)
    assert st["roads"][0, 1] == 5 and st["route"][0, 1].tolist() == kept and st["revisits"][0, 1] == revisits
    assert st["roads"][0, 1] > L      # truncated


def test_costs_excess_and_an_unreachable_destination():
    dist, slot = _tables()
    a_dest = np.array([[0, 4, 5, 1]])
    kw = dict(a_dest=a_dest, weights=W, dist=dist, dest_slot=slot, A=4)
    on_tree = _walk([1, 2, 3], 4, agent=1, **kw)                 # 1 -> 2 (4) -> 3 (16): the tree towards 4
    assert on_tree["path_cost"][0, 1] == 20.0 and on_tree["excess"][0, 1] == 0.0 and on_tree["off_tree"][0, 1] == 0
    detour = _walk([1, 0, 1], 4, agent=1, **kw)                  # 1 -> 0 (2) -> 1 (first match: 1)
    assert detour["path_cost"][0, 1] == 3.0 and detour["excess"][0, 1] == ((2.0 + 85.0) - 84.0) + ((1.0 + 84.0) - 85.0)
    lost = _walk([1, 2], 4, agent=2, **kw)                       # bound for 5: no path
    assert lost["path_cost"][0, 2] == 4.0 and lost["off_tree"][0, 2] == 1 and lost["excess"][0, 2] == 0.0
    no_slot = _walk([1, 2], 4, agent=3, **kw)                    # bound for road 1: no tree was built for it
    assert no_slot["off_tree"][0, 3] == 1
    without = _walk([1, 2, 3], 4)
    assert without["path_cost"][0, 1] == 0.0 and without["roads"][0, 1] == 3


def test_what_the_pass_ignores_and_what_it_counts_as_bad():
    g = P.csr(EI, N6)
    st = P.new_state(2, 3, 2)
    P.sighting_pass(st, _hd({(0, 0): (1, 0), (1, 0): (2, 0x80), (2, 0): (0, 3), (3, 1): (7, 1)}, B=2), g)
    assert st["roads"].sum() == 0 and (st["last_road"] == -1).all()      # stale id, DIRTY empty row, agent 0
    assert st["bad"].tolist() == [0, 1]                                  # a head id beyond the agent table
    P.sighting_pass(st, _hd({(0, 0): (1, 1)}, B=2), g)
    P.sighting_pass(st, _hd({(4, 0): (1, 1)}, B=2), g)                   # 0 -> 4: no such edge
    assert st["bad"].tolist() == [1, 1] and st["roads"][0, 1] == 2 and st["route"][0, 1].tolist() == [0, 4]


# ---- 3. one defect at a time ------------------------------------------------------------------------------------------------------
def _defect_cases(defect):
    dist, slot = _tables()
    g = P.csr(EI, N6)
    kw = dict(a_dest=np.array([[0, 4, 4], [0, 5, 4]]), weights=W, dist=dist, dest_slot=slot)
    out = {}
    st = P.new_state(1, 3, 2)
    P.sighting_pass(st, _hd({(3, 0): (1, 0)}), g, defect=defect)
    out["stale_head"] = P.arrays(st)
    out["one_road"] = P.arrays(_walk([2, 2, 2], 4, defect=defect))
    out["ambiguous_edge"] = P.arrays(_walk([0, 1], 4, defect=defect, a_dest=kw["a_dest"][:1], weights=W, dist=dist, dest_slot=slot))
    big = dist.copy()
    big[0, 0] = big[0, 1] = BIG
    out["rounding"] = P.arrays(_walk([1, 0], 4, defect=defect, a_dest=kw["a_dest"][:1], weights=W, dist=big, dest_slot=slot))
    out["prefix"] = P.arrays(_walk([0, 1, 0, 1, 2], 1, defect=defect))
    st = P.new_state(2, 3, 2)
    for u in (1, 2):
        P.sighting_pass(st, _hd({(u, 1): (1, 1)}, B=2), g, defect=defect, **kw)
    out["second_environment"] = P.arrays(st)
    return out


CHANGES = {"count_dropped": "stale_head", "same_road_appended": "one_road", "last_match": "ambiguous_edge",
           "excess_reordered": "rounding", "scan_all_h": "prefix", "wrong_env_dest": "second_environment"}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("defect", sorted(CHANGES))
def test_each_defect_changes_its_case(defect):
    good, bad = _defect_cases(None), _defect_cases(defect)
    assert not _same(good[CHANGES[defect]], bad[CHANGES[defect]]), defect
    for name in good:      # and nothing but its own case
        if name != CHANGES[defect]:
            assert _same(good[name], bad[name]), (defect, name)
    assert set(CHANGES) == set(P.DEFECTS)
    with pytest.raises(ValueError, match="defect"):
        _walk([0], 1, defect="other")


def test_the_named_cases_hold_what_they_are_built_for():
    good = _defect_cases(None)
    assert good["ambiguous_edge"]["path_cost"][0, 1] == 1.0          # edge id 0, not id 5 (32)
    assert good["rounding"]["excess"][0, 1] == 0.0                   # (2 + 2^60) - 2^60: the weight is rounded away
    assert _defect_cases("excess_reordered")["rounding"]["excess"][0, 1] == 2.0
    assert good["second_environment"]["off_tree"][1, 1] == 1 and good["second_environment"]["excess"][1, 1] == 0.0
    assert good["prefix"]["revisits"][0, 1] == 1 and _defect_cases("scan_all_h")["prefix"]["revisits"][0, 1] == 2


def test_agent_stats_restatement_on_a_small_table():
    st = P.new_state(3, 3, 2)
    st["roads"][:, 1] = [3, 0, 5]
    st["revisits"][:, 1] = [0, 0, 2]
    st["path_cost"][:, 1] = [10.0, 0.0, 30.0]
    st["excess"][:, 1] = [0.0, 0.0, 4.0]
    done = np.array([[0, 1, 0], [0, 0, 0], [0, 1, 0]], bool)
    s = P.agent_stats(st, done, 2)
    assert s["n_done"][1] == 2 and s["n_seen"][1] == 2 and s["n_trunc"][1] == 2 and s["n_loop"][1] == 1
    assert s["n_zero_excess"][1] == 1 and s["roads_max"][1] == 5 and s["moves_sum"][1] == 6.0 and s["moves_sumsq"][1] == 20.0
    assert s["cost_sum"][1] == 40.0 and s["excess_sumsq"][1] == 16.0 and s["n_done"][2] == 0
    pair = P.agent_stats(st, done, 2, st, done)
    assert pair["n_both"][1] == 2 and pair["dmoves_sum"][1] == 0.0 and pair["dexcess_sumsq"][1] == 0.0


# ---- 4. the host side ----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_and_refuse_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert int(re.search(r"#define TARL_ABI_VERSION (\d+)", hdr).group(1)) == 5 and L.tarl_abi_version() == 5
    for name in ("tarl_path_trace_reset", "tarl_fused_path_trace", "tarl_path_agent_stats"):
        assert name in lib.SIGNATURES and name in hdr
    null = None
    one = ctypes.c_void_p(8)      # never dereferenced: every call below is refused on the host
    state = [one] * 8
    assert L.tarl_path_trace_reset(1, 2, 1, *([null] * 8), null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_path_trace_reset(1, 0, 1, *state, null) == -1 and b"num_agents" in L.tarl_last_error()
    assert L.tarl_path_trace_reset(1, (1 << 24) + 1, 1, *state, null) == -1
    assert L.tarl_path_trace_reset(1, 2, 4097, *state, null) == -1 and b"4096" in L.tarl_last_error()
    assert L.tarl_path_trace_reset(1, 2, -1, *state, null) == -1
    assert L.tarl_path_trace_reset(0, 2, 1, *state, null) == -1
    assert L.tarl_path_trace_reset((1 << 31) - 1, 1 << 24, 4096, *state, null) == -1 and b"overflow" in L.tarl_last_error()
    assert L.tarl_path_trace_reset(1, 2, 1, *(state[:6] + [null, one]), null) == -1 and b"route" in L.tarl_last_error()
    assert L.tarl_fused_path_trace(null, null, 1, 15, 2, 1, *state, null, null, null, 0, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_path_agent_stats(*([null] * 6), 18, null, null, null, 0, 1, 2, 1, null, null, null) == -1
    assert L.tarl_path_agent_stats(*([one] * 6), 18, one, null, null, 0, 1, 2, 1, one, one, null) == -1
    assert b"come together" in L.tarl_last_error()
    assert L.tarl_path_agent_stats(*([one] * 6), 17, null, null, null, 0, 1, 2, 1, one, one, null) == -1
    assert b"overlap" in L.tarl_last_error()
    assert L.tarl_path_agent_stats(*([one] * 6), 18, null, null, null, 0, 1, 2, 5000, one, one, null) == -1


def test_the_fused_handle_did_not_grow():
    from tarl_hip import lib
    hdr = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    body = re.search(r"typedef struct tarl_fused \{(.*?)\} tarl_fused;", hdr, flags=re.S).group(1)
    assert "path" not in body.lower()
    assert ctypes.sizeof(lib.FusedStruct) == 8 * 31


def test_parser_and_argument_rules():
    import importlib
    main = importlib.import_module("main")
    from src.runner import RunnerArgs
    ns = main.build_parser().parse_args(["--eval-paths", "--eval-paths-max-hops", "0", "--eval-paths-routes", "3"])
    assert ns.eval_paths is True and ns.eval_paths_max_hops == 0 and ns.eval_paths_routes == 3
    ns = main.build_parser().parse_args([])
    assert ns.eval_paths is False and ns.eval_paths_max_hops is None and ns.eval_paths_routes == 0
    sc = dict(scenario="synthetic-1024-300")
    ok = RunnerArgs(algo="mpnn", mode="eval", eval_envs=2, eval_paths=True, eval_paths_max_hops=0, **sc)
    assert ok.eval_paths and RunnerArgs(algo="dijkstra", mode="eval", dijkstra_envs=2, eval_paths=True, eval_paths_routes=1, **sc)
    for kw, msg in ((dict(eval_paths=True), "eval_envs > 0 or dijkstra_envs > 0"),
                    (dict(eval_envs=2, eval_paths=True, mode="train"), "mode 'eval'"),
                    (dict(eval_envs=2, eval_paths_max_hops=4), "needs that flag"),
                    (dict(eval_envs=2, eval_paths_routes=1), "needs that flag"),
                    (dict(eval_envs=2, eval_paths=True, eval_paths_max_hops=4097), r"\[0, 4096\]"),
                    (dict(eval_envs=2, eval_paths=True, eval_paths_max_hops=-1), r"\[0, 4096\]"),
                    (dict(eval_envs=2, eval_paths=True, eval_paths_routes=-1), ">= 0"),
                    (dict(eval_envs=2, eval_paths=True, eval_paths_max_hops=0, eval_paths_routes=1), "none is kept")):
        with pytest.raises(ValueError, match=msg):
            RunnerArgs(**{"algo": "mpnn", "mode": "eval", **sc, **kw})


def test_evaluator_signature_and_the_reports_of_a_run_without_the_flag():
    """The new arguments are off by default, and everything a run without them reports is still the snapshot recorded before
    the trip reward existed (tests/golden/trip_reward_off_snapshot.json, built by test_trip_reward_host.build_snapshot)."""
    import inspect
    import json
    import test_trip_reward_host as TR
    from tarl_hip.evaluator import EvalResult, VecEvaluator, path_lines, path_report
    sig = inspect.signature(VecEvaluator.__init__).parameters
    assert sig["paths"].default is False and sig["path_max_hops"].default is None and sig["path_weights"].default is None
    assert inspect.signature(VecEvaluator.run).parameters["path_pair"].default is None
    assert json.dumps(TR.build_snapshot(), indent=1) + "\n" == open(TR.GOLDEN).read()
    res = EvalResult(envs=2, head="embedding", deterministic=True, frames_run=10)
    assert res.paths is None and "paths" not in res.to_dict(per_env=True)
    rep = path_report(res)
    assert rep == {"available": False, "reason": "the run did not trace its paths"} and path_lines(rep)[0].startswith("not available")


def _result(excess, head="embedding", pair=None):
    """An EvalResult as ``VecEvaluator(paths=True)`` leaves it, from hand-made traces of two agents in two environments."""
    from tarl_hip.evaluator import EvalResult
    st = P.new_state(2, 3, 2)
    st["roads"][:] = [[0, 3, 1], [0, 4, 0]]
    st["revisits"][:] = [[0, 0, 0], [0, 1, 0]]
    st["path_cost"][:] = [[0, 20.0, 0], [0, 30.0, 0]]
    st["excess"][:] = excess
    done = np.array([[0, 1, 0], [0, 1, 0]], bool)
    stats = P.agent_stats(st, done, 2, *(pair or ()))
    res = EvalResult(envs=2, head=head, deterministic=True, frames_run=50, settings=dict(seed=1, env_base=0))
    res.paths = dict(P.arrays(st), done=done)
    res.path_stats = stats
    res.path_meta = dict(max_hops=2, weights=True, note=None, first_bin=5, bin_seconds=3600, num_bins=1,
                         origin=np.array([0, 4, 5]), destination=np.array([0, 9, 8]), departure=np.array([1e9, 21540.0, 21550.0]),
                         paired=pair is not None)
    res.path_routes = (st["route"], np.minimum(st["roads"], 2))
    return res, st, done


def test_report_on_hand_made_traces():
    from tarl_hip.evaluator import path_lines, path_report, path_summary
    res, st, done = _result([[0, 0.0, 0], [0, 10.0, 0]])
    rep = path_report(res)
    s = rep["summary"]
    assert s["trips"] == 2 and s["mean_moves"] == 2.5 and s["share_loop"] == 0.5 and s["share_truncated"] == 1.0
    assert (s["seen_in_every"], s["seen_in_some"], s["seen_in_none"]) == (1, 1, 0)
    assert s["weights"]["mean_cost"] == 25.0 and s["weights"]["mean_excess"] == 5.0 and s["weights"]["excess_over_cost"] == 0.2
    assert s["weights"]["share_zero_excess"] == 0.5 and s["open"]["traces"] == 1 and s["weights"]["mean_travel_time"] is None
    row = rep["rows"][0]
    assert row["agent"] == 1 and row["moves_mean"] == 2.5 and row["excess_mean"] == 5.0 and row["n_trunc"] == 2
    assert rep["rows"][1]["moves_mean"] is None and rep["by_departure"][0]["trips"] == 2
    assert [r["agent"] for r in s["top_excess"]] == [1]
    text = "\n".join(path_lines(rep))
    assert "mean excess:" in text and "agents with the largest mean excess" in text
    import json
    json.dumps(path_summary(rep))
    # the baseline's launch pairs baseline - policy; the report turns it round
    base, _, _ = _result([[0, 0.0, 0], [0, 0.0, 0]], head="dijkstra_hold", pair=(st, done))
    paired = path_report(res, baseline=base)
    assert paired["rows"][0]["paired_n"] == 2 and paired["rows"][0]["paired_excess_diff_mean"] == 5.0
    assert paired["rows"][0]["paired_moves_diff_mean"] == 0.0 and paired["summary"]["paired"]["mean_excess_diff"] == 5.0
    unpaired, _, _ = _result([[0, 0.0, 0], [0, 0.0, 0]], head="dijkstra_hold")
    assert path_report(res, baseline=unpaired)["summary"]["paired"]["available"] is False


def test_ops_refuse_wrong_arguments_without_a_gpu():
    from tarl_hip import lib, ops
    with pytest.raises(ValueError, match="L must be"):
        ops.path_trace_state(1, 2, 4097, "cpu")
    with pytest.raises(ValueError, match="L must be"):
        ops.path_trace_state(1, 2, -1, "cpu")
    with pytest.raises(ValueError, match="A in"):
        ops.path_trace_state(1, 0, 4, "cpu")
    st = ops.path_trace_state(2, 3, 4, "cpu")
    assert tuple(st.route.shape) == (2, 3, 4) and st.path_cost.dtype == torch.float64 and set(st.tensors()) == {
        "last_road", "roads", "revisits", "off_tree", "path_cost", "excess", "route", "bad"}
    with pytest.raises(lib.TarlError, match="GPU"):      # no CPU fallback
        ops.path_trace_reset(st)
    with pytest.raises(ValueError, match="state is for"):
        ops.path_agent_stats(st, torch.zeros((2, 4, 9)))
    with pytest.raises(ValueError, match="come together"):
        ops.path_agent_stats(st, torch.zeros((2, 3, 9)), state_b=st)
