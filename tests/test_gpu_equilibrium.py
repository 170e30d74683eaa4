"""GPU: equilibrium metrics (csrc/equilibrium.hip, the gap outputs of csrc/msa.hip, src/algorithms/equilibrium.py) against
the float64 numpy restatement of tests/equilibrium_restatement.py (scipy's Dijkstra, the formulas of the model)."""
import importlib
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG

import equilibrium_restatement as R

pytestmark = pytest.mark.gpu
OBJECTIVES = ("ue", "so")
SOLVERS = ("cfw", "fw", "msa")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def _agents(features):
    return types.SimpleNamespace(agent_features=features.cuda(), ORIGIN=0, DESTINATION=1)


def _torus(W, H, agents, seed=5):
    from src._compat import Data
    from tarl_hip import synth
    net = synth.torus_network(W, H, heterogeneous=True, seed=1)
    graph = Data(x=net.x.cuda(), edge_index=net.edge_index.cuda(), num_roads=net.num_roads)
    return graph, _agents(synth.population(agents, net.num_roads, seed=seed))


def _matsim_grid(tmp_path, trips=600):
    """A MATSim grid with SRC / DEST pseudo-nodes (zero-cost nodes) and trips between arbitrary nodes, so that some OD
    pairs have no path."""
    from src.matsim_io import build_network
    from tarl_hip import synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, _ = build_network(str(tmp_path / "network"))
    graph.x, graph.edge_index = graph.x.cuda(), graph.edge_index.cuda()
    N = graph.x.size(0)
    gen = torch.Generator().manual_seed(3)
    feats = torch.zeros((trips + 1, 9))
    feats[1:, 0] = torch.randint(0, N, (trips,), generator=gen).float()
    feats[1:, 1] = torch.randint(0, N, (trips,), generator=gen).float()
    return graph, _agents(feats)


def _four_roads(trips_od=15, trips_bd=4):
    """The hand-built graph of equilibrium_restatement.four_road_model as a simulator graph and an agent table."""
    from src._compat import Data
    m = R.four_road_model(trips_od, trips_bd)
    Nmax = 2
    x = torch.zeros((4, 3 * Nmax + 7))
    x[:, 3 * Nmax + 2] = torch.tensor(m.ff, dtype=torch.float32)
    x[:, 3 * Nmax + 4] = torch.tensor(m.cap, dtype=torch.float32)
    x[:, 3 * Nmax + 6] = torch.arange(4, dtype=torch.float32)
    graph = Data(x=x.cuda(), edge_index=torch.tensor(np.stack([m.src, m.dst]), dtype=torch.int64).cuda(), num_roads=4)
    feats = torch.zeros((1 + trips_od + trips_bd, 9))
    feats[1:1 + trips_od, 0], feats[1:1 + trips_od, 1] = 0.0, 3.0
    feats[1 + trips_od:, 0], feats[1 + trips_od:, 1] = 2.0, 3.0
    return graph, _agents(feats)


def _close(a, b, rtol):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


# ---- 1. assignment with gap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["torus25", "matsim"])
def test_assignment_with_gap(ops, tmp_path, case):
    from src.algorithms.user_equilibrium_msa import build_demand
    graph, ag = _torus(25, 25, 16_384) if case == "torus25" else _matsim_grid(tmp_path)
    model = R.Model.from_graph(graph, ag)
    N, ei = graph.x.size(0), graph.edge_index
    plan = ops.Plan(ei.cpu(), N)
    # node costs of some loaded state: the BPR cost at pseudo-random volume / capacity ratios, 0 off the roads
    ratio = torch.rand(N, generator=torch.Generator().manual_seed(7), dtype=torch.float64) * 2.0
    cost_h = np.where(model.road, model.ff * (1.0 + 0.15 * ((ratio.numpy() ** 2) ** 2)), 0.0)
    cost = torch.tensor(cost_h).cuda()
    w = cost[ei[1]].contiguous()
    od_o, od_d, od_vol = (t.cuda() for t in build_demand(ag, N))
    assert np.array_equal(od_o.cpu().numpy(), model.od_o) and np.array_equal(od_d.cpu().numpy(), model.od_d)
    origins, per = torch.unique_consecutive(od_o, return_counts=True)
    od_ptr = torch.zeros(origins.numel() + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(per, 0, out=od_ptr[1:])
    road = torch.tensor(model.road).to(torch.uint8).cuda()
    zeros = lambda: torch.zeros(N, dtype=torch.float64, device="cuda")        # noqa: E731

    # per origin: flows as the existing entry point, SPTT from tarl_sssp_f64's distances
    aux0, aux1 = zeros(), zeros()
    ops.msa_assign_trees(plan, w, origins, od_ptr, od_d, od_vol, road, aux0)
    sptt_part, unr_part = ops.msa_assign_trees_gap(plan, w, origins, od_ptr, od_d, od_vol, road, aux1)
    assert float(aux0.sum()) > 0 and torch.allclose(aux1, aux0, rtol=1e-12, atol=0.0)
    dist = ops.shortest_path_trees(plan, w, origins, want_pred=False)[0].cpu().numpy()
    pd = dist[model.slot, model.od_d]
    fin = np.isfinite(pd)
    assert _close(float(sptt_part.sum()), float(np.sum(model.od_vol[fin] * pd[fin])), 1e-12)
    part, unr = np.zeros(origins.numel()), np.zeros(origins.numel())
    for p in range(pd.size):                               # pair order, float64, one addition at a time
        if fin[p]:
            part[model.slot[p]] += model.od_vol[p] * pd[p]
        else:
            unr[model.slot[p]] += model.od_vol[p]
    assert np.array_equal(sptt_part.cpu().numpy(), part), "per-origin SPTT is not the pair-order sum"
    assert np.array_equal(unr_part.cpu().numpy(), unr)

    # the restatement: Dijkstra distances bit for bit, unrouted volume exactly
    sptt_r, unrouted_r, pd_r, part_r, _ = model.sptt(cost_h)
    assert np.array_equal(pd, pd_r)
    assert float(unr_part.sum()) == unrouted_r
    assert (unrouted_r > 0) == (case == "matsim")
    assert _close(float(sptt_part.sum()), sptt_r, 1e-12)

    # all pairs: flows as the existing entry point, pair costs = the restatement's distances bit for bit
    next_hop = ops.all_pairs_shortest_paths(plan, w)[0][0]
    aux2, aux3 = zeros(), zeros()
    ops.msa_assign(next_hop, od_o, od_d, od_vol, road, aux2)
    pc = ops.msa_assign_gap(next_hop, od_o, od_d, od_vol, road, cost, aux3)
    assert torch.allclose(aux3, aux2, rtol=1e-12, atol=0.0)
    assert np.array_equal(pc.cpu().numpy(), pd_r), "pair_cost differs from Dijkstra's distances"
    ok = torch.isfinite(pc)
    sptt_ap = float((od_vol * torch.where(ok, pc, torch.zeros_like(pc))).sum())
    assert _close(sptt_ap, float(sptt_part.sum()), 1e-12)
    assert float(od_vol[~ok].sum()) == unrouted_r
    if case == "torus25":                                   # no ties on the heterogeneous torus: the same paths
        assert torch.allclose(aux3, aux1, rtol=1e-9, atol=1e-9)

    # two calls: bitwise equal
    s2, u2 = ops.msa_assign_trees_gap(plan, w, origins, od_ptr, od_d, od_vol, road, zeros())
    pc2 = ops.msa_assign_gap(next_hop, od_o, od_d, od_vol, road, cost, zeros())
    assert torch.equal(s2, sptt_part) and torch.equal(u2, unr_part) and torch.equal(pc2, pc)


# ---- 2. the step kernel ------------------------------------------------------------------------------------------------------
def _step_inputs(N, seed, kind="random"):
    rng = np.random.default_rng(seed)
    ff, cap = rng.uniform(5.0, 20.0, N), rng.uniform(5.0, 30.0, N)
    road = rng.uniform(size=N) > 0.2
    road[0] = True
    f, y = rng.uniform(0.0, 40.0, N), rng.uniform(0.0, 40.0, N)
    if kind == "conjugate":                                 # a previous target that gives 0 < alpha < 0.99
        sp = np.maximum(f - 0.5 * (y - f) + rng.uniform(0.0, 0.5, N), 0.0)
    elif kind == "zigzag":
        # the all-or-nothing flows point against the previous direction u and, across it, from the dear roads to the cheap
        # ones (v): a conjugate weight inside (0, 0.99) and a descent direction. v is scaled up until the full step
        # overshoots (the restatement's g(1) > 0, both objectives), so that the line search has its root inside (0, 1)
        f = rng.uniform(20.0, 40.0, N)
        u = rng.uniform(-4.0, 4.0, N)
        c = R.bpr(ff, cap, road, f, 0.15)
        v = -(c - np.median(c[road])) / c[road].std()
        sp, m = f + u, 1.0
        while True:
            y = np.maximum(f - u + m * v, 0.0)
            if all(R.step(f, y, sp, ff, cap, road, o, "cfw", 5)["g1"] > 0.0 for o in OBJECTIVES):
                break
            m *= 2.0
    else:
        sp = rng.uniform(0.0, 40.0, N)
    return ff, cap, road, f, y, sp


def _run_step(ops, ff, cap, road, f, y, sp, objective, rule, iteration=5, msa_step=0.2):
    dev = lambda a: torch.tensor(a).cuda()                   # noqa: E731
    fd, sd = dev(f), dev(sp)
    cost, rec = ops.bpr_step(fd, dev(y), sd, dev(ff), dev(cap), dev(road).to(torch.uint8), objective=objective,
                             rule=rule, msa_step=msa_step, iteration=iteration)
    return fd, sd, cost, rec


@pytest.mark.parametrize("N", [7, 256, 2_500, 25_000, 300_000])
def test_step_kernel_against_restatement(ops, N):
    for objective in OBJECTIVES:
        for rule, kind in (("msa", "random"), ("fw", "random"), ("cfw", "random"), ("cfw", "conjugate"),
                           ("cfw", "zigzag"), ("fw", "zigzag")):
            ff, cap, road, f, y, sp = _step_inputs(N, seed=N + len(rule), kind=kind)
            assert (~road).any() or N == 7
            fd, sd, cost, rec = _run_step(ops, ff, cap, road, f, y, sp, objective, rule)
            alpha, lam, tstt, fc, g0, g1, halvings, it = rec.cpu().tolist()
            ref = R.step(f, y, sp, ff, cap, road, objective, rule, 5, msa_step=0.2, lam=lam)
            tag = f"N={N} {objective} {rule} {kind}"
            print(f"{tag}: alpha {alpha!r} (ref {ref['alpha']!r}) lambda {lam!r} (ref {ref['lam']!r}, "
                  f"bound {ref['lam_bound']:.3e}) halvings {halvings:.0f}")
            assert it == 5.0
            assert _close(alpha, ref["alpha"], 1e-12), tag
            if kind == "conjugate":
                assert 0.0 < alpha < 0.99, tag
            if kind == "zigzag" and N in (256, 300_000):            # what the restatement gives on these inputs
                assert 0.0 < lam < 1.0 and halvings >= 50 and (rule == "fw" or 0.0 < ref["alpha"] < 0.99), tag
            if rule == "msa":
                assert lam == 0.2
            else:
                assert abs(lam - ref["lam"]) <= ref["lam_bound"], tag
                assert halvings <= 60
            assert np.allclose(sd.cpu().numpy(), ref["s"], rtol=1e-12, atol=0.0), tag
            assert np.allclose(fd.cpu().numpy(), ref["f"], rtol=1e-12, atol=0.0), tag
            assert np.allclose(cost.cpu().numpy(), ref["cost"], rtol=1e-12, atol=0.0), tag
            assert bool((cost.cpu().numpy()[~road] == 0.0).all())
            assert _close(tstt, ref["tstt"], 1e-12) and _close(fc, ref["fc"], 1e-12), tag
            # bitwise repeatability
            fd2, sd2, cost2, rec2 = _run_step(ops, ff, cap, road, f, y, sp, objective, rule)
            assert torch.equal(fd2, fd) and torch.equal(sd2, sd) and torch.equal(cost2, cost) and torch.equal(rec2, rec)


@pytest.mark.parametrize("N", [7, 2_500, 300_000])
def test_step_kernel_forced_cases(ops, N):
    ff, cap, road, f, y, sp = _step_inputs(N, seed=11)
    for objective in OBJECTIVES:
        for rule in ("fw", "cfw"):
            # every component moves down: g(1) < 0, the full step
            fd, sd, _, rec = _run_step(ops, ff, cap, road, f, 0.5 * f, sp if rule == "fw" else f.copy(), objective, rule)
            assert rec[5].item() <= 0.0 and rec[1].item() == 1.0
            # the first conjugate step (s_prev = f): Dn = 0, alpha = 0
            _, sd, _, rec = _run_step(ops, ff, cap, road, f, y, f.copy(), objective, "cfw")
            assert rec[0].item() == 0.0 and np.array_equal(sd.cpu().numpy(), y)
            # y = f: nothing moves
            fd, _, _, rec = _run_step(ops, ff, cap, road, f, f.copy(), sp, objective, rule)
            assert np.array_equal(fd.cpu().numpy(), f) and rec[0].item() == 0.0
        # the first load: lambda = 1 whatever the rule; evaluation: nothing changes, the same totals as a zero step
        for rule in SOLVERS:
            fd, _, _, rec = _run_step(ops, ff, cap, road, np.zeros(N), y, np.zeros(N), objective, rule, iteration=1, msa_step=1.0)
            assert rec[1].item() == 1.0 and np.array_equal(fd.cpu().numpy(), y)
        fd = torch.tensor(f).cuda()
        cost, rec = ops.bpr_step(fd, None, None, torch.tensor(ff).cuda(), torch.tensor(cap).cuda(),
                                 torch.tensor(road).to(torch.uint8).cuda(), objective=objective, rule="eval")
        fz, _, cost_z, rec_z = _run_step(ops, ff, cap, road, f, y, sp, objective, "msa", msa_step=0.0)
        assert np.array_equal(fd.cpu().numpy(), f) and torch.equal(fz, fd)
        assert torch.equal(cost, cost_z) and torch.equal(rec[2:4], rec_z[2:4])
        assert np.allclose(cost.cpu().numpy(), R.bpr(ff, cap, road, f, R.C_OF[objective]), rtol=1e-12, atol=0.0)


# ---- 3. closed form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["all_pairs", "per_origin"])
def test_closed_form_four_roads(ops, method):
    from src.algorithms.equilibrium import assignment_gap, equilibrium_report, solve_assignment
    cf = R.four_road_closed_form()
    graph, ag = _four_roads()
    for solver in ("cfw", "fw"):
        res = {}
        for objective in OBJECTIVES:
            r = res[objective] = solve_assignment(graph, ag, objective=objective, solver=solver, gap_tol=1e-13,
                                                  max_iter=50, method=method)
            fl = r.flow.cpu().tolist()
            print(f"{method} {solver} {objective}: flows {fl} gap {r.relative_gap:.3e} iterations {r.iterations}")
            assert abs(fl[1] - cf[objective][0]) < 1e-6 and abs(fl[2] - cf[objective][1]) < 1e-6
            assert fl[0] == 0.0 and abs(fl[3] - 19.0) < 1e-12          # the B -> D trips load D only
            assert r.relative_gap >= -1e-12 and r.unrouted_volume == 0.0 and r.routed_volume == 19.0
        poa = res["ue"].tstt / res["so"].tstt
        assert abs(poa - cf["tstt_ue"] / cf["tstt_so"]) < 1e-7
        assert res["so"].tstt_lower_bound <= cf["tstt_so"] * (1 + 1e-9)
        assert cf["tstt_so"] <= res["so"].tstt * (1 + 1e-9)
        # the bound also follows from the user-equilibrium flows, through their marginal-cost gap
        lb_ue = assignment_gap(graph, ag, res["ue"].flow, objective="so", method=method).tstt_lower_bound
        assert lb_ue <= cf["tstt_so"] * (1 + 1e-9) and lb_ue <= res["ue"].tstt
    rep = equilibrium_report(graph, ag, gap_tol=1e-13, max_iter=50, method=method)
    assert abs(rep["price_of_anarchy"] - cf["tstt_ue"] / cf["tstt_so"]) < 1e-7
    lo, hi = rep["price_of_anarchy_interval"]
    assert lo <= rep["price_of_anarchy"] <= hi
    assert abs(rep["ue_flows"][1] - cf["ue"][0]) < 1e-6 and abs(rep["so_flows"][1] - cf["so"][0]) < 1e-6
    # 13 trips: the corner equilibrium, nothing on A; the gap may come out a few ulps below zero
    cf13 = R.four_road_closed_form(13)
    assert cf13["ue"] == (0.0, 13.0)
    graph, ag = _four_roads(13)
    r = solve_assignment(graph, ag, objective="ue", solver="cfw", gap_tol=1e-13, max_iter=50, method=method)
    assert r.flow.cpu().tolist() == [0.0, 0.0, 13.0, 17.0]
    assert -1e-12 <= r.relative_gap <= 1e-13 and r.converged


# ---- 4. the solver against the restatement ----------------------------------------------------------------------------------
def test_solver_against_restatement(ops):
    from src.algorithms.equilibrium import assignment_gap, solve_assignment
    graph, ag = _torus(8, 8, 300)
    model = R.Model.from_graph(graph, ag)
    for objective in OBJECTIVES:
        for solver in SOLVERS:
            flows = []
            res = solve_assignment(graph, ag, objective=objective, solver=solver, gap_tol=0.0, max_iter=10,
                                   flow_callback=lambda k, f: flows.append(f.cpu().numpy().copy()))
            trace_r, flows_r = model.solve(objective, solver, 10)
            assert res.iterations == 10 and len(res.trace) == 10 and len(flows) == 10
            for k in range(10):
                (g, lam, al), (gr, lr, ar) = res.trace[k], trace_r[k]
                print(f"{objective} {solver} k={k + 1}: gap {g:.12e} / {gr:.12e}  lambda {lam:.12f} / {lr:.12f}  "
                      f"alpha {al:.9f} / {ar:.9f}")
                assert abs(g - gr) <= 1e-8 and abs(lam - lr) <= 1e-8 and abs(al - ar) <= 1e-6, (objective, solver, k)
                assert np.abs(flows[k] - flows_r[k]).max() <= 1e-8 * flows_r[k].max(), (objective, solver, k)
            assert res.relative_gap == res.trace[-1][0]
    # convergence, the restatement's own count beside the device's
    for objective in OBJECTIVES:
        for solver in ("cfw", "fw"):
            res = solve_assignment(graph, ag, objective=objective, solver=solver, gap_tol=1e-3, max_iter=100)
            count_r = model.iterations_to_gap(objective, solver, 1e-3, 100)
            print(f"{objective} {solver}: gap 1e-3 after {res.iterations} iterations (restatement: {count_r})")
            assert count_r is not None and count_r <= 100
            assert res.converged and res.iterations <= 100 and res.relative_gap <= 1e-3
    # MSA cut off at 20 iterations: not converged, and the gap it reports is the true gap of its flows
    res = solve_assignment(graph, ag, objective="ue", solver="msa", gap_tol=1e-4, max_iter=20)
    trace_r, flows_r = model.solve("ue", "msa", 20)
    assert res.converged is False and res.iterations == 20
    assert res.relative_gap > 1e-4 and abs(res.relative_gap - trace_r[-1][0]) <= 1e-8
    again = assignment_gap(graph, ag, res.flow, objective="ue")
    assert _close(again.relative_gap, res.relative_gap, 1e-12)
    assert _close(model.evaluate(res.flow.cpu().numpy(), "ue")["gap"], res.relative_gap, 1e-9)
    # the host may look at the record every k-th iteration only: the same iterates, a later stop
    a = solve_assignment(graph, ag, solver="cfw", gap_tol=1e-3, max_iter=100, check_every=1)
    b = solve_assignment(graph, ag, solver="cfw", gap_tol=1e-3, max_iter=100, check_every=7)
    assert b.converged and b.iterations % 7 == 0 and b.iterations >= a.iterations      # the gap is not monotone
    n = a.iterations - 1
    assert np.allclose(np.array(b.trace[:n]), np.array(a.trace[:n]), rtol=1e-9, atol=1e-12)   # fp64 atomics reorder


# ---- 5. invariants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,agents", [(12, 9, 1_500), (25, 25, 2_500)])
def test_invariants(ops, W, H, agents):
    from src.algorithms.equilibrium import assignment_gap, equilibrium_report, solve_assignment
    from src.algorithms.user_equilibrium_msa import run_msa
    graph, ag = _torus(W, H, agents)
    model = R.Model.from_graph(graph, ag)
    results = {}
    for objective in OBJECTIVES:
        for solver in SOLVERS:
            flows = []
            res = results[objective, solver] = solve_assignment(
                graph, ag, objective=objective, solver=solver, gap_tol=0.0, max_iter=60,
                flow_callback=lambda k, f: flows.append(f.cpu().numpy().copy()))
            tag = f"{W}x{H} {objective} {solver}"
            gaps = [t[0] for t in res.trace]
            print(f"{tag}: gap {res.relative_gap:.3e} after {res.iterations} iterations, TSTT {res.tstt:.9g}")
            assert len(gaps) == 60 and all(-1e-12 <= g < 1.0 for g in gaps), tag
            assert res.unrouted_volume == 0.0 and res.routed_volume == float(model.od_vol.sum())
            # self-consistent, and equal to the restatement's values on that flow
            again = assignment_gap(graph, ag, res.flow, objective=objective)
            for key in ("tstt", "sptt", "relative_gap"):
                assert _close(getattr(again, key), getattr(res, key), 1e-12), (tag, key)
            ev = model.evaluate(res.flow.cpu().numpy(), objective)
            assert _close(res.tstt, ev["tstt"], 1e-9) and _close(res.sptt, ev["sptt"], 1e-9), tag
            assert _close(res.relative_gap, ev["gap"], 1e-9), tag
            assert _close(res.average_excess_cost, (ev["fc"] - ev["sptt"]) / res.routed_volume, 1e-9), tag
            # an exact line search along a descent direction cannot increase a convex objective
            if solver != "msa":
                obj = [model.beckmann(f) if objective == "ue" else model.tstt(f) for f in flows]
                for k in range(1, len(obj)):
                    assert obj[k] <= obj[k - 1] * (1 + 1e-12), (tag, k, obj[k - 1], obj[k])
    # the rigorous chain, from the SO flows, the UE flows and run_msa's flows alike
    msa = run_msa(graph, ag, max_iter=50)
    msa_flow = torch.tensor([msa[i] for i in range(len(msa))], dtype=torch.float64)
    candidates = [("msa", msa_flow)] + [(f"{o} {s}", r.flow) for (o, s), r in results.items()]
    for name, f in candidates:
        g = assignment_gap(graph, ag, f, objective="so")
        assert g.tstt_lower_bound <= g.tstt, name
        for (o, s), r in results.items():
            if o == "so":
                assert g.tstt_lower_bound <= r.tstt * (1 + 1e-12), (name, s)
    assert _close(assignment_gap(graph, ag, msa).tstt, model.tstt(msa_flow.numpy()), 1e-9)   # the {road: flow} map as is
    rep = equilibrium_report(graph, ag, gap_tol=0.0, max_iter=60)
    lo, hi = rep["price_of_anarchy_interval"]
    assert lo <= rep["price_of_anarchy"] <= hi and math.isfinite(hi)
    assert _close(rep["relative_gap_ue"], results["ue", "cfw"].relative_gap, 1e-6)      # the same solver again


# ---- 6. scale ----------------------------------------------------------------------------------------------------------------
def test_config5_scale(ops):
    from src.algorithms.equilibrium import solve_assignment
    graph, ag = _torus(25, 250, 262_144)
    res = solve_assignment(graph, ag, solver="cfw", gap_tol=0.0, max_iter=3)
    assert res.method == "per_origin" and res.iterations == 3
    vals = [res.tstt, res.sptt, res.relative_gap, res.average_excess_cost] + [v for t in res.trace for v in t]
    assert all(math.isfinite(v) for v in vals) and bool(torch.isfinite(res.flow).all())
    assert 0.0 < res.relative_gap < 1.0 and res.unrouted_volume == 0.0 and res.routed_volume == 262_144.0
    small, ag4 = _torus(25, 25, 2_500)
    assert solve_assignment(small, ag4, max_iter=2, gap_tol=0.0).method == "all_pairs"
    per = solve_assignment(small, ag4, max_iter=2, gap_tol=0.0, method="per_origin")
    assert per.method == "per_origin"
    assert _close(per.relative_gap, solve_assignment(small, ag4, max_iter=2, gap_tol=0.0).relative_gap, 1e-9)


# ---- 7. the runner ----------------------------------------------------------------------------------------------------------
def test_runner_equilibrium_metrics(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, PKG)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main").main
    base = ["--algo", "random", "--mode", "eval", "--scenario", "synthetic-1024-300", "--steps", "10"]
    main(base + ["--equilibrium-metrics", "--output-dir", str(tmp_path / "on")])
    out = capsys.readouterr().out
    assert "Simulation Summary" in out and "Equilibrium Metrics" in out and "Price of Anarchy" in out
    assert out.index("Equilibrium Metrics") > out.index("Simulation Summary")
    assert "skipped" not in out
    doc = json.load(open(tmp_path / "on" / "equilibrium_metrics.json"))
    for key in ("price_of_anarchy", "relative_gap_ue", "relative_gap_so", "tstt_ue", "tstt_so", "tstt_lower_bound",
                "unrouted_volume"):
        assert math.isfinite(doc[key]), key
    lo, hi = doc["price_of_anarchy_interval"]
    assert math.isfinite(hi) and lo <= doc["price_of_anarchy"] <= hi
    assert math.isfinite(doc["msa"]["relative_gap"]) and doc["ue"]["iterations"] >= 1
    rows = open(tmp_path / "on" / "equilibrium_flows.csv").read().splitlines()
    assert rows[0] == "road,ue_flow,so_flow" and len(rows) == 1 + 256
    assert all(math.isfinite(float(v)) for r in rows[1:] for v in r.split(",")[1:])
    assert os.path.exists(tmp_path / "on" / "msa_expected_flows.csv")
    # without the flag: neither file, no new line
    main(base + ["--output-dir", str(tmp_path / "off")])
    out = capsys.readouterr().out
    assert "Simulation Summary" in out and "Equilibrium" not in out and "Anarchy" not in out
    assert os.path.exists(tmp_path / "off" / "msa_expected_flows.csv")
    assert not os.path.exists(tmp_path / "off" / "equilibrium_metrics.json")
    assert not os.path.exists(tmp_path / "off" / "equilibrium_flows.csv")
