"""GPU: the dynamic relative gap — tarl_td_road_times and tarl_td_hindsight against the numpy restatement with == (the crafted
cases, random road times on graphs of 2 to 257 roads, 1 200 searches on one launch, both irregular graphs; two runs bit-identical,
every output entry written, a refused call writes nothing), the free-flow identity, VecEvaluator(dynamic_gap=True) against the
CPU oracle, non-perturbation, dynamic_gap_envs, the domain exit and the CLI end to end."""
import csv
import importlib
import json

import numpy as np
import pytest
import torch

import dynamic_gap_restatement as R
import occupancy_restatement as O

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.crafted_cases()}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plan(edges, N):
    from tarl_hip import ops
    return ops.Plan(torch.from_numpy(np.ascontiguousarray(edges)), N)


def _road_times(veh, fpb, mx, ff, cc, bin_seconds, first_bin, out=None):
    from tarl_hip import ops
    tau, env = ops.td_road_times(_cuda(veh), _cuda(fpb), _cuda(mx), _cuda(ff), _cuda(cc), bin_seconds=bin_seconds,
                                 first_bin=first_bin, out=out)
    return tau, env


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. road times -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 33), (2, 5, 257)])
def test_road_times_equal_the_restatement(shape):
    """Random counts up to and past the capacity; road 0 sits exactly at MAX + 10 in the first bin of every environment (a zero
    denominator) and, where H > 1, the second bin has no frames. == on tau (fp32) and env (fp64), NaN bits included; the
    outputs are sentinel-filled before the call and hold no sentinel after it."""
    K, H, N = shape
    rng = np.random.default_rng(900 + N)
    fpb = rng.integers(1, 40, size=H).astype(np.int32)
    if H > 1:
        fpb[1] = 0
    mx = rng.choice(np.array([2.0, 5.0, 14.0, 129.0], np.float32), size=N)
    ff = (0.7 * rng.integers(1, 90, size=N)).astype(np.float32)
    cc = (ff.astype(np.float64) * (mx + 10.0 - rng.random(N) * 3.0)).astype(np.float32)
    veh = (rng.integers(0, 30, size=(K, H, N)) * np.maximum(fpb, 1)[None, :, None] + rng.integers(0, 3, size=(K, H, N))).astype(np.int32)
    veh[:, 0, 0] = int(mx[0] + 10) * fpb[0]
    want_tau, want_env = R.road_times(veh, fpb, mx, ff, cc, 60, 7)
    assert np.isinf(want_tau[:, 0, 0]).all() and (H == 1 or (want_tau[:, 1, :] == ff[None, :]).all())
    assert (want_tau > ff[None, None, :]).any() or N == 1
    out = (torch.full((K, H, N), -77.0, dtype=torch.float32, device="cuda"),
           torch.full((K, H + 1, N), -77.0, dtype=torch.float64, device="cuda"))
    tau, env = _road_times(veh, fpb, mx, ff, cc, 60, 7, out=out)
    assert tau is out[0] and env is out[1]
    assert _same_bits(tau.cpu().numpy(), want_tau) and _same_bits(env.cpu().numpy(), want_env)
    assert not bool((tau == -77).any()) and not bool((env == -77).any())


# ---- 2. the searches ---------------------------------------------------------------------------------------------------------------
def _hindsight(plan, tau, env, agents, bin_seconds, first_bin, **kw):
    from tarl_hip import ops
    return ops.td_hindsight(plan, tau if torch.is_tensor(tau) else _cuda(tau), env if torch.is_tensor(env) else _cuda(env),
                            agents if torch.is_tensor(agents) else _cuda(agents), bin_seconds=bin_seconds, first_bin=first_bin, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_kernels_on_the_crafted_cases(name):
    c = CASES[name]
    want_tau, want_env, want = R.run_case(c)
    tau, env = _road_times(c["veh"], c["frames_per_bin"], c["max_agents"], c["free_flow"], c["cong"], c["bin_seconds"], c["first_bin"])
    assert _same_bits(tau.cpu().numpy(), want_tau) and _same_bits(env.cpu().numpy(), want_env)
    best = _hindsight(_plan(c["edges"], c["N"]), tau, env, c["agents"], c["bin_seconds"], c["first_bin"]).cpu().numpy()
    assert _same_bits(best, want), (name, best, want)
    if c["want"] is not None:
        assert np.array_equal(best, c["want"])


RANDOM = {"2x1x1": (2, 1, 1, 30, 100), "33x2x3": (33, 2, 3, 60, 7), "257x5x3": (257, 5, 3, 40, 60), "33x5x1": (33, 5, 1, 60, 1),
          "257x1x1": (257, 1, 1, 80, 3600), "32x2x3": (32, 2, 3, 40, 60)}


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_searches_on_random_road_times(name):
    """N = 33 and 257: one road past a bitmap word, more roads than threads; N = 32: the word exactly full. Fractional times
    with +inf, zero and NaN entries; the envelope from the restatement (the kernel under test is the search alone). ==, and a
    second run gives the same bits."""
    N, H, K, A, bs = RANDOM[name]
    seed = 1000 + N + H
    edges, tau = R.random_edges(N, seed), R.random_tau(K, H, N, seed)
    env = R.envelope(tau, bs, 11)
    ag = R.random_agents(K, A, N, H, bs, 11, seed)
    want = R.hindsight(edges, N, tau, env, ag, bs, 11)
    plan = _plan(edges, N)
    best = _hindsight(plan, tau, env, ag, bs, 11).cpu().numpy()
    fin = np.isfinite(want)
    print(f"[{name}] {int((ag[:, 1:, R.DONE] == 1).sum())} searches, {int(fin.sum())} finite, {int(np.isnan(tau).sum())} NaN and "
          f"{int(np.isinf(tau).sum())} inf road times")
    assert _same_bits(best, want), (name, np.argwhere(best != want)[:5])
    assert fin.any() and (N == 2 or (~fin[:, 1:] & (ag[:, 1:, R.DONE] == 1)).any())
    assert np.isinf(best[:, 0]).all() and (A <= 4 or np.isinf(best[:, 2:4]).all())          # the dummy, the foreign ids
    assert _same_bits(_hindsight(plan, tau, env, ag, bs, 11).cpu().numpy(), best)


def test_more_searches_than_workgroups():
    """K A = 3 x 400 = 1 200 searches on the 21-road graph: more than the 1 024 workgroups of one launch, so the grid stride
    runs; every workgroup reuses its label row."""
    net = O.small_graph()
    N, K, A, H, bs = net.num_roads, 3, 400, 5, 60
    edges = net.edge_index.numpy()
    tau = R.random_tau(K, H, N, 77)
    env = R.envelope(tau, bs, 11)
    ag = R.random_agents(K, A, N, H, bs, 11, 77)
    want = R.hindsight(edges, N, tau, env, ag, bs, 11)
    out = torch.full((K, A), -77.0, dtype=torch.float64, device="cuda")
    best = _hindsight(_plan(edges, N), tau, env, ag, bs, 11, out=out)
    assert best is out and _same_bits(best.cpu().numpy(), want) and int(np.isfinite(want).sum()) > 600


@pytest.mark.parametrize("graph", ["MIXED", "HUB126"])
def test_searches_on_the_irregular_graphs(graph):
    """Degrees up to 126 in and out, dead ends, an unsorted edge list."""
    import irregular_graphs as ig
    net = ig.graph(graph)
    N, K, A, H, bs = net.num_roads, 2, 60, 2, 100
    edges = net.edge_index.numpy()
    din, dout = ig.degrees(net)
    assert int(dout.min()) == 0 and (graph != "HUB126" or int(din.max()) == 126 == int(dout.max()))
    tau = R.random_tau(K, H, N, 55)
    env = R.envelope(tau, bs, 11)
    ag = R.random_agents(K, A, N, H, bs, 11, 55)
    want = R.hindsight(edges, N, tau, env, ag, bs, 11)
    best = _hindsight(_plan(edges, N), tau, env, ag, bs, 11).cpu().numpy()
    assert _same_bits(best, want) and np.isfinite(want).sum() > 20


def test_every_output_entry_is_written_and_a_refused_call_writes_nothing():
    from tarl_hip import lib, ops
    c = CASES["master"]
    K, A, H, N = c["K"], c["agents"].shape[1], c["H"], c["N"]
    plan = _plan(c["edges"], N)
    _, _, want = R.run_case(c)
    tau, env = _road_times(c["veh"], c["frames_per_bin"], c["max_agents"], c["free_flow"], c["cong"], c["bin_seconds"], c["first_bin"])
    out = torch.full((K, A), -77.0, dtype=torch.float64, device="cuda")
    ag = _cuda(c["agents"])
    _hindsight(plan, tau, env, ag, 100, 2, out=out)
    assert _same_bits(out.cpu().numpy(), want)                       # no entry kept the sentinel
    out.fill_(-77.0)
    t_out = (torch.full_like(tau, -77.0), torch.full_like(env, -77.0))
    for kw, msg in ((dict(bin_seconds=0, first_bin=2), "bin_seconds"), (dict(bin_seconds=100, first_bin=-1), "first_bin")):
        with pytest.raises(ValueError, match=msg):
            ops.td_hindsight(plan, tau, env, ag, out=out, **kw)
        with pytest.raises(ValueError, match=msg):
            ops.td_road_times(_cuda(c["veh"]), _cuda(c["frames_per_bin"]), _cuda(c["max_agents"]), _cuda(c["free_flow"]),
                              _cuda(c["cong"]), out=t_out, **kw)
    L = lib.load()
    small = torch.empty(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.TarlError, match="scratch too small"):
        ops.td_hindsight(plan, tau, env, ag, out=out, scratch=small, bin_seconds=100, first_bin=2)
    head = (plan.handle, tau.data_ptr(), env.data_ptr(), ag.data_ptr())
    scratch = torch.empty(ops.td_hindsight_bytes(plan, K, A), dtype=torch.uint8, device="cuda")
    tail = (scratch.data_ptr(), scratch.numel(), out.data_ptr(), lib.current_stream())
    for mid, msg in (((K, A, 9 * A - 1, 100, 2, H), b"overlap"), ((0, A, 9 * A, 100, 2, H), b"bad sizes"),
                     ((K, A, 9 * A, 100, 2, 0), b"H must be"), ((K, A, 9 * A, 0, 2, H), b"bin_seconds")):
        assert L.tarl_td_hindsight(*head, *mid, *tail) == -1 and msg in L.tarl_last_error()
    v = [_cuda(c[k]).data_ptr() for k in ("veh", "frames_per_bin", "max_agents", "free_flow", "cong")]
    assert L.tarl_td_road_times(*v, K, 0, N, 100, 2, t_out[0].data_ptr(), t_out[1].data_ptr(), lib.current_stream()) == -1
    assert L.tarl_td_road_times(*v, K, H, N, 100, -1, t_out[0].data_ptr(), t_out[1].data_ptr(), lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == -77).all()) and bool((t_out[0] == -77).all()) and bool((t_out[1] == -77).all())


# ---- 3. the evaluator ----------------------------------------------------------------------------------------------------------------
BIN = 100
EMB_SEED = 32       # the configuration of test_gpu_trips.test_trips_replayed_by_the_oracle, whose MODE runs deliver trips


def _torus():
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(EMB_SEED))
    _, action, succ = O.oracle_mode(net, emb)
    return net, action, O.deliverable_population(net, succ), emb


def _evaluator(net, pop, K, emb, seed=3, **kw):
    from tarl_hip.evaluator import VecEvaluator
    return VecEvaluator(O.engine_of(net, pop, K, seed), "embedding", emb=emb.cuda(), **kw)


def test_free_flow_identity():
    """tau = FF in one bin: the hindsight time of every trip is the free-flow time of trip_free_flow_times under the weights
    w(u -> v) = FF[v]. The search adds the road times from the origin outwards onto the departure clock, the reverse tree
    from the destination backwards: the two differ by rounding alone, within A 2^-52 max ht (A: the rows of the table)."""
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import trip_free_flow_times
    net, _, pop, _ = _torus()
    eng = O.engine_of(net, pop, 1)
    N, A = net.num_roads, pop.size(0)
    ffr = net.x[:, 3 * net.Nmax + 2].clone()
    ff_w = ffr[net.edge_index[1]].cuda()
    want = trip_free_flow_times(eng, ff_w).cpu().numpy()
    first = EPISODE_START // 3600
    tau, env = _road_times(np.zeros((1, 1, N), np.int32), np.ones(1, np.int32), np.full(N, 5, np.float32), ffr.numpy(),
                           np.zeros(N, np.float32), 3600, first)
    assert torch.equal(tau[0, 0].cpu(), ffr)
    ag = eng.agents.clone()
    ag[:, 1:, 8] = 1.0
    best = _hindsight(eng.plan, tau, env, ag, 3600, first).cpu().numpy()
    ht = best[0] - ag[0, :, 2].double().cpu().numpy()
    assert np.isinf(ht[0]) and np.isinf(want[0]) and np.isfinite(ht[1:]).all()
    err = np.abs(ht[1:] - want[1:]).max()
    bound = A * 2.0 ** -52 * ht[1:].max()
    print(f"[free flow] largest difference {err:.3e}, bound {bound:.3e}, largest ht {ht[1:].max():.3f}")
    assert err <= bound


def _oracle_replay(net, action, pop, eng, noise0, K, T):
    """Every environment frame by frame with oracle.sim.env_step under the exported Gumbel values -> (agent tables (K, A, 9),
    veh int32 (K, H, N): the counts after every frame summed per bin, frames per bin, first_bin)."""
    from oracle import sim
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    N, Nmax = net.num_roads, net.Nmax
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    first = EPISODE_START // BIN
    H = (EPISODE_START + T - 1) // BIN - first + 1
    veh, tables = np.zeros((K, H, N), np.int32), []
    for b in range(K):
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pop.clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        for t in range(T):
            g = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
            sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, float(EPISODE_START + t), Nmax, gumbel=g,
                         congestion_constant=net.congestion_constant)
            veh[b, (EPISODE_START + t) // BIN - first] += x[:, c.N].numpy().astype(np.int32)
        assert torch.equal(ag, eng.agents[b].cpu()), f"agent table of environment {b}"
        tables.append(ag.numpy())
    fpb = np.bincount((EPISODE_START + np.arange(T)) // BIN - first, minlength=H).astype(np.int32)
    return np.stack(tables), veh, fpb, first


def test_dynamic_gap_replayed_by_the_oracle():
    """The 8 x 8 torus of test_gpu_trips (128 agents, every other one bound three MODE steps from its origin, embedding seed
    32, engine seed 3), K = 2, T = 300, bins of 100 s from bin 215. Checked beforehand on the CPU oracle under torch's own noise
    (noise seeds 0 - 5, two environments each): 52 - 56 usable trips, 34 - 40 of them with g > 0 and 12 - 21 with g < 0, and 5 - 6
    trips whose free-flow path, travelled under the run's road times, arrives later than the hindsight path; the largest road
    time is 2.1 times the free-flow time and no road reaches a zero denominator. oracle.sim.env_step replays every
    environment with the exported Gumbel values; the restatement applied to the oracle's counts and agent tables must equal
    res.dynamic_gap: == on best (every value is the same chain of fp64 operations), == on the counts, minima and maxima, and
    within 2 n 2^-53 sum |x| on the fp64 sums (an n-term sum in any order is within (n - 1) 2^-53 sum |x| of the exact one;
    torch and numpy each choose their own). Conditions on the run, from the oracle's own tables: at least 20 usable trips,
    one with g > 0, one whose hindsight path differs from its free-flow path; the test prints the counts."""
    from tarl_hip.evaluator import dynamic_gap_report
    net, action, pop, emb = _torus()
    N, K, T = net.num_roads, 2, 300
    ev = _evaluator(net, pop, K, emb, dynamic_gap=True, link_bin_seconds=BIN)
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T and res.occupancy is None and res.trips is None
    tables, veh, fpb, first = _oracle_replay(net, action, pop, eng, noise0, K, T)
    H = veh.shape[1]
    dg = res.dynamic_gap
    meta = dg["meta"]
    assert (meta["envs"], meta["first_bin"], meta["bin_seconds"], meta["frames_per_bin"]) == (K, first, BIN, fpb.tolist()) and first == 215
    assert np.array_equal(ev.occ_acc["veh"].cpu().numpy(), veh)
    c3 = 3 * net.Nmax
    tau, env = R.road_times(veh, fpb, net.x[:, c3].numpy(), net.x[:, c3 + 2].numpy(), net.congestion_constant.numpy(), BIN, first)
    edges = net.edge_index.numpy()
    want = R.hindsight(edges, N, tau, env, tables, BIN, first)
    assert _same_bits(dg["best"], want)
    tt, ht, g, use = R.gap(tables, want)
    outs = R.out_lists(edges, N)
    tau_ff = np.broadcast_to(net.x[:, c3 + 2].numpy()[None, None, :], (K, 1, N)).copy()
    env_ff = R.envelope(tau_ff, BIN, first)
    differ = 0
    for k in range(K):
        for a in np.nonzero(use[k])[0]:
            o, d, t0 = int(tables[k, a, 0]), int(tables[k, a, 1]), float(tables[k, a, 2])
            _, path = R.hindsight_path(outs, tau_ff[k], env_ff[k], o, d, t0, BIN, first)
            differ += R.along(path, tau[k], env[k], t0, BIN, first) > want[k, a]
    print(f"[dynamic gap replay] usable trips {int(use.sum())} ({use.sum(axis=1).tolist()} per environment), g > 0: "
          f"{int((g[use] > 0).sum())}, g < 0: {int((g[use] < 0).sum())}, hindsight path quicker than the free-flow path: {differ}, "
          f"largest tau / FF {float(np.max(tau / tau_ff)):.2f}, searches {meta['searches']}")
    assert int(use.sum()) >= 20 and int((g[use] > 0).sum()) >= 1 and differ >= 1
    dep_bin = np.array([R.clock_bin(t, BIN, first, H) for t in tables[0, :, R.DEP]])
    pa, pe, pb = R.reductions(tables, want, dep_bin, H)
    u = 2.0 ** -53
    z = np.where(use, g, 0.0)
    bounds = {("per_agent", "g_sum"): 2 * K * u * np.abs(z).sum(axis=0), ("per_agent", "g_sumsq"): 2 * K * u * (z * z).sum(axis=0),
              ("per_env", "tt_sum"): 2 * use.sum(axis=1) * u * np.where(use, tt, 0.0).sum(axis=1),
              ("per_env", "ht_sum"): 2 * use.sum(axis=1) * u * np.where(use, np.abs(np.where(use, ht, 0.0)), 0.0).sum(axis=1),
              ("per_bin", "g_sum"): 2 * use.sum(axis=1)[:, None] * u * np.abs(z).sum(axis=1)[:, None] * np.ones((1, H))}
    for part, wants in (("per_agent", pa), ("per_env", pe), ("per_bin", pb)):
        assert set(dg[part]) == set(wants)
        for key, w in wants.items():
            got = dg[part][key]
            assert got.shape == w.shape, (part, key)
            if (part, key) in bounds:
                assert (np.abs(got - w) <= bounds[(part, key)]).all(), (part, key, np.abs(got - w).max())
            else:
                assert np.array_equal(got, w), (part, key)
    assert meta["searches"] == int((tables[:, 1:, R.DONE] == 1).sum()) == sum(res.arrived)
    rep = dynamic_gap_report(res)
    rg = R.relative_gaps(pe)
    assert rep["available"] and rep["summary"]["trips"] == int(use.sum()) and rep["bins"] == ["bin215", "bin216", "bin217", "bin218"]
    assert all(abs(x - y) <= 1e-12 for x, y in zip(rep["summary"]["relative_gap_per_env"], rg))


@pytest.mark.parametrize("head", ["embedding", "dijkstra"])
def test_the_dynamic_gap_does_not_perturb_the_run(head):
    from tarl_hip.evaluator import PER_ENV_KEYS, VecEvaluator
    net, _, pop, emb = _torus()
    runs = []
    for flag in (False, True):
        kw = dict(dynamic_gap=True, link_bin_seconds=BIN) if flag else {}
        if head == "embedding":
            ev = _evaluator(net, pop, 4, emb, **kw)
        else:
            ev = VecEvaluator(O.engine_of(net, pop, 4), "dijkstra", **kw)
        runs.append((ev, ev.run(200)))
    (e0, r0), (e1, r1) = runs
    assert not r0.domain_exit and not r1.domain_exit and r0.frames_run == r1.frames_run == 200
    for k in PER_ENV_KEYS:
        assert getattr(r0, k) == getattr(r1, k), k
    assert r0 == r1 and r0.aggregate == r1.aggregate and r0.settings == r1.settings
    assert torch.equal(e0.reward[:200], e1.reward[:200]) and float(e0.reward.abs().sum()) > 0
    assert torch.equal(e0.eng.x, e1.eng.x) and torch.equal(e0.eng.agents, e1.eng.agents)
    assert r0.dynamic_gap is None and not hasattr(e0, "occ_ring") and not hasattr(e0, "_gap_buf")
    assert r1.dynamic_gap["best"].shape == (4, pop.size(0)) and r1.occupancy is None and r1.occupancy_stats is None
    assert r1.dynamic_gap["meta"]["searches"] == sum(r1.arrived)
    assert "dynamic_gap" not in r1.to_dict(per_env=True)        # the arrays never enter the JSON document


def test_dynamic_gap_envs_and_refusals():
    """dynamic_gap_envs = 1 of 2: the first environment of the full run, bit for bit; the occupancy report is still there when
    it is asked for; bad values are refused."""
    net, _, pop, emb = _torus()
    full = _evaluator(net, pop, 2, emb, dynamic_gap=True, link_bin_seconds=BIN).run(300)
    part = _evaluator(net, pop, 2, emb, dynamic_gap=True, dynamic_gap_envs=1, occupancy=True, link_bin_seconds=BIN).run(300)
    f, p = full.dynamic_gap, part.dynamic_gap
    assert p["meta"]["envs"] == 1 and p["best"].shape == (1, pop.size(0)) and _same_bits(p["best"], f["best"][:1])
    assert part.occupancy is not None and part.occupancy["veh"].shape[0] == 2
    for key in ("tt_sum", "ht_sum", "n", "n_neg", "n_nonpos"):
        assert np.array_equal(p["per_env"][key], f["per_env"][key][:1]), key
    assert np.array_equal(p["per_bin"]["n"], f["per_bin"]["n"][:1]) and int(p["per_env"]["n"][0]) > 0
    for bad in (0, 3):
        with pytest.raises(ValueError, match="dynamic_gap_envs"):
            _evaluator(net, pop, 2, emb, dynamic_gap=True, dynamic_gap_envs=bad)
    with pytest.raises(ValueError, match="dynamic_gap=True"):
        _evaluator(net, pop, 2, emb, dynamic_gap_envs=1)
    tables = pop.unsqueeze(0).repeat(2, 1, 1)
    tables[1, 5, 2] += 1.0
    with pytest.raises(ValueError, match="same population"):
        _evaluator(net, tables, 2, emb, dynamic_gap=True).run(8)
    with pytest.raises(ValueError, match="TRIP_MAX_BINS"):
        _evaluator(net, pop, 2, emb, dynamic_gap=True, link_bin_seconds=1).run(5000)


def test_a_domain_exit_carries_no_dynamic_gap():
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import dynamic_gap_report
    net = synth.torus_network(8, 8)
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    ev, _ = O.embedding_evaluator(net, pop, 2, dynamic_gap=True)
    res = ev.run(256)
    assert res.domain_exit and res.aggregate is None and res.dynamic_gap is None and res.occupancy is None
    assert not dynamic_gap_report(res)["available"]
    ev.eng.reset()
    ev.eng.check_flags()
    again = ev.run(8, deterministic=False)
    assert not again.domain_exit and again.dynamic_gap["best"].shape == (2, 1025) and again.dynamic_gap["meta"]["first_bin"] == 5


# ---- 4. CLI end to end ---------------------------------------------------------------------------------------------------------------
STEPS = 1800      # the untrained MODE policy delivers nobody in the first 600 frames (test_gpu_trips): 8 trips by frame 1 800


def test_cli_dynamic_gap_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-300"
    on = tmp_path / "on"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--eval-baseline", "dijkstra", "--steps",
          str(STEPS), "--eval-dynamic-gap", "--eval-dynamic-gap-envs", "3", "--output-dir", str(on)])
    text = capsys.readouterr().out
    assert "=== Dynamic gap ===" in text and "=== Occupancy ===" not in text and "=== Trips ===" not in text
    block = text[text.index("=== Dynamic gap ==="):]
    assert "definition:" in block and "hindsight searches over 3 environments" in block and "By departure time" in block
    assert "=== Dynamic gap: baseline (dijkstra) ===" in block and "(paired) ===" in block
    assert block.index("=== Dynamic gap: baseline") < block.index("(paired) ===") < block.index("policy - dijkstra:")
    assert block.count("hindsight searches over 3 environments") == 2 and block.count("policy - dijkstra:") == 1
    doc = json.load(open(on / "eval_envs.json"))
    assert not doc["mode"]["domain_exit"], "the synthetic scenario left the domain under MODE"
    dg = doc["dynamic_gap"]
    rows = list(csv.DictReader(open(on / "eval_dynamic_gap.csv")))
    assert dg["available"] and "rows" not in dg and "by_departure" not in dg and dg["columns"] == list(rows[0])
    assert len(rows) == 300 and [int(r["agent"]) for r in rows] == list(range(1, 301))
    s = dg["summary"]
    print(f"[cli] {STEPS} frames: {s['searches']} searches, {s['trips']} usable trips, relative gap {s['relative_gap']['mean']}, "
          f"paired {s['paired']}")
    assert s["envs"] == 3 and s["frames_run"] == STEPS and s["trips"] == sum(int(r["envs_usable"]) for r in rows) > 0
    assert len(s["relative_gap_per_env"]) == 3 and s["relative_gap"]["n"] + s["relative_gap"]["missing"] == 3
    assert s["paired"]["baseline_head"] == "dijkstra" and s["paired"]["available"]
    by = list(csv.DictReader(open(on / "eval_dynamic_gap_by_departure.csv")))
    assert list(by[0]) == dg["by_departure_columns"] and [r["bin"] for r in by] == dg["bins"] == ["5h", "6h"]
    base_rows = list(csv.DictReader(open(on / "eval_dynamic_gap_baseline.csv")))
    assert len(base_rows) == 300 and dg["baseline"]["available"] and dg["baseline"]["head"] == "dijkstra"
    assert dg["baseline"]["summary"]["relative_gap"] == s["paired"]["baseline_relative_gap"]
    assert len(json.dumps(dg)) < 20000 and "dynamic_gap" not in doc["mode"] and "occupancy" not in doc
    assert set(doc) == {"mode", "baseline", "paired", "dynamic_gap"}
    # without the flag: none of it
    off = tmp_path / "off"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--steps", "60", "--output-dir", str(off)])
    assert "Dynamic gap" not in capsys.readouterr().out
    assert not (off / "eval_dynamic_gap.csv").exists() and set(json.load(open(off / "eval_envs.json"))) == {"mode"}
    # the router alone
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--mode", "eval", "--scenario", scenario, "--dijkstra-envs", "4", "--eval-dynamic-gap", "--steps", "60",
          "--output-dir", str(dj)])
    out = capsys.readouterr().out
    assert "=== Dynamic gap ===" in out and "policy - dijkstra" not in out
    assert len(list(csv.DictReader(open(dj / "dijkstra_dynamic_gap.csv")))) == 300
    assert (dj / "dijkstra_dynamic_gap_by_departure.csv").exists()
    assert json.load(open(dj / "dijkstra_envs.json"))["dynamic_gap"]["summary"]["envs"] == 4
