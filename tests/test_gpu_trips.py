"""GPU: the per-trip report — tarl_trip_agent_stats and tarl_trip_bin_stats against the numpy restatement (== on every array
of the integer-valued cases, the n-term bound on the fractional one, two runs bit-identical), VecEvaluator(trips=True) against
the CPU oracle, its identities with the episode summary, non-perturbation, the paired launch, the refusals and the CLI end to
end."""
import csv
import importlib
import json

import numpy as np
import pytest
import torch

import occupancy_restatement as O
import trips_restatement as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.crafted_cases()}
FP64 = ("tt_sum", "tt_sumsq", "d_sum", "d_sumsq", "dep_tt", "dep_ff")


# ---- 1. both kernels on the crafted cases ------------------------------------------------------------------------------------------
def _tables(t, pad):
    """(K, A, 9) on the device, environment k at k * (9 A + pad) floats: the gap holds NaN, which must never be read."""
    K, A, _ = t.shape
    buf = torch.full((K, 9 * A + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :9 * A] = torch.from_numpy(t).cuda().reshape(K, 9 * A)
    v = buf[:, :9 * A].unflatten(1, (A, 9))
    assert v.data_ptr() == buf.data_ptr() and v.stride() == (9 * A + pad, 9, 1)
    return v


def _device(case, paired=True, with_ff=True, pad=None, out=None):
    from tarl_hip import ops
    pad = case["pad"] if pad is None else pad
    ag = _tables(case["agents"], pad)
    base = _tables(case["agents_b"], pad) if paired else None
    ff = torch.from_numpy(case["ff"]).cuda() if with_ff else None
    pa = ops.trip_agent_stats(ag, base, free_flow=ff, out=None if out is None else out[0])
    pb = ops.trip_bin_stats(ag, bin_seconds=case["bin_seconds"], first_bin=case["first_bin"], num_bins=case["H"], free_flow=ff,
                            out=None if out is None else out[1])
    return {k: v.cpu().numpy() for k, v in pa.items()}, {k: v.cpu().numpy() for k, v in pb.items()}


def _assert_case(case, got, want):
    bounds = R.sum_bounds(case["agents"], case["agents_b"], case["ff"], case["bin_seconds"], case["first_bin"], case["H"])
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, k
            if case["exact"] or k not in FP64:
                assert np.array_equal(g[k], w[k]), (case["name"], k)
            else:       # n * 2^-53 * sum |x|, the worst case of an n-term fp64 sum: no free tolerance
                err = np.abs(g[k] - w[k])
                print(f"[{case['name']}] {k}: largest difference {err.max():.3e}, its bound {bounds[k].flat[err.argmax()]:.3e}")
                assert (err <= bounds[k]).all(), (case["name"], k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_kernels_equal_the_restatement(name):
    case = CASES[name]
    want = R.run_case(case)
    got = _device(case)
    _assert_case(case, got, want)
    again = _device(case)                       # bit-identical from run to run, the fp64 sums included
    for g, a in zip(got, again):
        assert all(np.array_equal(g[k].view(np.uint8), a[k].view(np.uint8)) for k in g), name
    assert all(v[0] == 0 for v in got[0].values())          # entry 0, the dummy, is written as zero
    assert int(want[0]["n_done"].sum()) > 0 and int(want[1]["arr"].sum()) == int(want[0]["n_done"].sum())


def test_results_do_not_depend_on_the_table_stride():
    """a_bstride = 9 A + 5 (the crafted case), 9 A and 9 A + 64 give the same bits, also where the fp64 sums round."""
    for name in ("stride-5x70", "fractional-33x200"):
        case = CASES[name]
        runs = [_device(case, pad=pad) for pad in (5, 0, 64)]
        _assert_case(case, runs[0], R.run_case(case))
        for other in runs[1:]:
            for g, o in zip(runs[0], other):
                assert all(np.array_equal(g[k].view(np.uint8), o[k].view(np.uint8)) for k in g), name


def test_optional_inputs_only_add_outputs():
    """Without agents_b there are no paired outputs, without free_flow no n_under / dep_ff / dep_ff_n; the others are what
    they are with them."""
    case = CASES["130x300"]
    full = _device(case)
    bare = _device(case, paired=False, with_ff=False)
    assert set(bare[0]) == set(R.AGENT_KEYS) and set(bare[1]) == set(R.BIN_KEYS)
    assert set(full[0]) == set(R.AGENT_KEYS + R.PAIR_KEYS + ("n_under",)) and set(full[1]) == set(R.BIN_KEYS + R.FF_KEYS)
    for b, f in zip(bare, full):
        assert all(np.array_equal(b[k], f[k]) for k in b)


def test_every_output_entry_is_written_and_a_refused_call_writes_nothing():
    from tarl_hip import lib, ops
    case = CASES["65x1025"]
    K, A, H = case["K"], case["A"], case["H"]
    spec_a = dict(ops._TRIP_AGENT_SPEC + ops._TRIP_PAIR_SPEC + (("n_under", torch.int32),))
    spec_b = dict(ops._TRIP_BIN_SPEC + ops._TRIP_FF_SPEC)

    def filled():
        return ({k: torch.full((A,), -77, dtype=dt, device="cuda") for k, dt in spec_a.items()},
                {k: torch.full((K, H), -77, dtype=dt, device="cuda") for k, dt in spec_b.items()})
    out = filled()
    got = _device(case, out=out)
    _assert_case(case, got, R.run_case(case))                   # == the restatement: no entry kept the sentinel ...
    for d in out:
        for k, v in d.items():
            assert np.array_equal(v.cpu().numpy(), (got[0] if k in got[0] else got[1])[k]), k      # ... in the caller's tensors
    assert all(float(v[0]) == 0 for v in out[0].values())
    # refusals: the wrapper raises and the entry point returns -1; the sentinel stays everywhere
    out = filled()
    ag = _tables(case["agents"], 0)
    ff = torch.from_numpy(case["ff"]).cuda()
    order = ops.trip_departure_order(ag[0, :, 2], bin_seconds=100, first_bin=200, num_bins=H)
    for kw, msg in ((dict(bin_seconds=100, first_bin=200, num_bins=ops.TRIP_MAX_BINS + 1), "num_bins"),
                    (dict(bin_seconds=0, first_bin=200, num_bins=H), "bin_seconds"),
                    (dict(bin_seconds=100, first_bin=-1, num_bins=H), "first_bin")):
        with pytest.raises(ValueError, match=msg):
            ops.trip_bin_stats(ag, free_flow=ff, out=out[1], **kw)
    L = lib.load()
    ptrs = [out[1][k].data_ptr() for k, _ in ops._TRIP_BIN_SPEC + ops._TRIP_FF_SPEC]
    head = (ag.data_ptr(), K, A, ag.stride(0), order[0].data_ptr(), order[1].data_ptr(), ff.data_ptr())
    for bins, msg in (((100, 200, ops.TRIP_MAX_BINS + 1), b"H must be"), ((0, 200, H), b"bin_seconds"), ((100, -1, H), b"first_bin"),
                      ((100, 200, 0), b"H must be")):
        assert L.tarl_trip_bin_stats(*head, *bins, *ptrs, lib.current_stream()) == -1 and msg in L.tarl_last_error()
    pa = [out[0][k].data_ptr() for k in ("n_under",) + tuple(k for k, _ in ops._TRIP_AGENT_SPEC + ops._TRIP_PAIR_SPEC)]
    assert L.tarl_trip_agent_stats(ag.data_ptr(), ag.data_ptr(), ff.data_ptr(), K, A, 9 * A - 1, 9 * A, *pa,
                                   lib.current_stream()) == -1 and b"overlap" in L.tarl_last_error()
    assert L.tarl_trip_agent_stats(ag.data_ptr(), None, ff.data_ptr(), 0, A, 9 * A, 0, *pa, lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((v == -77).all()) for d in out for v in d.values())


# ---- 2. the evaluator against the CPU oracle ---------------------------------------------------------------------------------------
BIN = 100
EMB_SEED = 32       # picked on the CPU oracle: see test_trips_replayed_by_the_oracle


def _torus():
    """The 8 x 8 torus, the MODE action of the embedding of seed EMB_SEED and the population whose every other agent is bound
    three MODE steps from its origin -> (net, action, population, embedding)."""
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(EMB_SEED))
    _, action, succ = O.oracle_mode(net, emb)
    return net, action, O.deliverable_population(net, succ), emb


def _evaluator(net, pop, K, emb, seed=3, **kw):
    from tarl_hip.evaluator import VecEvaluator
    return VecEvaluator(O.engine_of(net, pop, K, seed), "embedding", emb=emb.cuda(), **kw)


def _free_flow_weights(net):
    return net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].clone()


def _host_free_flow(net, pop):
    """Free-flow time per agent by Floyd-Warshall in float64 on the host: FREE_FLOW of the origin road plus the cheapest sum
    of the FREE_FLOW of the roads that follow, +inf where there is no path; row 0 (the dummy) +inf."""
    N = net.num_roads
    own = net.x[:, 3 * net.Nmax + 2].double().numpy()
    d = np.full((N, N), np.inf)
    np.fill_diagonal(d, 0.0)
    src, dst = net.edge_index.numpy()
    np.minimum.at(d, (src, dst), own[dst])
    for k in range(N):
        d = np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :])
    o, t = pop[:, 0].long().numpy(), pop[:, 1].long().numpy()
    ff = own[o] + d[o, t]
    ff[0] = np.inf
    return ff


def test_trips_replayed_by_the_oracle():
    """The 8 x 8 torus recipe of test_occupancy_replayed_by_the_oracle (128 agents departing in the first 200 s, every other
    one bound three MODE steps from its origin, engine seed 3), K = 2, T = 300, bins of 100 s: the clock starts at 21 540, so
    the stored bins are 215 .. 218. The embedding seed is 32, not that test's 0: under seed 0 the MODE cycles jam and only 11 -
    12 agents arrive in both environments however long the run (CPU oracle, T = 300 .. 900), below the guard of 20. Seed 32 was
    picked on the CPU oracle under torch's own noise (noise seeds 0 - 5, two environments each): 24 - 26 agents arrive in both
    environments and 3 - 6 in one, 199 - 203 (agent, environment) pairs are on the way at the end, arrived agents by departure
    bin 19 - 21 / 30 - 31 / 4 - 5 / 0, arrivals by bin 0 / 18 - 21 / 32 - 35 / 1 - 2, largest count 13 of Nmax 15. oracle.sim.env_step replays every environment with the exported
    Gumbel values; the restatement applied to the oracle's two final agent tables must equal res.trips and res.trip_bins with
    == (the times are whole seconds, so every summation order gives the same fp64 value). Guards, from the oracle's own tables:
    at least 20 agents arrived in both environments, at least one is on the way at the end, at least two departure bins and
    two arrival bins are non-empty; the test prints the numbers. The identities with the episode summary are checked on the
    same run, and the free-flow times against a Floyd-Warshall pass on the host."""
    from oracle import sim
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import trip_report
    net, action, pop, emb = _torus()
    N, Nmax, K, T = net.num_roads, net.Nmax, 2, 300
    ev = _evaluator(net, pop, K, emb, trips=True, link_bin_seconds=BIN, trip_free_flow=_free_flow_weights(net).cuda())
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    assert res.trip_meta["first_bin"] == EPISODE_START // BIN == 215 and res.trip_meta["bin_seconds"] == BIN
    assert not res.trip_meta["paired"] and "n_both" not in res.trips
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    tables = []
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
        assert torch.equal(ag, eng.agents[b].cpu()), f"agent table of environment {b}"
        tables.append(ag.numpy())
    tables = np.stack(tables)
    ff = _host_free_flow(net, pop)
    got_ff = res.trip_meta["free_flow"]
    assert got_ff.shape == ff.shape and np.array_equal(np.isinf(got_ff), np.isinf(ff)) and np.isinf(got_ff[0])
    assert np.allclose(got_ff[1:], ff[1:], rtol=1e-12, atol=0) and np.isfinite(ff[1:]).all()
    want_a = R.agent_stats(tables, None, got_ff)
    want_b = R.bin_stats(tables, BIN, 215, 4, got_ff)
    both = int((want_a["n_done"][1:] == K).sum())
    print(f"[trips replay] arrived in both environments {both}, trips {int(want_a['n_done'].sum())}, on the way "
          f"{want_a['n_way'].sum()}, departures by bin {want_b['dep_done'].sum(axis=0).tolist()} (+ on the way "
          f"{want_b['dep_way'].sum(axis=0).tolist()}), arrivals by bin {want_b['arr'].sum(axis=0).tolist()}, trips below free flow "
          f"{int(want_a['n_under'].sum())}")
    assert both >= 20 and int(want_a["n_way"].sum()) >= 1
    assert int((want_b["dep_done"].sum(axis=0) > 0).sum()) >= 2 and int((want_b["arr"].sum(axis=0) > 0).sum()) >= 2
    assert set(res.trips) == set(want_a) and set(res.trip_bins) == set(want_b)
    for k, w in want_a.items():
        assert res.trips[k].dtype == w.dtype and np.array_equal(res.trips[k], w), k
    for k, w in want_b.items():
        assert res.trip_bins[k].dtype == w.dtype and np.array_equal(res.trip_bins[k], w), k
    # identities with the episode summary of the same run
    assert int(res.trips["n_done"].sum()) == sum(res.arrived)
    for b in range(K):
        assert int(res.trip_bins["dep_done"][b].sum()) == int(res.trip_bins["arr"][b].sum()) == res.arrived[b]
        assert int(res.trip_bins["dep_way"][b].sum()) == res.on_way[b]
    assert float(res.trips["tt_sum"].sum()) == float(ev.summary["sums"][:, 0].sum())          # whole seconds: ==
    assert float(res.trip_bins["dep_tt"].sum()) == float(ev.summary["sums"][:, 0].sum())
    rep = trip_report(res)
    assert rep["available"] and len(rep["rows"]) == pop.size(0) - 1 and rep["summary"]["trips"] == sum(res.arrived)
    assert rep["bins"] == ["bin215", "bin216", "bin217", "bin218"] and rep["summary"]["arrived_in_every"] == both


# ---- 3. reducing the trips does not perturb the run --------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["embedding", "dijkstra"])
def test_reducing_the_trips_does_not_perturb_the_run(head):
    from tarl_hip.evaluator import PER_ENV_KEYS, VecEvaluator
    net, _, pop, emb = _torus()
    runs = []
    for flag in (False, True):
        kw = dict(trips=True, link_bin_seconds=BIN, trip_free_flow=_free_flow_weights(net).cuda()) if flag else {}
        if head == "embedding":
            ev = _evaluator(net, pop, 4, emb, **kw)
        else:
            ev = VecEvaluator(O.engine_of(net, pop, 4), "dijkstra", **kw)
        runs.append((ev, ev.run(200)))
    (e0, r0), (e1, r1) = runs
    assert not r0.domain_exit and not r1.domain_exit and r0.frames_run == r1.frames_run == 200
    for k in PER_ENV_KEYS:
        assert getattr(r0, k) == getattr(r1, k), k
    assert r0 == r1                                       # every compared field of the dataclass
    assert r0.aggregate == r1.aggregate and r0.settings == r1.settings
    assert torch.equal(e0.reward[:200], e1.reward[:200]) and float(e0.reward.abs().sum()) > 0
    assert torch.equal(e0.eng.x, e1.eng.x) and torch.equal(e0.eng.agents, e1.eng.agents)
    assert r0.trips is None and r0.trip_bins is None and r0.trip_meta is None and not hasattr(e0, "trip_ff")
    assert r1.trips["n_done"].shape == (pop.size(0),) and r1.trip_bins["arr"].shape == (4, 3)
    assert int(r1.trips["n_done"].sum()) == sum(r1.arrived)
    assert "trips" not in r1.to_dict(per_env=True)        # the arrays never enter the JSON document


# ---- 4. the paired launch ------------------------------------------------------------------------------------------------------------
def test_paired_with_the_router_against_the_restatement():
    """The embedding policy and the router on two engines of one seed, K = 4, 200 frames: the router's launch takes the
    policy's tables as agents_b; both results against the restatement on the host copies of the two tables. In the
    environment's step order the router delivers only agents whose last hop was delayed: on this torus nobody in
    200 frames, so this pairing has no usable pair (the test prints the counts) and test_paired_mode_against_sampled pairs
    two runs that both deliver."""
    from tarl_hip.evaluator import VecEvaluator, trip_lines, trip_report
    net, _, pop, emb = _torus()
    w = _free_flow_weights(net).cuda()
    ev = _evaluator(net, pop, 4, emb, trips=True, link_bin_seconds=BIN, trip_free_flow=w)
    res = ev.run(200)
    router = VecEvaluator(O.engine_of(net, pop, 4), "dijkstra", trips=True, link_bin_seconds=BIN, trip_free_flow=w)
    base = router.run(200, trip_pair=ev.eng.agents)
    pol, rout = ev.eng.agents.cpu().numpy(), router.eng.agents.cpu().numpy()
    ff = res.trip_meta["free_flow"]
    assert np.array_equal(ff, base.trip_meta["free_flow"]) and base.trip_meta["paired"] and not res.trip_meta["paired"]
    for got, want in ((res.trips, R.agent_stats(pol, None, ff)), (base.trips, R.agent_stats(rout, pol, ff)),
                      (res.trip_bins, R.bin_stats(pol, BIN, 215, 3, ff)), (base.trip_bins, R.bin_stats(rout, BIN, 215, 3, ff))):
        assert set(got) == set(want)
        for k, v in want.items():
            assert np.array_equal(got[k], v), k
    print(f"[paired] policy trips {int(res.trips['n_done'].sum())}, router trips {int(base.trips['n_done'].sum())}, pairs "
          f"{int(base.trips['n_both'].sum())}, router faster / slower {int(base.trips['n_faster'].sum())} / "
          f"{int(base.trips['n_slower'].sum())}")
    rep = trip_report(res, baseline=base)
    p = rep["summary"]["paired"]
    assert p["available"] and p["baseline_head"] == "dijkstra" and p["pairs"] == int(base.trips["n_both"].sum())
    assert sum(r["n_faster"] for r in rep["rows"]) == int(base.trips["n_slower"][1:].sum())       # faster under the policy
    assert "policy - dijkstra:" in "\n".join(trip_lines(rep))
    other = VecEvaluator(O.engine_of(net, pop, 4, seed=4), "dijkstra", trips=True, link_bin_seconds=BIN).run(8)
    with pytest.raises(ValueError, match="seed"):
        trip_report(res, baseline=other)
    with pytest.raises(ValueError, match="trip_pair"):         # another population
        moved = ev.eng.agents.clone()
        moved[:, 3, 2] += 1
        router.run(8, trip_pair=moved)
    with pytest.raises(ValueError, match="trips=True"):
        VecEvaluator(O.engine_of(net, pop, 4), "dijkstra").run(8, trip_pair=ev.eng.agents)


def test_paired_launch_on_runs_that_both_deliver():
    """The router (and the sampled policy) deliver next to nobody on this torus, so the pairing with real pairs is MODE
    against MODE: on a second engine of ANOTHER noise seed the same agents arrive with other travel times, and the evaluator's
    paired launch must equal the restatement on the host copies of the two tables, with usable pairs and both signs of d
    (asserted). trip_report refuses that pairing (the seeds differ); on a second engine of the SAME seed the runs are
    identical, every pair has d = 0 and every classified agent is "neither"."""
    from tarl_hip.evaluator import trip_report
    net, _, pop, emb = _torus()
    w = _free_flow_weights(net).cuda()
    kw = dict(trips=True, link_bin_seconds=BIN, trip_free_flow=w)
    mode = _evaluator(net, pop, 4, emb, **kw)
    res = mode.run(300)
    other = _evaluator(net, pop, 4, emb, seed=4, **kw)
    base = other.run(300, trip_pair=mode.eng.agents)
    a, b = mode.eng.agents.cpu().numpy(), other.eng.agents.cpu().numpy()
    want = R.agent_stats(b, a, res.trip_meta["free_flow"])
    assert set(base.trips) == set(want) and all(np.array_equal(base.trips[k], v) for k, v in want.items())
    print(f"[paired, MODE seed 4 - MODE seed 3] trips {int(base.trips['n_done'].sum())} / {int(res.trips['n_done'].sum())}, pairs "
          f"{int(want['n_both'].sum())}, d < 0: {int(want['n_faster'].sum())}, d > 0: {int(want['n_slower'].sum())}")
    assert int(want["n_both"].sum()) >= 20 and int(want["n_faster"].sum()) > 0 and int(want["n_slower"].sum()) > 0
    with pytest.raises(ValueError, match="seed"):
        trip_report(res, baseline=base)
    twin = _evaluator(net, pop, 4, emb, **kw).run(300, trip_pair=mode.eng.agents)
    assert np.array_equal(twin.trips["n_both"], res.trips["n_done"]) and not twin.trips["d_sumsq"].any()
    rep = trip_report(res, baseline=twin)
    p = rep["summary"]["paired"]
    assert p["available"] and p["pairs"] == int(res.trips["n_done"].sum()) > 0 and p["mean_paired_diff"] == 0.0
    assert p["agents_faster"] == p["agents_slower"] == 0 and p["agents_neither"] == p["agents_classified"] > 0
    assert p["agents_classified"] == int((res.trips["n_done"][1:] >= 2).sum()) and p["expected_by_chance"] == 0.025 * p["agents_classified"]
    for r in rep["rows"]:
        assert r["paired_n"] == int(res.trips["n_done"][r["agent"]]) and r["n_faster"] == r["n_slower"] == 0
        assert r["baseline_tt_mean"] == r["tt_mean"] and (r["paired_diff_mean"] == 0.0 if r["paired_n"] else r["paired_diff_mean"] is None)


# ---- 5. refusals and the domain exit -------------------------------------------------------------------------------------------------
def test_environments_with_different_populations_are_refused():
    net, _, pop, emb = _torus()
    tables = pop.unsqueeze(0).repeat(2, 1, 1)
    tables[1, 5, 2] += 1.0                                 # one departure time, one environment
    with pytest.raises(ValueError, match="same population"):
        _evaluator(net, tables, 2, emb, trips=True).run(8)
    assert _evaluator(net, pop.unsqueeze(0).repeat(2, 1, 1), 2, emb, trips=True).run(8).trips is not None
    assert _evaluator(net, tables, 2, emb).run(8).trips is None          # without the flag nobody compares the tables
    with pytest.raises(ValueError, match="trips=True"):
        _evaluator(net, pop, 2, emb, trip_free_flow=_free_flow_weights(net).cuda())
    with pytest.raises(ValueError, match="TRIP_MAX_BINS"):
        _evaluator(net, pop, 2, emb, trips=True, link_bin_seconds=1).run(5000)


def test_a_domain_exit_returns_no_trips_and_leaves_the_engine_usable():
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import trip_report
    net = synth.torus_network(8, 8)
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    ev, _ = O.embedding_evaluator(net, pop, 2, trips=True)
    res = ev.run(256)
    assert res.domain_exit and res.aggregate is None
    assert res.trips is None and res.trip_bins is None and res.trip_meta is None and not trip_report(res)["available"]
    ev.eng.reset()
    ev.eng.check_flags()
    again = ev.run(8, deterministic=False)
    assert not again.domain_exit and again.frames_run == 8
    assert again.trips["n_done"].shape == (1025,) and again.trip_bins["arr"].shape == (2, 1) and again.trip_meta["first_bin"] == 5
    assert int(again.trips["n_done"].sum()) == sum(again.arrived) and int(again.trips["n_way"].sum()) == sum(again.on_way)


# ---- 6. CLI end to end ---------------------------------------------------------------------------------------------------------------
STEPS = 1800      # the untrained MODE policy delivers nobody in the first 600 frames; 8 trips of 2 agents by frame 1 800


def test_cli_trips_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-300"
    common = ["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--eval-baseline", "dijkstra",
              "--steps", str(STEPS)]
    on = tmp_path / "on"
    main(common + ["--eval-trips", "--output-dir", str(on)])
    text = capsys.readouterr().out
    assert "=== Trips ===" in text
    block = text[text.index("=== Trips ==="):]
    assert "agents:" in block and "By departure time" in block and "policy - dijkstra:" in block
    assert "expected by chance alone" in block and "below free flow:" in block
    doc = json.load(open(on / "eval_envs.json"))
    assert not doc["mode"]["domain_exit"], "the synthetic scenario left the domain under MODE"
    rows = list(csv.DictReader(open(on / "eval_trips.csv")))
    tr = doc["trips"]
    assert tr["available"] and "rows" not in tr and "by_departure" not in tr and tr["columns"] == list(rows[0])
    assert len(rows) == 300 == tr["summary"]["agents"] and [int(r["agent"]) for r in rows] == list(range(1, 301))
    assert tr["columns"][-9:] == ["baseline_arrival_share", "baseline_tt_mean", "paired_n", "paired_diff_mean", "paired_diff_se",
                                  "paired_diff_ci95_lo", "paired_diff_ci95_hi", "n_faster", "n_slower"]
    s = tr["summary"]
    arrived = sum(round(float(r["arrival_share"]) * 4) for r in rows)
    print(f"[cli] {STEPS} frames: {s['trips']} trips completed under the policy, {s['paired']['pairs']} pairs with the router")
    assert s["envs"] == 4 and s["frames_run"] == STEPS and s["trips"] == arrived > 0              # the run shows arrivals
    assert s["arrived_in_every"] + s["arrived_in_some"] + s["arrived_in_none"] == 300
    assert s["paired"]["available"] and s["paired"]["baseline_head"] == "dijkstra" and s["free_flow"]["trips"] > 0
    by = list(csv.DictReader(open(on / "eval_trips_by_departure.csv")))
    assert list(by[0]) == tr["by_departure_columns"] and [r["bin"] for r in by] == tr["bins"] == ["5h", "6h"]
    assert sum(int(r["scheduled"]) for r in by) == 300
    assert len(json.dumps(tr)) < 20000                                   # the summary only, never the A-row tables
    assert "trips" not in doc["mode"] and "trips" not in doc["baseline"]
    # without the flag: none of it, and the rest of the document is what it was
    off = tmp_path / "off"
    main(common + ["--output-dir", str(off)])
    assert "Trips" not in capsys.readouterr().out
    assert not (off / "eval_trips.csv").exists() and not (off / "eval_trips_by_departure.csv").exists()
    plain = json.load(open(off / "eval_envs.json"))
    assert set(plain) == {"mode", "baseline", "paired"} == set(doc) - {"trips"}
    for key in ("mode", "baseline"):
        for d in (plain[key], doc[key]):
            d.pop("computation_time_ms")
    assert plain == {k: v for k, v in doc.items() if k != "trips"}
    # the router alone
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--mode", "eval", "--scenario", scenario, "--dijkstra-envs", "4", "--eval-trips", "--steps", "60",
          "--output-dir", str(dj)])
    out = capsys.readouterr().out
    assert "=== Trips ===" in out and "policy - dijkstra" not in out
    rows = list(csv.DictReader(open(dj / "dijkstra_trips.csv")))
    assert len(rows) == 300 and "paired_n" not in rows[0]
    assert (dj / "dijkstra_trips_by_departure.csv").exists()
    assert json.load(open(dj / "dijkstra_envs.json"))["trips"]["summary"]["envs"] == 4
