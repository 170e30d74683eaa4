"""CPU: the host side of the per-trip report — the numpy restatement against a brute-force triple loop, the deliberate defects
against the crafted cases the GPU suite runs, trip_report / trip_lines / trip_summary on hand-made results, the flag's
refusal, and the argument validation of the two entry points and their ops wrappers (nothing here launches a kernel)."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import trips_restatement as R

CASES = R.crafted_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- the restatement against a brute-force triple loop ---------------------------------------------------------------------------
def _brute(case):
    """Everything by loops over (environment, agent), one scalar at a time, python floats (fp64) for the sums."""
    ag, base, ff = case["agents"], case["agents_b"], case["ff"]
    K, A, H, bs, fb = case["K"], case["A"], case["H"], case["bin_seconds"], case["first_bin"]
    pa = {k: [0] * A for k in ("n_done", "n_way", "n_under", "n_both", "n_faster", "n_slower")}
    pa.update({k: [0.0] * A for k in ("tt_sum", "tt_sumsq", "d_sum", "d_sumsq")})
    pa["tt_min"], pa["tt_max"] = [math.inf] * A, [-math.inf] * A
    pa["tt_min"][0] = pa["tt_max"][0] = 0.0
    pb = {k: [[0] * H for _ in range(K)] for k in ("dep_done", "dep_way", "arr", "dep_ff_n")}
    pb.update({k: [[0.0] * H for _ in range(K)] for k in ("dep_tt", "dep_ff")})
    clamp = lambda c: min(max(int(math.floor(float(c))) // bs - fb, 0), H - 1)      # noqa: E731
    for k in range(K):
        for a in range(1, A):
            row, rb = ag[k, a], base[k, a]
            hd = clamp(row[R.DEP])
            if row[R.DONE] == 1.0:
                tt = float(np.float32(row[R.ARR] - row[R.DEP]))
                pa["n_done"][a] += 1
                pa["tt_sum"][a] += tt
                pa["tt_sumsq"][a] += tt * tt
                pa["tt_min"][a], pa["tt_max"][a] = min(pa["tt_min"][a], tt), max(pa["tt_max"][a], tt)
                pa["n_under"][a] += math.isfinite(ff[a]) and tt < ff[a]
                pb["dep_done"][k][hd] += 1
                pb["dep_tt"][k][hd] += tt
                pb["arr"][k][clamp(row[R.ARR])] += 1
                if math.isfinite(ff[a]):
                    pb["dep_ff"][k][hd] += float(ff[a])
                    pb["dep_ff_n"][k][hd] += 1
                if rb[R.DONE] == 1.0:
                    d = tt - float(np.float32(rb[R.ARR] - rb[R.DEP]))
                    pa["n_both"][a] += 1
                    pa["d_sum"][a] += d
                    pa["d_sumsq"][a] += d * d
                    pa["n_faster"][a] += d < 0
                    pa["n_slower"][a] += d > 0
            elif row[R.ON_WAY] == 1.0:
                pa["n_way"][a] += 1
                pb["dep_way"][k][hd] += 1
    return pa, pb


@pytest.mark.parametrize("name", ["1x2", "2x65", "17x130", "stride-5x70", "H1-6x40", "H3-outer-empty-6x40", "fractional-33x200"])
def test_restatement_equals_the_triple_loop(name):
    """Same order of summation on both sides (ascending environment per agent, ascending agent per bin): == also on the
    fractional case."""
    case = BY_NAME[name]
    pa, pb = R.run_case(case)
    ba, bb = _brute(case)
    assert set(pa) == set(ba) and set(pb) == set(bb)
    for k, v in pa.items():
        assert np.array_equal(v, np.asarray(ba[k], dtype=v.dtype)), (name, k)
    for k, v in pb.items():
        assert np.array_equal(v, np.asarray(bb[k], dtype=v.dtype)), (name, k)
    assert pa["n_done"].dtype == np.int32 and pa["tt_sum"].dtype == np.float64 and pa["tt_min"].dtype == np.float32
    assert pb["arr"].dtype == np.int32 and pb["dep_tt"].dtype == np.float64 and pb["dep_ff_n"].dtype == np.int32


def test_restatement_by_hand():
    """Two environments, three agents and the dummy, bins of 10 s from bin 1 (clock 10), H = 2. Agent 1 departs at 12 and
    arrives at 19 / 25 (tt 7 and 13; arrivals in bins 0 and 1); agent 2 departs at 3 (below the first bin: bin 0) and is on
    the way in environment 0, arrived at 40 (past the last bin: bin 1, tt 37) in environment 1; agent 3 never departs. The
    baseline delivers agent 1 with tt 7 and 15 (d = 0 and -2) and agent 2 in environment 0 only (no usable pair)."""
    ag = np.zeros((2, 4, 9), np.float32)
    ag[:, 1, R.DEP], ag[:, 2, R.DEP], ag[:, 3, R.DEP] = 12, 3, 500
    ag[0, 1, [R.ARR, R.DONE]] = 19, 1
    ag[1, 1, [R.ARR, R.DONE]] = 25, 1
    ag[0, 2, R.ON_WAY] = 1
    ag[1, 2, [R.ARR, R.DONE]] = 40, 1
    base = ag.copy()
    base[1, 1, R.ARR] = 27
    base[0, 2, [R.ARR, R.ON_WAY, R.DONE]] = 9, 0, 1
    base[1, 2, [R.ARR, R.DONE]] = 0, 0
    ff = np.array([0.0, 8.0, np.inf, 5.0])
    pa = R.agent_stats(ag, base, ff)
    assert pa["n_done"].tolist() == [0, 2, 1, 0] and pa["n_way"].tolist() == [0, 0, 1, 0]
    assert pa["tt_sum"].tolist() == [0, 20, 37, 0] and pa["tt_sumsq"].tolist() == [0, 49 + 169, 37 * 37, 0]
    assert pa["tt_min"].tolist() == [0, 7, 37, np.inf] and pa["tt_max"].tolist() == [0, 13, 37, -np.inf]
    assert pa["n_under"].tolist() == [0, 1, 0, 0]
    assert pa["n_both"].tolist() == [0, 2, 0, 0] and pa["d_sum"].tolist() == [0, -2, 0, 0] and pa["d_sumsq"].tolist() == [0, 4, 0, 0]
    assert pa["n_faster"].tolist() == [0, 1, 0, 0] and pa["n_slower"].tolist() == [0, 0, 0, 0]
    pb = R.bin_stats(ag, 10, 1, 2, ff)
    assert pb["dep_done"].tolist() == [[1, 0], [2, 0]] and pb["dep_way"].tolist() == [[1, 0], [0, 0]]
    assert pb["arr"].tolist() == [[1, 0], [0, 2]] and pb["dep_tt"].tolist() == [[7, 0], [50, 0]]
    assert pb["dep_ff"].tolist() == [[8, 0], [8, 0]] and pb["dep_ff_n"].tolist() == [[1, 0], [1, 0]]      # ff = inf left out
    assert R.clock_bin(np.float32([9.99, 10.0, 19.5, 20.0, -3.0, 1e9]), 10, 1, 2).tolist() == [0, 0, 0, 1, 0, 1]


def test_crafted_cases_hold_what_they_promise():
    names = [c["name"] for c in CASES]
    for K, A in ((1, 2), (2, 65), (63, 64), (64, 257), (65, 1025), (130, 300)):
        assert f"{K}x{A}" in names
    assert BY_NAME["stride-5x70"]["pad"] == 5 and BY_NAME["H1-6x40"]["H"] == 1 and BY_NAME["H3-outer-empty-6x40"]["H"] == 3
    assert sum(1 for c in CASES if not c["exact"]) == 1 and sum(1 for c in CASES if c["full_roles"]) >= 8
    for c in CASES:
        ag, base, ff, K = c["agents"], c["agents_b"], c["ff"], c["K"]
        assert ag.dtype == np.float32 and ag.shape == base.shape == (K, c["A"], 9) and ff.shape == (c["A"],)
        assert np.array_equal(ag[:, :, :3], np.broadcast_to(ag[:1, :, :3], ag[:, :, :3].shape))          # one population
        assert np.array_equal(ag[:, :, :3], base[:, :, :3])
        if c["exact"]:
            for t in (ag, base):
                assert np.array_equal(t[:, :, [R.DEP, R.ARR]], np.round(t[:, :, [R.DEP, R.ARR]])) and float(t.max()) < 2 ** 24
        else:
            frac = ag[0, 1:, R.DEP] - np.floor(ag[0, 1:, R.DEP])
            assert set(frac.tolist()) == {0.25, 0.5}
        pa, pb = R.run_case(c)
        assert int(pa["n_done"].sum()) > 0 and int(pb["dep_done"].sum()) == int(pb["arr"].sum()) == int(pa["n_done"].sum())
        if c["name"].startswith("H3"):
            assert not pb["dep_done"][:, [0, 2]].any() and not pb["arr"][:, [0, 2]].any() and pb["dep_done"][:, 1].all()
        if not c["full_roles"]:
            continue
        n = pa["n_done"][1:]
        assert (n == K).any() and ((n > 0) & (n < K)).any() and (n == 0).any()           # in all, in some, in no environment
        assert int(pa["n_way"].sum()) > 0                                                # on the way at the end
        lo = np.floor(ag[0, 1:, R.DEP]) // c["bin_seconds"] - c["first_bin"]
        assert (lo < 0).any() and (lo > c["H"] - 1).any()                                # both clamps, by departure
        arr_bin = np.floor(ag[:, 1:, R.ARR]) // c["bin_seconds"] - c["first_bin"]
        assert ((arr_bin == c["H"] - 1) & (ag[:, 1:, R.DONE] == 1)).any()                # an arrival IN the last bin
        assert np.isinf(ff[1:]).any() and np.isfinite(ff[1:]).any()
        assert int(pa["n_faster"].sum()) > 0 and int(pa["n_slower"].sum()) > 0
        assert int(pa["n_both"].sum()) > int(pa["n_faster"].sum()) + int(pa["n_slower"].sum())        # pairs with d == 0
        one_sided = (ag[:, 1:, R.DONE] == 1) != (base[:, 1:, R.DONE] == 1)
        assert (one_sided & (ag[:, 1:, R.DONE] == 1)).any() and (one_sided & (base[:, 1:, R.DONE] == 1)).any()
        assert int(pa["n_under"].sum()) > 0 and bool((ag[:, 1:, R.DONE] + ag[:, 1:, R.ON_WAY] == 2).any())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_noticed_by_the_crafted_cases(defect):
    """The restatement with one defect differs from the true one on the crafted cases; per defect at least on the case named
    here (a partial tile: A = 300 is no multiple of 64)."""
    must = {"last_agent_of_partial_tile_skipped": "130x300", "no_low_clamp": "2x65", "no_high_clamp": "2x65"}.get(defect, "63x64")
    noticed = []
    for c in CASES:
        good, bad = R.run_case(c), R.run_case(c, defect=defect)
        if not (R.same(good[0], bad[0]) and R.same(good[1], bad[1])):
            noticed.append(c["name"])
    assert must in noticed and len(noticed) >= 8, (defect, noticed)


# ---- the report on hand-made results --------------------------------------------------------------------------------------------
def _result(agents, other=None, ff=None, head="embedding", H=4, first_bin=R.FIRST_BIN, bins=R.BIN_SECONDS, frames=300, seed=3):
    """An EvalResult as VecEvaluator(trips=True).run(trip_pair=other) leaves it, from the restatement."""
    from tarl_hip.evaluator import EvalResult
    K = agents.shape[0]
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=frames, settings={"seed": seed, "env_base": 0})
    res.trips = R.agent_stats(agents, other, ff)
    res.trip_bins = R.bin_stats(agents, bins, first_bin, H, ff)
    res.trip_meta = dict(first_bin=first_bin, bin_seconds=bins, origin=agents[0, :, 0].astype(np.int64),
                         destination=agents[0, :, 1].astype(np.int64), departure=agents[0, :, 2].copy(), free_flow=ff,
                         paired=other is not None)
    return res


def _close(a, b):
    return (a is None and b is None) or (a is not None and b is not None and math.isclose(a, b, rel_tol=1e-9, abs_tol=1e-9))


@pytest.mark.parametrize("name", ["17x130", "1x2"])
def test_report_against_numpy(name):
    from tarl_hip.evaluator import TRIP_FF_NOTE, trip_lines, trip_report, trip_summary
    c = BY_NAME[name]
    ag, ff, K, A = c["agents"], c["ff"], c["K"], c["A"]
    rep = trip_report(_result(ag, ff=ff))
    assert rep["available"] and rep["bins"] == ["bin200", "bin201", "bin202", "bin203"] and rep["first_bin"] == 200
    assert rep["columns"] == ["agent", "origin", "destination", "departure", "free_flow", "arrival_share", "envs_on_way",
                              "tt_mean", "tt_sd", "tt_se", "tt_ci95_lo", "tt_ci95_hi", "tt_min", "tt_max", "delay_mean",
                              "delay_ratio"]
    assert len(rep["rows"]) == A - 1 and [r["agent"] for r in rep["rows"]] == list(range(1, A))
    tts_all, ffs_all, under = [], [], 0
    for r in rep["rows"]:
        a = r["agent"]
        assert list(r) == rep["columns"]
        done = ag[:, a, R.DONE] == 1
        tts = (ag[:, a, R.ARR] - ag[:, a, R.DEP]).astype(np.float64)[done]
        m = R.moments(tts)
        assert r["origin"] == int(ag[0, a, 0]) and r["destination"] == int(ag[0, a, 1]) and r["departure"] == float(ag[0, a, 2])
        assert r["free_flow"] == (float(ff[a]) if np.isfinite(ff[a]) else None)
        assert r["arrival_share"] == done.sum() / K and r["envs_on_way"] == int((~done & (ag[:, a, R.ON_WAY] == 1)).sum())
        for key in ("mean", "sd", "se", "ci95_lo", "ci95_hi"):
            assert _close(r[f"tt_{key}"], m[key]), (a, key)
        if tts.size == 0:
            assert r["tt_mean"] is None and r["tt_min"] is None and r["tt_max"] is None and r["delay_mean"] is None
        else:
            assert r["tt_min"] == tts.min() and r["tt_max"] == tts.max()
        if tts.size == 1:
            assert r["tt_mean"] == tts[0] and r["tt_sd"] is None and r["tt_se"] is None and r["tt_ci95_lo"] is None
        if tts.size and np.isfinite(ff[a]):
            assert _close(r["delay_mean"], tts.mean() - ff[a]) and _close(r["delay_ratio"], tts.mean() / ff[a])
            tts_all += tts.tolist()
            ffs_all += [ff[a]] * tts.size
            under += int((tts < ff[a]).sum())
        else:
            assert r["delay_mean"] is None and r["delay_ratio"] is None
    s = rep["summary"]
    n = (ag[:, 1:, R.DONE] == 1).sum(axis=0)
    assert (s["envs"], s["agents"], s["trips"]) == (K, A - 1, int(n.sum()))
    assert (s["arrived_in_every"], s["arrived_in_some"], s["arrived_in_none"]) == \
        (int((n == K).sum()), int(((n > 0) & (n < K)).sum()), int((n == 0).sum()))
    f = s["free_flow"]
    assert f["trips"] == len(tts_all) and f["note"] == TRIP_FF_NOTE
    assert _close(f["mean_delay"], float(np.mean(np.asarray(tts_all) - np.asarray(ffs_all))))       # trip-weighted
    assert _close(f["delay_ratio"], float(np.sum(tts_all) / np.sum(ffs_all)))
    assert _close(f["share_trips_below_free_flow"], under / len(tts_all))
    delays = sorted(((r["delay_mean"], r["agent"]) for r in rep["rows"] if r["delay_mean"] is not None), key=lambda t: (-t[0], t[1]))
    assert [t["agent"] for t in s["top_delays"]] == [a for _, a in delays[:10]]
    # by departure time
    pb = R.bin_stats(ag, c["bin_seconds"], c["first_bin"], 4, ff)
    assert rep["by_departure_columns"] == ["bin", "scheduled", "arrived_mean", "arrived_se", "on_way_mean", "tt_mean", "tt_se",
                                           "delay_mean", "delay_se", "arrivals_mean"]
    sched = np.bincount(R.clock_bin(ag[0, 1:, R.DEP], c["bin_seconds"], c["first_bin"], 4), minlength=4)
    for h, r in enumerate(rep["by_departure"]):
        assert r["bin"] == rep["bins"][h] and r["scheduled"] == sched[h]
        m = R.moments(pb["dep_done"][:, h])
        assert _close(r["arrived_mean"], m["mean"]) and _close(r["arrived_se"], m["se"])
        per_env = [pb["dep_tt"][k, h] / pb["dep_done"][k, h] for k in range(K) if pb["dep_done"][k, h] > 0]
        assert _close(r["tt_mean"], R.moments(per_env)["mean"]) and _close(r["tt_se"], R.moments(per_env)["se"])
        dl = [pb["dep_tt"][k, h] / pb["dep_done"][k, h] - pb["dep_ff"][k, h] / pb["dep_ff_n"][k, h] for k in range(K)
              if pb["dep_done"][k, h] > 0 and pb["dep_ff_n"][k, h] > 0]
        assert _close(r["delay_mean"], R.moments(dl)["mean"])
        assert r["arrivals_mean"] == pb["arr"][:, h].mean() and r["on_way_mean"] == pb["dep_way"][:, h].mean()
    text = "\n".join(trip_lines(rep))
    assert "agents:" in text and "mean delay:" in text and "below free flow:" in text and "By departure time" in text
    assert "not a lower bound" in text and "paired" not in text and ("+-" in text) == (K > 1)
    assert len([ln for ln in text.splitlines() if ln.startswith("  agent ")]) == min(10, len(delays))
    doc = trip_summary(rep)
    assert "rows" not in doc and "by_departure" not in doc and doc["columns"] == rep["columns"] and doc["summary"]["envs"] == K
    json.loads(json.dumps(doc, allow_nan=False))
    # without free-flow times: no delay columns' values, and the block says so
    bare = trip_report(_result(ag))
    assert bare["summary"]["free_flow"] is None and all(r["free_flow"] is None and r["delay_mean"] is None for r in bare["rows"])
    assert "no free-flow weights" in "\n".join(trip_lines(bare))


def test_paired_report_and_its_classification():
    """Six agents, K = 3, both runs deliver everybody except agent 4 (one usable pair). Differences policy - baseline:
    agent 1: -2, -2, -2 (se = 0, mean < 0: faster); 2: 0, 0, 0 (se = 0, mean 0: neither); 3: +1, +1, +1 (slower);
    4: one pair (not classified); 5: -10, -11, -9 (interval below 0: faster); 6: -5, +5, 0 (neither)."""
    from tarl_hip.evaluator import TRIP_CHANCE, trip_lines, trip_report
    diffs = {1: [-2, -2, -2], 2: [0, 0, 0], 3: [1, 1, 1], 4: [4], 5: [-10, -11, -9], 6: [-5, 5, 0]}
    K, A = 3, 7
    pol = np.zeros((K, A, 9), np.float32)
    pol[:, :, R.DEP] = 20010
    base = pol.copy()
    for a, ds in diffs.items():
        for k, d in enumerate(ds):
            base[k, a, [R.ARR, R.DONE]] = 20010 + 50 + 3 * k, 1
            pol[k, a, [R.ARR, R.DONE]] = 20010 + 50 + 3 * k + d, 1
    pol[1:, 4, R.ON_WAY] = 1
    res = _result(pol)
    rep = trip_report(res, baseline=_result(base, other=pol, head="dijkstra"))
    assert rep["columns"][-9:] == ["baseline_arrival_share", "baseline_tt_mean", "paired_n", "paired_diff_mean", "paired_diff_se",
                                   "paired_diff_ci95_lo", "paired_diff_ci95_hi", "n_faster", "n_slower"]
    for r in rep["rows"]:
        ds = diffs[r["agent"]]
        m = R.moments(ds)
        assert r["paired_n"] == len(ds) and _close(r["paired_diff_mean"], m["mean"]) and _close(r["paired_diff_se"], m["se"])
        assert _close(r["paired_diff_ci95_lo"], m["ci95_lo"]) and _close(r["paired_diff_ci95_hi"], m["ci95_hi"])
        assert r["n_faster"] == sum(d < 0 for d in ds) and r["n_slower"] == sum(d > 0 for d in ds)
        assert r["baseline_arrival_share"] == len(ds) / K and r["baseline_tt_mean"] == 50 + 3 * (len(ds) - 1) / 2
    assert rep["rows"][3]["paired_diff_se"] is None and rep["rows"][3]["envs_on_way"] == 2
    p = rep["summary"]["paired"]
    want = [R.classify(diffs[a]) for a in range(1, A)]
    assert want == ["faster", "neither", "slower", None, "faster", "neither"]
    assert (p["agents_faster"], p["agents_slower"], p["agents_neither"], p["agents_classified"]) == (2, 1, 2, 5)
    assert p["expected_by_chance"] == TRIP_CHANCE * 5 == 0.125 and p["pairs"] == 16
    assert _close(p["mean_paired_diff"], sum(sum(d) for d in diffs.values()) / 16)
    text = "\n".join(trip_lines(rep))
    assert "policy - dijkstra:" in text and "expected by chance alone: 0.1" in text and "faster under the policy 2, slower 1" in text
    # refusals, as paired_report: another seed, env_base, K, population, frames; a baseline that was not paired
    for change in (dict(seed=4), dict(frames=299)):
        with pytest.raises(ValueError, match="seed" if "seed" in change else "same frames"):
            trip_report(res, baseline=_result(base, other=pol, **change))
    other = _result(base, other=pol)
    other.settings["env_base"] = 8
    with pytest.raises(ValueError, match="env_base"):
        trip_report(res, baseline=other)
    with pytest.raises(ValueError, match="same environments"):
        trip_report(res, baseline=_result(base[:2], other=pol[:2]))
    moved = base.copy()
    moved[:, 2, R.DEP] += 1
    with pytest.raises(ValueError, match="same population"):
        trip_report(res, baseline=_result(moved, other=pol))
    unpaired = trip_report(res, baseline=_result(base))
    assert not unpaired["summary"]["paired"]["available"] and "not paired" in "\n".join(trip_lines(unpaired))


def test_report_of_runs_without_trips():
    from tarl_hip.evaluator import EvalResult, trip_lines, trip_report, trip_summary
    out = EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64, domain_exit=True, domain_exit_frames=(0, 64))
    rep = trip_report(out)
    assert not rep["available"] and "left the domain" in rep["reason"]
    assert trip_lines(rep) == [f"not available: {rep['reason']}"] and trip_summary(rep) == rep
    assert not trip_report(EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64))["available"]
    res = _result(BY_NAME["2x65"]["agents"])
    nothing = EvalResult(envs=2, head="dijkstra", deterministic=True, frames_run=300, settings=dict(res.settings))
    assert not trip_report(res, baseline=nothing)["summary"]["paired"]["available"]


# ---- flags ----------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_refusals():
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    assert main.build_parser().parse_args([]).eval_trips is False
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "4", "--eval-trips", "--eval-link-bin", "900"])
    a = RunnerArgs(**vars(ns))
    assert a.eval_trips and a.eval_link_bin == 900 and not a.eval_occupancy and not a.eval_link_counts
    base = dict(algo="mpnn", scenario="synthetic-1024-1024", mode="eval")
    assert RunnerArgs(**base).eval_trips is False
    assert RunnerArgs(**base, eval_envs=4, eval_trips=True).eval_trips
    assert RunnerArgs(**dict(base, algo="dijkstra"), dijkstra_envs=4, eval_trips=True).eval_trips
    with pytest.raises(ValueError, match="eval_trips"):
        RunnerArgs(**base, eval_trips=True)
    with pytest.raises(ValueError, match="eval_trips"):
        RunnerArgs(**dict(base, algo="dijkstra"), eval_trips=True)


def test_cli_refuses_the_flag_alone():
    main = importlib.import_module("main").main
    with pytest.raises(ValueError, match="eval_trips"):
        main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--eval-trips"])


# ---- the entry points and their wrappers validate on the host -----------------------------------------------------------------------
def test_entry_point_validation():
    from tarl_hip import lib, ops
    assert "tarl_trip_agent_stats" in lib.SIGNATURES and "tarl_trip_bin_stats" in lib.SIGNATURES
    assert ops.TRIP_MAX_BINS >= 2048
    L = lib.load()
    null = None
    p = torch.zeros(64).data_ptr()      # everything is checked before anything is launched: the address is never dereferenced
    ag = L.tarl_trip_agent_stats
    #         agents b  ff    K  A  abs bbs under  n_done n_way sum sumsq min max  both dsum dsq fast slow  stream
    good = [p, null, null, 2, 3, 27, 0, null] + [p] * 6 + [null] * 5 + [null]
    for i in (0, 8, 9, 10, 11, 12, 13):
        a = list(good)
        a[i] = null
        assert ag(*a) == -1 and b"null" in L.tarl_last_error(), i
    a = list(good)
    a[1] = p                                                            # agents_b without its outputs
    assert ag(*a) == -1 and b"paired outputs" in L.tarl_last_error()
    a = list(good)
    a[2] = p                                                            # ff without n_under
    assert ag(*a) == -1 and b"ff and n_under" in L.tarl_last_error()
    for i, v, msg in ((3, 0, b"bad sizes"), (4, 0, b"bad sizes"), (3, 1 << 31, b"bad sizes"), (5, 26, b"overlap")):
        a = list(good)
        a[i] = v
        assert ag(*a) == -1 and msg in L.tarl_last_error(), (i, v)
    a = [p, p, null, 2, 3, 27, 26, null] + [p] * 6 + [p] * 5 + [null]
    assert ag(*a) == -1 and b"agents_b" in L.tarl_last_error()
    bn = L.tarl_trip_bin_stats
    #         agents K  A  abs perm seg ff   bin first H  dep_done dep_way arr dep_tt dep_ff dep_ff_n stream
    good = [p, 2, 3, 27, p, p, null, 100, 0, 4, p, p, p, p, null, null, null]
    for i in (0, 4, 5, 10, 11, 12, 13):
        a = list(good)
        a[i] = null
        assert bn(*a) == -1 and b"null" in L.tarl_last_error(), i
    a = list(good)
    a[6] = p                                                            # ff without dep_ff / dep_ff_n
    assert bn(*a) == -1 and b"ff needs" in L.tarl_last_error()
    for i, v, msg in ((1, 0, b"bad sizes"), (2, 0, b"bad sizes"), (3, 26, b"overlap"), (7, 0, b"bin_seconds"), (8, -1, b"first_bin"),
                      (9, 0, b"H must be"), (9, ops.TRIP_MAX_BINS + 1, b"H must be"), (1, 1 << 20, b"too many")):
        a = list(good)
        a[i] = v
        if msg == b"too many":
            a[9] = ops.TRIP_MAX_BINS
        assert bn(*a) == -1 and msg in L.tarl_last_error(), (i, v)


def test_ops_wrappers_refuse_bad_arguments():
    from tarl_hip import lib, ops
    K, A, H = 2, 5, 3
    ag = torch.zeros((K, A, 9))
    with pytest.raises(lib.TarlError, match="GPU"):                      # everything else in order: a host tensor is refused
        ops.trip_agent_stats(ag)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=H, order=(torch.zeros(A - 1, dtype=torch.int32),
                                                                                torch.zeros(H + 1, dtype=torch.int32)))
    with pytest.raises(TypeError, match="agents"):
        ops.trip_agent_stats(ag.double())
    with pytest.raises(ValueError, match="agents"):
        ops.trip_agent_stats(ag[0])
    with pytest.raises(ValueError, match="agents"):
        ops.trip_agent_stats(torch.zeros((K, A, 8)))
    with pytest.raises(ValueError, match="overlap"):
        ops.trip_agent_stats(ag[:1].expand(K, A, 9))
    with pytest.raises(ValueError, match="agents_b"):
        ops.trip_agent_stats(ag, torch.zeros((K, A + 1, 9)))
    with pytest.raises(TypeError, match="free_flow"):
        ops.trip_agent_stats(ag, free_flow=torch.zeros(A))
    with pytest.raises(ValueError, match="free_flow"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=H, free_flow=torch.zeros(A + 1, dtype=torch.float64))
    with pytest.raises(TypeError, match="n_done"):
        ops.trip_agent_stats(ag, out={"n_done": torch.zeros(A)})
    with pytest.raises(ValueError, match="dep_tt"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=H, out={"dep_tt": torch.zeros((K, H + 1), dtype=torch.float64)})
    with pytest.raises(ValueError, match="num_bins"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=ops.TRIP_MAX_BINS + 1)
    with pytest.raises(ValueError, match="num_bins"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=0)
    with pytest.raises(ValueError, match="bin_seconds"):
        ops.trip_bin_stats(ag, bin_seconds=0, first_bin=0, num_bins=H)
    with pytest.raises(ValueError, match="first_bin"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=-1, num_bins=H)
    with pytest.raises(ValueError, match="perm"):
        ops.trip_bin_stats(ag, bin_seconds=100, first_bin=0, num_bins=H, order=(torch.zeros(A, dtype=torch.int32),
                                                                                torch.zeros(H + 1, dtype=torch.int32)))


def test_departure_order_and_clock_bins_in_torch():
    """The torch plumbing of the per-bin kernel on the host: the bins agree with the restatement's rule (NaN, negative and
    huge clocks included), perm lists the agents 1 .. A - 1 bin by bin in ascending id, seg delimits the segments."""
    from tarl_hip import ops
    c = BY_NAME["130x300"]
    dep = torch.from_numpy(c["agents"][0, :, R.DEP].copy())
    bins = ops.trip_clock_bin(dep, c["bin_seconds"], c["first_bin"], c["H"]).numpy()
    assert np.array_equal(bins, R.clock_bin(dep.numpy(), c["bin_seconds"], c["first_bin"], c["H"]))
    odd = torch.tensor([float("nan"), -5.0, -1e30, float("-inf"), 0.0, 99.9, 100.0, 1e30, float("inf")])
    assert ops.trip_clock_bin(odd, 100, 0, 7).tolist() == [0, 0, 0, 0, 0, 0, 1, 6, 6]
    perm, seg = ops.trip_departure_order(dep, bin_seconds=c["bin_seconds"], first_bin=c["first_bin"], num_bins=c["H"])
    assert perm.dtype == seg.dtype == torch.int32 and perm.shape == (c["A"] - 1,) and seg.shape == (c["H"] + 1,)
    assert sorted(perm.tolist()) == list(range(1, c["A"])) and seg[0] == 0 and seg[-1] == c["A"] - 1
    for h in range(c["H"]):
        part = perm[int(seg[h]):int(seg[h + 1])].tolist()
        assert part == sorted(part) and all(bins[a] == h for a in part)
    perm, seg = ops.trip_departure_order(torch.zeros(1), bin_seconds=10, first_bin=0, num_bins=2)      # the dummy alone
    assert perm.shape == (1,) and seg.tolist() == [0, 0, 0]
