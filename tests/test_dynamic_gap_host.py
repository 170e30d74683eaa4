"""CPU: the host side of the dynamic relative gap — the numpy restatement (a heap-based time-dependent Dijkstra with the leave
rule) against an enumeration of paths and one hand-computed case, the situations the crafted cases must hold, the deliberate
defects against those cases, dynamic_gap_report / _lines / _summary on hand-made results, the flags' refusals, and the argument
validation of the entry points and their ops wrappers (nothing here launches a kernel)."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import dynamic_gap_restatement as R

CASES = R.crafted_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_restatement_equals_the_enumeration_of_paths(name):
    """Every crafted case has at most 6 roads: the minimum over all simple paths of leave composed road by road is the
    hindsight arrival, with == (both sides compose the same fp64 operations along the winning path)."""
    c = BY_NAME[name]
    tau, env, best = R.run_case(c)
    assert tau.dtype == np.float32 and env.dtype == np.float64 and best.dtype == np.float64
    assert tau.shape == (c["K"], c["H"], c["N"]) and env.shape == (c["K"], c["H"] + 1, c["N"])
    assert np.array_equal(best, R.brute(c["edges"], c["N"], tau, env, c["agents"], c["bin_seconds"], c["first_bin"]))
    assert np.isinf(env[:, -1]).all() and (env[:, :-1] <= env[:, 1:]).all()          # the envelope is non-decreasing in h


def test_master_case_by_hand():
    """tau = 200 / (20 - cbar): 10 everywhere, +inf on road 3 in bin 1 of environment 0; road 1 (10, 40, 10, 10), road 2 (20,
    20, 10, 20) and road 4 (10, 100, 10, 10) in environment 1; bin 2 has no frames and gets FF = 10. S = 200, 300, 400, 500.
    Environment 0: agent 1 (0 -> 3 at 205) 215, 225, 235 on either path; agent 2 (at 295) 305, 315 and road 3 entered in bin
    1 at +inf: left at env[2] = 410; agent 5 (3 -> 4 at 380) 410 by the same wait, then 420; agent 7 (0 -> 4 at 585) 595, 605,
    615 (the clock 605 lies past the last bin: clamped), 625; agent 9 (1 -> 3 at 295) 305, then 410.
    Environment 1: agent 2: 305, road 1 at 40 s gives 345, road 2 at 20 s gives 325, then 335 through road 2, although road
    1 is the quicker one in the departure bin; agent 5: 390, road 4 entered at 390 would be left at 490, waiting for bin 2
    gives 410; agent 8 (2 -> 3 at 210): 230, 240; agent 9: 305 (bin 0), 315."""
    c = R.master_case()
    tau, env, best = R.run_case(c)
    assert tau[0, 1, 3] == np.inf and np.isinf(tau).sum() == 1 and (tau[:, 2, :] == 10).all()
    assert tau[1, :, 1].tolist() == [10, 40, 10, 10] and tau[1, :, 2].tolist() == [20, 20, 10, 20]
    assert tau[1, :, 4].tolist() == [10, 100, 10, 10]
    assert env[0, :, 3].tolist() == [210, 410, 410, 510, np.inf] and env[1, :, 1].tolist() == [210, 340, 410, 510, np.inf]
    assert env[1, :, 2].tolist() == [220, 320, 410, 520, np.inf] and env[1, :, 4].tolist() == [210, 400, 410, 510, np.inf]
    assert np.array_equal(best, c["want"])
    tt, ht, g, use = R.gap(c["agents"], best)
    assert use[0].tolist() == [False, True, True, True, False, True, True, True, False, True]
    assert ht[1, 2] == 40 and tt[1, 2] == 50 and g[1, 2] == 10 and g[0, 2] == 50 - 115
    pa, pe, pb = R.reductions(c["agents"], best, np.zeros(10, np.int64), 1)
    assert pe["n"].tolist() == [7, 8] and pe["n_neg"][0] >= 1 and pa["n"].tolist() == [0, 2, 2, 2, 0, 2, 2, 2, 1, 2]
    assert pb["n"][:, 0].tolist() == [7, 8] and pa["g_min"][4] == np.inf and pa["g_max"][4] == -np.inf
    rg = R.relative_gaps(pe)
    assert rg[1] == (pe["tt_sum"][1] - pe["ht_sum"][1]) / pe["tt_sum"][1] and R.relative_gaps({"tt_sum": [0.0], "ht_sum": [0.0],
                                                                                              "n": [0]}) == [None]


def test_crafted_cases_hold_what_they_promise():
    """Each case against the list of situations it must contain; every situation of the issue occurs in the master case, and
    the random cases hold fractional times."""
    seen = set()
    for c in CASES:
        found = R.situations(c)
        assert set(c["must"]) <= found, (c["name"], set(c["must"]) - found)
        seen |= found
        assert c["N"] <= 6 and c["agents"].dtype == np.float32 and c["veh"].dtype == np.int32
        assert np.array_equal(c["agents"][:, :, :3], np.broadcast_to(c["agents"][:1, :, :3], c["agents"][:, :, :3].shape))
    assert set(BY_NAME["master"]["must"]) == set(R.SITUATIONS) == seen
    assert {c["H"] for c in CASES} >= {1, 2, 4, 5} and {c["bin_seconds"] for c in CASES} >= {1, 7, 100}
    frac = [c for c in CASES if c["name"].startswith("random")]
    assert all((c["free_flow"] != np.round(c["free_flow"])).any() for c in frac)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_noticed_by_the_crafted_cases(defect):
    """The restatement with one defect differs from the true one: in the gaps of the master case, and on at least three
    cases in all."""
    noticed = []
    for c in CASES:
        _, _, good = R.run_case(c)
        _, _, bad = R.run_case(c, defect=defect)
        g0, g1 = R.gap(c["agents"], good)[2], R.gap(c["agents"], bad, defect)[2]
        if not np.array_equal(g0, g1, equal_nan=True):
            noticed.append(c["name"])
    assert "master" in noticed and len(noticed) >= 3, (defect, noticed)


def test_bin_rule_and_leave():
    assert [R.clock_bin(t, 100, 2, 3) for t in (-5.0, 0.0, 199.9, 200.0, 299.5, 300.0, 499.9, 500.0, 1e30, float("nan"))] == \
        [0, 0, 0, 0, 0, 1, 2, 2, 2, 0]
    assert R.clock_bin(150.0, 100, 2, 3, "no_low_clamp") is None and R.clock_bin(500.0, 100, 2, 3, "no_high_clamp") is None
    tau = np.array([[10.0], [2.0]], np.float32)
    env = R.envelope(tau[None], 100, 2)[0]
    assert env[:, 0].tolist() == [210, 302, np.inf]
    kw = dict(bin_seconds=100, first_bin=2)
    assert R.leave(tau, env, 0, 250.0, **kw) == 260 and R.leave(tau, env, 0, 295.0, **kw) == 302          # waiting wins
    assert R.leave(tau, env, 0, 300.0, **kw) == 302 and R.leave(tau, env, 0, 777.0, **kw) == 779
    assert R.leave(tau, env, 0, math.inf, **kw) == math.inf and R.leave(tau, env, 0, float("nan"), **kw) == math.inf
    ts = np.linspace(100, 600, 1001)
    out = [R.leave(tau, env, 0, t, **kw) for t in ts]
    assert all(b >= a for a, b in zip(out, out[1:]))                                  # non-decreasing in t
    nan = np.array([[np.nan], [2.0]], np.float32)
    e2 = R.envelope(nan[None], 100, 2)[0]
    assert e2[:, 0].tolist() == [302, 302, np.inf] and R.leave(nan, e2, 0, 250.0, **kw) == 302      # a NaN tau is +inf


# ---- the report on hand-made results -------------------------------------------------------------------------------------------------
def _result(case, best=None, head="embedding", frames=300, seed=3, envs=None, defect=None):
    """An EvalResult as VecEvaluator(dynamic_gap=True).run() leaves it, from the restatement."""
    from tarl_hip.evaluator import EvalResult
    if best is None:
        best = R.run_case(case)[2]
    ag = case["agents"]
    J = ag.shape[0] if envs is None else envs
    ag, best = ag[:J], best[:J]
    H = case["H"]
    dep_bin = np.array([R.clock_bin(t, case["bin_seconds"], case["first_bin"], H) for t in ag[0, :, R.DEP]])
    pa, pe, pb = R.reductions(ag, best, dep_bin, H, defect)
    res = EvalResult(envs=case["K"], head=head, deterministic=True, frames_run=frames, settings={"seed": seed, "env_base": 0})
    res.dynamic_gap = dict(best=best, per_agent=pa, per_env=pe, per_bin=pb,
                           meta=dict(envs=J, first_bin=case["first_bin"], bin_seconds=case["bin_seconds"],
                                     frames_per_bin=[int(x) for x in case["frames_per_bin"]],
                                     origin=ag[0, :, 0].astype(np.int64), destination=ag[0, :, 1].astype(np.int64),
                                     departure=ag[0, :, 2].copy(), searches=int((ag[:, 1:, R.DONE] == 1).sum()), wall_ms=1.5))
    return res


def _close(a, b):
    return (a is None and b is None) or (a is not None and b is not None and math.isclose(a, b, rel_tol=1e-9, abs_tol=1e-9))


@pytest.mark.parametrize("name", ["master", "random-5x3x5-702"])
def test_report_against_numpy(name):
    from tarl_hip.evaluator import DYNAMIC_GAP_NOTE, dynamic_gap_lines, dynamic_gap_report, dynamic_gap_summary
    c = BY_NAME[name]
    ag, K, A, H = c["agents"], c["K"], c["agents"].shape[1], c["H"]
    best = R.run_case(c)[2]
    tt, ht, g, use = R.gap(ag, best)
    rep = dynamic_gap_report(_result(c))
    assert rep["available"] and rep["definition"] == DYNAMIC_GAP_NOTE and len(rep["bins"]) == H
    assert rep["columns"] == ["agent", "origin", "destination", "departure", "envs_usable", "gap_mean", "gap_sd", "gap_se",
                              "gap_ci95_lo", "gap_ci95_hi", "gap_min", "gap_max", "envs_negative"]
    assert [r["agent"] for r in rep["rows"]] == list(range(1, A))
    for r in rep["rows"]:
        a = r["agent"]
        v = g[:, a][use[:, a]]
        m = R.moments(v)
        assert list(r) == rep["columns"] and r["envs_usable"] == v.size and r["envs_negative"] == int((v < 0).sum())
        assert r["origin"] == int(ag[0, a, 0]) and r["destination"] == int(ag[0, a, 1]) and r["departure"] == float(ag[0, a, 2])
        # the report forms the variance from sum g and sum g^2: (s2 - s1^2 / n) / (n - 1) cancels, with an absolute error of
        # a few 2^-52 s2, so the spread agrees with numpy's two-pass value within sqrt(2^-48 s2)
        tol = math.sqrt(2.0 ** -48 * float((v * v).sum()))
        assert _close(r["gap_mean"], m["mean"])
        for key in ("sd", "se", "ci95_lo", "ci95_hi"):
            assert (r[f"gap_{key}"] is None) == (m[key] is None) and (m[key] is None or abs(r[f"gap_{key}"] - m[key]) <= 1.96 * tol), (a, key)
        assert (r["gap_min"], r["gap_max"]) == ((float(v.min()), float(v.max())) if v.size else (None, None))
    s = rep["summary"]
    rg = [float((tt[k][use[k]].sum() - ht[k][use[k]].sum()) / tt[k][use[k]].sum()) if use[k].any() else None for k in range(K)]
    assert all(_close(x, y) for x, y in zip(s["relative_gap_per_env"], rg))
    m = R.moments(rg)
    assert s["relative_gap"]["n"] == m["n"] and _close(s["relative_gap"]["mean"], m["mean"]) and _close(s["relative_gap"]["se"], m["se"])
    assert _close(s["relative_gap"]["std"], m["sd"])
    assert (s["relative_gap"]["ci95"] is None) == (m["se"] is None)
    if m["se"] is not None:
        assert _close(s["relative_gap"]["ci95"][0], m["ci95_lo"]) and _close(s["relative_gap"]["ci95"][1], m["ci95_hi"])
    n = int(use.sum())
    assert (s["envs"], s["agents"], s["trips"], s["searches"]) == (K, A - 1, n, int((ag[:, 1:, R.DONE] == 1).sum()))
    assert _close(s["mean_gap"], float(g[use].sum()) / n)
    assert s["share_negative"] == int((g[use] < 0).sum()) / n and s["share_nonpositive"] == int((g[use] <= 0).sum()) / n
    means = sorted(((r["gap_mean"], r["agent"]) for r in rep["rows"] if r["gap_mean"] is not None), key=lambda t: (-t[0], t[1]))
    assert [t["agent"] for t in s["top_gaps"]] == [a for _, a in means[:10]]
    dep_bin = np.array([R.clock_bin(t, c["bin_seconds"], c["first_bin"], H) for t in ag[0, :, R.DEP]])
    assert rep["by_departure_columns"] == ["bin", "trips_mean", "gap_mean", "gap_se", "envs"]
    for h, r in enumerate(rep["by_departure"]):
        sel = use & (dep_bin == h)[None, :]
        per_env = [float(g[k][sel[k]].sum()) / int(sel[k].sum()) for k in range(K) if sel[k].any()]
        mm = R.moments(per_env)
        assert r["bin"] == rep["bins"][h] and r["trips_mean"] == sel.sum(axis=1).mean() and r["envs"] == len(per_env)
        assert _close(r["gap_mean"], mm["mean"]) and _close(r["gap_se"], mm["se"])
    text = "\n".join(dynamic_gap_lines(rep))
    assert "definition:" in text and "relative gap:" in text and "mean gap:" in text and "g < 0 in" in text and "g <= 0 in" in text
    assert f"{s['searches']}   hindsight searches" in text and "1.5 ms" in text and "By departure time" in text
    assert "policy -" not in text and len([ln for ln in text.splitlines() if ln.startswith("  agent ")]) == min(10, len(means))
    doc = dynamic_gap_summary(rep)
    assert "rows" not in doc and "by_departure" not in doc and doc["columns"] == rep["columns"]
    json.loads(json.dumps(doc, allow_nan=False))
    turned = dynamic_gap_report(_result(c, defect="gap_sign_turned"))["rows"]
    assert all(_close(t["gap_mean"], None if r["gap_mean"] is None else -r["gap_mean"]) for t, r in zip(turned, rep["rows"]))
    assert any(r["gap_mean"] for r in rep["rows"])


def test_report_with_one_environment_and_without_a_usable_trip():
    from tarl_hip.evaluator import EvalResult, dynamic_gap_lines, dynamic_gap_report, dynamic_gap_summary
    c = BY_NAME["master"]
    one = dynamic_gap_report(_result(c, envs=1))                      # dynamic_gap_envs = 1: one environment, no spread
    s = one["summary"]
    assert s["envs"] == 1 and s["relative_gap"]["n"] == 1 and s["relative_gap"]["se"] is None and s["relative_gap"]["ci95"] is None
    assert all(r["gap_sd"] is None and r["envs_usable"] <= 1 for r in one["rows"]) and "+-" not in "\n".join(dynamic_gap_lines(one))
    nobody = dict(c, agents=c["agents"].copy())
    nobody["agents"][:, :, R.DONE] = 0
    rep = dynamic_gap_report(_result(nobody))
    s = rep["summary"]
    assert s["trips"] == 0 and s["mean_gap"] is None and s["share_negative"] is None and s["relative_gap"]["mean"] is None
    assert s["relative_gap_per_env"] == [None, None] and s["relative_gap"]["missing"] == 2 and s["top_gaps"] == []
    assert "no environment with a completed trip" in "\n".join(dynamic_gap_lines(rep))
    json.loads(json.dumps(dynamic_gap_summary(rep), allow_nan=False))
    out = EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64, domain_exit=True, domain_exit_frames=(0, 64))
    gone = dynamic_gap_report(out)
    assert not gone["available"] and "left the domain" in gone["reason"]
    assert dynamic_gap_lines(gone) == [f"not available: {gone['reason']}"] and dynamic_gap_summary(gone) == gone
    assert not dynamic_gap_report(EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64))["available"]


def test_paired_report_and_its_refusals():
    """The baseline: the same case with every arrival 7 s later in environment 0 and 3 s earlier in environment 1."""
    from tarl_hip.evaluator import EvalResult, dynamic_gap_lines, dynamic_gap_report
    c = BY_NAME["master"]
    b = dict(c, agents=c["agents"].copy())
    done = b["agents"][:, :, R.DONE] == 1
    b["agents"][0, :, R.ARR] += np.where(done[0], 7, 0).astype(np.float32)
    b["agents"][1, :, R.ARR] -= np.where(done[1], 3, 0).astype(np.float32)
    res, base = _result(c), _result(b, head="dijkstra")
    rep = dynamic_gap_report(res, baseline=base)
    p = rep["summary"]["paired"]
    rg = rep["summary"]["relative_gap_per_env"]
    brg = dynamic_gap_report(base)["summary"]["relative_gap_per_env"]
    d = [x - y for x, y in zip(rg, brg)]
    m = R.moments(d)
    assert p["available"] and p["baseline_head"] == "dijkstra" and p["n"] == 2 and p["dropped"] == 0
    assert _close(p["mean"], m["mean"]) and _close(p["se"], m["se"]) and _close(p["ci95"][0], m["ci95_lo"])
    assert d[0] < 0 < d[1] and _close(p["baseline_relative_gap"]["mean"], float(np.mean(brg)))
    from tarl_hip.evaluator import dynamic_gap_paired_lines
    assert "policy - dijkstra:" in "\n".join(dynamic_gap_lines(rep)) and "paired" in "\n".join(dynamic_gap_lines(rep))
    assert dynamic_gap_lines(rep) == dynamic_gap_lines(rep, paired=False) + dynamic_gap_paired_lines(rep)
    assert len(dynamic_gap_paired_lines(rep)) == 1 and dynamic_gap_paired_lines(dynamic_gap_report(res)) == []
    for change, msg in ((dict(seed=4), "seed"), (dict(frames=299), "same frames"), (dict(envs=1), "same frames")):
        with pytest.raises(ValueError, match=msg):
            dynamic_gap_report(res, baseline=_result(b, **change))
    other = _result(b)
    other.settings["env_base"] = 8
    with pytest.raises(ValueError, match="env_base"):
        dynamic_gap_report(res, baseline=other)
    other = _result(b)
    other.envs = 3
    with pytest.raises(ValueError, match="same environments"):
        dynamic_gap_report(res, baseline=other)
    moved = dict(b, agents=b["agents"].copy())
    moved["agents"][:, 2, R.DEP] += 1
    with pytest.raises(ValueError, match="same population"):
        dynamic_gap_report(res, baseline=_result(moved))
    wider = dict(b, bin_seconds=200, first_bin=1)
    with pytest.raises(ValueError, match="bins"):
        dynamic_gap_report(res, baseline=_result(wider))
    nothing = EvalResult(envs=2, head="dijkstra", deterministic=True, frames_run=300, settings=dict(res.settings))
    un = dynamic_gap_report(res, baseline=nothing)
    assert not un["summary"]["paired"]["available"] and "not available" in "\n".join(dynamic_gap_lines(un))


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_refusals():
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.eval_dynamic_gap is False and ns.eval_dynamic_gap_envs is None
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "4", "--eval-dynamic-gap",
                                         "--eval-dynamic-gap-envs", "2", "--eval-link-bin", "900"])
    a = RunnerArgs(**vars(ns))
    assert a.eval_dynamic_gap and a.eval_dynamic_gap_envs == 2 and a.eval_link_bin == 900
    assert not a.eval_occupancy and not a.eval_trips and not a.eval_link_counts
    base = dict(algo="mpnn", scenario="synthetic-1024-1024", mode="eval")
    assert RunnerArgs(**base).eval_dynamic_gap is False
    assert RunnerArgs(**base, eval_envs=4, eval_dynamic_gap=True).eval_dynamic_gap_envs is None
    assert RunnerArgs(**dict(base, algo="dijkstra"), dijkstra_envs=4, eval_dynamic_gap=True, eval_dynamic_gap_envs=4).eval_dynamic_gap
    with pytest.raises(ValueError, match="eval_dynamic_gap"):
        RunnerArgs(**base, eval_dynamic_gap=True)
    with pytest.raises(ValueError, match="eval_dynamic_gap"):
        RunnerArgs(**dict(base, algo="dijkstra"), eval_dynamic_gap=True)
    with pytest.raises(ValueError, match="mode 'eval'"):
        RunnerArgs(**dict(base, algo="mpnn+ppo", mode="train"), eval_envs=4, eval_dynamic_gap=True)
    with pytest.raises(ValueError, match="eval_dynamic_gap_envs"):
        RunnerArgs(**base, eval_envs=4, eval_dynamic_gap_envs=2)
    for j in (0, 5):
        with pytest.raises(ValueError, match="eval_dynamic_gap_envs"):
            RunnerArgs(**base, eval_envs=4, eval_dynamic_gap=True, eval_dynamic_gap_envs=j)


def test_cli_refuses_the_flags_alone():
    main = importlib.import_module("main").main
    with pytest.raises(ValueError, match="eval_dynamic_gap"):
        main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--eval-dynamic-gap"])
    with pytest.raises(ValueError, match="eval_dynamic_gap_envs"):
        main(["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--eval-envs", "2",
              "--eval-dynamic-gap-envs", "1"])


# ---- the entry points and their wrappers validate on the host ---------------------------------------------------------------------
def _plan_like(N):
    """A tarl_plan whose only fields the checks read are N and E: the checks run before anything is dereferenced."""
    import ctypes
    buf = (ctypes.c_int64 * 64)()
    buf[0], buf[1], buf[2] = N, 0, 0
    return buf


def test_entry_point_validation():
    import ctypes
    from tarl_hip import lib, ops
    for name in ("tarl_td_road_times", "tarl_td_hindsight", "tarl_td_hindsight_scratch_bytes"):
        assert name in lib.SIGNATURES
    L = lib.load()
    null = None
    p = torch.zeros(64).data_ptr()      # everything is checked before anything is launched: the address is never dereferenced
    rt = L.tarl_td_road_times
    #       veh fpb max ff cc  K  H  N  bin  first tau env stream
    good = [p, p, p, p, p, 2, 3, 5, 100, 0, p, p, null]
    for i in (0, 1, 2, 3, 4, 10, 11):
        a = list(good)
        a[i] = null
        assert rt(*a) == -1 and b"null" in L.tarl_last_error(), i
    for i, v, msg in ((5, 0, b"bad sizes"), (5, 65536, b"bad sizes"), (7, 0, b"bad sizes"), (7, 1 << 31, b"bad sizes"),
                      (8, 0, b"bin_seconds"), (9, -1, b"first_bin"), (6, 0, b"H must be"), (6, ops.TRIP_MAX_BINS + 1, b"H must be")):
        a = list(good)
        a[i] = v
        assert rt(*a) == -1 and msg in L.tarl_last_error(), (i, v)
    a = list(good)
    a[5], a[6], a[7] = 65535, 4096, (1 << 31) - 1
    assert rt(*a) == -1 and b"2^40" in L.tarl_last_error()
    plan_buf = _plan_like(21)
    plan = ctypes.cast(plan_buf, ctypes.c_void_p)
    sb = L.tarl_td_hindsight_scratch_bytes
    assert sb(plan, 3, 400) == 1024 * 256 and sb(plan, 3, 10) == 30 * 256          # one fp64 row of 21, rounded to 256 B
    assert sb(null, 3, 10) == -1 and sb(plan, 0, 10) == -1 and sb(plan, 3, 0) == -1 and sb(plan, 1 << 31, 1) == -1
    hs = L.tarl_td_hindsight
    #       plan tau env agents K  A  abs bin  first H  scratch bytes  best stream
    good = [plan, p, p, p, 2, 3, 27, 100, 0, 4, p, 6 * 256, p, null]
    for i in (0, 1, 2, 3, 12):
        a = list(good)
        a[i] = null
        assert hs(*a) == -1 and b"null" in L.tarl_last_error(), i
    for i, v, msg in ((4, 0, b"bad sizes"), (5, 0, b"bad sizes"), (4, 1 << 31, b"bad sizes"), (6, 26, b"overlap"),
                      (7, 0, b"bin_seconds"), (8, -1, b"first_bin"), (9, 0, b"H must be"), (9, ops.TRIP_MAX_BINS + 1, b"H must be"),
                      (10, null, b"scratch too small"), (11, 6 * 256 - 1, b"scratch too small")):
        a = list(good)
        a[i] = v
        assert hs(*a) == -1 and msg in L.tarl_last_error(), (i, v)
    a = list(good)
    a[0] = ctypes.cast(_plan_like(327681), ctypes.c_void_p)                 # the graph-size limit of tarl_dest_trees
    assert hs(*a) == -1 and b"N > 327680" in L.tarl_last_error()
    a[0] = ctypes.cast(_plan_like(0), ctypes.c_void_p)
    assert hs(*a) == -1 and b"no road" in L.tarl_last_error()


def test_ops_wrappers_refuse_bad_arguments():
    from tarl_hip import lib, ops
    K, H, N, A = 2, 3, 5, 4
    veh, fpb = torch.zeros((K, H, N), dtype=torch.int32), torch.ones(H, dtype=torch.int32)
    f = torch.ones(N)
    kw = dict(bin_seconds=100, first_bin=0)
    with pytest.raises(lib.TarlError, match="GPU"):                      # everything else in order: a host tensor is refused
        ops.td_road_times(veh, fpb, f, f, f, **kw)
    with pytest.raises(ValueError, match="veh"):
        ops.td_road_times(veh[0], fpb, f, f, f, **kw)
    with pytest.raises(TypeError, match="veh"):
        ops.td_road_times(veh.long(), fpb, f, f, f, **kw)
    with pytest.raises(ValueError, match="frames_per_bin"):
        ops.td_road_times(veh, torch.ones(H + 1, dtype=torch.int32), f, f, f, **kw)
    with pytest.raises(TypeError, match="frames_per_bin"):
        ops.td_road_times(veh, fpb.long(), f, f, f, **kw)
    for i, name in enumerate(("max_agents", "free_flow", "cong")):
        args = [f, f, f]
        args[i] = torch.ones(N + 1)
        with pytest.raises(ValueError, match=name):
            ops.td_road_times(veh, fpb, *args, **kw)
        args[i] = f.double()
        with pytest.raises(TypeError, match=name):
            ops.td_road_times(veh, fpb, *args, **kw)
    with pytest.raises(ValueError, match="bin_seconds"):
        ops.td_road_times(veh, fpb, f, f, f, bin_seconds=0, first_bin=0)
    with pytest.raises(ValueError, match="first_bin"):
        ops.td_road_times(veh, fpb, f, f, f, bin_seconds=100, first_bin=-1)
    with pytest.raises(ValueError, match="num_bins"):
        big = ops.TRIP_MAX_BINS + 1
        ops.td_road_times(torch.zeros((1, big, 1), dtype=torch.int32), torch.ones(big, dtype=torch.int32), f[:1], f[:1], f[:1], **kw)
    with pytest.raises(ValueError, match="tau"):
        ops.td_road_times(veh, fpb, f, f, f, out=(torch.zeros((K, H, N + 1)), torch.zeros((K, H + 1, N), dtype=torch.float64)), **kw)
    with pytest.raises(TypeError, match="env"):
        ops.td_road_times(veh, fpb, f, f, f, out=(torch.zeros((K, H, N)), torch.zeros((K, H + 1, N))), **kw)

    class FakePlan:
        num_nodes = N
    plan = FakePlan()
    tau, env, ag = torch.zeros((K, H, N)), torch.zeros((K, H + 1, N), dtype=torch.float64), torch.zeros((K, A, 9))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.td_hindsight(plan, tau, env, ag, **kw)
    with pytest.raises(ValueError, match="agents"):
        ops.td_hindsight(plan, tau, env, ag[0], **kw)
    with pytest.raises(TypeError, match="agents"):
        ops.td_hindsight(plan, tau, env, ag.double(), **kw)
    with pytest.raises(ValueError, match="overlap"):
        ops.td_hindsight(plan, tau, env, ag[:1].expand(K, A, 9), **kw)
    with pytest.raises(ValueError, match="tau"):
        ops.td_hindsight(plan, tau[:, :, :4], env, ag, **kw)
    with pytest.raises(ValueError, match="tau"):
        ops.td_hindsight(plan, tau[0], env, ag, **kw)
    with pytest.raises(TypeError, match="tau"):
        ops.td_hindsight(plan, tau.double(), env, ag, **kw)
    with pytest.raises(ValueError, match="env"):
        ops.td_hindsight(plan, tau, env[:, :H], ag, **kw)
    with pytest.raises(TypeError, match="env"):
        ops.td_hindsight(plan, tau, env.float(), ag, **kw)
    with pytest.raises(ValueError, match="bin_seconds"):
        ops.td_hindsight(plan, tau, env, ag, bin_seconds=0, first_bin=0)
    with pytest.raises(ValueError, match="first_bin"):
        ops.td_hindsight(plan, tau, env, ag, bin_seconds=100, first_bin=-1)
    with pytest.raises(ValueError, match="out"):
        ops.td_hindsight(plan, tau, env, ag, out=torch.zeros((K, A + 1), dtype=torch.float64), **kw)
    with pytest.raises(TypeError, match="out"):
        ops.td_hindsight(plan, tau, env, ag, out=torch.zeros((K, A)), **kw)
    with pytest.raises(TypeError, match="scratch"):
        ops.td_hindsight(plan, tau, env, ag, scratch=torch.zeros(64), **kw)
