"""CPU: the host side of the per-road occupancy — the numpy restatement against hand-computed cases, the deliberate defects
against the crafted cases the GPU suite runs, occupancy_report / occupancy_lines / occupancy_summary against numpy, the flag's
refusals, and the argument validation of the entry point and its ops wrapper (nothing here launches a kernel)."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import occupancy_restatement as R

CASES = R.crafted_cases()


# ---- the restatement against hand-computed cases -------------------------------------------------------------------------------
def test_accumulate_restatement_by_hand():
    """Frames at the clocks 8, 9, 10 with bins of 10 s: the first two fall in bin 0, the third in bin 1 (the clock at which the
    frame STARTS). Two roads (MAX 5 and 3: thr 2 and 0), one environment. Road 0 holds 1, 2, 3 vehicles after the three
    frames: 3 vehicle-frames and one frame at capacity (2 >= 2) in bin 0, 3 and one in bin 1, peak 3. Road 1 holds 0, 0, 4:
    thr 0 makes every frame a frame at capacity, also the empty ones."""
    thr = R.threshold([5.0, 3.0])
    assert thr.tolist() == [2, 0] and thr.dtype == np.int32
    ring = np.array([[[1.0], [0.0]], [[2.0], [0.0]], [[3.0], [4.0]]], dtype=np.float32)        # (F, N, K) = (3, 2, 1)
    veh, full, peak = (np.zeros((1, 2, 2), np.int32), np.zeros((1, 2, 2), np.int32), np.zeros((1, 1, 2), np.int32))
    R.accumulate(ring, thr, veh, full, peak, 8, 1, 10, 0)
    assert veh.tolist() == [[[3, 0], [3, 4]]] and full.tolist() == [[[1, 2], [1, 1]]] and peak.tolist() == [[[3, 4]]]
    # a second call continues the first: the sums add, the peak is max-merged
    R.accumulate(np.array([[[1.0], [9.0]]], dtype=np.float32), thr, veh, full, peak, 11, 1, 10, 0)
    assert veh.tolist() == [[[3, 0], [4, 13]]] and full.tolist() == [[[1, 2], [1, 2]]] and peak.tolist() == [[[3, 9]]]
    # thr = ceil(MAX - 3) for a fractional MAX, literally for MAX <= 3
    assert R.threshold([14.0, 0.0, 3.5, 2.0, 3.0]).tolist() == [11, -3, 1, -1, 0]


def test_value_conversion_by_hand():
    v = np.array([0.0, 0.99, 1.0, 7.9, 255.0, 255.5, 300.0, 1e30, np.inf, -0.5, -1.0, -np.inf, np.nan], dtype=np.float32)
    assert R.to_count(v).tolist() == [0, 0, 1, 7, 255, 255, 255, 255, 255, 0, 0, 0, 0]


def test_crafted_cases_cover_what_the_issue_lists():
    names = {c["name"] for c in CASES}
    for K, N, F in ((1, 1, 1), (5, 6, 7), (3, 21, 64), (64, 64, 3), (65, 63, 9), (2, 257, 64), (130, 70, 5)):
        for clock in ("no-edge", "edge-first", "edge-last", "skipping"):
            assert f"{K}x{N}x{F}-{clock}" in names
    by = {c["name"]: c for c in CASES}
    for c in CASES:
        assert c["ring"].dtype == np.float32 and c["ring"].shape[1:] == (c["N"], c["K"])
        thr = c["thr"].astype(np.int64)[None, :, None]
        allowed = (c["ring"] == 0) | (c["ring"] == thr - 1) | (c["ring"] == thr) | (c["ring"] == thr + 1) | (c["ring"] == 127)
        assert allowed.all(), c["name"]
        if c["N"] >= 2:
            assert c["thr"][0] < 0 and c["thr"][1] == 0                         # roads with thr <= 0
        veh, full, peak = R.run_case(c)
        assert int(veh.sum()) > 0 and int(full.sum()) > 0 and int(peak.max()) == 127
        assert not veh[:, 0].any() and not veh[:, -1].any() and not full[:, 0].any() and not full[:, -1].any()
    # the clocks do what their names say (bins of the frames, relative to the first stored bin, which stays empty)
    def bins(c):
        F = c["ring"].shape[0]
        return [(c["calls"][0]["t0"] + f * c["timestep"]) // c["bin_seconds"] - c["first_bin"] for f in range(F)]
    assert set(bins(by["3x21x64-no-edge"])) == {1}
    b = bins(by["3x21x64-edge-first"])
    assert b[0] == 1 and by["3x21x64-edge-first"]["calls"][0]["t0"] % 3600 == 0
    b = bins(by["3x21x64-edge-last"])
    assert b[:-1] == [1] * 63 and b[-1] == 2
    b = bins(by["5x6x7-skipping"])
    assert b == sorted(b) and len(set(b)) == 7 and b[1] - b[0] >= 2            # every frame its own bin, bins skipped
    # values at every one of the five levels on a road with thr > 1, and in a partial tile beyond the first
    c = by["130x70x5-no-edge"]
    n = int(np.argmax(c["thr"] > 1))
    assert {0, int(c["thr"][n]) - 1, int(c["thr"][n]), int(c["thr"][n]) + 1, 127} <= set(c["ring"][:, n, :].ravel().tolist())
    c = by["5x6x7-timestep-0"]                                             # the clock stands still: one bin holds every frame
    assert c["timestep"] == 0 and c["ring"].shape == (7, 6, 5) and c["H"] == 3 and set(bins(c)) == {1}
    veh, full, peak = R.run_case(c)
    counts = R.to_count(c["ring"])
    assert np.array_equal(veh[:, 1], counts.sum(axis=0).T) and np.array_equal(peak[:, 0], counts.max(axis=0).T)
    assert len(by["two-calls"]["calls"]) == 2 and by["two-calls"]["calls"][1]["partial"]
    assert [x["partial"] for x in by["three-calls"]["calls"]] == [False, False, True]


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_noticed_by_the_crafted_cases(defect):
    """The restatement with one defect differs from the true one on the crafted cases; per defect at least on the case named
    here, which is the one that exists for it."""
    must = {"clock_after_step": "3x21x64-edge-last", "count_before_frame": "64x64x3-no-edge",
            "greater_than": "5x6x7-no-edge", "threshold_max_minus_2": "5x6x7-no-edge", "peak_added": "two-calls",
            "overwrite_second_call": "two-calls", "skip_partial_block": "three-calls", "swap_in_tile": "65x63x9-no-edge"}[defect]
    noticed = []
    for c in CASES:
        good, bad = R.run_case(c), R.run_case(c, defect=defect)
        if any(not np.array_equal(g, b) for g, b in zip(good, bad)):
            noticed.append(c["name"])
    assert must in noticed, (defect, noticed)


# ---- the report against numpy ----------------------------------------------------------------------------------------------------
def _result(K, seed, head="embedding", empty=False, H=2, N=5, frames=(60, 40)):
    """An EvalResult with random accumulators over H bins (``frames`` frames in each), MAX = (0, 3, 8, 14, 14) and a return
    that satisfies the identity."""
    from tarl_hip.evaluator import EvalResult, capacity_threshold, link_moments
    rng = np.random.default_rng(seed)
    cap = np.array([0.0, 3.0, 8.0, 14.0, 14.0])[:N]
    thr = capacity_threshold(cap)
    T = int(sum(frames))
    if empty:
        veh = np.zeros((K, H, N), dtype=np.int32)
        peak = np.zeros((K, 1, N), dtype=np.int32)
    else:
        veh = np.stack([rng.integers(0, 12 * frames[h], size=(K, N)) for h in range(H)], axis=1).astype(np.int32)
        peak = rng.integers(1, 15, size=(K, 1, N)).astype(np.int32)
    full = np.stack([rng.integers(0, frames[h] + 1, size=(K, N)) for h in range(H)], axis=1).astype(np.int32)
    full[:, :, thr <= 0] = np.asarray(frames, dtype=np.int32)[None, :, None]      # at capacity in every frame
    if empty:
        full[:, :, thr > 0] = 0
    occ = {"veh": veh, "full": full, "peak": peak}
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=T, settings={"seed": 3, "env_base": 0})
    res.episode_return = [-float(veh[b].astype(np.int64).sum()) for b in range(K)]
    res.occupancy = occ
    res.occupancy_stats = {k: link_moments(R.stats(v), K) for k, v in occ.items()}
    res.occupancy_frames_per_bin = list(frames)
    res.occupancy_meta = dict(first_bin=5, bin_seconds=3600, timestep=2, max=cap, thr=thr)
    return res, occ


@pytest.mark.parametrize("K", [1, 4])
def test_report_against_numpy(K):
    from tarl_hip.evaluator import occupancy_lines, occupancy_report, occupancy_summary
    res, occ = _result(K, seed=K)
    rep = occupancy_report(res)
    assert rep["available"] and rep["bins"] == ["occ_5h", "occ_6h"] and rep["first_bin"] == 5 and rep["bin_seconds"] == 3600
    assert rep["columns"] == ["road", "max_agents", "thr", "veh_seconds_mean", "veh_seconds_sd", "veh_seconds_se",
                              "veh_seconds_ci95_lo", "veh_seconds_ci95_hi", "veh_seconds_min", "veh_seconds_max", "occ_5h",
                              "occ_6h", "vc_mean", "peak_mean", "peak_max", "full_frames_mean", "full_frames_min",
                              "full_frames_max", "full_share"]
    veh, full, peak = (occ[k].astype(np.float64) for k in ("veh", "full", "peak"))
    T, step, cap = 100, 2, np.array([0.0, 3.0, 8.0, 14.0, 14.0])
    for n, row in enumerate(rep["rows"]):
        assert list(row) == rep["columns"]
        tot = veh[:, :, n].sum(axis=1) * step                                   # vehicle-seconds per environment
        assert row["road"] == n and row["max_agents"] == cap[n] and row["thr"] == math.ceil(cap[n] - 3)
        assert math.isclose(row["veh_seconds_mean"], tot.mean(), rel_tol=1e-12)
        assert row["veh_seconds_min"] == tot.min() and row["veh_seconds_max"] == tot.max()
        if K == 1:
            assert all(row[f"veh_seconds_{k}"] is None for k in ("sd", "se", "ci95_lo", "ci95_hi"))
        else:
            sd = tot.std(ddof=1)
            se = sd / math.sqrt(K)
            assert math.isclose(row["veh_seconds_sd"], sd, rel_tol=1e-12, abs_tol=1e-9)
            assert math.isclose(row["veh_seconds_se"], se, rel_tol=1e-12, abs_tol=1e-9)
            assert math.isclose(row["veh_seconds_ci95_lo"], tot.mean() - 1.96 * se, rel_tol=1e-12, abs_tol=1e-9)
            assert math.isclose(row["veh_seconds_ci95_hi"], tot.mean() + 1.96 * se, rel_tol=1e-12, abs_tol=1e-9)
        assert math.isclose(row["occ_5h"], veh[:, 0, n].mean() / 60, rel_tol=1e-12)
        assert math.isclose(row["occ_6h"], veh[:, 1, n].mean() / 40, rel_tol=1e-12)
        assert math.isclose(row["vc_mean"], veh[:, :, n].sum(axis=1).mean() / T / max(cap[n], 1.0), rel_tol=1e-12)
        assert row["peak_mean"] == peak[:, 0, n].mean() and row["peak_max"] == peak[:, 0, n].max()
        ff = full[:, :, n].sum(axis=1)
        assert row["full_frames_mean"] == ff.mean() and row["full_frames_min"] == ff.min() and row["full_frames_max"] == ff.max()
        assert math.isclose(row["full_share"], ff.mean() / T, rel_tol=1e-12)
    assert rep["rows"][0]["full_share"] == 1.0 and rep["rows"][1]["full_share"] == 1.0        # MAX 0 and 3: thr <= 0
    s = rep["summary"]
    vh = veh.sum(axis=(1, 2)) * step / 3600.0
    assert s["envs"] == K and s["roads"] == 5 and s["frames_run"] == T and s["timestep"] == step
    assert math.isclose(s["vehicle_hours"]["mean"], vh.mean(), rel_tol=1e-12) and s["vehicle_hours"]["n"] == K
    if K == 1:
        assert s["vehicle_hours"]["se"] is None and s["vehicle_hours"]["ci95"] is None
    else:
        assert math.isclose(s["vehicle_hours"]["se"], vh.std(ddof=1) / math.sqrt(K), rel_tol=1e-12)
    vc = veh / np.array([60.0, 40.0])[None, :, None] / np.maximum(cap, 1.0)[None, None, :]
    assert np.allclose(s["vc_mean_per_bin"], vc.mean(axis=2).mean(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(s["vc_sd_per_bin"], vc.std(axis=2).mean(axis=0), rtol=1e-12, atol=0)
    assert s["frames_per_bin"] == [60, 40]
    assert math.isclose(s["share_road_frames_at_capacity"], full.sum() / (K * T * 5), rel_tol=1e-12)
    assert s["mean_roads_ever_at_capacity"] == (full.sum(axis=1) > 0).sum(axis=1).mean()
    assert s["largest_peak"] == peak.max()
    assert s["identity"]["holds"] and s["identity"]["vehicle_frames"] == [int(x) for x in veh.sum(axis=(1, 2))]
    assert "paired" not in s
    text = "\n".join(occupancy_lines(rep))
    assert "vehicle-hours:" in text and "v/c occ_5h:" in text and "at capacity:" in text and "identity:" in text
    assert "in every environment: yes" in text and "roads with the most frames at capacity" in text
    assert ("(se)" in text) == (K > 1)
    top = [line for line in text.splitlines() if line.startswith("  road")]
    order = sorted(rep["rows"], key=lambda r: (-r["full_frames_mean"], r["road"]))
    assert len(top) == 5 and [int(line.split()[1]) for line in top] == [r["road"] for r in order]
    doc = occupancy_summary(rep)
    assert "rows" not in doc and doc["summary"]["envs"] == K and doc["columns"] == rep["columns"]
    json.loads(json.dumps(doc, allow_nan=False))                       # plain JSON: no nan, no array
    # a broken identity is reported, not hidden
    res.episode_return[0] -= 1.0
    bad = occupancy_report(res)
    assert not bad["summary"]["identity"]["holds"] and "in every environment: NO" in "\n".join(occupancy_lines(bad))


def test_report_of_a_run_with_no_vehicle_and_of_runs_without_occupancy():
    from tarl_hip.evaluator import EvalResult, occupancy_lines, occupancy_report, occupancy_summary
    res, _ = _result(3, seed=0, empty=True)
    rep = occupancy_report(res)
    s = rep["summary"]
    assert s["vehicle_hours"]["mean"] == 0.0 and s["vehicle_hours"]["se"] == 0.0 and s["identity"]["holds"]
    assert s["vc_mean_per_bin"] == [0.0, 0.0] and s["vc_sd_per_bin"] == [0.0, 0.0] and s["largest_peak"] == 0
    assert s["mean_roads_ever_at_capacity"] == 2.0 and s["share_road_frames_at_capacity"] == 2 / 5      # the two thr <= 0 roads
    for row in rep["rows"]:
        assert row["veh_seconds_mean"] == 0.0 and row["vc_mean"] == 0.0 and row["peak_max"] == 0 and row["occ_5h"] == 0.0
    assert len(occupancy_lines(rep)) >= 6
    # a bin without a frame (bins skipped by a large timestep) has no occupancy: None, and None in the JSON summary
    res.occupancy_frames_per_bin = [100, 0]
    rep = occupancy_report(res)
    assert rep["rows"][2]["occ_6h"] is None and rep["rows"][2]["occ_5h"] == 0.0
    doc = occupancy_summary(rep)
    assert doc["summary"]["vc_mean_per_bin"] == [0.0, None]
    json.dumps(doc, allow_nan=False)
    # no occupancy: a domain exit, or a run without the flag
    out = EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64, domain_exit=True, domain_exit_frames=(0, 64))
    rep = occupancy_report(out)
    assert not rep["available"] and "left the domain" in rep["reason"]
    assert occupancy_lines(rep) == [f"not available: {rep['reason']}"] and occupancy_summary(rep) == rep
    assert not occupancy_report(EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64))["available"]


@pytest.mark.parametrize("K", [1, 4])
def test_paired_report_against_numpy(K, monkeypatch):
    """The paired numbers come from the two-input statistics kernel; here its numpy restatement stands in for the launch, so
    that the host arithmetic behind it is checked without a GPU."""
    from tarl_hip import eval_reports, evaluator as E
    monkeypatch.setattr(eval_reports, "_paired_moments", lambda a, b, K: E.link_moments(R.stats(a, b), K))
    res, a = _result(K, seed=1)
    base, b = _result(K, seed=2, head="dijkstra")
    rep = E.occupancy_report(res, baseline=base)
    assert rep["columns"][-10:] == ["baseline_veh_seconds_mean", "paired_veh_seconds_mean", "paired_veh_seconds_se",
                                    "paired_veh_seconds_ci95_lo", "paired_veh_seconds_ci95_hi", "baseline_full_frames_mean",
                                    "paired_full_frames_mean", "paired_full_frames_se", "paired_full_frames_ci95_lo",
                                    "paired_full_frames_ci95_hi"]
    step = 2
    dv = (a["veh"].astype(np.int64) - b["veh"]).sum(axis=1).astype(np.float64) * step          # (K, N)
    df = (a["full"].astype(np.int64) - b["full"]).sum(axis=1).astype(np.float64)
    excl = {"veh_seconds": 0, "full_frames": 0}
    for n, row in enumerate(rep["rows"]):
        assert list(row) == rep["columns"]
        assert math.isclose(row["baseline_veh_seconds_mean"], b["veh"][:, :, n].sum(axis=1).mean() * step, rel_tol=1e-12)
        assert row["baseline_full_frames_mean"] == b["full"][:, :, n].sum(axis=1).mean()
        for key, d in (("veh_seconds", dv), ("full_frames", df)):
            assert math.isclose(row[f"paired_{key}_mean"], d[:, n].mean(), rel_tol=1e-12, abs_tol=1e-12)
            if K == 1:
                assert row[f"paired_{key}_se"] is None and row[f"paired_{key}_ci95_lo"] is None
                continue
            se = d[:, n].std(ddof=1) / math.sqrt(K)
            assert math.isclose(row[f"paired_{key}_se"], se, rel_tol=1e-12, abs_tol=1e-9)
            assert math.isclose(row[f"paired_{key}_ci95_lo"], d[:, n].mean() - 1.96 * se, rel_tol=1e-12, abs_tol=1e-9)
            assert math.isclose(row[f"paired_{key}_ci95_hi"], d[:, n].mean() + 1.96 * se, rel_tol=1e-12, abs_tol=1e-9)
            excl[key] += (d[:, n].mean() - 1.96 * se > 0) or (d[:, n].mean() + 1.96 * se < 0)
    p = rep["summary"]["paired"]
    assert p["available"] and p["baseline_head"] == "dijkstra"
    assert p["roads_interval_excludes_zero"] == ({"veh_seconds": None, "full_frames": None} if K == 1 else excl)
    dvh = (a["veh"].astype(np.int64).sum(axis=(1, 2)) - b["veh"].astype(np.int64).sum(axis=(1, 2))) * step / 3600.0
    assert math.isclose(p["vehicle_hours"]["mean"], dvh.mean(), rel_tol=1e-12)
    if K > 1:
        assert math.isclose(p["vehicle_hours"]["se"], dvh.std(ddof=1) / math.sqrt(K), rel_tol=1e-12)
    assert "policy - dijkstra" in "\n".join(E.occupancy_lines(rep))
    other, _ = _result(K + 1, seed=2)
    with pytest.raises(ValueError, match="same environments"):
        E.occupancy_report(res, baseline=other)
    short, _ = _result(K, seed=2, frames=(60, 39))
    with pytest.raises(ValueError, match="same frames and bins"):
        E.occupancy_report(res, baseline=short)
    nothing = E.EvalResult(envs=K, head="dijkstra", deterministic=True, frames_run=100, settings=dict(res.settings))
    assert not E.occupancy_report(res, baseline=nothing)["summary"]["paired"]["available"]
    base.settings["seed"] = 4
    with pytest.raises(ValueError, match="seed"):
        E.occupancy_report(res, baseline=base)


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn", scenario="synthetic-1024-1024", mode="eval")
    base.update(kw)
    return RunnerArgs(**base)


def test_flag_defaults_and_refusals():
    main = importlib.import_module("main")
    assert main.build_parser().parse_args([]).eval_occupancy is False
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "4", "--eval-occupancy", "--eval-link-bin", "900"])
    from src.runner import RunnerArgs
    a = RunnerArgs(**vars(ns))
    assert a.eval_occupancy and a.eval_link_bin == 900 and not a.eval_link_counts
    assert _args().eval_occupancy is False
    assert _args(eval_envs=4, eval_occupancy=True).eval_occupancy
    assert _args(algo="dijkstra", dijkstra_envs=4, eval_occupancy=True).eval_occupancy
    with pytest.raises(ValueError, match="eval_occupancy"):
        _args(eval_occupancy=True)
    with pytest.raises(ValueError, match="eval_occupancy"):
        _args(algo="dijkstra", eval_occupancy=True)
    with pytest.raises(ValueError, match="eval_link_bin"):
        _args(eval_envs=4, eval_occupancy=True, eval_link_bin=0)


# ---- the entry point and its wrapper validate on the host ------------------------------------------------------------------------
def test_entry_point_validation():
    from tarl_hip import lib, ops
    assert "tarl_occupancy_accumulate" in lib.SIGNATURES
    assert 255 * ops.OCCUPANCY_MAX_FRAMES < 2 ** 31 <= 255 * (ops.OCCUPANCY_MAX_FRAMES + 2 ** 16)
    L = lib.load()
    null = None
    buf = torch.zeros(64)
    p = buf.data_ptr()      # sizes and bins are checked before anything is launched: the address is never dereferenced
    acc = L.tarl_occupancy_accumulate
    #        ring thr F  K  N  t0 step bin first H  veh full peak stream
    for i in (0, 1, 10, 11, 12):
        a = [p, p, 1, 1, 1, 0, 1, 10, 0, 1, p, p, p, null]
        a[i] = null
        assert acc(*a) == -1 and b"null" in L.tarl_last_error(), i
    assert acc(p, p, 0, 1, 1, 0, 1, 10, 0, 1, p, p, p, null) == -1 and b"F must be" in L.tarl_last_error()
    assert acc(p, p, ops.OCCUPANCY_MAX_FRAMES + 1, 1, 1, 0, 0, 10, 0, 1, p, p, p, null) == -1 and b"F must be" in L.tarl_last_error()
    assert acc(p, p, 1, 0, 1, 0, 1, 10, 0, 1, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 0, 0, 1, 10, 0, 1, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, 1, 10, 0, 0, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1 << 40, 1, 0, 1, 10, 0, 1, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1 << 20, 1 << 20, 0, 1, 10, 0, 1, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1 << 20, 1 << 10, 1 << 10, 0, 0, 10, 0, 1, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, 1, 0, 0, 1, p, p, p, null) == -1 and b"bin_seconds" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, -1, 10, 0, 1, p, p, p, null) == -1 and b"clock" in L.tarl_last_error()
    assert acc(p, p, 2, 1, 1, 9, 1, 10, 0, 1, p, p, p, null) == -1 and b"bin >= H" in L.tarl_last_error()      # frame 1 in bin 1
    assert acc(p, p, 2, 1, 1, 9, 1, 10, 1, 1, p, p, p, null) == -1 and b"below first_bin" in L.tarl_last_error()


def test_ops_wrapper_refuses_bad_arguments():
    from tarl_hip import lib, ops
    F, N, K, H = 4, 3, 2, 2
    ring, thr = torch.zeros((F, N, K)), torch.zeros(N, dtype=torch.int32)
    veh, full = torch.zeros((K, H, N), dtype=torch.int32), torch.zeros((K, H, N), dtype=torch.int32)
    peak = torch.zeros((K, 1, N), dtype=torch.int32)
    ok = dict(t0=100, timestep=1, bin_seconds=3600, first_bin=0)
    with pytest.raises(lib.TarlError, match="GPU"):                      # everything else in order: a host tensor is refused
        ops.occupancy_accumulate(ring, thr, veh, full, peak, **ok)
    with pytest.raises(TypeError, match="ring"):
        ops.occupancy_accumulate(ring.to(torch.float64), thr, veh, full, peak, **ok)
    with pytest.raises(TypeError, match="thr"):
        ops.occupancy_accumulate(ring, thr.to(torch.int64), veh, full, peak, **ok)
    with pytest.raises(TypeError, match="full"):
        ops.occupancy_accumulate(ring, thr, veh, full.to(torch.int64), peak, **ok)
    with pytest.raises(ValueError, match="ring"):
        ops.occupancy_accumulate(ring[0], thr, veh, full, peak, **ok)
    with pytest.raises(ValueError, match="thr"):
        ops.occupancy_accumulate(ring, thr[:2], veh, full, peak, **ok)
    with pytest.raises(ValueError, match="veh"):                        # env-major accumulators: (K, H, N), not (N, H, K)
        ops.occupancy_accumulate(ring, thr, torch.zeros((N, H, K), dtype=torch.int32), full, peak, **ok)
    with pytest.raises(ValueError, match="peak"):
        ops.occupancy_accumulate(ring, thr, veh, full, torch.zeros((K, H, N), dtype=torch.int32), **ok)
    with pytest.raises(ValueError, match="contiguous"):
        ops.occupancy_accumulate(ring.transpose(1, 2).contiguous().transpose(1, 2), thr, veh, full, peak, **ok)
    with pytest.raises(ValueError, match="bin out of range"):           # frames 2, 3 reach bin 2 of the 2 stored
        ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=7198, timestep=1, bin_seconds=3600, first_bin=0)
    with pytest.raises(ValueError, match="bin out of range"):           # the first frame lies below first_bin
        ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=100, timestep=1, bin_seconds=3600, first_bin=1)
    with pytest.raises(ValueError, match="frames"):
        ops.occupancy_accumulate(ring, thr, veh, full, peak, frames=5, **ok)
    with pytest.raises(ValueError, match="bin_seconds"):
        ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=100, timestep=1, bin_seconds=0)
    with pytest.raises(ValueError, match="timestep"):
        ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=100, timestep=-1)
