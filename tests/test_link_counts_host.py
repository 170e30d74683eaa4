"""CPU: the host side of the per-road link counts — the numpy restatement against hand-computed cases, the deliberate
defects against the crafted cases the GPU suite runs, link_count_report / link_count_lines against numpy, the flag refusals,
and the argument validation of the two entry points and their ops wrappers (nothing here launches a kernel)."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import link_counts_restatement as R
from conftest import ROOT


# ---- the restatement against hand-computed cases -------------------------------------------------------------------------------
def test_accumulate_restatement_by_hand():
    """Frames at the clocks 8, 9, 10 with bins of 10 s: the first two fall in bin 0, the third in bin 1 (the clock at which the
    frame STARTS). Road 0 is popped and withdrawn from in frame 1: that frame counts 2."""
    popped = np.array([[[1, 0]], [[1, 1]], [[0, 1]]], dtype=np.uint8)
    withdrawn = np.array([[[0, 0]], [[1, 0]], [[0, 1]]], dtype=np.uint8)
    counts = np.zeros((1, 2, 2), dtype=np.int32)
    R.accumulate(popped, withdrawn, counts, 8, 1, 10, 0)
    assert counts.tolist() == [[[3, 1], [0, 2]]]
    R.accumulate(popped[:1], withdrawn[:1], counts, 11, 1, 10, 0)         # a second call adds
    assert counts.tolist() == [[[3, 1], [1, 2]]]
    first, c = R.binned(popped, withdrawn, 8, 1, 10)
    assert first == 0 and c.tolist() == [[[3, 1], [0, 2]]]
    first, c = R.binned(popped, withdrawn, 21540, 1, 3600)                # EPISODE_START: the column is count_5h
    assert first == 5 and c.tolist() == [[[3, 3]]]
    # timestep 25, bins of 10 s: frames at 1000, 1025, 1050 -> bins 100, 102, 105; the bins between stay empty
    first, c = R.binned(popped, withdrawn, 1000, 25, 10)
    assert first == 100 and c.shape == (1, 6, 2)
    assert c[0].tolist() == [[1, 0], [0, 0], [2, 1], [0, 0], [0, 0], [0, 2]]


def test_stats_restatement_and_geh_by_hand():
    a = np.array([[[1], [2]], [[3], [6]]], dtype=np.int32)                # K = 2, H = 2, N = 1
    s = R.stats(a)
    assert s["sum"].tolist() == [[4], [8], [12]] and s["sumsq"].tolist() == [[10], [40], [90]]
    assert s["min"].tolist() == [[1], [2], [3]] and s["max"].tolist() == [[3], [6], [9]]
    assert s["sum"].dtype == np.int64 and s["min"].dtype == np.int32
    b = np.ones_like(a)
    d = R.stats(a, b)
    assert d["sum"].tolist() == [[2], [6], [8]] and d["sumsq"].tolist() == [[4], [26], [50]]
    assert d["min"].tolist() == [[0], [1], [1]] and d["max"].tolist() == [[2], [5], [7]]
    m = R.moments(a)
    assert m["mean"].tolist() == [[2.0], [4.0], [6.0]] and m["std"][2, 0] == math.sqrt(18.0)
    assert R.moments(a[:1])["std"] is None
    assert R.geh([10.0, 0.0, 8.0, 3.0], [10.0, 0.0, 0.0, 5.0]).tolist() == [0.0, 0.0, 4.0, 1.0]


def test_crafted_cases_cover_what_the_issue_lists():
    cases = {c["name"]: c for c in R.crafted_cases()}
    assert len(cases) == 4 * len(R.SHAPES) + 3
    for B, N, F in R.SHAPES:
        for kind in ("no-edge", "edge-first", "edge-last", "skipping"):
            c = cases[f"{B}x{N}x{F}-{kind}"]
            call, = c["calls"]
            assert call["popped"].shape == (F, B, N) and not call["partial"]
            bins = [(call["t0"] + f * c["timestep"]) // c["bin_seconds"] - c["first_bin"] for f in range(F)]
            assert 1 <= min(bins) and max(bins) <= c["H"] - 2              # an empty bin on either side
            if kind == "no-edge":
                assert len(set(bins)) == 1
            if kind == "edge-first":
                assert call["t0"] % c["bin_seconds"] == 0 and len(set(bins)) == 1
            if kind == "edge-last" and F > 1:
                assert bins[-1] == bins[0] + 1 and bins[-2] == bins[0]
            if kind == "skipping" and F > 1:
                assert len(set(bins)) == F and max(np.diff(bins)) == 3     # every frame a bin of its own, bins skipped
    assert any((B * N) % 4 for B, N, _ in R.SHAPES) and any(N % 2 for _, N, _ in R.SHAPES)
    two = cases["two-calls"]
    assert [c["popped"].shape[0] for c in two["calls"]] == [64, 30] and two["calls"][1]["partial"]
    last_of_first = (two["calls"][0]["t0"] + 63) // 3600
    assert two["calls"][0]["t0"] // 3600 == last_of_first - 1 and two["calls"][1]["t0"] // 3600 == last_of_first
    still = cases["5x6x7-timestep-0"]                                      # the clock stands still: one bin holds every frame
    assert still["timestep"] == 0 and still["calls"][0]["popped"].shape == (7, 5, 6) and still["H"] == 3
    got = R.run_case(still)
    assert not got[:, 0].any() and not got[:, 2].any()
    assert np.array_equal(got[:, 1], (still["calls"][0]["popped"].astype(np.int32) + still["calls"][0]["withdrawn"]).sum(axis=0))
    ones = cases["all-ones-max-F-twice"]
    assert [c["popped"].shape for c in ones["calls"]] == [(R.MAX_FRAMES, 1, 5)] * 2
    got = R.run_case(ones)
    assert got[:, 1, :].tolist() == [[4 * R.MAX_FRAMES] * 5] and int(got.sum()) == 5 * 4 * R.MAX_FRAMES


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_noticed_by_the_crafted_cases(defect):
    """What the GPU cases compare against is the true restatement; an implementation with one of these defects computes the
    defective restatement, so a defect the crafted inputs cannot tell from the truth would pass unseen."""
    differing = [c["name"] for c in R.crafted_cases() if not np.array_equal(R.run_case(c), R.run_case(c, defect=defect))]
    print(f"[defect {defect}] noticed by {len(differing)} cases: {differing}")
    assert differing
    if defect in ("overwrite_second_block", "skip_partial_block"):
        assert "two-calls" in differing
    if defect == "saturate_255":
        assert differing == ["all-ones-max-F-twice"]
    if defect == "clock_after_step":
        assert any(n.endswith("edge-last") for n in differing) and any(n.endswith("skipping") for n in differing)


# ---- link_count_report / link_count_lines against numpy -------------------------------------------------------------------------
def _result(K, H=2, N=6, seed=0, head="embedding", first_bin=5, bin_seconds=3600):
    from tarl_hip.evaluator import EvalResult, link_moments
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 40, size=(K, H, N)).astype(np.int32)
    a[:, :, 3] = 0                                  # a road nobody used
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=300, settings=dict(seed=3, env_base=0))
    res.link_counts, res.link_first_bin, res.link_bin_seconds = a, first_bin, bin_seconds
    res.link_stats = link_moments(R.stats(a), K)
    return res, a


@pytest.mark.parametrize("K", [1, 2, 5])
def test_link_moments_against_numpy(K):
    from tarl_hip.evaluator import link_moments
    _, a = _result(K, seed=K)
    got = link_moments(R.stats(a), K)
    R.assert_moments_close(got, R.moments(a), K)
    assert got["n"] == K and np.array_equal(got["min"], R.stats(a)["min"])
    b = np.roll(a, 1, axis=2)
    R.assert_moments_close(link_moments(R.stats(a, b), K), R.moments(a, b), K)


def test_report_against_numpy_with_zero_expected_flow_and_a_constant_vector():
    from tarl_hip.evaluator import LINK_PARTIAL_NOTE, link_count_lines, link_count_report, link_count_summary
    K, H, N = 5, 2, 6
    res, a = _result(K)
    msa = {0: 30.0, 1: 0.0, 2: 45.5, 3: 0.0, 4: 12.0}           # road 5 missing (0), road 3: simulated 0 and expected 0
    ue = np.full(N, 7.0)                                       # a constant vector: no correlation
    rep = link_count_report(res, expected={"msa": msa, "ue": ue})
    assert rep["available"] and rep["bins"] == ["count_5h", "count_6h"] and rep["note"] == LINK_PARTIAL_NOTE
    assert rep["columns"] == ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max", "count_5h", "count_6h",
                              "expected_msa", "diff_msa", "geh_msa", "ue_flow", "diff_ue", "geh_ue"]
    tot = a.sum(axis=1).astype(np.float64)                      # (K, N)
    c = np.array([30.0, 0.0, 45.5, 0.0, 12.0, 0.0])
    mean, sd = tot.mean(axis=0), tot.std(axis=0, ddof=1)
    g = R.geh(mean, c)
    for n, row in enumerate(rep["rows"]):
        assert set(row) == set(rep["columns"]) and row["road"] == n
        assert row["mean"] == mean[n] and row["min"] == tot[:, n].min() and row["max"] == tot[:, n].max()
        assert math.isclose(row["sd"], sd[n], rel_tol=1e-12, abs_tol=1e-9)
        assert math.isclose(row["se"], sd[n] / math.sqrt(K), rel_tol=1e-12, abs_tol=1e-9)
        assert math.isclose(row["ci95_lo"], mean[n] - 1.96 * sd[n] / math.sqrt(K), rel_tol=1e-12, abs_tol=1e-9)
        assert row["count_5h"] == a[:, 0, n].mean() and row["count_6h"] == a[:, 1, n].mean()
        assert row["expected_msa"] == c[n] and row["diff_msa"] == mean[n] - c[n]
        assert math.isclose(row["geh_msa"], g[n], rel_tol=1e-12, abs_tol=0.0)
        assert row["ue_flow"] == 7.0
    assert rep["rows"][3]["geh_msa"] == 0.0 and rep["rows"][3]["mean"] == 0.0       # both 0: GEH 0, not nan
    s = rep["summary"]
    assert s["envs"] == K and s["roads"] == N and s["frames_run"] == 300 and s["roads_counted"] == N - 1
    e = s["expected"]["msa"]
    d = mean - c
    assert math.isclose(e["rmse"], math.sqrt((d * d).mean()), rel_tol=1e-12)
    assert math.isclose(e["mean_abs_diff"], np.abs(d).mean(), rel_tol=1e-12)
    assert e["geh_below_5_share"] == float((g < 5).mean())
    assert math.isclose(e["pearson"], np.corrcoef(mean, c)[0, 1], rel_tol=1e-9)
    assert math.isclose(e["total_ratio"], mean.sum() / c.sum(), rel_tol=1e-12)
    assert math.isnan(s["expected"]["ue"]["pearson"])
    assert link_count_summary(rep)["summary"]["expected"]["ue"]["pearson"] is None and "rows" not in link_count_summary(rep)
    text = "\n".join(link_count_lines(rep))
    assert "vs msa:" in text and "vs ue:" in text and "part of the demand" in text and "GEH < 5" in text
    # no expected flows (the MSA block was skipped): no comparison columns, and the block says so
    bare = link_count_report(res)
    assert bare["columns"] == ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max", "count_5h", "count_6h"]
    assert "not available" in "\n".join(link_count_lines(bare)) and bare["summary"]["expected"] == {}
    with pytest.raises(ValueError, match="named among"):
        link_count_report(res, expected={"other": ue})
    with pytest.raises(ValueError, match="one value per road"):
        link_count_report(res, expected={"so": np.zeros(N + 1)})
    # bins that are not hours are named by their absolute number
    res25, _ = _result(2, first_bin=861, bin_seconds=25)
    assert link_count_report(res25)["bins"] == ["count_bin861", "count_bin862"]


def test_report_for_one_environment_and_for_a_run_without_counts():
    from tarl_hip.evaluator import EvalResult, link_count_lines, link_count_report
    res, a = _result(1)
    rep = link_count_report(res, expected={"msa": np.ones(6)})
    for n, row in enumerate(rep["rows"]):
        assert row["mean"] == float(a[0, :, n].sum()) and row["min"] == row["max"] == int(a[0, :, n].sum())
        assert row["sd"] is None and row["se"] is None and row["ci95_lo"] is None and row["ci95_hi"] is None
    assert link_count_lines(rep)
    gone = EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64, domain_exit=True,
                      domain_exit_frames=(0, 64))
    rep = link_count_report(gone)
    assert not rep["available"] and "domain" in rep["reason"] and "not available" in link_count_lines(rep)[0]
    assert not link_count_report(EvalResult(envs=2, head="embedding", deterministic=True, frames_run=64))["available"]


@pytest.mark.parametrize("K", [1, 4])
def test_paired_report_against_numpy(K, monkeypatch):
    """The paired numbers come from the two-input statistics kernel; here its numpy restatement stands in for the launch, so
    that the host arithmetic behind it is checked without a GPU."""
    from tarl_hip import eval_reports, evaluator as E
    monkeypatch.setattr(eval_reports, "_paired_moments", lambda a, b, K: E.link_moments(R.stats(a, b), K))
    res, a = _result(K, seed=1)
    base, b = _result(K, seed=2, head="dijkstra")
    rep = E.link_count_report(res, baseline=base)
    assert rep["columns"][-5:] == ["baseline_mean", "paired_diff_mean", "paired_diff_se", "paired_diff_ci95_lo",
                                   "paired_diff_ci95_hi"]
    d = (a.astype(np.int64) - b).sum(axis=1).astype(np.float64)            # (K, N)
    excl = 0
    for n, row in enumerate(rep["rows"]):
        assert row["baseline_mean"] == b[:, :, n].sum(axis=1).mean() and row["paired_diff_mean"] == d[:, n].mean()
        if K == 1:
            assert row["paired_diff_se"] is None and row["paired_diff_ci95_lo"] is None
            continue
        se = d[:, n].std(ddof=1) / math.sqrt(K)
        assert math.isclose(row["paired_diff_se"], se, rel_tol=1e-12, abs_tol=1e-9)
        excl += (d[:, n].mean() - 1.96 * se > 0) or (d[:, n].mean() + 1.96 * se < 0)
    p = rep["summary"]["paired"]
    assert p["available"] and p["baseline_head"] == "dijkstra"
    assert p["roads_interval_excludes_zero"] == (None if K == 1 else excl)
    assert "policy - dijkstra" in "\n".join(E.link_count_lines(rep))
    other, _ = _result(K + 1, seed=2)
    with pytest.raises(ValueError, match="same environments"):
        E.link_count_report(res, baseline=other)
    base.settings["seed"] = 4
    with pytest.raises(ValueError, match="seed"):
        E.link_count_report(res, baseline=base)


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn", scenario="synthetic-1024-1024", mode="eval")
    base.update(kw)
    return RunnerArgs(**base)


def test_flags_defaults_and_refusals():
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.eval_link_counts is False and ns.eval_link_bin == 3600
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "4", "--eval-link-counts", "--eval-link-bin", "900"])
    from src.runner import RunnerArgs
    a = RunnerArgs(**vars(ns))
    assert a.eval_link_counts and a.eval_link_bin == 900
    assert _args().eval_link_counts is False and _args().eval_link_bin == 3600
    assert _args(eval_envs=4, eval_link_counts=True).eval_link_counts
    assert _args(algo="dijkstra", dijkstra_envs=4, eval_link_counts=True).eval_link_counts
    with pytest.raises(ValueError, match="eval_link_counts"):
        _args(eval_link_counts=True)
    with pytest.raises(ValueError, match="eval_link_counts"):
        _args(algo="dijkstra", eval_link_counts=True)
    for bad in (0, -5, None):
        with pytest.raises(ValueError, match="eval_link_bin"):
            _args(eval_envs=4, eval_link_counts=True, eval_link_bin=bad)


# ---- the entry points and their wrappers validate on the host ------------------------------------------------------------------
def test_declared_maximum_and_entry_point_validation():
    from tarl_hip import lib, ops
    hdr = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert int(re.search(r"#define TARL_LINK_COUNTS_MAX_FRAMES (\d+)", hdr).group(1)) == ops.LINK_COUNTS_MAX_FRAMES == R.MAX_FRAMES
    assert 2 * ops.LINK_COUNTS_MAX_FRAMES <= 255            # 8-bit partial sums, at most 2 per frame
    assert "tarl_link_counts_accumulate" in lib.SIGNATURES and "tarl_link_count_stats" in lib.SIGNATURES
    L = lib.load()
    null = None
    buf = torch.zeros(64)
    p = buf.data_ptr()      # sizes and bins are checked before anything is launched: the address is never dereferenced
    acc = L.tarl_link_counts_accumulate
    assert acc(null, p, 1, 1, 1, 0, 1, 10, 0, 1, p, null) == -1 and b"null" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, 1, 10, 0, 1, null, null) == -1 and b"null" in L.tarl_last_error()
    assert acc(p, p, 0, 1, 1, 0, 1, 10, 0, 1, p, null) == -1 and b"MAX_FRAMES" in L.tarl_last_error()
    assert acc(p, p, 128, 1, 1, 0, 1, 10, 0, 1, p, null) == -1 and b"MAX_FRAMES" in L.tarl_last_error()
    assert acc(p, p, 1, 0, 1, 0, 1, 10, 0, 1, p, null) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, 1, 0, 0, 1, p, null) == -1 and b"bin_seconds" in L.tarl_last_error()
    assert acc(p, p, 1, 1, 1, 0, -1, 10, 0, 1, p, null) == -1 and b"clock" in L.tarl_last_error()
    assert acc(p, p, 2, 1, 1, 9, 1, 10, 0, 1, p, null) == -1 and b"bin >= H" in L.tarl_last_error()      # frame 1 in bin 1
    assert acc(p, p, 2, 1, 1, 9, 1, 10, 1, 1, p, null) == -1 and b"below first_bin" in L.tarl_last_error()
    st = L.tarl_link_count_stats
    assert st(null, null, 1, 1, 1, p, p, p, p, null) == -1 and b"null" in L.tarl_last_error()
    assert st(p, null, 1, 1, 1, p, p, p, null, null) == -1 and b"null" in L.tarl_last_error()
    assert st(p, null, 0, 1, 1, p, p, p, p, null) == -1 and b"bad sizes" in L.tarl_last_error()


def test_ops_wrappers_refuse_bad_arguments():
    from tarl_hip import lib, ops
    F, B, N, H = 4, 2, 3, 2
    pop, wd = torch.zeros((F, B, N), dtype=torch.uint8), torch.zeros((F, B, N), dtype=torch.uint8)
    counts = torch.zeros((B, H, N), dtype=torch.int32)
    ok = dict(t0=100, timestep=1, bin_seconds=3600, first_bin=0)
    with pytest.raises(lib.TarlError, match="GPU"):                      # everything else in order: a host tensor is refused
        ops.link_counts_accumulate(pop, wd, counts, **ok)
    with pytest.raises(TypeError, match="popped"):
        ops.link_counts_accumulate(pop.to(torch.int32), wd, counts, **ok)
    with pytest.raises(TypeError, match="counts"):
        ops.link_counts_accumulate(pop, wd, counts.to(torch.int64), **ok)
    with pytest.raises(ValueError, match="withdrawn"):
        ops.link_counts_accumulate(pop, wd[:, :1], counts, **ok)
    with pytest.raises(ValueError, match="counts"):
        ops.link_counts_accumulate(pop, wd, torch.zeros((B, H, N + 1), dtype=torch.int32), **ok)
    with pytest.raises(ValueError, match="popped"):
        ops.link_counts_accumulate(pop[0], wd[0], counts, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        ops.link_counts_accumulate(pop.transpose(1, 2).contiguous().transpose(1, 2), wd, counts, **ok)
    with pytest.raises(ValueError, match="bin out of range"):           # frames 2, 3 reach bin 2 of the 2 stored
        ops.link_counts_accumulate(pop, wd, counts, t0=7198, timestep=1, bin_seconds=3600, first_bin=0)
    with pytest.raises(ValueError, match="bin out of range"):           # the first frame lies below first_bin
        ops.link_counts_accumulate(pop, wd, counts, t0=100, timestep=1, bin_seconds=3600, first_bin=1)
    with pytest.raises(ValueError, match="frames"):
        ops.link_counts_accumulate(pop, wd, counts, frames=5, **ok)
    big = torch.zeros((ops.LINK_COUNTS_MAX_FRAMES + 1, 1, 1), dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 127"):
        ops.link_counts_accumulate(big, big, torch.zeros((1, 1, 1), dtype=torch.int32), **ok)
    a = torch.zeros((3, H, N), dtype=torch.int32)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.link_count_stats(a)
    with pytest.raises(TypeError, match="counts_a"):
        ops.link_count_stats(a.to(torch.int64))
    with pytest.raises(ValueError, match="counts_b"):
        ops.link_count_stats(a, a[:2])
    with pytest.raises(ValueError, match="counts_a"):
        ops.link_count_stats(a[0])
    with pytest.raises(ValueError, match="sum"):
        ops.link_count_stats(a, out={"sum": torch.zeros((H, N), dtype=torch.int64)})
