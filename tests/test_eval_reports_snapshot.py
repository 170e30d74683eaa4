"""CPU: everything the evaluation reports return, print and write, pinned to a recorded snapshot — link_count_report,
occupancy_report, trip_report with their ``*_lines`` and ``*_summary``, paired_report / paired_lines / paired_scalars and
EvalResult.summary_lines on small seeded results (6 roads, 2 time bins, 8 agents; 1 and 4 environments): without a baseline,
with one, with one that lacks the data, with and without free-flow times, and after a domain exit. The comparison is exact:
both sides as JSON text, which keeps every float64 bit, the order of the keys (the columns of the CSV files) and nan, which
only a ``*_summary`` turns into null. The numpy restatement of the two-input statistics kernel stands in for its launch, as in
the host tests of the reports. tests/golden/eval_reports_snapshot.json was recorded by :func:`build_snapshot` from the reports
as they were before their shared pieces were factored out."""
import json
import os

import numpy as np
import pytest

import link_counts_restatement as LR
import trips_restatement as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_reports_snapshot.json")
N, H, A = 6, 2, 8                               # roads, time bins, agents (the tables hold the dummy row 0 as well)
FIRST_BIN, BIN_SECONDS, STEP, FRAMES = 5, 3600, 2, (60, 40)
MAX_AGENTS = np.array([0.0, 3.0, 8.0, 14.0, 14.0, 5.0])
SETTINGS = dict(seed=3, env_base=0, bin_width=10.0, num_bins=720)


def _agents(rng, K, population=None, none_in_last=False):
    """Agent tables (K, A + 1, 9): one population, per environment who arrived and when. Agent 1 arrives nowhere, agent 2 in
    environment 0 only, agent 3 everywhere; ``none_in_last``: the last environment sees no arrival at all."""
    ag = np.zeros((K, A + 1, 9), dtype=np.float32)
    if population is None:
        population = np.stack([rng.integers(0, N, A + 1), rng.integers(0, N, A + 1),
                               rng.integers(FIRST_BIN * BIN_SECONDS, (FIRST_BIN + H) * BIN_SECONDS - 1000, A + 1)], axis=1)
        population[0] = 0
    ag[:, :, :3] = population[None]
    done = rng.random((K, A + 1)) < 0.7
    done[:, 1], done[:, 2], done[0, 2], done[:, 3] = False, False, True, True
    if none_in_last:
        done[-1] = False
    done[:, 0] = False
    tt = rng.integers(30, 900, (K, A + 1)).astype(np.float32) + rng.integers(0, 2, (K, A + 1)) * 0.5
    ag[:, :, TR.ARR] = np.where(done, ag[:, :, TR.DEP] + tt, 0.0)
    ag[:, :, TR.DONE] = done
    ag[:, :, TR.ON_WAY] = ~done & (rng.random((K, A + 1)) < 0.5)
    ag[:, 0, TR.ON_WAY] = 0
    return ag


def _result(K, seed, head, free_flow=None, population=None, pair=None, none_in_last=False):
    """An EvalResult as VecEvaluator(link_counts=True, occupancy=True, trips=True).run(trip_pair=pair) leaves it -> (result,
    its agent tables)."""
    from tarl_hip.evaluator import EvalResult, capacity_threshold, link_moments, summarise
    rng = np.random.default_rng(seed)
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=sum(FRAMES), settings=dict(SETTINGS))
    res.link_counts = rng.integers(0, 40, size=(K, H, N)).astype(np.int32)
    res.link_counts[:, :, 3] = 0                    # a road nobody used
    res.link_first_bin, res.link_bin_seconds = FIRST_BIN, BIN_SECONDS
    res.link_stats = link_moments(LR.stats(res.link_counts), K)
    thr = capacity_threshold(MAX_AGENTS)
    veh = np.stack([rng.integers(0, 12 * f, size=(K, N)) for f in FRAMES], axis=1).astype(np.int32)
    full = np.stack([rng.integers(0, f + 1, size=(K, N)) for f in FRAMES], axis=1).astype(np.int32)
    full[:, :, thr <= 0] = np.asarray(FRAMES, dtype=np.int32)[None, :, None]
    res.occupancy = {"veh": veh, "full": full, "peak": rng.integers(1, 15, size=(K, 1, N)).astype(np.int32)}
    res.occupancy_stats = {k: link_moments(LR.stats(v), K) for k, v in res.occupancy.items()}
    res.occupancy_frames_per_bin = list(FRAMES)
    res.occupancy_meta = dict(first_bin=FIRST_BIN, bin_seconds=BIN_SECONDS, timestep=STEP, max=MAX_AGENTS, thr=thr)
    ag = _agents(rng, K, population, none_in_last)
    res.trips = TR.agent_stats(ag, pair, free_flow)
    res.trip_bins = TR.bin_stats(ag, BIN_SECONDS, FIRST_BIN, H, free_flow)
    res.trip_meta = dict(first_bin=FIRST_BIN, bin_seconds=BIN_SECONDS, origin=ag[0, :, 0].astype(np.int64),
                         destination=ag[0, :, 1].astype(np.int64), departure=ag[0, :, 2].copy(), free_flow=free_flow,
                         paired=pair is not None)
    # the per-environment lists and their aggregate, by summarise() from what tarl_episode_summary would have returned
    done = ag[:, 1:, TR.DONE] == 1
    tt = (ag[:, 1:, TR.ARR] - ag[:, 1:, TR.DEP]).astype(np.float64) * done
    counts = np.stack([done.sum(axis=1), (ag[:, 1:, TR.ON_WAY] == 1).sum(axis=1), (~done).sum(axis=1)], axis=1)
    sums = np.stack([tt.sum(axis=1), (tt * tt).sum(axis=1), tt.max(axis=1)], axis=1)
    hist = np.stack([np.bincount((tt[k][done[k]] // 10).astype(np.int64), minlength=720)[:720] for k in range(K)])
    ret = -veh.astype(np.int64).sum(axis=(1, 2)).astype(np.float64)          # the identity of the occupancy report holds
    per, res.aggregate, res.envs_without_arrival = summarise(counts, sums, ret, hist, sum(FRAMES), 10.0)
    for k, v in per.items():
        setattr(res, k, v)
    return res, ag


def _nan_as_null(v):
    if isinstance(v, dict):
        return {k: _nan_as_null(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_nan_as_null(x) for x in v]
    return None if isinstance(v, float) and not np.isfinite(v) else v


def _table(rows):
    """A list of dicts with one key order (the rows of a CSV file) as that order and the values: nothing is lost."""
    keys = list(rows[0]) if rows else []
    assert all(list(r) == keys for r in rows)
    return {"keys": keys, "values": [list(r.values()) for r in rows]}


def build_snapshot():
    """{case: what the reports return for it}, plain JSON apart from nan. The caller has replaced the paired-statistics
    launch of the reports by its numpy restatement."""
    from tarl_hip import evaluator as E
    out = {}
    for K in (1, 4):
        ff = np.random.default_rng(50 + K).integers(20, 400, A + 1).astype(np.float64)
        ff[0] = ff[5] = np.inf
        res, ag = _result(K, 10 + K, "embedding", free_flow=ff, none_in_last=K > 1)
        no_ff, _ = _result(K, 10 + K, "embedding", none_in_last=K > 1)
        base, _ = _result(K, 20 + K, "dijkstra", free_flow=ff, population=ag[0, :, :3], pair=ag)
        unpaired, _ = _result(K, 20 + K, "dijkstra", free_flow=ff, population=ag[0, :, :3])
        lacking = E.EvalResult(envs=K, head="dijkstra", deterministic=True, frames_run=sum(FRAMES), settings=dict(SETTINGS))
        gone = E.EvalResult(envs=K, head="embedding", deterministic=True, frames_run=64, domain_exit=True,
                            domain_exit_frames=(0, 64), settings=dict(SETTINGS))
        expected = {"msa": {0: 30.0, 1: 0.0, 2: 45.5, 3: 0.0, 4: 12.0}, "ue": np.full(N, 7.0)}       # ue: constant, Pearson nan
        reports = {
            "link/alone": E.link_count_report(res, expected=expected), "link/no-expected": E.link_count_report(res),
            "link/baseline": E.link_count_report(res, expected=expected, baseline=base),
            "link/baseline-lacking": E.link_count_report(res, baseline=lacking), "link/domain-exit": E.link_count_report(gone),
            "occupancy/alone": E.occupancy_report(res), "occupancy/baseline": E.occupancy_report(res, baseline=base),
            "occupancy/baseline-lacking": E.occupancy_report(res, baseline=lacking),
            "occupancy/domain-exit": E.occupancy_report(gone),
            "trips/alone": E.trip_report(res), "trips/no-free-flow": E.trip_report(no_ff),
            "trips/baseline": E.trip_report(res, baseline=base), "trips/baseline-unpaired": E.trip_report(res, baseline=unpaired),
            "trips/baseline-lacking": E.trip_report(res, baseline=lacking), "trips/domain-exit": E.trip_report(gone)}
        seen = {}
        for name, rep in reports.items():
            kind, variant = name.split("/")
            if K == 1 and variant not in ("alone", "baseline", "domain-exit"):      # one environment: the paths without a spread
                continue
            lines, summary = {"link": (E.link_count_lines, E.link_count_summary), "occupancy": (E.occupancy_lines, E.occupancy_summary),
                              "trips": (E.trip_lines, E.trip_summary)}[kind]
            # the summary is what the runner writes into its JSON file: the report without its tables, nan and inf as null
            slim = {k: v for k, v in rep.items() if k not in ("rows", "by_departure")}
            assert json.dumps(summary(rep), allow_nan=False) == json.dumps(_nan_as_null(slim)), name
            rep, text = dict(rep), lines(rep)
            for table in ("rows", "by_departure"):      # stored as keys + values, and once if an earlier case holds the same
                if table in rep:
                    rep[table] = _table(rep[table])
                    first = seen.setdefault((kind, table, json.dumps(rep[table])), name)
                    if first != name:
                        rep[table] = {"same_as": first}
            out[f"K{K}/{name}"] = {"report": rep, "lines": text}
        for name, other in (("baseline", base), ("domain-exit", gone)):
            rep = E.paired_report(res, other)
            out[f"K{K}/paired/{name}"] = {"report": rep, "lines": E.paired_lines(rep), "scalars": E.paired_scalars(rep)}
        out[f"K{K}/summary_lines"] = {"run": res.summary_lines(), "baseline": base.summary_lines(), "domain-exit": gone.summary_lines()}
    return out


@pytest.fixture(scope="module")
def snapshot():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_reports_equal_the_recorded_snapshot(snapshot, monkeypatch):
    from tarl_hip import eval_reports, evaluator as E
    monkeypatch.setattr(eval_reports, "_paired_moments", lambda a, b, K: E.link_moments(LR.stats(a, b), K))
    got = build_snapshot()
    assert sorted(got) == sorted(snapshot) and len(got) == (9 + 15) + 2 * (2 + 1)
    for name, want in snapshot.items():
        assert list(got[name]) == list(want), name
        for part in want:
            assert json.dumps(got[name][part]) == json.dumps(want[part]), (name, part)
    # the snapshot holds the situations it is there for
    for kind in ("link", "occupancy", "trips"):
        assert snapshot[f"K4/{kind}/baseline"]["report"]["summary"]["paired"]["available"]
        assert not snapshot[f"K4/{kind}/baseline-lacking"]["report"]["summary"]["paired"]["available"]
        assert "paired" not in snapshot[f"K4/{kind}/alone"]["report"]["summary"]
        assert not snapshot[f"K4/{kind}/domain-exit"]["report"]["available"]
    assert not snapshot["K4/trips/baseline-unpaired"]["report"]["summary"]["paired"]["available"]
    assert snapshot["K4/trips/alone"]["report"]["summary"]["free_flow"] and not snapshot["K4/trips/no-free-flow"]["report"]["summary"]["free_flow"]
    assert snapshot["K1/link/baseline"]["report"]["rows"]["values"][0][2] is None                # one environment: no sd
    assert snapshot["K4/paired/baseline"]["report"]["metrics"]["mean_travel_time"]["dropped"] == 1
    assert str(snapshot["K4/link/alone"]["report"]["summary"]["expected"]["ue"]["pearson"]) == "nan"
