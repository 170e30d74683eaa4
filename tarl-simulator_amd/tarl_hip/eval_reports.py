"""The reports of the vectorised evaluation beyond the per-environment aggregate — per-road link counts, per-road occupancy
and time at capacity, per-trip travel times, the dynamic relative gap, per-turn movement counts — each as ``*_report`` (rows and a summary, formed in float64 on the host from the
kernels' integer accumulators), ``*_lines`` (its printable block) and ``*_summary`` (what the JSON files carry), and the pieces
they share. :mod:`tarl_hip.evaluator` re-exports every public name and is never imported here: an ``EvalResult`` is only read."""
from __future__ import annotations

import math
from functools import partial

import numpy as np
import torch

from . import ops

_CI95_KIND = "normal approximation, mean -+ 1.96 se"


# ---- shared pieces ----------------------------------------------------------------------------------------------------------------
def _sample_moments(v):
    """mean, std (ddof = 1), se = std / sqrt(n), ci95 = mean -+ 1.96 se of a float64 vector; ``None`` below 1 / 2 values."""
    out = {"mean": None, "std": None, "se": None, "ci95": None}
    if v.size >= 1:
        out["mean"] = float(v.mean())
    if v.size >= 2:
        std = float(v.std(ddof=1))
        se = std / math.sqrt(v.size)
        out.update(std=std, se=se, ci95=(out["mean"] - 1.96 * se, out["mean"] + 1.96 * se))
    return out


def aggregate(values):
    """Mean and spread of one per-environment quantity over the K environments. ``None`` entries (an environment without
    an arrival has no travel time) are left out and counted in ``missing``. ``std`` is the sample standard deviation
    (ddof = 1), ``se = std / sqrt(n)``, ``ci95 = mean -+ 1.96 se``: a NORMAL-APPROXIMATION interval, ``None`` (like std and
    se) when fewer than two environments contribute."""
    v = np.asarray([x for x in values if x is not None], dtype=np.float64)
    out = {"n": int(v.size), "missing": int(len(values) - v.size), "mean": None, "std": None, "se": None, "min": None,
           "max": None, "ci95": None, "ci95_kind": _CI95_KIND}
    if v.size:
        out.update(_sample_moments(v), min=float(v.min()), max=float(v.max()))
    return out


def _interval(g):
    """The spread of an :func:`aggregate`-like dict as the text behind its mean; empty without a standard error."""
    return "" if g["se"] is None else f"  +- {g['se']:.3f} (se)  95% [{g['ci95'][0]:.3f}, {g['ci95'][1]:.3f}] (normal approx.)"


def _unavailable(result: "EvalResult", data, why):
    """The report of a run without ``data`` (a domain exit has no statistics; otherwise ``why``); ``None`` if it has it."""
    if result.domain_exit:
        return {"available": False, "reason": "a run that left the domain has no statistics"}
    return {"available": False, "reason": why} if data is None else None


def _check_pair(fn_name, result: "EvalResult", baseline: "EvalResult"):
    """``ValueError`` unless ``baseline`` ran on the environments of ``result``: same K, seed and env_base."""
    if baseline.envs != result.envs:
        raise ValueError(f"{fn_name} needs the same environments: envs {result.envs} / {baseline.envs}")
    for k in ("seed", "env_base"):
        if result.settings.get(k) != baseline.settings.get(k):
            raise ValueError(f"{fn_name} needs equal {k}: {result.settings.get(k)!r} / {baseline.settings.get(k)!r}")


def _paired_moments(a, b, K):
    """:func:`link_moments` of a - b per environment, two int32 (K, H, N) arrays, by the two-input statistics kernel."""
    dev = torch.device("cuda")
    st = ops.link_count_stats(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    return link_moments({k: v.cpu().numpy() for k, v in st.items()}, K)


def _json_clean(v):
    """``v`` as plain JSON: dicts, lists and tuples (as lists) recursed, nan and +-inf as ``None``."""
    if isinstance(v, dict):
        return {k: _json_clean(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_clean(x) for x in v]
    return None if isinstance(v, float) and not math.isfinite(v) else v


def _summary(report: dict):
    """A report without its tables (``rows``, ``by_departure``), nan and inf as ``None``: what the JSON files carry."""
    return _json_clean({k: v for k, v in report.items() if k not in ("rows", "by_departure")})


def _spread(prefix, m, row, n, scale=1.0, sd=True):
    """``<prefix>sd`` (if ``sd``), ``se``, ``ci95_lo``, ``ci95_hi`` at (row, n) of :func:`link_moments`; ``None`` for K = 1."""
    return {prefix + name: None if m[key] is None else float(m[key][row, n]) * scale
            for name, key in (("sd", "std"), ("se", "se"), ("ci95_lo", "ci95_lo"), ("ci95_hi", "ci95_hi"))[0 if sd else 1:]}


def _bin_names(prefix, first_bin, num_bins, bin_seconds):
    """Names of the stored bins, by ABSOLUTE bin: ``<prefix>5h``, ``<prefix>6h`` for hourly bins, ``<prefix>bin<k>`` else."""
    return [f"{prefix}{first_bin + h}h" if int(bin_seconds) == 3600 else f"{prefix}bin{first_bin + h}" for h in range(num_bins)]


link_bin_names = partial(_bin_names, "count_")        # (first_bin, num_bins, bin_seconds) -> the link-count columns
occupancy_bin_names = partial(_bin_names, "occ_")     # ... the occupancy columns
trip_bin_names = partial(_bin_names, "")              # ... the labels of the by-departure table
turn_bin_names = partial(_bin_names, "turns_")        # ... the turn-count columns


# ---- per-road link counts (VecEvaluator(link_counts=True)) --------------------------------------------------------------------
LINK_RING_BYTES = 256 << 20         # both mask rings of the evaluator together
LINK_EXPECTED = {"msa": "expected_msa", "ue": "ue_flow", "so": "so_flow"}      # expected-flow vector -> its column
LINK_PARTIAL_NOTE = ("counts are not rescaled: a run shorter than the demand's horizon sees only part of the demand, so the "
                     "simulated totals fall short of the expected flows by the trips that had not yet passed")


def link_moments(ints, K):
    """Host side of ``ops.link_count_stats``: its integer arrays ``sum``, ``sumsq`` (int64), ``min``, ``max`` (int32), each
    (H + 1, N) with the episode total in the last row, -> the same plus ``mean`` and, for K >= 2, the sample standard
    deviation ``std`` (ddof = 1, from the exact integer K sum d^2 - (sum d)^2), ``se = std / sqrt(K)`` and ``ci95_lo`` /
    ``ci95_hi = mean -+ 1.96 se`` (normal approximation), all float64; ``None`` for K = 1, as in :func:`aggregate`."""
    K = int(K)
    s, q = np.asarray(ints["sum"], dtype=np.int64), np.asarray(ints["sumsq"], dtype=np.int64)
    out = {"n": K, "sum": s, "sumsq": q, "min": np.asarray(ints["min"], dtype=np.int32),
           "max": np.asarray(ints["max"], dtype=np.int32), "mean": s / float(K), "std": None, "se": None, "ci95_lo": None,
           "ci95_hi": None}
    if K >= 2:
        std = np.sqrt((K * q - s * s) / float(K * (K - 1)))
        se = std / math.sqrt(K)
        out.update(std=std, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def geh(m, c):
    """The GEH statistic ``sqrt(2 (m - c)^2 / (m + c))`` of a simulated count m against an expected count c, elementwise;
    0 where both are 0."""
    m, c = np.asarray(m, dtype=np.float64), np.asarray(c, dtype=np.float64)
    tot = m + c
    return np.sqrt(2.0 * (m - c) ** 2 / np.where(tot == 0, 1.0, tot)) * (tot != 0)


def _flow_vector(flows, N, name):
    if isinstance(flows, dict):
        v = np.zeros(N, dtype=np.float64)
        for road, flow in flows.items():
            if 0 <= int(road) < N:
                v[int(road)] = float(flow)
        return v
    v = np.asarray(flows, dtype=np.float64).reshape(-1)
    if v.size != N:
        raise ValueError(f"expected flows {name!r} must hold one value per road ({N}), got {v.size}")
    return v


def _pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    den = math.sqrt(float((a * a).sum()) * float((b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


def link_count_report(result: "EvalResult", expected=None, baseline: "EvalResult | None" = None) -> dict:
    """Per-road rows and a summary of the link counts of one evaluation (``VecEvaluator(link_counts=True)``).
    Every row: ``road``, the episode total's ``mean``, ``sd``, ``se``, ``ci95_lo``, ``ci95_hi`` (``None`` for K = 1), ``min``,
    ``max`` over the K environments, and the per-bin means (:func:`link_bin_names`). ``expected``: ``{name: flows}`` with
    names of :data:`LINK_EXPECTED` (``msa``, ``ue``, ``so``) and flows a ``{road: flow}`` map (roads it lacks: 0) or an array
    (N,); per name the row gains the flow (column ``expected_msa`` / ``ue_flow`` / ``so_flow``), ``diff_<name>`` = mean -
    expected and ``geh_<name>`` (:func:`geh`), the summary RMSE, mean absolute difference, share of roads with GEH < 5, Pearson
    correlation (nan for a constant vector) and simulated total over expected total. NOTHING is rescaled
    (:data:`LINK_PARTIAL_NOTE`, carried as ``note``). ``baseline``: the evaluation of another head on the same environments
    (same K, seed, frames and bins: ``ValueError`` otherwise); the row gains ``baseline_mean`` and the paired difference
    result - baseline, ``paired_diff_mean`` / ``paired_diff_se`` / ``paired_diff_ci95_lo`` / ``_hi``, from the two-input
    ``ops.link_count_stats``; the summary counts the roads whose interval excludes 0. A run without link counts (a domain
    exit has none): ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.link_counts, "the run did not count links")) is not None:
        return gone
    K, H, N = result.link_counts.shape
    st = result.link_stats
    names = link_bin_names(result.link_first_bin, H, result.link_bin_seconds)
    rows = []
    for n in range(N):
        row = {"road": n, "mean": float(st["mean"][H, n]), **_spread("", st, H, n), "min": int(st["min"][H, n]),
               "max": int(st["max"][H, n])}
        row.update({name: float(st["mean"][h, n]) for h, name in enumerate(names)})
        rows.append(row)
    mean = st["mean"][H].astype(np.float64)
    summary = {"envs": K, "roads": N, "frames_run": result.frames_run, "simulated_total": float(mean.sum()),
               "roads_counted": int((st["max"][H] > 0).sum()), "expected": {}}
    columns = ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max"] + names
    for name, flows in (expected or {}).items():
        if name not in LINK_EXPECTED:
            raise ValueError(f"expected flows must be named among {tuple(LINK_EXPECTED)}, got {name!r}")
        c = _flow_vector(flows, N, name)
        d, g = mean - c, geh(mean, c)
        col = LINK_EXPECTED[name]
        for n, row in enumerate(rows):
            row.update({col: float(c[n]), f"diff_{name}": float(d[n]), f"geh_{name}": float(g[n])})
        columns += [col, f"diff_{name}", f"geh_{name}"]
        tot = float(c.sum())
        summary["expected"][name] = {"rmse": float(math.sqrt(float((d * d).mean()))), "mean_abs_diff": float(np.abs(d).mean()),
                                     "geh_below_5_share": float((g < 5.0).mean()), "pearson": _pearson(mean, c),
                                     "total_ratio": float(mean.sum()) / tot if tot != 0 else float("nan"),
                                     "expected_total": tot}
    rep = {"available": True, "head": result.head, "bin_seconds": result.link_bin_seconds,
           "first_bin": result.link_first_bin, "bins": names, "note": LINK_PARTIAL_NOTE}
    if baseline is not None:
        _check_pair("link_count_report", result, baseline)
        if baseline.domain_exit or baseline.link_counts is None:
            summary["paired"] = {"available": False, "reason": "the baseline run has no link counts"}
        else:
            if baseline.link_counts.shape != result.link_counts.shape or baseline.frames_run != result.frames_run or \
                    (baseline.link_first_bin, baseline.link_bin_seconds) != (result.link_first_bin, result.link_bin_seconds):
                raise ValueError("link_count_report needs the same frames and bins in both runs")
            pd = _paired_moments(result.link_counts, baseline.link_counts, K)
            pair = pd["std"] is not None
            for n, row in enumerate(rows):
                row.update(baseline_mean=float(baseline.link_stats["mean"][H, n]), paired_diff_mean=float(pd["mean"][H, n]),
                           **_spread("paired_diff_", pd, H, n, sd=False))
            columns += ["baseline_mean", "paired_diff_mean", "paired_diff_se", "paired_diff_ci95_lo", "paired_diff_ci95_hi"]
            excl = int(((pd["ci95_lo"][H] > 0) | (pd["ci95_hi"][H] < 0)).sum()) if pair else None
            summary["paired"] = {"available": True, "baseline_head": baseline.head, "roads_interval_excludes_zero": excl,
                                 "mean_abs_paired_diff": float(np.abs(pd["mean"][H]).mean()),
                                 "baseline_total": float(baseline.link_stats["mean"][H].sum())}
    rep.update(columns=columns, rows=rows, summary=summary)
    return rep


def link_count_lines(report: dict):
    """:func:`link_count_report` as printable lines (the ``Link counts`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"{'roads counted:':22} {s['roads_counted']:12d} of {s['roads']}  (pops + withdrawals per road, {s['envs']} "
           f"environments, {s['frames_run']} frames, bins of {report['bin_seconds']} s: {', '.join(report['bins'])})",
           f"{'simulated total:':22} {s['simulated_total']:12.3f}  (sum over the roads of the mean episode total)"]
    if not s["expected"]:
        out.append("expected flows:        not available (the MSA / equilibrium block was skipped): no comparison columns")
    for name, e in s["expected"].items():
        out.append(f"{'vs ' + name + ':':22} RMSE {e['rmse']:.3f}  mean |diff| {e['mean_abs_diff']:.3f}  GEH < 5 on "
                   f"{100.0 * e['geh_below_5_share']:.1f} % of the roads  Pearson r {e['pearson']:.4f}  simulated / expected "
                   f"total {e['total_ratio']:.4f}")
    if s["expected"]:
        out.append(f"note: {report['note']}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        line = f"{'policy - ' + p['baseline_head'] + ':':22} mean |paired diff| {p['mean_abs_paired_diff']:.3f} per road"
        if p["roads_interval_excludes_zero"] is not None:
            line += f"; the 95% interval excludes 0 on {p['roads_interval_excludes_zero']} of {s['roads']} roads (normal approx.)"
        else:
            line += "; one environment: no interval"
        out.append(line)
    return out


link_count_summary = _summary


# ---- per-road occupancy and time at capacity (VecEvaluator(occupancy=True)) ----------------------------------------------------
OCCUPANCY_RING_BYTES = 256 << 20    # the fp32 ring of frame_fused's `counts` slices
CONGESTION_FILE = 3                 # src/feature_helpers.py: has_room = n_i < max_i - CONGESTION_FILE


def capacity_threshold(max_agents):
    """``thr[n] = ceil(MAX[n] - 3)`` int32: the count from which road n admits nobody, the negation of Direction's
    ``has_room = n_i < max_i - CONGESTION_FILE`` and of the insert's capacity rule, taken literally (a road with MAX <= 3 is
    at capacity in every frame)."""
    return np.ceil(np.asarray(max_agents, dtype=np.float64) - CONGESTION_FILE).astype(np.int32)


def occupancy_report(result: "EvalResult", baseline: "EvalResult | None" = None) -> dict:
    """Per-road rows and a summary of the occupancy of one evaluation (``VecEvaluator(occupancy=True)``), formed in float64
    on the host from the integer accumulators ``veh`` (vehicle-frames per environment, bin and road), ``full`` (frames at
    capacity) and ``peak`` and their integer moments over the K environments.
    Every row: ``road``, ``max_agents`` (MAX) and ``thr``; ``veh_seconds_*`` of the episode (vehicle-frames x timestep):
    mean, sd, se, ci95_lo, ci95_hi (``None`` for K = 1), min, max over K; the mean occupancy per bin
    (:func:`occupancy_bin_names`: veh / frames in the bin, averaged over K; ``None`` for a bin without a frame); ``vc_mean``,
    the time-averaged count / max(MAX, 1) (the reference's v/c ratio); ``peak_mean`` / ``peak_max``; ``full_frames_mean`` /
    ``_min`` / ``_max`` and ``full_share`` of the frames run. ``baseline``: the evaluation of another head on the same
    environments (same K, seed, frames and bins: ``ValueError`` otherwise); the row gains the baseline's means and the paired
    differences result - baseline of veh_seconds and full_frames with se and interval, from the two-input
    ``ops.link_count_stats``. The summary: network vehicle-hours per environment (mean, se, interval over K; paired with a
    baseline), per bin the network mean and population sd of v/c averaged over K, the share of road-frames at capacity,
    the mean number of roads ever at capacity, the roads whose paired interval excludes 0, and the identity
    sum(veh[b]) == -episode_return[b]. A run without occupancy (a domain exit has none):
    ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.occupancy, "the run did not accumulate occupancy")) is not None:
        return gone
    veh, full, peak = (result.occupancy[k] for k in ("veh", "full", "peak"))
    K, H, N = veh.shape
    meta, st = result.occupancy_meta, result.occupancy_stats
    step, T = int(meta["timestep"]), int(result.frames_run)
    cap = np.asarray(meta["max"], dtype=np.float64)
    thr = np.asarray(meta["thr"], dtype=np.int64)
    fpb = np.asarray(result.occupancy_frames_per_bin, dtype=np.float64)
    names = occupancy_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    sv, sf, sp = st["veh"], st["full"], st["peak"]
    den = np.maximum(cap, 1.0)
    rows = []
    for n in range(N):
        row = {"road": n, "max_agents": float(cap[n]), "thr": int(thr[n]),
               "veh_seconds_mean": float(sv["mean"][H, n]) * step, **_spread("veh_seconds_", sv, H, n, step),
               "veh_seconds_min": int(sv["min"][H, n]) * step, "veh_seconds_max": int(sv["max"][H, n]) * step}
        row.update({name: float(sv["mean"][h, n]) / fpb[h] if fpb[h] > 0 else None for h, name in enumerate(names)})
        row.update(vc_mean=float(sv["mean"][H, n]) / T / den[n], peak_mean=float(sp["mean"][0, n]),
                   peak_max=int(sp["max"][0, n]), full_frames_mean=float(sf["mean"][H, n]), full_frames_min=int(sf["min"][H, n]),
                   full_frames_max=int(sf["max"][H, n]), full_share=float(sf["mean"][H, n]) / T)
        rows.append(row)
    columns = list(rows[0])
    v64, f64 = veh.astype(np.int64), full.astype(np.int64)
    veh_env = v64.sum(axis=(1, 2))                                     # vehicle-frames per environment
    ret = np.asarray(result.episode_return, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        vc = v64 / fpb[None, :, None] / den[None, None, :]             # (K, H, N); nan in a bin without a frame
    vc_mean, vc_sd = vc.mean(axis=2).mean(axis=0), vc.std(axis=2).mean(axis=0)
    summary = {"envs": K, "roads": N, "frames_run": T, "timestep": step,
               "vehicle_hours": aggregate(list(veh_env * step / 3600.0)),
               "vc_mean_per_bin": [float(x) for x in vc_mean], "vc_sd_per_bin": [float(x) for x in vc_sd],
               "frames_per_bin": [int(x) for x in fpb],
               "share_road_frames_at_capacity": float(f64.sum()) / (float(K) * T * N),
               "mean_roads_ever_at_capacity": float((f64.sum(axis=1) > 0).sum(axis=1).mean()),
               "largest_peak": int(peak.max()),
               "identity": {"holds": bool(np.array_equal(veh_env.astype(np.float64), -ret)),
                            "vehicle_frames": [int(x) for x in veh_env], "minus_episode_return": [float(-x) for x in ret]}}
    rep = {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
           "bins": names}
    if baseline is not None:
        _check_pair("occupancy_report", result, baseline)
        if baseline.domain_exit or baseline.occupancy is None:
            summary["paired"] = {"available": False, "reason": "the baseline run has no occupancy"}
        else:
            bm = baseline.occupancy_meta
            if baseline.occupancy["veh"].shape != veh.shape or baseline.frames_run != T or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds", "timestep")):
                raise ValueError("occupancy_report needs the same frames and bins in both runs")
            pv, pf = (_paired_moments(result.occupancy[k], baseline.occupancy[k], K) for k in ("veh", "full"))
            bv, bf = baseline.occupancy_stats["veh"], baseline.occupancy_stats["full"]
            for n, row in enumerate(rows):
                row.update(baseline_veh_seconds_mean=float(bv["mean"][H, n]) * step,
                           paired_veh_seconds_mean=float(pv["mean"][H, n]) * step,
                           **_spread("paired_veh_seconds_", pv, H, n, step, sd=False))
                row.update(baseline_full_frames_mean=float(bf["mean"][H, n]), paired_full_frames_mean=float(pf["mean"][H, n]),
                           **_spread("paired_full_frames_", pf, H, n, sd=False))
            columns = list(rows[0])
            pair = pv["std"] is not None
            excl = {k: int(((m["ci95_lo"][H] > 0) | (m["ci95_hi"][H] < 0)).sum()) if pair else None
                    for k, m in (("veh_seconds", pv), ("full_frames", pf))}
            base_env = baseline.occupancy["veh"].astype(np.int64).sum(axis=(1, 2))
            summary["paired"] = {"available": True, "baseline_head": baseline.head,
                                 "vehicle_hours": aggregate(list((veh_env - base_env) * step / 3600.0)),
                                 "baseline_vehicle_hours": aggregate(list(base_env * step / 3600.0)),
                                 "roads_interval_excludes_zero": excl}
    rep.update(columns=columns, rows=rows, summary=summary)
    return rep


def occupancy_lines(report: dict):
    """:func:`occupancy_report` as printable lines (the ``Occupancy`` block), the ten roads with the most frames at capacity
    included."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    g = s["vehicle_hours"]
    out = [f"{'vehicle-hours:':22} {g['mean']:12.3f}{_interval(g)}  min {g['min']:.3f}  max {g['max']:.3f}  n {g['n']}  (network "
           f"total per environment, {s['envs']} environments, {s['frames_run']} frames of {s['timestep']} s)"]
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        g = p["vehicle_hours"]
        line = f"{'policy - ' + p['baseline_head'] + ':':22} {g['mean']:12.3f} vehicle-hours{_interval(g)}"
        e = p["roads_interval_excludes_zero"]
        if e["veh_seconds"] is not None:
            line += (f"; per road the 95% interval excludes 0 on {e['veh_seconds']} (vehicle-seconds) and {e['full_frames']} "
                     f"(frames at capacity) of {s['roads']} roads")
        else:
            line += "; one environment: no interval"
        out.append(line)
    for name, frames, m, sd in zip(report["bins"], s["frames_per_bin"], s["vc_mean_per_bin"], s["vc_sd_per_bin"]):
        out.append(f"{'v/c ' + name + ':':22} mean {m:.4f}  sd {sd:.4f} over the roads, averaged over the environments "
                   f"({frames} frames)")
    out.append(f"{'at capacity:':22} {100.0 * s['share_road_frames_at_capacity']:.3f} % of the road-frames; "
               f"{s['mean_roads_ever_at_capacity']:.2f} of {s['roads']} roads ever at capacity (mean over the environments); "
               f"largest count {s['largest_peak']}")
    i = s["identity"]
    out.append(f"{'identity:':22} sum of vehicle-frames == -episode return in every environment: "
               f"{'yes' if i['holds'] else 'NO'} (environment 0: {i['vehicle_frames'][0]} / {i['minus_episode_return'][0]:.0f})")
    top = sorted(report["rows"], key=lambda r: (-r["full_frames_mean"], r["road"]))[:10]
    out.append("roads with the most frames at capacity (mean over the environments):")
    for r in top:
        out.append(f"  road {r['road']:6d}  full {r['full_frames_mean']:10.2f} frames ({100.0 * r['full_share']:.1f} %)  "
                   f"peak {r['peak_max']:3d} of MAX {r['max_agents']:.0f} (thr {r['thr']})  "
                   f"vehicle-seconds {r['veh_seconds_mean']:.1f}")
    return out


occupancy_summary = _summary


# ---- per-trip report (VecEvaluator(trips=True)) ----------------------------------------------------------------------------------
TRIP_FF_CHUNK_BYTES = 256 << 20     # the fp64 distance rows of one ops.destination_trees call of the free-flow times
TRIP_CHANCE = 0.025                 # share of agents without an effect whose 95 % interval lies on one side of 0
TRIP_FF_NOTE = ("free_flow is a reference value, not a lower bound: the withdraw rule and the step order decide when a trip "
                "ends, so a travel time can lie below it")


def trip_free_flow_times(engine, weights):
    """The free-flow time of every agent of ``engine`` (environment 0's table) -> fp64 (A,) on the device: FREE_FLOW of its
    origin road plus the distance origin -> destination under the edge weights ``weights`` fp32 (E,) from
    ``ops.destination_trees(want_dist=True)`` over the distinct destinations (src.agents.base.destination_set's rule), built
    a block of destinations at a time; +inf where the destination cannot be reached or an id is out of range, and for the
    dummy row 0. :data:`TRIP_FF_NOTE` applies."""
    N, dev = engine.N, engine.device
    w = weights.detach().to(dev, torch.float32).reshape(-1).contiguous()
    if w.numel() != engine.E:
        raise ValueError(f"trip_free_flow must hold one weight per edge ({engine.E}), got {w.numel()}")
    ag = engine.agents[0]
    o, d = ag[:, 0].to(torch.int64), ag[:, 1].to(torch.int64)
    ok = (o >= 0) & (o < N) & (d >= 0) & (d < N)
    ok[0] = False
    dests = torch.unique(d[ok]).contiguous()
    ff = torch.full((engine.A,), float("inf"), dtype=torch.float64, device=dev)
    if dests.numel() == 0:
        return ff
    slot = torch.full((N,), -1, dtype=torch.int64, device=dev)
    slot[dests] = torch.arange(dests.numel(), dtype=torch.int64, device=dev)
    oc, sl = o.clamp(0, N - 1), slot[d.clamp(0, N - 1)]
    own = engine.static_node_features[0, :, 2].to(torch.float64)        # FREE_FLOW_TIME_TRAVEL of the origin road
    rows = max(1, TRIP_FF_CHUNK_BYTES // (8 * N))
    for c0 in range(0, int(dests.numel()), rows):
        _, dist = ops.destination_trees(engine.plan, w, dests[c0:c0 + rows].contiguous(), want_next_hop=False, want_dist=True)
        here = ok & (sl >= c0) & (sl < c0 + dist.size(0))
        val = own[oc] + dist[(sl - c0).clamp(0, dist.size(0) - 1), oc]
        ff = torch.where(here, val, ff)
    return ff


def _trip_moments(n, s1, s2):
    """mean, sd (ddof 1), se and interval of n values with sum s1 and sum of squares s2, the rules of :func:`aggregate`:
    the mean needs one value, the others two."""
    out = {"mean": None, "sd": None, "se": None, "ci95_lo": None, "ci95_hi": None}
    n = int(n)
    if n >= 1:
        out["mean"] = float(s1) / n
    if n >= 2:
        sd = math.sqrt(max(0.0, (float(s2) - float(s1) * float(s1) / n) / (n - 1)))
        se = sd / math.sqrt(n)
        out.update(sd=sd, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def _trip_same_population(a: "EvalResult", b: "EvalResult"):
    return all(np.array_equal(a.trip_meta[k], b.trip_meta[k]) for k in ("origin", "destination", "departure"))


def trip_report(result: "EvalResult", baseline: "EvalResult | None" = None) -> dict:
    """Per-agent rows, a by-departure table and a summary of the trips of one evaluation (``VecEvaluator(trips=True)``),
    formed in float64 on the host from the kernels' counts and sums.
    Every row: ``agent``, ``origin``, ``destination``, ``departure``, ``free_flow`` (``None``: none); ``arrival_share`` =
    n_done / K and ``envs_on_way``; ``tt_mean``, ``tt_sd`` (ddof 1), ``tt_se``, ``tt_ci95_lo`` / ``_hi`` (mean -+ 1.96 se, normal
    approximation), ``tt_min``, ``tt_max`` over the environments in which the agent arrived — the mean, min and max ``None``
    without an arrival, the spread ``None`` below two, as in :func:`aggregate`; ``delay_mean`` = tt_mean - free_flow and
    ``delay_ratio`` = tt_mean / free_flow (``None`` without either). :data:`TRIP_FF_NOTE` applies.
    ``baseline``: the evaluation of another head on the same environments, run with ``run(..., trip_pair=<this run's agent
    tables>)`` (same K, seed, env_base, frames, bins and population: ``ValueError`` otherwise). The row gains
    ``baseline_arrival_share``, ``baseline_tt_mean`` and, over the environments in which the agent arrived in BOTH runs, the
    paired difference result - baseline: ``paired_n``, ``paired_diff_mean``, ``paired_diff_se``, ``paired_diff_ci95_lo`` /
    ``_hi``, ``n_faster`` and ``n_slower`` (environments in which the trip was faster / slower than under the baseline).
    The summary classifies every agent with paired_n >= 2 as faster (interval entirely below 0), slower (entirely above) or
    neither, the sign of the mean deciding where se = 0, and sets next to both counts the number expected by chance alone,
    :data:`TRIP_CHANCE` x the classified agents. A run without trips (a domain exit has none):
    ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.trips, "the run did not reduce its trips")) is not None:
        return gone
    tr, tb, meta = result.trips, result.trip_bins, result.trip_meta
    K, H = tb["dep_done"].shape
    A = tr["n_done"].shape[0]
    ff = meta["free_flow"]
    has_ff = ff is not None
    pair = None
    if baseline is not None:
        _check_pair("trip_report", result, baseline)
        if baseline.domain_exit or baseline.trips is None:
            pair = {"available": False, "reason": "the baseline run has no trips"}
        else:
            bm = baseline.trip_meta
            if baseline.frames_run != result.frames_run or baseline.trip_bins["dep_done"].shape != (K, H) or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds")):
                raise ValueError("trip_report needs the same frames and bins in both runs")
            if baseline.trips["n_done"].shape[0] != A or not _trip_same_population(result, baseline):
                raise ValueError("trip_report needs the same population in both runs (origin, destination, departure)")
            if not bm.get("paired") or "n_both" not in baseline.trips:
                pair = {"available": False, "reason": "the baseline run was not paired with this one (run(trip_pair=...))"}
            else:
                pair = {"available": True, "baseline_head": baseline.head}
    paired = pair is not None and pair["available"]
    n_done = tr["n_done"].astype(np.int64)
    rows = []
    cls = {"faster": 0, "slower": 0, "neither": 0}
    for a in range(1, A):
        n = int(n_done[a])
        m = _trip_moments(n, tr["tt_sum"][a], tr["tt_sumsq"][a])
        f = float(ff[a]) if has_ff and math.isfinite(float(ff[a])) else None
        row = {"agent": a, "origin": int(meta["origin"][a]), "destination": int(meta["destination"][a]),
               "departure": float(meta["departure"][a]), "free_flow": f, "arrival_share": n / K,
               "envs_on_way": int(tr["n_way"][a]), "tt_mean": m["mean"], "tt_sd": m["sd"], "tt_se": m["se"],
               "tt_ci95_lo": m["ci95_lo"], "tt_ci95_hi": m["ci95_hi"], "tt_min": float(tr["tt_min"][a]) if n else None,
               "tt_max": float(tr["tt_max"][a]) if n else None,
               "delay_mean": m["mean"] - f if n and f is not None else None,
               "delay_ratio": m["mean"] / f if n and f is not None and f > 0 else None}
        if paired:      # the baseline's launch holds d = baseline - result: the difference result - baseline is its negative
            bt = baseline.trips
            nb = int(bt["n_both"][a])
            d = _trip_moments(nb, -float(bt["d_sum"][a]), bt["d_sumsq"][a])
            row.update(baseline_arrival_share=int(bt["n_done"][a]) / K,
                       baseline_tt_mean=float(bt["tt_sum"][a]) / int(bt["n_done"][a]) if int(bt["n_done"][a]) else None,
                       paired_n=nb, paired_diff_mean=d["mean"], paired_diff_se=d["se"], paired_diff_ci95_lo=d["ci95_lo"],
                       paired_diff_ci95_hi=d["ci95_hi"], n_faster=int(bt["n_slower"][a]), n_slower=int(bt["n_faster"][a]))
            if nb >= 2:
                lo, hi = (d["ci95_lo"], d["ci95_hi"]) if d["se"] > 0 else (d["mean"], d["mean"])
                cls["faster" if hi < 0 else ("slower" if lo > 0 else "neither")] += 1
        rows.append(row)
    columns = list(rows[0]) if rows else []
    live = n_done[1:]
    trips_total = int(live.sum())
    summary = {"envs": K, "agents": A - 1, "frames_run": result.frames_run, "trips": trips_total,
               "arrived_in_every": int((live == K).sum()), "arrived_in_some": int(((live > 0) & (live < K)).sum()),
               "arrived_in_none": int((live == 0).sum()), "agents_on_way_somewhere": int((tr["n_way"][1:] > 0).sum()),
               "free_flow": None, "top_delays": []}
    if has_ff:
        f = np.asarray(ff, dtype=np.float64)[1:]
        use = np.isfinite(f) & (live > 0)
        w = live[use].astype(np.float64)
        tts, fs = tr["tt_sum"][1:][use].astype(np.float64), f[use]
        per_delay, per_ratio = tts / w - fs, (tts / w) / np.where(fs > 0, fs, np.nan)
        n_use = int(w.sum())
        spread = lambda v: float(np.nanstd(v, ddof=1)) if np.isfinite(v).sum() >= 2 else None      # noqa: E731
        summary["free_flow"] = {
            "agents": int(use.sum()), "trips": n_use, "note": TRIP_FF_NOTE,
            "mean_delay": float((tts - w * fs).sum()) / n_use if n_use else None,
            "delay_ratio": float(tts.sum()) / float((w * fs).sum()) if n_use and float((w * fs).sum()) > 0 else None,
            "mean_delay_sd_over_agents": spread(per_delay), "delay_ratio_sd_over_agents": spread(per_ratio),
            "share_trips_below_free_flow": int(tr["n_under"][1:].sum()) / n_use if n_use else None}
        top = sorted((r for r in rows if r["delay_mean"] is not None), key=lambda r: (-r["delay_mean"], r["agent"]))[:10]
        summary["top_delays"] = [{k: r[k] for k in ("agent", "origin", "destination", "departure", "free_flow", "tt_mean",
                                                    "delay_mean", "arrival_share")} for r in top]
    # by departure time: per bin over the K environments
    names = trip_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    dep_bin = trip_host_bin(meta["departure"][1:], meta["bin_seconds"], meta["first_bin"], H)
    scheduled = np.bincount(dep_bin, minlength=H)
    dd, dt = tb["dep_done"].astype(np.float64), tb["dep_tt"].astype(np.float64)
    by_rows = []
    for h in range(H):
        g = aggregate(list(dd[:, h]))
        tt = aggregate([dt[k, h] / dd[k, h] if dd[k, h] > 0 else None for k in range(K)])
        row = {"bin": names[h], "scheduled": int(scheduled[h]), "arrived_mean": g["mean"], "arrived_se": g["se"],
               "on_way_mean": float(tb["dep_way"][:, h].mean()), "tt_mean": tt["mean"], "tt_se": tt["se"], "delay_mean": None,
               "delay_se": None, "arrivals_mean": float(tb["arr"][:, h].mean())}
        if has_ff:
            fn, fs = tb["dep_ff_n"].astype(np.float64), tb["dep_ff"].astype(np.float64)
            dl = aggregate([dt[k, h] / dd[k, h] - fs[k, h] / fn[k, h] if dd[k, h] > 0 and fn[k, h] > 0 else None
                            for k in range(K)])
            row.update(delay_mean=dl["mean"], delay_se=dl["se"])
        by_rows.append(row)
    if pair is not None:
        if paired:
            n_cls = sum(cls.values())
            pair.update(agents_classified=n_cls, agents_faster=cls["faster"], agents_slower=cls["slower"],
                        agents_neither=cls["neither"], expected_by_chance=TRIP_CHANCE * n_cls,
                        pairs=int(baseline.trips["n_both"][1:].sum()),
                        mean_paired_diff=(-float(baseline.trips["d_sum"][1:].sum()) / int(baseline.trips["n_both"][1:].sum())
                                          if int(baseline.trips["n_both"][1:].sum()) else None))
        summary["paired"] = pair
    return {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
            "bins": names, "columns": columns, "rows": rows, "by_departure_columns": list(by_rows[0]),
            "by_departure": by_rows, "summary": summary}


def trip_host_bin(clock, bin_seconds, first_bin, num_bins):
    """The kernels' bin rule on the host: ``clamp(floor(c) // bin_seconds - first_bin, 0, num_bins - 1)`` of fp32 clock values
    (NaN and negatives as 0) -> int64."""
    c = np.nan_to_num(np.asarray(clock, dtype=np.float32).astype(np.float64), nan=0.0, posinf=2.0 ** 62, neginf=0.0)
    c = np.clip(np.floor(c), 0.0, 2.0 ** 62)
    return np.clip(c.astype(np.int64) // int(bin_seconds) - int(first_bin), 0, int(num_bins) - 1)


def _f(v, fmt=".2f"):
    return "-" if v is None else format(v, fmt)


def trip_lines(report: dict):
    """:func:`trip_report` as printable lines (the ``Trips`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"{'agents:':22} {s['agents']:12d}   arrived in every environment {s['arrived_in_every']}, in some "
           f"{s['arrived_in_some']}, in none {s['arrived_in_none']} ({s['envs']} environments, {s['frames_run']} frames; "
           f"{s['trips']} trips completed, {s['agents_on_way_somewhere']} agents still on the way somewhere)"]
    f = s["free_flow"]
    if f is None:
        out.append("free flow:             not available (no free-flow weights): no delay columns")
    elif not f["trips"]:
        out.append("free flow:             no completed trip with a free-flow time")
    else:
        out.append(f"{'mean delay:':22} {f['mean_delay']:12.3f} s  (tt - free flow, trip-weighted over {f['trips']} trips of "
                   f"{f['agents']} agents; sd over the agents {_f(f['mean_delay_sd_over_agents'], '.3f')})")
        out.append(f"{'delay ratio:':22} {_f(f['delay_ratio'], '12.4f')}    (sum tt / sum free flow; sd over the agents "
                   f"{_f(f['delay_ratio_sd_over_agents'], '.4f')})")
        out.append(f"{'below free flow:':22} {100.0 * f['share_trips_below_free_flow']:12.2f} % of the trips have tt < free flow "
                   f"(a reference value, not a lower bound)")
        out.append("agents with the largest mean delay:")
        for r in s["top_delays"]:
            out.append(f"  agent {r['agent']:7d}  {r['origin']:6d} -> {r['destination']:6d}  departs {r['departure']:9.1f}  "
                       f"free flow {r['free_flow']:8.1f}  tt {r['tt_mean']:9.2f}  delay {r['delay_mean']:9.2f}  "
                       f"arrived in {100.0 * r['arrival_share']:.0f} %")
    out.append(f"By departure time (bins of {report['bin_seconds']} s; means over the environments, arrived with its standard error):")
    out.append(f"  {'bin':>8} {'scheduled':>9} {'arrived':>18} {'mean tt':>10} {'mean delay':>10} {'arrivals in bin':>15}")
    for r in report["by_departure"]:
        arrived = f"{_f(r['arrived_mean'])}" + (f" +- {_f(r['arrived_se'])}" if r["arrived_se"] is not None else "")
        out.append(f"  {r['bin']:>8} {r['scheduled']:9d} {arrived:>18} {_f(r['tt_mean']):>10} {_f(r['delay_mean']):>10} "
                   f"{_f(r['arrivals_mean']):>15}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        out.append(f"{'policy - ' + p['baseline_head'] + ':':22} {_f(p['mean_paired_diff'], '12.3f')} s mean paired difference "
                   f"over {p['pairs']} trips completed in both runs")
        out.append(f"{'per agent:':22} faster under the policy {p['agents_faster']}, slower {p['agents_slower']}, neither "
                   f"{p['agents_neither']} of {p['agents_classified']} agents with >= 2 pairs (95% interval of the paired "
                   f"difference entirely below / above 0, normal approx.); expected by chance alone: "
                   f"{p['expected_by_chance']:.1f} on either side")
    return out


trip_summary = _summary


# ---- per-agent path trace (VecEvaluator(paths=True)) ------------------------------------------------------------------
PATH_NOTE = ("a road counts when the agent is seen as the head of its FIFO after a frame; moves = roads - 1; path cost = the "
             "weights of the hops between them; excess = the reduced cost of every hop against the shortest-path distances to "
             "the agent's own destination under the same weights (0 on a shortest path); a loop is a road met again among the "
             "KEPT roads of the trace (the first max_hops), a truncated trace saw more roads than it keeps")


def path_report(result: "EvalResult", baseline: "EvalResult | None" = None) -> dict:
    """Per-agent rows, a by-departure table and a summary of the path trace of one evaluation (``VecEvaluator(paths=True)``),
    formed in float64 on the host from the kernels' counts and sums.
    Every row: ``agent``, ``origin``, ``destination``, ``departure``; ``envs_seen`` (roads > 0), ``arrival_share`` = n_done / K,
    ``n_zero_excess``, ``n_loop``, ``n_trunc`` (over the environments in which the agent arrived), ``n_loop_all``,
    ``roads_max``; ``moves_*``, ``cost_*`` and ``excess_*`` with ``mean``, ``sd`` (ddof 1), ``se``, ``ci95_lo`` / ``_hi``
    (mean -+ 1.96 se, normal approximation) over the environments in which it arrived — ``None`` as in :func:`trip_report`,
    cost and excess ``None`` throughout where the run had no weights or no distance table.
    ``baseline``: the evaluation of another head on the same environments, run with ``run(..., path_pair=<this run's state
    and agent tables>)``; the row gains ``paired_n`` and the paired difference result - baseline of moves and of excess with
    se and interval. The summary splits a completed trip's travel time (where the run also reduced its trips) into path cost
    and the rest. A run without a trace (a domain exit has none): ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.path_stats, "the run did not trace its paths")) is not None:
        return gone
    ps, pa, meta = result.path_stats, result.paths, result.path_meta
    K, A = pa["roads"].shape
    has_w = bool(meta["weights"])
    pair = None
    if baseline is not None:
        _check_pair("path_report", result, baseline)
        if baseline.domain_exit or baseline.path_stats is None:
            pair = {"available": False, "reason": "the baseline run has no path trace"}
        elif baseline.frames_run != result.frames_run or baseline.paths["roads"].shape != (K, A) or not all(
                np.array_equal(baseline.path_meta[k], meta[k]) for k in ("origin", "destination", "departure")):
            raise ValueError("path_report needs the same frames and population in both runs")
        elif not baseline.path_meta.get("paired") or "n_both" not in baseline.path_stats:
            pair = {"available": False, "reason": "the baseline run was not paired with this one (run(path_pair=...))"}
        else:
            pair = {"available": True, "baseline_head": baseline.head}
    paired = pair is not None and pair["available"]
    n_done = ps["n_done"].astype(np.int64)
    rows = []
    for a in range(1, A):
        n = int(n_done[a])
        row = {"agent": a, "origin": int(meta["origin"][a]), "destination": int(meta["destination"][a]),
               "departure": float(meta["departure"][a]), "envs_seen": int(ps["n_seen"][a]), "arrival_share": n / K,
               "n_zero_excess": int(ps["n_zero_excess"][a]) if has_w else None, "n_loop": int(ps["n_loop"][a]),
               "n_trunc": int(ps["n_trunc"][a]), "n_loop_all": int(ps["n_loop_all"][a]), "roads_max": int(ps["roads_max"][a])}
        for name, key, on in (("moves", "moves", True), ("cost", "cost", has_w), ("excess", "excess", has_w)):
            m = _trip_moments(n if on else 0, ps[key + "_sum"][a], ps[key + "_sumsq"][a])
            row.update({f"{name}_mean": m["mean"], f"{name}_sd": m["sd"], f"{name}_se": m["se"],
                        f"{name}_ci95_lo": m["ci95_lo"], f"{name}_ci95_hi": m["ci95_hi"]})
        if paired:      # the baseline's launch holds d = baseline - result: the difference result - baseline is its negative
            bs = baseline.path_stats
            nb = int(bs["n_both"][a])
            row["paired_n"] = nb
            for name, key, on in (("moves", "dmoves", True), ("excess", "dexcess", has_w and bool(baseline.path_meta["weights"]))):
                d = _trip_moments(nb if on else 0, -float(bs[key + "_sum"][a]), bs[key + "_sumsq"][a])
                row.update({f"paired_{name}_diff_mean": d["mean"], f"paired_{name}_diff_se": d["se"],
                            f"paired_{name}_diff_ci95_lo": d["ci95_lo"], f"paired_{name}_diff_ci95_hi": d["ci95_hi"]})
        rows.append(row)
    live, seen = n_done[1:], ps["n_seen"][1:].astype(np.int64)
    trips = int(live.sum())
    w = live.astype(np.float64)
    spread = lambda v: float(np.std(v, ddof=1)) if v.size >= 2 else None      # noqa: E731
    per = lambda key: ps[key][1:][live > 0].astype(np.float64) / w[live > 0]   # noqa: E731  (the agents' own means)
    tot = lambda key: float(ps[key][1:].astype(np.float64).sum())             # noqa: E731
    done = pa["done"].copy()
    done[:, 0] = True       # the dummy is nobody's unfinished trip
    open_ = ~done & (pa["roads"] > 0)
    summary = {"envs": K, "agents": A - 1, "frames_run": result.frames_run, "max_hops": int(meta["max_hops"]), "note": PATH_NOTE,
               "seen_in_every": int((seen == K).sum()), "seen_in_some": int(((seen > 0) & (seen < K)).sum()),
               "seen_in_none": int((seen == 0).sum()), "trips": trips,
               "mean_moves": tot("moves_sum") / trips if trips else None, "mean_moves_sd_over_agents": spread(per("moves_sum")),
               "share_loop": int(ps["n_loop"][1:].sum()) / trips if trips else None,
               "share_truncated": int(ps["n_trunc"][1:].sum()) / trips if trips else None,
               "open": {"traces": int(open_.sum()), "with_loop": int((open_ & (pa["revisits"] > 0)).sum()),
                        "truncated": int((open_ & (pa["roads"] > meta["max_hops"])).sum()),
                        "mean_moves": float(np.maximum(pa["roads"][open_] - 1, 0).mean()) if open_.any() else None},
               "weights": None, "excess_note": meta["note"], "top_excess": []}
    if has_w:
        cost, exc = tot("cost_sum"), tot("excess_sum")
        wsum = {"mean_cost": cost / trips if trips else None, "mean_cost_sd_over_agents": spread(per("cost_sum")),
                "mean_excess": exc / trips if trips else None, "mean_excess_sd_over_agents": spread(per("excess_sum")),
                "excess_over_cost": exc / cost if cost > 0 else None,
                "share_zero_excess": int(ps["n_zero_excess"][1:].sum()) / trips if trips else None,
                "off_tree_hops": int(pa["off_tree"][:, 1:].sum()),
                "open_zero_excess": int((open_ & (pa["excess"] == 0.0) & (pa["off_tree"] == 0)).sum()),
                "excess_over_travel_time": None, "mean_travel_time": None, "mean_residual": None}
        if result.trips is not None and trips and int(result.trips["n_done"][1:].sum()) == trips:
            tt = float(result.trips["tt_sum"][1:].astype(np.float64).sum())
            wsum.update(excess_over_travel_time=exc / tt if tt > 0 else None, mean_travel_time=tt / trips,
                        mean_residual=(tt - cost) / trips)
        summary["weights"] = wsum
        top = sorted((r for r in rows if r["excess_mean"] is not None and r["excess_mean"] > 0), key=lambda r: (-r["excess_mean"], r["agent"]))[:10]
        summary["top_excess"] = [{k: r[k] for k in ("agent", "origin", "destination", "departure", "moves_mean", "cost_mean",
                                                    "excess_mean", "n_loop", "arrival_share")} for r in top]
    H = int(meta["num_bins"])
    names = trip_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    dep_bin = trip_host_bin(meta["departure"][1:], meta["bin_seconds"], meta["first_bin"], H)
    by_rows = []
    for h in range(H):
        m = dep_bin == h
        t = int(live[m].sum())
        s = lambda key: float(ps[key][1:][m].astype(np.float64).sum())      # noqa: E731
        by_rows.append({"bin": names[h], "scheduled": int(m.sum()), "trips": t, "moves_mean": s("moves_sum") / t if t else None,
                        "cost_mean": s("cost_sum") / t if t and has_w else None,
                        "excess_mean": s("excess_sum") / t if t and has_w else None,
                        "share_loop": int(ps["n_loop"][1:][m].sum()) / t if t else None,
                        "share_truncated": int(ps["n_trunc"][1:][m].sum()) / t if t else None})
    if pair is not None:
        if paired:
            bs = baseline.path_stats
            nb = int(bs["n_both"][1:].sum())
            pair.update(pairs=nb, mean_moves_diff=-float(bs["dmoves_sum"][1:].sum()) / nb if nb else None,
                        mean_excess_diff=(-float(bs["dexcess_sum"][1:].sum()) / nb
                                          if nb and has_w and baseline.path_meta["weights"] else None))
        summary["paired"] = pair
    return {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
            "bins": names, "columns": list(rows[0]) if rows else [], "rows": rows, "by_departure_columns": list(by_rows[0]),
            "by_departure": by_rows, "summary": summary}


def path_route_rows(result: "EvalResult", envs: int):
    """The kept routes of the first ``envs`` environments as rows of ``eval_paths_routes.csv``: env, agent, roads, truncated,
    route (the kept road ids, space-separated). Agents never seen are left out."""
    routes, length = result.path_routes
    roads = result.paths["roads"]
    rows = []
    for k in range(min(int(envs), roads.shape[0])):
        for a in range(1, roads.shape[1]):
            if roads[k, a] > 0:
                rows.append({"env": k, "agent": a, "roads": int(roads[k, a]), "truncated": int(roads[k, a] > length[k, a]),
                             "route": " ".join(str(int(u)) for u in routes[k, a, :length[k, a]])})
    return rows


def path_lines(report: dict):
    """:func:`path_report` as printable lines (the ``Paths`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    pct = lambda v: "-" if v is None else f"{100.0 * v:.2f} %"      # noqa: E731
    out = [f"definition:            {s['note']}",
           f"{'agents:':22} {s['agents']:12d}   seen as a head in every environment {s['seen_in_every']}, in some "
           f"{s['seen_in_some']}, in none {s['seen_in_none']} ({s['envs']} environments, {s['frames_run']} frames; "
           f"{s['trips']} trips completed; {s['max_hops']} roads kept per trace)",
           f"{'mean moves:':22} {_f(s['mean_moves'], '12.3f')}    (trip-weighted; sd over the agents "
           f"{_f(s['mean_moves_sd_over_agents'], '.3f')})"]
    w = s["weights"]
    if w is None:
        out.append(f"{'path cost, excess:':22} {s['excess_note'] or 'not available (no edge weights): roads and loops only'}")
    else:
        out.append(f"{'mean path cost:':22} {_f(w['mean_cost'], '12.3f')} s  (sd over the agents {_f(w['mean_cost_sd_over_agents'], '.3f')})")
        out.append(f"{'mean excess:':22} {_f(w['mean_excess'], '12.3f')} s  (wandering: cost beyond the shortest path; sd over the "
                   f"agents {_f(w['mean_excess_sd_over_agents'], '.3f')})")
        out.append(f"{'excess / path cost:':22} {_f(w['excess_over_cost'], '12.4f')}    (sum excess / sum path cost)")
        if w["mean_travel_time"] is not None:
            out.append(f"{'excess / travel time:':22} {_f(w['excess_over_travel_time'], '12.4f')}    (sum excess / sum travel time)")
            out.append(f"{'travel time:':22} {w['mean_travel_time']:12.3f} s = shortest free-flow cost "
                       f"{w['mean_cost'] - w['mean_excess']:.3f} + wandering {w['mean_excess']:.3f} + everything else "
                       f"{w['mean_residual']:.3f} (travel time - path cost: the first road, queues and the wait for the "
                       f"withdraw rule)")
        out.append(f"{'completed trips:':22} zero excess {pct(w['share_zero_excess'])}, with a loop {pct(s['share_loop'])}, "
                   f"truncated {pct(s['share_truncated'])}; {w['off_tree_hops']} off-tree hops in all traces")
    o = s["open"]
    out.append(f"{'not arrived:':22} {o['traces']} traces of agents seen but not DONE at the end: with a loop {o['with_loop']}, "
               f"truncated {o['truncated']}" + (f", zero excess {w['open_zero_excess']}" if w is not None else "") +
               f", mean moves {_f(o['mean_moves'])}")
    if w is None:
        out.append(f"{'completed trips:':22} with a loop {pct(s['share_loop'])}, truncated {pct(s['share_truncated'])}")
    if s["top_excess"]:
        out.append("agents with the largest mean excess:")
        for r in s["top_excess"]:
            out.append(f"  agent {r['agent']:7d}  {r['origin']:6d} -> {r['destination']:6d}  departs {r['departure']:9.1f}  moves "
                       f"{r['moves_mean']:7.2f}  cost {r['cost_mean']:9.2f}  excess {r['excess_mean']:9.2f}  loops in "
                       f"{r['n_loop']} trips  arrived in {100.0 * r['arrival_share']:.0f} %")
    out.append(f"By departure time (bins of {report['bin_seconds']} s; over the completed trips of the agents that depart in the bin):")
    out.append(f"  {'bin':>8} {'scheduled':>9} {'trips':>8} {'moves':>9} {'cost':>10} {'excess':>10} {'loop':>9} {'truncated':>9}")
    for r in report["by_departure"]:
        out.append(f"  {r['bin']:>8} {r['scheduled']:9d} {r['trips']:8d} {_f(r['moves_mean']):>9} {_f(r['cost_mean']):>10} "
                   f"{_f(r['excess_mean']):>10} {pct(r['share_loop']):>9} {pct(r['share_truncated']):>9}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        out.append(f"{'policy - ' + p['baseline_head'] + ':':22} moves {_f(p['mean_moves_diff'], '.3f')}, excess "
                   f"{_f(p['mean_excess_diff'], '.3f')} s mean paired difference over {p['pairs']} trips completed in both runs")
    return out


path_summary = _summary


# ---- dynamic relative gap (VecEvaluator(dynamic_gap=True)) ------------------------------------------------------------------------
DYNAMIC_GAP_NOTE = ("g = travel time - hindsight time: the hindsight time is the quickest way from origin to destination (both "
                    "roads traversed) under the road times of the run's own mean occupancy per time bin, waiting allowed; "
                    "RG = sum g / sum tt over the completed trips of an environment. g can be negative: the road time is a bin "
                    "mean and the withdraw rule decides when a trip ends")


def _gap_relative(per_env):
    """RG_k per environment, ``None`` without a usable trip."""
    return [float((per_env["tt_sum"][k] - per_env["ht_sum"][k]) / per_env["tt_sum"][k])
            if int(per_env["n"][k]) > 0 and float(per_env["tt_sum"][k]) != 0.0 else None for k in range(len(per_env["n"]))]


def dynamic_gap_report(result: "EvalResult", baseline: "EvalResult | None" = None) -> dict:
    """Per-agent rows, a by-departure table and a summary of the dynamic gap of one evaluation
    (``VecEvaluator(dynamic_gap=True)``), formed in float64 on the host from the device's sums. :data:`DYNAMIC_GAP_NOTE` is the
    definition.
    Every row: ``agent``, ``origin``, ``destination``, ``departure``; ``envs_usable``, the environments in which the agent
    arrived and had a finite hindsight time; ``gap_mean``, ``gap_sd`` (ddof 1), ``gap_se``, ``gap_ci95_lo`` / ``_hi``, ``gap_min``,
    ``gap_max`` over them (``None`` as in :func:`aggregate`) and ``envs_negative`` (g < 0).
    The summary: ``relative_gap``, :func:`aggregate` of RG_k over the environments (mean, std, se, ci95; an environment without
    a usable trip is missing) and ``relative_gap_per_env``; ``mean_gap``, the trip-weighted mean of g in seconds;
    ``share_negative`` (g < 0) and ``share_nonpositive`` (g <= 0) of the usable trips; ``top_gaps``, the ten agents with the
    largest mean gap; ``searches`` and ``search_wall_ms``.
    ``baseline``: the evaluation of another head on the same environments with ``dynamic_gap=True`` (same K, seed, env_base,
    frames, bins, population and ``dynamic_gap_envs``: ``ValueError`` otherwise); the summary gains ``paired``, the difference
    RG_k(result) - RG_k(baseline) over the environments in which both have one: n, mean, std, se, ci95.
    A run without the gap (a domain exit has none): ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.dynamic_gap, "the run did not compute the dynamic gap")) is not None:
        return gone
    dg = result.dynamic_gap
    pa, pe, pb, meta = dg["per_agent"], dg["per_env"], dg["per_bin"], dg["meta"]
    J, H = pb["n"].shape
    A = pa["n"].shape[0]
    rg = _gap_relative(pe)
    pair = None
    if baseline is not None:
        _check_pair("dynamic_gap_report", result, baseline)
        if baseline.domain_exit or baseline.dynamic_gap is None:
            pair = {"available": False, "reason": "the baseline run has no dynamic gap"}
        else:
            bm = baseline.dynamic_gap["meta"]
            if baseline.frames_run != result.frames_run or baseline.dynamic_gap["per_bin"]["n"].shape != (J, H) or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds", "envs")):
                raise ValueError("dynamic_gap_report needs the same frames, bins and dynamic_gap_envs in both runs")
            if baseline.dynamic_gap["per_agent"]["n"].shape[0] != A or \
                    not all(np.array_equal(bm[k], meta[k]) for k in ("origin", "destination", "departure")):
                raise ValueError("dynamic_gap_report needs the same population in both runs (origin, destination, departure)")
            brg = _gap_relative(baseline.dynamic_gap["per_env"])
            d = np.asarray([x - y for x, y in zip(rg, brg) if x is not None and y is not None], dtype=np.float64)
            pair = {"available": True, "baseline_head": baseline.head, "n": int(d.size), "dropped": int(J - d.size),
                    **_sample_moments(d), "ci95_kind": _CI95_KIND, "baseline_relative_gap": aggregate(brg)}
    rows = []
    for a in range(1, A):
        n = int(pa["n"][a])
        m = _trip_moments(n, pa["g_sum"][a], pa["g_sumsq"][a])
        rows.append({"agent": a, "origin": int(meta["origin"][a]), "destination": int(meta["destination"][a]),
                     "departure": float(meta["departure"][a]), "envs_usable": n, "gap_mean": m["mean"], "gap_sd": m["sd"],
                     "gap_se": m["se"], "gap_ci95_lo": m["ci95_lo"], "gap_ci95_hi": m["ci95_hi"],
                     "gap_min": float(pa["g_min"][a]) if n else None, "gap_max": float(pa["g_max"][a]) if n else None,
                     "envs_negative": int(pa["n_neg"][a])})
    trips = int(pe["n"].sum())
    top = sorted((r for r in rows if r["gap_mean"] is not None), key=lambda r: (-r["gap_mean"], r["agent"]))[:10]
    summary = {"envs": J, "agents": A - 1, "frames_run": result.frames_run, "trips": trips,
               "searches": int(meta["searches"]), "search_wall_ms": float(meta["wall_ms"]),
               "relative_gap": aggregate(rg), "relative_gap_per_env": rg,
               "mean_gap": float(pe["tt_sum"].sum() - pe["ht_sum"].sum()) / trips if trips else None,
               "share_negative": int(pe["n_neg"].sum()) / trips if trips else None,
               "share_nonpositive": int(pe["n_nonpos"].sum()) / trips if trips else None,
               "top_gaps": [{k: r[k] for k in ("agent", "origin", "destination", "departure", "envs_usable", "gap_mean")}
                            for r in top]}
    names = trip_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    by_rows = []
    for h in range(H):
        g = aggregate([float(pb["g_sum"][k, h]) / int(pb["n"][k, h]) if int(pb["n"][k, h]) > 0 else None for k in range(J)])
        by_rows.append({"bin": names[h], "trips_mean": float(pb["n"][:, h].mean()), "gap_mean": g["mean"], "gap_se": g["se"],
                        "envs": g["n"]})
    if pair is not None:
        summary["paired"] = pair
    return {"available": True, "head": result.head, "definition": DYNAMIC_GAP_NOTE, "bin_seconds": int(meta["bin_seconds"]),
            "first_bin": int(meta["first_bin"]), "bins": names, "columns": list(rows[0]) if rows else [], "rows": rows,
            "by_departure_columns": list(by_rows[0]), "by_departure": by_rows, "summary": summary}


def dynamic_gap_paired_lines(report: dict):
    """The paired part of :func:`dynamic_gap_report` as printable lines; empty for a report without a baseline."""
    p = report["summary"].get("paired") if report["available"] else None
    if p is None:
        return []
    if not p["available"]:
        return [f"paired:                not available: {p['reason']}"]
    if p["mean"] is None:
        return [f"{'policy - ' + p['baseline_head'] + ':':22} no environment with a relative gap in both runs"]
    return [f"{'policy - ' + p['baseline_head'] + ':':22} {p['mean']:12.5f}{_interval(p)}  n {p['n']}  (paired difference of the "
            f"relative gap per environment)"]


def dynamic_gap_lines(report: dict, paired=True):
    """:func:`dynamic_gap_report` as printable lines (the ``Dynamic gap`` block); ``paired=False`` leaves the paired line to
    :func:`dynamic_gap_paired_lines`."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    out = [f"definition:            {report['definition']}",
           f"{'searches:':22} {s['searches']:12d}   hindsight searches over {s['envs']} environments in {s['search_wall_ms']:.1f} ms "
           f"(road times and reductions included)"]
    g = s["relative_gap"]
    if g["mean"] is None:
        out.append("relative gap:          no environment with a completed trip that has a hindsight time")
    else:
        out.append(f"{'relative gap:':22} {g['mean']:12.5f}{_interval(g)}  n {g['n']}"
                   + (f"  ({g['missing']} environments without a usable trip left out)" if g["missing"] else ""))
        out.append(f"{'mean gap:':22} {s['mean_gap']:12.3f} s  (trip-weighted over {s['trips']} trips); g < 0 in "
                   f"{100.0 * s['share_negative']:.2f} % of the trips, g <= 0 in {100.0 * s['share_nonpositive']:.2f} %")
        out.append("agents with the largest mean gap:")
        for r in s["top_gaps"]:
            out.append(f"  agent {r['agent']:7d}  {r['origin']:6d} -> {r['destination']:6d}  departs {r['departure']:9.1f}  "
                       f"gap {r['gap_mean']:9.2f}  over {r['envs_usable']} environments")
    out.append(f"By departure time (bins of {report['bin_seconds']} s; means over the environments with their standard error):")
    out.append(f"  {'bin':>8} {'trips':>10} {'mean gap':>20}")
    for r in report["by_departure"]:
        gap = _f(r["gap_mean"]) + (f" +- {_f(r['gap_se'])}" if r["gap_se"] is not None else "")
        out.append(f"  {r['bin']:>8} {_f(r['trips_mean']):>10} {gap:>20}")
    return out + (dynamic_gap_paired_lines(report) if paired else [])


dynamic_gap_summary = _summary


# ---- per-turn movement counts (VecEvaluator(turns=True)) --------------------------------------------------------------------------
TURN_RING_BYTES = 256 << 20         # the three rings of the evaluator together: popped, SELECTED_ROAD bytes, counts
TURN_LOST_NOTE = ("an agent that moves into an EMPTY road u from a road v with an edge u -> v is accepted on both edges by the "
                  "reference's ResponseMPNN: u is popped although nothing left it and the agent is queued nowhere from then "
                  "on (DESIGN quirk Q24); it stays flagged ON_WAY and never arrives")


def turn_report(result: "EvalResult", baseline: "EvalResult | None" = None) -> dict:
    """Per-route-edge rows, the roads with a loss and a summary of the turn counts of one evaluation
    (``VecEvaluator(turns=True)``), formed in float64 on the host from the integer tables and their integer moments.
    Every row: ``edge`` (the caller's edge id), ``from_road``, ``to_road``; the episode total's ``mean``, ``sd``, ``se``,
    ``ci95_lo``, ``ci95_hi`` (``None`` for K = 1), ``min``, ``max`` over the K environments; the per-bin means
    (:func:`turn_bin_names`); ``share``, the edge's part of all movements out of ``from_road`` (over all environments;
    ``None`` where nothing left the road); for the state-independent head ``embedding`` the policy's ``policy_prob`` of the
    edge and ``share_minus_prob``. ``baseline``: the evaluation of another head on the same environments (same K, seed,
    frames, bins and edges: ``ValueError`` otherwise); the row gains ``baseline_mean`` and the paired difference result -
    baseline, ``paired_diff_mean`` / ``_se`` / ``_ci95_lo`` / ``_hi``, from the two-input ``ops.link_count_stats``; the summary
    counts the turns whose interval excludes 0. ``lost_rows``: one row per road with a phantom pop (``road``, ``mean``, ``se``,
    ``min``, ``max`` of the episode total, the per-bin means). The summary also carries the movements and the lost agents
    per environment (:func:`aggregate`), the turns used, the ten busiest turns, the per-bin totals and the identity lost ==
    ON_WAY - queued per environment. A run without turn counts (a domain exit has none):
    ``{"available": False, "reason": ...}``."""
    if (gone := _unavailable(result, result.turn_counts, "the run did not count turns")) is not None:
        return gone
    tc, tl, meta = result.turn_counts, result.turn_lost, result.turn_meta
    K, H, E = tc.shape
    N = tl.shape[2]
    st, sl = result.turn_stats["turns"], result.turn_stats["lost"]
    names = turn_bin_names(meta["first_bin"], H, meta["bin_seconds"])
    src, dst = (np.asarray(meta["edge_index"][i], dtype=np.int64) for i in (0, 1))
    total = st["sum"][H].astype(np.float64)                             # movements per edge over all environments
    out_of = np.zeros(N, dtype=np.float64)
    np.add.at(out_of, src, total)
    prob = meta.get("policy_prob")
    rows = []
    for e in range(E):
        den = out_of[src[e]]
        row = {"edge": e, "from_road": int(src[e]), "to_road": int(dst[e]), "mean": float(st["mean"][H, e]),
               **_spread("", st, H, e), "min": int(st["min"][H, e]), "max": int(st["max"][H, e])}
        row.update({name: float(st["mean"][h, e]) for h, name in enumerate(names)})
        row["share"] = float(total[e] / den) if den > 0 else None
        if prob is not None:
            row["policy_prob"] = float(prob[e])
            row["share_minus_prob"] = None if row["share"] is None else row["share"] - float(prob[e])
        rows.append(row)
    columns = list(rows[0])
    lost_rows = []
    for n in np.nonzero(sl["max"][H] > 0)[0]:
        row = {"road": int(n), "mean": float(sl["mean"][H, n]), **_spread("", sl, H, n), "min": int(sl["min"][H, n]),
               "max": int(sl["max"][H, n])}
        row.update({name.replace("turns_", "lost_"): float(sl["mean"][h, n]) for h, name in enumerate(names)})
        lost_rows.append(row)
    lost_columns = ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max"] + [n.replace("turns_", "lost_") for n in names]
    moved_env = tc.astype(np.int64).sum(axis=(1, 2))
    lost_env = tl.astype(np.int64).sum(axis=(1, 2))
    missing = [a - b for a, b in zip(meta["on_way"], meta["queued"])]
    top = sorted(rows, key=lambda r: (-r["mean"], r["edge"]))[:10]
    summary = {"envs": K, "edges": E, "roads": N, "frames_run": result.frames_run,
               "movements": aggregate(list(moved_env.astype(np.float64))), "movements_per_env": [int(x) for x in moved_env],
               "turns_used": int((st["max"][H] > 0).sum()),
               "roads_using_two_turns": int((np.bincount(src, weights=(st["max"][H] > 0), minlength=N) >= 2).sum()),
               "lost": aggregate(list(lost_env.astype(np.float64))), "lost_per_env": [int(x) for x in lost_env],
               "roads_with_a_loss": len(lost_rows), "lost_note": TURN_LOST_NOTE,
               "identity": {"holds": [int(x) for x in lost_env] == missing, "on_way": list(meta["on_way"]),
                            "queued": list(meta["queued"])},
               "movements_per_bin": [float(x) for x in st["mean"][:H].sum(axis=1)],
               "lost_per_bin": [float(x) for x in sl["mean"][:H].sum(axis=1)],
               "top_turns": [{k: r[k] for k in ("edge", "from_road", "to_road", "mean", "share")} for r in top]}
    rep = {"available": True, "head": result.head, "bin_seconds": int(meta["bin_seconds"]), "first_bin": int(meta["first_bin"]),
           "bins": names}
    if baseline is not None:
        _check_pair("turn_report", result, baseline)
        if baseline.domain_exit or baseline.turn_counts is None:
            summary["paired"] = {"available": False, "reason": "the baseline run has no turn counts"}
        else:
            bm = baseline.turn_meta
            if baseline.turn_counts.shape != tc.shape or baseline.frames_run != result.frames_run or \
                    any(bm[k] != meta[k] for k in ("first_bin", "bin_seconds")) or \
                    not np.array_equal(bm["edge_index"], meta["edge_index"]):
                raise ValueError("turn_report needs the same frames, bins and edges in both runs")
            pd = _paired_moments(tc, baseline.turn_counts, K)
            bs = baseline.turn_stats["turns"]
            for e, row in enumerate(rows):
                row.update(baseline_mean=float(bs["mean"][H, e]), paired_diff_mean=float(pd["mean"][H, e]),
                           **_spread("paired_diff_", pd, H, e, sd=False))
            columns = list(rows[0])
            excl = int(((pd["ci95_lo"][H] > 0) | (pd["ci95_hi"][H] < 0)).sum()) if pd["std"] is not None else None
            summary["paired"] = {"available": True, "baseline_head": baseline.head, "turns_interval_excludes_zero": excl,
                                 "mean_abs_paired_diff": float(np.abs(pd["mean"][H]).mean()),
                                 "baseline_movements": float(bs["mean"][H].sum()),
                                 "baseline_lost": float(baseline.turn_stats["lost"]["mean"][H].sum())}
    rep.update(columns=columns, rows=rows, lost_columns=lost_columns, lost_rows=lost_rows, summary=summary)
    return rep


def turn_lines(report: dict):
    """:func:`turn_report` as printable lines (the ``Turns`` block)."""
    if not report["available"]:
        return [f"not available: {report['reason']}"]
    s = report["summary"]
    g, lo = s["movements"], s["lost"]
    i = s["identity"]
    out = [f"{'movements:':22} {g['mean']:12.3f}{_interval(g)}  min {g['min']:.0f}  max {g['max']:.0f}  n {g['n']}  (vehicles that "
           f"crossed a route edge, per environment; {s['envs']} environments, {s['frames_run']} frames)",
           f"{'turns used:':22} {s['turns_used']:12d} of {s['edges']}  ({s['roads_using_two_turns']} of {s['roads']} roads sent "
           f"vehicles over at least two of their out-edges)",
           f"{'agents lost (Q24):':22} {lo['mean']:12.3f}{_interval(lo)}  on {s['roads_with_a_loss']} roads; lost == ON_WAY - queued "
           f"in every environment: {'yes' if i['holds'] else 'NO'} (environment 0: {s['lost_per_env'][0]} == "
           f"{i['on_way'][0]} - {i['queued'][0]})"]
    for name, m, gone in zip(report["bins"], s["movements_per_bin"], s["lost_per_bin"]):
        out.append(f"{name + ':':22} {m:12.3f} movements, {gone:.3f} lost (mean over the environments)")
    out.append("busiest turns (mean movements per environment, share of the movements out of the road):")
    for r in s["top_turns"]:
        out.append(f"  edge {r['edge']:7d}  {r['from_road']:6d} -> {r['to_road']:6d}  {r['mean']:10.2f}  "
                   f"share {_f(r['share'], '.3f')}")
    p = s.get("paired")
    if p is not None and not p["available"]:
        out.append(f"paired:                not available: {p['reason']}")
    elif p is not None:
        line = (f"{'policy - ' + p['baseline_head'] + ':':22} mean |paired diff| {p['mean_abs_paired_diff']:.3f} per turn "
                f"(baseline: {p['baseline_movements']:.3f} movements, {p['baseline_lost']:.3f} lost per environment)")
        if p["turns_interval_excludes_zero"] is not None:
            line += f"; the 95% interval excludes 0 on {p['turns_interval_excludes_zero']} of {s['edges']} turns (normal approx.)"
        else:
            line += "; one environment: no interval"
        out.append(line)
    return out


def turn_summary(report: dict):
    """A turn report without its tables (``rows``, ``lost_rows``): what the JSON files carry."""
    return _json_clean({k: v for k, v in report.items() if k not in ("rows", "lost_rows")})
