"""TEST INFRASTRUCTURE: numpy restatement of the per-trip reductions (``tarl_trip_agent_stats``, ``tarl_trip_bin_stats``) and of
the arithmetic of ``tarl_hip.evaluator.trip_report``, the crafted cases shared by the host and the GPU suite, and the same
restatement with ONE deliberate defect at a time. Plain module: no fixtures; nothing at import time needs a GPU.

Definitions (agent tables fp32 (K, A, 9), row 0 the dummy and skipped): an agent has arrived when DONE == 1 and its travel time
is tt = ARRIVAL_TIME - DEPARTURE_TIME in fp32, widened to fp64; it is on the way when it has not arrived and ON_WAY == 1. The
bin of a clock value c is clamp(floor(c) // bin_seconds - first_bin, 0, H - 1). Every fp64 sum here runs in plain ascending
order (environments for the per-agent sums, agents for the per-bin sums)."""
from __future__ import annotations

import math

import numpy as np

ORIGIN, DEST, DEP, ARR, ON_WAY, DONE = 0, 1, 2, 3, 7, 8
TILE = 64                   # agents per workgroup of the per-agent kernel
DEFECTS = ("dummy_counted", "last_env_skipped", "last_agent_of_partial_tile_skipped", "arr_dep_swapped", "on_way_for_done",
           "pair_with_one_arrival", "faster_includes_equal", "arrivals_by_departure", "no_low_clamp", "no_high_clamp",
           "ff_inf_added", "minmax_seeded_zero")
AGENT_KEYS = ("n_done", "n_way", "tt_sum", "tt_sumsq", "tt_min", "tt_max")
PAIR_KEYS = ("n_both", "d_sum", "d_sumsq", "n_faster", "n_slower")
BIN_KEYS = ("dep_done", "dep_way", "arr", "dep_tt")
FF_KEYS = ("dep_ff", "dep_ff_n")


def clock_bin(c, bin_seconds, first_bin, H, low=True, high=True):
    """Bin of fp32 clock values -> int64; without ``low`` / ``high`` the value is NOT clamped on that side (a defect): -1
    marks an element that then falls outside the stored bins."""
    q = np.floor(np.asarray(c, dtype=np.float32).astype(np.float64)).astype(np.int64) // int(bin_seconds) - int(first_bin)
    out = np.clip(q, 0 if low else None, H - 1 if high else None)
    return np.where((out < 0) | (out > H - 1), -1, out)


def _flags(agents, defect):
    done = agents[..., ON_WAY if defect == "on_way_for_done" else DONE] == 1.0
    way = ~done & (agents[..., ON_WAY] == 1.0)
    tt32 = agents[..., DEP] - agents[..., ARR] if defect == "arr_dep_swapped" else agents[..., ARR] - agents[..., DEP]
    return done, way, tt32.astype(np.float32)


def _rows(A, defect):
    """The agents a restatement visits."""
    first = 0 if defect == "dummy_counted" else 1
    last = A - 1 if defect == "last_agent_of_partial_tile_skipped" and A % TILE != 0 else A
    return first, last


def agent_stats(agents, agents_b=None, ff=None, defect=None):
    """``tarl_trip_agent_stats``: dict of (A,) arrays; entry 0 zero. fp64 sums over k = 0, 1, ... in ascending order."""
    K, A, _ = agents.shape
    done, way, tt32 = _flags(agents, defect)
    tt = tt32.astype(np.float64)
    out = {"n_done": np.zeros(A, np.int32), "n_way": np.zeros(A, np.int32), "tt_sum": np.zeros(A), "tt_sumsq": np.zeros(A),
           "tt_min": np.full(A, 0.0 if defect == "minmax_seeded_zero" else np.inf, np.float32),
           "tt_max": np.full(A, 0.0 if defect == "minmax_seeded_zero" else -np.inf, np.float32)}
    if ff is not None:
        out["n_under"] = np.zeros(A, np.int32)
    if agents_b is not None:
        done_b, _, tt32_b = _flags(agents_b, defect)
        d = tt - tt32_b.astype(np.float64)
        out.update(n_both=np.zeros(A, np.int32), d_sum=np.zeros(A), d_sumsq=np.zeros(A), n_faster=np.zeros(A, np.int32),
                   n_slower=np.zeros(A, np.int32))
    for k in range(K - 1 if defect == "last_env_skipped" else K):
        m = done[k]
        out["n_done"] += m
        out["n_way"] += way[k]
        out["tt_sum"] += np.where(m, tt[k], 0.0)
        out["tt_sumsq"] += np.where(m, tt[k] * tt[k], 0.0)
        out["tt_min"] = np.where(m, np.minimum(out["tt_min"], tt32[k]), out["tt_min"])
        out["tt_max"] = np.where(m, np.maximum(out["tt_max"], tt32[k]), out["tt_max"])
        if ff is not None:
            out["n_under"] += m & np.isfinite(ff) & (tt[k] < ff)
        if agents_b is not None:
            both = (m | done_b[k]) if defect == "pair_with_one_arrival" else (m & done_b[k])
            out["n_both"] += both
            out["d_sum"] += np.where(both, d[k], 0.0)
            out["d_sumsq"] += np.where(both, d[k] * d[k], 0.0)
            out["n_faster"] += both & ((d[k] <= 0) if defect == "faster_includes_equal" else (d[k] < 0))
            out["n_slower"] += both & (d[k] > 0)
    first, last = _rows(A, defect)
    for v in out.values():
        v[:first] = 0
        v[last:] = 0
    if last < A:            # (a skipped agent is left as the kernel's seed would leave it)
        out["tt_min"][last:], out["tt_max"][last:] = np.inf, -np.inf
    return {k: v.astype(np.int32) if v.dtype.kind in "ib" else v for k, v in out.items()}


def bin_stats(agents, bin_seconds, first_bin, H, ff=None, defect=None):
    """``tarl_trip_bin_stats``: dict of (K, H) arrays; fp64 sums over the agents 1, 2, ... in ascending order (np.add.at adds
    element by element)."""
    K, A, _ = agents.shape
    done, way, tt32 = _flags(agents, defect)
    tt = tt32.astype(np.float64)
    kw = dict(low=defect != "no_low_clamp", high=defect != "no_high_clamp")
    out = {"dep_done": np.zeros((K, H), np.int32), "dep_way": np.zeros((K, H), np.int32), "arr": np.zeros((K, H), np.int32),
           "dep_tt": np.zeros((K, H))}
    if ff is not None:
        out.update(dep_ff=np.zeros((K, H)), dep_ff_n=np.zeros((K, H), np.int32))
    first, last = _rows(A, defect)
    sel = np.zeros(A, bool)
    sel[first:last] = True
    for k in range(K - 1 if defect == "last_env_skipped" else K):
        hd = clock_bin(agents[k, :, DEP], bin_seconds, first_bin, H, **kw)
        ha = hd if defect == "arrivals_by_departure" else clock_bin(agents[k, :, ARR], bin_seconds, first_bin, H, **kw)
        m = sel & done[k] & (hd >= 0)
        np.add.at(out["dep_done"][k], hd[m], 1)
        np.add.at(out["dep_tt"][k], hd[m], tt[k][m])
        w = sel & way[k] & (hd >= 0)
        np.add.at(out["dep_way"][k], hd[w], 1)
        ma = sel & done[k] & (ha >= 0)
        np.add.at(out["arr"][k], ha[ma], 1)
        if ff is not None:
            f = m & (np.ones(A, bool) if defect == "ff_inf_added" else np.isfinite(ff))
            with np.errstate(invalid="ignore"):
                np.add.at(out["dep_ff"][k], hd[f], ff[f])
            np.add.at(out["dep_ff_n"][k], hd[f], 1)
    return out


def sum_bounds(agents, agents_b, ff, bin_seconds, first_bin, H):
    """n * 2^-53 * sum |x| of every fp64 sum, the worst-case bound of an n-term fp64 sum: the dict of the fp64 outputs of
    both entry points -> arrays of their shapes."""
    u = 2.0 ** -53
    done, _, tt32 = _flags(agents, None)
    tt = np.abs(tt32.astype(np.float64))
    n = done.sum(axis=0)
    out = {"tt_sum": n * u * np.where(done, tt, 0).sum(axis=0), "tt_sumsq": n * u * np.where(done, tt * tt, 0).sum(axis=0)}
    if agents_b is not None:
        done_b, _, tt32_b = _flags(agents_b, None)
        both = done & done_b
        d = np.abs(tt32.astype(np.float64) - tt32_b.astype(np.float64))
        nb = both.sum(axis=0)
        out.update(d_sum=nb * u * np.where(both, d, 0).sum(axis=0), d_sumsq=nb * u * np.where(both, d * d, 0).sum(axis=0))
    K, A, _ = agents.shape
    out["dep_tt"], out["dep_ff"] = np.zeros((K, H)), np.zeros((K, H))
    for k in range(K):
        hd = clock_bin(agents[k, :, DEP], bin_seconds, first_bin, H)
        m = done[k].copy()
        m[0] = False
        cnt = np.bincount(hd[m], minlength=H)
        out["dep_tt"][k] = cnt * u * np.bincount(hd[m], weights=tt[k][m], minlength=H)
        if ff is not None:
            f = m & np.isfinite(ff)
            out["dep_ff"][k] = np.bincount(hd[f], minlength=H) * u * np.bincount(hd[f], weights=np.abs(ff[f]), minlength=H)
    for v in out.values():
        if v.ndim == 1:
            v[0] = 0.0
    return out


# ---- the report's arithmetic -----------------------------------------------------------------------------------------------------
def moments(values):
    """mean, sd (ddof 1), se, interval of a list of numbers by numpy's own two-pass formulas: the mean needs one value, the
    others two (``None`` below)."""
    v = np.asarray(values, dtype=np.float64)
    out = {"mean": None, "sd": None, "se": None, "ci95_lo": None, "ci95_hi": None}
    if v.size >= 1:
        out["mean"] = float(v.mean())
    if v.size >= 2:
        sd = float(v.std(ddof=1))
        se = sd / math.sqrt(v.size)
        out.update(sd=sd, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


def classify(diffs):
    """The paired classification of one agent from its list of differences: ``None`` below two pairs, else "faster" (the 95 %
    interval lies entirely below 0), "slower" (entirely above) or "neither"; where se = 0 the sign of the mean decides."""
    if len(diffs) < 2:
        return None
    m = moments(diffs)
    lo, hi = (m["ci95_lo"], m["ci95_hi"]) if m["se"] > 0 else (m["mean"], m["mean"])
    return "faster" if hi < 0 else ("slower" if lo > 0 else "neither")


# ---- crafted cases -----------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 2), (2, 65), (63, 64), (64, 257), (65, 1025), (130, 300))        # K x A, A counting the dummy
BIN_SECONDS, FIRST_BIN, BINS = 100, 200, 4                                      # the stored clocks: [20 000, 20 400)
ROLES = 12


def _population(A, rng, fractional):
    """Origin, destination, departure (integer-valued, or integer + 0.25 / 0.5) and the free-flow time per agent. The role of
    agent a is (a - 1) % 12; role 4 departs before the first stored bin, role 5 past the last one, role 7 has ff = +inf."""
    pop = np.zeros((A, 9), np.float32)
    a = np.arange(A)
    role = (a - 1) % ROLES
    pop[:, ORIGIN], pop[:, DEST] = a % 17, (a * 7 + 3) % 19
    dep = 20000 + rng.integers(0, 300, size=A)
    dep = np.where(role == 4, 19000 + (a % 50), dep)
    dep = np.where(role == 5, 20900 + (a % 50), dep)
    dep = np.where(role == 6, 20250, dep)
    pop[:, DEP] = dep + (np.where(a % 2 == 0, 0.25, 0.5) if fractional else 0.0)
    ff = (10.0 + (a % 50)) * (1.1 if fractional else 1.0)      # 1.1: not a dyadic fraction, the fp64 sums round
    ff = np.where(role == 7, np.inf, ff)
    pop[0] = 0.0
    return pop, ff.astype(np.float64), role


def _tables(K, A, seed, fractional=False, middle_only=False):
    """The two agent tables (the run and its baseline) of one case. By role, for environment k:
      0, 8, 10, 11  arrive in every environment (tt 1 .. 300, integer-valued); the baseline too, its tt differing by -3, 0 or
                    +5 ((a + k) % 3): pairs with d > 0, d == 0 and d < 0
      1             arrives where k is even, on the way where k is odd; the baseline arrives everywhere (one-sided pairs)
      2             never departs here (flags 0); the baseline delivers it (arrived in the baseline alone)
      3             on the way in every environment, in both runs
      4, 5          as role 0 with the departure outside the stored bins (both clamps)
      6             departs at 20 250 and arrives in the last stored bin, 20 310 .. 20 339
      7             as role 0 with ff = +inf
      9             arrives everywhere with ON_WAY left at 1 (DONE decides); never arrives in the baseline
    A row that has not arrived keeps ARRIVAL_TIME 0, as after a reset."""
    rng = np.random.default_rng(seed)
    pop, ff, role = _population(A, rng, fractional)
    if middle_only:         # every clock inside one bin: the H = 3 case whose outer bins stay empty
        pop[1:, DEP] = 20000 + rng.integers(0, 40, size=A - 1)
    a = np.arange(A)
    ag, base = np.repeat(pop[None], K, axis=0), np.repeat(pop[None], K, axis=0)
    for k in range(K):
        tt = rng.integers(1, 60 if middle_only else 300, size=A).astype(np.float64)
        if not middle_only:
            tt = np.where(role == 6, 60 + (k % 30), tt)
        if fractional:
            tt = tt + np.float32(1.0 / 3.0)
        arrives = np.isin(role, (0, 4, 5, 6, 7, 8, 9, 10, 11)) | ((role == 1) & (k % 2 == 0))
        on_way = (role == 3) | ((role == 1) & (k % 2 == 1)) | (role == 9)
        ag[k, :, ARR] = np.where(arrives, (pop[:, DEP].astype(np.float64) + tt).astype(np.float32), 0.0)
        ag[k, :, DONE], ag[k, :, ON_WAY] = arrives, on_way
        delta = np.choose((a + k) % 3, (-3.0, 0.0, 5.0))
        b_arrives = np.isin(role, (0, 1, 2, 4, 5, 6, 7, 8, 10, 11))
        tb = np.where(role == 2, 40.0, np.maximum(tt + delta, 1.0))
        base[k, :, ARR] = np.where(b_arrives, (pop[:, DEP].astype(np.float64) + tb).astype(np.float32), 0.0)
        base[k, :, DONE], base[k, :, ON_WAY] = b_arrives, role == 3
    ag[:, 0], base[:, 0] = 0.0, 0.0
    ag[:, 0, DONE] = 1.0            # a dummy row that LOOKS arrived, with a travel time of 7: it must still be skipped
    ag[:, 0, ARR] = 7.0
    base[:, 0, DONE], base[:, 0, ARR] = 1.0, 7.0
    return ag, base, ff


def _case(name, K, A, seed, H=BINS, first_bin=FIRST_BIN, pad=0, **kw):
    ag, base, ff = _tables(K, A, seed, **kw)
    return dict(name=name, K=K, A=A, H=H, first_bin=first_bin, bin_seconds=BIN_SECONDS, pad=pad, agents=ag, agents_b=base,
                ff=ff, exact=not kw.get("fractional", False), full_roles=K >= 2 and A > ROLES and not kw.get("middle_only"))


def crafted_cases():
    """Every case of the GPU suite. The six shapes lie below, at and above one wave (64 lanes) and one workgroup (64 agents x
    16 environments per pass of the per-agent kernel; 256 agents per (environment, bin) segment and 1 024 agents per pass of
    the arrivals kernel) on each axis; 17 x 130 adds the kernel's own edge K = 16 + 1. Then: tables whose environments lie
    9 A + 5 floats apart; H = 1 (every clock clamped into the one bin); H = 3 with every clock in the middle bin; one
    fractional case (DEPARTURE_TIME = integer + 0.25 / 0.5, travel times with a third of a second, ff a multiple of 1.1).
    All other cases hold integer-valued times below 2^24: every summation order gives the same fp64 value and == is the
    test. Cases with ``full_roles`` hold all twelve roles of :func:`_tables` (K >= 2 and more than 12 agents)."""
    cases = [_case(f"{K}x{A}", K, A, seed=500 + i) for i, (K, A) in enumerate(SHAPES)]
    cases.append(_case("17x130", 17, 130, seed=520))
    cases.append(_case("stride-5x70", 5, 70, seed=521, pad=5))
    cases.append(_case("H1-6x40", 6, 40, seed=522, H=1))
    cases.append(_case("H3-outer-empty-6x40", 6, 40, seed=523, H=3, first_bin=199, middle_only=True))
    cases.append(_case("fractional-33x200", 33, 200, seed=524, fractional=True))
    return cases


def run_case(case, defect=None, paired=True):
    """Both restatements on one case -> (per agent, per bin)."""
    per_agent = agent_stats(case["agents"], case["agents_b"] if paired else None, case["ff"], defect=defect)
    per_bin = bin_stats(case["agents"], case["bin_seconds"], case["first_bin"], case["H"], case["ff"], defect=defect)
    return per_agent, per_bin


def same(a, b):
    """Two result dicts equal in every array, inf == inf."""
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
