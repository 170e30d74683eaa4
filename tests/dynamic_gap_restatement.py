"""TEST INFRASTRUCTURE: numpy restatement of the dynamic relative gap (``tarl_td_road_times``, ``tarl_td_hindsight`` and the
reductions of ``VecEvaluator(dynamic_gap=True)``), a brute-force enumeration of paths for graphs of at most 6 roads, the crafted
cases shared by the host and the GPU suite, and the same restatement with ONE deliberate defect at a time. Plain module: no
fixtures; nothing at import time needs a GPU.

Definitions (all fp64 unless said; S(h) = (first_bin + h) * bin_seconds):
  tau[k][h][n] = (float) max(FF[n], cc[n] / ((MAX[n] + 10) - veh[k][h][n] / frames_per_bin[h])), FF[n] for a bin without
                 frames, +inf for a denominator <= 0; max(v, FF) = v if v > FF else FF
  env[k][H][n] = +inf, env[k][h][n] = min(S(h) + tau[k][h][n], env[k][h + 1][n]), min(x, m) = x if x < m else m
  leave(n, t)  = min(t + tau[k][h][n], env[k][h + 1][n]) at h = clamp(floor(t) // bin_seconds - first_bin, 0, H - 1), a NaN or
                 negative clock taken as 0; +inf for t = +inf or NaN
  L[o] = leave(o, t0), L[v] = min over in-edges (u -> v) of leave(v, L[u]), best = L[d]; +inf for an unreachable d, an id out
  of range, row 0 and an agent with DONE != 1
  tt = fp32 ARRIVAL - DEPARTURE widened, ht = best - t0, g = tt - ht; a trip is usable when DONE == 1 and ht is finite."""
from __future__ import annotations

import heapq
import math

import numpy as np

ORIGIN, DEST, DEP, ARR, ON_WAY, DONE = 0, 1, 2, 3, 7, 8
INF = math.inf
DEFECTS = ("no_envelope", "bin_at_leaving_time", "departure_bin_for_path", "origin_not_traversed",
           "destination_not_traversed", "no_low_clamp", "no_high_clamp", "veh_not_divided", "gap_sign_turned")


# ---- road times and envelope ---------------------------------------------------------------------------------------------------
def road_tau(veh, frames_per_bin, max_agents, free_flow, cong, defect=None):
    """``tau`` fp32 (K, H, N)."""
    K, H, N = veh.shape
    ff, cc = np.asarray(free_flow, np.float32).astype(np.float64), np.asarray(cong, np.float32).astype(np.float64)
    room = np.asarray(max_agents, np.float32).astype(np.float64) + 10.0
    tau = np.empty((K, H, N), np.float32)
    for h in range(H):
        frames = int(frames_per_bin[h])
        if frames <= 0:
            tau[:, h, :] = ff.astype(np.float32)
            continue
        cbar = veh[:, h, :].astype(np.float64) / (1.0 if defect == "veh_not_divided" else float(frames))
        den = room[None, :] - cbar
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(den > 0.0, cc[None, :] / np.where(den > 0.0, den, 1.0), INF)
        tau[:, h, :] = np.where(v > ff[None, :], v, ff[None, :]).astype(np.float32)
    return tau


def envelope(tau, bin_seconds, first_bin, defect=None):
    """``env`` fp64 (K, H + 1, N) of ``tau`` fp32 (K, H, N)."""
    K, H, N = tau.shape
    env = np.full((K, H + 1, N), INF)
    if defect == "no_envelope":
        return env
    for h in range(H - 1, -1, -1):
        with np.errstate(invalid="ignore"):
            x = float((int(first_bin) + h) * int(bin_seconds)) + tau[:, h, :].astype(np.float64)
            env[:, h, :] = np.where(x < env[:, h + 1, :], x, env[:, h + 1, :])
    return env


def road_times(veh, frames_per_bin, max_agents, free_flow, cong, bin_seconds, first_bin, defect=None):
    """``tarl_td_road_times`` -> (tau, env)."""
    tau = road_tau(veh, frames_per_bin, max_agents, free_flow, cong, defect)
    return tau, envelope(tau, bin_seconds, first_bin, defect)


def raw_bin(t, bin_seconds, first_bin):
    """floor(t) // bin_seconds - first_bin, unclamped (t finite or +inf; NaN and negatives as 0)."""
    t = float(t)
    if not t > 0.0:
        t = 0.0
    if t >= 2.0 ** 62:
        return 1 << 62
    return int(math.floor(t)) // int(bin_seconds) - int(first_bin)


def clock_bin(t, bin_seconds, first_bin, H, defect=None):
    """The stored bin of a clock, or ``None`` where a missing clamp (a defect) lets it fall outside the tables."""
    q = raw_bin(t, bin_seconds, first_bin)
    if q < 0:
        return None if defect == "no_low_clamp" else 0
    if q > H - 1:
        return None if defect == "no_high_clamp" else H - 1
    return q


def leave(tau_k, env_k, n, t, bin_seconds, first_bin, defect=None, frozen=None, flags=None):
    """When an agent that enters road ``n`` at clock ``t`` has left it. ``frozen``: the bin to use whatever ``t`` (the defect
    ``departure_bin_for_path``). ``flags``: a set that gains "envelope" where waiting wins and "past_last_bin" where the
    clamp at the last bin acts."""
    t = float(t)
    if not t < INF:
        return INF
    H = tau_k.shape[0]
    h = clock_bin(t, bin_seconds, first_bin, H, defect) if frozen is None else frozen
    if h is None:
        return INF
    if defect == "bin_at_leaving_time":
        h2 = clock_bin(t + float(tau_k[h, n]), bin_seconds, first_bin, H)
        h = h if h2 is None else h2
    x = t + float(tau_k[h, n])
    m = float(env_k[h + 1, n]) if frozen is None else INF       # one bin for the whole path: static times, nothing to wait for
    if flags is not None:
        if m < x:
            flags.add("envelope")
        if raw_bin(t, bin_seconds, first_bin) > H - 1:
            flags.add("past_last_bin")
    return x if x < m else m


# ---- the hindsight arrival -------------------------------------------------------------------------------------------------------
def out_lists(edge_index, N):
    lists = [[] for _ in range(N)]
    for s, d in np.asarray(edge_index).T.tolist():
        lists[int(s)].append(int(d))
    return lists


def searched(row, a, N):
    """(origin, destination) of an agent row that is searched, else ``None``."""
    o, d = float(row[ORIGIN]), float(row[DEST])
    if a < 1 or row[DONE] != 1.0 or not (0.0 <= o < N) or not (0.0 <= d < N):
        return None
    return int(o), int(d)


def hindsight_one(outs, tau_k, env_k, o, d, t0, bin_seconds, first_bin, defect=None, pred=None):
    """Heap-based time-dependent Dijkstra from road ``o`` entered at ``t0`` -> the clock at which ``d`` is left. leave is
    non-decreasing in t and never below t (tau >= 0), so a label is final when it is popped. ``pred``: a list of N that
    receives the predecessor of every labelled road (-1 at the origin)."""
    N = len(outs)
    frozen = clock_bin(t0, bin_seconds, first_bin, tau_k.shape[0]) if defect == "departure_bin_for_path" else None
    kw = dict(bin_seconds=bin_seconds, first_bin=first_bin, defect=defect, frozen=frozen)
    L = [INF] * N
    enter = [INF] * N           # the clock at which the road is entered on the best path (destination_not_traversed)
    enter[o] = float(t0)
    L[o] = float(t0) if defect == "origin_not_traversed" else leave(tau_k, env_k, o, t0, **kw)
    heap = [(L[o], o)] if L[o] < INF else []
    while heap:
        lu, u = heapq.heappop(heap)
        if lu > L[u]:
            continue
        for v in outs[u]:
            lv = leave(tau_k, env_k, v, lu, **kw)
            if lu < enter[v]:
                enter[v] = lu
            if lv < L[v]:
                L[v] = lv
                if pred is not None:
                    pred[v] = u
                heapq.heappush(heap, (lv, v))
    if defect == "destination_not_traversed":
        return enter[d] if L[d] < INF or d == o else INF
    return L[d]


def hindsight(edge_index, N, tau, env, agents, bin_seconds, first_bin, defect=None):
    """``tarl_td_hindsight`` -> best fp64 (K, A)."""
    K, A, _ = agents.shape
    outs = out_lists(edge_index, N)
    best = np.full((K, A), INF)
    for k in range(K):
        for a in range(A):
            od = searched(agents[k, a], a, N)
            if od is not None:
                best[k, a] = hindsight_one(outs, tau[k], env[k], od[0], od[1], float(agents[k, a, DEP]), bin_seconds,
                                           first_bin, defect)
    return best


def hindsight_path(outs, tau_k, env_k, o, d, t0, bin_seconds, first_bin):
    """(arrival, the roads of one best path o .. d), the path ``None`` where d is unreachable."""
    pred = [-1] * len(outs)
    best = hindsight_one(outs, tau_k, env_k, o, d, t0, bin_seconds, first_bin, pred=pred)
    if not best < INF:
        return best, None
    path = [d]
    while path[-1] != o:
        path.append(pred[path[-1]])
    return best, path[::-1]


def along(path, tau_k, env_k, t0, bin_seconds, first_bin):
    """The clock at which the last road of ``path`` is left by an agent that enters its first road at ``t0``."""
    t = float(t0)
    for n in path:
        t = leave(tau_k, env_k, n, t, bin_seconds, first_bin)
    return t


def simple_paths(outs, o, d):
    """Every simple path o -> d as a list of roads (o == d: the road alone)."""
    if o == d:
        return [[o]]
    found, stack = [], [[o]]
    while stack:
        p = stack.pop()
        for v in outs[p[-1]]:
            if v == d:
                found.append(p + [v])
            elif v not in p:
                stack.append(p + [v])
    return found


def brute_paths(outs, tau_k, env_k, o, d, t0, bin_seconds, first_bin, frozen=None):
    """[(leaving time of d, path, flags)] over every simple path, leave composed road by road."""
    out = []
    for p in simple_paths(outs, o, d):
        t, flags = float(t0), set()
        for n in p:
            t = leave(tau_k, env_k, n, t, bin_seconds, first_bin, frozen=frozen, flags=flags)
        out.append((t, p, flags))
    return out


def brute(edge_index, N, tau, env, agents, bin_seconds, first_bin):
    """best (K, A) by enumeration (graphs of at most 6 roads)."""
    assert N <= 6
    K, A, _ = agents.shape
    outs = out_lists(edge_index, N)
    best = np.full((K, A), INF)
    for k in range(K):
        for a in range(A):
            od = searched(agents[k, a], a, N)
            if od is not None:
                vals = [v for v, _, _ in brute_paths(outs, tau[k], env[k], od[0], od[1], float(agents[k, a, DEP]),
                                                    bin_seconds, first_bin)]
                best[k, a] = min(vals) if vals else INF
    return best


# ---- the gap and its reductions -------------------------------------------------------------------------------------------------
def gap(agents, best, defect=None):
    """-> (tt, ht, g, usable), each (K, A): tt fp32 ARRIVAL - DEPARTURE widened, ht = best - t0, g = tt - ht."""
    tt = (agents[..., ARR] - agents[..., DEP]).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ht = best - agents[..., DEP].astype(np.float64)
        g = (ht - tt) if defect == "gap_sign_turned" else (tt - ht)
    usable = (agents[..., DONE] == 1.0) & np.isfinite(ht)
    usable[:, 0] = False
    return tt, ht, g, usable


def reductions(agents, best, dep_bin, H, defect=None):
    """What the evaluator reduces from (K, A), in plain ascending order: per agent over the environments (n, g_sum, g_sumsq,
    g_min, g_max, n_neg), per environment (tt_sum, ht_sum, n, n_neg, n_nonpos) and per (environment, departure bin) (g_sum, n).
    ``dep_bin`` int (A,): the departure bin of every agent."""
    tt, ht, g, use = gap(agents, best, defect)
    K, A = g.shape
    z = np.where(use, g, 0.0)
    per_agent = {"n": use.sum(axis=0).astype(np.int64), "g_sum": z.sum(axis=0), "g_sumsq": (z * z).sum(axis=0),
                 "g_min": np.where(use, g, INF).min(axis=0), "g_max": np.where(use, g, -INF).max(axis=0),
                 "n_neg": (use & (g < 0)).sum(axis=0).astype(np.int64)}
    per_env = {"tt_sum": np.where(use, tt, 0.0).sum(axis=1), "ht_sum": np.where(use, ht, 0.0).sum(axis=1),
               "n": use.sum(axis=1).astype(np.int64), "n_neg": (use & (g < 0)).sum(axis=1).astype(np.int64),
               "n_nonpos": (use & (g <= 0)).sum(axis=1).astype(np.int64)}
    per_bin = {"g_sum": np.zeros((K, H)), "n": np.zeros((K, H), np.int64)}
    for k in range(K):
        np.add.at(per_bin["g_sum"][k], dep_bin[use[k]], g[k][use[k]])
        np.add.at(per_bin["n"][k], dep_bin[use[k]], 1)
    return per_agent, per_env, per_bin


def relative_gaps(per_env):
    """RG_k = (sum tt - sum ht) / sum tt per environment, ``None`` without a usable trip."""
    return [float((per_env["tt_sum"][k] - per_env["ht_sum"][k]) / per_env["tt_sum"][k]) if per_env["n"][k] > 0 else None
            for k in range(len(per_env["n"]))]


def moments(values):
    v = np.asarray([x for x in values if x is not None], dtype=np.float64)
    out = {"n": int(v.size), "mean": None, "sd": None, "se": None, "ci95_lo": None, "ci95_hi": None}
    if v.size >= 1:
        out["mean"] = float(v.mean())
    if v.size >= 2:
        sd = float(v.std(ddof=1))
        se = sd / math.sqrt(v.size)
        out.update(sd=sd, se=se, ci95_lo=out["mean"] - 1.96 * se, ci95_hi=out["mean"] + 1.96 * se)
    return out


# ---- crafted cases ---------------------------------------------------------------------------------------------------------------
SITUATIONS = ("o_equals_d", "unreachable", "dead_end", "tie", "later_bin_slower", "envelope", "past_last_bin",
              "before_first_bin", "inf_in_one_bin", "bin_without_frames", "not_done", "dummy_row")


def _agents(K, rows):
    """rows: (origin, destination, departure, DONE per environment) per agent, the dummy first. ARRIVAL = departure + 40 +
    5 a (whole seconds) where the agent arrived."""
    A = len(rows)
    ag = np.zeros((K, A, 9), np.float32)
    for a, (o, d, dep, done) in enumerate(rows):
        ag[:, a, ORIGIN], ag[:, a, DEST], ag[:, a, DEP] = o, d, dep
        for k in range(K):
            ag[k, a, DONE] = done[k]
            ag[k, a, ON_WAY] = 0 if done[k] else 1
            ag[k, a, ARR] = dep + 40 + 5 * a if done[k] else 0
    return ag


def master_case():
    """Six roads, K = 2, bins of 100 s from bin 2, H = 4 of which bin 2 has no frames. Edges 0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3,
    3 -> 4, 5 -> 0: road 4 is a dead end, road 5 cannot be reached. MAX = 10, FF = 10, cc = 200, so tau = 200 / (20 - cbar):
    10, 20, 40, 100, +inf at cbar 0, 10, 15, 18, 20. Environment 0: tau = 10 everywhere, +inf on road 3 in bin 1 only.
    Environment 1: road 1 (10, 40, 10, 10), road 2 (20, 20, 10, 20), road 4 (10, 100, 10, 10), else 10. ``want``: the
    hand-computed hindsight arrivals (test_dynamic_gap_host.test_master_case_by_hand derives them)."""
    N, K, H, frames = 6, 2, 4, 4
    edges = np.array([[0, 0, 1, 2, 3, 5], [1, 2, 3, 3, 4, 0]], dtype=np.int64)
    cbar = np.zeros((K, H, N), np.int64)
    cbar[0, 1, 3] = 20
    cbar[1, 1, 1], cbar[1, :, 2], cbar[1, 1, 4] = 15, 10, 18
    veh = (cbar * frames).astype(np.int32)
    veh[:, 2, :] = 77                                   # the bin without frames: whatever it holds is not read
    one = (1, 1)
    rows = [(0, 3, 205, one),                           # 0 the dummy, looking like an arrived agent
            (0, 3, 205, one),                           # 1 two paths that tie (environment 0)
            (0, 3, 295, one),                           # 2 road 2 wins only because road 1 is slower in bin 1 (environment 1);
            #                                               +inf on road 3 in bin 1, left at the start of bin 2 (environment 0)
            (3, 3, 250, one),                           # 3 o == d
            (0, 5, 205, one),                           # 4 unreachable
            (3, 4, 380, one),                           # 5 road 4 drops from 100 to 10 at the bin edge: waiting wins (env. 1)
            (0, 1, 150, one),                           # 6 departs before the first stored bin
            (0, 4, 585, one),                           # 7 labels past the last bin; ends in the dead end
            (2, 3, 210, (0, 1)),                        # 8 not DONE in environment 0
            (1, 3, 295, one)]                           # 9 enters road 1 in bin 0 and leaves it in bin 1
    want = np.array([[INF, 235, 410, 260, INF, 420, 170, 625, INF, 410],
                     [INF, 235, 335, 260, INF, 410, 170, 625, 240, 315]], dtype=np.float64)
    return dict(name="master", N=N, K=K, H=H, bin_seconds=100, first_bin=2, edges=edges, veh=veh,
                frames_per_bin=np.array([frames, frames, 0, frames], np.int32), max_agents=np.full(N, 10, np.float32),
                free_flow=np.full(N, 10, np.float32), cong=np.full(N, 200, np.float32), agents=_agents(K, rows), want=want,
                must=SITUATIONS)


def _random_small(seed, N, K, H, A, bin_seconds, first_bin):
    """A random graph of at most 6 roads with fractional road times (FF a multiple of 0.7, counts up to the capacity)."""
    rng = np.random.default_rng(seed)
    pairs = [(s, d) for s in range(N) for d in range(N) if s != d and rng.random() < 0.45]
    edges = np.array(pairs, dtype=np.int64).T.reshape(2, -1)
    frames = rng.integers(0, 5, size=H).astype(np.int32)
    frames[0] = max(int(frames[0]), 1)
    mx = rng.choice(np.array([2.0, 5.0, 14.0], np.float32), size=N)
    ff = (0.7 * rng.integers(1, 60, size=N)).astype(np.float32)
    cc = (ff.astype(np.float64) * (mx + 10.0 - 0.5)).astype(np.float32)
    veh = (rng.integers(0, 17, size=(K, H, N)) * np.maximum(frames, 1)[None, :, None]).astype(np.int32)
    start = first_bin * bin_seconds
    rows = [(0, 0, start, (1,) * K)]
    for a in range(1, A):
        rows.append((int(rng.integers(0, N)), int(rng.integers(0, N)),
                     float(start + rng.integers(-bin_seconds, (H + 1) * bin_seconds)) + (0.5 if a % 3 == 0 else 0.0),
                     tuple(int(rng.random() < 0.85) for _ in range(K))))
    return dict(name=f"random-{N}x{K}x{H}-{seed}", N=N, K=K, H=H, bin_seconds=bin_seconds, first_bin=first_bin, edges=edges,
                veh=veh, frames_per_bin=frames, max_agents=mx, free_flow=ff, cong=cc, agents=_agents(K, rows), want=None,
                must=())


def crafted_cases():
    """The master case (every situation of :data:`SITUATIONS`), one road alone (N = K = H = 1, o == d), and random graphs of
    2 to 6 roads with fractional times, H in {1, 2, 5}, bins of 7, 60 and 100 s and one of 1 s (the quotient without a
    division). All have at most 6 roads: the enumeration of paths checks every one of them."""
    one = dict(name="one-road", N=1, K=1, H=1, bin_seconds=3600, first_bin=5, edges=np.zeros((2, 0), np.int64),
               veh=np.array([[[8]]], np.int32), frames_per_bin=np.array([2], np.int32), max_agents=np.array([5], np.float32),
               free_flow=np.array([12.5], np.float32), cong=np.array([12.5 * 14], np.float32),
               agents=_agents(1, [(0, 0, 18000, (1,)), (0, 0, 18010, (1,)), (0, 0, 18020, (0,))]), want=None,
               must=("o_equals_d", "not_done", "dummy_row"))
    cases = [master_case(), one]
    for i, (N, K, H, bs, fb) in enumerate(((2, 1, 1, 100, 3), (3, 2, 2, 7, 40), (5, 3, 5, 60, 10), (6, 2, 5, 100, 0),
                                           (6, 3, 2, 1, 500), (4, 2, 5, 7, 1))):
        cases.append(_random_small(700 + i, N, K, H, 24, bs, fb))
    return cases


def run_case(case, defect=None):
    """-> (tau, env, best) of the restatement, with at most one defect."""
    tau, env = road_times(case["veh"], case["frames_per_bin"], case["max_agents"], case["free_flow"], case["cong"],
                          case["bin_seconds"], case["first_bin"], defect)
    return tau, env, hindsight(case["edges"], case["N"], tau, env, case["agents"], case["bin_seconds"], case["first_bin"], defect)


def situations(case):
    """The situations of :data:`SITUATIONS` that ``case`` holds, found from the true tables and the enumeration of paths."""
    tau, env, best = run_case(case)
    N, K, H, bs, fb, ag = case["N"], case["K"], case["H"], case["bin_seconds"], case["first_bin"], case["agents"]
    outs = out_lists(case["edges"], N)
    found = set()
    if (np.asarray(case["frames_per_bin"]) == 0).any():
        found.add("bin_without_frames")
    if (np.isinf(tau).sum(axis=1) == 1).any() and H > 1:
        found.add("inf_in_one_bin")
    if (ag[:, 1:, DONE] != 1.0).any():
        found.add("not_done")
    if (ag[:, 0, DONE] == 1.0).all() and 0 <= ag[0, 0, ORIGIN] < N and np.isinf(best[:, 0]).all():
        found.add("dummy_row")
    for k in range(K):
        for a in range(1, ag.shape[1]):
            od = searched(ag[k, a], a, N)
            if od is None:
                continue
            o, d = od
            t0 = float(ag[k, a, DEP])
            if o == d:
                found.add("o_equals_d")
            if raw_bin(t0, bs, fb) < 0:
                found.add("before_first_bin")
            paths = brute_paths(outs, tau[k], env[k], o, d, t0, bs, fb)
            if not paths:
                found.add("unreachable")
                continue
            if not outs[d]:
                found.add("dead_end")
            lo = min(v for v, _, _ in paths)
            winners = [(p, f) for v, p, f in paths if v == lo]
            if len(winners) >= 2 and lo < INF:
                found.add("tie")
            for _, f in winners:
                found |= f
            frozen = brute_paths(outs, tau[k], env[k], o, d, t0, bs, fb, frozen=clock_bin(t0, bs, fb, H))
            flo = min(v for v, _, _ in frozen)
            if lo < INF and {tuple(p) for v, p, _ in frozen if v == flo}.isdisjoint({tuple(p) for p, _ in winners}):
                found.add("later_bin_slower")
    return found


# ---- random road times on larger graphs (the GPU suite) --------------------------------------------------------------------------
def random_edges(N, seed):
    """(2, E) int64: about one road in eight is a dead end; every other road leads to the next one (a ring, so that most pairs
    are connected) and to up to three random others, no edge twice; the edge list is shuffled: neither source- nor
    destination-sorted."""
    rng = np.random.default_rng(seed)
    pairs = set()
    for s in range(N):
        if N > 2 and rng.random() < 0.125:
            continue
        if N > 1:
            pairs.add((s, (s + 1) % N))
        for _ in range(int(rng.integers(0, 4)) if N > 2 else 0):
            d = int(rng.integers(0, N - 1))
            pairs.add((s, d + (d >= s)))
    pairs = sorted(pairs)
    order = rng.permutation(len(pairs))
    return np.array([pairs[i] for i in order], dtype=np.int64).T.reshape(2, -1)


def random_tau(K, H, N, seed):
    """tau fp32 (K, H, N): fractional times in [0.5, 90), about 3 % of them +inf, one NaN where there is room, a few zeros."""
    rng = np.random.default_rng(seed)
    tau = (0.5 + 89.5 * rng.random((K, H, N))).astype(np.float32)
    tau[rng.random((K, H, N)) < 0.03] = np.inf
    tau[rng.random((K, H, N)) < 0.02] = 0.0
    if N >= 4:
        tau[K - 1, H - 1, N // 2] = np.nan
    return tau


def random_agents(K, A, N, H, bin_seconds, first_bin, seed):
    """(K, A, 9) fp32: one population, departures from one bin before the stored ones to one bin past them (half of them with
    a fraction), about one agent in ten not DONE in an environment, two agents with an id out of range; row 0 looks arrived."""
    rng = np.random.default_rng(seed)
    start = first_bin * bin_seconds
    rows = [(0, min(1, N - 1), start + 1, (1,) * K)]
    for a in range(1, A):
        dep = float(start + rng.integers(-bin_seconds, (H + 1) * bin_seconds)) + (0.25 if a % 2 else 0.0)
        rows.append((int(rng.integers(0, N)), int(rng.integers(0, N)), max(dep, 0.0), tuple(int(rng.random() < 0.9) for _ in range(K))))
    ag = _agents(K, rows)
    if A > 4:
        ag[:, 2, ORIGIN], ag[:, 3, DEST] = N, -1.0
        ag[:, 2:4, DONE] = 1
    return ag
