"""Per-decision PPO credit restated in numpy float64 (TEST INFRASTRUCTURE): who a road decides for, the
traveller's frames to go against its free-flow frames to go, the statistics over the live decisions, and the clipped
objective per live road with its gradient. ``defect`` names one deliberate mistake (DEFECTS): test_decision_credit_host shows
that each of them moves a named case by at least ten times the tolerance the GPU tests use.

Plain loops over (row, road): the cases are small, and the order of every sum is written out."""
import numpy as np

ORIGIN, DESTINATION, DEPARTURE_TIME, ARRIVAL_TIME, ON_WAY, DONE = 0, 1, 2, 3, 7, 8
LOG_EPS_P = 1e-8
STD_FLOOR = 1e-6

DEFECTS = ("arrival_frame_owed",      # the frame that withdraws the traveller counted as owed (times[k] <= ARRIVAL_TIME)
           "never_arrived_as_arrived",  # DONE not looked at: a lost traveller read as arrived at its initial ARRIVAL_TIME
           "stale_head",              # an empty road credited with the head id its word still holds
           "wrong_env",               # the agent row of the next environment
           "dist_transposed",         # dist[u][s] for dist[s][u]
           "stats_over_all",          # mean / std over every (row, road) element instead of the live ones
           "clip_wrong_side",         # the clip taken on the ratio (min(r, clamp r) A): the wrong side for a negative advantage
           "no_p_factor",             # the factor p / (p + 1e-8) missing from the gradient
           "no_temperature",          # the 1 / temperature missing from the gradient
           "skip_last_of_long")       # the last entry of an out-list longer than four skipped


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


def out_lists(edge_index, N):
    """The plan's CSR order: per node the ORIGINAL edge ids of its out-edges, a stable sort of the edge list by source."""
    src = np.asarray(edge_index[0], dtype=np.int64)
    order = np.argsort(src, kind="stable")
    cut = np.searchsorted(src[order], np.arange(N + 1))
    return [order[cut[u]:cut[u + 1]] for u in range(N)]


def heads(x, Nmax, defect=None):
    """x (B, N, F) exported state -> int64 (B, N): FIFO slot 0 where NUMBER_OF_AGENT > 0, else 0."""
    _check(defect)
    x = np.asarray(x, dtype=np.float64)
    h = x[..., 0].astype(np.int64)
    return h if defect == "stale_head" else np.where(x[..., 3 * Nmax + 1] > 0, h, 0)


def owed(n, gamma):
    """S(n): n for gamma == 1, (1 - gamma^n) / (1 - gamma) otherwise."""
    n = np.float64(n)
    return n if gamma == 1.0 else (1.0 - np.float64(gamma) ** n) / (1.0 - np.float64(gamma))


def frames_to_go(times, t, t_end, done, arrival, defect=None):
    """n: the frames k in [t, t_end) with times[k] < ARRIVAL_TIME where the traveller is DONE, found by searching the
    clocks; t_end - t (and truncated) otherwise. -> (n, truncated)."""
    if done != 1.0 and defect != "never_arrived_as_arrived":
        return t_end - t, True
    seg = np.asarray(times[t:t_end], dtype=np.float32)
    side = "right" if defect == "arrival_frame_owed" else "left"
    return int(np.searchsorted(seg, np.float32(arrival), side=side)), False


def decision_advantage(head_keep, frame, env, agents, times, t_end, dist, dest_slot, out_deg, timestep=1.0, gamma=1.0,
                       defect=None):
    """head_keep (rows, N) int: the captured heads; frame / env (rows,); agents (B, A, 9) as the segment's last frame left
    them; times: the frame clocks (fp32 values); dist (D, N) float64; dest_slot (N,); out_deg (N,).
    -> dict: adv (rows, N) float64 (0 where not live), live (rows, N) bool, n (rows, N) int (-1 where not live),
    truncated, bad."""
    _check(defect)
    head_keep = np.asarray(head_keep, dtype=np.int64)
    agents = np.asarray(agents)
    dist = np.asarray(dist, dtype=np.float64)
    rows, N = head_keep.shape
    B, A = agents.shape[0], agents.shape[1]
    D = dist.shape[0]
    adv = np.zeros((rows, N))
    live = np.zeros((rows, N), dtype=bool)
    nn = np.full((rows, N), -1, dtype=np.int64)
    truncated = bad = 0
    for j in range(rows):
        t, b = int(frame[j]), int(env[j])
        if not (0 <= t < t_end and 0 <= b < B):
            continue
        tab = agents[(b + 1) % B] if defect == "wrong_env" else agents[b]
        for u in range(N):
            a = int(head_keep[j, u])
            if a <= 0:
                continue
            if a >= A:
                bad += 1
                continue
            if out_deg[u] == 0:
                continue
            d = float(tab[a, DESTINATION])
            if not (0 <= d < N):
                continue
            s = int(dest_slot[int(d)])
            if not (0 <= s < D):
                continue
            du = dist.reshape(-1)[u * D + s] if defect == "dist_transposed" else dist[s, u]
            if not np.isfinite(du):
                continue
            n, trunc = frames_to_go(times, t, t_end, float(tab[a, DONE]), float(tab[a, ARRIVAL_TIME]), defect)
            truncated += int(trunc)
            adv[j, u] = owed(du / np.float64(timestep), gamma) - owed(n, gamma)        # G - G_ff = -S(n) + S(n_ff)
            live[j, u] = True
            nn[j, u] = n
    return dict(adv=adv, live=live, n=nn, truncated=truncated, bad=bad)


def decision_stats(adv32, live, defect=None):
    """{sum, sum of squares, count} of the fp32 raw advantages over the live decisions, in float64."""
    _check(defect)
    a = np.asarray(adv32, dtype=np.float32).astype(np.float64)
    m = np.ones_like(a, dtype=bool) if defect == "stats_over_all" else np.asarray(live, dtype=bool)
    v = a[m]
    return np.array([v.sum(), (v * v).sum(), float(v.size)])


def normalise(adv, stats, dtype=np.float64):
    """tarl_advantage_normalize's rule: (A - mean) / max(std, 1e-6), unbiased std."""
    cnt = stats[2]
    mean = stats[0] / cnt
    with np.errstate(invalid="ignore", divide="ignore"):
        var = (stats[1] - cnt * mean * mean) / (cnt - 1.0)
    var = var if var >= 0.0 else 0.0
    sd = max(dtype(np.sqrt(var)), dtype(STD_FLOOR))
    return (np.asarray(adv, dtype=dtype) - dtype(mean)) / sd


def _softmax(z, dtype):
    """k_softmax's expressions: the max subtracted, the sum left to right."""
    mx = z.max()
    e = np.exp(z - mx, dtype=dtype)
    s = dtype(0.0)
    for v in e:
        s = dtype(s + v)
    return e / s


def node_logprob(edge_index, N, logits, choice, temperature=1.0, dtype=np.float64):
    """(M, N): log(p_choice + 1e-8); 0 where ``choice`` (M, N) edge ids, -1: none names no out-edge of the node."""
    lists = out_lists(edge_index, N)
    logits = np.asarray(logits, dtype=dtype)
    M = logits.shape[0]
    out = np.zeros((M, N), dtype=dtype)
    for m in range(M):
        for u in range(N):
            es, c = lists[u], int(choice[m, u])
            if c < 0 or c not in es:
                continue
            p = _softmax(logits[m, es] / dtype(temperature), dtype)
            out[m, u] = np.log(p[list(es).index(c)] + dtype(LOG_EPS_P), dtype=dtype)
    return out


def decision_ppo(edge_index, N, logits, choice, live, lp_old, adv_raw, stats, n_live, clip_epsilon=0.2, temperature=1.0,
                 grad_scale=1.0, dtype=np.float64, defect=None):
    """The objective of DESIGN 4.26 on the live decisions of a minibatch, forward and backward.
    -> dict: out4 (M, 4) = per sample {sum of s, live, ratios outside the clip, sum of lp_old - lp}; grad (M, E): the
    gradient of -(grad_scale / L) sum s with respect to the logits (0 off the live nodes); objective = -(1 / L) sum s."""
    _check(defect)
    lists = out_lists(edge_index, N)
    logits = np.asarray(logits, dtype=dtype)
    M, E = logits.shape
    T = dtype(temperature)
    eps = dtype(clip_epsilon)
    a_hat = normalise(np.asarray(adv_raw, dtype=np.float32), stats, dtype)
    out4 = np.zeros((M, 4))
    grad = np.zeros((M, E), dtype=dtype)
    L = int(n_live)
    for m in range(M):
        for u in range(N):
            es, c = lists[u], int(choice[m, u])
            if not live[m, u] or c < 0 or c not in es:
                continue
            if defect == "skip_last_of_long" and len(es) > 4:
                es = es[:-1]
                if c not in es:
                    continue
            at = list(es).index(c)
            p = _softmax(logits[m, es] / T, dtype)
            lp = np.log(p[at] + dtype(LOG_EPS_P), dtype=dtype)
            lo = dtype(lp_old[m, u])
            r = np.exp(lp - lo, dtype=dtype)
            a = a_hat[m, u]
            rc = min(max(r, dtype(1.0) - eps), dtype(1.0) + eps)
            g1, g2 = r * a, rc * a
            if defect == "clip_wrong_side":
                flows = r <= rc
                s = min(r, rc) * a
            else:
                flows = g1 <= g2                    # the unclipped term is the minimum; a tie flows
                s = g1 if flows else g2
            out4[m] += (float(s), 1.0, float(r < 1.0 - eps or r > 1.0 + eps), float(lo - lp))
            if flows and L > 0:
                pf = dtype(1.0) if defect == "no_p_factor" else p[at] / (p[at] + dtype(LOG_EPS_P))
                coef = -(dtype(grad_scale) / dtype(L)) * g1 * pf
                one = np.zeros(len(es), dtype=dtype)
                one[at] = 1.0
                grad[m, es] += coef * (one - p) / (dtype(1.0) if defect == "no_temperature" else T)
    tot = out4.sum(0)
    return dict(out4=out4, grad=grad, objective=-tot[0] / max(tot[1], 1.0), a_hat=a_hat)
