"""TEST INFRASTRUCTURE: the per-agent path trace of the vectorised evaluation (csrc/path_trace.hip) written out in
plain numpy, element by element, and the per-agent reduction summed in the kernel's order. The same rule is available with ONE
defect at a time (:data:`DEFECTS`): what a wrong kernel would compute, for the tests that show the right one matters.

State per (environment b, agent a), a in [1, A): last_road (-1), roads, revisits, off_tree (0) int32, path_cost, excess (0.0)
fp64, route int32 [L] (-1); bad int32 per environment. One sighting pass after every frame over the packed words
``hdp[u][b] = head_id << 8 | count byte`` (count = bits 0..6; bit 7 is the packed state's DIRTY flag)."""
import numpy as np

DEFECTS = ("count_dropped",        # the count test dropped: a stale head id on an empty row is a sighting
           "same_road_appended",   # p == u appended again
           "last_match",           # the LAST entry of p's out-list that leads to u instead of the first
           "excess_reordered",     # w + (dist[u] - dist[p]) instead of (w + dist[u]) - dist[p]
           "scan_all_h",           # the revisit scan over h entries of the route instead of min(h, L)
           "wrong_env_dest")       # the destination of environment 0's agent table


def new_state(B, A, L):
    return dict(last_road=np.full((B, A), -1, np.int32), roads=np.zeros((B, A), np.int32), revisits=np.zeros((B, A), np.int32),
                off_tree=np.zeros((B, A), np.int32), path_cost=np.zeros((B, A), np.float64),
                excess=np.zeros((B, A), np.float64), route=np.full((B, A, L), -1, np.int32), bad=np.zeros(B, np.int32))


def csr(edge_index, N):
    """-> (out_ptr (N + 1,), out_dst (E,), out_eid (E,)): the out-lists by source, a stable sort of the caller's edge order
    (the plan's CSR, GraphDistribution's sorted order)."""
    src, dst = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(N + 1, np.int64)
    np.add.at(ptr, src + 1, 1)
    return np.cumsum(ptr), dst[order], order


def _candidates(st, hd, A, defect):
    """The (road, environment) pairs the loop below has to look at, in its order. Only a shortcut for long test runs: where
    every head id stands once per environment, an element whose head was last seen on this very road cannot be an event and
    is skipped before the loop; where an id stands twice (which the simulator never shows) every pair is looked at."""
    N, B = hd.shape
    full = [(u, b) for u in range(N) for b in range(B)]
    if defect is not None:
        return full
    a = hd >> 8
    live = ((hd & 0x7F) != 0) & (a != 0)
    for b in range(B):
        ids = a[live[:, b], b]
        if np.unique(ids).size != ids.size:
            return full
    inside = live & (a < A)
    lr = np.full(hd.shape, -2, np.int64)
    uu, bb = np.nonzero(inside)
    lr[uu, bb] = st["last_road"][bb, a[uu, bb]]
    event = live & (~inside | (lr != np.arange(N)[:, None]))
    return list(zip(*np.nonzero(event)))


def sighting_pass(st, hd, graph, a_dest=None, weights=None, dist=None, dest_slot=None, *, defect=None):
    """One pass over ``hd`` uint32 / int (N, B) — word 0 of the packed pairs after a frame — in place on ``st``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    ptr, dst, eid = graph
    hd = np.asarray(hd).astype(np.int64) & 0xFFFFFFFF
    N, B = hd.shape
    A, L = st["roads"].shape[1], st["route"].shape[2]
    for u, b in _candidates(st, hd, A, defect):      # (u, b) ascending, u the outer index
        w0 = int(hd[u, b])
        if (w0 & 0x7F) == 0 and defect != "count_dropped":
            continue
        a = w0 >> 8
        if a == 0:
            continue
        if a >= A:
            st["bad"][b] += 1
            continue
        p = int(st["last_road"][b, a])
        if p == u and defect != "same_road_appended":
            continue
        h = int(st["roads"][b, a])
        if p >= 0 and p != u:
            cand = [q for q in range(int(ptr[p]), int(ptr[p + 1])) if int(dst[q]) == u]
            if not cand:
                st["bad"][b] += 1
            elif weights is not None:
                e = cand[-1] if defect == "last_match" else cand[0]
                w = np.float64(np.float32(weights[eid[e]]))
                st["path_cost"][b, a] += w
                d = int(a_dest[0 if defect == "wrong_env_dest" else b, a])
                s = int(dest_slot[d]) if 0 <= d < N else -1
                ok = 0 <= s < dist.shape[0] and np.isfinite(dist[s, u]) and np.isfinite(dist[s, p])
                if not ok:
                    st["off_tree"][b, a] += 1
                elif defect == "excess_reordered":
                    st["excess"][b, a] += w + (np.float64(dist[s, u]) - np.float64(dist[s, p]))
                else:
                    st["excess"][b, a] += (w + np.float64(dist[s, u])) - np.float64(dist[s, p])
        if defect == "scan_all_h":
            # (a kernel scanning h entries would run past the kept prefix into its neighbours' routes; the defect is
            #  given the roads the agent really took, kept in st["_full"], so that it shows as a wrong count)
            full = st.setdefault("_full", {}).setdefault((b, a), [])
            seen = u in full[:h]
            full.append(u)
        else:
            seen = u in st["route"][b, a, :min(h, L)].tolist()
        if seen:
            st["revisits"][b, a] += 1
        if h < L:
            st["route"][b, a, h] = u
        st["roads"][b, a] = h + 1
        st["last_road"][b, a] = u
    return st


def arrays(st):
    """The state without the restatement's own bookkeeping."""
    return {k: v for k, v in st.items() if not k.startswith("_")}


def agent_stats(st, done, L, st_b=None, done_b=None):
    """tarl_path_agent_stats: ``done`` bool (K, A). Every sum adds k = 0, 1, ... in order from +0.0, as the kernel does."""
    K, A = st["roads"].shape
    i32 = {k: np.zeros(A, np.int32) for k in ("n_done", "n_zero_excess", "n_loop", "n_trunc", "n_seen", "n_loop_all",
                                              "roads_max")}
    f64 = {k: np.zeros(A, np.float64) for k in ("moves_sum", "moves_sumsq", "cost_sum", "cost_sumsq", "excess_sum",
                                                "excess_sumsq")}
    if st_b is not None:
        i32["n_both"] = np.zeros(A, np.int32)
        f64.update({k: np.zeros(A, np.float64) for k in ("dmoves_sum", "dmoves_sumsq", "dexcess_sum", "dexcess_sumsq")})
    for a in range(1, A):
        for k in range(K):
            r, rv = int(st["roads"][k, a]), int(st["revisits"][k, a])
            i32["n_seen"][a] += r > 0
            i32["n_loop_all"][a] += rv > 0
            i32["roads_max"][a] = max(int(i32["roads_max"][a]), r)
            if not done[k, a]:
                continue
            mv = np.float64(max(r - 1, 0))
            pc, ex = np.float64(st["path_cost"][k, a]), np.float64(st["excess"][k, a])
            i32["n_done"][a] += 1
            i32["n_zero_excess"][a] += bool(ex == 0.0 and st["off_tree"][k, a] == 0)
            i32["n_loop"][a] += rv > 0
            i32["n_trunc"][a] += r > L
            for key, v in (("moves", mv), ("cost", pc), ("excess", ex)):
                f64[key + "_sum"][a] = f64[key + "_sum"][a] + v
                f64[key + "_sumsq"][a] = f64[key + "_sumsq"][a] + v * v
            if st_b is not None and done_b[k, a]:
                dm = mv - np.float64(max(int(st_b["roads"][k, a]) - 1, 0))
                dx = ex - np.float64(st_b["excess"][k, a])
                i32["n_both"][a] += 1
                for key, v in (("dmoves", dm), ("dexcess", dx)):
                    f64[key + "_sum"][a] = f64[key + "_sum"][a] + v
                    f64[key + "_sumsq"][a] = f64[key + "_sumsq"][a] + v * v
    return {**i32, **f64}


def heads_of(x, Nmax):
    """The packed word 0 of every road of one oracle state ``x`` (N, F): head id << 8 | count (the oracle keeps the head in
    slot 0 and NUMBER_OF_AGENT at column 3 Nmax + 1)."""
    x = np.asarray(x)
    return (x[:, 0].astype(np.int64) << 8) | x[:, 3 * Nmax + 1].astype(np.int64)
