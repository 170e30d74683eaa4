"""CPU restatement of src/algorithms/equilibrium.py and csrc/equilibrium.hip in float64 numpy: the BPR model of run_msa,
scipy's Dijkstra (left-to-right fp64 sums, explicit zero-weight edges kept), the all-or-nothing load, the conjugate /
plain Frank-Wolfe / MSA step with a bisection line search, and the metrics. Written from the definitions, not from the
kernels: sums are numpy's pairwise sums, so it differs from the device by the order of fp64 additions only."""
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

U = 2.0 ** -53
C_OF = {"ue": 0.15, "so": 0.75}


def bpr(ff, cap, road, x, c):
    r = x / np.maximum(cap, 1e-8)
    r2 = r * r
    return np.where(road, ff * (1.0 + c * (r2 * r2)), 0.0)


def dbpr(ff, cap, road, x, c):
    cp = np.maximum(cap, 1e-8)
    r = x / cp
    return np.where(road, ff * (4.0 * c) * ((r * r) * r) / cp, 0.0)


def bisect(g):
    """The root of a monotone g on [0, 1], given g(1) > 0: halve until the midpoint meets an end, at most 60 times."""
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if g(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def step(f, y, s_prev, ff, cap, road, objective, rule, iteration, msa_step=0.0, lam=None):
    """One tarl_bpr_step. ``lam``: take this step instead of searching (to compare the rest given the kernel's own)."""
    c = C_OF[objective]
    cost = lambda x: bpr(ff, cap, road, x, c)                       # noqa: E731
    first = iteration <= 1
    alpha, Nn, Dn = 0.0, 0.0, 0.0
    if rule == "cfw" and not first:
        dh = (s_prev - f) * dbpr(ff, cap, road, f, c)
        Nn, Dn = float(np.sum(dh * (y - f))), float(np.sum(dh * (y - s_prev)))
        if Dn != 0.0:
            alpha = Nn / Dn
            alpha = 0.0 if not alpha > 0.0 else min(alpha, 0.99)
    s = alpha * s_prev + (1.0 - alpha) * y if alpha != 0.0 else y.copy()
    d = s - f
    g = lambda l: float(np.sum(d * cost(f + l * d)))               # noqa: E731
    g0, g1 = g(0.0), g(1.0)
    if first:
        lam_ref = 1.0
    elif rule == "msa":
        lam_ref = msa_step
    elif g1 <= 0.0:
        lam_ref = 1.0
    else:
        lam_ref = bisect(g)
    use = lam_ref if lam is None else lam
    fn = f + use * d
    # the bound on |lambda - lambda_ref| that follows from the rounding of g: |delta g| <= 4 (N + 8) u sum |d cost|,
    # divided by the slope g' = sum d^2 H at the root
    x = f + lam_ref * d
    num = float(np.sum(np.abs(d * cost(x))))
    den = float(np.sum(d * d * dbpr(ff, cap, road, x, c)))
    bound = (4.0 * (f.size + 8) * U * num / den if den > 0 else math.inf) + 2.0 ** -50
    return dict(alpha=alpha, Nn=Nn, Dn=Dn, s=s, lam=lam_ref, lam_bound=bound, f=fn, cost=cost(fn), g0=g0, g1=g1,
                tstt=float(np.sum(fn * bpr(ff, cap, road, fn, 0.15))), fc=float(np.sum(fn * cost(fn))))


class Model:
    def __init__(self, ff, cap, road, edge_index, od_o, od_d, od_vol):
        self.ff, self.cap, self.road = (np.asarray(a) for a in (ff, cap, road))
        self.ff, self.cap, self.road = self.ff.astype(np.float64), self.cap.astype(np.float64), self.road.astype(bool)
        self.N = self.ff.size
        self.src, self.dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
        self.od_o, self.od_d = np.asarray(od_o), np.asarray(od_d)
        self.od_vol = np.asarray(od_vol, dtype=np.float64)
        self.origins, self.slot = np.unique(self.od_o, return_inverse=True)

    @classmethod
    def from_graph(cls, graph, agents):
        x = graph.x.detach().cpu()
        Nmax = (x.size(1) - 7) // 3
        feats = agents.agent_features.detach().cpu()[1:]
        N = x.size(0)
        flat = feats[:, 0].long() * N + feats[:, 1].long()
        pairs, counts = np.unique(flat.numpy(), return_counts=True)
        return cls(x[:, 3 * Nmax + 2].double().numpy(), x[:, 3 * Nmax + 4].double().numpy(),
                   (x[:, 3 * Nmax + 6] >= 0).numpy(), graph.edge_index.detach().cpu().numpy(), pairs // N, pairs % N,
                   counts.astype(np.float64))

    def cost(self, f, objective):
        return bpr(self.ff, self.cap, self.road, f, C_OF[objective])

    def tstt(self, f):
        return float(np.sum(f * self.cost(f, "ue")))

    def beckmann(self, f):
        """sum_v int_0^f t_v = ff f (1 + 0.03 r^4)."""
        r = f / np.maximum(self.cap, 1e-8)
        r2 = r * r
        return float(np.sum(np.where(self.road, self.ff * f * (1.0 + 0.03 * (r2 * r2)), 0.0)))

    def trees(self, cost, want_pred=False):
        """dist [origins][N] (and predecessors) at node costs ``cost``: an edge costs what its head node costs."""
        m = sp.csr_matrix((cost[self.dst], (self.src, self.dst)), shape=(self.N, self.N))
        return dijkstra(m, directed=True, indices=self.origins, return_predecessors=want_pred)

    def sptt(self, cost):
        """(SPTT, unrouted volume, pair distances, per-origin partial sums in pair order)."""
        dist = self.trees(cost)
        pd = dist[self.slot, self.od_d]
        part = np.zeros(self.origins.size)
        unr = np.zeros(self.origins.size)
        for p in range(pd.size):                     # pair order, one fp64 addition at a time
            if self.od_vol[p] > 0.0:
                if np.isfinite(pd[p]):
                    part[self.slot[p]] += self.od_vol[p] * pd[p]
                else:
                    unr[self.slot[p]] += self.od_vol[p]
        return float(part.sum()), float(unr.sum()), pd, part, unr

    def assign(self, cost):
        """All-or-nothing load: (y, SPTT, unrouted volume)."""
        dist, pred = self.trees(cost, want_pred=True)
        y = np.zeros(self.N)
        sptt = unrouted = 0.0
        for p in range(self.od_d.size):
            j, d, vol = self.slot[p], int(self.od_d[p]), self.od_vol[p]
            if not np.isfinite(dist[j, d]):
                unrouted += vol
                continue
            sptt += vol * dist[j, d]
            o, v = int(self.origins[j]), d
            while v != o:                            # path[1:]: d included, o not
                if self.road[v]:
                    y[v] += vol
                v = int(pred[j, v])
        return y, sptt, unrouted

    def evaluate(self, f, objective):
        c = self.cost(f, objective)
        sptt, unrouted, _, _, _ = self.sptt(c)
        fc = float(np.sum(f * c))
        tstt = self.tstt(f)
        return dict(tstt=tstt, fc=fc, sptt=sptt, gap=(fc - sptt) / fc, unrouted=unrouted,
                    lower_bound=tstt - (fc - sptt))

    def solve(self, objective, solver, iterations):
        """-> (trace [(gap of f_k, lambda_k, alpha_k)], [f_k]) for k = 1 .. iterations."""
        f, s_prev = np.zeros(self.N), np.zeros(self.N)
        trace, flows, fc_prev = [], [], None
        for k in range(1, iterations + 1):
            y, sptt, _ = self.assign(self.cost(f, objective))
            if k > 1:
                trace[-1][0] = (fc_prev - sptt) / fc_prev
            r = step(f, y, s_prev, self.ff, self.cap, self.road, objective, solver, k, msa_step=1.0 / k)
            f, s_prev, fc_prev = r["f"], r["s"], r["fc"]
            trace.append([math.nan, r["lam"], r["alpha"]])
            flows.append(f.copy())
        _, sptt, _ = self.assign(self.cost(f, objective))
        trace[-1][0] = (fc_prev - sptt) / fc_prev
        return [tuple(t) for t in trace], flows

    def iterations_to_gap(self, objective, solver, gap, max_iter):
        f, s_prev, fc_prev = np.zeros(self.N), np.zeros(self.N), None
        for k in range(1, max_iter + 2):
            y, sptt, _ = self.assign(self.cost(f, objective))
            if k > 1 and (fc_prev - sptt) / fc_prev <= gap:
                return k - 1
            r = step(f, y, s_prev, self.ff, self.cap, self.road, objective, solver, k, msa_step=1.0 / k)
            f, s_prev, fc_prev = r["f"], r["s"], r["fc"]
        return None


def four_road_model(trips_od=15.0, trips_bd=4.0):
    """Origin road O (0), parallel roads A (1: ff 15, capacity 1e6) and B (2: ff 10, capacity 10), destination road D
    (3: ff 5, capacity 20); edges O->A, O->B, A->D, B->D; demand O->D and B->D (the latter loads D only)."""
    ff = np.array([1.0, 15.0, 10.0, 5.0])
    cap = np.array([100.0, 1e6, 10.0, 20.0])
    ei = np.array([[0, 0, 1, 2], [1, 2, 3, 3]])
    return Model(ff, cap, np.ones(4, bool), ei, np.array([0, 2]), np.array([3, 3]), np.array([trips_od, trips_bd]))


def four_road_closed_form(trips_od=15.0, trips_bd=4.0):
    """The A / B split at user equilibrium (t_A = t_B) and at system optimum (m_A = m_B) as one-dimensional roots, or the
    corner with nothing on A when B is cheaper even with all the trips: -> dict(ue=(a, b), so=(a, b), tstt_ue, tstt_so)."""
    from scipy.optimize import brentq
    m = four_road_model(trips_od, trips_bd)
    out = {}
    for name, c in C_OF.items():
        def diff(a):
            x = np.array([0.0, a, trips_od - a, trips_od + trips_bd])
            cc = bpr(m.ff, m.cap, m.road, x, c)
            return cc[1] - cc[2]
        a = 0.0 if diff(0.0) >= 0.0 else brentq(diff, 0.0, trips_od, xtol=1e-15, rtol=8.9e-16)
        out[name] = (a, trips_od - a)
        out["tstt_" + name] = m.tstt(np.array([0.0, a, trips_od - a, trips_od + trips_bd]))
    return out
