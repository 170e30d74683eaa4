"""Float64 restatement of the PPO update arithmetic and of GraphDistribution on arbitrary graphs (TEST INFRASTRUCTURE:
plain torch on the CPU, no kernel involved). ``test_update_host.py`` pins it to ``oracle/dist.py``, ``oracle/ppo.py`` and
the reference's golden vectors; ``test_gpu_update_fp64.py`` and ``test_gpu_draw_variants.py`` compare the HIP kernels with
it on the fp32-rounded inputs. It also holds the inputs of those GPU cases and the tolerance rule, so that the host test
can check — without a GPU — that every case would notice a lost row, element or wave.

Why not ``oracle.dist.GraphDist`` alone: it indexes per-group arrays by node id, so it needs compact source ids (every id
in 0..max has an out-edge). The plan accepts any graph, and the generic draw kernel exists for exactly those."""
from __future__ import annotations

import math

import numpy as np
import torch

LOG_EPS_P = 1e-8            # log(p + 1e-8), src/reinforcement_learning.py:27
ADV_STD_FLOOR = 1e-6        # oracle/ppo.py ADV_STD_FLOOR = csrc/ppo.hip TARL_ADV_STD_FLOOR
U24 = 2.0 ** -24            # fp32 unit round-off
RING_OFFSETS = (1, 7, 13, 29, 31, 37, 41, 43, 47, 53, 59, 61)   # out-edge k of node i leads to (i + o_k) % N


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def ring_graph(N, D, sorted=True, holes=False, seed=0):
    """Node i has ``1 + i % D`` out-edges to ``(i + o_k) % N``: max_out = D exactly. ``sorted=False`` permutes the edge
    columns (seeded); ``holes=True`` removes the out-edges of the nodes with ``i % 17 == 5`` (then groups != nodes)."""
    assert 1 <= D <= len(RING_OFFSETS)
    i = torch.arange(N)
    deg = 1 + i % D
    if holes:
        deg = torch.where(i % 17 == 5, torch.zeros_like(deg), deg)
    src = torch.repeat_interleave(i, deg)
    first = torch.cumsum(deg, 0) - deg
    k = torch.arange(src.numel()) - first[src]
    dst = (src + torch.tensor(RING_OFFSETS)[k]) % N
    ei = torch.stack([src, dst])
    if not sorted:
        ei = ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(seed))]
    return ei.contiguous()


def star_graph(hub_degree):
    """Node 0 -> 1..hub_degree, every other node (hub_degree + 3 in all) -> 0: one node of out-degree ``hub_degree``."""
    n = hub_degree + 3
    leaves = torch.arange(1, n)
    src = torch.cat([torch.zeros(hub_degree, dtype=torch.int64), leaves])
    dst = torch.cat([torch.arange(1, hub_degree + 1), torch.zeros(n - 1, dtype=torch.int64)])
    return torch.stack([src, dst]).contiguous(), n


class PlanOrder:
    """The static part: edges stably sorted by source (= tarl_plan's out_eid), group boundaries, ranks."""

    def __init__(self, edge_index, num_nodes):
        src = edge_index[0]
        self.N, self.E = int(num_nodes), src.numel()
        self.src = src
        self.order = torch.sort(src, stable=True)[1]           # sorted position -> edge id
        self.deg = torch.bincount(src, minlength=self.N)
        self.start = torch.cumsum(self.deg, 0) - self.deg      # node -> first sorted position
        self.pos = torch.empty_like(self.order)
        self.pos[self.order] = torch.arange(self.E)            # edge id -> sorted position
        self.rank = self.pos - self.start[src]                 # edge id -> rank within its node
        self.nodes = torch.nonzero(self.deg > 0).view(-1)      # group -> node
        self.G = self.nodes.numel()


# ---- GraphDistribution ---------------------------------------------------------------------------------------------------
class SegmentDist:
    """One categorical per source node over its out-edges: p = softmax(logits / T) per source, log(p + 1e-8). Works in
    the dtype of ``logits`` (float64 for the reference, float32 for the error yardstick), batched over leading dims,
    differentiable."""

    def __init__(self, logits, edge_index, temperature=1.0, num_nodes=None):
        src = edge_index[0]
        self.src, self.E = src, src.numel()
        self.N = int(num_nodes) if num_nodes is not None else int(src.max()) + 1
        self.has_out = torch.bincount(src, minlength=self.N) > 0
        z = logits / temperature
        idx = src.view((1,) * (z.dim() - 1) + (-1,)).expand_as(z)
        self._idx = idx
        mx = z.detach().new_full(z.shape[:-1] + (self.N,), float("-inf")).scatter_reduce(-1, idx, z.detach(), reduce="amax")
        ex = (z - mx.gather(-1, idx)).exp()
        sm = z.new_zeros(z.shape[:-1] + (self.N,)).scatter_add(-1, idx, ex)
        self.proba = ex / sm.gather(-1, idx)
        self.log_proba = torch.log(self.proba + LOG_EPS_P)

    def onehot(self, choice):
        """choice (..., N) edge ids (-1 = none) -> one-hot (..., E); an id that is no out-edge of its node is dropped."""
        c = choice.long()
        ok = c >= 0
        own = torch.zeros_like(ok)
        own[ok] = self.src[c[ok]] == torch.arange(self.N).expand_as(c)[ok]
        a = torch.zeros(choice.shape[:-1] + (self.E + 1,), dtype=torch.int64)
        a.scatter_(-1, torch.where(own, c, torch.full_like(c, self.E)), 1)
        return a[..., :self.E]

    def log_prob(self, choice=None, onehot=None):
        """sum of log(p + eps) over the chosen edges; -inf for a row in which a node with out-edges has not exactly one."""
        a = self.onehot(choice) if onehot is None else onehot
        cnt = torch.zeros(a.shape[:-1] + (self.N,), dtype=torch.int64).scatter_add(-1, self._idx.expand_as(a), a)
        possible = (cnt[..., self.has_out] == 1).all(-1)
        if choice is not None:      # an id outside the node's out-edges also makes the action impossible
            possible = possible & ((choice >= 0) == self.has_out).all(-1)
        lp = (a.to(self.log_proba.dtype) * self.log_proba).sum(-1)
        return torch.where(possible, lp, torch.full_like(lp, float("-inf")))

    def entropy(self):
        return -(self.proba * self.log_proba).sum(-1)

    def node_terms(self, choice):
        """Per-node contributions (..., N) to log_prob and entropy: what a kernel that skips a node would lose."""
        a = self.onehot(choice).to(self.log_proba.dtype)
        z = self.proba.new_zeros(self.proba.shape[:-1] + (self.N,))
        return (z.scatter_add(-1, self._idx, a * self.log_proba), z.scatter_add(-1, self._idx, -self.proba * self.log_proba))


def segment_dist(logits, edge_index, temperature=1.0, num_nodes=None):
    return SegmentDist(logits, edge_index, temperature, num_nodes)


def rebased_cumsum(proba32, po: PlanOrder):
    """``src/reinforcement_learning.py:38-42`` per node: the global cumulative sum over the sorted edges, accumulated in
    double and rounded to fp32 at every edge (torch's CPU cumsum), minus the fp32 value at the previous node's last edge.
    Returns the fp32 thresholds in sorted order."""
    ps = proba32.float()[po.order].tolist()
    deg = po.deg.tolist()
    run = 0.0                                  # a Python float is a double
    cum = np.empty(po.E, dtype=np.float32)
    base32 = np.float32(0.0)
    k = 0
    for i in po.nodes.tolist():
        for _ in range(deg[i]):
            run += ps[k]
            cum[k] = np.float32(run) - base32  # fp32 - fp32
            k += 1
        base32 = np.float32(run)
    return torch.from_numpy(cum)


def sample_choice(proba32, po: PlanOrder, u):
    """``:62-80`` per node: the first sorted edge with ``u[group] < cum`` (strict); -1 where there is none. ``u`` (G,).
    Returns (choice (N,) int64 edge ids, rank (N,) int64, 0 where nothing was drawn)."""
    cum = rebased_cumsum(proba32, po).tolist()
    choice = torch.full((po.N,), -1, dtype=torch.int64)
    rank = torch.zeros(po.N, dtype=torch.int64)
    ul = u.float().tolist()                    # fp32 values, compared as doubles: exact
    start, deg, order = po.start.tolist(), po.deg.tolist(), po.order.tolist()
    for g, i in enumerate(po.nodes.tolist()):
        k0 = start[i]
        for q in range(deg[i]):
            if ul[g] < cum[k0 + q]:
                choice[i], rank[i] = order[k0 + q], q
                break
    return choice, rank


def choice_from_onehot(onehot, po: PlanOrder):
    """One-hot (E,) (at most one edge per node) -> (choice (N,), rank (N,)) as :func:`sample_choice`."""
    choice = torch.full((po.N,), -1, dtype=torch.int64)
    rank = torch.zeros(po.N, dtype=torch.int64)
    e = torch.nonzero(onehot).view(-1)
    assert torch.unique(po.src[e]).numel() == e.numel()
    choice[po.src[e]] = e
    rank[po.src[e]] = po.rank[e]
    return choice, rank


# ---- PPO arithmetic ------------------------------------------------------------------------------------------------------
def clip_thresholds32(clip_epsilon, device="cpu"):
    """The kernel's thresholds: log1p(-eps), log1p(eps) evaluated in fp32 on the fp32 epsilon (k_ppo_loss), as doubles."""
    t = torch.log1p(torch.tensor([-clip_epsilon, clip_epsilon], dtype=torch.float32, device=device)).cpu().double()
    return float(t[0]), float(t[1])


def ppo_terms64(lp_new, lp_old, adv, value, target, entropy, clip_epsilon=0.2, entropy_coef=0.01, critic_coef=1.0, lo=None,
                hi=None):
    """Per-row terms of the six outputs of tarl_ppo_loss (before the mean): dict of (M,) tensors. ``lo`` / ``hi``: the clip
    thresholds on the log-ratio (default: log1p(-+eps) in double, as oracle/ppo.py)."""
    lo = math.log1p(-clip_epsilon) if lo is None else lo
    hi = math.log1p(clip_epsilon) if hi is None else hi
    lw = lp_new - lp_old
    r = lw.exp()
    gain = torch.min(r * adv, lw.clamp(lo, hi).exp() * adv)
    d = value - target
    ad = d.abs()
    sl1 = torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    return {"obj": -gain, "critic": critic_coef * sl1, "entropy": -entropy_coef * entropy,
            "clip": ((lw < lo) | (lw > hi)).to(lw.dtype), "kl": -lw, "w": r, "w2": r * r}


def ppo_loss64(lp_new, lp_old, adv, value, target, entropy, clip_epsilon=0.2, entropy_coef=0.01, critic_coef=1.0,
               grad_scale=1.0, lo=None, hi=None):
    """-> (out6, g_lp, g_ent, g_val, mean_abs_term6): loss_objective, loss_critic, loss_entropy, clip fraction, mean(-lw),
    ESS = (sum r)^2 / sum r^2; the gradients of grad_scale * (sum of the three losses) w.r.t. lp_new, entropy and value
    (autograd); and mean|term| of each output (for ESS: the value itself, see :func:`scalar_bound`)."""
    lp_new, value, entropy = (t.detach().clone().requires_grad_(True) for t in (lp_new, value, entropy))
    t = ppo_terms64(lp_new, lp_old, adv, value, target, entropy, clip_epsilon, entropy_coef, critic_coef, lo, hi)
    obj, cr, en = t["obj"].mean(), t["critic"].mean(), t["entropy"].mean()
    g_lp, g_ent, g_val = torch.autograd.grad(grad_scale * (obj + cr + en), (lp_new, entropy, value))
    ess = t["w"].sum() ** 2 / (t["w2"]).sum()
    out = torch.stack([obj, cr, en, t["clip"].mean(), t["kl"].mean(), ess]).detach()
    mean_abs = torch.stack([t[k].detach().abs().mean() for k in ("obj", "critic", "entropy", "clip", "kl")] + [ess.detach()])
    return out, g_lp, g_ent, g_val, mean_abs


def gae64(reward, value, next_value, done=None, terminated=None, gamma=0.99, lmbda=0.95):
    """Time-major (T, B): delta = r + gamma V' (1 - terminated) - V; A_t = delta_t + gamma lambda (1 - done_t) A_{t+1};
    target = A + V. Un-normalised. -> (advantage, value_target)."""
    nt = 1.0 if terminated is None else 1.0 - terminated.to(reward.dtype)
    nd = torch.ones_like(reward) if done is None else 1.0 - done.to(reward.dtype)
    delta = reward + gamma * next_value * nt - value
    adv = torch.zeros_like(delta)
    run = torch.zeros_like(delta[0])
    for t in range(reward.size(0) - 1, -1, -1):
        run = delta[t] + gamma * lmbda * nd[t] * run
        adv[t] = run
    return adv, adv + value


def adv_stats64(a):
    """{sum, sumsq, n} of the fp32 values, exactly rounded (math.fsum over doubles; a square of an fp32 is exact there)."""
    x = a.double().view(-1).tolist()
    return {"sum": math.fsum(x), "sumsq": math.fsum(v * v for v in x), "n": float(len(x))}


def normalize64(a, stats=None):
    """(a - mean) / max(std, floor) with the unbiased std, from ``stats`` (default: the tensor's own)."""
    s = adv_stats64(a) if stats is None else stats
    mean = s["sum"] / s["n"]
    var = max((s["sumsq"] - s["n"] * mean * mean) / (s["n"] - 1.0), 0.0) if s["n"] > 1 else 0.0
    return (a - mean) / max(math.sqrt(var), ADV_STD_FLOOR)


def adam64(param, grad, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """torch.optim.Adam's single-tensor update on ``grad * grad_scale``; ``step`` 1-based. -> (param, m, v), new tensors."""
    g = grad * grad_scale
    m = m + (1 - beta1) * (g - m)
    v = v * beta2 + (1 - beta2) * g * g
    denom = v.sqrt() / math.sqrt(1 - beta2 ** step) + eps
    return param - (lr / (1 - beta1 ** step)) * (m / denom), m, v


# ---- the tolerance rule --------------------------------------------------------------------------------------------------
def tensor_bound(e32, ref, relative_scale=False):
    """max(8 e32, 2^-22 scale): e32 = max|fp32 oracle - float64 reference| on the same inputs (the margin of 8: another,
    but fixed, order of the same operations on the device); scale = max(1, max|ref|). ``relative_scale``: scale = max|ref|
    without the floor of 1 — for the O(1/M) gradient seeds, where 2^-22 absolute would be a tenth of a seed at M = 4 133
    (never wider than the rule, since max|ref| <= max(1, max|ref|))."""
    mx = float(ref.detach().abs().max()) if ref.numel() else 0.0
    scale = mx if relative_scale else max(1.0, mx)
    return max(8.0 * float(e32), 2.0 ** -22 * scale)


def scalar_bound(M, mean_abs_term, ess=False):
    """The six reduced scalars: depth bound of k_ppo_loss's documented reduction (ceil(M / 256) sequential additions per
    thread, a six-level shuffle tree, four waves, the products with 1/M and the coefficient; 16 covers those and the ulp
    of expf): (ceil(M / 256) + 16) 2^-24 mean|term|. ESS = S1^2 / S2 with S1, S2 sums of positive terms, each within that
    RELATIVE bound: to first order 3 times it, relative to ESS."""
    b = (math.ceil(M / 256) + 16) * U24 * float(mean_abs_term)
    return 3.0 * b if ess else b


def max_err(got, ref):
    return float((got.double() - ref.double()).abs().max()) if ref.numel() else 0.0


# ---- inputs of the GPU cases (shared with the host sensitivity checks) -----------------------------------------------
PPO_SIZES = (1, 63, 65, 255, 256, 257, 1000, 4133)
PPO_COEFS = ({}, dict(clip_epsilon=0.1, entropy_coef=0.03, critic_coef=0.5, grad_scale=0.25))
GAE_B, GAE_T = (1, 255, 256, 257, 600), (1, 2, 50)
GAE_MASKS = ("none", "done", "both")
GAE_GL = ((0.99, 0.95), (0.9, 0.8), (1.0, 1.0), (0.99, 0.0))
STATS_N = (2, 255, 257, 65536, 65537, 200003)
ADAM_N = (1, 255, 257, 100003)
DIST_GRAPHS = {"ring300x12_holes": dict(N=300, D=12, sorted=False, holes=True, seed=3),
               "ring2500x4": dict(N=2500, D=4, sorted=True, holes=False, seed=0)}
DIST_T = (1.0, 0.7)


def ppo_inputs(M, seed=0):
    """fp32: lp_old ~ -U(0, 3000) (the magnitude at 2 500 nodes: the log-ratio carries fp32 rounding), log-ratios
    randn * 0.3 (both sides of the clip), |value - target| on both sides of 1, entropies of that graph size."""
    g = torch.Generator().manual_seed(1000 + 7 * M + seed)
    lp_old = -torch.rand(M, generator=g) * 3000
    lp_new = lp_old + torch.randn(M, generator=g) * 0.3
    adv = torch.randn(M, generator=g)
    value = torch.randn(M, generator=g) * 2
    target = torch.randn(M, generator=g) * 2
    ent = torch.rand(M, generator=g) * 2000 + 500
    return lp_new, lp_old, adv, value, target, ent


def gae_inputs(B, T, masks, seed=0):
    g = torch.Generator().manual_seed(2000 + 13 * B + T + seed)
    r = torch.randn((T, B), generator=g) * 5 - 20
    v = torch.randn((T + 1, B), generator=g) * 3
    done = (torch.rand((T, B), generator=g) < 0.1).to(torch.uint8)
    term = (done.bool() & (torch.rand((T, B), generator=g) < 0.5)).to(torch.uint8)
    return (r, v[:-1].contiguous(), v[1:].contiguous(), done if masks != "none" else None, term if masks == "both" else None)


def stats_inputs(n, kind="wide"):
    """wide: randn * 3 + 5 (|mean| <= 10 std: also normalised); narrow: mean 1 000, std 0.01; const: all 3.7."""
    g = torch.Generator().manual_seed(3000 + n)
    if kind == "wide":
        return torch.randn(n, generator=g) * 3 + 5
    if kind == "narrow":
        return torch.randn(n, generator=g) * 0.01 + 1000
    return torch.full((n,), 3.7)


ADAM_HYPER = dict(lr=3e-4, beta1=0.8, beta2=0.99, eps=1e-6)


def adam_inputs(n):
    """(param, grad, m, v) fp32: a state to resume from (m, v of a run with gradients of this size)."""
    g = torch.Generator().manual_seed(4000 + n)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 2
    m = torch.randn(n, generator=g) * 0.3
    v = torch.rand(n, generator=g) * 0.5 + 0.05
    return p, grad, m, v


def dist_inputs(name, B=3):
    """(edge_index, N, logits (B, E) = randn * 6: some p < 1e-8, so the epsilon matters; choice (B, N) a valid action;
    w_lp, w_ent (B,) gradient weights)."""
    spec = DIST_GRAPHS[name]
    ei = ring_graph(spec["N"], spec["D"], spec["sorted"], spec["holes"], spec["seed"])
    N, E = spec["N"], ei.size(1)
    g = torch.Generator().manual_seed(5000 + N)
    logits = torch.randn((B, E), generator=g) * 6
    po = PlanOrder(ei, N)
    q = (torch.rand((B, N), generator=g) * po.deg).long().clamp(max=(po.deg - 1).clamp(min=0))
    choice = po.order[(po.start + q).clamp(max=E - 1)]
    choice = torch.where(po.deg > 0, choice, torch.full_like(choice, -1))
    w_lp = torch.randn(B, generator=g)
    w_ent = torch.randn(B, generator=g)
    return ei, N, logits, choice, w_lp, w_ent


def dist_reference(ei, N, logits, choice, w_lp, w_ent, T):
    """References (float64 on the fp32 logits) and tolerances of the distribution forward / backward case — used by
    test_gpu_update_fp64.py and the host sensitivity check. e32: the same restatement in fp32 (oracle.dist.GraphDist cannot take the graph with holes)."""
    out = {}

    def run(dtype):
        l = logits.to(dtype).clone().requires_grad_(True)
        d = segment_dist(l, ei, T, N)
        lp, ent = d.log_prob(choice), d.entropy()
        bad = choice.clone()
        bad[1, int(torch.nonzero(d.has_out)[3])] = -1       # row 1: an impossible action
        lp_bad = d.log_prob(bad)
        fin = torch.isfinite(lp_bad)
        g_lp, = torch.autograd.grad((lp * w_lp.to(dtype)).sum(), l, retain_graph=True)
        g_ent, = torch.autograd.grad((ent * w_ent.to(dtype)).sum(), l, retain_graph=True)
        g_both, = torch.autograd.grad((lp_bad[fin] * w_lp.to(dtype)[fin]).sum() + (ent * w_ent.to(dtype)).sum(), l)
        return dict(proba=d.proba.detach(), lp=lp.detach(), ent=ent.detach(), grad_lp=g_lp, grad_ent=g_ent, grad_both=g_both,
                    bad=bad, lp_bad=lp_bad.detach())

    r64, r32 = run(torch.float64), run(torch.float32)
    for k in ("proba", "lp", "ent", "grad_lp", "grad_ent", "grad_both"):
        out["ref_" + k] = r64[k]
        out["e32_" + k] = max_err(r32[k], r64[k])
        out[k] = tensor_bound(out["e32_" + k], r64[k])
    out["bad"], out["lp_bad"] = r64["bad"], r64["lp_bad"]
    return out


# the action draw's launch shapes: name -> (N, D, sorted, holes, kernel reached)
DRAW_CASES = {
    "r1x4s": (40, 4, True, False, "reg<1,4,sorted>"),
    "r1x4u": (1024, 4, False, False, "reg<1,4,unsorted>"),
    "r2x4u": (1030, 4, False, False, "reg<2,4,unsorted>"),
    "r3x4u": (2050, 4, False, False, "reg<3,4,unsorted>"),
    "r2x4s": (2047, 4, True, False, "reg<2,4,sorted>"),      # (these two also run in test_gpu_dist_parity.py: here so that
    "r3x4s": (2049, 4, True, False, "reg<3,4,sorted>"),      # this table alone executes all twelve instantiations)
    "r4x4s": (4096, 4, True, False, "reg<4,4,sorted>"),
    "r4x4u": (3073, 4, False, False, "reg<4,4,unsorted>"),
    "r1x8s": (1000, 8, True, False, "reg<1,8,sorted>"),
    "r1x8u": (1024, 8, False, False, "reg<1,8,unsorted>"),
    "r2x8s": (2048, 8, True, False, "reg<2,8,sorted>"),
    "r2x8u": (1025, 8, False, False, "reg<2,8,unsorted>"),
    "g4097": (4097, 4, True, False, "generic"),
    "g2049": (2049, 8, True, False, "generic"),
    "g9": (1500, 9, False, False, "generic"),
    "gholes": (1500, 4, False, True, "generic"),
}
DRAW_B, DRAW_T = 5, 0.8


def draw_inputs(name):
    """(edge_index, N, logits (5, E) = randn * 3, host uniforms (5, G), previous rank bytes (N, 5) in 0..2)."""
    N, D, srt, holes, _ = DRAW_CASES[name]
    ei = ring_graph(N, D, srt, holes, seed=N)
    g = torch.Generator().manual_seed(6000 + N + D)
    logits = torch.randn((DRAW_B, ei.size(1)), generator=g) * 3
    G = int((torch.bincount(ei[0], minlength=N) > 0).sum())
    u = torch.rand((DRAW_B, G), generator=g)
    prev = torch.randint(0, 3, (N, DRAW_B), generator=g).to(torch.uint8)
    return ei, N, logits, u, prev


def draw_dispatch(N, G, max_out, src_sorted):
    """The launcher's choice (tarl_graphdist_rollout_at), restated from the plan's numbers."""
    J = -(-N // 1024)
    D = 4 if max_out <= 4 else 8
    if G == N and max_out <= 8 and J * D <= 16:
        return f"reg<{J},{D},{'sorted' if src_sorted else 'unsorted'}>"
    return "generic"
