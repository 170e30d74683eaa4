"""Float64 restatement of the backward of the per-edge MLP head (csrc/edge_mlp.hip: x = [obs[src], obs[dst], edge_attr],
33 -> 64 -> 32 -> 1 with ReLU) written out by hand, and an emulation of how ``tarl_policy_edge_mlp_bwd`` partitions its work
(TEST INFRASTRUCTURE: plain torch on the CPU, no kernel involved). ``test_edge_mlp_host.py`` pins the backward to float64
autograd of ``oracle.nets.edge_mlp_logits`` and to the reference's golden; ``test_gpu_edge_mlp_bwd.py`` compares the kernels with
it. The module also holds the inputs of those GPU cases (``BWD_CASES``), so that the host test can check — without a GPU —
that every case would notice each unit of work the kernel could lose or misplace by 10x the tolerance the GPU test applies.

The kernel, restated. Stage 1 (``k_edge_mlp_bwd_edges``): the edges of sample m are cut into CH = ceil(E / 32) chunks of 32 lanes,
chunk g = m * CH + c; the launch has min(256, ceil(M * CH / 16)) workgroups of four waves, wave gw walks the contiguous range
[gw * per, min((gw + 1) * per, M * CH)) with per = ceil(M * CH / waves), carrying (m, c) by increments (``emr_walk``, the walk the
forwards use as well: one division for the range's first chunk, then c counts up inside a sample and m steps at its end).
Lane j of chunk (m, c) is edge e = 32 c + j, live when e < E, and stores its record — x, h1, h2 and the gradients d1, d2 of the
two pre-activations — k-major at the flat index l = m * E + e of a scratch of 225 * L floats, L = M * E. Stage 2 (``k_nt_dot``):
every gradient is a dot product over l, cut into ND_SPLIT = 64 ranges of span = ceil(L / 64); in a range 256 threads stride in
steps of 256 (pass p = (l - z * span) // 256). ``k_nt_reduce`` adds the 64 partial sums, in order, INTO the caller's gradient.
gb3 = sum(grad_logits) reads the caller's tensor, never the scratch: nothing stage 1 does reaches it.

Weights are ``edge_mlp.{0,2,4}.{weight,bias}``: w1 (64, 33), b1 (64,), w2 (32, 64), b2 (32,), w3 (32,) or (1, 32), b3 (1,)."""
from __future__ import annotations

import functools

import torch

D = torch.float64
IN, H1, H2 = 33, 64, 32
LANES = 32              # edges per chunk
EMR_WAVES = 4           # waves per workgroup
CHUNKS_PER_WAVE = 4     # the launcher asks for EMR_WAVES * 4 chunks per workgroup ...
MAX_BLOCKS = 256        # ... and caps the grid here
ND_SPLIT = 64
ND_T = 256
SCRATCH_ROWS = IN + 2 * H1 + 2 * H2      # 225 k-major rows of L floats
GRAD_NAMES = ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3")
GRAD_SHAPES = ((H1, IN), (H1,), (H2, H1), (H2,), (H2,), (1,))
TOL = 1e-4              # the GPU tolerance on a gradient: TOL * max(1, scale) per tensor (tests/test_gpu_edge_mlp.py)
FWD_TOL = 1e-5          # fp32 forward against float64: FWD_TOL * scale


# ---- the head and its backward, by hand ---------------------------------------------------------------------------------------
class Records:
    """What stage 1 stores per edge, row l = m * E + e: x (L, 33), h1 (L, 64), h2 (L, 32), d1 (L, 64), d2 (L, 32), g (L,)."""

    def __init__(self, x, h1, h2, d1, d2, g):
        self.x, self.h1, self.h2, self.d1, self.d2, self.g = x, h1, h2, d1, d2, g


def _w64(weights):
    w1, b1, w2, b2, w3, b3 = (w.detach().to(D) for w in weights)
    return w1, b1, w2, b2, w3.reshape(-1), b3.reshape(())


def edge_inputs64(obs, edge_index, edge_attr, m_idx, e_idx, obs_sample=None):
    """x of the edges (m_idx[k], e_idx[k]): cat(obs[m, src(e)], obs[m, dst(e)], edge_attr[e]) in float64. ``obs_sample``: the
    sample whose observation is read instead of m (a mutation of the host test)."""
    om = m_idx if obs_sample is None else obs_sample
    o = obs.to(D)
    ea = edge_attr.to(D).reshape(-1)
    return torch.cat([o[om, edge_index[0][e_idx]], o[om, edge_index[1][e_idx]], ea[e_idx].unsqueeze(1)], dim=1)


def records_of(x, g, weights):
    """The forward and the two masked gradients of the edges whose inputs are the rows of ``x``, seeded with ``g``."""
    w1, b1, w2, b2, w3, _ = _w64(weights)
    g = g.to(D)
    z1 = x @ w1.t() + b1
    h1 = z1.clamp(min=0)
    z2 = h1 @ w2.t() + b2
    h2 = z2.clamp(min=0)
    d2 = (z2 > 0).to(D) * g.unsqueeze(1) * w3.unsqueeze(0)
    d1 = (z1 > 0).to(D) * (d2 @ w2)
    return Records(x, h1, h2, d1, d2, g)


def records64(obs, edge_index, edge_attr, weights, grad_logits):
    M, E = obs.size(0), edge_index.size(1)
    m_idx = torch.arange(M).repeat_interleave(E)
    e_idx = torch.arange(E).repeat(M)
    return records_of(edge_inputs64(obs, edge_index, edge_attr, m_idx, e_idx), grad_logits.reshape(-1), weights)


def reduce64(rec):
    """Stage 2: the six gradients as sums over the rows of ``rec``."""
    return [rec.d1.t() @ rec.x, rec.d1.sum(0), rec.d2.t() @ rec.h1, rec.d2.sum(0), rec.h2.t() @ rec.g, rec.g.sum().reshape(1)]


def backward64(obs, edge_index, edge_attr, weights, grad_logits):
    """dW1, db1, dW2, db2, dw3, db3 of sum(logits * grad_logits), float64, shaped like ``GRAD_SHAPES``."""
    return reduce64(records64(obs, edge_index, edge_attr, weights, grad_logits))


def logits64(obs, edge_index, edge_attr, weights):
    M, E = obs.size(0), edge_index.size(1)
    rec = records64(obs, edge_index, edge_attr, weights, torch.zeros(M * E))
    _, _, _, _, w3, b3 = _w64(weights)
    return (rec.h2 @ w3 + b3).view(M, E)


def single_edge64(obs, edge_index, edge_attr, weights, m, e):
    """The gradient of the one logit (m, e): what a one-hot ``grad_logits`` must give."""
    x = edge_inputs64(obs, edge_index, edge_attr, torch.tensor([m]), torch.tensor([e]))
    return reduce64(records_of(x, torch.ones(1), weights))


# ---- how the kernel partitions the work ------------------------------------------------------------------------------------
class Walk:
    """The backward's ``emr_walk`` for (E, M): the grid, and per chunk g its wave and the (m, c) the walker holds when it
    computes it — obtained by WALKING (one division for the first chunk of a range, the carry into the next sample
    afterwards), not by dividing g."""

    def __init__(self, E, M):
        self.E, self.M = E, M
        self.CH = (E + LANES - 1) // LANES
        self.total = M * self.CH
        self.uncapped_blocks = -(-self.total // (EMR_WAVES * CHUNKS_PER_WAVE))
        self.blocks = min(MAX_BLOCKS, self.uncapped_blocks)
        self.waves = self.blocks * EMR_WAVES
        self.per = -(-self.total // self.waves)
        self.ranges = []                       # per wave (g0, g1), g0 >= g1: the wave leaves at once
        self.owner = [[] for _ in range(self.total)]
        self.m = [None] * self.total
        self.c = [None] * self.total
        for gw in range(self.waves):
            g0 = gw * self.per
            g1 = min(g0 + self.per, self.total)
            self.ranges.append((g0, g1))
            if g0 >= g1:
                continue
            mn = g0 // self.CH
            cn = g0 - mn * self.CH
            for g in range(g0, g1):
                m, c = mn, cn
                cn += 1
                if cn == self.CH:
                    cn, mn = 0, mn + 1
                self.owner[g].append(gw)
                self.m[g], self.c[g] = m, c

    @property
    def active(self):
        return [gw for gw, (g0, g1) in enumerate(self.ranges) if g0 < g1]

    @property
    def idle(self):
        return self.waves - len(self.active)

    def partial_last_wave(self):
        """The last active wave when its range is shorter than ``per``, else None."""
        gw = self.active[-1]
        g0, g1 = self.ranges[gw]
        return gw if g1 - g0 < self.per else None

    def lanes(self, g):
        """Live edges of chunk g."""
        return range(self.c[g] * LANES, min(self.c[g] * LANES + LANES, self.E))

    def flat(self, g):
        """The flat indices l = m * E + e of chunk g's live lanes."""
        return [self.m[g] * self.E + e for e in self.lanes(g)]

    def wave_flat(self, gw):
        g0, g1 = self.ranges[gw]
        return [l for g in range(g0, g1) for l in self.flat(g)]

    def mid_sample_starts(self):
        """Waves (beyond wave 0) whose range starts inside a sample (c != 0)."""
        return [gw for gw in self.active if gw > 0 and self.c[self.ranges[gw][0]] != 0]

    def crossings(self):
        """(wave, g): g is the first chunk of a new sample INSIDE the wave's range (the walker's carry: a new segment)."""
        out = []
        for gw in self.active:
            g0, g1 = self.ranges[gw]
            out += [(gw, g) for g in range(g0 + 1, g1) if self.c[g] == 0]
        return out


class Split:
    """``k_nt_dot`` for L: which (range z, stride pass p, thread) adds element l."""

    def __init__(self, L):
        self.L = L
        self.span = -(-L // ND_SPLIT)

    def bounds(self, z):
        l0 = z * self.span
        return l0, max(l0, min(l0 + self.span, self.L))

    def where(self, l):
        z = l // self.span
        off = l - z * self.span
        return z, off // ND_T, off % ND_T

    def nonempty(self):
        return [z for z in range(ND_SPLIT) if self.bounds(z)[0] < self.bounds(z)[1]]

    def pass_sizes(self, z):
        l0, l1 = self.bounds(z)
        n = l1 - l0
        return [min(ND_T, n - p * ND_T) for p in range(-(-n // ND_T))]

    def owners(self):
        """Per l the list of (z, p, thread) that the loops of the kernel visit it from (by running the loops)."""
        seen = [[] for _ in range(self.L)]
        for z in range(ND_SPLIT):
            l0, l1 = self.bounds(z)
            for t in range(ND_T):
                for p, l in enumerate(range(l0 + t, l1, ND_T)):
                    seen[l].append((z, p, t))
        return seen


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------------
# (E, M) -> what it reaches (tests/test_edge_mlp_host.py asserts every statement from the emulation above):
#   (1, 1)      L = 1: one chunk, three of the four waves leave at once, 63 empty split ranges
#   (32, 3)     exactly one full chunk per sample, no tail lanes, one chunk per wave
#   (33, 7)     a tail chunk with ONE live lane; 14 chunks on 4 waves: ranges cross samples, a partial last wave; span = 4
#   (185, 5)    6 chunks per sample against 4 per wave, two workgroups: ranges that start mid-sample, ranges that cross
#   (1, 4097)   4097 chunks: the grid is capped at 256 (257 uncapped), 5 chunks per wave, a partial last wave, 204 idle waves;
#               every range spans five samples; span = 65
#   (400, 100)  on MIXED (unsorted edge list): L = 40000, span = 625: three stride passes (256, 256, 113)
#   (185, 700)  4200 chunks: the cap AND several chunks per sample; L = 129500, span = 2024, eight passes; 117 MB of scratch
BWD_CASES = ((1, 1), (32, 3), (33, 7), (185, 5), (1, 4097), (400, 100), (185, 700))
GRAPH_OF = {(400, 100): "MIXED"}      # every other case: synth.torus_network(3, 4, heterogeneous=True), trailing edges dropped
# (E, M) -> seed offset, for a case whose first inputs fail a check of test_edge_mlp_host.py ON THE REFERENCE ALONE (no kernel
# involved): the inputs change, never the factor. Empty: every case holds with its first seed — also (1, 4097), where a chunk is a
# single edge and the margin is the thinnest (28x the tolerance on gb3 for the tail chunk of one sample, against the 10x asked).
RESEED = {}


def case_id(c):
    return f"E{c[0]}xM{c[1]}"


class Case:
    """Inputs of one case at unit scale — ``randn * 2`` observations, ``randn * 0.2`` weights, ``randn`` grad_logits, as the
    tests of tests/test_gpu_edge_mlp.py draw them — a function of the shape; ``G0``: what the gradient buffers hold before the
    call (every entry in +-[4, 8): far above 10x the tolerance of every case, so that a reduction which overwrote would
    show). The float64 reference is computed once and shared."""

    def __init__(self, E, M):
        import irregular_graphs
        from tarl_hip import synth
        self.E, self.M, self.L = E, M, E * M
        name = GRAPH_OF.get((E, M))
        net = irregular_graphs.graph(name) if name else synth.torus_network(3, 4, heterogeneous=True, seed=5)
        assert E <= net.edge_index.size(1)
        self.graph = name or "torus 3x4"
        self.N = net.num_roads
        self.edge_index = net.edge_index[:, :E].contiguous()
        self.edge_attr = net.edge_attr[:E].contiguous()
        gen = torch.Generator().manual_seed(7_000_000 + E * 10007 + M + RESEED.get((E, M), 0))
        self.weights = [torch.randn(s, generator=gen) * 0.2 for s in ((H1, IN), (H1,), (H2, H1), (H2,), (1, H2), (1,))]
        self.obs = torch.randn((M, self.N, 16), generator=gen) * 2.0
        self.grad_logits = torch.randn((M, E), generator=gen)
        self.G0 = [(4.0 + 4.0 * torch.rand(s, generator=gen)) * (torch.randint(0, 2, s, generator=gen).float() * 2 - 1)
                   for s in GRAD_SHAPES]
        self.walk = Walk(E, M)
        self.split = Split(self.L)

    def records(self, rows):
        """The true records of the flat indices ``rows``."""
        rows_t = torch.as_tensor(rows)
        x = edge_inputs64(self.obs, self.edge_index, self.edge_attr, rows_t // self.E, rows_t % self.E)
        return records_of(x, self.grad_logits.reshape(-1)[rows_t], self.weights)

    @functools.cached_property
    def grads64(self):
        return backward64(self.obs, self.edge_index, self.edge_attr, self.weights, self.grad_logits)

    @functools.cached_property
    def logits64(self):
        return logits64(self.obs, self.edge_index, self.edge_attr, self.weights)

    def bounds(self):
        """The GPU test's allowance per tensor."""
        return [TOL * max(1.0, float(g.abs().max())) for g in self.grads64]

    def single(self, m, e):
        return single_edge64(self.obs, self.edge_index, self.edge_attr, self.weights, m, e)

    # -- the one-hot probes of the GPU test, from the emulation ------------------------------------------------------------------
    def probes(self):
        """name -> (m, e), at most a dozen distinct positions: the corners; the last live lane of a tail chunk; the first
        chunk of a wave whose range starts mid-sample; the first chunk after a sample crossing inside a range; the split
        ranges' edges l in {span - 1, span, 63 span, L - 1}; the 256th and 257th element of a range where span > 256."""
        E, M, L, w, s = self.E, self.M, self.L, self.walk, self.split
        want = {"first edge, first sample": (0, 0), "last edge, first sample": (0, E - 1), "first edge, last sample": (M - 1, 0),
                "last edge, last sample": (M - 1, E - 1)}
        if E % LANES:
            want["last live lane of a tail chunk"] = (M // 2, E - 1)
        mids = w.mid_sample_starts()
        if mids:
            g = w.ranges[mids[len(mids) // 2]][0]
            want["first chunk of a range that starts mid-sample"] = (w.m[g], w.c[g] * LANES)
        cross = w.crossings()
        if cross:
            g = cross[(2 * len(cross)) // 3][1]
            want["first chunk after a sample crossing"] = (w.m[g], 0)
        for what, l in (("l = span - 1", s.span - 1), ("l = span", s.span), ("l = 63 span", (ND_SPLIT - 1) * s.span),
                        ("l = L - 1", L - 1)):
            if 0 <= l < L:
                want[what] = divmod(l, E)
        if s.span > ND_T:
            z = s.nonempty()[len(s.nonempty()) * 3 // 5]
            want["256th element of a range"] = divmod(s.bounds(z)[0] + ND_T - 1, E)
            want["257th element of a range"] = divmod(s.bounds(z)[0] + ND_T, E)
        out, seen = {}, set()
        for what, pos in want.items():
            if pos not in seen:
                seen.add(pos)
                out[what] = pos
        assert len(out) <= 12
        return out

    # -- the units of work the kernel could lose or misplace ---------------------------------------------------------------------
    def units(self):
        """name -> None (the case has no such unit) or (rows l, replacement): the records at ``rows`` are lost (replacement
        None: they add nothing to any sum) or replaced by the Records ``replacement``. "reduce overwrites" is not among them:
        it loses G0, see the host test."""
        E, M, L, w, s = self.E, self.M, self.L, self.walk, self.split
        act = w.active
        out = {}
        out["one wave's whole range"] = (w.wave_flat(act[len(act) // 2]), None)
        last = w.partial_last_wave()
        out["the partial last wave"] = None if last is None else (w.wave_flat(last), None)
        out["the tail chunk of one sample"] = ((w.flat((M // 2) * w.CH + w.CH - 1), None) if E % LANES else None)
        zs = s.nonempty()
        z = zs[len(zs) // 2]
        out["one split range"] = (list(range(*s.bounds(z))), None)
        out["after the first stride pass of one range"] = ((list(range(s.bounds(z)[0] + ND_T, s.bounds(z)[1])), None)
                                                           if s.span > ND_T else None)
        # the walker's carry lost: the chunks of a range past its first sample read the FIRST sample's observation (their
        # store index and grad_logits stay right)
        crossing = sorted({gw for gw, _ in w.crossings()})
        if crossing:
            gw = crossing[len(crossing) // 2]
            g0, g1 = w.ranges[gw]
            rows = [l for g in range(g0, g1) if w.m[g] != w.m[g0] for l in w.flat(g)]
            out["a range's chunks after a sample crossing read the previous sample's observation"] = (
                rows, self._replaced(rows, obs_sample=[w.m[g0]] * len(rows)))
        else:
            out["a range's chunks after a sample crossing read the previous sample's observation"] = None
        # the `live` guard lost: a dead lane of the tail chunk holds edge E - 1 and the store index of edge 0 (with edge 0's
        # grad_logits); in every sample edge 0's record becomes edge E - 1's. (E = 1: the dead lanes repeat edge 0 itself.)
        if E % LANES and E > 1:
            rows = [m * E for m in range(M)]
            out["a tail lane stored onto l = m E + 0"] = (rows, self._replaced(rows, edge=[E - 1] * M))
        else:
            out["a tail lane stored onto l = m E + 0"] = None
        return out

    def _replaced(self, rows, obs_sample=None, edge=None):
        rows_t = torch.tensor(rows)
        m_idx, e_idx = rows_t // self.E, rows_t % self.E
        x = edge_inputs64(self.obs, self.edge_index, self.edge_attr, m_idx, e_idx if edge is None else torch.tensor(edge),
                          None if obs_sample is None else torch.tensor(obs_sample))
        return records_of(x, self.grad_logits.reshape(-1)[rows_t], self.weights)

    def moved(self, unit):
        """Max abs change of each of the six float64 gradients when ``unit`` = (rows, replacement) happens."""
        rows, repl = unit
        true = reduce64(self.records(rows))
        mut = reduce64(repl) if repl is not None else [torch.zeros_like(t) for t in true]
        return [float((a - b).abs().max()) for a, b in zip(mut, true)]


@functools.lru_cache(maxsize=None)
def case(E, M):
    return Case(E, M)
