"""Cases shared by the tests of the two graph-transformer networks (test_gpu_gt_head.py, test_gpu_gt_value.py and their CPU
proof test_gt_attention_host.py): the closeness check, the reference's initialisation, scaled random and sharp weights, the
graphs, observations as the simulator builds them, a case's inputs and its two restatement references, the tolerances, the
attention census and its conditions, the kernels' summation bound and a parameter's span in the trainer's flat gradient."""
import types

import torch

# "sharp" weights: the scaled random ones with WQ and WK of both layers multiplied by this. The random weights leave the
# attention scores below 0.07 (softmax = 1 / in-degree to three digits), the reference's initialisation on raw observations
# drives them to 1e8 (one-hot); at 32 they decide the output while fp32 still resolves them.
SHARP_SCALE = 32.0
SHARP_KEYS = tuple(f"gt_layers.{L}.{w}.weight" for L in (0, 1) for w in ("WQ", "WK"))
# sharp cases, output: |kernel - float64| <= SHARP_FACTOR * max |fp32 restatement - float64| + SHARP_FLOOR_ULPS fp32 ulps of
# the output's scale (16: the gradient check's factor between two valid fp32 forms of one function; 8 ulps: the critic tests')
SHARP_FACTOR = 16.0
SHARP_FLOOR_ULPS = 8.0
# the sharp cases of both GPU tests (kind, M), and every case this adds to them
SHARP_CASES = [("torus16", 7), ("config4", 7), ("matsim", 7), ("MIXED", 1), ("MIXED", 3), ("HUB126", 3)]
ATTENTION_CASES = ([(kind, M, "sharp") for kind, M in SHARP_CASES[:5]] + [("MIXED", 3, "random"), ("HUB126", 3, "sharp"),
                                                                          ("HUB126", 1, "reference")])
# the census conditions of a sharp case, per attention layer, over the segments of in-degree >= 2
CENSUS_MAX_ONE_HOT, CENSUS_MAX_FLAT, CENSUS_MIN_MEDIAN_SPREAD, CENSUS_MAX_SCORE, CENSUS_OVERFLOW_SCORE = 0.15, 0.30, 0.2, 1e3, 88.0


def _close(a, b, what, tol=1e-4):
    scale = max(float(b.abs().max()), 1.0)
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * scale, f"{what}: {err} > {tol} * {scale}"


def _random_state(seed, scale=0.4, critic=False):
    """Scaled random weights: random normal matrices of std 1 / fan-in (node_emb 1e-4 / fan-in: the observations carry raw
    clock times of ~2e4), random biases, BatchNorm gamma / beta and statistics; of the policy head's keys, or the critic's."""
    sd = _reference_state(seed)
    from tarl_hip import ops
    params, buffers = ((ops.GT_VALUE_PARAM_KEYS, ops.GT_VALUE_BUFFER_KEYS) if critic else
                       (ops.GT_PARAM_KEYS, ops.GT_BUFFER_KEYS))
    gen = torch.Generator().manual_seed(seed + 1)
    for k in params:
        if k.endswith("weight") and "norm" not in k:
            sd[k] = torch.randn(sd[k].shape, generator=gen) / sd[k].size(-1) * (1e-4 if k == "node_emb.weight" else 1.0)
        if k.endswith("bias") or "norm" in k:
            sd[k] = sd[k] + scale * torch.randn(sd[k].shape, generator=gen)
    for k in buffers:
        sd[k] = (torch.rand(16, generator=gen) + 0.5) if k.endswith("var") else 0.3 * torch.randn(16, generator=gen)
    return sd


def _sharp_state(seed, critic=False):
    """:func:`_random_state` with WQ and WK of both layers multiplied by SHARP_SCALE."""
    sd = _random_state(seed, critic=critic)
    for k in SHARP_KEYS:
        sd[k] = sd[k] * SHARP_SCALE
    return sd


def _state(weights, seed, critic=False):
    """The state dict of a weight kind: "reference", "random" or "sharp"."""
    if weights == "reference":
        return _reference_state(seed)
    return {"random": _random_state, "sharp": _sharp_state}[weights](seed, critic=critic)


def _reference_state(seed):
    """The reference's initialisation (GraphTransformerNet's construction order and reset_parameters; BatchNorm statistics
    at their defaults), seeded."""
    from src.transformer import GraphTransformerNet
    torch.manual_seed(seed)
    net = GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4, dropout=0.1)
    return {k: v.clone() for k, v in net.state_dict().items()}


def _graph(kind, tmp_path):
    """(edge_index, edge_attr (E, 1), x, Nmax, num_roads, road-graph edge_index) of a torus, of a MATSim grid with SRC /
    DEST pseudo-nodes (SRC: no in-edges, DEST: no out-edges, uneven degrees) or of an irregular road graph (MIXED: degrees
    0 - 9, HUB126: one hub of 126 in- and out-edges; edge lists in no order)."""
    from tarl_hip import synth
    if kind in ("MIXED", "HUB126"):
        import irregular_graphs
        net = irregular_graphs.graph(kind)
        return net.edge_index, net.edge_attr, net.x, net.Nmax, net.num_roads, net.edge_index
    if kind == "matsim":
        from src.matsim_io import build_network
        synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 4, 6, seed=3)
        g, Nmax = build_network(str(tmp_path / "network"))
        return g.edge_index, g.edge_attr, g.x, Nmax, g.num_roads, g.edge_index_routes
    W, H = {"torus8": (8, 8), "torus16": (16, 16), "config4": (25, 25)}[kind]
    net = synth.torus_network(W, H, heterogeneous=True, seed=W)
    return net.edge_index, net.edge_attr, net.x, net.Nmax, net.num_roads, net.edge_index


def _real_obs(x, Nmax, num_roads, M, seed):
    """Observations as the simulator builds them: the static node columns, counts in [0, MAXN], the head agent's row of a
    synthetic population (raw origin / destination ids and clock-time departure columns)."""
    from tarl_hip import synth
    g = torch.Generator().manual_seed(seed)
    N = x.size(0)
    nf = x[:, 3 * Nmax:3 * Nmax + 7].clone().unsqueeze(0).repeat(M, 1, 1)
    nf[..., 1] = torch.floor(torch.rand((M, N), generator=g) * (nf[..., 0] + 1))
    pop = synth.population(4 * N, num_roads, seed=seed, t0=21540, t1=25200)
    ag = pop[torch.randint(0, pop.size(0), (M, N), generator=g)]
    ag[..., 3] = torch.where(ag[..., 2] < 23000, ag[..., 2] + 600 * torch.rand((M, N), generator=g), torch.zeros(()))
    return torch.cat((nf, ag), dim=-1).contiguous()


SHARP_CRITIC_RESEED = {("MIXED", 1): 4, ("HUB126", 3): 2}


def case_inputs(kind, M, weights, critic, tmp_path):
    """The inputs of one case of test_forward_and_backward_match_the_restatement (policy head, or critic), built once the
    same way for the GPU test and for the CPU proof of what that test can see. Seeds: the policy's tests draw the weights
    with E + M and the observations with M + 5, the critic's with N + M and M + 9; the critic's sharp cases take the
    policy's seeds, with which they meet the census conditions (with the critic's own, three do not), and where the layer-1
    scores still stay below CENSUS_OVERFLOW_SCORE the first later weight seed that meets them all (SHARP_CRITIC_RESEED)."""
    from src.transformer import laplacian_pe
    ei, ea, x, Nmax, R, routes = _graph(kind, tmp_path)
    N, E = x.size(0), ei.size(1)
    own = critic and weights != "sharp"
    reseed = SHARP_CRITIC_RESEED.get((kind, M), 0) if critic and weights == "sharp" else 0
    sd = _state(weights, (N if own else E) + M + reseed, critic)
    pe = laplacian_pe(routes, R, N)
    obs = _real_obs(x, Nmax, R, M, seed=M + (9 if own else 5))
    if critic:
        coef = torch.randn(M, generator=torch.Generator().manual_seed(M + 1))
    else:
        coef = torch.randn(M, E, generator=torch.Generator().manual_seed(M))
    return types.SimpleNamespace(kind=kind, M=M, weights=weights, critic=critic, ei=ei, ea=ea, x=x, Nmax=Nmax, R=R, N=N, E=E,
                                 sd=sd, pe=pe, obs=obs, coef=coef)


def param_keys(critic):
    from tarl_hip import ops
    return ops.GT_VALUE_PARAM_KEYS if critic else ops.GT_PARAM_KEYS


def restate(c, dt, device="cpu", capture=None, grad=True):
    """The restatement of case ``c`` in ``dt``: (output, parameters) — the policy's logits (M, E) or the critic's values
    (M,); the parameters of the kernel's list require a gradient when ``grad``."""
    import gt_restatement as R
    import gt_value_restatement as RV
    keys = param_keys(c.critic)
    p = {k: (v.to(device, dt, copy=True).requires_grad_(True) if grad and k in keys else v.to(device, dt))
         for k, v in c.sd.items()}
    if c.critic:
        out = RV.gt_value(p, c.obs.to(device, dt), c.ei.to(device), c.pe.to(device, dt), capture=capture)
    else:
        out = R.gt_logits(p, c.obs.to(device, dt), c.ei.to(device), c.ea.to(device, dt), c.pe.to(device, dt), capture=capture)
    return out, p


def references(c, device="cpu"):
    """Case ``c`` in float64 (the exact reference) and in float32 (what plain fp32 autograd of the same function achieves:
    its distance from float64 measures how the inputs condition the function at fp32 precision), with the gradients of
    sum(coef * output): (ref64, ref32, g64, g32, S) on the CPU in float64; S the float64 run's term magnitudes."""
    import gt_restatement as R
    out = {}
    for dt in (torch.float64, torch.float32):
        cap = []
        ref, p = restate(c, dt, device, capture=cap)
        (c.coef.to(device, dt) * ref).sum().backward()
        out[dt] = (ref.detach().double().cpu(), {k: p[k].grad.double().cpu() for k in param_keys(c.critic)},
                   {k: v.double().cpu() for k, v in R.term_magnitudes(cap).items()} if dt == torch.float64 else None)
    ref64, g64, S = out[torch.float64]
    ref32, g32, _ = out[torch.float32]
    return ref64, ref32, g64, g32, S


def sharp_tolerance(ref64, ref32):
    """The output tolerance of a sharp case: SHARP_FACTOR x the fp32 restatement's own distance from float64 + a floor of
    SHARP_FLOOR_ULPS fp32 ulps of the output's scale. It depends on the two restatements alone."""
    return (SHARP_FACTOR * float((ref32 - ref64).abs().max())
            + SHARP_FLOOR_ULPS * 2.0 ** -24 * max(float(ref64.abs().max()), 1.0))


def items_per_sample(k, critic, N, E):
    """Items (nodes, edges, or the sample itself) per sample in the sum that is parameter ``k``'s gradient."""
    if critic:
        return 1 if k.startswith("mu_mlp") else N
    node_side = k.startswith(("node_emb", "pe_emb")) or (k.startswith("gt_layers.") and not any(
        s_ in k for s_ in ("WE", "WOe", "norm1e", "norm2e", "ffn_e")))
    return N if node_side else E


def grad_allowance(k, g64, g32, S, c):
    """The elementwise allowance of parameter ``k``'s gradient: the kernel's error may exceed fp32 autograd's (largest over
    the tensor) by at most a factor 16 — the two evaluate the same function in different, equally valid fp32 forms (e.g. the
    softmax backward as alpha * (g - sum alpha g) against autograd of exp / sum), and on raw observations the saturated
    softmax makes each form's error proportional to the score magnitude rather than to u — plus the kernel's own summation
    bound."""
    return (16 * float((g32[k] - g64[k]).abs().max())
            + _sum_bound(S[k].double().cpu(), c.M, items_per_sample(k, c.critic, c.N, c.E)).view_as(g64[k]))


def attention_census(sd, obs, ei, pe, critic, edge_attr=None):
    """What the attention of the float64 restatement looks like on these inputs: per attention layer the kernel evaluates
    (the policy: layer 0; the critic: layers 0 and 1), over the segments (sample, node, head) of in-degree >= 2, a dict of
    max |score| (over all edges), the median over segments of (max - min score), the share of segments whose largest alpha
    exceeds 0.999 and the share whose spread is below 0.1. The scores are the restatement's own, recorded in
    ``gt_restatement._segment_softmax``. (``edge_attr`` does not reach the policy's layer-0 scores; zeros when not given.)"""
    import gt_restatement as R
    import gt_value_restatement as RV
    p = {k: v.double() for k, v in sd.items()}
    rec = []
    R._SCORES = rec
    try:
        with torch.no_grad():
            if critic:
                RV.gt_value(p, obs.double(), ei, pe.double())
            else:
                ea = torch.zeros((ei.size(1), 1)) if edge_attr is None else edge_attr
                R.gt_logits(p, obs.double(), ei, ea.double(), pe.double())
    finally:
        R._SCORES = None
    assert len(rec) == (2 if critic else 1)
    out = []
    for L, (s, index, N) in enumerate(rec):
        M, E, H = s.shape
        idx = index.view(1, E, 1).expand(M, E, H)
        hi = torch.full((M, N, H), float("-inf"), dtype=s.dtype).scatter_reduce(1, idx, s, "amax")
        lo = torch.full((M, N, H), float("inf"), dtype=s.dtype).scatter_reduce(1, idx, s, "amin")
        top = torch.zeros((M, N, H), dtype=s.dtype).scatter_reduce(1, idx, R._segment_softmax(s, index, N), "amax")
        seg = (torch.bincount(index, minlength=N) >= 2).view(1, N, 1).expand(M, N, H)
        spread = (hi - lo)[seg]
        out.append(dict(layer=L, max_abs_score=float(s.abs().max()), median_spread=float(spread.median()),
                        share_one_hot=float((top[seg] > 0.999).double().mean()),
                        share_flat=float((spread < 0.1).double().mean())))
    return out


def check_census(census, critic):
    """The conditions a sharp case's inputs meet before a kernel is called: the attention is neither one-hot nor uniform, the
    scores are within fp32's reach, and the critic's layer-1 scores would overflow expf without the max subtraction."""
    for f in census:
        assert f["share_one_hot"] <= CENSUS_MAX_ONE_HOT, f
        assert f["share_flat"] <= CENSUS_MAX_FLAT, f
        assert f["median_spread"] >= CENSUS_MIN_MEDIAN_SPREAD, f
        assert f["max_abs_score"] < CENSUS_MAX_SCORE, f
    if critic:
        assert census[1]["max_abs_score"] > CENSUS_OVERFLOW_SCORE, census[1]


def graph_facts(ei, N):
    """(max in-degree, max out-degree, nodes of in-degree 0, nodes of out-degree 0, is the edge list sorted by source)."""
    indeg, outdeg = torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)
    return (int(indeg.max()), int(outdeg.max()), int((indeg == 0).sum()), int((outdeg == 0).sum()),
            bool((ei[0][1:] >= ei[0][:-1]).all()))


IRREGULAR_MAX_DEGREE = {"MIXED": 9, "HUB126": 126}


def order_preserving_shuffle(ei, seed):
    """Another order of the edge list that keeps every node's in-edges and every node's out-edges in their relative order
    (the plan sorts both segments by edge id, so the kernels walk them exactly as before): ``order`` (E,), the old id of
    the edge at each new position — a random linear extension of "comes after the previous edge with my target and after
    the previous edge with my source"."""
    E = ei.size(1)
    succ, waits = [[] for _ in range(E)], [0] * E
    for row in (0, 1):
        last = {}
        for e, n in enumerate(ei[row].tolist()):
            if n in last:
                succ[last[n]].append(e)
                waits[e] += 1
            last[n] = e
    g = torch.Generator().manual_seed(seed)
    ready = [e for e in range(E) if waits[e] == 0]
    order = []
    while ready:
        e = ready.pop(int(torch.randint(0, len(ready), (1,), generator=g)))
        order.append(e)
        for f in succ[e]:
            waits[f] -= 1
            if waits[f] == 0:
                ready.append(f)
    assert len(order) == E
    order = torch.tensor(order)
    for row in (0, 1):                       # every segment's old ids still ascend
        key = ei[row][order]
        by_node = order[torch.argsort(key, stable=True)]
        same = torch.sort(key).values
        assert bool(((by_node[1:] > by_node[:-1]) | (same[1:] != same[:-1])).all())
    return order


def _sum_bound(S, M, items_per_sample):
    """Rounding bound of the kernel's summation of a weight gradient, an fp32 sum of n terms t_i (S = sum |t_i|, from the
    float64 restatement): sequential sums of 1 024-item chunks, then the chunk partials in order, err <= (1024 + chunks) u S
    (u = 2^-24; the classical bound of recursive summation)."""
    chunks = -(-M * items_per_sample // 1024)
    return (1024 + chunks) * 2.0 ** -24 * S


def _span(tr, p):
    off, n = tr.flat.offsets[id(p)]
    return off, off + n
