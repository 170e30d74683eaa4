"""Pure-torch CPU restatement of the graph-transformer policy head (policy_head = "graph_transformer"), written from the
semantics in DESIGN.md §4.10: GraphTransformerNet(16, 1, 16, hidden 16, gate=True, 2 layers, 4 heads) in evaluation mode,
edge output. ``sd`` maps GraphTransformerNet state-dict keys to tensors; autograd through it gives the parameter gradients.

``capture`` (a list) records, per parameter use, the per-item operand and output of every Linear / BatchNorm, so that after
``backward()`` :func:`term_magnitudes` gives, for each parameter element, the sum over items (sample, node) or (sample, edge)
of the absolute values of the terms its gradient is the sum of: the scale of the rounding error of a summed gradient.

Two seams for the tests of the tests: ``_SCORES`` (a list, when set) receives the scores of every segment softmax
(gt_cases.attention_census), and gt_mutants.py swaps ``_segment_softmax`` / ``_gather_k`` for deliberately wrong variants.
"""
import torch

_CAPTURE = []


def _record(key, kind, a, y):
    if _CAPTURE and _CAPTURE[-1] is not None and y.requires_grad:
        y.retain_grad()
        _CAPTURE[-1].append((key, kind, a.detach(), y))


def _lin(sd, key, x, bias=True):
    y = x @ sd[key + ".weight"].t()
    y = y + sd[key + ".bias"] if bias else y
    _record(key, "lin_b" if bias else "lin", x, y)
    return y


def _bn(sd, key, x):
    xh = (x - sd[key + ".running_mean"]) / torch.sqrt(sd[key + ".running_var"] + 1e-5)
    y = xh * sd[key + ".weight"] + sd[key + ".bias"]
    _record(key, "bn", xh, y)
    return y


def term_magnitudes(capture):
    """{parameter key: sum over items of |term|} from a ``capture`` list filled by :func:`gt_logits` and a backward."""
    out = {}
    for key, kind, a, y in capture:
        g = y.grad.abs().reshape(-1, y.size(-1))
        a = a.abs().reshape(-1, a.size(-1))
        if kind == "bn":
            w = {key + ".weight": (g * a).sum(0), key + ".bias": g.sum(0)}
        else:
            w = {key + ".weight": g.t() @ a}
            if kind == "lin_b":
                w[key + ".bias"] = g.sum(0)
        for k, v in w.items():
            out[k] = out.get(k, 0) + v
    return out


def _ffn(sd, key, x):
    return _lin(sd, key + ".mlp.3", torch.relu(_lin(sd, key + ".mlp.0", x)))


_SCORES = None      # optional recorder: a list that receives (scores (M, E, H) detached, index, N) of every segment softmax


def _gather_k(K, u):
    """K of every edge's source node: (M, N, 16) -> (M, E, 16)."""
    return K.index_select(1, u)


def _segment_softmax(s, index, N):
    """s (M, E, H) over the edges of each target index (PyG 2.5 utils.softmax: max subtracted, + 1e-16)."""
    if _SCORES is not None:
        _SCORES.append((s.detach(), index, N))
    M, E, H = s.shape
    mx = torch.full((M, N, H), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(1, index.view(1, E, 1).expand(M, E, H),
                                                                               s.detach(), "amax", include_self=True)
    w = torch.exp(s - mx.index_select(1, index))
    den = torch.zeros((M, N, H), dtype=s.dtype, device=s.device).index_add(1, index, w) + 1e-16
    return w / den.index_select(1, index)


def gt_logits(sd, obs, edge_index, edge_attr, pe, capture=None):
    """obs (M, N, 16) or (N, 16), edge_attr (E, 1) or (E,), pe (N, 16) -> logits (M, E) or (E,)."""
    _CAPTURE.append(capture)
    try:
        return _gt_logits(sd, obs, edge_index, edge_attr, pe)
    finally:
        _CAPTURE.pop()


def _gt_logits(sd, obs, edge_index, edge_attr, pe):
    single = obs.dim() == 2
    x = obs.unsqueeze(0) if single else obs
    M, N, _ = x.shape
    u, v = edge_index[0], edge_index[1]
    E = u.numel()
    # (the per-sample operands are expanded before the products so that every item's term is recorded)
    x = _lin(sd, "node_emb", x, False) + _lin(sd, "pe_emb", pe.expand(M, N, 16), False)
    e = _lin(sd, "edge_emb", edge_attr.reshape(1, E, 1).expand(M, E, 1), False)
    for L in range(2):
        p = f"gt_layers.{L}."
        Q = _lin(sd, p + "WQ", x, False)
        K = _lin(sd, p + "WK", x, False)
        Qi, Kj = Q.index_select(1, v), _gather_k(K, u)
        q = (Qi * Kj) / 2.0
        eij = _lin(sd, p + "WE", e) * q
        if L == 0:        # the last layer's node update reaches only x2 (pool / value), not the logits
            V = _lin(sd, p + "WV", x, False)
            G = _lin(sd, p + "n_gate", x)
            score = (Qi * Kj).view(M, E, 4, 4).sum(-1) / 2.0
            alpha = _segment_softmax(score, v, N)
            msg = (alpha.unsqueeze(-1) * (V * torch.sigmoid(G)).index_select(1, u).view(M, E, 4, 4)).reshape(M, E, 16)
            agg = torch.zeros((M, N, 16), dtype=x.dtype, device=x.device).index_add(1, v, msg)
            y = _bn(sd, p + "norm1", _lin(sd, p + "WO", agg) + x)
            x_new = _bn(sd, p + "norm2", y + _ffn(sd, p + "ffn", y))
        z = _bn(sd, p + "norm1e", _lin(sd, p + "WOe", eij) + e)
        e = _bn(sd, p + "norm2e", z + _ffn(sd, p + "ffn_e", z))
        if L == 0:
            x = x_new
    logits = _lin(sd, "edge_linear", e).squeeze(-1)
    return logits[0] if single else logits


def torus(W, H):
    """Directed W x H torus: node (i, j) -> its four neighbours, edges grouped by source (int64 (2, 4WH))."""
    src, dst = [], []
    for i in range(H):
        for j in range(W):
            n = i * W + j
            for di, dj in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                src.append(n)
                dst.append(((i + di) % H) * W + (j + dj) % W)
    return torch.tensor([src, dst], dtype=torch.int64)
