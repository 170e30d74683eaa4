"""Pure-torch CPU restatement of the graph-transformer critic (value_head = "graph_transformer"), written from the semantics
in DESIGN.md §4.11: the node output of GraphTransformerNet(16, 1, 16, hidden 16, gate=True, 2 layers, 4 heads) in
evaluation mode, summed over each sample's nodes, then mu_mlp. ``sd`` maps GraphTransformerNet state-dict keys to tensors.
``capture``: as :func:`gt_restatement.gt_logits` (per-item operands and outputs for :func:`gt_restatement.term_magnitudes`).
"""
import torch

import gt_restatement as G


def gt_value(sd, obs, edge_index, pe, capture=None):
    """obs (M, N, 16) or (N, 16), pe (N, 16) -> value (M,) or a scalar tensor."""
    G._CAPTURE.append(capture)
    try:
        return _gt_value(sd, obs, edge_index, pe)
    finally:
        G._CAPTURE.pop()


def _gt_value(sd, obs, edge_index, pe):
    single = obs.dim() == 2
    x = obs.unsqueeze(0) if single else obs
    M, N, _ = x.shape
    u, v = edge_index[0], edge_index[1]
    E = u.numel()
    x = G._lin(sd, "node_emb", x, False) + G._lin(sd, "pe_emb", pe.expand(M, N, 16), False)
    for L in range(2):
        p = f"gt_layers.{L}."
        Q = G._lin(sd, p + "WQ", x, False)
        K = G._lin(sd, p + "WK", x, False)
        V = G._lin(sd, p + "WV", x, False)
        gate = G._lin(sd, p + "n_gate", x)
        score = (Q.index_select(1, v) * G._gather_k(K, u)).view(M, E, 4, 4).sum(-1) / 2.0
        alpha = G._segment_softmax(score, v, N)
        msg = (alpha.unsqueeze(-1) * (V * torch.sigmoid(gate)).index_select(1, u).view(M, E, 4, 4)).reshape(M, E, 16)
        agg = torch.zeros((M, N, 16), dtype=x.dtype, device=x.device).index_add(1, v, msg)
        y = G._bn(sd, p + "norm1", G._lin(sd, p + "WO", agg) + x)
        x = G._bn(sd, p + "norm2", y + G._ffn(sd, p + "ffn", y))
    pooled = x.sum(1)                                   # MultiAggregation(["sum"]) over the sample's nodes
    value = G._lin(sd, "mu_mlp.mlp.2", torch.relu(G._lin(sd, "mu_mlp.mlp.0", pooled))).squeeze(-1)
    return value[0] if single else value
