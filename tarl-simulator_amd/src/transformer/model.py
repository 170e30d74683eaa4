"""GraphTransformerNet / GTConv / MLP with the reference's module tree, construction order and initialisation
(src/transformer/model.py, gt_conv.py, mlp.py), so that state-dict keys and seeded initial values match a reference
module of the same dimensions. ``GraphTransformerNet.edge_logits`` is the edge output (raw=True, model.py:174-178) in
evaluation mode on the kernels (tarl_policy_gt_fwd / _bwd): BatchNorm on its running statistics, dropout = identity. The
node / value outputs (global pool, mu_mlp, log_var_mlp) are not implemented; their parameters stay in the tree.
"""
from __future__ import annotations

import torch
from torch import nn


class MLP(nn.Module):
    """Linear -> ReLU -> [Dropout if dropout > 0] -> Linear (src/transformer/mlp.py): keys mlp.0 / mlp.3 (or mlp.2)."""

    def __init__(self, input_dim, output_dim, hidden_dims, num_hidden_layers=1, dropout=0.0, act="relu"):
        super().__init__()
        if act != "relu":
            raise ValueError("only act='relu' is implemented")
        if isinstance(hidden_dims, int):
            hidden_dims = [hidden_dims] * num_hidden_layers
        dims = [input_dim] + list(hidden_dims)
        layers = []
        for i, o in zip(dims[:-1], dims[1:]):
            layers += [nn.Linear(i, o, bias=True), nn.ReLU()]
            if dropout > 0.0:
                layers.append(nn.Dropout(p=dropout))
        layers.append(nn.Linear(dims[-1], output_dim, bias=True))
        self.mlp = nn.Sequential(*layers)


class GTConv(nn.Module):
    """Parameters of one graph-transformer layer (src/transformer/gt_conv.py:17-141), edge features and gate on."""

    def __init__(self, node_in_dim, hidden_dim, edge_in_dim, num_heads=8, gate=True, qkv_bias=False, dropout=0.0,
                 act="relu"):
        super().__init__()
        if not gate or qkv_bias or edge_in_dim is None:
            raise ValueError("the kernels implement gate=True, qkv_bias=False with edge features")
        self.WQ = nn.Linear(node_in_dim, hidden_dim, bias=False)
        self.WK = nn.Linear(node_in_dim, hidden_dim, bias=False)
        self.WV = nn.Linear(node_in_dim, hidden_dim, bias=False)
        self.WO = nn.Linear(hidden_dim, node_in_dim, bias=True)
        self.WE = nn.Linear(edge_in_dim, hidden_dim, bias=True)
        self.WOe = nn.Linear(hidden_dim, edge_in_dim, bias=True)
        self.ffn_e = MLP(edge_in_dim, edge_in_dim, hidden_dim, 1, dropout, act)
        self.norm1e = nn.BatchNorm1d(edge_in_dim)
        self.norm2e = nn.BatchNorm1d(edge_in_dim)
        self.norm1 = nn.BatchNorm1d(node_in_dim)
        self.norm2 = nn.BatchNorm1d(node_in_dim)
        self.n_gate = nn.Linear(node_in_dim, hidden_dim, bias=True)
        self.e_gate = nn.Linear(edge_in_dim, hidden_dim, bias=True)
        self.dropout_layer = nn.Dropout(p=dropout)
        self.ffn = MLP(node_in_dim, node_in_dim, hidden_dim, 1, dropout, act)
        self.num_heads = num_heads
        for lin in (self.WQ, self.WK, self.WV, self.WO, self.WE, self.WOe):      # reset_parameters (gt_conv.py:132-141)
            nn.init.xavier_uniform_(lin.weight)


class _GtLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs16, plan, ec, pe, tensors, *params):
        from tarl_hip import ops
        w = ops.GtWeights(tensors)
        ctx.saved = (obs16, plan, ec, pe, w)
        return ops.policy_gt_logits(plan, obs16, ec, pe, w)

    @staticmethod
    def backward(ctx, grad_logits):
        from tarl_hip import ops
        obs16, plan, ec, pe, w = ctx.saved
        grads = [torch.zeros_like(p) for p in w.params]
        ops.policy_gt_bwd(plan, obs16, ec, pe, w, grad_logits.contiguous(), grads)
        return (None, None, None, None, None) + tuple(grads)


class GraphTransformerNet(nn.Module):
    """src/transformer/model.py:15-143 for the head MLAgents builds; construction order (and so the seeded initial
    values) as the reference's."""

    def __init__(self, node_dim_in=16, edge_dim_in=1, pe_in_dim=16, hidden_dim=16, gate=True, qkv_bias=False,
                 num_gt_layers=2, num_heads=4, act="relu", dropout=0.0):
        super().__init__()
        if (node_dim_in, edge_dim_in, pe_in_dim, hidden_dim, num_gt_layers, num_heads) != (16, 1, 16, 16, 2, 4):
            raise ValueError("the kernels implement GraphTransformerNet(16, 1, 16, hidden 16, 2 layers, 4 heads)")
        self.node_emb = nn.Linear(node_dim_in, hidden_dim, bias=False)
        self.edge_emb = nn.Linear(edge_dim_in, hidden_dim, bias=False)
        self.pe_emb = nn.Linear(pe_in_dim, hidden_dim, bias=False)
        self.gt_layers = nn.ModuleList(
            GTConv(hidden_dim, hidden_dim, hidden_dim, num_heads, gate, qkv_bias, dropout, act) for _ in range(num_gt_layers))
        self.mu_mlp = MLP(hidden_dim, 1, hidden_dim, 1, 0.0, act)
        self.log_var_mlp = MLP(hidden_dim, 1, hidden_dim, 1, 0.0, act)
        self.edge_linear = nn.Linear(hidden_dim, 1)
        for lin in (self.node_emb, self.edge_emb, self.pe_emb, self.edge_linear):     # model.py:120-134
            nn.init.xavier_uniform_(lin.weight)

    def kernel_tensors(self):
        """{state-dict key: tensor} of what the kernels read (ops.GT_PARAM_KEYS + GT_BUFFER_KEYS)."""
        from tarl_hip import ops
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        return {k: sd[k] for k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS}

    def edge_logits(self, obs16, plan, ec, pe):
        """obs16 (M, N, 16) -> logits (M, E) on the kernels; gradients reach the parameters of ops.GT_PARAM_KEYS (the
        others get none, as they do not reach the logits)."""
        from tarl_hip import ops
        t = self.kernel_tensors()
        return _GtLogits.apply(obs16, plan, ec, pe, t, *(t[k] for k in ops.GT_PARAM_KEYS))
