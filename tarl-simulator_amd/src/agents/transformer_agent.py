"""ValueNet — the graph-transformer critic of the reference (src/agents/transformer_agent.py:257-323, ``ValueNet(MLAgents)``).

A second GraphTransformerNet (hidden 16, 4 heads, gate, 2 layers, dropout 0.1 — the policy head's shape, its own
parameters) on the same observation the graph-transformer policy reads: value = mu_mlp(sum over all N nodes of x2), the
``raw=True`` branch of model.py:174-178 with ``MultiAggregation(["sum"])`` over each sample's nodes (SRC / DEST pseudo-nodes
included). Evaluation mode on the kernels of csrc/gt_value.hip: BatchNorm on its running statistics, dropout = identity,
node input 16 columns (``obs16``, not the reference's stale ``node_dim_in=15``).

Reference quirk: its unbatched branch (:310-322) never binds ``edge_index`` or ``positional_embedding`` and raises
UnboundLocalError. Here the unbatched call uses the module's own edge index and encoding: the batched path with M = 1.
"""
from __future__ import annotations

import torch

from .._compat import MessagePassingBase, cached_plan, require_cuda
from ..transformer import GraphTransformerNet
from .base import Agents


class _GtValue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs16, plan, pe, tensors, *params):
        from tarl_hip import ops
        w = ops.GtValueWeights(tensors)
        ctx.saved = (obs16, plan, pe, w)
        return ops.value_gt_forward(plan, obs16, pe, w)

    @staticmethod
    def backward(ctx, grad_value):
        from tarl_hip import ops
        obs16, plan, pe, w = ctx.saved
        grads = [torch.zeros_like(p) for p in w.params]
        ops.value_gt_backward(plan, obs16, pe, w, grad_value.contiguous(), grads)
        return (None, None, None, None) + tuple(grads)


class ValueNet(MessagePassingBase, Agents):
    """``transformer``: GraphTransformerNet(16, 1, 16, 16, gate=True, 2 layers, 4 heads, dropout 0.1), evaluation mode;
    ``gt_pe`` (N, 16): the positional encoding (the same ``cached_laplacian_pe`` as the policy's, MLAgents builds both with
    ``compute_encodings`` on the same road graph). ``agent_features``: the population, as every ``Agents``."""

    def __init__(self, edge_index, num_nodes, device, pe: torch.Tensor):
        Agents.__init__(self, device=device)
        MessagePassingBase.__init__(self, aggr="add", flow="source_to_target")
        if tuple(pe.shape) != (num_nodes, 16):
            raise ValueError(f"pe must be ({num_nodes}, 16)")
        self.edge_index = edge_index
        self.num_nodes = num_nodes
        self.transformer = GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4, dropout=0.1)
        self.register_buffer("gt_pe", pe.detach().to(torch.float32).contiguous())
        self.eval()
        self.to(device)

    def kernel_tensors(self):
        """{state-dict key of ``transformer``: tensor} of what the kernels read (ops.GT_VALUE_PARAM_KEYS +
        GT_VALUE_BUFFER_KEYS)."""
        from tarl_hip import ops
        sd = dict(self.transformer.named_parameters())
        sd.update(dict(self.transformer.named_buffers()))
        return {k: sd[k] for k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS}

    def value(self, obs16):
        """obs16 (M, N, 16) -> value (M,) on the kernels; gradients reach the parameters of ops.GT_VALUE_PARAM_KEYS (the
        edge side of the network gets none: it does not reach the node output)."""
        from tarl_hip import ops
        plan = cached_plan(self.edge_index, self.num_nodes)
        t = self.kernel_tensors()
        return _GtValue.apply(obs16, plan, self.gt_pe, t, *(t[k] for k in ops.GT_VALUE_PARAM_KEYS))

    def forward(self, node_features, edge_features, agent_index, time=None):
        """node_features (N,7) or (B,N,7), agent_index (N,) or (B,N) -> (1,1) or (B,1). ``edge_features`` and ``time``
        (the ValueOperator's in_keys) are not read: the node output never sees the edge features."""
        require_cuda(node_features, "node_features")
        if self.training:
            raise RuntimeError("ValueNet runs in evaluation mode only: call .eval() (the kernels implement BatchNorm on its "
                               "running statistics and Dropout as the identity)")
        from tarl_hip import ops
        obs16 = ops.policy_obs16(node_features, agent_index, self.agent_features.to(node_features.device))
        return self.value(obs16).view(-1, 1)
