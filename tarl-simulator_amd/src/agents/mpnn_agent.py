"""MPNNPolicyNet / MPNNValueNetSimple — the learned actor and critic (reference: src/agents/mpnn_agent.py).

Same constructors, ``forward`` signatures and state-dict keys (``nodes_embedding.weight``, ``edge_mlp.{0,2,4}.*``,
``edge_mlp_test.{0,2}.*``, ``final_mlp.{0,2,4}.*``). Live actor: logits[e] = W_emb[ROAD_INDEX(dst(e))]
(``tarl_policy_edge_logits_fwd/bwd``); live critic: MLP(cat(NUMBER_OF_AGENT per node, time)) on fp32 MFMA
(``tarl_critic_mlp_fwd/bwd``). What the reference computes and discards after the logits (Dijkstra prior, travel
time, norm — :181-190) is not evaluated by the default head; ``policy_head = "embedding_dijkstra"`` adds the prior
(``tarl_policy_prior_logits``). The all-pairs Dijkstra matrix of its constructor is built lazily on request;
``prior_method = "per_destination"`` replaces it by one column per destination of the agent table.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .._compat import MessagePassingBase, cached_plan, require_cuda
from ..algorithms.user_equilibrium_msa import ALL_PAIRS_MAX_NODES
from ..feature_helpers import ObservationFeatureHelpers
from .base import Agents, destination_set


class _EdgeLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb_weight, node_features, plan):
        from tarl_hip import ops
        ctx.plan, ctx.nf, ctx.shape = plan, node_features, emb_weight.shape
        return ops.policy_edge_logits(plan, node_features, emb_weight.detach().reshape(-1).contiguous())

    @staticmethod
    def backward(ctx, grad_logits):
        from tarl_hip import ops
        g = ops.policy_edge_logits_bwd(ctx.plan, ctx.nf, grad_logits.contiguous(), int(torch.Size(ctx.shape).numel()))
        return g.view(ctx.shape), None, None


class _PriorLogits(torch.autograd.Function):
    """The embedding plus the weighted shortest-path prior (tarl_policy_prior_logits); the prior has no parameters, so the
    embedding receives the logits' gradient through tarl_policy_edge_logits_bwd (ROAD_INDEX = observation column 6)."""

    @staticmethod
    def forward(ctx, emb_weight, obs16, plan, table, prior_weight, dest_slot):
        from tarl_hip import ops
        ctx.plan, ctx.obs, ctx.shape = plan, obs16, emb_weight.shape
        return ops.policy_prior_logits(plan, obs16, emb_weight.detach().reshape(-1).contiguous(), table, prior_weight,
                                       dest_slot=dest_slot)

    @staticmethod
    def backward(ctx, grad_logits):
        from tarl_hip import ops
        g = ops.policy_edge_logits_bwd(ctx.plan, ctx.obs, grad_logits.contiguous(), int(torch.Size(ctx.shape).numel()))
        return g.view(ctx.shape), None, None, None, None, None


class _EdgeMlp(torch.autograd.Function):
    """The per-edge MLP head on the HIP kernels (tarl_policy_edge_mlp_fwd / _bwd); gradients for its six parameters."""

    @staticmethod
    def forward(ctx, obs16, plan, ec, bf16, w1, b1, w2, b2, w3, b3):
        from tarl_hip import ops
        w = ops.EdgeMlpWeights(w1, b1, w2, b2, w3, b3)
        ctx.saved = (obs16, plan, ec, w, [t.shape for t in (w1, b1, w2, b2, w3, b3)])
        return ops.policy_edge_mlp(plan, obs16, ec, w, bf16=bf16)

    @staticmethod
    def backward(ctx, grad_logits):
        from tarl_hip import ops
        obs16, plan, ec, w, shapes = ctx.saved
        grads = [torch.zeros_like(t) for t in (w.w1, w.b1, w.w2, w.b2, w.w3, w.b3)]
        ops.policy_edge_mlp_bwd(plan, obs16, ec, w, grad_logits.contiguous(), grads)
        return (None, None, None, None) + tuple(g.view(sh) for g, sh in zip(grads, shapes))


class _GoalMlp(torch.autograd.Function):
    """The goal-conditioned MLP head on the HIP kernels (tarl_policy_goal_mlp_fwd / _bwd); gradients for its four
    parameters, cut from the kernels' flat (161,) gradient."""

    @staticmethod
    def forward(ctx, obs16, plan, table, dest_slot, time_scale, w1, b1, w2, b2):
        from tarl_hip import ops
        w = ops.GoalMlpWeights(w1, b1, w2, b2)
        ctx.saved = (obs16, plan, table, dest_slot, time_scale, w, [t.shape for t in (w1, b1, w2, b2)])
        return ops.policy_goal_mlp(plan, obs16, w, table, time_scale, dest_slot=dest_slot)

    @staticmethod
    def backward(ctx, grad_logits):
        from tarl_hip import ops
        obs16, plan, table, dest_slot, time_scale, w, shapes = ctx.saved
        flat = torch.zeros(ops.GOAL_MLP_PARAMS, dtype=torch.float32, device=obs16.device)
        ops.policy_goal_mlp_bwd(plan, obs16, w, table, time_scale, grad_logits.contiguous(), flat, dest_slot=dest_slot)
        parts = torch.split(flat, [int(torch.Size(s).numel()) for s in shapes])
        return (None, None, None, None, None) + tuple(g.view(s) for g, s in zip(parts, shapes))


class MPNNPolicyNet(MessagePassingBase, Agents):
    h = ObservationFeatureHelpers()
    # Which head produces the logits. "embedding": the reference's live forward (logit = nodes_embedding of the target
    # road, src/agents/mpnn_agent.py:215-217). "edge_mlp" / "edge_mlp_fp32" / "edge_mlp_bf16": the per-edge MLP the reference
    # keeps as parameters and spells out in its commented lines (:227-231), on fp32 / bf16 MFMA — a state-dependent policy
    # (this module's forward runs the fp32 MFMA kernel for the first two; the names differ in the ROLLOUT kernel the trainer
    # picks: fp32 accuracy on the bf16 pipe / exact fp32 products / bf16). "embedding_dijkstra": the embedding plus
    # ``prior_weight`` times the shortest-path prior the reference computes and leaves commented out (:180-190):
    # -dist[dst(e), DESTINATION of the head agent of src(e)] - time_travel(dst(e)), dist = ``dist_matrix`` (state-dependent,
    # no parameters of its own; prior_weight = 1 is the reference's literal sum).
    # "graph_transformer": the reference's GraphTransformerNet edge output (src/transformer/model.py, as MLAgents builds it),
    # evaluation-mode BatchNorm; its ``transformer`` submodule and ``gt_pe`` buffer exist only after
    # :meth:`use_graph_transformer`, so the other heads' state dicts do not change.
    # "goal_mlp" (not in the reference): a trainable per-edge MLP 8 -> 16 -> 1 on destination-relative features built from the
    # prior head's quantities (csrc/goal_mlp.hip); its ``goal_mlp`` submodule and ``goal_scale`` buffer exist only after
    # :meth:`use_goal_mlp`. It reads the same distance tables as the prior (``prior_method`` below).
    # Where the prior's distances come from: "all_pairs" = ``dist_matrix`` (N x N, tarl_apsp); "per_destination" = one
    # column per distinct DESTINATION of the agent table, (N, D) fp32 (tarl_prior_dest_table; ``dist_matrix`` is never
    # built); "auto" = all_pairs up to ALL_PAIRS_MAX_NODES nodes, per_destination above. The same logits either way
    # wherever tarl_dest_trees' exactness condition holds.
    policy_head = "embedding"
    prior_weight = 1.0
    prior_method = "all_pairs"
    PRIOR_METHODS = ("all_pairs", "per_destination", "auto")

    def __init__(self, edge_index, num_nodes, free_flow_time_travel, device):
        Agents.__init__(self, device=device)
        MessagePassingBase.__init__(self, aggr="mean", flow="target_to_source")
        self.edge_index = edge_index
        self.num_nodes = num_nodes
        self.num_edges = edge_index.size(1)
        self.dim_node_features = 16
        self.dim_edge_features = 1
        self._free_flow = free_flow_time_travel
        self._dist_matrix = None
        self._prior_dest = None         # per_destination: (table (N, D), dest_slot (N,), the agent table it covers)
        self.nodes_embedding = nn.Embedding(num_nodes, 1)
        self.edge_mlp_test = nn.Sequential(nn.Linear(2 * self.dim_node_features, 16), nn.ReLU(), nn.Linear(16, 1))
        self.edge_mlp = nn.Sequential(nn.Linear(2 * self.dim_node_features + self.dim_edge_features, 64), nn.ReLU(),
                                      nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 1))
        for seq in (self.edge_mlp, self.edge_mlp_test):       # dormant heads: U(-0.1, 0.1) weights, zero bias
            for m in seq:
                if isinstance(m, nn.Linear):
                    nn.init.uniform_(m.weight, -0.1, 0.1)
                    nn.init.constant_(m.bias, 0)
        self.to(device)

    @property
    def dist_matrix(self):
        """All-pairs free-flow shortest-path matrix, built on first access (the reference builds it eagerly with
        networkx in the constructor although the live forward never reads it)."""
        if self._dist_matrix is None:
            self.refresh_dijkstra(self.edge_index, self._free_flow)
        return self._dist_matrix

    def refresh_dijkstra(self, edge_index: torch.Tensor, free_flow_travel: torch.Tensor):
        """All-pairs free-flow distances (src/agents/mpnn_agent.py:53-79) by ``tarl_apsp`` on the device."""
        from tarl_hip import ops
        assert free_flow_travel.size(0) == edge_index.size(1) and edge_index.size(0) == 2
        plan = cached_plan(edge_index, self.num_nodes)
        w = free_flow_travel.detach().to(self.device, torch.float32)
        require_cuda(w, "free_flow_travel")
        self._dist_matrix = ops.all_pairs_shortest_paths(plan, w, want_next_hop=False, want_dist=True)[1][0]

    def resolve_prior_method(self) -> str:
        if self.prior_method not in self.PRIOR_METHODS:
            raise ValueError(f"prior_method must be one of {self.PRIOR_METHODS}, got {self.prior_method!r}")
        if self.prior_method != "auto":
            return self.prior_method
        return "all_pairs" if self.num_nodes <= ALL_PAIRS_MAX_NODES else "per_destination"

    def free_flow_weights(self) -> torch.Tensor:
        """The prior's edge weights: free-flow travel times, fp32 (E,) on the module's device."""
        w = self._free_flow.detach().to(self.device, torch.float32).reshape(-1).contiguous()
        require_cuda(w, "free_flow_travel")
        return w

    def prior_tables(self):
        """-> (table, dest_slot) the prior head reads: (``dist_matrix``, None) under all_pairs; else the (N, D) table over
        the destinations of ``agent_features`` and its column map (src.agents.base.destination_set), rebuilt when the agent
        table is replaced."""
        if self.resolve_prior_method() == "all_pairs":
            return self.dist_matrix, None
        if self.agent_features is None:
            raise RuntimeError("the per-destination prior needs agent_features (its destinations are the table's columns)")
        if self._prior_dest is None or self._prior_dest[2] is not self.agent_features:
            from tarl_hip import ops
            dests, slot = destination_set(self.agent_features.to(self.device), self.num_nodes)
            table = ops.prior_dest_table(cached_plan(self.edge_index, self.num_nodes), self.free_flow_weights(), dests)
            self._prior_dest = (table, slot, self.agent_features)
        return self._prior_dest[0], self._prior_dest[1]

    def compute_dijkstra_logits(self, agent_destination: torch.Tensor, time_travel: torch.Tensor) -> torch.Tensor:
        """Shortest-path prior (src/agents/mpnn_agent.py:81-113; dormant in the live forward):
        logits[e] = -dist[dst(e), destination[e]] - time_travel[e]; a destination vector of k * E entries is batched.
        Under per_destination every destination must have a column (be a DESTINATION of ``agent_features``)."""
        E = self.edge_index.size(1)
        rep = agent_destination.size(0) // E
        table, slot = self.prior_tables()
        head = self.edge_index[1].to(table.device).repeat(rep)
        col = agent_destination.to(head.device)
        if slot is not None:
            col = slot[col].long()
            if bool((col < 0).any()):
                raise ValueError("a destination without a per-destination column (not a DESTINATION of agent_features)")
        logits = -table[head, col] - time_travel
        return logits.view(rep, -1) if rep > 1 else logits.view(-1)

    def use_graph_transformer(self, pe: torch.Tensor):
        """Switch to the graph-transformer head: creates ``transformer`` (GraphTransformerNet(16, 1, 16, hidden 16, gate,
        2 layers, 4 heads, dropout 0.1), evaluation mode) and the positional-encoding buffer ``gt_pe`` (N, 16)."""
        from ..transformer import GraphTransformerNet
        if tuple(pe.shape) != (self.num_nodes, 16):
            raise ValueError(f"pe must be ({self.num_nodes}, 16)")
        self.policy_head = "graph_transformer"
        if getattr(self, "transformer", None) is None:
            self.transformer = GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4, dropout=0.1)
        self.register_buffer("gt_pe", pe.detach().to(torch.float32).contiguous())
        self.transformer.eval()
        self.to(self.device)
        return self

    def use_goal_mlp(self, time_scale: float):
        """Switch to the goal-conditioned head (NOT in the reference; csrc/goal_mlp.hip): creates ``goal_mlp`` (Linear(8, 16),
        ReLU, Linear(16, 1); U(-0.1, 0.1) weights, zero bias) on destination-relative features and the buffer ``goal_scale``
        (``time_scale``: the mean FREE_FLOW over the roads, ops.goal_time_scale). Both exist only after this call, so the
        other heads' state dicts do not change. The distances come from :meth:`prior_tables`."""
        s = float(time_scale)
        if not (0.0 < s < float("inf")):
            raise ValueError("time_scale must be finite and > 0")
        self.policy_head = "goal_mlp"
        if getattr(self, "goal_mlp", None) is None:
            self.goal_mlp = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 1))
            for m in self.goal_mlp:
                if isinstance(m, nn.Linear):
                    nn.init.uniform_(m.weight, -0.1, 0.1)
                    nn.init.constant_(m.bias, 0)
        self.register_buffer("goal_scale", torch.tensor(s, dtype=torch.float32))
        self.to(self.device)
        return self

    def forward(self, node_features: torch.Tensor, edge_features: torch.Tensor, agent_index: torch.Tensor):
        """node_features (N,7) or (B,N,7) -> logits (E,) or (B,E)."""
        require_cuda(node_features, "node_features")
        plan = cached_plan(self.edge_index, self.num_nodes)
        if self.policy_head == "goal_mlp":
            from tarl_hip import ops
            if getattr(self, "goal_mlp", None) is None:
                raise RuntimeError("policy_head 'goal_mlp' needs use_goal_mlp(time_scale) first")
            obs16 = ops.policy_obs16(node_features, agent_index, self.agent_features.to(node_features.device))
            table, slot = self.prior_tables()
            m = self.goal_mlp
            logits = _GoalMlp.apply(obs16, plan, table, slot, float(self.goal_scale), m[0].weight, m[0].bias, m[2].weight,
                                    m[2].bias)
            return logits if node_features.dim() == 3 else logits.view(-1)
        if self.policy_head == "graph_transformer":
            from tarl_hip import ops
            from .._compat import cached_edge_const
            ea = edge_features if edge_features.dim() <= 2 else edge_features[0]
            ec = cached_edge_const(ea.reshape(-1, 1), node_features.device)
            obs16 = ops.policy_obs16(node_features, agent_index, self.agent_features.to(node_features.device))
            logits = self.transformer.edge_logits(obs16, plan, ec, self.gt_pe)
            return logits if node_features.dim() == 3 else logits.view(-1)
        if self.policy_head == "embedding_dijkstra":
            from tarl_hip import ops
            obs16 = ops.policy_obs16(node_features, agent_index, self.agent_features.to(node_features.device))
            table, slot = self.prior_tables()
            logits = _PriorLogits.apply(self.nodes_embedding.weight, obs16, plan, table, float(self.prior_weight), slot)
            return logits if node_features.dim() == 3 else logits.view(-1)
        if self.policy_head != "embedding":
            from tarl_hip import ops
            from .._compat import cached_edge_const
            ea = edge_features if edge_features.dim() <= 2 else edge_features[0]     # static: the same for every sample
            ec = cached_edge_const(ea.reshape(-1, 1), node_features.device)
            obs16 = ops.policy_obs16(node_features, agent_index, self.agent_features.to(node_features.device))
            m = self.edge_mlp
            logits = _EdgeMlp.apply(obs16, plan, ec, self.policy_head == "edge_mlp_bf16", m[0].weight, m[0].bias,
                                    m[2].weight, m[2].bias, m[4].weight, m[4].bias)
            return logits if node_features.dim() == 3 else logits.view(-1)
        return _EdgeLogits.apply(self.nodes_embedding.weight, node_features, plan)

    def update_edges(self, x, edge_index, edge_attr=None):
        plan = cached_plan(edge_index, x.size(0))
        return _EdgeLogits.apply(self.nodes_embedding.weight, x[:, :7], plan).view(-1, 1)


class _CriticMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, counts, time_rows, w1, b1, w2, b2, w3, b3):
        from tarl_hip import ops
        cw = ops.CriticWeights(w1.detach().contiguous(), b1.detach().contiguous(), w2.detach().contiguous(),
                               b2.detach().contiguous(), w3.detach().reshape(-1).contiguous(), b3.detach().contiguous())
        value, h1, h2 = ops.critic_forward(cw, counts, time_rows, 1, keep_hidden=True)
        ctx.cw, ctx.saved = cw, (counts, time_rows, h1, h2)
        ctx.w3_shape = w3.shape
        return value

    @staticmethod
    def backward(ctx, grad_value):
        from tarl_hip import ops
        counts, time_rows, h1, h2 = ctx.saved
        cw = ctx.cw
        grads = [torch.zeros_like(t) for t in (cw.w1, cw.b1, cw.w2, cw.b2, cw.w3, cw.b3)]
        ops.critic_backward(cw, counts, time_rows, 1, h1, h2, grad_value.contiguous(), grads)
        return None, None, grads[0], grads[1], grads[2], grads[3], grads[4].view(ctx.w3_shape), grads[5]


class _ValueMPNN(torch.autograd.Function):
    """MPNNValueNet forward / backward on the HIP kernels (tarl_value_mpnn_{fwd,bwd}); gradients for the 12 parameters."""

    @staticmethod
    def forward(ctx, plan, nf, ar, ef, tm, *params):
        from tarl_hip import ops
        value, act, agg = ops.value_mpnn_forward(plan, nf, ar, ef, tm, params, keep=True)
        ctx.plan, ctx.saved, ctx.params = plan, (nf, ar, ef, tm, act, agg), params
        return value

    @staticmethod
    def backward(ctx, grad_value):
        from tarl_hip import ops
        nf, ar, ef, tm, act, agg = ctx.saved
        grads = ops.value_mpnn_backward(ctx.plan, nf, ar, ef, tm, ctx.params, grad_value.contiguous(), act, agg)
        return (None, None, None, None, None) + tuple(g.view_as(p) for g, p in zip(grads, ctx.params))


class MPNNValueNet(MessagePassingBase, Agents):
    """The message-passing critic of the reference (src/agents/mpnn_agent.py:265-402; never instantiated by its runner):
    per-edge message tanh(Linear(17,1)), mean over a road's out-edges, tanh(Linear(1,1)), a 1-32-32-1 time MLP and a
    final Linear(N+1, 1). Same module tree / state-dict keys. The Dropout(0.05) layers are kept in the tree but the
    kernels implement evaluation-mode semantics (identity); ``forward`` refuses training-mode dropout explicitly."""

    def __init__(self, edge_index, num_nodes, device):
        Agents.__init__(self, device=device)
        MessagePassingBase.__init__(self, aggr="mean", flow="target_to_source")
        self.edge_index = edge_index
        self.num_nodes = num_nodes
        self.num_edges = edge_index.size(1)
        self.dim_nodes_features = 16
        self.dim_edges_features = 1
        self.message_mlp = nn.Sequential(nn.Dropout(0.05), nn.Linear(17, 1), nn.Tanh())
        self.node_mlp = nn.Sequential(nn.Linear(1, 1), nn.Tanh())
        self.final_mlp = nn.Sequential(nn.Linear(num_nodes + 1, 1))
        self.time_net = nn.Sequential(nn.Linear(1, 32), nn.Dropout(0.05), nn.ReLU(), nn.Linear(32, 32), nn.Dropout(0.05),
                                      nn.ReLU(), nn.Linear(32, 1))
        self.to(device)

    def _params(self):
        m, n, f, t = self.message_mlp[1], self.node_mlp[0], self.final_mlp[0], self.time_net
        return (m.weight, m.bias, n.weight, n.bias, f.weight, f.bias, t[0].weight, t[0].bias, t[3].weight, t[3].bias,
                t[6].weight, t[6].bias)

    def forward(self, node_features, edge_features, agent_index, time):
        """node_features (N,7) or (B,N,7); edge_features (E,1) or (B,E,1); agent_index (N,) or (B,N); time (1,) or
        (B,1) -> (1,) or (B,1)."""
        require_cuda(node_features, "node_features")
        if self.training:
            raise RuntimeError("MPNNValueNet runs with evaluation-mode dropout only: call .eval() (the kernels implement "
                               "Dropout as the identity)")
        batched = node_features.dim() == 3
        nf = node_features.reshape(-1, self.num_nodes, node_features.size(-1)).to(torch.float32).contiguous()
        M = nf.size(0)
        ar = None
        if self.agent_features is not None:
            ar = self.agent_features[agent_index.reshape(M, self.num_nodes).long()].to(torch.float32).contiguous()
        ef = edge_features.reshape(-1, self.num_edges).to(torch.float32).contiguous()
        tm = time.reshape(-1).to(torch.float32).contiguous()
        plan = cached_plan(self.edge_index, self.num_nodes)
        v = _ValueMPNN.apply(plan, nf, ar, ef, tm, *self._params())
        return v.view(M, 1) if batched else v.view(1)


class MPNNValueNetSimple(MessagePassingBase, Agents):
    """Critic actually used by the runner: ``final_mlp`` = Linear(N+1,64)-ReLU-Linear(64,64)-ReLU-Linear(64,1)."""

    def __init__(self, edge_index, num_nodes, device):
        Agents.__init__(self, device=device)
        MessagePassingBase.__init__(self, aggr="mean", flow="target_to_source")
        self.edge_index = edge_index
        self.num_nodes = num_nodes
        self.num_edges = edge_index.size(1)
        self.dim_nodes_features = 16
        self.dim_edges_features = 1
        self.final_mlp = nn.Sequential(nn.Linear(num_nodes + 1, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(),
                                       nn.Linear(64, 1))
        self.to(device)

    def forward(self, node_features, edge_features, agent_index, time):
        """node_features (...,N,7), time (...,1) -> (...,1)."""
        require_cuda(node_features, "node_features")
        lead = node_features.shape[:-2]
        counts = node_features[..., 1].reshape(-1, self.num_nodes).contiguous()
        time_rows = time.reshape(-1).to(torch.float32).contiguous()
        l0, l2, l4 = self.final_mlp[0], self.final_mlp[2], self.final_mlp[4]
        v = _CriticMLP.apply(counts, time_rows, l0.weight, l0.bias, l2.weight, l2.bias, l4.weight, l4.bias)
        return v.view(*lead, 1)
