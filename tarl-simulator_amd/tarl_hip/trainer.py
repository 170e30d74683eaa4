"""VecPPOTrainer — the reference's ``ppo_train`` loop (src/rl/ppo_trainer.py:21-39,129-145) on B vectorised
environments per GPU, every arithmetic step a HIP kernel behind the C ABI:

  HOT LOOP A (T frames): policy logits -> GraphDistribution softmax / sample / log_prob -> env step
  HOT LOOP B (num_epochs): critic over all frames (MFMA) -> GAE -> advantage normalisation (global statistics) ->
                           minibatch of ``sub_batch_size`` frames -> clipped PPO loss fwd+bwd -> one gradient
                           all-reduce (RCCL) -> fused Adam.

Semantics kept from the reference: ONE collector batch per call (``total_frames == frames_per_batch``), the
environment is reset at the start of the batch (``reset_at_each_iter=True``), GAE is recomputed every epoch with the
current critic, one minibatch + one Adam step per epoch, loss = objective + critic + entropy, no gradient clipping.
Multi-GPU: one process per GPU, each with its own environments and minibatch; gradients are averaged.
"""
from __future__ import annotations

import math
import os
from bisect import bisect_left

import numpy as np
import torch

from . import dist_utils, ops
from .engine import EPISODE_END
from .flatparams import FlatParams


class StageTimer:
    """HIP-event timing of the update's stages (``bench.py``'s ``update_path`` object): a pair of events on the launch
    stream (torch's current stream — the stream every ``ops`` call enqueues on) around each stage; ``ms()`` synchronises
    and returns {stage: (summed ms, calls)}."""

    def __init__(self):
        self.ev = {}

    class _Span:
        def __init__(self, timer, name):
            self.t, self.name = timer, name

        def __enter__(self):
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

        def __exit__(self, *exc):
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.t.ev.setdefault(self.name, []).append((self.a, b))

    def __call__(self, name):
        return StageTimer._Span(self, name)

    def ms(self):
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in self.ev.items()}


class NoStageTimer:
    def __call__(self, name):
        return self

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_POINT_AFTER_THE_DRAW = ("draw the actions of all frames ahead of the frames, so there is no point between a frame's draw "
                            "and its Direction launch where the rule could read that frame's state")


def _not_for_embedding(what, why):
    """The refusal of an option that needs the shared loop of the state-dependent heads."""
    return (f"{what} is not available for policy='embedding': its rollouts (tarl_fused_rollout, tarl_rollout_env) {why}; "
            "use a state-dependent head (edge_mlp, embedding_dijkstra, graph_transformer, goal_mlp)")


class VecPPOTrainer:
    def __init__(self, engine, emb_param, critic_params, *, rollout_steps, num_epochs=1, sub_batch_size=32, lr=1e-3,
                 gamma=0.99, lmbda=0.95, clip_epsilon=0.2, entropy_coef=0.01, critic_coef=1.0, temperature=1.0,
                 extra_params=(), seed=0, lazy_log_prob=False, rank_offset=True, rollout=None, metrics_envs=1,
                 policy="embedding", edge_mlp_params=None, policy_bf16=False, policy_precision=None, prior_table=None,
                 prior_weight=1.0, gt_params=None, gt_pe=None, value="simple", gt_value_params=None, gt_value_pe=None,
                 prior_free_flow=None, prior_dests=None, policy_hold=False, goal_mlp_params=None,
                 route_departures=False, reward="queue", credit="joint", decision_gamma=1.0, credit_baseline="free_flow",
                 decision_critic_params=None, decision_critic_coef=1.0, decision_delay_scale=16.0, credit_scope="headed",
                 credit_horizon="charge"):
        """``emb_param``: nn.Parameter (num_nodes, 1) — MPNNPolicyNet.nodes_embedding.weight;
        ``critic_params``: [w1 (64,N+1), b1, w2 (64,64), b2, w3 (1,64), b3] — MPNNValueNetSimple.final_mlp.{0,2,4};
        ``extra_params``: further actor/critic parameters that never receive gradient on the live path (the dormant
        edge MLPs) — they sit in the flat buffer so that the optimiser covers ``loss_module.parameters()`` like the
        reference's does.
        ``value``: "simple" = MPNNValueNetSimple over the count bytes and the clock (``critic_params`` as above);
        "graph_transformer" = ValueNet (src/agents/transformer_agent.py, csrc/gt_value.hip) on the policy's observation:
        ``critic_params`` = every parameter of its GraphTransformerNet, ``gt_value_params`` maps the state-dict keys of
        ops.GT_VALUE_PARAM_KEYS + GT_VALUE_BUFFER_KEYS to its tensors, ``gt_value_pe`` (N, 16) is its positional encoding.
        It needs a state-dependent policy head (the rollout builds the observation of every frame) and keeps all (T + 1) * B
        observations (``obs_all``, fp32 (T+1, B, N, 16)) for GAE's all-frames critic pass.
        ``policy_hold`` (an action shield of the ENVIRONMENT, not in the reference): in every collected frame a
        row with a non-empty FIFO whose drawn road is its head agent's destination selects itself instead, between the draw
        and the frame (ops.fused_set_policy_hold). ``collect()`` stores the draw's bytes and log-prob, so the update is
        unchanged; ``held`` (B,) int32 counts the held rows of the last ``collect()``. State-dependent heads only.
        ``route_departures`` (an environment-side rule, not in the reference): in every collected frame an EMPTY
        road with an agent ready to depart from it selects that agent's first hop, looked up in a free-flow per-destination
        table built once after the first reset (ops.fused_set_departure_router), after the optional hold launch. The stored
        action and log-prob are the draw's; ``departures_routed`` (B,) int32 counts the rows written by the last
        ``collect()``. State-dependent heads only.
        ``reward``: ``"queue"`` (the default) is the reference's -sum of the FIFO counts after the frame;
        ``"trip"`` (an environment-side rule, not in the reference) is -(agents on the way + waiting agents that are due),
        so that a lost agent and a blocked departure keep costing until the horizon: ``collect()`` sets the switch of the
        shared rollout loop (ops.fused_set_trip_reward) and ``self.reward`` then holds the trip reward; GAE, the critic and
        the update read it as before. State-dependent heads on the fused path only.
        ``credit``: ``"joint"`` (the default) is the reference's update, one ratio and one advantage per (frame,
        environment); ``"decision"`` (not in the reference) credits every road's categorical with the delay of the traveller
        at the head of its FIFO beyond free flow: ``collect()`` captures the heads of the kept rows (ops.fused_set_head_capture)
        and takes their raw advantages per segment (ops.decision_advantage), ``minibatch_step`` replaces the joint policy term
        by ops.graphdist_decision_ppo; critic and entropy terms are unchanged. ``decision_gamma``: the discount of a
        traveller's frames to go, separate from GAE's ``gamma``. State-dependent heads on the fused path with the default
        critic only. ``self.last["decision"]`` then carries the live decisions, their mean delay in frames, the truncated
        share, the objective, the clip fraction and the approximate KL of the last minibatch (0-d device tensors).
        ``credit_scope`` / ``credit_horizon`` (``credit="decision"`` only, both combine with the learned baseline):
        ``"due"`` credits only the roads whose head is due at the frame's clock (the draw of a road whose head is still
        travelling reaches nobody; ops.fused_set_head_capture(scope="due")); ``"bootstrap"`` continues a traveller still under
        way when a segment is cut by the batch in free flow from the road it is queued on (ops.fused_agent_roads, once per
        segment) instead of charging it the frames to the horizon; a segment that ends with the episode keeps the charge.
        ``self.last["decision"]`` then gains ``credit_scope`` / ``decisions_headed`` and ``credit_horizon`` / ``bootstrapped``.
        ``credit_baseline`` (``credit="decision"`` only): ``"free_flow"`` (the default) is the baseline above;
        ``"learned"`` (not in the reference) adds a per-decision critic (csrc/decision_critic.hip) on the state in front of
        the decision: ``decision_critic_params`` = [w1 (16, 8), b1 (16,), w2 (1, 16), b2 (1,)], consecutive in
        ``extra_params`` like ``goal_mlp_params`` (ops.decision_critic_init makes them). Once per update it is evaluated on
        all kept rows with the rollout's parameters and the policy term reads ``adv_raw + decision_delay_scale * value``;
        every minibatch step adds the gradient of ``decision_critic_coef`` times its smooth-L1 loss against
        ``-adv_raw / decision_delay_scale`` (stage ``decision_critic``). ``self.last["decision"]`` gains ``critic_loss``,
        ``explained_variance`` and ``value_mean`` of the last epoch."""
        self.eng = engine
        # policy: "embedding" = the reference's live head (logit = embedding of the target road: state-independent, its
        # distribution is tabulated once per update); "edge_mlp" = the per-edge MLP head it carries as parameters
        # (src/agents/mpnn_agent.py:35-41,227-231): state-DEPENDENT, so every frame evaluates observation -> MLP (MFMA) ->
        # segment softmax -> sample -> log-prob before the simulation step. ``edge_mlp_params`` = [w1, b1, w2, b2, w3, b3]
        # (edge_mlp.{0,2,4}.{weight,bias}; they must also be in ``extra_params`` so that they live in the flat buffer);
        # ``policy_bf16``: rollout logits on the bf16 MFMA path (the update always runs in fp32). ``policy_precision``
        # ("fp32" | "bf16" | "x3") names the rollout kernel outright; the default for a non-bf16 policy is "x3": logits
        # within a few fp32 ulp of the fp32 MFMA kernel's (the north star's 1e-4 contract) at 2.7x its matrix rate.
        # "embedding_dijkstra" = the embedding plus ``prior_weight`` times the shortest-path prior of the reference
        # (src/agents/mpnn_agent.py:180-190, csrc/prior.hip): state-DEPENDENT like the MLP head, but without parameters of
        # its own; ``prior_table`` (N, N) = MPNNPolicyNet.dist_matrix. Gradients reach the embedding alone. Per-destination
        # prior instead (MPNNPolicyNet.prior_method): no ``prior_table``, but ``prior_free_flow`` (E,) fp32 free-flow
        # weights and ``prior_dests`` = (dests, dest_slot) of src.agents.base.destination_set over the agent tables of all B
        # environments; the trainer builds the (N, D) table (ops.prior_dest_table) after checking that it fits.
        # "graph_transformer" = the reference's GraphTransformerNet edge output (csrc/gt_policy.hip), evaluation-mode
        # BatchNorm: ``gt_params`` maps the state-dict keys of ops.GT_PARAM_KEYS + GT_BUFFER_KEYS to the module's tensors
        # (the parameters must also be in ``extra_params``), ``gt_pe`` (N, 16) is its positional encoding.
        # "goal_mlp" = the goal-conditioned MLP on destination-relative features (csrc/goal_mlp.hip; not in the reference):
        # state-DEPENDENT, trainable; ``goal_mlp_params`` = [w1, b1, w2, b2] (goal_mlp.{0,2}.{weight,bias}), consecutive in
        # ``extra_params`` so that they are ONE run of 161 floats of the flat buffer; the distances come from the prior head's
        # arguments (``prior_table``, or ``prior_free_flow`` + ``prior_dests``), the time scale from the engine's roads.
        self.policy = policy
        self.prior_table = prior_table
        self.prior_dest_slot = None
        self.prior_weight = float(prior_weight)
        self.policy_precision = policy_precision or ("bf16" if policy_bf16 else "x3")
        if self.policy_precision not in ops.EDGE_MLP_PRECISIONS:
            raise ValueError(f"policy_precision must be one of {ops.EDGE_MLP_PRECISIONS}")
        self.policy_bf16 = self.policy_precision == "bf16"
        self.edge_mlp_params = list(edge_mlp_params) if edge_mlp_params is not None else None
        if policy == "edge_mlp":
            if engine.fs is None or self.edge_mlp_params is None or len(self.edge_mlp_params) != 6:
                raise ValueError("policy='edge_mlp' needs the fused engine and the six edge_mlp parameter tensors")
            ids = {id(p) for p in extra_params}
            if not all(id(p) in ids for p in self.edge_mlp_params):
                raise ValueError("edge_mlp_params must be part of extra_params (the optimiser's flat buffer)")
        elif policy in ("embedding_dijkstra", "goal_mlp"):
            if policy == "goal_mlp":
                needs = ("policy='goal_mlp' needs the fused engine and goal_mlp_params = the four tensors "
                         "goal_mlp.{0,2}.{weight,bias} (8 -> 16 -> 1)")
                if engine.fs is None:
                    raise ValueError(needs)
                self._mlp8_params("goal_mlp_params", goal_mlp_params, extra_params, needs)
            if engine.fs is not None and prior_table is None and prior_free_flow is not None and prior_dests is not None:
                self.prior_table, self.prior_dest_slot = self._build_prior_dest(engine, prior_free_flow, *prior_dests)
            elif engine.fs is None or prior_table is None:
                raise ValueError(f"policy={policy!r} needs the fused engine and the (N, N) prior_table, or "
                                 "prior_free_flow and prior_dests for the per-destination table")
            elif tuple(prior_table.shape) != (engine.N, engine.N):
                raise ValueError(f"prior_table must be ({engine.N}, {engine.N})")
        elif policy == "graph_transformer":
            if engine.fs is None or gt_params is None or gt_pe is None:
                raise ValueError("policy='graph_transformer' needs the fused engine, gt_params and the (N, 16) gt_pe")
            ids = {id(p) for p in extra_params}
            if not all(id(gt_params[k]) in ids for k in ops.GT_PARAM_KEYS):
                raise ValueError("the graph-transformer parameters must be part of extra_params (the optimiser's flat buffer)")
            # the backward keeps every node's and edge's activations of the minibatch (~2 KB per node and per edge and
            # sample): refuse a sub-batch it cannot take here rather than inside the library
            m = min(int(sub_batch_size), int(rollout_steps) * engine.B)
            need, cap = ops.gt_bwd_scratch_bytes(engine.plan, m), ops.gt_bwd_max_samples(engine.plan)
            free = torch.cuda.mem_get_info(engine.device)[0]
            if m > cap or need > free // 2:
                raise ValueError(f"sub_batch_size {m} is too large for the graph-transformer backward on this graph: it "
                                 f"takes at most {cap} samples and needs {need / 2**20:.0f} MiB of scratch "
                                 f"({free / 2**20:.0f} MiB free); use a smaller sub_batch_size")
        elif policy != "embedding":
            raise ValueError("policy must be 'embedding', 'edge_mlp', 'embedding_dijkstra', 'graph_transformer' or 'goal_mlp'")
        self.gt_params = dict(gt_params) if gt_params is not None else None
        self.gt_pe = gt_pe
        self.value = value
        self.gt_value_params = dict(gt_value_params) if gt_value_params is not None else None
        self.gt_value_pe = gt_value_pe
        if value == "graph_transformer":
            self._check_gt_value(engine, policy, critic_params, extra_params, rollout_steps, sub_batch_size)
        elif value != "simple":
            raise ValueError("value must be 'simple' or 'graph_transformer'")
        # the state-dependent heads evaluate their logits in front of every frame and draw the minibatch frames up front
        self.state_dep = policy != "embedding"
        self.policy_hold = bool(policy_hold)
        if self.policy_hold and not self.state_dep:
            raise ValueError(_not_for_embedding("policy_hold", _NO_POINT_AFTER_THE_DRAW))
        self.held = torch.zeros(engine.B, dtype=torch.int32, device=engine.device) if self.policy_hold else None
        self.route_departures = bool(route_departures)
        if self.route_departures and not self.state_dep:
            raise ValueError(_not_for_embedding("route_departures", _NO_POINT_AFTER_THE_DRAW))
        self.departures_routed = self._departure_router = None
        if self.route_departures:
            if engine.fs is None:
                raise ops._lib.TarlError("route_departures needs the fused engine (ops.fused_path_supported): the packed state "
                                     "cannot represent this graph and there is no fall-back")
            from .evaluator import router_buffers
            self.departures_routed = torch.zeros(engine.B, dtype=torch.int32, device=engine.device)
            self._departure_router = router_buffers(engine, None, 1) + (
                torch.empty((engine.N, engine.B), dtype=torch.int32, device=engine.device),)
            self._departure_table_built = False
        if reward not in ("queue", "trip"):
            raise ValueError("reward must be 'queue' or 'trip'")
        self.reward_kind = reward
        if reward == "trip" and not self.state_dep:
            raise ValueError(_not_for_embedding(
                "reward='trip'", "do not go through the shared loop of the state-dependent heads, where the trip launch "
                                 "follows every frame's insert"))
        if reward == "trip" and engine.fs is None:
            raise ops._lib.TarlError("reward='trip' needs the fused engine (ops.fused_path_supported): the packed state "
                                     "cannot represent this graph and there is no fall-back")
        if credit not in ("joint", "decision"):
            raise ValueError("credit must be 'joint' or 'decision'")
        self.credit = credit
        self.decision_gamma = float(decision_gamma)
        if credit == "decision":
            self._check_decision_credit(engine, value)
        self._check_credit_scope(credit, credit_scope, credit_horizon)
        self.credit_scope, self.credit_horizon = credit_scope, credit_horizon
        if credit_scope == "due":           # {headed, due} over the kept rows of one collect()
            self.decision_counts = torch.zeros(2, dtype=torch.int32, device=engine.device)
        if credit_horizon == "bootstrap":   # where every agent stands when a segment ends; the decisions continued from there
            self.agent_road = torch.empty((engine.B, engine.A), dtype=torch.int32, device=engine.device)
            self.decision_bootstrapped = torch.zeros(1, dtype=torch.int32, device=engine.device)
        if credit_baseline not in ("free_flow", "learned"):
            raise ValueError("credit_baseline must be 'free_flow' or 'learned'")
        self.credit_baseline = credit_baseline
        self.decision_critic_coef = float(decision_critic_coef)
        self.decision_delay_scale = float(decision_delay_scale)
        self.decision_critic_params = None
        if credit_baseline == "learned":
            self.decision_critic_params = self._check_decision_critic(credit, decision_critic_params, extra_params)
        # lazy_log_prob: do not produce sample_log_prob for every collected frame (as the reference's collector does)
        # but only, exactly, for the frames a minibatch actually reads. Same training result; off by default so that a
        # frame does everything the reference's frame does.
        self.lazy_log_prob = bool(lazy_log_prob)
        if self.lazy_log_prob and self.state_dep:
            raise ValueError("lazy_log_prob re-evaluates the state-independent embedding head only")
        self.T = int(rollout_steps)
        self.num_epochs = int(num_epochs)
        self.M = int(sub_batch_size)
        self.lr, self.gamma, self.lmbda = lr, gamma, lmbda
        self.clip_epsilon, self.entropy_coef, self.critic_coef, self.temperature = clip_epsilon, entropy_coef, critic_coef, temperature
        self.rank, self.world = dist_utils.world()
        self.emb_param = emb_param
        self.critic_params = list(critic_params)
        self.flat = FlatParams([emb_param] + self.critic_params + list(extra_params), device=engine.device)
        # replicas start identical: rank 0's initial weights win
        dist_utils.broadcast_(self.flat.flat, src=0)
        self.goal_mlp_params = list(goal_mlp_params) if policy == "goal_mlp" else None
        if policy == "goal_mlp":      # one run of the flat buffer, in the kernels' order; the time scale of the engine's roads
            self._goal_off = self._mlp8_offset(self.goal_mlp_params)
            self.goal_scale = ops.goal_time_scale(engine._x[0, :, 3 * engine.Nmax:])
        if self.decision_critic_params is not None:      # one run of the flat buffer, as the goal head's
            self._dcritic_off = self._mlp8_offset(self.decision_critic_params)
            self.frames_left = self.adv_dec = None
        B, N, dev = engine.B, engine.N, engine.device
        # which rollout kernel family: "env" = one workgroup per environment, records in LDS, one launch for all frames
        # (tarl_rollout_env; env-major buffers), "frames" = four env-minor launches per frame (tarl_fused_rollout).
        # Default (TARL_ROLLOUT or "auto"): "env" when the graph fits a CU's LDS AND B * N <= 800k (node, environment)
        # pairs — measured crossover on MI355X: N = 256: env 2.1x at B = 1, 2.7x at B = 256, 1.5x at B = 2048, tie at
        # 8192; N = 1024, B = 1024: frames 1.24x; N = 2500: env +19 % at B = 256, frames +13 % at B = 512. One environment
        # keeps one CU busy for the whole frame; the four-launch path spreads the same work over the chip but needs
        # enough environments to fill its lanes and hide four dependent launches.
        mode = rollout or os.environ.get("TARL_ROLLOUT", "auto")
        if engine.fs is None:
            mode = "unfused"
        elif self.state_dep:    # per-frame policy evaluation in front of the four-launch frame
            mode = {"edge_mlp": "frames+policy", "graph_transformer": "frames+gt", "goal_mlp": "frames+goal"}.get(
                policy, "frames+prior")
        elif mode == "auto":
            mode = "env" if (engine.env_rollout_supported and engine.B * engine.N <= 800_000) else "frames"
        elif mode == "env" and not engine.env_rollout_supported:
            raise ValueError("rollout='env' needs a graph whose hot records fit the LDS (tarl_rollout_env_supported)")
        self.rollout = mode
        self.layout_tag = ops.FUSED_LAYOUT
        # rollout buffers, written directly by the kernels: ENV-MINOR ([frame][node][env]) for the "frames" family
        self.env_minor = mode.startswith("frames")
        shp = (lambda t: (t, N, B)) if self.env_minor else (lambda t: (t, B, N))
        # fused rollouts write one BYTE per (frame, node, env): the count and the rank of the chosen out-edge
        byte = mode != "unfused"
        self.counts = torch.zeros(shp(self.T + 1), dtype=torch.uint8 if byte else torch.float32, device=dev)
        # state-dependent heads: the per-frame sampler (one workgroup per environment) writes its rank bytes env-major
        self.choice = torch.zeros((self.T, B, N) if self.state_dep else shp(self.T),
                                  dtype=torch.uint8 if byte else torch.int32, device=dev)
        # per-step logs of SimulatorEnv._step, accumulated on the device by the rollout kernels: the leg histogram's
        # (departed, arrived) per frame for every environment, delta_travel_time / pop + withdraw masks per node for the
        # first ``metrics_envs`` environments (the reference logs them for its single environment)
        self.metrics_envs = min(int(metrics_envs), B) if byte else 0
        m = self.metrics_envs
        self.leg = torch.zeros((self.T, B, 2), dtype=torch.int32, device=dev) if byte else None
        self.dtt_node = torch.zeros(shp(self.T)[:1] + ((N, m) if self.env_minor else (m, N)), dtype=torch.float32,
                                    device=dev) if m else None
        self.events = torch.zeros_like(self.dtt_node, dtype=torch.uint8) if m else None
        self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory() if byte else None
        self._flag_event = None
        self.logp = torch.zeros((self.T, B), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((self.T, B), dtype=torch.float32, device=dev)
        self.times = torch.zeros(self.T + 1, dtype=torch.float32, device=dev)
        self.values = torch.zeros((self.T + 1, B), dtype=torch.float32, device=dev)
        # graph-transformer critic: the observation of every frame 0..T of every environment (frames 0..T-1 written by the
        # rollout's keep path, frame T from the final state), and one forward / one backward scratch reused across calls
        self.obs_all = (torch.empty((self.T + 1, B, N, 16), dtype=torch.float32, device=dev)
                        if value == "graph_transformer" else None)
        # every rank draws its own minibatches / action noise; rank_offset=False (test hook) makes replicas identical
        off = self.rank if rank_offset else 0
        # minibatch draw: M distinct frames out of T * B (the reference's SamplerWithoutReplacement hands out sub-batches of a
        # shuffled buffer). Drawn on the HOST in O(M) (numpy's Floyd sampler) and copied behind the launches already queued:
        # a device randperm of T * B = 4.2 M keys is seven radix-sort passes + key generation per optimiser step (0.3 ms and a
        # dozen launches per iteration in profiles/r03_default_kernel_stats.csv) for 32 indices
        self.np_rng = np.random.Generator(np.random.Philox(key=int(seed) + 7919 * off))
        self.seed = int(seed) + off
        self.sample_counter = 0
        self.last = {}
        self.done_frames = torch.zeros(self.T, dtype=torch.bool)
        self.done_mask = None
        self.obs_idx = None
        self.stage = NoStageTimer()          # bench.py swaps in a StageTimer for its update_path object

    def _check_decision_credit(self, engine, value):
        """Refusals of credit="decision", each naming its limit; its counters and the slot of the distance table."""
        if not self.state_dep:
            raise ValueError(_not_for_embedding(
                "credit='decision'", "draw the actions of all frames ahead of the frames, so there is no point in front of a "
                                     "frame's draw where the heads of that frame's state could be captured"))
        if engine.fs is None:
            raise ops._lib.TarlError("credit='decision' needs the fused engine (ops.fused_path_supported): the packed state "
                                     "cannot represent this graph and there is no fall-back")
        if value == "graph_transformer":
            raise ValueError("credit='decision' is not available for value='graph_transformer': its observation store keeps "
                             "every one of the T * B frames, and per-decision buffers for T * B rows are out of scope; use "
                             "the default critic (value='simple')")
        if not 0.0 < self.decision_gamma <= 1.0:
            raise ValueError("decision_gamma must be in (0, 1]")
        dev = engine.device
        self.decision_truncated = torch.zeros(1, dtype=torch.int32, device=dev)
        self.decision_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bad_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._decision_dist = None          # (dist float64 (D, N), dest_slot int32 (N,)): built once, after the first reset
        self.head_keep = self.adv_raw = self.lp_old_node = None

    @staticmethod
    def _check_credit_scope(credit, credit_scope, credit_horizon):
        """Refusals of credit_scope / credit_horizon."""
        if credit_scope not in ("headed", "due"):
            raise ValueError("credit_scope must be 'headed' or 'due'")
        if credit_horizon not in ("charge", "bootstrap"):
            raise ValueError("credit_horizon must be 'charge' or 'bootstrap'")
        if credit_scope != "headed" and credit != "decision":
            raise ValueError("credit_scope narrows the per-decision credit: it needs credit decision")
        if credit_horizon != "charge" and credit != "decision":
            raise ValueError("credit_horizon closes the per-decision return: it needs credit decision")

    def _check_decision_critic(self, credit, params, extra_params):
        """Refusals of credit_baseline="learned" -> the four parameter tensors."""
        if credit != "decision":
            raise ValueError("credit_baseline='learned' is the baseline of the per-decision advantage: it needs "
                             "credit='decision'")
        cp = self._mlp8_params("decision_critic_params", params, extra_params,
                               "credit_baseline='learned' needs decision_critic_params = the four tensors w1 (16, 8), b1 (16,), "
                               "w2 (1, 16), b2 (1,) (8 -> 16 -> 1)")
        if not self.decision_critic_coef >= 0.0 or not math.isfinite(self.decision_critic_coef):
            raise ValueError("decision_critic_coef must be finite and >= 0")
        if not (math.isfinite(self.decision_delay_scale) and self.decision_delay_scale > 0.0):
            raise ValueError("decision_delay_scale must be positive and finite")
        return cp

    @staticmethod
    def _mlp8_params(name, params, extra_params, needs):
        """The four tensors of an 8 -> 16 -> 1 network (the goal head, the decision critic) -> their list; refused (``needs``)
        unless they are w1 (16, 8), b1 (16,), w2 (1, 16), b2 (1,) and one consecutive run of ``extra_params``, so that the
        kernels read them as ONE run of the flat buffer."""
        ps = list(params) if params is not None else []
        if [tuple(p.shape) for p in ps] != [(16, 8), (16,), (1, 16), (1,)]:
            raise ValueError(needs)
        pos = {id(p): i for i, p in enumerate(extra_params)}
        at = [pos.get(id(p), -9) for p in ps]
        if at[0] < 0 or at != list(range(at[0], at[0] + 4)):
            raise ValueError(f"{name} must be part of extra_params (the optimiser's flat buffer), in order and "
                             "next to each other")
        return ps

    def _mlp8_offset(self, params):
        """Where the run of :meth:`_mlp8_params` starts in the flat buffer."""
        off = self.flat.offsets[id(params[0])][0]
        assert self.flat.offsets[id(params[3])][0] == off + ops.GOAL_MLP_PARAMS - 1
        return off

    def _mlp8_view(self, buf, off):
        """The network's 161 floats of ``buf`` (``flat.flat`` or ``flat.grad``) in the kernels' order: one layout for the
        goal head and the decision critic (csrc/mlp8.h)."""
        assert ops.GOAL_MLP_PARAMS == ops.DECISION_CRITIC_PARAMS
        return buf[off:off + ops.GOAL_MLP_PARAMS]

    def _dcritic(self):
        return ops.DecisionCriticWeights(flat=self._mlp8_view(self.flat.flat, self._dcritic_off))

    def _build_decision_dist(self):
        """Free-flow shortest-path distances to every distinct destination (ops.destination_trees on the travel times of the
        empty network, as the departure router and the path trace build theirs): the baseline of the per-decision return."""
        eng = self.eng
        N, dev = eng.N, eng.device
        d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))      # src.agents.base.destination_set's rule
        d = d[(d >= 0) & (d < N)].contiguous()
        if d.numel() == 0:
            raise ValueError("credit='decision': no agent has a destination in range")
        free = int(torch.cuda.mem_get_info(dev)[0])
        if 8 * d.numel() * N > free // 2:
            raise ValueError(f"credit='decision': the free-flow distance table ({8 * d.numel() * N / 2**30:.2f} GiB for D = "
                             f"{d.numel()} destinations x N = {N} roads) exceeds half the free device memory "
                             f"({free / 2**30:.2f} GiB free)")
        slot = torch.full((N,), -1, dtype=torch.int32, device=dev)
        slot[d] = torch.arange(d.numel(), dtype=torch.int32, device=dev)
        w = ops.fused_edge_travel_time(eng.plan, eng.fs)[0].contiguous()      # after the reset every count is 0: free flow
        _, dist = ops.destination_trees(eng.plan, w, d, want_next_hop=False, want_dist=True)
        self._decision_dist = (dist, slot)

    GTV_FWD_CHUNK_BYTES = 1 << 30      # scratch of one all-frames critic call: the store is evaluated in chunks of rows

    def _gtv_sizes(self, plan, B, T, m):
        """(rows per all-frames forward call, forward scratch bytes, backward scratch bytes, store bytes per row)."""
        per = ops.value_gt_fwd_scratch_bytes(plan, 2) - ops.value_gt_fwd_scratch_bytes(plan, 1)
        chunk = max(1, min((T + 1) * B, (self.GTV_FWD_CHUNK_BYTES - ops.value_gt_fwd_scratch_bytes(plan, 0)) // per))
        return chunk, ops.value_gt_fwd_scratch_bytes(plan, chunk), ops.value_gt_bwd_scratch_bytes(plan, m), plan.num_nodes * 64

    @staticmethod
    def _build_prior_dest(engine, free_flow, dests, dest_slot):
        """The per-destination prior table (N, D) and its column map, refused when the destination set misses a destination
        of some environment's agent table or when table and scratch take more than half of the free device memory."""
        N = engine.N
        ad = engine.agents[..., 1].reshape(-1).to(torch.int64)        # DESTINATION of every agent of every environment
        ad = ad[(ad >= 0) & (ad < N)]
        if tuple(dest_slot.shape) != (N,) or bool((dest_slot.to(engine.device)[ad] < 0).any()):
            raise ValueError("prior_dests must cover the destinations of all environments' agent tables "
                             "(src.agents.base.destination_set(engine.agents, N))")
        table_bytes, scratch_bytes = ops.prior_dest_table_bytes(engine.plan, dests.numel())
        free = torch.cuda.mem_get_info(engine.device)[0]
        if table_bytes + scratch_bytes > free // 2:
            raise ValueError(f"the per-destination prior table ({N} x {dests.numel()} fp32, {table_bytes / 2**20:.0f} MiB) "
                             f"and its scratch ({scratch_bytes / 2**20:.0f} MiB) need more than half of the free device "
                             f"memory ({free / 2**20:.0f} MiB free)")
        w = free_flow.detach().to(engine.device, torch.float32).contiguous()
        return ops.prior_dest_table(engine.plan, w, dests.to(engine.device)), dest_slot.to(engine.device).contiguous()

    def _check_gt_value(self, engine, policy, critic_params, extra_params, rollout_steps, sub_batch_size):
        """Refusals of value="graph_transformer", each naming its limit."""
        if policy == "embedding":
            raise ValueError("value='graph_transformer' needs a state-dependent policy head (edge_mlp, embedding_dijkstra, "
                             "graph_transformer or goal_mlp): the embedding head's rollout builds no observation")
        if engine.fs is None or self.gt_value_params is None or self.gt_value_pe is None:
            raise ValueError("value='graph_transformer' needs the fused engine, gt_value_params and the (N, 16) gt_value_pe")
        ids = {id(p) for p in list(critic_params) + list(extra_params)}
        if not all(id(self.gt_value_params[k]) in ids for k in ops.GT_VALUE_PARAM_KEYS):
            raise ValueError("the graph-transformer critic's parameters must be part of critic_params or extra_params (the "
                             "optimiser's flat buffer)")
        T, B = int(rollout_steps), engine.B
        m = min(int(sub_batch_size), T * B)
        cap = ops.value_gt_bwd_max_samples(engine.plan)
        if m > cap:
            raise ValueError(f"sub_batch_size {m} is too large for the graph-transformer critic's backward on this graph: it "
                             f"takes at most {cap} samples")
        _, fwd, bwd, row = self._gtv_sizes(engine.plan, B, T, m)
        budget = torch.cuda.mem_get_info(engine.device)[0] // 2
        need = (T + 1) * B * row + fwd + bwd
        if need > budget:
            fit = max(0, (budget - fwd - bwd) // row)
            raise ValueError(f"the graph-transformer critic's observation store of (T + 1) * B = {(T + 1) * B} frames "
                             f"({(T + 1) * B * row / 2**30:.1f} GiB) plus its scratch ({(fwd + bwd) / 2**30:.2f} GiB) exceeds "
                             f"half the free device memory ({budget / 2**30:.1f} GiB): at most (T + 1) * B = {fit} frames fit "
                             f"(T = {max(0, fit // B - 1)} at B = {B})")

    # -- views of the live parameters -----------------------------------------------------------------------------------
    def _emb(self):
        return self.emb_param.data.reshape(-1)

    def _critic(self):
        w1, b1, w2, b2, w3, b3 = (p.data for p in self.critic_params)
        return ops.CriticWeights(w1, b1, w2, b2, w3.reshape(-1), b3)

    def _edge_mlp(self):
        return ops.EdgeMlpWeights(*(p.data for p in self.edge_mlp_params))

    def _gt(self):
        return ops.GtWeights(self.gt_params)

    def _goal(self):
        return ops.GoalMlpWeights(flat=self._mlp8_view(self.flat.flat, self._goal_off))

    def _gt_value(self):
        return ops.GtValueWeights(self.gt_value_params)

    # -- HOT LOOP A -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def collect(self):
        """T frames for all B environments (SyncDataCollector with reset_at_each_iter=True, ExplorationType.RANDOM).
        An episode that ends inside the batch (clock past 7 h: ``done = terminated``, src/reinforcement_learning.py:273-276)
        is followed by a reset, like the collector's auto-reset: the rollout is split at that frame, the reset observation
        becomes the next frame's observation and ``done_frames`` marks the frame for GAE."""
        eng = self.eng
        eng.reset()
        T = self.T
        host_times, done = [], [False] * T
        if eng.fs is not None:
            # fused path: every output lands directly in the rollout buffers (no copies), one foreign call per segment
            self.counts[0].zero_()
            if self.policy_hold:        # the shared loop of the state-dependent rollouts consults the switch per frame
                self.held.zero_()
                ops.fused_set_policy_hold(eng.fs, True, self.held)
            if self.route_departures:   # and this one, after the hold launch: the first hop of the agents about to depart
                dests, slot, weights, table, scratch, pend = self._departure_router
                if not self._departure_table_built:     # after the reset every count is 0: free-flow times, built once
                    ops.fused_edge_travel_time(eng.plan, eng.fs, out=weights)
                    ops.destination_trees_batched(eng.plan, weights[:1], dests, out=table, scratch=scratch)
                    self._departure_table_built = True
                self.departures_routed.zero_()
                ops.fused_set_departure_router(eng.fs, True, slot, table[0], pend, self.departures_routed, plan=eng.plan)
            if self.reward_kind == "trip":      # and after every frame's insert: the trip reward over the queue reward
                ops.fused_set_trip_reward(eng.fs, True)
            if self.state_dep:
                self._draw_minibatch_frames()
                if self.credit == "decision":       # and in front of every frame's head: whom the kept rows decide for
                    if self._decision_dist is None:
                        self._build_decision_dist()
                    self.decision_truncated.zero_()
                    if self.credit_horizon == "bootstrap":
                        self.decision_bootstrapped.zero_()
                    if self.credit_scope == "due":
                        self.decision_counts.zero_()
                        ops.fused_set_head_capture(eng.fs, True, self.head_keep, plan=eng.plan, scope="due",
                                                   counts=self.decision_counts)
                    else:
                        ops.fused_set_head_capture(eng.fs, True, self.head_keep, plan=eng.plan)
            else:
                emb = self._emb()
                eng.prepare_policy(emb, self.temperature)      # once per parameter update, not per frame
                # sample_log_prob is only ever read for the <= sub_batch_size frames of each minibatch: keep the behaviour
                # policy's parameters and evaluate it (exactly, with the unfused kernel) for those frames at update time
                self.emb_rollout = emb.clone()
                self.poll_flags()
            for sl in self._segments(done):
                host_times += self._queue(sl)[:-1]
                if self.credit == "decision":       # before _segments resets the engine: the agent table is this segment's
                    self._decision_advantage(sl, host_times)
            host_times.append(float(eng.time))
            if self.credit == "decision":
                ops.fused_set_head_capture(eng.fs, False)
                self._bad_host.copy_(self.decision_bad, non_blocking=True)
            if self.policy_hold:        # off again: whoever else runs this engine gets the loop as it always was
                ops.fused_set_policy_hold(eng.fs, False)
            if self.route_departures:
                ops.fused_set_departure_router(eng.fs, False)
            if self.reward_kind == "trip":
                ops.fused_set_trip_reward(eng.fs, False)
            if self.obs_all is not None:      # frame T: the final state (an episode end at T - 1 is not followed by a reset)
                eng.obs16(out=self.obs_all[T])
            # the device status word travels to pinned host memory behind the rollout; it is looked at when it has
            # arrived (no stall of the launch pipeline) and by check_flags() at the caller's synchronisation points
            self._flag_host.copy_(eng.fs.flags, non_blocking=True)
            self._flag_event = torch.cuda.Event()
            self._flag_event.record()
        else:
            emb = self._emb()
            for t in range(T):
                self.counts[t].copy_(eng.counts)
                host_times.append(float(eng.time))
                logits = ops.policy_edge_logits(eng.plan, eng.node_features, emb)
                proba = ops.graphdist_softmax(eng.plan, logits, self.temperature)
                self.sample_counter += 1
                _, choice = ops.graphdist_sample(eng.plan, proba, seed=self.seed ^ 0x5DEECE66D,
                                                 counter=self.sample_counter, want_onehot=False, want_choice=True)
                lp, _ = ops.graphdist_logprob_entropy(eng.plan, proba, choice=choice, want_entropy=False)
                self.choice[t].copy_(choice)
                self.logp[t].copy_(lp)
                reward, is_done = eng.step(choice=choice)
                self.reward[t].copy_(reward)
                if is_done:
                    done[t] = True
                    if t + 1 < T:
                        eng.reset()
            self.counts[T].copy_(eng.counts)
            host_times.append(float(eng.time))
        self.times.copy_(torch.tensor(host_times, dtype=torch.float32))
        self.done_frames = torch.tensor(done, dtype=torch.bool)
        # (T, B) mask for tarl_gae, only when an episode actually ended inside the batch
        self.done_mask = (self.done_frames.to(eng.device, torch.uint8).view(T, 1).expand(T, eng.B).contiguous()
                          if any(done) else None)
        return T * eng.B

    def _segments(self, done):
        """The batch's frames as episode segments (slices), each queued by one foreign call: frames until the episode ends
        (the frame whose step pushes the clock past EPISODE_END is the last) or the batch is full. After an episode end
        the engine is reset, the reset observation becomes the next frame's and ``done`` marks the frame."""
        eng, T, t = self.eng, self.T, 0
        while t < T:
            n = int(min(T - t, max(1, (EPISODE_END - eng.time) // eng.timestep + 1)))
            yield slice(t, t + n)
            t += n
            if eng.time > EPISODE_END:
                done[t - 1] = True
                if t < T:
                    eng.reset()
                    self.counts[t].zero_()

    def _decision_advantage(self, sl, host_times):
        """The raw per-decision advantages of the kept rows of segment ``sl`` (ops.decision_advantage), from the agent table
        as the segment's last frame left it."""
        eng = self.eng
        t_sorted, keep_env, keep_slot = self._keep
        lo, hi = bisect_left(t_sorted, sl.start), bisect_left(t_sorted, sl.stop)
        if hi == lo:
            return
        if self.decision_critic_params is not None:      # t_end - t of every kept row of this segment
            self.frames_left.index_copy_(0, keep_slot[lo:hi].to(torch.int64), sl.stop - self._keep_frames[lo:hi])
        self.times[sl.start:sl.stop].copy_(torch.tensor(host_times[sl.start:sl.stop], dtype=torch.float32))
        dist, slot = self._decision_dist
        boot = {}
        if self.credit_horizon == "bootstrap":      # a segment cut by the batch is bootstrapped; an episode that ended is not
            ops.fused_agent_roads(eng.plan, eng.fs, eng.Nmax, out=self.agent_road, bad=self.decision_bad)
            boot = dict(agent_road=self.agent_road, bootstrap=bool(eng.time <= EPISODE_END),
                        bootstrapped=self.decision_bootstrapped)
        ops.decision_advantage(eng.plan, self.head_keep, self._keep_frames[lo:hi], keep_env[lo:hi], keep_slot[lo:hi],
                               eng.agents, self.times, sl.stop, dist, slot, B=eng.B, timestep=eng.timestep,
                               decision_gamma=self.decision_gamma, adv_raw=self.adv_raw, truncated=self.decision_truncated,
                               bad=self.decision_bad, **boot)

    def _draw_minibatch_frames(self):
        """State-dependent heads: the update only ever reads the observations of its minibatch frames, and those frames are
        a random draw that does not depend on the data. The draw is made up front and the rollout keeps only their
        observations, so that the update recomputes exactly the rollout's logits."""
        eng = self.eng
        T, B, N = self.T, eng.B, eng.N
        if self.obs_idx is not None:                    # test hook: these frames instead of a random draw
            host = [self.obs_idx.cpu()]
        else:
            host = [self.draw_frames(T * B, min(self.M, T * B), device=False) for _ in range(self.num_epochs)]
        self._mb_idx = [h.pin_memory().to(eng.device, non_blocking=True) for h in host]
        self._epoch = 0
        flat = torch.cat(host)      # (the frame list stays on the host: no device round trip before the rollout)
        order = torch.argsort(flat, stable=True)
        if self.obs_all is not None:
            # the graph-transformer critic keeps every (frame, environment) observation: row t * B + b of the store; the
            # minibatches read their rows from it
            self._keep = ([t for t in range(T) for _ in range(B)],
                          torch.arange(B, dtype=torch.int32, device=eng.device).repeat(T),
                          torch.arange(T * B, dtype=torch.int32, device=eng.device))
            self.obs_mb = self.obs_all.view((T + 1) * B, N, 16)
            return
        self._keep = (torch.div(flat[order], B, rounding_mode="floor").tolist(),        # frames, sorted
                      (flat[order] % B).to(torch.int32).pin_memory().to(eng.device, non_blocking=True),
                      order.to(torch.int32).pin_memory().to(eng.device, non_blocking=True))
        self.obs_mb = torch.empty((flat.numel(), N, 16), dtype=torch.float32, device=eng.device)
        if self.credit == "decision":       # per kept row and road: the head, its raw advantage, the behaviour log-prob
            self._keep_frames = torch.tensor(self._keep[0], dtype=torch.int32).pin_memory().to(eng.device, non_blocking=True)
            if self.head_keep is None or self.head_keep.size(0) != flat.numel():
                self.head_keep = torch.empty((flat.numel(), N), dtype=torch.int32, device=eng.device)
                self.adv_raw = torch.empty((flat.numel(), N), dtype=torch.float32, device=eng.device)
                self.lp_old_node = torch.empty((flat.numel(), N), dtype=torch.float32, device=eng.device)
            if self.decision_critic_params is not None and (self.adv_dec is None or self.adv_dec.size(0) != flat.numel()):
                self.frames_left = torch.zeros(flat.numel(), dtype=torch.int32, device=eng.device)
                self.adv_dec = torch.empty((flat.numel(), N), dtype=torch.float32, device=eng.device)
                self.value_old = torch.empty((flat.numel(), N), dtype=torch.float32, device=eng.device)

    def _queue(self, sl):
        """Frames ``sl`` (one episode segment) in one foreign call; returns the clock values. The embedding head draws from
        its tables (tarl_rollout_env / tarl_fused_rollout); the state-dependent heads evaluate their logits from the packed
        state per frame (tarl_fused_rollout_policy: observation -> edge MLP; tarl_fused_rollout_prior: shortest-path
        prior, without the per-step logs leg / dtt_node / events) -> GraphDistribution sample + log_prob -> the frame."""
        eng, n = self.eng, sl.stop - sl.start
        counts = self.counts[sl.start:sl.stop + 1]
        logs = dict(metrics_envs=self.metrics_envs, dtt_node=None if self.dtt_node is None else self.dtt_node[sl],
                    events=None if self.events is None else self.events[sl], leg=self.leg[sl])
        if not self.state_dep:
            run = eng.rollout_env if self.rollout == "env" else eng.rollout_fused
            return run(n, choice=self.choice[sl], log_prob=None if self.lazy_log_prob else self.logp[sl],
                       reward=self.reward[sl], counts=counts, check=False, **logs)
        # the kept (frame, environment) pairs of this segment with their offsets per frame
        t_sorted, keep_env, keep_slot = self._keep
        lo, hi = bisect_left(t_sorted, sl.start), bisect_left(t_sorted, sl.stop)
        keep = ([bisect_left(t_sorted, t) - lo for t in range(sl.start, sl.stop + 1)], keep_env[lo:hi],
                keep_slot[lo:hi]) if hi > lo else None
        kw = dict(temperature=self.temperature, policy_seed=self.seed ^ 0x5DEECE66D, policy_counter0=self.sample_counter + 1,
                  choice8=self.choice[sl], log_prob=self.logp[sl], reward=self.reward[sl], counts=counts, keep=keep,
                  obs_keep=self.obs_mb, check=False)
        if self.policy == "edge_mlp":
            times = eng.rollout_policy(n, self._edge_mlp(), precision=self.policy_precision, **logs, **kw)
        elif self.policy == "graph_transformer":
            times = eng.rollout_gt(n, self.gt_pe, self._gt(), **kw)
        elif self.policy == "goal_mlp":
            times = eng.rollout_goal(n, self._goal(), self.prior_table, self.goal_scale, self.prior_dest_slot, **kw)
        else:
            times = eng.rollout_prior(n, self._emb(), self.prior_table, prior_weight=self.prior_weight,
                                      dest_slot=self.prior_dest_slot, **kw)
        self.sample_counter += n
        return times

    def draw_frames(self, n, M, device=True):
        """M distinct flat frame indices t * B + b out of n, uniform, int64 (host draw; device=True: asynchronous copy)."""
        idx = torch.from_numpy(self.np_rng.choice(n, size=M, replace=False, shuffle=True).astype("int64"))
        return idx.pin_memory().to(self.eng.device, non_blocking=True) if device else idx

    def poll_flags(self):
        """Raise if a finished rollout flagged a domain exit (non-blocking)."""
        if self._flag_event is not None and self._flag_event.query():
            self._flag_event = None
            if int(self._flag_host[0]) != 0:
                self.eng.check_flags()
            if self.credit == "decision" and int(self._bad_host[0]) != 0:
                self._raise_bad_heads(int(self._bad_host[0]))

    def check_flags(self):
        """Blocking form of :meth:`poll_flags` (call at a synchronisation point, e.g. the end of training)."""
        self._flag_event = None
        self.eng.check_flags()
        if self.credit == "decision" and int(self.decision_bad.item()) != 0:
            self._raise_bad_heads(int(self.decision_bad.item()))

    def _raise_bad_heads(self, n):
        raise ops._lib.TarlError(f"credit='decision': {n} captured head ids lie at or beyond the agent table's {self.eng.A} "
                                 "rows: the packed state and the agent table do not belong together")

    # -- HOT LOOP B -------------------------------------------------------------------------------------------------------
    def _actor_logits(self, obs):
        """The policy head's logits (M, E) for the minibatch observations ``obs``, fp32, current parameters (the prior
        head's equal the rollout's, recomputed from the kept observations)."""
        eng = self.eng
        if self.policy == "edge_mlp":
            return ops.policy_edge_mlp(eng.plan, obs, eng.ec, self._edge_mlp())          # fp32 MFMA
        if self.policy == "graph_transformer":
            return ops.policy_gt_logits(eng.plan, obs, eng.ec, self.gt_pe, self._gt())
        if self.policy == "goal_mlp":
            return ops.policy_goal_mlp(eng.plan, obs, self._goal(), self.prior_table, self.goal_scale,
                                       dest_slot=self.prior_dest_slot)
        if self.policy == "embedding_dijkstra":
            return ops.policy_prior_logits(eng.plan, obs, self._emb(), self.prior_table, self.prior_weight,
                                           dest_slot=self.prior_dest_slot)
        return ops.policy_edge_logits(eng.plan, obs, self._emb())

    def _actor_logits_bwd(self, obs, g_logits):
        """Backward of :meth:`_actor_logits`: the parameter gradients land in the flat gradient buffer."""
        eng = self.eng
        if self.policy == "edge_mlp":
            gm = [self.flat.grad_view(p) for p in self.edge_mlp_params]
            ops.policy_edge_mlp_bwd(eng.plan, obs, eng.ec, self._edge_mlp(), g_logits,
                                    (gm[0], gm[1], gm[2], gm[3], gm[4].view(-1), gm[5]))
        elif self.policy == "graph_transformer":
            need = ops.gt_bwd_scratch_bytes(eng.plan, obs.size(0)) // 4
            if getattr(self, "_gt_scratch", None) is None or self._gt_scratch.numel() < need:
                self._gt_scratch = torch.empty(need, dtype=torch.float32, device=eng.device)     # once per trainer
            ops.policy_gt_bwd(eng.plan, obs, eng.ec, self.gt_pe, self._gt(), g_logits,
                              [self.flat.grad_view(self.gt_params[k]) for k in ops.GT_PARAM_KEYS], scratch=self._gt_scratch)
        elif self.policy == "goal_mlp":
            need = ops.goal_mlp_bwd_scratch_floats(eng.plan, obs.size(0))
            if getattr(self, "_goal_scratch", None) is None or self._goal_scratch.numel() < need:
                self._goal_scratch = torch.empty(need, dtype=torch.float32, device=eng.device)     # once per trainer
            ops.policy_goal_mlp_bwd(eng.plan, obs, self._goal(), self.prior_table, self.goal_scale, g_logits,
                                    self._mlp8_view(self.flat.grad, self._goal_off),
                                    dest_slot=self.prior_dest_slot, scratch=self._goal_scratch)
        else:       # the prior has no parameters: the embedding receives the logits' gradient as is
            g_emb = ops.policy_edge_logits_bwd(eng.plan, obs, g_logits, self.emb_param.numel())
            self.flat.grad_view(self.emb_param).add_(g_emb.view_as(self.emb_param))

    def advantages(self):
        """GAE(gamma, lmbda, average_gae=True) with the current critic over all (T+1)*B observations."""
        eng = self.eng
        T, B, N = self.T, eng.B, eng.N
        cw = None if self.obs_all is not None else self._critic()
        with self.stage("critic_all_frames"):
            if self.obs_all is not None:
                v = self._gt_value_all_frames()
            elif self.env_minor and B % 128 == 0:
                v = ops.critic_forward_slabs(cw, self.counts, self.times)           # reads [frame][node][env] bytes as is
            elif self.env_minor and self.counts.dtype == torch.uint8:    # odd batch sizes: the count bytes as fp32 rows first
                _, rows = ops.rollout_gather(eng.plan, T + 1, B, True, counts=self.counts)
                v, _, _ = ops.critic_forward(cw, rows, self.times, rows_per_time=B)
            elif self.env_minor:
                rows = self.counts.permute(0, 2, 1).contiguous().view((T + 1) * B, N)
                v, _, _ = ops.critic_forward(cw, rows, self.times, rows_per_time=B)
            else:
                v, _, _ = ops.critic_forward(cw, self.counts.view((T + 1) * B, N), self.times, rows_per_time=B)
        self.values = v.view(T + 1, B)
        # done = terminated (src/reinforcement_learning.py:296): no bootstrap across an episode end
        with self.stage("gae"):
            adv, target = ops.gae(self.reward, self.values[:T], self.values[1:], done=self.done_mask,
                                  terminated=self.done_mask, gamma=self.gamma, lmbda=self.lmbda)
            stats = ops.advantage_stats(adv)
            dist_utils.allreduce_sum_(stats)          # global mean / std over all ranks' frames
            ops.advantage_normalize_(adv, stats)
        return adv, target

    def _gt_value_all_frames(self):
        """The graph-transformer critic over all (T + 1) * B stored observations, in chunks of rows -> (T + 1) * B values."""
        eng = self.eng
        rows = self.obs_all.view(-1, eng.N, 16)
        chunk, fwd, _, _ = self._gtv_sizes(eng.plan, eng.B, self.T, 1)
        if getattr(self, "_gtv_fwd_scratch", None) is None:
            self._gtv_fwd_scratch = torch.empty(fwd // 4, dtype=torch.float32, device=eng.device)     # once per trainer
        v = torch.empty(rows.size(0), dtype=torch.float32, device=eng.device)
        w = self._gt_value()
        for lo in range(0, rows.size(0), chunk):
            hi = min(lo + chunk, rows.size(0))
            ops.value_gt_forward(eng.plan, rows[lo:hi], self.gt_value_pe, w, out=v[lo:hi], scratch=self._gtv_fwd_scratch)
        return v

    def minibatch_step(self, adv, target, idx=None):
        """One minibatch + one Adam step. ``idx`` (test hook): flat frame indices t * B + b instead of a random draw."""
        eng = self.eng
        T, B, N = self.T, eng.B, eng.N
        if self.state_dep:       # the draw was made before the rollout (its observations were kept)
            idx = self._mb_idx[self._epoch]
            off = sum(i.numel() for i in self._mb_idx[:self._epoch])
            if self.obs_all is not None:         # rows t * B + b of the observation store (the same values)
                obs = self.obs_mb.index_select(0, idx)
            else:
                obs = self.obs_mb[off:off + idx.numel()]
            self._epoch += 1
        else:
            idx = self.draw_frames(T * B, min(self.M, T * B)) if idx is None else idx.to(eng.device)
            # the live policy reads only the static ROAD_INDEX column: one observation broadcast over the minibatch
            obs = eng.static_node_features[:1].expand(idx.numel(), N, 7)
        M = idx.numel()
        st = self.stage
        with st("minibatch_gather"):
            if self.state_dep:
                counts_mb = None if self.obs_all is not None else \
                    ops.rollout_gather(eng.plan, T, B, True, idx, counts=self.counts[:T])[1]            # env-minor bytes
                choice_mb, _ = ops.rollout_gather(eng.plan, T, B, False, idx, choice=self.choice)        # env-major bytes
            elif self.rollout == "unfused":
                counts_mb = self.counts[:T].view(T * B, N).index_select(0, idx)
                choice_mb = self.choice.view(T * B, N).index_select(0, idx)
            else:   # one launch: the sampled frames' action bytes -> edge ids, count bytes -> fp32 rows
                choice_mb, counts_mb = ops.rollout_gather(eng.plan, T, B, self.env_minor, idx, choice=self.choice,
                                                          counts=self.counts[:T])
            if eng.fs is not None and self.lazy_log_prob:   # behaviour log-prob of the sampled frames, rollout-time parameters
                p_old = ops.graphdist_softmax(eng.plan, ops.policy_edge_logits(eng.plan, obs, self.emb_rollout),
                                              self.temperature)
                lp_old, _ = ops.graphdist_logprob_entropy(eng.plan, p_old, choice=choice_mb, want_entropy=False)
            else:
                lp_old = self.logp.view(-1).index_select(0, idx)
            adv_mb = adv.view(-1).index_select(0, idx)
            tgt_mb = target.view(-1).index_select(0, idx)
            time_mb = self.times[:T].index_select(0, torch.div(idx, B, rounding_mode="floor"))
        with st("actor_logits_fwd"):
            logits = self._actor_logits(obs)
        with st("graphdist_fwd"):
            proba = ops.graphdist_softmax(eng.plan, logits, self.temperature)
            lp_new, ent = ops.graphdist_logprob_entropy(eng.plan, proba, choice=choice_mb)
        gtv = self.obs_all is not None
        cw = self._gt_value() if gtv else self._critic()
        with st("critic_fwd"):
            if gtv:
                value = ops.value_gt_forward(eng.plan, obs, self.gt_value_pe, cw)
            else:
                # split-K while the minibatch is far from filling the chip with 128-row MFMA tiles (M = 4 096: 32 workgroups
                # walking all N columns alone took 743 us, bench.py's update_path; spread over the columns: see DESIGN §4.7)
                value, h1, h2 = ops.critic_forward(cw, counts_mb, time_mb, 1, keep_hidden=True, split_k=M <= 16384)
        scale = 1.0 / self.world
        if self.credit == "decision":       # the policy term is the per-decision one below: no joint gradient (g_lp = 0)
            adv_mb = torch.zeros_like(adv_mb)
        with st("ppo_loss"):
            out, g_lp, g_ent, g_val = ops.ppo_loss(lp_new, lp_old, adv_mb, value, tgt_mb, ent,
                                                   clip_epsilon=self.clip_epsilon, entropy_coef=self.entropy_coef,
                                                   critic_coef=self.critic_coef, grad_scale=scale)
        # backward
        self.flat.zero_grad()
        with st("graphdist_bwd"):
            g_logits = ops.graphdist_logprob_entropy_bwd(eng.plan, proba, self.temperature, choice=choice_mb,
                                                         grad_log_prob=g_lp, grad_entropy=g_ent, log_prob_fwd=lp_new)
        if self.credit == "decision":
            with st("decision_ppo"):
                self._decision_step(logits, choice_mb, off, M, scale, g_logits)
            if self.decision_critic_params is not None:
                with st("decision_critic"):
                    self._decision_critic_step(obs, off, M, scale)
        with st("actor_logits_bwd"):
            self._actor_logits_bwd(obs, g_logits)
        with st("critic_bwd"):
            if gtv:
                need = ops.value_gt_bwd_scratch_bytes(eng.plan, M) // 4
                if getattr(self, "_gtv_bwd_scratch", None) is None or self._gtv_bwd_scratch.numel() < need:
                    self._gtv_bwd_scratch = torch.empty(need, dtype=torch.float32, device=eng.device)    # once per trainer
                ops.value_gt_backward(eng.plan, obs, self.gt_value_pe, cw, g_val,
                                      [self.flat.grad_view(self.gt_value_params[k]) for k in ops.GT_VALUE_PARAM_KEYS],
                                      scratch=self._gtv_bwd_scratch)
            else:
                gw = [self.flat.grad_view(p) for p in self.critic_params]
                ops.critic_backward(cw, counts_mb, time_mb, 1, h1, h2, g_val,
                                    (gw[0], gw[1], gw[2], gw[3], gw[4].view(-1), gw[5]))
        with st("grad_allreduce"):
            self.flat.allreduce_grads()               # ONE all-reduce of the fused gradient buffer (RCCL over xGMI)
        self.last_grad = self.flat.grad.clone() if getattr(self, "keep_grad", False) else None
        with st("adam"):
            self.flat.adam_step(lr=self.lr)
        return out

    def _decision_prepare(self):
        """credit="decision", after ``collect()`` and before the first optimiser step: the behaviour log-prob of every
        (kept row, road) from the forward the update uses, on the kept observations with the parameters the rollout used, and
        the statistics of the raw advantage over all live decisions of all kept rows (all ranks')."""
        eng = self.eng
        off = 0
        for idx in self._mb_idx:
            M = idx.numel()
            choice_mb, _ = ops.rollout_gather(eng.plan, self.T, eng.B, False, idx, choice=self.choice)
            ops.graphdist_node_logprob(eng.plan, self._actor_logits(self.obs_mb[off:off + M]), choice_mb, self.temperature,
                                       out=self.lp_old_node[off:off + M])
            off += M
        self._decision_local = ops.decision_stats(self.adv_raw, self.head_keep)      # this rank's {sum, sum of squares, count}
        self._decision_adv = self.adv_raw
        if self.decision_critic_params is not None:      # the learned baseline, once, with the parameters the rollout had
            dist, slot = self._decision_dist
            ops.decision_critic_forward(eng.plan, self.obs_mb, self.head_keep, self.frames_left, dist, slot, self._dcritic(),
                                        self.adv_raw, timestep=eng.timestep, delay_scale=self.decision_delay_scale,
                                        value=self.value_old, adv_out=self.adv_dec)
            self._decision_adv = self.adv_dec
            self._decision_stats = ops.decision_stats(self.adv_dec, self.head_keep)
            self._dcritic_last = None
        else:
            self._decision_stats = self._decision_local.clone()
        dist_utils.allreduce_sum_(self._decision_stats)
        self._decision_last = None

    def _decision_step(self, logits, choice_mb, off, M, scale, g_logits):
        """The per-decision policy term of one minibatch (rows ``off .. off + M`` of the kept buffers): its gradient is
        added into ``g_logits`` on the out-edges of the live roads."""
        head = self.head_keep[off:off + M]
        n_live = (head > 0).sum(dtype=torch.int32).reshape(1)
        need = (ops._lib.load().tarl_graphdist_decision_ppo_scratch_bytes(self.eng.plan.handle, M) + 7) // 8
        if getattr(self, "_decision_scratch", None) is None or self._decision_scratch.numel() < need:
            self._decision_scratch = torch.empty(need, dtype=torch.float64, device=self.eng.device)      # once per trainer
        out4 = ops.graphdist_decision_ppo(self.eng.plan, logits, choice_mb, head, self.lp_old_node[off:off + M],
                                          self._decision_adv[off:off + M], self._decision_stats, n_live,
                                          clip_epsilon=self.clip_epsilon, temperature=self.temperature, grad_scale=scale,
                                          grad_logits=g_logits, scratch=self._decision_scratch)
        self._decision_last = (out4.sum(0), n_live)

    def _decision_critic_step(self, obs, off, M, scale):
        """The critic's loss on the live decisions of one minibatch, current parameters: its gradient is added into the
        critic's run of the flat gradient buffer."""
        need = (ops.decision_critic_scratch_bytes(self.eng.plan, M) + 7) // 8
        if getattr(self, "_dcritic_scratch", None) is None or self._dcritic_scratch.numel() < need:
            self._dcritic_scratch = torch.empty(need, dtype=torch.float64, device=self.eng.device)      # once per trainer
        dist, slot = self._decision_dist
        out5 = ops.decision_critic_loss(
            self.eng.plan, obs, self.head_keep[off:off + M], self.frames_left[off:off + M], dist, slot, self._dcritic(),
            self.adv_raw[off:off + M], self._decision_last[1], timestep=self.eng.timestep,
            delay_scale=self.decision_delay_scale, coef=self.decision_critic_coef, grad_scale=scale,
            grads=self._mlp8_view(self.flat.grad, self._dcritic_off),
            scratch=self._dcritic_scratch)
        self._dcritic_last = (out5, off, M)      # summed where the report is built: no further launch per step

    def _decision_report(self):
        """``self.last["decision"]``: 0-d device tensors (no synchronisation here)."""
        tot, _ = self._decision_last
        live = tot[1].clamp(min=1.0)
        st = self._decision_local
        cnt = st[2].clamp(min=1.0)
        rep = {"decisions": st[2], "delay_frames": -st[0] / cnt,
               "truncated": self.decision_truncated[0].to(torch.float64) / cnt, "objective": -tot[0] / live,
               "clip_fraction": tot[2] / live, "kl": tot[3] / live}
        if self.credit_scope == "due":          # the kept rows' roads with a head, of which ``decisions`` were due and live
            rep["credit_scope"] = "due"
            rep["decisions_headed"] = self.decision_counts[0].to(torch.float64)
        if self.credit_horizon == "bootstrap":  # the share continued beyond the horizon (``truncated``: the share charged)
            rep["credit_horizon"] = "bootstrap"
            rep["bootstrapped"] = self.decision_bootstrapped[0].to(torch.float64) / cnt
        if self.decision_critic_params is not None:      # the last epoch's five sums, over all ranks
            out5, off, M = self._dcritic_last
            # ... and the sum of the values the advantages were formed with (0 where not live)
            s5 = torch.cat([out5.sum(0), self.value_old[off:off + M].sum(dtype=torch.float64).reshape(1)])
            if self.world > 1:
                s5 = s5.clone()
                dist_utils.allreduce_sum_(s5)
            n = s5[1].clamp(min=1.0)
            den = s5[3] - s5[2] * s5[2] / n
            rep["critic_loss"] = self.decision_critic_coef * s5[0] / n
            rep["explained_variance"] = torch.where(den > 0, 1.0 - s5[4] / den.clamp(min=1e-300), torch.zeros_like(den))
            rep["value_mean"] = s5[5] / n
        return rep

    def update(self):
        out = None
        if self.credit == "decision":
            self._decision_prepare()
        for _ in range(self.num_epochs):
            adv, target = self.advantages()
            out = self.minibatch_step(adv, target)
        self.last = {"losses": out}
        if self.credit == "decision":
            self.last["decision"] = self._decision_report()
        return out

    def train_iteration(self):
        frames = self.collect()
        self.update()
        return frames
