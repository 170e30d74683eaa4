"""Runner / RunnerArgs — CLI-facing orchestration (reference: src/runner.py). ``mpnn`` and ``mpnn+ppo`` run on the HIP
path; ``random`` and ``dijkstra`` run the classical loop on the same kernels (``dijkstra``: all-pairs next-hop table by
``tarl_apsp`` instead of networkx, or per-destination trees by ``tarl_dest_trees``, ``dijkstra_method``)."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import torch


@dataclass
class RunnerArgs:
    algo: str
    scenario: str
    mode: str
    timestep_size: int = 1
    start_end_time: list = (0, 86400)
    epochs: int = 1
    rollout_steps: int = 32
    seed: int = 0
    device: str = "cpu"
    output_dir: str = "runs"
    profile: bool = False
    torch_compile: bool = False
    steps: int = None          # README / BASELINE use --steps; the reference CLI lacks it
    num_envs: int = 1
    policy_head: str = "embedding"
    prior_weight: float = 1.0      # policy_head "embedding_dijkstra": weight of the shortest-path prior
    prior_method: str = "all_pairs"   # its distances: "all_pairs", "per_destination" or "auto" (MPNNPolicyNet.prior_method)
    #                                   (policy_head "goal_mlp" reads the same tables)
    value_head: str = "simple"     # "graph_transformer": ValueNet (src/agents/transformer_agent.py)
    dijkstra_method: str = "all_pairs"   # DijkstraAgents: "all_pairs", "per_destination" or "auto"
    equilibrium_metrics: bool = False    # eval: TSTT at UE and SO, both relative gaps, Price of Anarchy (algorithms/equilibrium.py)
    equilibrium_gap: float = 1e-4        # its relative-gap target
    equilibrium_max_iter: int = 500      # and its iteration limit per problem
    eval_envs: int = 0             # mpnn / mpnn+ppo: K > 0 adds the vectorised evaluation (tarl_hip.evaluator) on K environments
    eval_sampled: bool = False     # ... and also a sampled one next to the deterministic (MODE) one
    eval_baseline: str = "none"    # eval_envs: "dijkstra" adds the shortest-path baseline on a second engine + the paired report;
    #                                "dijkstra_hold": the router that holds one road short and delivers; "free_flow": that one on static tables
    policy_hold: bool = False      # mpnn / mpnn+ppo: the hold rule on the policy's action in the vectorised
    #                                evaluation (eval: needs eval_envs) and in vectorised training (not policy_head "embedding")
    route_departures: bool = False # the first-hop rule on empty origin roads: eval with eval_envs, dijkstra_envs
    #                                (routers hold / free_flow) or replan_days; train with the state-dependent heads
    reward: str = "queue"          # "trip": the trip reward of DESIGN 4.24 — train: what PPO optimises (state-dependent heads);
    #                                eval: computed beside the queue reward with eval_envs, dijkstra_envs or replan_days
    credit: str = "joint"          # train: "decision" = per-decision PPO credit (state-dependent heads, default critic)
    credit_gamma: float = None     # ... the discount of a traveller's frames to go, in (0, 1] (default 1.0)
    credit_baseline: str = None    # ... "learned" = the per-decision critic of DESIGN 4.27 (default "free_flow")
    credit_critic_coef: float = None   # ... the coefficient of that critic's loss (default 1.0)
    credit_scope: str = None       # ... "due" = only roads whose head is due are credited (default "headed")
    credit_horizon: str = None     # ... "bootstrap" = free-flow continuation past a segment cut by the batch (default "charge")
    dijkstra_envs: int = 0         # dijkstra, eval: K > 0 adds VecEvaluator(head="dijkstra") on K environments
    dijkstra_router: str = "reference"   # dijkstra_envs: "reference", "hold" (head "dijkstra_hold") or "free_flow" (hold, static tables)
    eval_link_counts: bool = False # eval_envs / dijkstra_envs: per-road link counts over the K environments (eval mode reports them)
    eval_link_bin: int = 3600      # ... in time bins of this many seconds
    eval_occupancy: bool = False   # eval_envs / dijkstra_envs: per-road occupancy and time at capacity (bins of eval_link_bin)
    eval_trips: bool = False       # eval_envs / dijkstra_envs: per-traveller travel time and delay (bins of eval_link_bin)
    eval_dynamic_gap: bool = False # eval_envs / dijkstra_envs, eval: the trips against the best path in hindsight (same bins)
    eval_dynamic_gap_envs: int = None   # ... over the first J of the K environments (default: all)
    eval_turns: bool = False       # eval_envs / dijkstra_envs: vehicles per route edge and the agents quirk Q24 loses (same bins)
    eval_paths: bool = False       # eval_envs / dijkstra_envs, eval: the per-agent path trace of DESIGN 4.25 (same bins)
    eval_paths_max_hops: int = None     # ... roads kept per trace (default 64; 0: none)
    eval_paths_routes: int = 0     # ... the kept routes of the first J environments into <prefix>_paths_routes.csv
    replan_days: int = 0           # eval, any algo: J > 0 adds the day-to-day replanning loop (tarl_hip.replanning)
    replan_envs: int = 1           # ... on this many environments of an engine of its own
    replan_fraction: object = 0.1  # ... the share that may switch per day, in (0, 1], or "msa"
    replan_max_hops: int = None    # ... the longest route stored (default: min(roads, 256))
    iterations: int = 1            # train: collector batches; total_frames = iterations * rollout_steps
    pretrain_bc: int = 0           # train, mpnn / mpnn+ppo: I > 0 behaviour-cloning iterations before PPO
    bc_expert: str = None          # ... the router imitated: "dijkstra" (default; congested times, refreshed) or "free_flow"
    bc_driver: str = None          # ... who drives the labelled rollout: "expert", "policy" or "dagger" (default)
    bc_envs: int = None            # ... environments of the BC engine (default 16)
    bc_frames: int = None          # ... frames per iteration (default: rollout_steps)
    bc_samples: int = None         # ... (environment, frame) pairs kept per iteration (default 256)
    bc_epochs: int = None          # ... passes over the store (default 4)
    bc_batch: int = None           # ... minibatch (default: the PPO sub-batch)
    bc_lr: float = None            # ... Adam step size (default: the PPO trainer's)
    checkpoint: str = None         # mpnn / mpnn+ppo: a policy.pt written by ppo_train, loaded after setup()

    @property
    def total_frames(self) -> int:
        return int(self.iterations) * int(self.rollout_steps)

    def __post_init__(self):
        if self.eval_envs is None or int(self.eval_envs) < 0:
            raise ValueError(f"eval_envs must be >= 0, got {self.eval_envs!r}")
        if self.eval_envs and self.algo in ("random", "dijkstra"):
            raise ValueError(f"eval_envs evaluates a policy network on the vectorised engine: not available for algo "
                             f"{self.algo!r} (use mpnn or mpnn+ppo)")
        if self.eval_sampled and not self.eval_envs:
            raise ValueError("eval_sampled adds a sampled run to the vectorised evaluation: it needs eval_envs > 0")
        if self.eval_baseline not in EVAL_BASELINE_NAMES:
            raise ValueError(f"eval_baseline must be one of {EVAL_BASELINE_NAMES}, got {self.eval_baseline!r}")
        if self.eval_baseline != "none" and not (self.eval_envs and self.algo in ("mpnn", "mpnn+ppo")):
            raise ValueError("eval_baseline compares the vectorised evaluation of a policy network with the shortest-path "
                             "router: it needs eval_envs > 0 and algo mpnn or mpnn+ppo")
        if self.policy_hold:
            if self.algo not in ("mpnn", "mpnn+ppo"):
                raise ValueError("policy_hold applies the hold rule to a policy network's action: it needs algo mpnn or "
                                 "mpnn+ppo (the dijkstra routers have their own: dijkstra_router / eval_baseline)")
            if self.mode == "eval" and not self.eval_envs:
                raise ValueError("policy_hold acts in the vectorised evaluation: in mode 'eval' it needs eval_envs > 0 (the "
                                 "single-environment, reference-shaped pass is not changed)")
            if self.mode == "train" and self.policy_head == "embedding":
                raise ValueError("policy_hold cannot train policy_head 'embedding': its rollout kernels draw the actions of "
                                 "all frames ahead of the frames, so the rule has no frame state to read; use a "
                                 "state-dependent head (edge_mlp*, embedding_dijkstra, graph_transformer, goal_mlp)")
        if self.dijkstra_envs is None or int(self.dijkstra_envs) < 0:
            raise ValueError(f"dijkstra_envs must be >= 0, got {self.dijkstra_envs!r}")
        if self.dijkstra_envs and not (self.algo == "dijkstra" and self.mode == "eval"):
            raise ValueError("dijkstra_envs evaluates the shortest-path router on the vectorised engine: only with algo "
                             "'dijkstra' and mode 'eval'")
        if self.dijkstra_router not in DIJKSTRA_ROUTER_NAMES:
            raise ValueError(f"dijkstra_router must be one of {DIJKSTRA_ROUTER_NAMES}, got {self.dijkstra_router!r}")
        if self.dijkstra_router != "reference" and not self.dijkstra_envs:
            raise ValueError("dijkstra_router selects the router of the vectorised dijkstra evaluation: it needs dijkstra_envs > 0")
        if self.route_departures:
            if self.mode == "eval" and not (self.eval_envs or self.dijkstra_envs or self.replan_days):
                raise ValueError("route_departures acts in the vectorised evaluation: in mode 'eval' it needs eval_envs > 0, "
                                 "dijkstra_envs > 0 (dijkstra_router hold or free_flow) or replan_days > 0 (the "
                                 "single-environment, reference-shaped pass is not changed)")
            if self.eval_baseline == "dijkstra":
                raise ValueError("route_departures leaves the reference-order router as the reference has it: use "
                                 "eval_baseline dijkstra_hold or free_flow")
            if self.dijkstra_envs and self.dijkstra_router == "reference":
                raise ValueError("route_departures leaves the reference-order router as the reference has it: use "
                                 "dijkstra_router hold or free_flow")
            if self.mode == "train" and self.algo not in ("mpnn", "mpnn+ppo"):
                raise ValueError("route_departures in mode 'train' acts on vectorised training: it needs algo mpnn or mpnn+ppo")
            if self.mode == "train" and self.policy_head == "embedding":
                raise ValueError("route_departures cannot train policy_head 'embedding': its rollout kernels draw the actions "
                                 "of all frames ahead of the frames, so the rule has no frame state to read; use a "
                                 "state-dependent head (edge_mlp*, embedding_dijkstra, graph_transformer, goal_mlp)")
        if self.reward not in ("queue", "trip"):
            raise ValueError(f"reward must be 'queue' or 'trip', got {self.reward!r}")
        if self.reward == "trip":
            if self.mode == "eval" and not (self.eval_envs or self.dijkstra_envs or self.replan_days):
                raise ValueError("reward trip is computed by the vectorised evaluation: in mode 'eval' it needs eval_envs > 0, "
                                 "dijkstra_envs > 0 or replan_days > 0 (the single-environment, reference-shaped pass is not "
                                 "changed)")
            if self.mode == "train" and self.algo not in ("mpnn", "mpnn+ppo"):
                raise ValueError("reward trip in mode 'train' acts on vectorised training: it needs algo mpnn or mpnn+ppo")
            if self.mode == "train" and self.policy_head == "embedding":
                raise ValueError("reward trip cannot train policy_head 'embedding': its rollout kernels do not go through the "
                                 "shared loop of the state-dependent heads, where the trip launch follows every frame's "
                                 "insert; use a state-dependent head (edge_mlp*, embedding_dijkstra, graph_transformer, "
                                 "goal_mlp)")
        if self.credit not in ("joint", "decision"):
            raise ValueError(f"credit must be 'joint' or 'decision', got {self.credit!r}")
        if self.credit_gamma is not None and self.credit != "decision":
            raise ValueError("credit_gamma discounts the per-decision return: it needs credit decision")
        if self.credit_baseline not in (None, "free_flow", "learned"):
            raise ValueError(f"credit_baseline must be 'free_flow' or 'learned', got {self.credit_baseline!r}")
        if self.credit_baseline is not None and self.credit != "decision":
            raise ValueError("credit_baseline names the baseline of the per-decision advantage: it needs credit decision")
        if self.credit_critic_coef is not None and self.credit != "decision":
            raise ValueError("credit_critic_coef weighs the per-decision critic's loss: it needs credit decision")
        if self.credit_scope not in (None, "headed", "due"):
            raise ValueError(f"credit_scope must be 'headed' or 'due', got {self.credit_scope!r}")
        if self.credit_scope is not None and self.credit != "decision":
            raise ValueError("credit_scope narrows the per-decision credit: it needs credit decision")
        if self.credit_horizon not in (None, "charge", "bootstrap"):
            raise ValueError(f"credit_horizon must be 'charge' or 'bootstrap', got {self.credit_horizon!r}")
        if self.credit_horizon is not None and self.credit != "decision":
            raise ValueError("credit_horizon closes the per-decision return: it needs credit decision")
        if self.credit_critic_coef is not None and self.credit_baseline != "learned":
            raise ValueError("credit_critic_coef weighs the learned per-decision critic's loss: it needs credit_baseline "
                             "learned (the free-flow baseline has nothing to train)")
        if self.credit == "decision":
            if self.credit_critic_coef is not None and not 0.0 <= float(self.credit_critic_coef) < float("inf"):
                raise ValueError(f"credit_critic_coef must be finite and >= 0, got {self.credit_critic_coef!r}")
            if self.mode != "train":
                raise ValueError("credit decision changes the PPO update: it needs mode 'train' (an evaluation has no update)")
            if self.algo not in ("mpnn", "mpnn+ppo"):
                raise ValueError("credit decision acts on vectorised training: it needs algo mpnn or mpnn+ppo")
            if self.policy_head == "embedding":
                raise ValueError("credit decision cannot train policy_head 'embedding': its rollout kernels draw the actions of "
                                 "all frames ahead of the frames, so there is no frame state whose heads could be captured; "
                                 "use a state-dependent head (edge_mlp*, embedding_dijkstra, graph_transformer, goal_mlp)")
            if self.value_head == "graph_transformer":
                raise ValueError("credit decision is not available with value_head 'graph_transformer': its observation store "
                                 "keeps every frame, and per-decision buffers for all of them are out of scope")
            if self.credit_gamma is not None and not 0.0 < float(self.credit_gamma) <= 1.0:
                raise ValueError(f"credit_gamma must be in (0, 1], got {self.credit_gamma!r}")
        if self.eval_link_counts and not (self.eval_envs or self.dijkstra_envs):
            raise ValueError("eval_link_counts counts per-road pops and withdrawals in the vectorised evaluation: it needs "
                             "eval_envs > 0 or dijkstra_envs > 0")
        if self.eval_occupancy and not (self.eval_envs or self.dijkstra_envs):
            raise ValueError("eval_occupancy sums per-road vehicle counts and frames at capacity in the vectorised "
                             "evaluation: it needs eval_envs > 0 or dijkstra_envs > 0")
        if self.eval_turns and not (self.eval_envs or self.dijkstra_envs):
            raise ValueError("eval_turns counts per-turn movements in the vectorised evaluation: it needs eval_envs > 0 or "
                             "dijkstra_envs > 0")
        if self.eval_trips and not (self.eval_envs or self.dijkstra_envs):
            raise ValueError("eval_trips reduces the agent tables of the vectorised evaluation per traveller: it needs "
                             "eval_envs > 0 or dijkstra_envs > 0")
        if self.eval_dynamic_gap and not ((self.eval_envs or self.dijkstra_envs) and self.mode == "eval"):
            raise ValueError("eval_dynamic_gap measures the trips of the vectorised evaluation against the best path in "
                             "hindsight: it needs mode 'eval' and eval_envs > 0 or dijkstra_envs > 0")
        if self.eval_paths and not ((self.eval_envs or self.dijkstra_envs) and self.mode == "eval"):
            raise ValueError("eval_paths traces every traveller's roads in the vectorised evaluation: it needs mode 'eval' and "
                             "eval_envs > 0 or dijkstra_envs > 0")
        if self.eval_paths_max_hops is not None:
            if not self.eval_paths:
                raise ValueError("eval_paths_max_hops sizes the routes of eval_paths: it needs that flag")
            if not 0 <= int(self.eval_paths_max_hops) <= 4096:
                raise ValueError(f"eval_paths_max_hops must be in [0, 4096], got {self.eval_paths_max_hops!r}")
        if self.eval_paths_routes is None or int(self.eval_paths_routes) < 0:
            raise ValueError(f"eval_paths_routes must be >= 0, got {self.eval_paths_routes!r}")
        if self.eval_paths_routes:
            if not self.eval_paths:
                raise ValueError("eval_paths_routes writes the routes of eval_paths: it needs that flag")
            if self.eval_paths_max_hops is not None and int(self.eval_paths_max_hops) == 0:
                raise ValueError("eval_paths_routes writes the kept routes: with eval_paths_max_hops 0 none is kept")
        if self.eval_dynamic_gap_envs is not None:
            if not self.eval_dynamic_gap:
                raise ValueError("eval_dynamic_gap_envs limits the environments of eval_dynamic_gap: it needs that flag")
            if not 1 <= int(self.eval_dynamic_gap_envs) <= int(self.eval_envs or self.dijkstra_envs):
                raise ValueError(f"eval_dynamic_gap_envs must be in [1, {int(self.eval_envs or self.dijkstra_envs)}] (the "
                                 f"environments of the evaluation), got {self.eval_dynamic_gap_envs!r}")
        if self.replan_days is None or int(self.replan_days) < 0:
            raise ValueError(f"replan_days must be >= 0, got {self.replan_days!r}")
        if self.replan_days and self.mode != "eval":
            raise ValueError("replan_days runs the day-to-day replanning loop after the evaluation: it needs mode 'eval'")
        if self.replan_envs is None or int(self.replan_envs) < 1:
            raise ValueError(f"replan_envs must be >= 1, got {self.replan_envs!r}")
        if self.replan_fraction != "msa" and not 0.0 < float(self.replan_fraction) <= 1.0:
            raise ValueError(f"replan_fraction must be 'msa' or in (0, 1], got {self.replan_fraction!r}")
        if self.replan_max_hops is not None and not 1 <= int(self.replan_max_hops) <= 1 << 20:
            raise ValueError(f"replan_max_hops must be in [1, 2^20], got {self.replan_max_hops!r}")
        if self.eval_link_bin is None or int(self.eval_link_bin) < 1:
            raise ValueError(f"eval_link_bin must be >= 1 second, got {self.eval_link_bin!r}")
        if int(self.iterations) < 1:
            raise ValueError(f"iterations must be >= 1, got {self.iterations!r}")
        given = [k for k in BC_FLAGS if getattr(self, k) is not None]
        if self.pretrain_bc is None or int(self.pretrain_bc) < 0:
            raise ValueError(f"pretrain_bc must be >= 0, got {self.pretrain_bc!r}")
        if given and not self.pretrain_bc:
            raise ValueError(f"{', '.join('--' + k.replace('_', '-') for k in given)} set(s) up the behaviour-cloning "
                             "iterations: it needs --pretrain-bc I with I > 0")
        if self.pretrain_bc:
            if self.mode != "train":
                raise ValueError("pretrain_bc clones the shortest-path router into the policy before training: it needs mode "
                                 "'train' (evaluate the cloned policy.pt with --checkpoint)")
            if self.algo not in ("mpnn", "mpnn+ppo"):
                raise ValueError(f"pretrain_bc trains a policy network: it needs algo mpnn or mpnn+ppo, not {self.algo!r}")
            if self.bc_expert is not None and self.bc_expert not in BC_EXPERT_NAMES:
                raise ValueError(f"bc_expert must be one of {BC_EXPERT_NAMES}, got {self.bc_expert!r}")
            if self.bc_driver is not None and self.bc_driver not in BC_DRIVER_NAMES:
                raise ValueError(f"bc_driver must be one of {BC_DRIVER_NAMES}, got {self.bc_driver!r}")
            for k in ("bc_envs", "bc_frames", "bc_samples", "bc_epochs", "bc_batch"):
                if getattr(self, k) is not None and int(getattr(self, k)) < 1:
                    raise ValueError(f"{k} must be >= 1, got {getattr(self, k)!r}")
            if self.bc_lr is not None and not float(self.bc_lr) > 0.0:
                raise ValueError(f"bc_lr must be positive, got {self.bc_lr!r}")
        if self.checkpoint is not None and self.algo in ("random", "dijkstra"):
            raise ValueError(f"checkpoint holds a policy network's parameters: not available for algo {self.algo!r}")
        from .agents.base import DijkstraAgents
        if self.dijkstra_method not in DijkstraAgents.METHODS:
            raise ValueError(f"dijkstra_method must be one of {DijkstraAgents.METHODS}, got {self.dijkstra_method!r}")
        from .agents.mpnn_agent import MPNNPolicyNet
        if self.prior_method not in MPNNPolicyNet.PRIOR_METHODS:
            raise ValueError(f"prior_method must be one of {MPNNPolicyNet.PRIOR_METHODS}, got {self.prior_method!r}")
        if self.value_head not in ("simple", "graph_transformer"):
            raise ValueError("value_head must be 'simple' or 'graph_transformer'")
        if self.value_head == "graph_transformer" and self.policy_head == "embedding":
            raise ValueError("value_head 'graph_transformer' reads the observation of every frame, which the 'embedding' "
                             "head's rollout does not build: use a state-dependent policy head (edge_mlp*, "
                             "embedding_dijkstra, graph_transformer or goal_mlp)")


EVAL_BASELINE_NAMES = ("none", "dijkstra", "dijkstra_hold", "free_flow")      # tarl_hip.evaluator.EVAL_BASELINES, and "none"
DIJKSTRA_ROUTER_NAMES = ("reference", "hold", "free_flow")                      # tarl_hip.evaluator.DIJKSTRA_ROUTERS

BC_FLAGS = ("bc_expert", "bc_driver", "bc_envs", "bc_frames", "bc_samples", "bc_epochs", "bc_batch", "bc_lr")
BC_EXPERT_NAMES = ("dijkstra", "free_flow")      # tarl_hip.imitation.EXPERTS
BC_DRIVER_NAMES = ("expert", "policy", "dagger")  # tarl_hip.imitation.DRIVERS

CHECKPOINT_PREFIX = "module.0.module."      # ProbabilisticActor -> TensorDictModule -> the network (ppo_train's keys)


def checkpoint_state(file_state, expected):
    """Map the state dict of a ``policy.pt`` written by ``ppo_train`` (keys ``module.0.module.<name>``, ``gt_pe`` among them
    where the network has one) onto a network whose ``state_dict()`` is ``expected``: -> {name: tensor}. A file whose keys
    or shapes do not match the network exactly is refused, with the offending key named."""
    mapped = {}
    for k, v in file_state.items():
        if not k.startswith(CHECKPOINT_PREFIX):
            raise ValueError(f"checkpoint key {k!r} does not start with {CHECKPOINT_PREFIX!r}: not a policy.pt of ppo_train")
        name = k[len(CHECKPOINT_PREFIX):]
        if name not in expected:
            raise ValueError(f"checkpoint key {k!r} has no counterpart in the network (policy head / graph mismatch?)")
        if tuple(v.shape) != tuple(expected[name].shape):
            raise ValueError(f"checkpoint key {k!r} has shape {tuple(v.shape)}, the network's {name!r} has "
                             f"{tuple(expected[name].shape)}")
        mapped[name] = v
    for name in expected:
        if name not in mapped:
            raise ValueError(f"the network's {name!r} is missing from the checkpoint (no key {CHECKPOINT_PREFIX + name!r})")
    return mapped


class Runner:
    def __init__(self, args: RunnerArgs):
        self.args = args
        # one process per GPU under torchrun: join the process group (backend nccl = RCCL) and bind this rank's device
        # BEFORE any GPU work; a single process (WORLD_SIZE unset) skips all of it
        from tarl_hip import dist_utils
        self.rank, self.world, local = dist_utils.init_from_env()
        # the path runs on the GPU only: "cuda" on ROCm is the HIP device
        if torch.cuda.is_available():
            local = local % torch.cuda.device_count()
            torch.cuda.set_device(local)
            self.device = torch.device("cuda", local)
        else:
            self.device = torch.device(args.device)
        torch.manual_seed(args.seed)          # identical initial weights on every rank (also broadcast by the trainer)

    def close(self, failed=False):
        """Leave the process group (if this process joined one). ``failed``: this rank is on its way out with an
        exception — no barrier (the peers are in other collectives), and a communicator that cannot be destroyed cleanly
        is left to the launcher, which kills the job when this process exits non-zero."""
        import torch.distributed as dist
        from tarl_hip import dist_utils
        if self.world > 1 and dist.is_initialized():
            if failed:
                try:
                    dist.destroy_process_group()
                except Exception:      # noqa: BLE001 — the original exception is the one to report
                    pass
                return
            dist_utils.barrier()
            dist.destroy_process_group()

    def setup(self):
        from .reinforcement_learning import SimulatorEnv
        from .transportation_simulator import TransportationSimulator
        from .agents.base import Agents, DijkstraAgents
        a = self.args
        if a.algo in {"dijkstra", "random"}:
            self.simulator = TransportationSimulator(str(self.device), torch_compile=a.torch_compile)
            self.simulator.load_network(scenario=a.scenario)
            if a.algo == "dijkstra":
                self.agent = DijkstraAgents(str(self.device), method=a.dijkstra_method)
            else:
                self.agent = Agents(str(self.device))
            self.simulator.agent = self.agent
            self.agent.load(scenario=a.scenario)
            self.simulator.config_parameters(timestep_size=a.timestep_size, start_time=a.start_end_time[0])
            self.agent.set_time(a.start_end_time[0])
            if a.dijkstra_envs:
                from tarl_hip import ops
                if not ops.fused_path_supported(self.simulator.graph.edge_index, self.simulator.Nmax):
                    raise ValueError("--dijkstra-envs needs the packed (fused) path, which cannot represent this graph (Nmax "
                                     "> 127, an out-degree above 126 or parallel edges); there is no fall-back for the "
                                     "vectorised evaluation: run without --dijkstra-envs")
                # the population as loaded: the single-environment pass below marks its agents on the way / arrived
                self._dijkstra_population = self.agent.agent_features.clone()
            if a.replan_days:
                self._replan_setup(self.simulator.graph.edge_index, self.simulator.Nmax, self.agent.agent_features)
        elif a.algo in {"mpnn", "mpnn+ppo"}:
            from .agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
            self.env = SimulatorEnv(device=str(self.device), timestep_size=a.timestep_size,
                                    start_time=a.start_end_time[0], scenario=a.scenario, torch_compile=a.torch_compile)
            g, h = self.env.simulator.graph, self.env.simulator.h
            free_flow = g.x[:, h.FREE_FLOW_TIME_TRAVEL][g.edge_index[1]]
            self.policy_net = MPNNPolicyNet(g.edge_index, g.x.size(0), free_flow, device=str(self.device))
            self.policy_net.policy_head = a.policy_head
            self.policy_net.prior_weight = float(a.prior_weight)
            self.policy_net.prior_method = a.prior_method
            pe = None
            if "graph_transformer" in (a.policy_head, a.value_head):
                from .transformer import cached_laplacian_pe
                # on the road graph (MLAgents: edge_index_routes, num_roads); the SRC / DEST rows stay zero
                roads = int(getattr(g, "num_roads", None) or g.x.size(0))
                routes = getattr(g, "edge_index_routes", None)
                cache = None if a.scenario.startswith("synthetic") else str(Path("save") / a.scenario)
                pe = cached_laplacian_pe(g.edge_index if routes is None else routes, roads, g.x.size(0), cache)
            if a.policy_head == "graph_transformer":
                self.policy_net.use_graph_transformer(pe)
            if a.policy_head == "goal_mlp":      # the time scale: the mean free-flow time of the graph's rows
                from tarl_hip import ops
                self.policy_net.use_goal_mlp(ops.goal_time_scale(g.x[:, 3 * self.env.simulator.Nmax:]))
            self.policy_net.load(a.scenario)
            if a.value_head == "graph_transformer":
                from .agents.transformer_agent import ValueNet
                # the same encoding as the policy's (ValueNet is an MLAgents: compute_encodings on the same road graph)
                self.value_net = ValueNet(g.edge_index, g.x.size(0), str(self.device), pe)
            else:
                self.value_net = MPNNValueNetSimple(g.edge_index, g.x.size(0), device=str(self.device))
            self.value_net.load(a.scenario)
            self.env.simulator.agent = self.policy_net     # the policy IS the population store used by the env
            if a.eval_envs:
                from tarl_hip import ops
                if not ops.fused_path_supported(g.edge_index, self.env.simulator.Nmax):
                    raise ValueError("--eval-envs needs the packed (fused) path, which cannot represent this graph (Nmax > "
                                     "127, an out-degree above 126 or parallel edges); there is no fall-back for the "
                                     "vectorised evaluation: run without --eval-envs")
            if a.pretrain_bc:
                from tarl_hip import ops
                if not ops.fused_path_supported(g.edge_index, self.env.simulator.Nmax):
                    raise ValueError("--pretrain-bc needs the packed (fused) path, which cannot represent this graph (Nmax > "
                                     "127, an out-degree above 126 or parallel edges); there is no fall-back for behaviour "
                                     "cloning: run without --pretrain-bc")
            if a.replan_days:
                self._replan_setup(g.edge_index, self.env.simulator.Nmax, self.policy_net.agent_features)
            if a.checkpoint is not None:
                self.load_checkpoint(a.checkpoint)
        else:
            raise ValueError(f"Unknown algorithm {a.algo}")

    def _replan_setup(self, edge_index, Nmax, agent_features):
        """--replan-days: refuse a graph the packed path cannot hold, and keep the population as loaded (the passes before the
        loop mark their agents on the way / arrived)."""
        from tarl_hip import ops
        if not ops.fused_path_supported(edge_index, Nmax):
            raise ValueError("--replan-days needs the packed (fused) path, which cannot represent this graph (Nmax > 127, an "
                             "out-degree above 126 or parallel edges); there is no fall-back: run without --replan-days")
        self._replan_population = agent_features.clone()

    def load_checkpoint(self, path):
        """Load a ``policy.pt`` written by ``ppo_train`` into the policy network (in place: views held elsewhere stay valid)."""
        state = torch.load(path, map_location=self.device)
        with torch.no_grad():
            own = self.policy_net.state_dict()
            for name, v in checkpoint_state(state, own).items():
                own[name].copy_(v)

    def _actor(self, return_log_prob):
        from .reinforcement_learning import GraphDistribution
        from .rl.modules import ProbabilisticActor, TensorDictModule
        inner = TensorDictModule(self.policy_net, in_keys=["node_features", "edge_features", "agent_index"],
                                 out_keys=["logits"])
        return ProbabilisticActor(module=inner, spec=self.env.action_spec, distribution_class=GraphDistribution,
                                  in_keys=["logits"],
                                  distribution_kwargs={"edge_index": self.env.simulator.graph.edge_index},
                                  return_log_prob=return_log_prob)

    def train(self):
        a = self.args
        bc_only = a.algo == "mpnn" and a.mode == "train" and bool(a.pretrain_bc)      # cloning alone: no PPO iteration follows
        if not (a.algo == "mpnn+ppo" and a.mode == "train") and not bc_only:
            raise RuntimeError("Training is only supported for algo 'mpnn+ppo' (and, with --pretrain-bc, 'mpnn')")
        from .rl.modules import TensorDictModule, ValueOperator
        from .rl.ppo_trainer import ppo_train
        policy_module = self._actor(return_log_prob=True)
        value_module = ValueOperator(TensorDictModule(self.value_net,
                                                      in_keys=["node_features", "edge_features", "agent_index", "time"],
                                                      out_keys=["value"]),
                                     in_keys=["node_features", "edge_features", "agent_index", "time"])
        # the evaluation environment of the reference's Runner.train (src/runner.py:111-118): a second SimulatorEnv that
        # shares the policy (= the population store)
        from .reinforcement_learning import SimulatorEnv
        eval_env = SimulatorEnv(device=str(self.device), timestep_size=a.timestep_size, start_time=a.start_end_time[0],
                                scenario=a.scenario, torch_compile=a.torch_compile)
        eval_env.simulator.agent = self.policy_net
        out = Path(a.output_dir)
        if self.rank == 0:
            out.mkdir(parents=True, exist_ok=True)
        # rank 0 alone writes the checkpoint and the logs; every rank takes part in the training collectives
        bc_kw = {}
        if a.pretrain_bc:
            bc_kw["pretrain_bc"] = dict(iterations=int(a.pretrain_bc), expert=a.bc_expert or "dijkstra",
                                        driver=a.bc_driver or "dagger", envs=a.bc_envs or 16,
                                        frames=a.bc_frames or a.rollout_steps, samples=a.bc_samples or 256,
                                        epochs=a.bc_epochs or 4, batch=a.bc_batch, lr=a.bc_lr)
        ppo_train(self.env, policy_module, value_module, total_frames=0 if bc_only else a.total_frames,
                  frames_per_batch=a.rollout_steps, num_epochs=a.epochs, device=self.device,
                  checkpoint_path=(out / "policy.pt") if self.rank == 0 else None,
                  log_dir=str(out) if self.rank == 0 else None, eval_env=eval_env, eval_interval=1,
                  num_envs=a.num_envs, seed=a.seed, eval_envs=a.eval_envs, stochastic_eval=a.eval_sampled,
                  eval_baseline=a.eval_baseline, **({"policy_hold": True} if a.policy_hold else {}),
                  **({"route_departures": True} if a.route_departures else {}),
                  **({"reward": "trip"} if a.reward == "trip" else {}),
                  **({"credit": "decision", "decision_gamma": 1.0 if a.credit_gamma is None else float(a.credit_gamma)}
                     if a.credit == "decision" else {}),
                  **({"credit_baseline": "learned",
                      "decision_critic_coef": 1.0 if a.credit_critic_coef is None else float(a.credit_critic_coef)}
                     if a.credit_baseline == "learned" else {}),
                  **({"credit_scope": "due"} if a.credit_scope == "due" else {}),
                  **({"credit_horizon": "bootstrap"} if a.credit_horizon == "bootstrap" else {}), **bc_kw)

    def eval(self):
        a = self.args
        n = a.steps if a.steps is not None else (a.start_end_time[1] - a.start_end_time[0]) // a.timestep_size
        if a.algo in {"dijkstra", "random"}:
            for _ in range(n):
                self.simulator.run()
            sim, agent = self.simulator, self.agent
        else:
            with torch.no_grad():
                self.env.rollout(n, self._actor(return_log_prob=False), break_when_any_done=False)
            sim, agent = self.env.simulator, self.env.simulator.agent
        mask = agent.agent_features[:, agent.DONE] == 1
        tt = agent.agent_features[mask, agent.ARRIVAL_TIME] - agent.agent_features[mask, agent.DEPARTURE_TIME]
        avg = float(tt.mean()) if bool(mask.any()) else float("nan")
        total = sim.inserting_time + sim.choice_time + sim.core_time + sim.withdraw_time
        if self.rank != 0:      # every rank evaluated its replica; one summary / one set of metric tables
            return {"steps": n, "arrived": int(mask.sum()), "avg_travel_time": avg}
        print("\n=== Simulation Summary ===")
        print(f"{'Steps:':25} {n:10d}")
        print(f"{'Agents arrived:':25} {int(mask.sum()):10d}")
        print(f"{'Average travel time:':25} {avg:10.2f} s")
        for label, v in (("Agent Insertion time:", sim.inserting_time), ("Route Choice time:", sim.choice_time),
                         ("Core Model time:", sim.core_time), ("Agent Withdrawal time:", sim.withdraw_time)):
            print(f"{label:25} {v:10.2f} s   (host enqueue time; kernels run asynchronously)")
        print("-" * 42)
        print(f"{'Total simulation time:':25} {total:10.2f} s")
        # the reference's eval report (src/runner.py:166-174, 219-226): phase-time pie, node metrics, leg histogram, road
        # optimality, and the simulated daily counts against the MSA assignment's expected flows
        out_dir = Path(a.output_dir)
        self._link_expected = {}        # the flow vectors computed below, handed on to the link-count report
        try:
            sim.plot_computation_time(str(out_dir))
            sim.compute_node_metrics(str(out_dir))
            sim.plot_leg_histogram(str(out_dir))
            sim.plot_road_optimality(str(out_dir))
            from .algorithms.user_equilibrium_msa import run_msa
            expected = run_msa(sim.graph, agent)         # all-pairs table on mid-size graphs, per-origin trees above
            out_dir.mkdir(parents=True, exist_ok=True)
            with open(out_dir / "msa_expected_flows.csv", "w") as f:
                f.write("road,expected_hourly_flow\n")
                f.writelines(f"{r},{v}\n" for r, v in expected.items())
            sim.plot_daily_counts(expected, str(out_dir))
            self._link_expected["msa"] = expected
            if a.equilibrium_metrics:
                self._equilibrium_metrics(sim.graph, agent, expected, out_dir)
            import matplotlib.pyplot as plt
            plt.close("all")
        except Exception as exc:  # noqa: BLE001 - analysis output must not fail the run
            print(f"metric tables / figures skipped: {exc}")
        result = {"steps": n, "arrived": int(mask.sum()), "avg_travel_time": avg}
        if a.eval_envs and a.algo in {"mpnn", "mpnn+ppo"}:
            result["vectorised"] = self._vectorised_eval(n, out_dir)
        elif a.dijkstra_envs and a.algo == "dijkstra":
            result["vectorised"] = self._vectorised_dijkstra(n, out_dir)
        if a.replan_days:
            result["replanning"] = self._replanning(n, out_dir, sim, result.get("vectorised"))
        return result

    def _eval_engine(self, sim, agent_features, num_envs):
        """A fused engine of its own for a vectorised evaluation: copies of the graph state and of the agent table, noise
        seed ``seed + 104729``. Two such engines see the same noise streams (common random numbers)."""
        from tarl_hip.engine import SimEngine
        g = sim.graph
        return SimEngine(g.x.clone(), g.edge_index, g.edge_attr, sim.Nmax, agent_features.clone(),
                         congestion_constant=getattr(g, "congestion_constant", None), num_envs=int(num_envs),
                         device=g.x.device, timestep=sim.timestep, seed=self.args.seed + 104729, fused=True)

    @staticmethod
    def _print_block(title, res):
        print(f"\n=== {title} ===")
        print(f"{'frames:':22} {res.frames_run:12d}   ({res.computation_time_ms:.1f} ms)")
        for line in res.summary_lines():
            print(line)

    def _link_kw(self):
        a = self.args
        kw = dict(link_counts=True, link_bin_seconds=a.eval_link_bin) if a.eval_link_counts else {}
        if a.eval_occupancy:
            kw.update(occupancy=True, link_bin_seconds=a.eval_link_bin)
        if a.eval_trips:        # the free-flow edge weights are those the policy net's shortest-path prior is built from
            sim = self.simulator if a.algo == "dijkstra" else self.env.simulator
            g, h = sim.graph, sim.h
            kw.update(trips=True, link_bin_seconds=a.eval_link_bin,
                      trip_free_flow=g.x[:, h.FREE_FLOW_TIME_TRAVEL][g.edge_index[1]])
        if a.eval_dynamic_gap:
            kw.update(dynamic_gap=True, dynamic_gap_envs=a.eval_dynamic_gap_envs, link_bin_seconds=a.eval_link_bin)
        if a.eval_turns:
            kw.update(turns=True, link_bin_seconds=a.eval_link_bin)
        if a.eval_paths:        # cost and detour under the free-flow weights of the per-trip report
            sim = self.simulator if a.algo == "dijkstra" else self.env.simulator
            g, h = sim.graph, sim.h
            kw.update(paths=True, path_max_hops=a.eval_paths_max_hops, link_bin_seconds=a.eval_link_bin,
                      path_weights=g.x[:, h.FREE_FLOW_TIME_TRAVEL][g.edge_index[1]])
        return kw

    @staticmethod
    def _report_output(title, report, lines_fn, summary_fn, tables):
        """One report of the vectorised evaluation: its ``title`` block and, where it is available, one CSV file per
        ``(path, columns_key, rows_key)`` of ``tables`` -> the summary for the JSON file (never a table or a tensor)."""
        import csv
        print(f"\n=== {title} ===")
        for line in lines_fn(report):
            print(line)
        if report["available"]:
            for path, columns, rows in tables:
                with open(path, "w", newline="") as f:
                    w = csv.DictWriter(f, fieldnames=report[columns])
                    w.writeheader()
                    w.writerows(report[rows])
        return summary_fn(report)

    def _reports_output(self, doc, res, baseline, out_dir, prefix):
        """--eval-link-counts, --eval-turns, --eval-occupancy, --eval-trips, --eval-dynamic-gap, --eval-paths: each report of ``res`` (against ``baseline``, the evaluation of
        the same environments, where there is one) printed, written to ``<prefix>_<report>.csv`` (one row per road; the
        link counts with the expected flows that Runner.eval computed; the trips one row per agent, and per departure bin in
        ``<prefix>_trips_by_departure.csv``; the turns one row per route edge, and per road with a loss in
        ``<prefix>_turns_lost.csv``) and summarised in ``doc``."""
        from tarl_hip import evaluator as E
        a = self.args
        if a.eval_link_counts:
            rep = E.link_count_report(res, expected=getattr(self, "_link_expected", {}), baseline=baseline)
            doc["link_counts"] = self._report_output("Link counts", rep, E.link_count_lines, E.link_count_summary,
                                                     [(out_dir / f"{prefix}_link_counts.csv", "columns", "rows")])
        if a.eval_turns:
            doc["turns"] = self._report_output("Turns", E.turn_report(res, baseline=baseline), E.turn_lines, E.turn_summary,
                                               [(out_dir / f"{prefix}_turns.csv", "columns", "rows"),
                                                (out_dir / f"{prefix}_turns_lost.csv", "lost_columns", "lost_rows")])
        if a.eval_occupancy:
            doc["occupancy"] = self._report_output("Occupancy", E.occupancy_report(res, baseline=baseline), E.occupancy_lines,
                                                   E.occupancy_summary, [(out_dir / f"{prefix}_occupancy.csv", "columns", "rows")])
        if a.eval_trips:
            doc["trips"] = self._report_output(
                "Trips", E.trip_report(res, baseline=baseline), E.trip_lines, E.trip_summary,
                [(out_dir / f"{prefix}_trips.csv", "columns", "rows"),
                 (out_dir / f"{prefix}_trips_by_departure.csv", "by_departure_columns", "by_departure")])
        if a.eval_dynamic_gap:
            from functools import partial
            rep = E.dynamic_gap_report(res, baseline=baseline)
            doc["dynamic_gap"] = self._report_output(
                "Dynamic gap", rep, partial(E.dynamic_gap_lines, paired=False), E.dynamic_gap_summary,
                [(out_dir / f"{prefix}_dynamic_gap.csv", "columns", "rows"),
                 (out_dir / f"{prefix}_dynamic_gap_by_departure.csv", "by_departure_columns", "by_departure")])
            if baseline is not None:      # the baseline's own block, then the paired difference of the relative gap
                doc["dynamic_gap"]["baseline"] = self._report_output(
                    f"Dynamic gap: baseline ({baseline.head})", E.dynamic_gap_report(baseline), E.dynamic_gap_lines,
                    E.dynamic_gap_summary, [(out_dir / f"{prefix}_dynamic_gap_baseline.csv", "columns", "rows")])
                print("\n=== Dynamic gap: policy \u2212 baseline (paired) ===")
                for line in E.dynamic_gap_paired_lines(rep):
                    print(line)
        if a.eval_paths:
            doc["paths"] = self._report_output(
                "Paths", E.path_report(res, baseline=baseline), E.path_lines, E.path_summary,
                [(out_dir / f"{prefix}_paths.csv", "columns", "rows"),
                 (out_dir / f"{prefix}_paths_by_departure.csv", "by_departure_columns", "by_departure")])
            if baseline is not None:      # the baseline's own block and file
                doc["paths"]["baseline"] = self._report_output(
                    f"Paths: baseline ({baseline.head})", E.path_report(baseline), E.path_lines, E.path_summary,
                    [(out_dir / f"{prefix}_paths_baseline.csv", "columns", "rows")])
            if a.eval_paths_routes and res.path_routes is not None:
                import csv
                with open(out_dir / f"{prefix}_paths_routes.csv", "w", newline="") as f:
                    w = csv.DictWriter(f, fieldnames=("env", "agent", "roads", "truncated", "route"))
                    w.writeheader()
                    w.writerows(E.path_route_rows(res, a.eval_paths_routes))

    def _replanning(self, frames, out_dir, sim, vectorised):
        """--replan-days J: the day-to-day replanning loop (tarl_hip.replanning.Replanner; not in the reference) on
        --replan-envs environments of a fused engine of its own, ``frames`` frames per day: a ``Replanning`` block with the
        day table and the last day's aggregate under the name ``routes``; replan_days.csv (one row per day), replan_envs.json
        (settings, day records, the last day's aggregate) and replan_envs.csv (one row per environment of the last day);
        replan_<report>.csv for every --eval-* report flag that is set. Where --eval-envs equals --replan-envs the policy's
        MODE run is paired with the last day (same seed: common random numbers). -> {"result": ReplanResult[, "paired"]}."""
        import csv
        import json
        from tarl_hip.evaluator import PER_ENV_KEYS, paired_lines, paired_report
        from tarl_hip.replanning import Replanner, replan_lines, replan_report
        a = self.args
        kw = {k: v for k, v in self._link_kw().items() if k not in ("occupancy", "dynamic_gap", "dynamic_gap_envs",
                                                                    "link_bin_seconds")}
        engine = self._eval_engine(sim, self._replan_population, a.replan_envs)
        rp = Replanner(engine, days=a.replan_days, fraction=a.replan_fraction, max_hops=a.replan_max_hops,
                       link_bin_seconds=a.eval_link_bin, seed=a.seed, **self._departures_kw(engine), **self._trip_kw(), **kw)
        result = rp.run(frames)
        rep = replan_report(result)
        print(f"\n=== Replanning ({a.replan_days} days, {a.replan_envs} environments) ===")
        for line in replan_lines(rep):
            print(line)
        out_dir.mkdir(parents=True, exist_ok=True)
        with open(out_dir / "replan_days.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=rep["columns"])
            w.writeheader()
            w.writerows(rep["rows"])
        doc = {"settings": rep["settings"], "days": rep["rows"], "days_per_env": rep["env_rows"], "note": rep["note"],
               "domain_exit_day": rep["domain_exit_day"]}
        out, rows = {"result": result}, []
        last = result.last
        if last is not None:
            self._print_block(f"Vectorised evaluation ({last.envs} environments, routes, last day)", last)
            doc["routes"] = last.to_dict()
            self._departures_output(doc["routes"], last)
            self._trip_output(doc["routes"], last)
            rows = [dict(kind="routes", **r) for r in last.rows()]
            self._reports_output(doc, last, None, out_dir, "replan")
            mode = (vectorised or {}).get("mode")
            if mode is not None and a.algo in {"mpnn", "mpnn+ppo"} and a.eval_envs == a.replan_envs:
                out["paired"] = doc["paired"] = paired_report(mode, last)
                print("\n=== Policy \u2212 replanned (paired) ===")
                for line in paired_lines(out["paired"]):
                    print(line)
        with open(out_dir / "replan_envs.json", "w") as f:
            json.dump(doc, f, indent=1)
        with open(out_dir / "replan_envs.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=("kind", "env") + PER_ENV_KEYS + self._trip_fields())
            w.writeheader()
            w.writerows(rows)
        return out

    def _departures_kw(self, engine):
        """--route-departures for an evaluator on ``engine``: the keyword, after the one refusal that needs the graph."""
        if not self.args.route_departures:
            return {}
        if engine.fs is None:
            raise ValueError("route_departures rewrites the packed state's SELECTED_ROAD bytes: this graph cannot be held by "
                             "the packed path (Nmax <= 127, out-degree <= 126, no parallel edges); run without the flag")
        return {"route_departures": True}

    def _trip_kw(self):
        """--reward trip for an evaluator: the keyword."""
        return {"trip_reward": True} if self.args.reward == "trip" else {}

    def _trip_fields(self):
        """... and the column it adds to the per-environment CSV files."""
        return ("trip_return",) if self.args.reward == "trip" else ()

    def _trip_output(self, doc, res):
        """One more line in the block just printed, and ``trip_return`` (per environment) / ``trip_parts_last`` in its JSON
        entry; the aggregate's ``trip_return`` is already in ``doc["aggregate"]``."""
        if self.args.reward != "trip" or res.trip_return is None:      # (a domain exit: no statistics)
            return
        doc["trip_return"] = list(res.trip_return)
        doc["trip_parts_last"] = [[int(v) for v in row] for row in res.trip_parts_last]
        on_way, ready = res.trip_parts_last.mean(axis=0)
        print(f"{'trip reward:':22} after the last frame {on_way:.1f} agents on the way and {ready:.1f} due and waiting per "
              f"environment still owe their trip (DESIGN 4.24)")

    def _departures_output(self, doc, res):
        """One more line in the block just printed, and ``route_departures`` / ``departures_routed`` in its JSON entry."""
        if not self.args.route_departures:
            return
        from tarl_hip.evaluator import aggregate
        doc["route_departures"] = True
        if res.departures_routed is None:       # (a domain exit: no statistics)
            print(f"{'departures routed:':22} ran with the first-hop rule (DESIGN 4.23)")
            return
        g = aggregate([int(v) for v in res.departures_routed])
        doc["departures_routed"] = [int(v) for v in res.departures_routed]
        print(f"{'departures routed:':22} {g['mean']:.1f}" + (f" \u00b1 {g['se']:.1f} (se)" if g.get("se") is not None else "")
              + " empty origin roads per environment selected for their departing agent (DESIGN 4.23)")

    def _vectorised_dijkstra(self, frames, out_dir):
        """--dijkstra-envs K: the shortest-path router on K environments of a fused engine (VecEvaluator, head "dijkstra", or
        "dijkstra_hold" with --dijkstra-router hold / free_flow:
        every environment routes on its own congested travel times, in the environment's step order) for the same number of
        frames as the pass above; prints the aggregate block, writes dijkstra_envs.json / dijkstra_envs.csv in the format of
        eval_envs.*. -> {"mode": EvalResult}."""
        import csv
        import json
        from tarl_hip.evaluator import DIJKSTRA_ROUTERS, PER_ENV_KEYS, VecEvaluator, router_label
        engine = self._eval_engine(self.simulator, self._dijkstra_population, self.args.dijkstra_envs)
        head, refresh = DIJKSTRA_ROUTERS[self.args.dijkstra_router]      # --dijkstra-router: reference / hold / free_flow
        res = VecEvaluator(engine, head, refresh_rate=self.agent.refresh_rate if refresh is None else refresh,
                           **self._departures_kw(engine), **self._trip_kw(), **self._link_kw()).run(frames)
        self._print_block(f"Vectorised evaluation ({res.envs} environments, {router_label(res)})", res)
        out_dir.mkdir(parents=True, exist_ok=True)
        doc = {"mode": res.to_dict()}
        self._departures_output(doc["mode"], res)
        self._trip_output(doc["mode"], res)
        self._reports_output(doc, res, None, out_dir, "dijkstra")
        with open(out_dir / "dijkstra_envs.json", "w") as f:
            json.dump(doc, f, indent=1)
        with open(out_dir / "dijkstra_envs.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=("kind", "env") + PER_ENV_KEYS + self._trip_fields())
            w.writeheader()
            w.writerows(dict(kind="mode", **r) for r in res.rows())
        return {"mode": res}

    def _vectorised_eval(self, frames, out_dir):
        """--eval-envs K: the policy on K environments of a fused engine of its own (copies of the graph state and the agent
        table; noise seed ``seed + 104729``) for the same number of frames as the pass above, MODE and with --eval-sampled
        also sampled: prints the aggregate block(s), writes eval_envs.json (aggregate + settings) and eval_envs.csv (one row
        per environment). With --eval-baseline dijkstra (dijkstra_hold, free_flow: the routers of DESIGN 4.13a, titled by their
        head's name) the shortest-path router then runs on a second engine of the same seed,
        K and population: a ``Baseline (dijkstra)`` block, a paired block, ``baseline`` / ``paired`` in the JSON, ``baseline_*``
        columns in the CSV. -> {"mode": EvalResult, "sampled": EvalResult or None[, "baseline": EvalResult, "paired": dict]}."""
        import csv
        import json
        from tarl_hip.evaluator import PER_ENV_KEYS, VecEvaluator, aggregate
        from .agents.base import destination_set
        a, sim = self.args, self.env.simulator
        engine = self._eval_engine(sim, self.policy_net.agent_features, a.eval_envs)
        dests = None
        if a.policy_head in ("embedding_dijkstra", "goal_mlp") and self.policy_net.resolve_prior_method() != "all_pairs":
            dests = destination_set(engine.agents, engine.N)
        ev = VecEvaluator.from_policy_net(engine, self.policy_net, prior_dests=dests, **self._link_kw(),
                                          **({"policy_hold": True} if a.policy_hold else {}), **self._departures_kw(engine),
                                          **self._trip_kw())
        results = {"mode": ev.run(frames, deterministic=True), "sampled": None}
        pair = None
        if a.eval_trips and a.eval_baseline != "none" and not results["mode"].domain_exit:
            # the MODE run's agent tables, for the baseline's paired launch: a sampled run would overwrite them
            pair = engine.agents.clone() if a.eval_sampled else engine.agents
        path_pair = None
        if a.eval_paths and a.eval_baseline != "none" and not results["mode"].domain_exit:      # likewise, the MODE run's trace
            path_pair = ((ev.path_state.clone(), engine.agents.clone()) if a.eval_sampled else (ev.path_state, engine.agents))
        if a.eval_sampled:
            results["sampled"] = ev.run(frames, deterministic=False)
        doc, rows = {}, []
        for key, label in (("mode", "MODE"), ("sampled", "sampled")):
            res = results[key]
            if res is None:
                continue
            self._print_block(f"Vectorised evaluation ({res.envs} environments, {label})", res)
            doc[key] = res.to_dict()
            if a.policy_hold:           # only the policy's engine: the baseline and the replanning loop keep their own rule
                doc[key]["policy_hold"] = True
                if res.held is not None:
                    g = aggregate([int(v) for v in res.held])
                    doc[key]["held"] = [int(v) for v in res.held]
                    print(f"{'policy hold:':22} ran with the hold rule on the policy's action (DESIGN 4.20); rows held per "
                          f"environment {g['mean']:.1f}" + (f" \u00b1 {g['se']:.1f} (se)" if g.get("se") is not None else ""))
                else:
                    print(f"{'policy hold:':22} ran with the hold rule on the policy's action (DESIGN 4.20)")
            self._departures_output(doc[key], res)
            self._trip_output(doc[key], res)
            rows += [dict(kind=key, **r) for r in res.rows()]
        fields = ("kind", "env") + PER_ENV_KEYS + self._trip_fields()
        if a.eval_baseline != "none":
            # the router on a second engine with the same seed, K and population: the same noise streams as the policy run
            from tarl_hip.evaluator import EVAL_BASELINES, paired_lines, paired_report, router_label
            b_head, b_kw = EVAL_BASELINES[a.eval_baseline]      # dijkstra / dijkstra_hold / free_flow (hold, static tables)
            base = VecEvaluator(self._eval_engine(sim, self.policy_net.agent_features, a.eval_envs), b_head,
                                **b_kw, **self._departures_kw(engine), **self._trip_kw(), **self._link_kw()).run(frames, trip_pair=pair, path_pair=path_pair)
            rep = paired_report(results["mode"], base)
            self._print_block(f"Baseline ({router_label(base)})", base)
            print("\n=== Policy \u2212 baseline (paired) ===")
            for line in paired_lines(rep):
                print(line)
            results["baseline"], results["paired"] = base, rep
            doc["baseline"], doc["paired"] = base.to_dict(), rep
            self._departures_output(doc["baseline"], base)
            self._trip_output(doc["baseline"], base)
            b_keys = PER_ENV_KEYS + self._trip_fields()
            fields += tuple(f"baseline_{k}" for k in b_keys)
            by_env = {r["env"]: r for r in base.rows()}
            for r in rows:
                r.update({f"baseline_{k}": by_env[r["env"]][k] for k in b_keys} if r["env"] in by_env else {})
        out_dir.mkdir(parents=True, exist_ok=True)
        self._reports_output(doc, results["mode"], results.get("baseline"), out_dir, "eval")      # of the MODE run
        with open(out_dir / "eval_envs.json", "w") as f:
            json.dump(doc, f, indent=1)
        with open(out_dir / "eval_envs.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=fields)
            w.writeheader()
            w.writerows(rows)
        return results

    def _equilibrium_metrics(self, graph, agent, msa_flows, out_dir):
        """--equilibrium-metrics: solve the user equilibrium and the system optimum of run_msa's static model, print the
        block below the summary and write equilibrium_metrics.json / equilibrium_flows.csv beside msa_expected_flows.csv.
        A Price of Anarchy is only ever shown with both gaps and its interval."""
        import json
        from .algorithms.equilibrium import assignment_gap, equilibrium_report
        a = self.args
        rep = equilibrium_report(graph, agent, gap_tol=a.equilibrium_gap, max_iter=a.equilibrium_max_iter)
        msa = assignment_gap(graph, agent, msa_flows, objective="ue")
        ue, so = rep["ue"], rep["so"]
        lo, hi = rep["price_of_anarchy_interval"]
        print("\n=== Equilibrium Metrics (static BPR model of the MSA step) ===")
        for label, r in (("User equilibrium:", ue), ("System optimum:", so)):
            state = "converged" if r["converged"] else "NOT converged"
            print(f"{label:25} TSTT {r['tstt']:.6g} s, relative gap {r['relative_gap']:.3e} after {r['iterations']} "
                  f"{r['solver']} iterations ({state} to {a.equilibrium_gap:g})")
        print(f"{'Price of Anarchy:':25} {rep['price_of_anarchy']:.6f} in [{lo:.6f}, {hi:.6f}] "
              f"(gaps: UE {ue['relative_gap']:.3e}, SO {so['relative_gap']:.3e}; lower bound on the optimal TSTT "
              f"{rep['tstt_lower_bound']:.6g} s)")
        print(f"{'MSA flows (run_msa):':25} TSTT {msa.tstt:.6g} s, relative gap {msa.relative_gap:.3e}")
        print(f"{'Unrouted volume:':25} {rep['unrouted_volume']:.0f} of {ue['routed_volume'] + ue['unrouted_volume']:.0f} trips")
        doc = {k: rep[k] for k in ("ue", "so", "price_of_anarchy", "price_of_anarchy_interval", "relative_gap_ue",
                                   "relative_gap_so", "tstt_ue", "tstt_so", "tstt_lower_bound", "unrouted_volume")}
        doc["msa"] = msa.scalars()
        doc["gap_tol"], doc["max_iter"] = a.equilibrium_gap, a.equilibrium_max_iter
        with open(out_dir / "equilibrium_metrics.json", "w") as f:
            json.dump(doc, f, indent=1)
        with open(out_dir / "equilibrium_flows.csv", "w") as f:
            f.write("road,ue_flow,so_flow\n")
            f.writelines(f"{r},{v},{rep['so_flows'][r]}\n" for r, v in rep["ue_flows"].items())
        if hasattr(self, "_link_expected"):
            self._link_expected.update(ue=rep["ue_flows"], so=rep["so_flows"])
