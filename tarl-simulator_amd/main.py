"""Command line of the MI355X build. The flag set is the reference CLI's contract (main.py of the reference: --algo,
--scenario, --mode, --timestep_size, --start-end-time, --epochs, --rollout-steps, --seed, --device, --output-dir,
--profile, --torch-compile) plus ``--steps`` (used by the reference's README but missing from its parser) and
``--num-envs`` (vectorised environments per GPU), ``--policy-head``, ``--value-head``, ``--prior-method``,
``--dijkstra-method``, ``--equilibrium-metrics`` (with ``--equilibrium-gap`` / ``--equilibrium-max-iter``), ``--iterations``,
``--checkpoint``, the vectorised evaluation ``--eval-envs`` / ``--eval-sampled``, its shortest-path baseline with the paired
comparison ``--eval-baseline``, the vectorised dijkstra evaluation ``--dijkstra-envs`` (its router: ``--dijkstra-router``) and the per-road link counts of either
``--eval-link-counts`` / ``--eval-link-bin`` (also the bins of ``--eval-occupancy``, ``--eval-trips``,
``--eval-dynamic-gap`` and ``--eval-turns``), and the day-to-day replanning loop ``--replan-days`` / ``--replan-envs`` /
``--replan-fraction`` / ``--replan-max-hops``."""
import argparse
import os
import sys

# before anything imports torch (the HIP runtime reads it once): dmabuf IPC, which RCCL needs on hosts without legacy IPC —
# also when the ranks were started by an external `torchrun main.py` whose environment lacks it. A launcher's value wins.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from src.agents.base import DijkstraAgents  # noqa: E402
from src.runner import Runner, RunnerArgs  # noqa: E402

ALGOS = ("dijkstra", "random", "mpnn", "mpnn+ppo")


def replan_fraction(text):
    """--replan-fraction: ``msa`` or a share in (0, 1]."""
    try:
        v = text if text == "msa" else float(text)
    except ValueError:
        v = None
    if v is None or (v != "msa" and not 0.0 < v <= 1.0):
        raise argparse.ArgumentTypeError(f"must be 'msa' or a share in (0, 1], got {text!r}")
    return v


# (flag, argparse keyword arguments)
OPTIONS = (
    ("--algo", dict(choices=ALGOS, default="dijkstra", help="routing agent")),
    ("--scenario", dict(type=str, default="Easy",
                        help="data/<scenario>/ (MATSim XML), save/<scenario>/ cache, or synthetic-<edges>-<agents>[-seed]")),
    ("--mode", dict(choices=("eval", "train"), default="eval")),
    ("--timestep_size", dict(type=int, default=1, help="seconds per simulation step")),
    ("--start-end-time", dict(type=int, nargs=2, default=[0, 86400], metavar=("START", "END"))),
    ("--epochs", dict(type=int, default=1, help="PPO minibatch steps on the collected batch")),
    ("--rollout-steps", dict(type=int, default=32, help="frames collected per environment")),
    ("--seed", dict(type=int, default=0)),
    ("--device", dict(type=str, default="cpu", help="kept for compatibility: the path always runs on the GPU")),
    ("--output-dir", dict(type=str, default="runs")),
    ("--profile", dict(action="store_true")),
    ("--torch-compile", dict(action="store_true", help="accepted and ignored: the kernels are hand-written HIP")),
    ("--steps", dict(type=int, default=None, help="number of eval steps (overrides start/end time)")),
    ("--num-envs", dict(type=int, default=1, help="vectorised environments per GPU for mpnn+ppo training")),
    ("--policy-head", dict(choices=("embedding", "edge_mlp", "edge_mlp_fp32", "edge_mlp_bf16", "embedding_dijkstra",
                                    "graph_transformer", "goal_mlp"),
                           default="embedding",
                           help="mpnn / mpnn+ppo: the reference's live embedding head, or the per-edge MLP head it keeps "
                                "as parameters (state-dependent; edge_mlp: rollout logits at fp32 accuracy on the bf16 matrix "
                                "pipe — operands in exact bf16 pieces —, edge_mlp_fp32: on the fp32 matrix pipe, exact fp32 "
                                "products, edge_mlp_bf16: bf16 logits; the PPO update runs in fp32), or embedding_dijkstra: "
                                "the embedding plus the free-flow shortest-path prior towards the head agent's destination, "
                                "or graph_transformer: the reference's GraphTransformerNet edge output (evaluation-mode "
                                "BatchNorm, Laplacian positional encoding), or goal_mlp: a small trainable per-edge MLP on "
                                "destination-relative features (detour over the best turn, distance left, congestion; the "
                                "distances of --prior-method; not in the reference)")),
    ("--prior-weight", dict(type=float, default=1.0,
                            help="embedding_dijkstra: weight of the shortest-path prior (1.0 = the reference's plain sum)")),
    ("--prior-method", dict(choices=("all_pairs", "per_destination", "auto"), default="all_pairs",
                            help="embedding_dijkstra, goal_mlp: free-flow distances from the all-pairs table (N x N), or one column "
                                 "per distinct agent destination ([N][D], for large networks), or auto: all_pairs up to "
                                 "4 096 nodes, per_destination above")),
    ("--dijkstra-method", dict(choices=DijkstraAgents.METHODS, default="all_pairs",
                               help="dijkstra: next-hop table from all-pairs shortest paths (N x N), or one reverse "
                                    "shortest-path tree per distinct agent destination ([D][N], for large networks), or "
                                    "auto: all_pairs up to 4 096 nodes, per_destination above")),
    ("--value-head", dict(choices=("simple", "graph_transformer"), default="simple",
                          help="mpnn+ppo critic: the reference runner's MPNNValueNetSimple (per-road counts and the clock), "
                               "or graph_transformer: the reference's ValueNet, a second GraphTransformerNet on the policy's "
                               "observation, node output summed and read by mu_mlp (needs a state-dependent policy head)")),
    ("--equilibrium-metrics", dict(action="store_true",
                                   help="eval: also solve the user equilibrium and the system optimum of the static BPR "
                                        "model behind the MSA flows; print TSTT, both relative gaps and the Price of "
                                        "Anarchy with its interval, write equilibrium_metrics.json and "
                                        "equilibrium_flows.csv")),
    ("--equilibrium-gap", dict(type=float, default=1e-4, help="--equilibrium-metrics: relative-gap target")),
    ("--equilibrium-max-iter", dict(type=int, default=500,
                                    help="--equilibrium-metrics: iteration limit per problem (conjugate Frank-Wolfe)")),
    ("--eval-envs", dict(type=int, default=0,
                         help="mpnn / mpnn+ppo: also evaluate the policy on K vectorised environments (same network and "
                              "population, K noise streams) with its deterministic (MODE) action: mean, standard error and "
                              "a normal-approximation interval of return and travel times over the K realisations; train: "
                              "eval_vec/* in train_log.jsonl, eval: a printed block, eval_envs.json and eval_envs.csv")),
    ("--eval-sampled", dict(action="store_true", help="--eval-envs: also report a run with sampled actions")),
    ("--eval-baseline", dict(choices=("none", "dijkstra", "dijkstra_hold", "free_flow"), default="none",
                             help="--eval-envs: also run the shortest-path router on a second engine with the same "
                                  "seed, K and population (the same noise streams: common random numbers) and report the "
                                  "per-environment differences policy - baseline with their standard error; train: "
                                  "eval_vec_baseline/* and eval_vec_paired/* in train_log.jsonl, eval: two more printed "
                                  "blocks, `baseline` and `paired` in eval_envs.json, baseline_* columns in eval_envs.csv. "
                                  "dijkstra: the reference's rule, which in the environment's step order strands its agents "
                                  "on their destination roads; dijkstra_hold: a row whose next hop is its head's destination "
                                  "holds, so the agent is withdrawn one road short and the router delivers; free_flow: "
                                  "dijkstra_hold on tables built once from the empty network")),
    ("--policy-hold", dict(action="store_true",
                           help="mpnn / mpnn+ppo: apply the hold rule of dijkstra_hold to the POLICY's action (an action shield of "
                                "the environment, DESIGN 4.20; not in the reference, off by default): a road with a vehicle at its "
                                "head whose chosen next road is that vehicle's destination selects itself instead, so the "
                                "environment's step order (choice, core, withdraw) collects the vehicle one road short instead "
                                "of stranding it on its destination road. One difference from the routers' rule: an empty road "
                                "is never touched. It does not hold a road next to the destination that chose another road, "
                                "and does not save a vehicle inserted directly onto its destination road. The policy's draw, "
                                "log-prob and the PPO update are unchanged. eval: needs --eval-envs and acts on the policy's "
                                "vectorised evaluation only (one more line in its block, `policy_hold` and `held` in "
                                "eval_envs.json); train: acts on vectorised training and its eval_vec runs (train/held and "
                                "eval_vec/held in train_log.jsonl), refused with --policy-head embedding, whose rollout "
                                "kernels draw every frame's action ahead of the frames. An agent inserted directly onto "
                                "its destination road: see --route-departures")),
    ("--route-departures", dict(action="store_true",
                                help="first-hop routing (an environment-side rule, DESIGN 4.23; not in the reference, off by "
                                     "default): an EMPTY road with an agent ready to depart from it selects for that agent (the "
                                     "smallest ready id of the origin) instead of for the dummy head agent 0, so the first hop "
                                     "of a trip heads for the traveller's own destination; a non-empty origin road keeps its "
                                     "head's choice. The routers look the hop up in their own tables, the replanning days in "
                                     "the plan, a policy head in a free-flow table built once; a policy's draw, log-prob and "
                                     "the PPO update are unchanged. eval: needs --eval-envs, --dijkstra-envs (routers hold / "
                                     "free_flow) or --replan-days and acts on the policy's vectorised run, on the baselines "
                                     "dijkstra_hold / free_flow and on the replanning days (one more line in each block, "
                                     "`route_departures` and `departures_routed` in the JSON files); refused with "
                                     "--eval-baseline dijkstra and --dijkstra-router reference (use dijkstra_hold / hold). "
                                     "train: acts on vectorised training and its eval_vec runs (train/departures_routed and "
                                     "eval_vec/departures_routed in train_log.jsonl), refused with --policy-head embedding. "
                                     "--pretrain-bc runs its own engine without the rule")),
    ("--reward", dict(choices=("queue", "trip"), default="queue",
                      help="queue (default): the reference's reward, minus the vehicles standing in FIFOs after the frame. trip "
                           "(an environment-side rule, DESIGN 4.24; not in the reference): minus the travellers who should be "
                           "under way and have not arrived, the agents on the way plus the waiting agents that are due, so that "
                           "an agent lost on the way or kept out by a full origin road keeps costing until the horizon. train: "
                           "what PPO optimises (train/reward_kind in train_log.jsonl; the eval_vec runs log "
                           "eval_vec/trip_return*), refused with --policy-head embedding. eval: needs --eval-envs, "
                           "--dijkstra-envs or --replan-days; computed BESIDE the queue reward for the policy run, the "
                           "baseline and the days (one more line per block, `trip_return` in the JSON files and the "
                           "eval_envs.csv columns, a `trip_return` difference in the paired block); every other number stays "
                           "as it is")),
    ("--credit", dict(choices=("joint", "decision"), default="joint",
                      help="train, mpnn / mpnn+ppo: how PPO assigns credit. joint (default): the reference's update, one "
                           "probability ratio over all roads' draws and one advantage per frame and environment. decision "
                           "(DESIGN 4.26; not in the reference): every road that had a traveller at the head of its queue is "
                           "credited on its own, with that traveller's frames until it was withdrawn (until the horizon if it "
                           "never was) against its free-flow frames to go, and the ratio and the clip act on that road's "
                           "choice alone; critic and entropy terms are unchanged. train_log.jsonl gains train/credit, "
                           "train/decisions, train/decision_delay_frames, train/decision_truncated, "
                           "train/decision_clip_fraction and train/decision_kl. Refused in eval mode, with --policy-head "
                           "embedding and with --value-head graph_transformer; combines with --reward, --policy-hold, "
                           "--route-departures and --pretrain-bc")),
    ("--credit-gamma", dict(type=float, default=None, metavar="G",
                            help="--credit decision: the discount of a traveller's frames to go, in (0, 1] (default 1.0); "
                                 "separate from GAE's gamma")),
    ("--credit-baseline", dict(choices=("free_flow", "learned"), default=None,
                               help="--credit decision: the baseline of the per-decision advantage (default free_flow, the "
                                    "traveller's free-flow frames to go). learned (DESIGN 4.27; not in the reference) adds a "
                                    "small critic on the state in front of the decision (the road, the destination, the load "
                                    "around it, the frames left in the segment), trained beside the policy on the delay beyond "
                                    "free flow; it never reads the action. It is not saved in policy.pt. train_log.jsonl gains "
                                    "train/credit_baseline, train/decision_critic_loss, train/decision_explained_variance and "
                                    "train/decision_value_mean")),
    ("--credit-critic-coef", dict(type=float, default=None, metavar="C",
                                  help="--credit decision --credit-baseline learned: the coefficient of the per-decision "
                                       "critic's loss, >= 0 (default 1.0); refused without --credit-baseline learned")),
    ("--credit-scope", dict(choices=("headed", "due"), default=None,
                            help="--credit decision: which roads are credited (default headed: every road with a traveller "
                                 "at the head of its queue). due (DESIGN 4.28; not in the reference) credits only the roads "
                                 "whose head is due at the frame's clock: the draw of a road whose head is still travelling "
                                 "reaches nobody. train_log.jsonl gains train/credit_scope and train/decisions_headed")),
    ("--credit-horizon", dict(choices=("charge", "bootstrap"), default=None,
                              help="--credit decision: what a traveller still under way owes when a segment ends (default "
                                   "charge: the frames to the horizon). bootstrap (DESIGN 4.28; not in the reference) adds "
                                   "the free-flow time from the road it is queued on where the batch cut the segment (an "
                                   "optimistic estimate); an episode that ended keeps the charge. train_log.jsonl gains "
                                   "train/credit_horizon and train/decision_bootstrapped")),
    ("--dijkstra-envs", dict(type=int, default=0,
                             help="--algo dijkstra --mode eval: after the single-environment report, evaluate the router on K "
                                  "vectorised environments (each routing on its own congested travel times, in the "
                                  "environment's step order); prints the aggregate block, writes dijkstra_envs.json and "
                                  "dijkstra_envs.csv")),
    ("--dijkstra-router", dict(choices=("reference", "hold", "free_flow"), default="reference",
                               help="--dijkstra-envs: the router of the K environments; reference: DijkstraAgents.choice's rule, "
                                    "hold: the one that holds one road short of the destination and delivers (head "
                                    "dijkstra_hold), free_flow: hold on tables built once from the empty network")),
    ("--replan-days", dict(type=int, default=0, metavar="J",
                           help="eval, any --algo: J > 0 adds the day-to-day replanning loop (DESIGN 4.19, not in the reference): "
                                "J simulated days on --replan-envs environments of a fused engine of its own; day 0 follows the "
                                "quickest routes of the empty network, after every day a share of the agents re-routes onto the "
                                "quickest route under the road times experienced so far; a `Replanning` block with the day table "
                                "(arrivals, travel time, dynamic relative gap, share that switched), replan_days.csv, "
                                "replan_envs.json / replan_envs.csv, and replan_*.csv for the --eval-* report flags that are set")),
    ("--replan-envs", dict(type=int, default=1, metavar="K",
                           help="--replan-days: the environments of the loop; equal to --eval-envs it adds the paired block "
                                "policy - replanned on the last day (same seed: common random numbers)")),
    ("--replan-fraction", dict(type=replan_fraction, default=0.1, metavar="F|msa",
                               help="--replan-days: the share of the agents that may switch per day, in (0, 1], or msa: "
                                    "1 / (day + 2)")),
    ("--replan-max-hops", dict(type=int, default=None, metavar="L",
                               help="--replan-days: the longest route stored, in roads (default: min(roads, 256)); an agent "
                                    "whose quickest route is longer has no route")),
    ("--eval-link-counts", dict(action="store_true",
                                help="--eval-envs / --dijkstra-envs, eval: count per road the frames in which its head was "
                                     "popped plus those in which an agent was withdrawn from it, over the K environments; a "
                                     "`Link counts` block, eval_link_counts.csv (dijkstra_link_counts.csv) with mean, standard "
                                     "error and interval per road against the MSA (and, with --equilibrium-metrics, UE / SO) "
                                     "flows and, with --eval-baseline, the paired difference; `link_counts` in the JSON file")),
    ("--eval-link-bin", dict(type=int, default=3600, metavar="SECONDS", help="--eval-link-counts: width of the time bins")),
    ("--eval-occupancy", dict(action="store_true",
                              help="--eval-envs / --dijkstra-envs, eval: sum per road and time bin (of --eval-link-bin seconds) "
                                   "the vehicles on it after every frame, count the frames in which it was at capacity and "
                                   "keep its peak, over the K environments; an `Occupancy` block, eval_occupancy.csv "
                                   "(dijkstra_occupancy.csv) with vehicle-seconds, occupancy per bin, v/c, peak and frames "
                                   "at capacity per road and, with --eval-baseline, the paired differences; `occupancy` in "
                                   "the JSON file")),
    ("--eval-trips", dict(action="store_true",
                          help="--eval-envs / --dijkstra-envs, eval: reduce the K agent tables per traveller: arrival share, "
                               "travel time (mean, sd, se, interval, min, max) over the environments, delay against the "
                               "free-flow time and, with --eval-baseline, the paired difference per trip; a `Trips` block "
                               "with a table by departure time (bins of --eval-link-bin seconds), eval_trips.csv and "
                               "eval_trips_by_departure.csv (dijkstra_trips*.csv); `trips` in the JSON file")),
    ("--eval-dynamic-gap", dict(action="store_true",
                                help="--eval-envs / --dijkstra-envs, eval: measure every completed trip against the quickest "
                                     "path in hindsight under the time-dependent road times the run itself produced (mean "
                                     "occupancy per bin of --eval-link-bin seconds): a `Dynamic gap` block with the relative gap "
                                     "over the environments, eval_dynamic_gap.csv and eval_dynamic_gap_by_departure.csv "
                                     "(dijkstra_dynamic_gap*.csv) and, with --eval-baseline, the paired difference; "
                                     "`dynamic_gap` in the JSON file")),
    ("--eval-dynamic-gap-envs", dict(type=int, default=None, metavar="J",
                                     help="--eval-dynamic-gap: search the first J of the K environments only (default: all)")),
    ("--eval-turns", dict(action="store_true",
                          help="--eval-envs / --dijkstra-envs, eval: count per route edge u -> v and time bin (of --eval-link-bin "
                               "seconds) the vehicles that crossed it, and per road the agents lost to the reference's U-turn "
                               "double pop, over the K environments; a `Turns` block, eval_turns.csv (dijkstra_turns.csv) with "
                               "mean, standard error and interval per turn, its share of the movements out of its road, for "
                               "the embedding head the policy's probability and, with --eval-baseline, the paired "
                               "difference; eval_turns_lost.csv; `turns` in the JSON file")),
    ("--eval-paths", dict(action="store_true",
                          help="--eval-envs / --dijkstra-envs, eval: trace per (environment, traveller) the roads it was seen on "
                               "as the head of a queue (DESIGN 4.25, not in the reference): how many, the free-flow cost of the "
                               "hops, how much of it was detour against the free-flow shortest path to its own destination, and "
                               "how often it came back to a road; a `Paths` block that splits the travel time of a completed trip "
                               "into shortest free-flow cost + wandering + everything else (with --eval-trips), names the agents "
                               "that loop and gives a table by departure time (bins of --eval-link-bin seconds); eval_paths.csv "
                               "(dijkstra_paths.csv) with one row per agent and, with --eval-baseline, the paired differences; "
                               "`paths` in the JSON file; also through --replan-days (replan_paths.csv)")),
    ("--eval-paths-max-hops", dict(type=int, default=None, metavar="L",
                                   help="--eval-paths: roads kept per trace (default 64, at most 4096; 0 keeps no routes: counts "
                                        "and costs only, and no loop is recognised)")),
    ("--eval-paths-routes", dict(type=int, default=0, metavar="J",
                                 help="--eval-paths: also write the kept routes of the first J environments to "
                                      "eval_paths_routes.csv (env, agent, roads, truncated, route as space-separated road ids)")),
    ("--iterations", dict(type=int, default=1,
                          help="train: collector batches (total frames per environment = iterations x rollout steps)")),
    ("--pretrain-bc", dict(type=int, default=0, metavar="I",
                           help="train, mpnn / mpnn+ppo: I > 0 behaviour-cloning iterations before the first PPO iteration "
                                "(DESIGN 4.21, not in the reference): the shortest-path router labels every occupied road of a "
                                "rollout on --bc-envs environments with its pick among the road's out-edges, and the policy head "
                                "is trained on the cross-entropy of those labels; one printed line and one line of bc_log.jsonl "
                                "per iteration, then the usual policy.pt; with mpnn+ppo training continues from the cloned "
                                "weights, with mpnn no PPO iteration follows. Evaluate with --policy-hold")),
    ("--bc-expert", dict(choices=("dijkstra", "free_flow"), default=None,
                         help="--pretrain-bc: the router imitated; dijkstra (default): every environment's own congested "
                              "times, tables rebuilt every 10 frames; free_flow: tables built once at frame 0")),
    ("--bc-driver", dict(choices=("expert", "policy", "dagger"), default=None,
                         help="--pretrain-bc: who drives the labelled rollout; expert: the holding router itself; policy: the "
                              "head's sampled action under the hold rule; dagger (default): iteration 0 as expert, every later "
                              "one as policy")),
    ("--bc-envs", dict(type=int, default=None, metavar="K", help="--pretrain-bc: environments of its engine (default 16)")),
    ("--bc-frames", dict(type=int, default=None, metavar="T",
                         help="--pretrain-bc: frames per iteration (default: --rollout-steps)")),
    ("--bc-samples", dict(type=int, default=None, metavar="S",
                          help="--pretrain-bc: (environment, frame) pairs kept per iteration (default 256)")),
    ("--bc-epochs", dict(type=int, default=None, help="--pretrain-bc: passes over the kept pairs (default 4)")),
    ("--bc-batch", dict(type=int, default=None, help="--pretrain-bc: minibatch (default: the PPO sub-batch)")),
    ("--bc-lr", dict(type=float, default=None, help="--pretrain-bc: Adam step size (default: the PPO trainer's)")),
    ("--checkpoint", dict(type=str, default=None,
                          help="mpnn / mpnn+ppo: load a policy.pt written by --mode train into the policy network; a file "
                               "whose keys or shapes do not match the network is refused")),
)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="TARL routing experiments on MI355X (classical agents, MPNN policy, PPO)")
    for flag, kw in OPTIONS:
        parser.add_argument(flag, **kw)
    return parser


def main(argv=None):
    """Under ``torchrun --nproc-per-node N main.py --algo mpnn+ppo --mode train ...`` every rank joins the process group
    (RCCL), binds its own GPU, trains on its own rollouts (engine seed + rank) with averaged gradients, and only rank 0
    writes logs / checkpoints / metric tables."""
    ns = build_parser().parse_args(argv)
    runner = Runner(RunnerArgs(**vars(ns)))       # joins the process group when launched by torchrun
    try:
        runner.setup()
        if ns.mode == "train":
            runner.train()
        runner.eval()
    except BaseException:
        # a rank that fails must not enter a collective its peers are not in (they may sit in a gradient all-reduce or in
        # ppo_train's trailing barrier): leave the group WITHOUT a barrier and exit non-zero so the launcher tears the
        # job down instead of waiting for the communicator's timeout
        runner.close(failed=True)
        raise
    else:
        runner.close()


if __name__ == "__main__":
    main()
