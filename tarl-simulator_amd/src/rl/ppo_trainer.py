"""ppo_train — same signature as the reference's (src/rl/ppo_trainer.py:12-14); the loop itself is
``tarl_hip.trainer.VecPPOTrainer`` (collector + GAE + clipped PPO loss + Adam, all HIP kernels). The replay-buffer round
trip through the CPU (:133) and per-frame TensorDict bookkeeping are not reproduced. The reference's scalar tags
(:60-88: ``PPO/avg_episode_return``, ``loss/*``, ``approx_kl``, ``clip_fraction``, ``grad_global_norm``,
``transport/*``) go to ``<log_dir>/train_log.jsonl`` — and to a TensorBoard ``SummaryWriter`` as well when
``torch.utils.tensorboard`` is importable. The periodic evaluation pass (:89-127,147-151) runs on ``eval_env`` through the drop-in classes (MODE = GraphDistribution.mode,
optionally a sampled rollout); its scalars ``eval/avg_return``, ``eval/episode_len``, ``eval/computation_time_ms`` and the
arrays behind the reference's histograms (``eval/nodes_metrics/avg_vc|std_vc``) and leg-histogram figure go into the same
record; matplotlib figures are not drawn.

Extension: ``eval_envs`` K > 0 adds a vectorised evaluation (``tarl_hip.evaluator.VecEvaluator``: the same policy on K
environments of its own fused engine, MODE, with ``stochastic_eval`` also sampled) to every periodic evaluation; its
scalars ``eval_vec/*`` (``eval_vec_stochastic/*``) carry the spread over the K realisations of the stochastic simulator
that the single drop-in rollout cannot give. The ``eval/*`` record is unchanged.

Extension: ``eval_baseline="dijkstra"`` (or ``"dijkstra_hold"`` / ``"free_flow"``, the routers that deliver in the environment's
step order; with ``eval_envs``) evaluates the shortest-path router once, at the first periodic
evaluation, on a second engine with the same seed, K and population (rank 0 alone, no collective): it is a function of the
seed only, so its per-environment values are cached, and every record that carries ``eval_vec/*`` also carries
``eval_vec_baseline/*`` and the paired differences policy - baseline ``eval_vec_paired/*`` (common random numbers).

Extension: ``num_envs`` (default 1) vectorises the rollout over B environments per GPU; under ``torchrun`` every rank
trains on its own environments and gradients are averaged with one RCCL all-reduce per optimiser step.
"""
from __future__ import annotations

import json
import os
import time

import torch

from ..agents.base import destination_set
from .modules import unwrap

EVAL_BASELINE_NAMES = ("none", "dijkstra", "dijkstra_hold", "free_flow")      # tarl_hip.evaluator.EVAL_BASELINES, and "none"


def _episode_returns(reward_tb, done_t):
    """The reference's logged return (src/rl/ppo_trainer.py:45-58): mean return of the episodes that END inside the batch,
    or — when none does — the sum of the rewards collected so far. ``reward_tb`` (T, B) on the host, ``done_t`` (T,) bool;
    averaged over the B environments."""
    returns, cum = [], torch.zeros(reward_tb.size(1))
    for t in range(reward_tb.size(0)):
        cum = cum + reward_tb[t]
        if bool(done_t[t]):
            returns.append(cum.mean().item())
            cum = torch.zeros_like(cum)
    return sum(returns) / len(returns) if returns else cum.mean().item()


def _evaluate(prefix, deterministic, eval_env, policy_module, frames_per_batch):
    """The reference's ``_evaluate`` (src/rl/ppo_trainer.py:89-127): one rollout of the policy on ``eval_env`` — its MODE
    (``deterministic``: GraphDistribution.mode, torchrl's ExplorationType.MODE) or a sampled action per frame — until the
    episode ends or ``frames_per_batch`` frames; scalars + the arrays behind the reference's histograms / figures."""
    start = time.perf_counter()
    actor = policy_module
    was = getattr(actor, "deterministic", False)
    actor.deterministic = bool(deterministic)
    try:
        with torch.no_grad():
            frames = eval_env.rollout(frames_per_batch, policy_module, break_when_any_done=True)
    finally:
        actor.deterministic = was
    comp_ms = (time.perf_counter() - start) * 1000.0
    rewards = torch.stack([f["next"]["reward"].reshape(-1) for f in frames]).view(-1)
    rec = {f"{prefix}/avg_return": float(rewards.sum()), f"{prefix}/episode_len": int(rewards.numel()),
           f"{prefix}/computation_time_ms": comp_ms}
    sim = getattr(eval_env, "simulator", None)
    if sim is not None:
        try:      # the data of writer.add_histogram(nodes_metrics/*) and of the leg-histogram figure, as arrays
            nm = sim.compute_node_metrics(output_dir=None)
            if nm:
                rec[f"{prefix}/nodes_metrics/avg_vc"] = [float(m["avg_vc"]) for m in nm.values()]
                rec[f"{prefix}/nodes_metrics/std_vc"] = [float(m["std_vc"]) for m in nm.values()]
            leg = sim.leg_histogram()           # (T, 4): departures, arrivals, on the way, time
            if leg.numel():
                rec[f"{prefix}/leg_histogram"] = leg.tolist()
        except Exception:  # noqa: BLE001 - the reference swallows metric errors here too (:125-126)
            pass
    return rec, frames


def _eval_engine(eval_env, eval_envs, seed, agent_features=None):
    """A fused engine of its own on copies of ``eval_env``'s graph state and agent table (``agent_features``: another copy
    of that table to start from; the drop-in environment is left alone), noise seed ``seed + 104729``: two of them see the
    same noise streams."""
    from tarl_hip import ops
    from tarl_hip.engine import SimEngine
    sim = eval_env.simulator
    g = sim.graph
    if not ops.fused_path_supported(g.edge_index, sim.Nmax):
        raise ValueError("eval_envs needs the packed (fused) path, which cannot represent this graph (Nmax > 127, an "
                         "out-degree above 126 or parallel edges): there is no fall-back for the vectorised evaluation")
    agents = sim.agent.agent_features if agent_features is None else agent_features
    return SimEngine(g.x.clone(), g.edge_index, g.edge_attr, sim.Nmax, agents.clone(),
                     congestion_constant=getattr(g, "congestion_constant", None), num_envs=int(eval_envs),
                     device=g.x.device, timestep=sim.timestep, seed=seed + 104729, fused=True)


def _vec_evaluator(eval_env, policy_net, eval_envs, seed, temperature, policy_hold=False, route_departures=False,
                   trip_reward=False):
    """The K-environment evaluator of ``ppo_train(eval_envs=K)``; ``policy_hold``: with the hold rule on the policy's action
    (DESIGN 4.20); ``route_departures``: with the first-hop rule on empty origin roads; ``trip_reward``: with the
    trip reward beside the queue reward."""
    from tarl_hip.evaluator import VecEvaluator
    engine = _eval_engine(eval_env, eval_envs, seed)
    dests = None
    if getattr(policy_net, "policy_head", "embedding") in ("embedding_dijkstra", "goal_mlp") and \
            policy_net.resolve_prior_method() != "all_pairs":
        dests = destination_set(engine.agents, engine.N)
    kw = {"policy_hold": True} if policy_hold else {}
    if route_departures:
        kw["route_departures"] = True
    if trip_reward:
        kw["trip_reward"] = True
    return VecEvaluator.from_policy_net(engine, policy_net, prior_dests=dests, temperature=temperature, **kw)


def _pretrain_bc(env, trainer, cfg, seed, log_dir):
    """The behaviour-cloning iterations in front of PPO: one printed line and one line of ``bc_log.jsonl`` each."""
    from tarl_hip.imitation import BCTrainer
    engine = _eval_engine(env, cfg["envs"], seed + 1)
    bc = BCTrainer(trainer, engine, expert=cfg["expert"], driver=cfg["driver"], frames=cfg["frames"], samples=cfg["samples"],
                   epochs=cfg["epochs"], batch=cfg["batch"] or trainer.M, lr=cfg["lr"] or trainer.lr, seed=seed)
    log = open(os.path.join(log_dir, "bc_log.jsonl"), "a") if log_dir is not None else None
    for _ in range(int(cfg["iterations"])):
        rec = bc.iterate()
        print(f"[bc {rec['iteration']}] driver {rec['driver']} ({rec['expert']}), {rec['frames']} frames x {rec['envs']} envs: "
              f"{rec['labelled']} labelled rows ({100 * rec['labelled_share']:.1f} %), loss {rec['loss_first']:.4f} -> "
              f"{rec['loss_last']:.4f}, accuracy {rec['accuracy_before']:.3f} -> {rec['accuracy_after']:.3f}, arrivals "
              f"{rec['arrivals']:.1f}, {rec['collect_seconds']:.2f} s + {rec['update_seconds']:.2f} s")
        if log is not None:
            log.write(json.dumps(rec) + "\n")
            log.flush()
    if log is not None:
        log.close()


def vec_eval_record(prefix, res):
    """The scalars of one vectorised evaluation (tarl_hip.evaluator.EvalResult) for the training log. After a domain exit
    only ``envs``, ``domain_exit`` and the time are numbers; the statistics are ``None`` (never an average of such a run)."""
    rec = {f"{prefix}/envs": res.envs, f"{prefix}/domain_exit": bool(res.domain_exit),
           f"{prefix}/computation_time_ms": res.computation_time_ms}
    agg = res.aggregate or {}
    for key, src, stat in (("avg_return", "episode_return", "mean"), ("avg_return_se", "episode_return", "se"),
                           ("avg_travel_time", "avg_travel_time", "mean"), ("avg_travel_time_se", "avg_travel_time", "se"),
                           ("arrived", "arrived", "mean"), ("p95_travel_time", "p95_travel_time", "mean")):
        rec[f"{prefix}/{key}"] = agg[src][stat] if src in agg else None
    return rec


def ppo_train(env, policy_module, value_module, *, total_frames=128, frames_per_batch=32, num_epochs=1,
              sub_batch_size=32, device=torch.device("cpu"), checkpoint_path=None, log_dir=None, eval_env=None,
              eval_interval=0, log_interval=1, stochastic_eval=False, num_envs=1, seed=0, eval_envs=0,
              eval_baseline="none", policy_hold=False, pretrain_bc=None, route_departures=False, reward="queue",
              credit="joint", decision_gamma=1.0, credit_baseline="free_flow", decision_critic_coef=1.0,
              credit_scope="headed", credit_horizon="charge"):
    """``pretrain_bc`` (not in the reference; None = off): a dict {iterations, expert, driver, envs, frames,
    samples, epochs, batch, lr} — that many behaviour-cloning iterations (tarl_hip.imitation.BCTrainer) run before the first
    PPO iteration, on an engine of their own; one line each is printed and appended to ``bc_log.jsonl``.
    ``reward``: ``"trip"`` trains on the trip reward (VecPPOTrainer(reward="trip")); the log records gain
    ``train/reward_kind`` and the ``eval_vec*`` evaluations run with ``trip_reward=True`` and log ``eval_vec/trip_return*``.
    ``credit``: ``"decision"`` trains with per-decision credit (VecPPOTrainer(credit="decision",
    decision_gamma=...)); the log records gain ``train/credit``, ``train/decisions``, ``train/decision_delay_frames``,
    ``train/decision_truncated``, ``train/decision_clip_fraction`` and ``train/decision_kl``.
    ``credit_baseline``: ``"learned"`` adds the per-decision critic (VecPPOTrainer(credit_baseline="learned",
    decision_critic_coef=...)); its 161 parameters are created here (ops.decision_critic_init), join the optimiser's buffer
    and are not saved with the policy, as no critic is. The log records gain ``train/credit_baseline``,
    ``train/decision_critic_loss``, ``train/decision_explained_variance`` and ``train/decision_value_mean``.
    ``credit_scope`` / ``credit_horizon``: ``"due"`` credits only the roads whose head is due, ``"bootstrap"``
    continues a traveller cut off by the batch in free flow (VecPPOTrainer(credit_scope=..., credit_horizon=...)). The log
    records gain ``train/credit_scope`` and ``train/decisions_headed``, ``train/credit_horizon`` and
    ``train/decision_bootstrapped``, each pair only with its non-default value."""
    if reward not in ("queue", "trip"):
        raise ValueError("reward must be 'queue' or 'trip'")
    if credit not in ("joint", "decision"):
        raise ValueError("credit must be 'joint' or 'decision'")
    if credit_baseline not in ("free_flow", "learned"):
        raise ValueError("credit_baseline must be 'free_flow' or 'learned'")
    if credit_baseline == "learned" and credit != "decision":
        raise ValueError("credit_baseline learned is the baseline of the per-decision advantage: it needs credit decision")
    learned = credit_baseline == "learned"
    if credit_scope not in ("headed", "due"):
        raise ValueError("credit_scope must be 'headed' or 'due'")
    if credit_horizon not in ("charge", "bootstrap"):
        raise ValueError("credit_horizon must be 'charge' or 'bootstrap'")
    if credit_scope != "headed" and credit != "decision":
        raise ValueError("credit_scope narrows the per-decision credit: it needs credit decision")
    if credit_horizon != "charge" and credit != "decision":
        raise ValueError("credit_horizon closes the per-decision return: it needs credit decision")
    trip = reward == "trip"
    from tarl_hip import dist_utils, ops
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer

    rank, world = dist_utils.world()
    policy_net = unwrap(policy_module, "MPNNPolicyNet")
    try:
        value_net, value_head = unwrap(value_module, "MPNNValueNetSimple"), "simple"
    except TypeError:
        value_net, value_head = unwrap(value_module, "ValueNet"), "graph_transformer"
    sim = env.simulator
    g = sim.graph
    agents = sim.agent.agent_features
    # every rank (one process per GPU) rolls out its own environments: the device noise streams are keyed by the engine
    # seed, so seed + rank gives different trajectories per rank; parameters stay replicated (rank 0's are broadcast)
    engine = SimEngine(g.x, g.edge_index, g.edge_attr, sim.Nmax, agents,
                       congestion_constant=getattr(g, "congestion_constant", None), num_envs=num_envs,
                       device=g.x.device, timestep=sim.timestep, seed=seed + 7919 * rank,
                       fused=ops.fused_path_supported(g.edge_index, sim.Nmax))   # same decision on every rank
    dormant = [p for n, p in policy_net.named_parameters() if not n.startswith("nodes_embedding")]
    if value_head == "simple":
        l = value_net.final_mlp
        critic = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
        critic_kw = {}
    else:       # every parameter of the critic's network goes to the optimiser, as loss_module.parameters() does
        critic = list(value_net.transformer.parameters())
        critic_kw = dict(value="graph_transformer", gt_value_params=value_net.kernel_tensors(), gt_value_pe=value_net.gt_pe)
    head = getattr(policy_net, "policy_head", "embedding")
    m = policy_net.edge_mlp
    prior_kw = {}
    if head in ("embedding_dijkstra", "goal_mlp"):      # the heads that read the shortest-path tables
        if policy_net.resolve_prior_method() == "all_pairs":
            prior_kw = dict(prior_table=policy_net.dist_matrix)
        else:       # one column per destination of every environment's agent table
            prior_kw = dict(prior_free_flow=policy_net.free_flow_weights(),
                            prior_dests=destination_set(engine.agents, engine.N))
    if head == "goal_mlp":
        gm = policy_net.goal_mlp
        prior_kw["goal_mlp_params"] = [gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias]
    dcritic = ops.decision_critic_init(engine.device, seed) if learned else []
    trainer = VecPPOTrainer(engine, policy_net.nodes_embedding.weight,
                            critic,
                            rollout_steps=frames_per_batch, num_epochs=num_epochs, sub_batch_size=sub_batch_size,
                            extra_params=dormant + dcritic, seed=seed,
                            policy=head if head in ("embedding", "embedding_dijkstra", "graph_transformer",
                                                    "goal_mlp") else "edge_mlp",
                            edge_mlp_params=[m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias],
                            policy_precision={"edge_mlp_bf16": "bf16", "edge_mlp_fp32": "fp32"}.get(head, "x3"),
                            prior_weight=getattr(policy_net, "prior_weight", 1.0), **prior_kw,
                            gt_params=policy_net.transformer.kernel_tensors() if head == "graph_transformer" else None,
                            gt_pe=getattr(policy_net, "gt_pe", None), **critic_kw,
                            **({"policy_hold": True} if policy_hold else {}),
                            **({"route_departures": True} if route_departures else {}),
                            **({"reward": "trip"} if trip else {}),
                            **({"credit": "decision", "decision_gamma": decision_gamma} if credit == "decision" else {}),
                            **({"credit_baseline": "learned", "decision_critic_params": dcritic,
                                "decision_critic_coef": decision_critic_coef} if learned else {}),
                            **({"credit_scope": "due"} if credit_scope == "due" else {}),
                            **({"credit_horizon": "bootstrap"} if credit_horizon == "bootstrap" else {}))
    log = writer = None
    if log_dir is not None and rank == 0:      # rank 0 alone writes
        os.makedirs(log_dir, exist_ok=True)
        log = open(os.path.join(log_dir, "train_log.jsonl"), "a")
        try:   # optional: the same scalars as TensorBoard events (tensorboard is not part of this image)
            from torch.utils.tensorboard import SummaryWriter
            writer = SummaryWriter(log_dir=log_dir)
        except Exception:  # noqa: BLE001
            writer = None
    trainer.keep_grad = log is not None
    if pretrain_bc:
        _pretrain_bc(env, trainer, dict(pretrain_bc), seed, log_dir if rank == 0 else None)
    if int(eval_envs) < 0:
        raise ValueError("eval_envs must be >= 0")
    # rank 0 alone evaluates (as it alone logs); the evaluator enters no collective
    vec_eval = (_vec_evaluator(eval_env, policy_net, eval_envs, seed, trainer.temperature, policy_hold, route_departures, trip)
                if eval_envs and eval_env is not None and log is not None else None)
    ppo_train.last_vec_eval = vec_eval
    if eval_baseline not in EVAL_BASELINE_NAMES:
        raise ValueError(f"eval_baseline must be one of {EVAL_BASELINE_NAMES}, got {eval_baseline!r}")
    if eval_baseline != "none" and not eval_envs:
        raise ValueError("eval_baseline needs eval_envs > 0")
    baseline_res = None                       # the router's EvalResult: evaluated once, a function of the seed only
    # the population as the policy's evaluator saw it (training marks its agents on the way / arrived in this table)
    baseline_agents = eval_env.simulator.agent.agent_features.clone() if vec_eval is not None and eval_baseline != "none" else None
    frames = 0
    it = 0
    h = sim.h
    ppo_train.last_eval = {}
    ppo_train.last_trainer = trainer          # introspection hooks for tests / notebooks
    while frames < total_frames:
        t0 = time.perf_counter()
        frames += trainer.collect() // engine.B
        out = trainer.update()
        rec = None
        if log is not None and it % max(1, log_interval) == 0:
            o = out.tolist()
            x0, ag0 = engine.x[0], engine.agents[0]                       # environment 0, like the reference's single env
            done = ag0[:, 8] == 1
            vc = x0[:, h.NUMBER_OF_AGENT] / x0[:, h.MAX_NUMBER_OF_AGENT].clamp(min=1)
            rec = {"global_step": frames,
                   "PPO/avg_episode_return": _episode_returns(trainer.reward.cpu(), trainer.done_frames),
                   "loss/objective": o[0], "loss/value": o[1], "loss/entropy": o[2], "loss/total": o[0] + o[1] + o[2],
                   "approx_kl": o[4], "clip_fraction": o[3], "ESS": o[5],
                   "grad_global_norm": float(trainer.last_grad.norm()) if trainer.last_grad is not None else float("nan"),
                   "transport/avg_vc_ratio": float(vc.mean()), "transport/std_vc_ratio": float(vc.std(unbiased=False)),
                   "iter_seconds": time.perf_counter() - t0}
            if policy_hold:               # rows the hold rule rewrote in this iteration's frames, per environment
                rec["train/held"] = float(trainer.held.sum()) / engine.B
            if route_departures:          # empty origin rows the first-hop rule wrote in this iteration's frames, per environment
                rec["train/departures_routed"] = float(trainer.departures_routed.sum()) / engine.B
            if trip:                      # PPO/avg_episode_return above is the return of the trip reward
                rec["train/reward_kind"] = "trip"
            if credit == "decision":      # the per-decision term of the last minibatch; loss/objective above is the joint one's 0
                dl = {k: float(v) for k, v in trainer.last["decision"].items() if not isinstance(v, str)}
                rec.update({"train/credit": "decision", "train/decisions": int(dl["decisions"]),
                            "train/decision_delay_frames": dl["delay_frames"], "train/decision_truncated": dl["truncated"],
                            "train/decision_clip_fraction": dl["clip_fraction"], "train/decision_kl": dl["kl"]})
                if learned:
                    rec.update({"train/credit_baseline": "learned", "train/decision_critic_loss": dl["critic_loss"],
                                "train/decision_explained_variance": dl["explained_variance"],
                                "train/decision_value_mean": dl["value_mean"]})
                if credit_scope == "due":
                    rec.update({"train/credit_scope": "due", "train/decisions_headed": int(dl["decisions_headed"])})
                if credit_horizon == "bootstrap":
                    rec.update({"train/credit_horizon": "bootstrap", "train/decision_bootstrapped": dl["bootstrapped"]})
            if bool(done.any()):
                rec["transport/avg_travel_time"] = float((ag0[done, 3] - ag0[done, 2]).mean())
        # periodic evaluation (src/rl/ppo_trainer.py:147-151): MODE rollout, optionally a sampled one, on eval_env
        if log is not None and eval_env is not None and eval_interval and it % eval_interval == 0:
            rec = rec if rec is not None else {"global_step": frames}
            ev, fr = _evaluate("eval", True, eval_env, policy_module, frames_per_batch)
            rec.update(ev)
            ppo_train.last_eval["eval"] = fr
            if stochastic_eval:
                ev, fr = _evaluate("eval_stochastic", False, eval_env, policy_module, frames_per_batch)
                rec.update(ev)
                ppo_train.last_eval["eval_stochastic"] = fr
            if vec_eval is not None:      # like _evaluate: frames_per_batch frames or the episode's end, whichever is first
                n_eval = min(int(frames_per_batch), vec_eval.episode_frames)
                for prefix, det in (("eval_vec", True),) + ((("eval_vec_stochastic", False),) if stochastic_eval else ()):
                    res = vec_eval.run(n_eval, deterministic=det)
                    rec.update(vec_eval_record(prefix, res))
                    if policy_hold and res.held is not None:
                        rec[f"{prefix}/held"] = float(res.held.mean())
                    if route_departures and res.departures_routed is not None:
                        rec[f"{prefix}/departures_routed"] = float(res.departures_routed.mean())
                    if trip and res.trip_return is not None:
                        g = res.aggregate["trip_return"]
                        rec[f"{prefix}/trip_return"], rec[f"{prefix}/trip_return_se"] = g["mean"], g["se"]
                    ppo_train.last_eval[prefix] = res
                if eval_baseline != "none":
                    from tarl_hip.evaluator import EVAL_BASELINES, VecEvaluator, paired_report, paired_scalars
                    if baseline_res is None:      # its engine and tables are released once the numbers are cached
                        b_head, b_kw = EVAL_BASELINES[eval_baseline]
                        baseline_res = VecEvaluator(_eval_engine(eval_env, eval_envs, seed, baseline_agents),
                                                    b_head, **b_kw,
                                                    **({"route_departures": True} if route_departures else {}),
                                                    **({"trip_reward": True} if trip else {})).run(n_eval)
                    rec.update(vec_eval_record("eval_vec_baseline", baseline_res))
                    rep = paired_report(ppo_train.last_eval["eval_vec"], baseline_res)
                    rec.update({f"eval_vec_paired/{k}": v for k, v in paired_scalars(rep).items()})
                    ppo_train.last_eval["eval_vec_baseline"], ppo_train.last_eval["eval_vec_paired"] = baseline_res, rep
        if rec is not None:
            log.write(json.dumps(rec) + "\n")
            log.flush()
            if writer is not None:
                for k, v in rec.items():
                    if k in ("global_step", "iter_seconds") or v is None or isinstance(v, str):
                        continue
                    if isinstance(v, list):
                        if k.endswith("_vc"):
                            writer.add_histogram(k, torch.tensor(v), frames)
                    else:
                        writer.add_scalar(k, v, frames)
        it += 1
    trainer.check_flags()
    sim.set_time(engine.time)
    if log is not None:
        log.close()
    if writer is not None:
        writer.close()
    if checkpoint_path is not None and rank == 0:
        try:
            # the reference saves policy_module.state_dict() of torchrl's ProbabilisticActor: keys module.0.module.<net
            # key> (ProbabilisticTensorDictSequential -> TensorDictModule -> the network). Same names here; tensors are
            # cloned so that the file holds the parameters alone, not the flat training buffer they are views of.
            sd = {f"module.0.module.{k}": v.detach().clone() for k, v in policy_net.state_dict().items()}
            torch.save(sd, checkpoint_path)
        except Exception:  # noqa: BLE001 - the reference swallows checkpoint errors too
            pass
    dist_utils.barrier()
    return None
