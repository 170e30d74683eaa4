#!/usr/bin/env python3
"""Developer tool: what a policy evaluation costs at BASELINE config 4 (25 x 25 torus, 2 500 roads, 10 000 edges, 16 384
agents; embedding head, MODE, --frames frames), warm, median of --reps runs with min - max:

  * the drop-in pass (src/rl/ppo_trainer._evaluate: SimulatorEnv.rollout, one environment, unfused entry points);
  * tarl_hip.evaluator.VecEvaluator on K in --envs environments (time per evaluation and per environment-frame);
  * one training iteration (VecPPOTrainer.collect + update) at --train-envs environments, the same number of frames;
  * the MODE kernel (tarl_graphdist_mode_rollout) next to the sampler (tarl_graphdist_rollout) on the same logits at
    --kernel-envs environments, with the MODE kernel's share of its byte bound (4 B E read + 2 B N written at 6.3 TB/s).

    python tools/time_eval.py [--frames 256] [--reps 5] [--envs 1,64,1024] [--train-envs 4096] [--kernel-envs 4096]
                              [--only kernels|evaluator] [--head embedding|dijkstra]

``--head dijkstra`` times the shortest-path baseline instead (VecEvaluator head "dijkstra": travel times + K x D reverse
trees every 10 frames, the select kernel every frame), next to the drop-in ``--algo dijkstra --dijkstra-method
per_destination`` loop on the same graph and population, and the select kernel alone against its byte count; a K whose
next-hop table does not fit half the free device memory is reported and left out.

``--only kernels`` runs the last part alone (the run to put under ``rocprofv3 --kernel-trace --stats``), ``--only evaluator``
one VecEvaluator evaluation at the largest K (the run behind profiles/eval_kernel_stats.txt)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.engine import SimEngine  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402

SCENARIO = "synthetic-10000-16384"
COPY_TBPS = 6.3


def spread(fn, reps):
    """Wall-clock milliseconds of ``fn`` (which ends in a device synchronisation): (median, min, max) after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_us(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def runner_for(scenario):
    from src.runner import Runner, RunnerArgs
    r = Runner(RunnerArgs(algo="mpnn+ppo", scenario=scenario, mode="train"))
    r.setup()
    return r


def engine_for(r, K, seed=104729):
    sim = r.env.simulator
    g = sim.graph
    return SimEngine(g.x.clone(), g.edge_index, g.edge_attr, sim.Nmax, r.policy_net.agent_features.clone(),
                     congestion_constant=getattr(g, "congestion_constant", None), num_envs=K, device=g.x.device,
                     timestep=sim.timestep, seed=seed, fused=True)


def time_kernels(r, B, reps):
    sim = r.env.simulator
    g = sim.graph
    plan = ops.Plan(g.edge_index, g.x.size(0))
    N, E = plan.num_nodes, plan.num_edges
    logits = torch.randn((B, E), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    sel8 = torch.zeros((N, B), dtype=torch.uint8, device="cuda")
    lp = torch.empty(B, device="cuda")
    scratch = torch.empty((int(ops._lib.load().tarl_graphdist_rollout_scratch_bytes(plan.handle, B)) + 7) // 8,
                          dtype=torch.float64, device="cuda")
    mode = event_us(lambda: ops.graphdist_mode_rollout(plan, logits, 1.0, choice8=c8, sel8=sel8, log_prob=lp), reps)
    samp = event_us(lambda: ops.graphdist_rollout(plan, logits, 1.0, seed=5, counter=1, choice8=c8, sel8=sel8, log_prob=lp,
                                                  scratch=scratch), reps)
    nbytes = 4 * B * E + 2 * B * N
    bound = nbytes / (COPY_TBPS * 1e12) * 1e6
    print(f"kernels, config 4, B = {B} (HIP events, {reps} launches each, outputs choice8 + sel8 + log_prob):")
    print(f"  tarl_graphdist_mode_rollout  {mode:8.1f} us   byte bound {bound:.1f} us ({nbytes / 1e6:.1f} MB at {COPY_TBPS} TB/s)"
          f" -> {bound / mode * 100:.1f} % of the bound's rate")
    print(f"  tarl_graphdist_rollout       {samp:8.1f} us   (the sampler on the same logits: {bound / samp * 100:.1f} %)", flush=True)


def dropin_dijkstra(T, reps):
    """The drop-in classical loop (``--algo dijkstra --dijkstra-method per_destination``): T steps from a fresh set-up."""
    from src.runner import Runner, RunnerArgs

    def run():
        r = Runner(RunnerArgs(algo="dijkstra", scenario=SCENARIO, mode="eval", dijkstra_method="per_destination",
                              start_end_time=[21540, 21540 + T]))
        r.setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(T):
            r.simulator.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    run()
    out = [run() for _ in range(reps)]
    return statistics.median(out), min(out), max(out)


def time_select(ev, reps):
    """tarl_fused_select_next_hop_dest alone on the evaluator's last state and tables (HIP events)."""
    eng = ev.eng
    us = event_us(lambda: ops.fused_select_next_hop_dest(eng.plan, eng.fs, ev.dest_slot, ev.table), reps)
    nbytes = 21 * eng.N * eng.B
    bound = nbytes / (COPY_TBPS * 1e12) * 1e6
    print(f"  tarl_fused_select_next_hop_dest, K = {eng.B}: {us:8.1f} us   byte count {nbytes / 1e6:.2f} MB (21 B per row and "
          f"environment) = {bound:.2f} us at {COPY_TBPS} TB/s -> {bound / us * 100:.1f} % of that rate", flush=True)


def time_baseline(r, T, reps, envs, only):
    from tarl_hip import lib
    print(f"{SCENARIO}, head dijkstra (refresh every 10 frames), {T} frames; wall clock around a device synchronisation, "
          f"median (min - max) of {reps} runs after one warm-up", flush=True)
    if only is None:
        med, lo, hi = dropin_dijkstra(T, reps)
        base_frame_us = med / T * 1e3
        print(f"drop-in dijkstra loop, per_destination (1 environment): {med:10.1f} ms ({lo:.1f} - {hi:.1f}) for {T} steps = "
              f"{base_frame_us:9.1f} us per environment-frame", flush=True)
    for K in ([max(envs)] if only == "evaluator" else envs):
        try:
            ev = VecEvaluator(engine_for(r, K), "dijkstra")
        except lib.TarlError as exc:
            print(f"VecEvaluator dijkstra K = {K:5d}: not run: {exc}", flush=True)
            continue
        times = []
        for i in range((1 if only == "evaluator" else reps) + 1):       # run 0 warms up; a line per run keeps long runs visible
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ev.run(T)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            print(f"  K = {K}: run {i}{' (warm-up)' if i == 0 else ''} {times[-1]:.1f} ms", flush=True)
        med, lo, hi = statistics.median(times[1:]), min(times[1:]), max(times[1:])
        n, D = res.frames_run, res.settings["destinations"]
        per = med / (n * K) * 1e3
        trees = K * D * ((n + 9) // 10)
        note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
        vs = "" if only else f" ({base_frame_us / per:.1f} x the drop-in loop)"
        print(f"VecEvaluator dijkstra K = {K:5d}, D = {D}: {med:10.1f} ms ({lo:.1f} - {hi:.1f}) for {n} frames = {per:9.3f} us per "
              f"environment-frame{vs}; {trees} trees per run{note}", flush=True)
        if only is None:        # the policy evaluation (embedding head, MODE) at the same K, for comparison
            pol = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net)
            last = []
            pm, plo, phi = spread(lambda: last.append(pol.run(T)), reps)
            pn = last[-1].frames_run
            pnote = f" DOMAIN EXIT in frames {last[-1].domain_exit_frames}" if last[-1].domain_exit else ""
            print(f"VecEvaluator embedding MODE K = {K:5d}: {pm:10.1f} ms ({plo:.1f} - {phi:.1f}) for {pn} frames = "
                  f"{pm / (pn * K) * 1e3:9.3f} us per environment-frame{pnote}", flush=True)
            del pol
        if only is None:
            time_select(ev, 20)
        del ev
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", default="1,64,1024")
    ap.add_argument("--train-envs", type=int, default=4096)
    ap.add_argument("--kernel-envs", type=int, default=4096)
    ap.add_argument("--only", choices=("kernels", "evaluator"), default=None)
    ap.add_argument("--head", choices=("embedding", "dijkstra"), default="embedding")
    a = ap.parse_args()
    T = a.frames
    envs = [int(v) for v in a.envs.split(",")]
    r = runner_for(SCENARIO)
    if a.head == "dijkstra":
        time_baseline(r, T, a.reps, envs, a.only)
        return
    if a.only == "kernels":
        time_kernels(r, a.kernel_envs, 20)
        return
    if a.only == "evaluator":
        ev = VecEvaluator.from_policy_net(engine_for(r, max(envs)), r.policy_net)
        ev.run(T)
        res = ev.run(T)
        print(f"VecEvaluator MODE K = {max(envs)}: {res.frames_run} frames, domain_exit {res.domain_exit}, "
              f"{res.computation_time_ms:.1f} ms")
        return
    print(f"{SCENARIO}, embedding head, MODE, {T} frames; wall clock around a device synchronisation, median (min - max) of "
          f"{a.reps} runs after one warm-up", flush=True)
    # the drop-in pass: the same code on the parent commit
    from src.rl.ppo_trainer import _evaluate
    actor = r._actor(return_log_prob=False)
    lens = []
    med, lo, hi = spread(lambda: lens.append(_evaluate("eval", True, r.env, actor, T)[0]["eval/episode_len"]), a.reps)
    n = lens[-1]
    print(f"drop-in _evaluate (1 environment):   {med:10.1f} ms ({lo:.1f} - {hi:.1f}) for {n} frames = "
          f"{med / n * 1e3:9.1f} us per environment-frame", flush=True)
    base_frame_us = med / n * 1e3
    for K in envs:
        ev = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net)
        last = []
        med, lo, hi = spread(lambda: last.append(ev.run(T)), a.reps)
        res = last[-1]
        n = res.frames_run
        per = med / (n * K) * 1e3
        note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
        print(f"VecEvaluator K = {K:5d}:                {med:10.1f} ms ({lo:.1f} - {hi:.1f}) for {n} frames = "
              f"{per:9.3f} us per environment-frame ({base_frame_us / per:.0f} x the drop-in pass){note}", flush=True)
        del ev
        torch.cuda.empty_cache()
    # one training iteration of the vectorised trainer, the same number of frames
    from tarl_hip.trainer import VecPPOTrainer
    pol, val = r.policy_net, r.value_net
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    extra = [p for nme, p in pol.named_parameters() if not nme.startswith("nodes_embedding")]
    tr = VecPPOTrainer(engine_for(r, a.train_envs, seed=0), pol.nodes_embedding.weight, crit, rollout_steps=T,
                       sub_batch_size=32, extra_params=extra)

    def iteration():
        tr.collect()
        tr.update()
    med, lo, hi = spread(iteration, a.reps)
    print(f"training iteration, {a.train_envs} environments x {T} frames (collect + update, rollout {tr.rollout}): "
          f"{med:10.1f} ms ({lo:.1f} - {hi:.1f})", flush=True)
    try:
        tr.check_flags()
    except Exception as exc:  # noqa: BLE001 - a loaded network may leave the domain; the time above stands
        print(f"  (status word after the iterations: {exc})")
    del tr
    torch.cuda.empty_cache()
    time_kernels(r, a.kernel_envs, 20)


if __name__ == "__main__":
    main()
