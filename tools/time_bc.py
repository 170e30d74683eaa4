#!/usr/bin/env python3
"""Developer tool for DESIGN 4.21: behaviour cloning of the shortest-path router (``--pretrain-bc``).

  (a) both kernels at BASELINE config 4 (25 x 25 torus, 2 500 roads, 10 000 edges, 16 384 agents): the label launch on the
      state that --frames frames of the holding router leave behind on B = 64 environments, and the loss launch
      (tarl_graphdist_bc, forward and backward) for M in --samples on random logits and the select kernel's bytes of that
      state as labels (every road labelled: the most work the kernel can have), against
      their byte counts at the 6.3 TB/s a copy reaches and, for the loss, against the existing chain graphdist_softmax ->
      graphdist_logprob_entropy forward -> backward at the same M. HIP events around --launches launches, warm, median of
      --reps with min - max.
  (b) with --table: arrivals and episode return under ``policy_hold``, MODE, K = --table-envs environments, of every head
      in --heads untrained and after --iterations DAgger iterations, next to ``dijkstra_hold``, on the 8 x 8 torus with
      128 agents (300 frames) and, with --table-config4, at config 4 (--table-frames frames).

    python tools/time_bc.py [--frames 60] [--samples 32,4096] [--reps 5] [--launches 20] [--parts a]
                            [--table] [--heads embedding,edge_mlp] [--iterations 6] [--table-envs 64] [--table-config4]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from tarl_hip import lib, ops  # noqa: E402
from tarl_hip.engine import EPISODE_START, SimEngine  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402

SCENARIO = "synthetic-10000-16384"
COPY_TBPS = 6.3


def events_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches * 1e3


def med(v):
    return f"{statistics.median(v):9.2f} us ({min(v):.2f} - {max(v):.2f})"


def timed(fn, reps, launches):
    return [events_us(fn, launches) for _ in range(reps + 1)][1:]


def config4():
    from src.runner import Runner, RunnerArgs
    r = Runner(RunnerArgs(algo="mpnn+ppo", scenario=SCENARIO, mode="train"))
    r.setup()
    sim = r.env.simulator
    g = sim.graph
    return dict(x=g.x.clone(), edge_index=g.edge_index.cpu(), edge_attr=g.edge_attr, Nmax=sim.Nmax,
                pop=r.policy_net.agent_features.clone(), cc=getattr(g, "congestion_constant", None))


def engine_of(c, K, seed=104729):
    return SimEngine(c["x"].clone().cuda(), c["edge_index"], c["edge_attr"], c["Nmax"], c["pop"].clone().cuda(),
                     congestion_constant=c["cc"], num_envs=K, seed=seed)


def time_kernels(c, frames, samples, reps, launches):
    B = 64
    ev = VecEvaluator(engine_of(c, B), "dijkstra_hold")
    ev.run(frames)
    eng, fs = ev.eng, ev.eng.fs
    N, E = eng.N, eng.E
    occupied = int(((fs.hdp[..., 0] & 127) != 0).sum())
    labels = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.fused_expert_labels(eng.plan, fs, ev.dest_slot, ev.table, out=labels, n_labelled=cnt)
    print(f"(a) config 4 ({SCENARIO}), B = {B}, state after {frames} frames of dijkstra_hold: {N * B} pairs, {occupied} occupied "
          f"({100.0 * occupied / (N * B):.1f} %), {int(cnt.sum())} labelled; HIP events around {launches} launches, median (min - "
          f"max) of {reps} after one warm-up round", flush=True)
    t = timed(lambda: ops.fused_expert_labels(eng.plan, fs, ev.dest_slot, ev.table, out=labels, n_labelled=cnt), reps, launches)
    nbytes = 9 * N * B
    print(f"  labels   {med(t)}   {nbytes / 1e6:.2f} MB (8 B of hdp per pair read, 1 B written) = "
          f"{nbytes / (COPY_TBPS * 1e12) * 1e6:.2f} us at {COPY_TBPS} TB/s; the occupied rows' three 4-byte gathers are not in it",
          flush=True)
    t = timed(lambda: ops.fused_select_next_hop_dest(eng.plan, fs, ev.dest_slot, ev.table, choice8=labels), reps, launches)
    print(f"  (select) {med(t)}   fused_select_next_hop_dest with choice8 on the same state, for scale", flush=True)
    L = lib.load()
    for M in samples:
        g = torch.Generator(device="cuda").manual_seed(M)
        logits = torch.randn((M, E), device="cuda", generator=g)
        lab = labels[torch.arange(M, device="cuda") % B].contiguous()
        need = int(L.tarl_graphdist_bc_scratch_bytes(eng.plan.handle, M))
        scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        nll = torch.empty(M, dtype=torch.float64, device="cuda")
        nl, nh = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
        grad = torch.empty_like(logits)

        def bc(gp):
            lib.check(L.tarl_graphdist_bc(eng.plan.handle, logits.data_ptr(), M, 1.0, lab.data_ptr(), 1e-3, nll.data_ptr(),
                                          nl.data_ptr(), nh.data_ptr(), gp, scratch.data_ptr(), lib.current_stream()))
        t_fb = timed(lambda: bc(grad.data_ptr()), reps, launches)
        t_f = timed(lambda: bc(None), reps, launches)
        choice = torch.full((M, N), -1, dtype=torch.int32, device="cuda")
        choice[:] = torch.arange(N, device="cuda", dtype=torch.int32) * (E // N)       # the first out-edge of every road
        glp = torch.full((M,), -1e-3, device="cuda")

        def chain():
            p = ops.graphdist_softmax(eng.plan, logits, 1.0)
            ops.graphdist_logprob_entropy(eng.plan, p, choice=choice, want_entropy=False)
            ops.graphdist_logprob_entropy_bwd(eng.plan, p, 1.0, choice=choice, grad_log_prob=glp)
        t_c = timed(chain, reps, launches)
        nbytes = 8 * M * E + M * N
        print(f"  M = {M}: {int(nl.sum())} labelled nodes of {M * N} (labels = the select launch's bytes above)\n"
              f"    loss fwd + bwd {med(t_fb)}   {nbytes / 1e6:.2f} MB (4 M E read, 4 M E written, M N label bytes) = "
              f"{nbytes / (COPY_TBPS * 1e12) * 1e6:.2f} us at {COPY_TBPS} TB/s\n"
              f"    loss fwd only  {med(t_f)}\n"
              f"    chain          {med(t_c)}   softmax -> logprob_entropy fwd -> bwd (three launches, two allocations, "
              f"every node labelled)", flush=True)
        del logits, grad, choice
        torch.cuda.empty_cache()


def _mean_se(v):
    n = len(v)
    m = sum(v) / n
    return m, (math.sqrt(sum((x - m) ** 2 for x in v) / (n - 1) / n) if n > 1 else float("nan"))


def _row(name, res, extra=""):
    if res.domain_exit:
        print(f"  {name:28} DOMAIN EXIT in frames {res.domain_exit_frames}", flush=True)
        return
    (am, ase), (rm, rse) = _mean_se(res.arrived), _mean_se(res.episode_return)
    print(f"  {name:28} arrivals {am:10.2f} +- {ase:.2f}   return {rm:14.1f} +- {rse:.1f}{extra}", flush=True)


def table_case(label, c, T, K, heads, iterations, bc_envs, samples, epochs, lr):
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip.imitation import BCTrainer
    from tarl_hip.trainer import VecPPOTrainer
    print(label, flush=True)
    _row("dijkstra_hold", VecEvaluator(engine_of(c, K, seed=3), "dijkstra_hold").run(T))
    N = c["x"].size(0)
    for head in heads:
        torch.manual_seed(1)
        pol = MPNNPolicyNet(c["edge_index"], N, None, device="cuda")
        pol.policy_head = head
        val = MPNNValueNetSimple(c["edge_index"], N, device="cuda")
        l, m = val.final_mlp, pol.edge_mlp
        kw = dict(edge_mlp_params=[m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]) if head == "edge_mlp" else {}
        ppo = VecPPOTrainer(engine_of(c, 2, seed=5), pol.nodes_embedding.weight,
                            [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias], rollout_steps=4,
                            sub_batch_size=4, extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")],
                            policy=head, **kw)
        _row(f"{head}, untrained + hold", VecEvaluator.from_policy_net(engine_of(c, K, seed=3), pol, policy_hold=True).run(T))
        bc = BCTrainer(ppo, engine_of(c, bc_envs, seed=11), expert="dijkstra", driver="dagger", frames=T, samples=samples,
                       epochs=epochs, batch=64, lr=lr)
        for _ in range(iterations):
            r = bc.iterate()
            print(f"    [bc {r['iteration']}] {r['driver']:6} labelled {r['labelled']:8d} ({100 * r['labelled_share']:.1f} %)  loss "
                  f"{r['loss_first']:.4f} -> {r['loss_last']:.4f}  accuracy {r['accuracy_before']:.3f} -> {r['accuracy_after']:.3f}  "
                  f"arrivals {r['arrivals']:.1f}  {r['collect_seconds']:.1f} s + {r['update_seconds']:.1f} s", flush=True)
        _row(f"{head}, cloned + hold", VecEvaluator.from_policy_net(engine_of(c, K, seed=3), pol, policy_hold=True).run(T))
        del bc, ppo, pol
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--samples", default="32,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parts", default="a")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-config4", action="store_true")
    ap.add_argument("--heads", default="embedding,edge_mlp")
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--table-frames", type=int, default=256)
    ap.add_argument("--bc-envs", type=int, default=16)
    ap.add_argument("--bc-samples", type=int, default=512)
    ap.add_argument("--bc-epochs", type=int, default=4)
    ap.add_argument("--bc-lr", type=float, default=1e-2)
    a = ap.parse_args()
    print("# tools/time_bc.py " + " ".join(sys.argv[1:]) + "   (one process; DESIGN 4.21)", flush=True)
    c4 = config4() if ("a" in a.parts or a.table_config4) else None
    if "a" in a.parts:
        time_kernels(c4, a.frames, [int(v) for v in a.samples.split(",")], a.reps, a.launches)
    if a.table or a.table_config4:
        print(f"(b) arrivals and episode return under policy_hold, MODE, mean +- se over K = {a.table_envs} environments; cloned = "
              f"{a.iterations} DAgger iterations (expert dijkstra) on {a.bc_envs} environments, {a.bc_samples} samples, "
              f"{a.bc_epochs} epochs of minibatches of 64, lr {a.bc_lr}", flush=True)
        args = (a.heads.split(","), a.iterations, a.bc_envs, a.bc_samples, a.bc_epochs, a.bc_lr)
        if a.table:
            from tarl_hip import synth
            net = synth.torus_network(8, 8)
            pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
            c = dict(x=net.x, edge_index=net.edge_index, edge_attr=net.edge_attr, Nmax=net.Nmax, pop=pop, cc=net.congestion_constant)
            table_case("8 x 8 torus, 128 agents bound anywhere, 300 frames", c, 300, a.table_envs, *args)
        if a.table_config4:
            table_case(f"config 4 ({SCENARIO}), {a.table_frames} frames", c4, a.table_frames, a.table_envs, *args)


if __name__ == "__main__":
    main()
