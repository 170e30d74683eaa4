#!/usr/bin/env python3
"""Developer tool for DESIGN 4.25: the per-agent path trace (``--eval-paths``).

  (a) tarl_fused_path_trace at BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents) for B in --envs environments, on
      the state that --frames live frames of the sampled embedding policy leave behind, traced from the first frame on: the
      launch on a state it has already seen (what most rows of most frames are: two loads and out), the launch right after a
      reset (every head a first sighting), and beside them a device-to-device copy of the hdp buffer and the reset alone. HIP
      events around --launches launches, warm, median of --reps with min - max, in one session.
  (b) a --eval-frames frame config-4 evaluation (embedding head, MODE) at --eval-envs environments without and with the trace:
      wall time of each, alternating --reps times.
  (c) with --table: the report's own numbers on the 8 x 8 torus (128 agents bound anywhere, 300 frames, --table-envs
      environments) for ``free_flow`` and ``dijkstra_hold`` with the first-hop rule, for the sampled embedding head and for
      the ``goal_mlp`` head cloned as in DESIGN 4.21 / 4.24 (two DAgger iterations, expert ``dijkstra``), MODE under
      ``policy_hold`` and ``route_departures``.
  (d) with --bench-lines FILE: the JSON result lines of ``bench.py --gpus 1 --steps 6 --warmup 2`` runs, each prefixed with
      ``[this i]`` or ``[parent i]`` (this commit and its parent, alternating), as one line per run.

    python tools/time_path_trace.py [--envs 64,4096] [--frames 60] [--reps 5] [--launches 50] [--max-hops 64]
                                    [--eval-envs 64] [--eval-frames 256] [--table] [--table-envs 64] [--bench-lines FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import lib, ops  # noqa: E402
from tarl_hip.engine import EPISODE_START, SimEngine  # noqa: E402
from tarl_hip.evaluator import VecEvaluator, path_lines, path_report  # noqa: E402

SCENARIO = "synthetic-10000-16384"


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


def config4():
    from src.runner import Runner, RunnerArgs
    r = Runner(RunnerArgs(algo="mpnn+ppo", scenario=SCENARIO, mode="train"))
    r.setup()
    sim = r.env.simulator
    g = sim.graph
    ff = g.x[:, sim.h.FREE_FLOW_TIME_TRAVEL][g.edge_index[1]].contiguous()

    def engine(K):
        return SimEngine(g.x.clone(), g.edge_index, g.edge_attr, sim.Nmax, r.policy_net.agent_features.clone(),
                         congestion_constant=getattr(g, "congestion_constant", None), num_envs=K, device=g.x.device,
                         timestep=sim.timestep, seed=104729, fused=True)
    return engine, ff


def _tables(eng, w):
    N = eng.N
    d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
    d = d[(d >= 0) & (d < N)].contiguous()
    slot = torch.full((N,), -1, dtype=torch.int32, device=eng.device)
    slot[d] = torch.arange(d.numel(), dtype=torch.int32, device=eng.device)
    _, dist = ops.destination_trees(eng.plan, w, d, want_next_hop=False, want_dist=True)
    return w, dist, slot


def time_launches(engine, ff, envs, frames, reps, launches, L):
    print(f"(a) tarl_fused_path_trace at config 4 ({SCENARIO}), {L} roads kept per trace, free-flow weights and the distances to "
          f"every destination, traced over {frames} live frames of the sampled embedding policy; HIP events around {launches} "
          f"launches, median (min - max) of {reps} after one warm-up round", flush=True)
    for B in envs:
        eng = engine(B)
        eng.reset()
        fs = eng.fs
        tables = _tables(eng, ff.to(eng.device, torch.float32))
        st = ops.path_trace_state(B, eng.A, L, eng.device)
        ops.path_trace_reset(st)
        eng.prepare_policy(torch.randn(eng.N, generator=torch.Generator().manual_seed(0)).to(eng.device), 1.0)
        for _ in range(frames):
            eng.frame_fused()
            ops.fused_path_trace(eng.plan, fs, st, *tables)
        fs.check_flags()
        assert not bool(st.bad.any())
        copy = torch.empty_like(fs.hdp)
        fresh = st.clone()
        f_seen = lambda: ops.fused_path_trace(eng.plan, fs, st, *tables)                      # noqa: E731
        # the C entry point itself, without the checks of the Python wrapper: at B = 64 the wrapper takes longer than the kernel
        args = (eng.plan.handle, fs.ref, B, fs.Nmax, eng.A, L, *st._ptrs(), *(t.data_ptr() for t in tables), tables[1].size(0),
                lib.current_stream())
        entry = lib.load().tarl_fused_path_trace
        f_direct = lambda: lib.check(entry(*args))                                            # noqa: E731
        f_reset = lambda: ops.path_trace_reset(fresh)                                         # noqa: E731
        f_first = lambda: (ops.path_trace_reset(fresh), ops.fused_path_trace(eng.plan, fs, fresh, *tables))      # noqa: E731
        f_copy = lambda: copy.copy_(fs.hdp)                                                   # noqa: E731
        times = {}
        for name, fn in (("trace, state seen", f_seen), ("the C call alone", f_direct), ("reset + trace", f_first), ("reset alone", f_reset),
                         ("copy of hdp", f_copy)):
            fn()
            times[name] = [events_us(fn, launches) for _ in range(reps + 1)][1:]
        pairs = eng.N * B
        occupied = int(((fs.hdp[..., 0] & 127) != 0).sum())
        seen = int((st.roads > 0).sum())
        print(f"B = {B}: {pairs} (road, environment) pairs, {occupied} of them occupied; after {frames} frames {seen} agents seen, "
              f"{int(st.roads.sum())} roads in all, {int((st.revisits > 0).sum())} traces with a loop, "
              f"{int((st.roads > L).sum())} truncated", flush=True)
        for name in times:
            print(f"  {name:20} {med(times[name])}", flush=True)
        m = lambda k: statistics.median(times[k])      # noqa: E731
        print(f"  trace / copy of hdp = {m('trace, state seen') / m('copy of hdp'):.2f} on a state already seen "
              f"({m('the C call alone') / m('copy of hdp'):.2f} for the C call alone), "
              f"{(m('reset + trace') - m('reset alone')) / m('copy of hdp'):.2f} right after a reset (every head a first "
              f"sighting); must move {4 * pairs / 1e6:.2f} MB of hdp words (8 B apart) + 4 B of last_road per occupied row = "
              f"{(4 * pairs + 4 * occupied) / 1e6:.2f} MB, the copy {16 * pairs / 1e6:.2f} MB read + written", flush=True)
        del eng, fs, st, fresh, tables, copy
        torch.cuda.empty_cache()


def time_eval(engine, ff, K, T, reps):
    print(f"(b) a {T}-frame config-4 evaluation at K = {K} (embedding head, MODE), wall time of run() without the trace, with it "
          f"(64 roads kept: the (K, A, 64) routes go to the host after the run) and with it and no routes kept, alternating "
          f"{reps} times after one warm-up run of each", flush=True)
    emb = torch.randn(engine(1).N, generator=torch.Generator().manual_seed(0)).cuda()
    evs = {"without": VecEvaluator(engine(K), "embedding", emb=emb),
           "paths, 64 kept": VecEvaluator(engine(K), "embedding", emb=emb, paths=True, path_weights=ff),
           "paths, 0 kept": VecEvaluator(engine(K), "embedding", emb=emb, paths=True, path_weights=ff, path_max_hops=0)}
    ms = {k: [] for k in evs}
    for i in range(reps + 1):
        for k, ev in evs.items():
            res = ev.run(T)
            if i:
                ms[k].append(res.computation_time_ms)
    for k, v in ms.items():
        print(f"  {k:16} {statistics.median(v):9.1f} ms ({min(v):.1f} - {max(v):.1f})", flush=True)


def table(K):
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    make = lambda: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),        # noqa: E731
                             congestion_constant=net.congestion_constant, num_envs=K, seed=3)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous()
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(11)).cuda()
    print(f"(c) the report on the 8 x 8 torus, 128 agents bound anywhere, 300 frames, K = {K}, free-flow weights", flush=True)
    for name, head, kw, det in (("free_flow + first hop", "dijkstra_hold", dict(refresh_rate=0, route_departures=True), True),
                                ("dijkstra_hold + first hop", "dijkstra_hold", dict(refresh_rate=10, route_departures=True), True),
                                ("embedding, sampled", "embedding", dict(emb=emb), False)):
        res = VecEvaluator(make(), head, paths=True, trips=True, trip_free_flow=ff, **kw).run(300, deterministic=det)
        _block(name, res)
    pol = cloned_goal_mlp(net, pop)
    res = VecEvaluator.from_policy_net(make(), pol, policy_hold=True, route_departures=True, paths=True, trips=True,
                                       trip_free_flow=ff).run(300)
    _block("goal_mlp, cloned (2 DAgger iterations), MODE, policy_hold + first hop", res)


def _block(name, res):
    print(f"--- {name} ---")
    for line in path_lines(path_report(res)):
        if line.startswith("By departure"):
            break
        print("  " + line, flush=True)


def cloned_goal_mlp(net, pop, iterations=2):
    """The goal_mlp head cloned from the ``dijkstra`` expert as tools/time_trip_reward.py --ppo clones it (part 3):
    16 environments, 512 samples, 4 epochs of minibatches of 64, lr 0.01, DAgger."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip.imitation import BCTrainer
    from tarl_hip.trainer import VecPPOTrainer
    N, Nmax, T = net.num_roads, net.Nmax, 300
    engine = lambda B, seed: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, Nmax, pop.cuda(),        # noqa: E731
                                       congestion_constant=net.congestion_constant, num_envs=B, seed=seed)
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]].cuda().contiguous()
    torch.manual_seed(1)
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.prior_method = "all_pairs"
    pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * Nmax:]))
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l, gm = val.final_mlp, pol.goal_mlp
    tr = VecPPOTrainer(engine(64, 5), pol.nodes_embedding.weight,
                       [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias], rollout_steps=T,
                       extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")],
                       policy="goal_mlp", goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias],
                       prior_table=pol.dist_matrix, policy_hold=True, route_departures=True)
    bc = BCTrainer(tr, engine(16, 11), expert="dijkstra", driver="dagger", frames=T, samples=512, epochs=4, batch=64, lr=1e-2)
    for _ in range(iterations):
        r = bc.iterate()
        print(f"    [bc {r['iteration']}] {r['driver']:6} loss {r['loss_first']:.4f} -> {r['loss_last']:.4f}  accuracy "
              f"{r['accuracy_before']:.3f} -> {r['accuracy_after']:.3f}  arrivals {r['arrivals']:.1f}", flush=True)
    return pol


def bench_lines(path):
    import json
    import re
    print("(d) bench.py --gpus 1 --steps 6 --warmup 2, this commit and its parent alternating on one device", flush=True)
    for line in open(path):
        m = re.match(r"\[(\w+) (\d+)\] (\{.*)", line.strip())
        if m:
            doc = json.loads(m.group(3))
            print(f"  {m.group(1):6} {m.group(2)}  {doc['ms_per_step']:8.2f} ms per step  {doc['value']:.0f} {doc['unit']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--max-hops", type=int, default=64)
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--eval-frames", type=int, default=256)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    engine, ff = config4()
    time_launches(engine, ff, [int(v) for v in a.envs.split(",")], a.frames, a.reps, a.launches, a.max_hops)
    time_eval(engine, ff, a.eval_envs, a.eval_frames, a.reps)
    if a.table:
        table(a.table_envs)
    if a.bench_lines:
        bench_lines(a.bench_lines)


if __name__ == "__main__":
    main()
