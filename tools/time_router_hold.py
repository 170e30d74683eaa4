#!/usr/bin/env python3
"""Developer tool for DESIGN 4.13a: the router that holds one road short of its destination.

  * the select launch alone, HOLD false / true, at BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents) for K in
    --envs environments, on the state and tables a "dijkstra_hold" evaluation of --frames frames leaves behind: HIP events
    around --launches launches, warm, median of --reps with min - max, the forms alternating in one process. With
    --parent-lib (a libtarl_hip.so built from the parent commit, same ABI) that library's tarl_fused_select_next_hop_dest
    takes part in the alternation, on the same buffers;
  * with --table: arrivals and episode return, mean +- se over --table-envs environments, of "dijkstra", "dijkstra_hold" and
    free_flow (dijkstra_hold, refresh_rate 0) on the two 8 x 8 torus cases of the design note and at config 4.

    python tools/time_router_hold.py [--envs 1,64,1024] [--frames 41] [--reps 5] [--launches 50] [--parent-lib PATH]
                                     [--table] [--table-envs 64] [--table-frames 256]"""
import argparse
import ctypes
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from tarl_hip import lib  # noqa: E402
from tarl_hip.engine import EPISODE_START, SimEngine  # noqa: E402
from tarl_hip.evaluator import EVAL_BASELINES, VecEvaluator  # noqa: E402

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


def config4():
    from src.runner import Runner, RunnerArgs
    r = Runner(RunnerArgs(algo="mpnn+ppo", scenario=SCENARIO, mode="train"))
    r.setup()
    sim = r.env.simulator
    g = sim.graph

    def engine(K):
        return SimEngine(g.x.clone(), g.edge_index, g.edge_attr, sim.Nmax, r.policy_net.agent_features.clone(),
                         congestion_constant=getattr(g, "congestion_constant", None), num_envs=K, device=g.x.device,
                         timestep=sim.timestep, seed=104729, fused=True)
    return engine


def time_select(engine, envs, frames, reps, launches, parent):
    print(f"select launch at config 4 ({SCENARIO}) on the state after {frames} frames of head dijkstra_hold; HIP events around "
          f"{launches} launches, median (min - max) of {reps} after one warm-up round, forms alternating", flush=True)
    for K in envs:
        try:
            ev = VecEvaluator(engine(K), "dijkstra_hold")
        except lib.TarlError as exc:
            print(f"K = {K}: not run: {exc}", flush=True)
            continue
        res = ev.run(frames)
        eng, fs = ev.eng, ev.eng.fs
        N, D = eng.N, int(ev.dests.numel())
        # every form through the same bare ctypes call: at these sizes the host's share of a launch is what an op wrapper costs
        L = lib.load()
        args = (eng.plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, ev.dest_slot.data_ptr(), ev.table.data_ptr(), D * N, D, None)
        entries = {"HOLD false": L.tarl_fused_select_next_hop_dest, "HOLD true": L.tarl_fused_select_next_hop_hold}
        if parent is not None:
            entries["parent"] = parent.tarl_fused_select_next_hop_dest
        forms = {k: (lambda f=f: lib.check(f(*args, lib.current_stream()))) for k, f in entries.items()}
        times = {k: [] for k in forms}
        for rep in range(reps + 1):
            for k, fn in forms.items():
                us = events_us(fn, launches)
                if rep:
                    times[k].append(us)
        nbytes = 21 * N * K
        note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
        print(f"K = {K}, D = {D}: {nbytes / 1e6:.2f} MB per launch (21 B per row and environment) = "
              f"{nbytes / (COPY_TBPS * 1e12) * 1e6:.2f} us at {COPY_TBPS} TB/s{note}")
        for k, v in times.items():
            print(f"  {k:10} {statistics.median(v):8.2f} us ({min(v):.2f} - {max(v):.2f})", flush=True)
        del ev, forms
        torch.cuda.empty_cache()


def _mean_se(v):
    n = len(v)
    m = sum(v) / n
    return m, (math.sqrt(sum((x - m) ** 2 for x in v) / (n - 1) / n) if n > 1 else float("nan"))


def table(engine, K, frames4):
    import baseline_restatement as BR
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    N = net.num_roads

    def torus_engine(pop):
        return lambda: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                                 congestion_constant=net.congestion_constant, num_envs=K, seed=3)
    spread = synth.population(128, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    few = BR.few_destination_population(500, N, [3, 17, 40, 66, 90, 101, 120, 127], seed=7, t0=EPISODE_START,
                                        t1=EPISODE_START + 40)
    cases = (("8 x 8 torus, 128 agents bound anywhere, 300 frames", torus_engine(spread), 300),
             ("8 x 8 torus, 500 agents bound for 8 roads, 120 frames", torus_engine(few), 120),
             (f"config 4 ({SCENARIO}), {frames4} frames", lambda: engine(K), frames4))
    print(f"arrivals and episode return, mean +- se over K = {K} environments (one engine seed per case, the same for every router)")
    for label, make, T in cases:
        print(label, flush=True)
        for name, (head, kw) in EVAL_BASELINES.items():
            res = VecEvaluator(make(), head, **kw).run(T)
            if res.domain_exit:
                print(f"  {name:14} DOMAIN EXIT in frames {res.domain_exit_frames}", flush=True)
                continue
            (am, ase), (rm, rse) = _mean_se(res.arrived), _mean_se(res.episode_return)
            print(f"  {name:14} arrivals {am:10.2f} +- {ase:.2f}   return {rm:14.1f} +- {rse:.1f}   on the way at the end "
                  f"{_mean_se(res.on_way)[0]:.1f}   {res.computation_time_ms:.0f} ms", flush=True)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,64,1024")
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--table-frames", type=int, default=256)
    a = ap.parse_args()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        f = parent.tarl_fused_select_next_hop_dest
        f.restype, f.argtypes = lib.SIGNATURES["tarl_fused_select_next_hop_dest"]
        assert parent.tarl_abi_version() == lib.load().tarl_abi_version(), "the parent library has another ABI"
    engine = config4()
    time_select(engine, [int(v) for v in a.envs.split(",")], a.frames, a.reps, a.launches, parent)
    if a.table:
        table(engine, a.table_envs, a.table_frames)


if __name__ == "__main__":
    main()
