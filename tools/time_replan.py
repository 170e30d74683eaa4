#!/usr/bin/env python3
"""Developer tool for DESIGN 4.19: what the day-to-day replanning costs and what it reaches, at BASELINE config 4
(synthetic-10000-16384: 25 x 25 torus, 2 500 roads, 16 384 agents), --frames frames, K = --envs environments.

  1. the select launches on the state a "routes" evaluation leaves behind, alternating in one process, HIP events around
     --launches launches, median (min - max) of --reps after one warm-up round: tarl_fused_select_route (per-environment plan
     and one shared plan) against tarl_fused_select_next_hop_hold on the free-flow table (the parent's kernel: one non-refresh
     frame of the hold router selects with it); the mean route length; and whole runs of T and 2 T frames, wall clock, whose
     difference is the cost of a frame without frame 0's tables: head "routes" (fallback select + route select + frame)
     against head "dijkstra_hold" with refresh_rate 0 (select + frame);
  2. tarl_td_routes against tarl_td_hindsight on the same K A searches (every agent marked DONE for the hindsight call): the
     walk's overhead;
  3. the day table of a --days day run (fraction --fraction), next to "dijkstra_hold" and free_flow on the same engine seed.

    python tools/time_replan.py [--envs 8] [--frames 256] [--days 10] [--fraction 0.1] [--reps 5] [--launches 50]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from tarl_hip import lib, ops  # noqa: E402
from tarl_hip.evaluator import EVAL_BASELINES, VecEvaluator  # noqa: E402
from tarl_hip.replanning import Replanner, replan_lines, replan_report  # noqa: E402
from time_router_hold import SCENARIO, _mean_se, config4, events_us  # noqa: E402

BIN = 60


def med(v):
    return f"{statistics.median(v):9.2f} us ({min(v):.2f} - {max(v):.2f})"


def select_and_frames(engine, K, frames, reps, launches):
    rp = Replanner(engine(K), days=1, link_bin_seconds=BIN)
    res = rp.run(frames)
    ev, eng = rp.ev, rp.eng
    fs, N, A = eng.fs, eng.N, eng.A
    ln = res.route_len[:, 1:]
    print(f"1. select launches at config 4 ({SCENARIO}), K = {K}, on the state after {frames} frames of head routes (day 0: "
          f"free-flow routes); max_hops {rp.max_hops}, mean route length {float(ln[ln > 0].float().mean()):.2f} roads (longest "
          f"{int(ln.max())}), {int((ln <= 0).sum())} of {ln.numel()} agents without a route", flush=True)
    L = lib.load()
    D = int(ev.dests.numel())
    per_env = (res.routes, res.route_len)
    shared = (res.routes[0].contiguous(), res.route_len[0].contiguous())
    s = lib.current_stream()
    forms = {
        "route, per-environment plan": lambda: lib.check(L.tarl_fused_select_route(
            eng.plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, per_env[0].data_ptr(), per_env[1].data_ptr(), A * rp.max_hops,
            rp.max_hops, None, s)),
        "route, shared plan": lambda: lib.check(L.tarl_fused_select_route(
            eng.plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, shared[0].data_ptr(), shared[1].data_ptr(), 0, rp.max_hops, None, s)),
        "hold, shared free-flow table": lambda: lib.check(L.tarl_fused_select_next_hop_hold(
            eng.plan.handle, fs.ref, fs.B, fs.Nmax, fs.A, ev.dest_slot.data_ptr(), ev.table.data_ptr(), 0, D, None, s)),
    }
    times = {k: [] for k in forms}
    for rep in range(reps + 1):
        for k, fn in forms.items():
            us = events_us(fn, launches)
            if rep:
                times[k].append(us)
    for k, v in times.items():
        print(f"  {k:30} {med(v)}   ({N * K} rows x environments)", flush=True)
    # whole runs: wall clock around a device synchronisation. A run of T frames pays for frame 0's tables (one free-flow table
    # for "routes", K of them for the hold router), so the cost of a FRAME is taken from two runs: (2 T frames - T frames) / T
    runs = {"routes (fallback + route + frame)": VecEvaluator(engine(K), "routes", routes=per_env),
            "dijkstra_hold, refresh_rate 0": VecEvaluator(engine(K), "dijkstra_hold", refresh_rate=0)}
    wall = {(k, n): [] for k in runs for n in (1, 2)}
    for rep in range(reps + 1):
        for k, e in runs.items():
            for n in (1, 2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                e.run(n * frames)
                torch.cuda.synchronize()
                if rep:
                    wall[(k, n)].append((time.perf_counter() - t) * 1e6)
    print(f"  whole runs, wall clock: {frames} frames, {2 * frames} frames, and the frames {frames} .. {2 * frames - 1} alone per frame "
          f"(frame 0 builds one free-flow table for routes, K = {K} for the hold router)")
    for k in runs:
        one, two = statistics.median(wall[(k, 1)]), statistics.median(wall[(k, 2)])
        print(f"  {k:38} {one / 1e3:8.2f} ms  {two / 1e3:8.2f} ms  {(two - one) / frames:8.2f} us per frame", flush=True)
    return rp, res


def searches(rp, res, reps):
    """On the road times of the day that select_and_frames ran (its occupancy sums, its bins)."""
    eng = rp.eng
    K, A, N = eng.B, eng.A, eng.N
    meta = res.last.dynamic_gap["meta"]
    veh = rp.ev.occ_acc["veh"]
    H = veh.size(1)
    fpb = torch.tensor(meta["frames_per_bin"], dtype=torch.int32, device=eng.device)
    kw = dict(bin_seconds=meta["bin_seconds"], first_bin=meta["first_bin"])
    tau, env = ops.td_road_times(veh, fpb, *rp.road, **kw)
    ag = eng.agents.clone()
    ag[:, 1:, 8] = 1.0          # every agent searched by the hindsight call too
    out = (rp.best, *rp.new)
    hs_out = torch.empty((K, A), dtype=torch.float64, device=eng.device)
    hs_scratch = torch.empty(ops.td_hindsight_bytes(eng.plan, K, A), dtype=torch.uint8, device=eng.device)
    forms = {"tarl_td_hindsight": lambda: ops.td_hindsight(eng.plan, tau, env, ag, out=hs_out, scratch=hs_scratch, **kw),
             "tarl_td_routes": lambda: ops.td_routes(eng.plan, tau, env, ag, max_hops=rp.max_hops, out=out, scratch=rp.scratch, **kw)}
    times = {k: [] for k in forms}
    for rep in range(reps + 1):
        for k, fn in forms.items():
            us = events_us(fn, 1)
            if rep:
                times[k].append(us)
    same = bool((hs_out[:, 1:] == rp.best[:, 1:]).all())
    print(f"2. the searches: K A = {K} x {A - 1} = {K * (A - 1)} searches, H = {H} bins of {BIN} s, N = {N} roads, max_hops "
          f"{rp.max_hops}; best equal to the bit: {same}")
    for k, v in times.items():
        m = statistics.median(v)
        print(f"  {k:20} {m / 1e3:9.2f} ms ({min(v) / 1e3:.2f} - {max(v) / 1e3:.2f}) = {m / (K * (A - 1)):.3f} us per search", flush=True)
    a, b = statistics.median(times["tarl_td_routes"]), statistics.median(times["tarl_td_hindsight"])
    print(f"  the walk and the copy-out: x{a / b:.3f} the hindsight search")


def day_table(engine, K, frames, days, fraction):
    print(f"3. {days} days at config 4, K = {K}, {frames} frames per day, fraction {fraction}, bins of {BIN} s", flush=True)
    res = Replanner(engine(K), days=days, fraction=fraction, link_bin_seconds=BIN).run(frames)
    for line in replan_lines(replan_report(res)):
        print("  " + line)
    print("  the routers on the same engine seed (dynamic gap on):")
    for name in ("dijkstra_hold", "free_flow"):
        head, kw = EVAL_BASELINES[name]
        r = VecEvaluator(engine(K), head, dynamic_gap=True, link_bin_seconds=BIN, **kw).run(frames)
        if r.domain_exit:
            print(f"  {name:14} DOMAIN EXIT in frames {r.domain_exit_frames}")
            continue
        pe = r.dynamic_gap["per_env"]
        rg = [float((pe["tt_sum"][k] - pe["ht_sum"][k]) / pe["tt_sum"][k]) for k in range(K) if pe["n"][k] > 0]
        (am, ase), (tm, tse), (gm, gse) = _mean_se(r.arrived), _mean_se([t for t in r.avg_travel_time if t is not None]), _mean_se(rg)
        print(f"  {name:14} arrivals {am:10.1f} +- {ase:.1f}   travel time {tm:8.2f} +- {tse:.2f} s   relative gap {gm:8.4f} +- "
              f"{gse:.4f}   {r.computation_time_ms:.0f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--fraction", default="0.1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    engine = config4()
    rp, res = select_and_frames(engine, a.envs, a.frames, a.reps, a.launches)
    searches(rp, res, a.reps)
    del rp, res
    torch.cuda.empty_cache()
    day_table(engine, a.envs, a.frames, a.days, a.fraction)


if __name__ == "__main__":
    main()
