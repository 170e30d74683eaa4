#!/usr/bin/env python3
"""Developer tool for DESIGN 4.23: first-hop routing (``--route-departures``).

  (a) the two launches at BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents) for B in --envs environments, on the
      state that --frames live frames of the sampled embedding policy leave behind: tarl_fused_pending_departures (its memset
      and its window scan), the same with the window withdrawn (every agent looked at), tarl_fused_route_departures, and
      beside them tarl_fused_hold_policy_actions on the same state. HIP events around --launches launches, warm, median of
      --reps with min - max, in one session; and the bytes each must move.
  (b) with --table: arrivals, mean travel time, episode return and ON_WAY - queued, mean +- se over --table-envs
      environments, without and with the rule: ``free_flow`` and ``dijkstra_hold`` on the 8 x 8 torus (128 agents bound
      anywhere, 300 frames) and at config 4 (--table-frames frames), and the ``embedding_dijkstra`` MODE policy under the hold
      rule.

    python tools/time_departures.py [--envs 64,4096] [--frames 60] [--reps 5] [--launches 50] [--table] [--table-envs 64]
                                    [--table-frames 256]"""
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
from tarl_hip.evaluator import VecEvaluator, router_buffers  # noqa: E402

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


def time_launches(engine, envs, frames, reps, launches):
    print(f"(a) the launches at config 4 ({SCENARIO}) on the state after {frames} live frames of the sampled embedding "
          f"policy, one free-flow table of every destination; HIP events around {launches} launches, median (min - max) of {reps} after one warm-up round", flush=True)
    L = lib.load()
    for B in envs:
        eng = engine(B)
        eng.reset()
        fs = eng.fs
        dests, dest_slot, weights, tbl, scratch = router_buffers(eng, None, 1)      # one free-flow table, as a policy head has it
        ops.fused_edge_travel_time(eng.plan, fs, out=weights)
        ops.destination_trees_batched(eng.plan, weights[:1], dests, out=tbl, scratch=scratch)
        tbl = tbl[0]
        eng.prepare_policy(torch.randn(eng.N, generator=torch.Generator().manual_seed(0)).to(eng.device), 1.0)
        for _ in range(frames):
            eng.frame_fused()
        fs.check_flags()
        t = float(eng.time)
        N, A = eng.N, eng.A
        pend = torch.empty((N, B), dtype=torch.int32, device=eng.device)
        routed = torch.zeros(B, dtype=torch.int32, device=eng.device)
        held = torch.zeros(B, dtype=torch.int32, device=eng.device)
        s = lib.current_stream()
        f_pend = lambda: lib.check(L.tarl_fused_pending_departures(eng.plan.handle, fs.ref, B, fs.Nmax, A, t, pend.data_ptr(), s))  # noqa: E731
        stride, D = ops._departure_table(eng.plan, fs, dest_slot, tbl)
        f_route = lambda: lib.check(L.tarl_fused_route_departures(eng.plan.handle, fs.ref, B, fs.Nmax, A, pend.data_ptr(),  # noqa: E731
                                                                  dest_slot.data_ptr(), tbl.data_ptr(), stride, D, None,
                                                                  routed.data_ptr(), s))
        Ag, abs_ = ops._agents(eng.agents, B)
        f_hold = lambda: lib.check(L.tarl_fused_hold_policy_actions(eng.plan.handle, fs.ref, B, fs.Nmax, eng.agents.data_ptr(),  # noqa: E731
                                                                    Ag, abs_, None, held.data_ptr(), s))
        f_set = lambda: pend.fill_(-1)                                                                                     # noqa: E731
        f_pend()
        f_route()
        pending = int((pend >= 0).sum())
        first = int(routed.sum())
        lo = fs.cur_lo.long()
        due = (fs.a_dep_sorted <= t).sum(1)
        window = int((due - lo).clamp(min=0).sum())
        ready = int(((fs.a_status == 0) & (fs.a_dep <= t)).sum())
        empty = int(((fs.hdp[..., 0] & 127) == 0).sum())
        times = {}
        for name, fn in (("pending", f_pend), ("route", f_route), ("hold", f_hold), ("fill of N B words alone", f_set)):
            fn()
            times[name] = [events_us(fn, launches) for _ in range(reps + 1)][1:]
        saved = fs.struct.a_order
        fs.struct.a_order = None
        f_pend()
        times["pending, every agent"] = [events_us(f_pend, launches) for _ in range(reps + 1)][1:]
        fs.struct.a_order = saved
        pairs = N * B
        b_pend = 4 * pairs + 17 * window + 64 * B + 4 * ready
        b_all = 4 * pairs + 5 * A * B + 8 * ready
        b_route = 4 * pairs + 4 * pending + first * 17
        b_hold = 8 * pairs + (pairs - empty) * 5
        print(f"B = {B}: {pairs} (road, environment) pairs, {empty} of them empty; window entries from the cursor to the last due "
              f"one {window} ({window / B:.1f} per environment), {ready} ready agents, {pending} pending roads, {first} rows routed "
              f"by the first launch", flush=True)
        for name, nbytes, what in (
                ("pending", b_pend, "4 B of pend set per pair, 16 + 1 B per window entry, one 64-lane step of the window per "
                                    "environment, a 4 B atomic per ready agent"),
                ("pending, every agent", b_all, "4 B of pend set per pair, 4 + 1 B per agent, 4 + 4 B per ready agent"),
                ("route", b_route, "4 B of pend per pair, 4 B of hdp per pending road, destination + slot + table word + 1 (+ 4) "
                                   "B stored per routed row"),
                ("hold", b_hold, "8 B of hdp per pair, 1 + 4 B per occupied row")):
            print(f"  {name:22} {med(times[name])}   {nbytes / 1e6:8.2f} MB = {nbytes / (COPY_TBPS * 1e12) * 1e6:6.2f} us at "
                  f"{COPY_TBPS} TB/s ({what})", flush=True)
        print(f"  {'fill of N B words alone':22} {med(times['fill of N B words alone'])}")
        pair = statistics.median(times["pending"]) + statistics.median(times["route"])
        print(f"  pending + route = {pair:.2f} us = {pair / statistics.median(times['hold']):.2f} x the hold launch", flush=True)
        del eng, fs, tbl, scratch, weights
        torch.cuda.empty_cache()


def _mean_se(v):
    v = [float(x) for x in v]
    n = len(v)
    m = sum(v) / n
    return m, (math.sqrt(sum((x - m) ** 2 for x in v) / (n - 1) / n) if n > 1 else float("nan"))


def table(engine, K, frames4):
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    spread = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    torus = lambda: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, spread.cuda(),        # noqa: E731
                              congestion_constant=net.congestion_constant, num_envs=K, seed=3)
    cases = (("8 x 8 torus, 128 agents bound anywhere, 300 frames", torus, 300),
             (f"config 4 ({SCENARIO}), {frames4} frames", lambda: engine(K), frames4))
    print(f"(b) mean +- se over K = {K} environments (one engine seed per case, the same for every row); policy = the "
          f"embedding_dijkstra head in MODE (free-flow all-pairs prior, weight 1, embedding 0.01 N(0, 1)) under --policy-hold")
    for label, make, T in cases:
        print(label, flush=True)
        for name in ("free_flow", "dijkstra_hold", "policy + hold"):
            for route in (False, True):
                eng = make()
                kw = dict(route_departures=True) if route else {}
                if name == "policy + hold":
                    ff = eng._x[0, :, 3 * eng.Nmax + 2][eng.edge_index[1].to(eng.device)].contiguous()
                    dist = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
                    emb = (0.01 * torch.randn(eng.N, generator=torch.Generator().manual_seed(5))).to(eng.device)
                    ev = VecEvaluator(eng, "embedding_dijkstra", emb=emb, prior_table=dist, prior_weight=1.0, policy_hold=True, **kw)
                else:
                    ev = VecEvaluator(eng, "dijkstra_hold", refresh_rate=0 if name == "free_flow" else 10, **kw)
                res = ev.run(T)
                if res.domain_exit:
                    print(f"  {name:14} {'with' if route else 'without':8} DOMAIN EXIT in frames {res.domain_exit_frames}", flush=True)
                    continue
                x = eng.x
                lost = (eng.agents[:, :, 7].sum(1) - x[:, :, 3 * eng.Nmax + 1].sum(1)).tolist()
                tt = [v for v in res.avg_travel_time if v is not None and v == v]
                (am, ase), (rm, rse), (lm, lse) = _mean_se(res.arrived), _mean_se(res.episode_return), _mean_se(lost)
                tm, tse = _mean_se(tt) if tt else (float("nan"), float("nan"))
                extra = f"   routed {_mean_se(res.departures_routed)[0]:.1f}" if res.departures_routed is not None else ""
                print(f"  {name:14} {'with' if route else 'without':8} arrivals {am:10.2f} +- {ase:.2f}   travel time {tm:8.2f} +- "
                      f"{tse:.2f} s   return {rm:14.1f} +- {rse:.1f}   ON_WAY - queued {lm:8.2f} +- {lse:.2f}{extra}   "
                      f"{res.computation_time_ms:.0f} ms", flush=True)
                del ev, eng
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--table-frames", type=int, default=256)
    a = ap.parse_args()
    engine = config4()
    time_launches(engine, [int(v) for v in a.envs.split(",")], a.frames, a.reps, a.launches)
    if a.table:
        table(engine, a.table_envs, a.table_frames)


if __name__ == "__main__":
    main()
