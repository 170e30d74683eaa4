#!/usr/bin/env python3
"""Developer tool: what the dynamic relative gap costs in a vectorised evaluation (embedding head, MODE, --frames frames, bins
of --bin seconds), warm, median of --reps runs with min - max, on BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents)
at K = 1, 8 and 64:

  * the time the flag adds per run: VecEvaluator without it and with ``dynamic_gap=True`` (the occupancy ring and its
    accumulate launches, ``tarl_td_road_times``, one ``tarl_td_hindsight`` search per arrived (environment, agent), the fp64
    reductions and their copies to the host), in the same process on engines of one seed, the runs of the two alternating;
    with ``--parent FILE`` also the VecEvaluator of another evaluator.py — the parent commit's, e.g. from
    ``git show HEAD~1:tarl-simulator_amd/tarl_hip/evaluator.py > FILE`` — on the same library, alternating with the other two:
    the flag-off figure must not have moved, and the added time is taken against it;
  * the time per search against the time per tree of ``tarl_dest_trees_batched`` on the same graph and K (HIP events): the
    static reverse tree is the same frontier scheme without the bin lookup. An untrained MODE policy delivers few agents in a
    short run, so the searches are timed on a copy of the agent tables with DONE set for the first --agents agents of every
    environment (K x --agents searches under the run's own road times), the trees over the K x D (environment, distinct
    destination) pairs under every environment's congested travel times.

    python tools/time_dynamic_gap.py [--frames 256] [--bin 60] [--reps 5] [--envs 1,8,64] [--agents 4096] [--parent FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_eval import engine_for, event_us, runner_for  # noqa: E402
from time_link_counts import alternating, parent_class  # noqa: E402
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402

SCENARIO = "synthetic-10000-16384"


def time_searches(ev, meta, agents_cap, reps):
    eng, b = ev.eng, ev._gap_buf
    K, A, N = eng.B, min(eng.A, agents_cap + 1), eng.N
    ag = eng.agents[:, :A].clone()
    ag[:, 1:, 8] = 1.0
    H = b["tau"].size(1)
    kw = dict(bin_seconds=meta["bin_seconds"], first_bin=meta["first_bin"])
    tau, env = b["tau"][:K], b["env"][:K]
    out = torch.empty((K, A), dtype=torch.float64, device=eng.device)
    scratch = torch.empty(max(ops.td_hindsight_bytes(eng.plan, K, A), 1), dtype=torch.uint8, device=eng.device)
    us = event_us(lambda: ops.td_hindsight(eng.plan, tau, env, ag, out=out, scratch=scratch, **kw), reps)
    n = K * (A - 1)
    finite = int(torch.isfinite(out[:, 1:]).sum())
    print(f"  tarl_td_hindsight: {us / 1e3:10.2f} ms for {n} searches (H = {H} bins, N = {N} roads, {finite} reach their "
          f"destination) = {us / n:8.3f} us per search", flush=True)
    d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
    d = d[(d >= 0) & (d < N)].contiguous()
    w = ops.fused_edge_travel_time(eng.plan, eng.fs)
    table = torch.empty((K, d.numel(), N), dtype=torch.int32, device=eng.device)
    _, need = ops.destination_trees_batched_bytes(eng.plan, K, d.numel())
    tscr = torch.empty(max(need, 1), dtype=torch.uint8, device=eng.device)
    tus = event_us(lambda: ops.destination_trees_batched(eng.plan, w, d, out=table, scratch=tscr), reps)
    trees = K * d.numel()
    print(f"  tarl_dest_trees_batched: {tus / 1e3:10.2f} ms for {trees} trees (distances, next hops and their [N] output rows) = "
          f"{tus / trees:8.3f} us per tree; a search costs x{(us / n) / (tus / trees):.2f} a tree", flush=True)
    ur = event_us(lambda: ops.td_road_times(ev.occ_acc["veh"], b["frames"], b["max"], b["ff"], b["cc"], out=(b["tau"], b["env"]),
                                            **kw), reps)
    print(f"  tarl_td_road_times: {ur:10.1f} us for K H N = {K} x {H} x {N}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--bin", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", default="1,8,64")
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    parent = parent_class(a.parent) if a.parent else None
    print(f"{SCENARIO} (BASELINE config 4), embedding head, MODE, {a.frames} frames, bins of {a.bin} s; wall clock around a device "
          f"synchronisation, median (min - max) of {a.reps} runs after one warm-up, the variants alternating", flush=True)
    r = runner_for(SCENARIO)
    for K in (int(v) for v in a.envs.split(",")):
        evs = {}
        if parent is not None:
            evs["parent"] = parent.from_policy_net(engine_for(r, K), r.policy_net)
        evs["gap off"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net)
        evs["gap on"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net, dynamic_gap=True, link_bin_seconds=a.bin)
        times, last = alternating(evs, a.frames, a.reps)
        off = times["parent" if parent is not None else "gap off"][0]
        for name, (med, lo, hi) in times.items():
            res = last[name]
            note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
            extra = f"  (+{med - off:.2f} ms per run, x{med / off:.4f})" if name == "gap on" else ""
            print(f"K = {K:5d}, {name + ':':9} {med:9.2f} ms ({lo:.2f} - {hi:.2f}) for {res.frames_run} frames{extra}{note}", flush=True)
        res = last["gap on"]
        if not res.domain_exit:
            m = res.dynamic_gap["meta"]
            same = all(getattr(last["gap off"], k) == getattr(res, k) for k in ("episode_return", "arrived"))
            print(f"  returns and arrivals equal with and without: {same}; {m['searches']} searches in the run, road times + searches "
                  f"+ reductions {m['wall_ms']:.2f} ms of it", flush=True)
            time_searches(evs["gap on"], m, a.agents, a.reps)
        del evs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
