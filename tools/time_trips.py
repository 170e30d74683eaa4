#!/usr/bin/env python3
"""Developer tool: what the per-trip report costs in a vectorised evaluation (embedding head, MODE, --frames frames), warm,
median of --reps runs with min - max, per (scenario, K) of --cases — by default BASELINE config 4 (25 x 25 torus, 2 500
roads, 16 384 agents) at K = 1, 64 and 1 024 and config 5 (25 000 roads, 262 144 agents) at K = 64:

  * VecEvaluator without the report and with it (``trips=True`` with free-flow weights: the population check after the reset,
    the sort by departure bin, ``tarl_trip_agent_stats`` and ``tarl_trip_bin_stats`` after the episode and the copies of their
    results to the host), in the same process on engines of one seed, the runs of the two alternating;
  * the set-up the flag adds once per evaluator: the free-flow time of every agent (``ops.destination_trees`` over the
    distinct destinations);
  * each entry point alone (HIP events) against a device-to-device copy of the same K A 36 bytes of agent table (twice
    that with a baseline): the per-agent reduction without and with ``agents_b``, the per-bin reduction at the run's own
    bins and at 60 s bins; and ``trip_report`` on the host.

    python tools/time_trips.py [--frames 256] [--reps 5] [--cases synthetic-10000-16384:1,64,1024/synthetic-100000-262144:64@128]

A case is ``scenario:K,K,...[@frames]``; config 5 runs 128 frames by default, since under the untrained MODE policy it leaves the
domain between frames 192 and 256 and a run that left the domain has no trips to reduce."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_eval import engine_for, event_us, runner_for  # noqa: E402
from time_link_counts import alternating  # noqa: E402
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.evaluator import VecEvaluator, trip_free_flow_times, trip_report  # noqa: E402

CASES = "synthetic-10000-16384:1,64,1024/synthetic-100000-262144:64@128"


def free_flow_weights(r):
    g, h = r.env.simulator.graph, r.env.simulator.h
    return g.x[:, h.FREE_FLOW_TIME_TRAVEL][g.edge_index[1]]


def time_kernels(ev, res, reps=10):
    ag = ev.eng.agents
    K, A = ag.size(0), ag.size(1)
    other = ag.clone()
    nbytes = K * A * 36
    copy = event_us(lambda: other.copy_(ag), reps)
    print(f"  device copy of the K A 36 bytes = {nbytes / 1e6:.1f} MB: {copy:9.1f} us = {2 * nbytes / copy / 1e6:.2f} TB/s read + "
          f"written", flush=True)
    ff = ev.trip_ff
    for label, fn, tables in (("tarl_trip_agent_stats", lambda: ops.trip_agent_stats(ag, free_flow=ff), 1),
                              ("tarl_trip_agent_stats + agents_b", lambda: ops.trip_agent_stats(ag, other, free_flow=ff), 2)):
        us = event_us(fn, reps)
        print(f"  {label + ':':36} {us:9.1f} us = {tables * nbytes / us / 1e6:.2f} TB/s of table read, x{us / (tables * copy):.2f} the "
              f"copy of {tables} table(s)", flush=True)
    meta = res.trip_meta
    H = res.trip_bins["arr"].shape[1]
    for label, bins, first, nb in ((f"the run's bins ({meta['bin_seconds']} s, H = {H})", meta["bin_seconds"], meta["first_bin"], H),
                                   ("60 s bins, H = 62", 60, 359, 62)):
        order = ops.trip_departure_order(ag[0, :, 2], bin_seconds=bins, first_bin=first, num_bins=nb)
        us = event_us(lambda: ops.trip_bin_stats(ag, bin_seconds=bins, first_bin=first, num_bins=nb, free_flow=ff, order=order), reps)
        srt = event_us(lambda: ops.trip_departure_order(ag[0, :, 2], bin_seconds=bins, first_bin=first, num_bins=nb), reps)
        print(f"  tarl_trip_bin_stats, {label}: {us:9.1f} us (two kernels, the table read twice: x{us / (2 * copy):.2f} the copy "
              f"of 2 tables); the sort by departure bin {srt:.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=CASES)
    a = ap.parse_args()
    print(f"embedding head, MODE, {a.frames} frames unless a case says otherwise; wall clock around a device synchronisation, "
          f"median (min - max) of {a.reps} runs after one warm-up, the variants alternating", flush=True)
    for case in a.cases.split("/"):
        scenario, envs = case.split(":")
        envs, _, frames = envs.partition("@")
        T = int(frames) if frames else a.frames
        r = runner_for(scenario)
        w = free_flow_weights(r)
        for K in (int(v) for v in envs.split(",")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            on = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net, trips=True, trip_free_flow=w)
            torch.cuda.synchronize()
            t_on = (time.perf_counter() - t0) * 1e3
            ffs = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                trip_free_flow_times(on.eng, w)
                torch.cuda.synchronize()
                ffs.append((time.perf_counter() - t0) * 1e3)
            evs = {"trips off": VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net), "trips on": on}
            times, last = alternating(evs, T, a.reps)
            off = times["trips off"][0]
            for name, (med, lo, hi) in times.items():
                res = last[name]
                n = res.frames_run
                note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
                extra = f"  (+{med - off:.2f} ms per run, x{med / off:.4f})" if name == "trips on" else ""
                print(f"{scenario}, K = {K:5d}, {name + ':':10} {med:9.2f} ms ({lo:.2f} - {hi:.2f}) for {n} frames{extra}{note}",
                      flush=True)
            res = last["trips on"]
            print(f"  set-up with the flag {t_on:.1f} ms, of it the free-flow times (destination trees) {statistics.median(ffs):.1f} ms "
                  f"(median of 3, warm)", flush=True)
            if not res.domain_exit:
                same = all(getattr(last["trips off"], k) == getattr(res, k) for k in ("episode_return", "arrived"))
                t0 = time.perf_counter()
                rep = trip_report(res)
                t_rep = (time.perf_counter() - t0) * 1e3
                print(f"  returns and arrivals equal with and without: {same}; n_done.sum() == sum(arrived): "
                      f"{int(res.trips['n_done'].sum()) == sum(res.arrived)}; trip_report on the host {t_rep:.1f} ms for "
                      f"{len(rep['rows'])} rows", flush=True)
                time_kernels(on, res)
            del evs, on
            torch.cuda.empty_cache()
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
