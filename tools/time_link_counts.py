#!/usr/bin/env python3
"""Developer tool: what per-road link counts cost in a vectorised evaluation at BASELINE config 4 (25 x 25 torus, 2 500
roads, 16 384 agents; embedding head, MODE, --frames frames), warm, median of --reps runs with min - max, per K in --envs:

  * VecEvaluator without link counts and with them (``link_counts=True``: the two mask outputs of every frame plus one
    ``tarl_link_counts_accumulate`` launch per block), in the same process, the runs of the two alternating;
  * with ``--parent FILE`` also the VecEvaluator of another evaluator.py — the parent commit's, e.g. from
    ``git show HEAD~1:tarl-simulator_amd/tarl_hip/evaluator.py > FILE`` — on the same library, alternating with the other
    two: the flag-off figure must not have moved;
  * ``tarl_link_counts_accumulate`` and ``tarl_link_count_stats`` alone (HIP events) against their byte counts.

    python tools/time_link_counts.py [--frames 256] [--reps 5] [--envs 1,64,1024] [--parent FILE] [--only evaluator]

``--only evaluator`` runs one warm-up and one evaluation with link counts at the largest K: the run to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel split (profiles/link_counts_kernel_stats.txt)."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_eval import COPY_TBPS, SCENARIO, engine_for, event_us, runner_for  # noqa: E402
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402


def parent_class(path):
    """``VecEvaluator`` of another evaluator.py, loaded as a sibling module of tarl_hip.evaluator (same library)."""
    spec = importlib.util.spec_from_file_location("tarl_hip.evaluator_parent", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.VecEvaluator


def alternating(evs, T, reps):
    """One warm-up each, then ``reps`` rounds in which every evaluator runs once: {name: (median, min, max) ms}, last result."""
    out = {k: [] for k in evs}
    last = {}
    for i in range(reps + 1):
        for name, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = ev.run(T)
            torch.cuda.synchronize()
            if i:
                out[name].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}, last


def time_kernels(ev, reps=20):
    K, N, F = ev.eng.B, ev.eng.N, ev.link_block
    acc = torch.zeros((K, 1, N), dtype=torch.int32, device="cuda")
    us = event_us(lambda: ops.link_counts_accumulate(ev.link_popped, ev.link_withdrawn, acc, t0=21600, timestep=1,
                                                     bin_seconds=3600), reps)      # (a bin's first frame: F <= 127 stay inside it)
    nbytes = 2 * F * K * N + 8 * K * N
    bound = nbytes / (COPY_TBPS * 1e12) * 1e6
    print(f"  tarl_link_counts_accumulate, K = {K}, F = {F}: {us:8.1f} us   byte count {nbytes / 1e6:.1f} MB (2 F K N mask bytes "
          f"+ 8 K N of counts) = {bound:.1f} us at {COPY_TBPS} TB/s -> {bound / us * 100:.1f} % of that rate")
    us = event_us(lambda: ops.link_count_stats(acc), reps)
    print(f"  tarl_link_count_stats, K = {K}, H = 1: {us:8.1f} us   ({8 * K * N / 1e6:.1f} MB read: both rows walk the counts)",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", default="1,64,1024")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--only", choices=("evaluator",), default=None)
    a = ap.parse_args()
    T = a.frames
    envs = [int(v) for v in a.envs.split(",")]
    r = runner_for(SCENARIO)
    if a.only == "evaluator":
        ev = VecEvaluator.from_policy_net(engine_for(r, max(envs)), r.policy_net, link_counts=True)
        ev.run(T)
        res = ev.run(T)
        print(f"VecEvaluator MODE + link counts K = {max(envs)}: {res.frames_run} frames, domain_exit {res.domain_exit}, "
              f"{res.computation_time_ms:.1f} ms, {int(res.link_counts.sum())} events counted")
        return
    parent = parent_class(a.parent) if a.parent else None
    print(f"{SCENARIO}, embedding head, MODE, {T} frames; wall clock around a device synchronisation, median (min - max) of "
          f"{a.reps} runs after one warm-up, the variants alternating", flush=True)
    for K in envs:
        evs = {}
        if parent is not None:
            evs["parent evaluator"] = parent.from_policy_net(engine_for(r, K), r.policy_net)
        evs["link counts off"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net)
        evs["link counts on"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net, link_counts=True)
        times, last = alternating(evs, T, a.reps)
        off = times["link counts off"][0]
        for name, (med, lo, hi) in times.items():
            res = last[name]
            n = res.frames_run
            note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
            extra = f"  (+{(med - off) / n * 1e3:.2f} us per frame, x{med / off:.3f})" if name == "link counts on" else ""
            print(f"K = {K:5d}, {name + ':':18} {med:9.2f} ms ({lo:.2f} - {hi:.2f}) for {n} frames = {med / (n * K) * 1e3:9.3f} us "
                  f"per environment-frame{extra}{note}", flush=True)
        on = evs["link counts on"]
        same = all(getattr(last["link counts off"], k) == getattr(last["link counts on"], k)
                   for k in ("episode_return", "arrived")) if not last["link counts on"].domain_exit else None
        print(f"K = {K:5d}, block F = {on.link_block}, rings {2 * on.link_popped.numel() / 2**20:.1f} MiB; per-environment returns "
              f"and arrivals equal with and without: {same}", flush=True)
        time_kernels(on)
        del evs, on
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
