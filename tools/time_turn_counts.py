#!/usr/bin/env python3
"""Developer tool: what the per-turn movement counts cost in a vectorised evaluation at BASELINE config 4 (25 x 25 torus, 2 500
roads, 10 000 route edges, 16 384 agents; embedding head, MODE, --frames frames), warm, median of --reps runs with min - max,
per K in --envs:

  * VecEvaluator without turn counts and with them (``turns=True``: the ``popped`` and fp32 ``counts`` outputs of every frame,
    a copy of the SELECTED_ROAD bytes after it, and one ``tarl_turn_counts_accumulate`` launch plus the carry copy per
    block), in the same process, the runs of the two alternating;
  * ``tarl_turn_counts_accumulate`` alone (HIP events) on the rings the last run left behind, against a device copy of the
    same ring bytes (popped + SELECTED_ROAD + counts = 6 F K N bytes, ``Tensor.copy_`` of the three rings) in the same session.

    python tools/time_turn_counts.py [--frames 256] [--reps 5] [--envs 1,64,1024]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_eval import SCENARIO, engine_for, event_us, runner_for  # noqa: E402
from time_link_counts import alternating  # noqa: E402
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402


def time_kernel(ev, reps=20):
    eng = ev.eng
    K, N, E, F = eng.B, eng.N, eng.E, ev.turn_block
    rings = (ev.turn_popped, ev.turn_sel, ev.turn_ring)
    twins = [torch.empty_like(r) for r in rings]
    pops = float((ev.turn_popped & 1).float().mean())

    def copy():
        for dst, src in zip(twins, rings):
            dst.copy_(src)

    copy_us = event_us(copy, reps)
    nbytes = sum(r.numel() * r.element_size() for r in rings)
    for H, bins, label in ((1, 3600, "one bin"), (2, F // 2 if F > 1 else 1, "two bins")):
        if H == 2 and F < 2:
            continue
        turns = torch.zeros((K, H, E), dtype=torch.int32, device="cuda")
        lost = torch.zeros((K, H, N), dtype=torch.int32, device="cuda")
        unres = torch.zeros(K, dtype=torch.int32, device="cuda")
        t0 = 21600 if H == 1 else 0
        frames = F if H == 1 else 2 * bins
        us = event_us(lambda: ops.turn_counts_accumulate(eng.plan, *rings, turns, lost, unres, prev_counts=ev.turn_prev, t0=t0,
                                                         timestep=1, bin_seconds=bins, first_bin=t0 // bins, frames=frames), reps)
        print(f"  tarl_turn_counts_accumulate, K = {K}, F = {frames}, {label}: {us:8.1f} us; device copy of the three rings "
              f"({nbytes / 1e6:.1f} MB read + written, F = {F}): {copy_us:8.1f} us; popped bits set: {100.0 * pops:.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", default="1,64,1024")
    a = ap.parse_args()
    T = a.frames
    r = runner_for(SCENARIO)
    print(f"{SCENARIO}, embedding head, MODE, {T} frames; wall clock around a device synchronisation, median (min - max) of "
          f"{a.reps} runs after one warm-up, the variants alternating", flush=True)
    for K in [int(v) for v in a.envs.split(",")]:
        evs = {"turns off": VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net),
               "turns on": VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net, turns=True)}
        times, last = alternating(evs, T, a.reps)
        off = times["turns off"][0]
        for name, (med, lo, hi) in times.items():
            res = last[name]
            n = res.frames_run
            note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
            extra = f"  (+{(med - off) / n * 1e3:.2f} us per frame, x{med / off:.3f})" if name == "turns on" else ""
            print(f"K = {K:5d}, {name + ':':18} {med:9.2f} ms ({lo:.2f} - {hi:.2f}) for {n} frames = {med / (n * K) * 1e3:9.3f} us "
                  f"per environment-frame{extra}{note}", flush=True)
        on, res = evs["turns on"], last["turns on"]
        same = all(getattr(last["turns off"], k) == getattr(res, k) for k in ("episode_return", "arrived")) \
            if not res.domain_exit else None
        moved = None if res.domain_exit else [int(x) for x in res.turn_counts.astype("int64").sum(axis=(1, 2))][:4]
        lost = None if res.domain_exit else [int(x) for x in res.turn_lost.astype("int64").sum(axis=(1, 2))][:4]
        ring = sum(x.numel() * x.element_size() for x in (on.turn_popped, on.turn_sel, on.turn_ring))
        print(f"K = {K:5d}, block F = {on.turn_block}, rings {ring / 2**20:.1f} MiB; per-environment returns and arrivals equal with "
              f"and without: {same}; movements of the first environments {moved}, lost {lost}", flush=True)
        time_kernel(on)
        del evs, on
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
