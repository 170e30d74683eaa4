#!/usr/bin/env python3
"""Developer tool: what per-road occupancy costs in a vectorised evaluation at BASELINE config 4 (25 x 25 torus, 2 500 roads,
16 384 agents; embedding head, MODE, --frames frames), warm, median of --reps runs with min - max, per K in --envs:

  * VecEvaluator without occupancy and with it (``occupancy=True``: the fp32 ``counts`` output of every frame plus one
    ``tarl_occupancy_accumulate`` launch per block), in the same process, the runs of the two alternating;
  * with ``--parent FILE`` also the VecEvaluator of another evaluator.py — the parent commit's, e.g. from
    ``git show HEAD~1:tarl-simulator_amd/tarl_hip/evaluator.py > FILE`` — on the same library, alternating with the other
    two: the flag-off figure must not have moved;
  * ``tarl_occupancy_accumulate`` alone (HIP events) against its byte count: 4 F K N of ring read plus, per bin touched,
    the read-modify-write of veh and full (2 x 8 K N) and once that of peak (8 K N).

    python tools/time_occupancy.py [--frames 256] [--reps 5] [--envs 1,64,1024] [--parent FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_eval import COPY_TBPS, SCENARIO, engine_for, event_us, runner_for  # noqa: E402
from time_link_counts import alternating, parent_class  # noqa: E402
import torch  # noqa: E402

from tarl_hip import ops  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402


def time_kernel(ev, reps=20):
    K, N, F = ev.eng.B, ev.eng.N, ev.occupancy_block
    for H, bins, label in ((1, 3600, "one bin"), (2, F // 2 if F > 1 else 1, "two bins")):
        if H == 2 and F < 2:
            continue
        veh, full = (torch.zeros((K, H, N), dtype=torch.int32, device="cuda") for _ in range(2))
        peak = torch.zeros((K, 1, N), dtype=torch.int32, device="cuda")
        t0 = 21600 if H == 1 else 0
        frames = F if H == 1 else 2 * bins
        us = event_us(lambda: ops.occupancy_accumulate(ev.occ_ring, ev.occ_thr, veh, full, peak, t0=t0, timestep=1,
                                                       bin_seconds=bins, first_bin=t0 // bins, frames=frames), reps)
        nbytes = 4 * frames * K * N + H * 16 * K * N + 8 * K * N
        bound = nbytes / (COPY_TBPS * 1e12) * 1e6
        print(f"  tarl_occupancy_accumulate, K = {K}, F = {frames}, {label}: {us:8.1f} us   byte count {nbytes / 1e6:.1f} MB "
              f"(4 F K N of ring + {H} x 16 K N of veh and full + 8 K N of peak) = {bound:.1f} us at {COPY_TBPS} TB/s -> "
              f"{bound / us * 100:.1f} % of that rate", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", default="1,64,1024")
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    T = a.frames
    envs = [int(v) for v in a.envs.split(",")]
    r = runner_for(SCENARIO)
    parent = parent_class(a.parent) if a.parent else None
    print(f"{SCENARIO}, embedding head, MODE, {T} frames; wall clock around a device synchronisation, median (min - max) of "
          f"{a.reps} runs after one warm-up, the variants alternating", flush=True)
    for K in envs:
        evs = {}
        if parent is not None:
            evs["parent evaluator"] = parent.from_policy_net(engine_for(r, K), r.policy_net)
        evs["occupancy off"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net)
        evs["occupancy on"] = VecEvaluator.from_policy_net(engine_for(r, K), r.policy_net, occupancy=True)
        times, last = alternating(evs, T, a.reps)
        off = times["occupancy off"][0]
        for name, (med, lo, hi) in times.items():
            res = last[name]
            n = res.frames_run
            note = f" DOMAIN EXIT in frames {res.domain_exit_frames}" if res.domain_exit else ""
            extra = f"  (+{(med - off) / n * 1e3:.2f} us per frame, x{med / off:.3f})" if name == "occupancy on" else ""
            print(f"K = {K:5d}, {name + ':':18} {med:9.2f} ms ({lo:.2f} - {hi:.2f}) for {n} frames = {med / (n * K) * 1e3:9.3f} us "
                  f"per environment-frame{extra}{note}", flush=True)
        on = evs["occupancy on"]
        res = last["occupancy on"]
        same = all(getattr(last["occupancy off"], k) == getattr(res, k) for k in ("episode_return", "arrived")) \
            if not res.domain_exit else None
        ident = None if res.domain_exit else \
            [-x for x in res.episode_return] == [float(v) for v in res.occupancy["veh"].astype("int64").sum(axis=(1, 2))]
        print(f"K = {K:5d}, block F = {on.occupancy_block}, ring {4 * on.occ_ring.numel() / 2**20:.1f} MiB; per-environment returns "
              f"and arrivals equal with and without: {same}; sum(veh) == -return: {ident}", flush=True)
        time_kernel(on)
        del evs, on
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
