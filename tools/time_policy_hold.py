#!/usr/bin/env python3
"""Developer tool for DESIGN 4.20: the hold rule on a policy's action (``--policy-hold``).

  (a) the hold launch alone at BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents) for B in --envs environments, on
      the state and the action bytes that --frames frames of the sampled embedding policy leave behind: HIP events around
      --launches launches, warm, median of --reps with min - max. (The first launch of a batch turns the held rows' bytes into
      the raw code, which later launches skip: under 1 % of the rows.)
  (b) the ``edge_mlp_bf16`` collect loop (tarl_fused_rollout_policy, --collect-frames frames per call on --collect-envs
      environments, each call from a reset): per frame with the switch off and on at this commit and, with --parent-lib (a
      libtarl_hip.so built from the parent commit, same ABI), off at the parent — the three alternating in one process, median
      (min - max) of --reps. The kernels each variant launches per call are counted with the torch profiler where it is
      available: off must equal the parent, on must add one per frame.
  (c) with --table: arrivals and episode return, mean +- se over --table-envs environments, of the ``embedding_dijkstra`` MODE
      policy without and with the rule next to ``dijkstra_hold`` on the two 8 x 8 torus cases of DESIGN 4.13a and at config 4.

    python tools/time_policy_hold.py [--envs 1,64,1024,4096] [--frames 41] [--reps 5] [--launches 50] [--parent-lib PATH]
                                     [--collect-envs 4096] [--collect-frames 16] [--parts ab] [--table] [--table-envs 64]
                                     [--table-frames 256]"""
import argparse
import ctypes
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
    return engine, r.policy_net


def time_launch(engine, envs, frames, reps, launches):
    print(f"(a) hold launch at config 4 ({SCENARIO}) on the state and bytes after {frames} frames of the sampled embedding "
          f"policy; HIP events around {launches} launches, median (min - max) of {reps} after one warm-up round", flush=True)
    for B in envs:
        eng = engine(B)
        eng.reset()
        eng.prepare_policy(torch.randn(eng.N, generator=torch.Generator().manual_seed(0)).to(eng.device), 1.0)
        for _ in range(frames):
            eng.frame_fused()
        eng.fs.check_flags()
        fs = eng.fs
        held = torch.zeros(B, dtype=torch.int32, device=eng.device)
        occupied = int(((fs.hdp[..., 0] & 127) != 0).sum())
        L = lib.load()
        A, abs_ = ops._agents(eng.agents, B)
        args = (eng.plan.handle, fs.ref, B, fs.Nmax, eng.agents.data_ptr(), A, abs_, None, held.data_ptr())
        fn = lambda: lib.check(L.tarl_fused_hold_policy_actions(*args, lib.current_stream()))      # noqa: E731
        fn()
        first = int(held.sum())
        times = [events_us(fn, launches) for _ in range(reps + 1)][1:]
        pairs = eng.N * B
        nbytes = 8 * pairs + occupied * 5
        print(f"B = {B}: {pairs} pairs, {occupied} occupied ({100.0 * occupied / pairs:.1f} %), {first} held by the first launch; "
              f"{nbytes / 1e6:.2f} MB (8 B of hdp per pair, 1 + 4 B per occupied row) = "
              f"{nbytes / (COPY_TBPS * 1e12) * 1e6:.2f} us at {COPY_TBPS} TB/s\n  launch {med(times)}", flush=True)
        del eng, fs
        torch.cuda.empty_cache()


def _bind(cdll):
    for name, (res, argt) in lib.SIGNATURES.items():
        if hasattr(cdll, name):
            f = getattr(cdll, name)
            f.restype, f.argtypes = res, argt
    return cdll


def _kernels(fn):
    """Device kernels one call of ``fn`` launches (torch profiler), or None where the profiler gives no device activity."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower() and
                 "memset" not in e.name.lower()]      # device-side kernel records only, not the runtime's launch calls
        return len(names), sum(1 for n in names if "hold_policy" in n)
    except Exception as exc:  # noqa: BLE001
        print(f"  (kernel count not available: {exc})")
        return None


def time_collect(engine, policy_net, B, T, reps, parent):
    print(f"(b) edge_mlp_bf16 collect loop at config 4: tarl_fused_rollout_policy, {T} frames per call on B = {B} environments, "
          f"each call from a reset; per FRAME, median (min - max) of {reps} after one warm-up round, variants alternating", flush=True)
    eng = engine(B)
    m = policy_net.edge_mlp
    w = ops.EdgeMlpWeights(*(p.data for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias)))
    N, dev = eng.N, eng.device
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device=dev)
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device=dev)
    lp, rw = torch.zeros((T, B), device=dev), torch.zeros((T, B), device=dev)
    held = torch.zeros(B, dtype=torch.int32, device=dev)
    this = lib.load()

    def call():
        eng.rollout_policy(T, w, precision="bf16", temperature=1.0, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp,
                           reward=rw, counts=ct, check=False)

    def variant(cdll, on):
        def run(count=False):
            lib._lib = cdll
            try:
                eng.reset()
                if cdll is this:
                    ops.fused_set_policy_hold(eng.fs, on, held if on else None)
                if count:
                    return _kernels(call)
                return events_us(call, 1) / T
            finally:
                if cdll is this:
                    ops.fused_set_policy_hold(eng.fs, False)
                lib._lib = this
        return run
    forms = {"off": variant(this, False), "on": variant(this, True)}
    if parent is not None:
        forms["off, parent"] = variant(parent, False)
    times = {k: [] for k in forms}
    for rep in range(reps + 1):
        for k, fn in forms.items():
            us = fn()
            if rep:
                times[k].append(us)
    for k, v in times.items():
        print(f"  {k:12} {med(v)} per frame", flush=True)
    if parent is not None:
        lo, hi = min(times["off, parent"]), max(times["off, parent"])
        m_off = statistics.median(times["off"])
        print(f"  off (median {m_off:.2f}) {'lies inside' if lo <= m_off <= hi else 'lies OUTSIDE'} the parent's range "
              f"[{lo:.2f}, {hi:.2f}]")
    print(f"  on - off: {statistics.median(times['on']) - statistics.median(times['off']):.2f} us per frame; rows held per 'on' "
          f"call and environment: {int(held.sum()) / (reps + 1) / B:.2f}")
    counts = {k: fn(count=True) for k, fn in forms.items()}
    if all(c is not None for c in counts.values()):
        for k, (n, h) in counts.items():
            print(f"  kernels per call, {k:12} {n} ({h} of them k_fused_hold_policy_actions)")
        print(f"  off queues {'exactly the parent loop' if parent is None or counts['off'] == counts['off, parent'] else 'NOT the parent loop'}"
              f"{'' if parent is not None else ' (no parent library given)'}; on adds {counts['on'][0] - counts['off'][0]} launches "
              f"for {T} frames")
    del eng
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

    print(f"(c) arrivals and episode return, mean +- se over K = {K} environments (one engine seed per case, the same for every "
          f"row); policy = the embedding_dijkstra head in MODE (free-flow all-pairs prior, weight 1, embedding 0.01 N(0, 1))")
    for label, make, T in cases:
        print(label, flush=True)
        for name in ("policy", "policy + hold", "dijkstra_hold"):
            eng = make()
            if name == "dijkstra_hold":
                ev = VecEvaluator(eng, "dijkstra_hold")
            else:
                ff = eng._x[0, :, 3 * eng.Nmax + 2][eng.edge_index[1].to(eng.device)].contiguous()      # free-flow edge weights
                dist = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
                emb = (0.01 * torch.randn(eng.N, generator=torch.Generator().manual_seed(5))).to(eng.device)
                ev = VecEvaluator(eng, "embedding_dijkstra", emb=emb, prior_table=dist, prior_weight=1.0,
                                  policy_hold=name == "policy + hold")
            res = ev.run(T)
            if res.domain_exit:
                print(f"  {name:14} DOMAIN EXIT in frames {res.domain_exit_frames}", flush=True)
                continue
            (am, ase), (rm, rse) = _mean_se(res.arrived), _mean_se(res.episode_return)
            extra = f"   held {_mean_se([int(v) for v in res.held])[0]:.1f}" if res.held is not None else ""
            print(f"  {name:14} arrivals {am:10.2f} +- {ase:.2f}   return {rm:14.1f} +- {rse:.1f}   on the way at the end "
                  f"{_mean_se(res.on_way)[0]:.1f}{extra}   {res.computation_time_ms:.0f} ms", flush=True)
            del ev, eng
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,64,1024,4096")
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--collect-envs", type=int, default=4096)
    ap.add_argument("--collect-frames", type=int, default=16)
    ap.add_argument("--parts", default="ab", help="which of (a) the launch and (b) the collect loop to run")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--table-frames", type=int, default=256)
    a = ap.parse_args()
    parent = None
    if a.parent_lib:
        parent = _bind(ctypes.CDLL(a.parent_lib))
        assert parent.tarl_abi_version() == lib.load().tarl_abi_version(), "the parent library has another ABI"
        assert not hasattr(parent, "tarl_fused_hold_policy_actions"), "that library already has the hold launch: not the parent"
    engine, policy_net = config4()
    if "a" in a.parts:
        time_launch(engine, [int(v) for v in a.envs.split(",")], a.frames, a.reps, a.launches)
    if "b" in a.parts:
        time_collect(engine, policy_net, a.collect_envs, a.collect_frames, a.reps, parent)
    if a.table:
        table(engine, a.table_envs, a.table_frames)


if __name__ == "__main__":
    main()
