#!/usr/bin/env python3
"""Developer tool for DESIGN 4.24: the trip reward (``--reward trip``). Everything printed also goes to --log (default
profiles/trip_reward_time.log).

  (a) the launch at BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents) for B in --envs environments, on the state
      that --frames live frames of the sampled embedding policy leave behind: tarl_fused_trip_reward with the departure window
      and with the window withdrawn (every waiting agent's departure tested beside its status), beside
      tarl_fused_hold_policy_actions and a device-to-device copy of the B * A status bytes on the same state. HIP events around
      --launches launches, warm, median of --reps with min - max, in one session; and the bytes each must move. Where the
      launch takes more than 4 x the copy (or with --split) also the split: the status pass with an empty walk (the cursor moved
      to the end for the measurement and put back), and the walk as the difference.
  (b) with --table: arrivals, episode return, trip return and ON_WAY - queued, mean +- se over --table-envs environments,
      without and with the first-hop rule: ``free_flow`` and ``dijkstra_hold`` on the 8 x 8 torus (128 agents bound anywhere,
      300 frames) and at config 4 (--table-frames frames), and the ``embedding_dijkstra`` MODE policy under the hold rule.
  (d) with --ppo: PPO after cloning on the torus case of (b): the goal_mlp head, --bc-iterations DAgger iterations (expert
      dijkstra, 16 environments, 512 samples, 4 epochs of minibatches of 64, lr 0.01), then --ppo-iterations PPO iterations of
      300 frames on --table-envs environments under the hold rule and the first-hop rule, once with reward "queue" and once with
      "trip", from the same cloned weights; the MODE evaluation of (c) before and after.
  (c) with --checkpoints A.pt,B.pt,...: each policy.pt of ``main.py --policy-head goal_mlp`` on --scenario evaluated in MODE
      under the hold rule and the first-hop rule over --table-envs environments and --ckpt-frames frames: arrivals, agents lost
      and both returns.

    python tools/time_trip_reward.py [--envs 64,4096] [--frames 60] [--reps 5] [--launches 50] [--split] [--table]
                                     [--table-envs 64] [--table-frames 256] [--ppo] [--checkpoints ...] [--scenario NAME]"""
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
from tarl_hip.evaluator import VecEvaluator  # noqa: E402

SCENARIO = "synthetic-10000-16384"
COPY_TBPS = 6.3
LOG = None


def say(text=""):
    print(text, flush=True)
    if LOG is not None:
        LOG.write(text + "\n")
        LOG.flush()


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


def time_launches(engine, envs, frames, reps, launches, split):
    say(f"(a) the launch at config 4 ({SCENARIO}) on the state after {frames} live frames of the sampled embedding policy; HIP "
        f"events around {launches} launches, median (min - max) of {reps} after one warm-up round")
    L = lib.load()
    for B in envs:
        eng = engine(B)
        eng.reset()
        fs = eng.fs
        eng.prepare_policy(torch.randn(eng.N, generator=torch.Generator().manual_seed(0)).to(eng.device), 1.0)
        for _ in range(frames):
            eng.frame_fused()
        fs.check_flags()
        t = float(eng.time) - float(eng.timestep)        # the clock of the frame that ran last
        N, A = eng.N, eng.A
        reward = torch.empty(B, dtype=torch.float32, device=eng.device)
        parts = torch.empty((B, 2), dtype=torch.int32, device=eng.device)
        held = torch.zeros(B, dtype=torch.int32, device=eng.device)
        status_copy = torch.empty_like(fs.a_status)
        s = lib.current_stream()
        f_trip = lambda: lib.check(L.tarl_fused_trip_reward(eng.plan.handle, fs.ref, B, fs.Nmax, A, t, reward.data_ptr(),  # noqa: E731
                                                            parts.data_ptr(), s))
        Ag, abs_ = ops._agents(eng.agents, B)
        f_hold = lambda: lib.check(L.tarl_fused_hold_policy_actions(eng.plan.handle, fs.ref, B, fs.Nmax, eng.agents.data_ptr(),  # noqa: E731
                                                                    Ag, abs_, None, held.data_ptr(), s))
        f_copy = lambda: status_copy.copy_(fs.a_status)                                                                      # noqa: E731
        f_trip()
        p = parts.cpu()
        on_way, ready = int(p[:, 0].sum()), int(p[:, 1].sum())
        lo = fs.cur_lo.long()
        due = (fs.a_dep_sorted <= t).sum(1)
        window = int((due - lo).clamp(min=0).sum())
        waiting = int((fs.a_status == 0).sum())
        empty = int(((fs.hdp[..., 0] & 127) == 0).sum())
        times = {}
        for name, fn in (("trip reward", f_trip), ("hold", f_hold), ("copy of the status bytes", f_copy)):
            fn()
            times[name] = [events_us(fn, launches) for _ in range(reps + 1)][1:]
        saved = fs.struct.a_order
        fs.struct.a_order = None
        f_trip()
        assert torch.equal(parts.cpu(), p), "the two paths disagree"
        times["trip reward, no window"] = [events_us(f_trip, launches) for _ in range(reps + 1)][1:]
        fs.struct.a_order = saved
        pairs = N * B
        b_status = A * B
        b_trip = b_status + 17 * window + 64 * 16 * B + 16 * B
        b_all = b_status + 4 * waiting + 16 * B
        b_hold = 8 * pairs + (pairs - empty) * 5
        say(f"B = {B}: A = {A} agents per environment, {b_status} status bytes; {on_way} agents on the way ({on_way / B:.1f} per "
            f"environment), {ready} ready ({ready / B:.2f}), {waiting} waiting; window entries from the cursor to the last due "
            f"one {window} ({window / B:.1f} per environment)")
        for name, nbytes, what in (
                ("trip reward", b_trip, "1 B per agent, 16 + 1 B per window entry, one 64-lane step of the window per "
                                        "environment, 4 B set + 12 B stored per environment"),
                ("trip reward, no window", b_all, "1 B per agent, 4 B per waiting agent, 4 B set + 12 B stored per environment"),
                ("hold", b_hold, "8 B of hdp per pair, 1 + 4 B per occupied row"),
                ("copy of the status bytes", 2 * b_status, "1 B read and 1 B written per agent")):
            say(f"  {name:26} {med(times[name])}   {nbytes / 1e6:8.2f} MB = {nbytes / (COPY_TBPS * 1e12) * 1e6:6.2f} us at "
                f"{COPY_TBPS} TB/s ({what})")
        m = {k: statistics.median(v) for k, v in times.items()}
        ratio = m["trip reward"] / m["copy of the status bytes"]
        say(f"  trip reward = {ratio:.2f} x the copy, {m['trip reward'] / m['hold']:.2f} x the hold launch; without the window "
            f"{m['trip reward, no window'] / m['copy of the status bytes']:.2f} x the copy")
        if split or ratio > 4.0:
            keep = fs.cur_lo.clone()
            fs.cur_lo.fill_(A)                             # an empty walk: the launch is the memset and the status pass
            f_trip()
            alone = [events_us(f_trip, launches) for _ in range(reps + 1)][1:]
            fs.cur_lo.copy_(keep)
            f_trip()
            assert torch.equal(parts.cpu(), p)
            say(f"  split: memset + status pass + an empty walk {med(alone)}; the walk of {window / B:.1f} entries per "
                f"environment is the difference, {m['trip reward'] - statistics.median(alone):.2f} us")
        del eng, fs
        torch.cuda.empty_cache()


def _mean_se(v):
    v = [float(x) for x in v]
    n = len(v)
    m = sum(v) / n
    return m, (math.sqrt(sum((x - m) ** 2 for x in v) / (n - 1) / n) if n > 1 else float("nan"))


def _row(name, tag, eng, res):
    x = eng.x
    lost = (eng.agents[:, :, 7].sum(1) - x[:, :, 3 * eng.Nmax + 1].sum(1)).tolist()
    (am, ase), (rm, rse), (lm, lse) = _mean_se(res.arrived), _mean_se(res.episode_return), _mean_se(lost)
    tm, tse = _mean_se(res.trip_return)
    on, ready = res.trip_parts_last.mean(axis=0)
    say(f"  {name:14} {tag:8} arrivals {am:10.2f} +- {ase:.2f}   return {rm:14.1f} +- {rse:.1f}   trip return {tm:14.1f} +- "
        f"{tse:.1f}   ON_WAY - queued {lm:8.2f} +- {lse:.2f}   owed after the last frame: on the way {on:.2f}, ready {ready:.2f}   "
        f"{res.computation_time_ms:.0f} ms")


def table(engine, K, frames4):
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    spread = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    torus = lambda: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, spread.cuda(),        # noqa: E731
                              congestion_constant=net.congestion_constant, num_envs=K, seed=3)
    cases = (("8 x 8 torus, 128 agents bound anywhere, 300 frames", torus, 300),
             (f"config 4 ({SCENARIO}), {frames4} frames", lambda: engine(K), frames4))
    say(f"(b) mean +- se over K = {K} environments (one engine seed per case, the same for every row); policy = the "
        f"embedding_dijkstra head in MODE (free-flow all-pairs prior, weight 1, embedding 0.01 N(0, 1)) under --policy-hold; "
        f"without / with = the first-hop rule of DESIGN 4.23")
    for label, make, T in cases:
        say(label)
        for name in ("free_flow", "dijkstra_hold", "policy + hold"):
            for route in (False, True):
                eng = make()
                kw = dict(route_departures=True) if route else {}
                if name == "policy + hold":
                    ff = eng._x[0, :, 3 * eng.Nmax + 2][eng.edge_index[1].to(eng.device)].contiguous()
                    dist = ops.all_pairs_shortest_paths(eng.plan, ff, want_next_hop=False, want_dist=True)[1][0]
                    emb = (0.01 * torch.randn(eng.N, generator=torch.Generator().manual_seed(5))).to(eng.device)
                    ev = VecEvaluator(eng, "embedding_dijkstra", emb=emb, prior_table=dist, prior_weight=1.0, policy_hold=True,
                                      trip_reward=True, **kw)
                else:
                    ev = VecEvaluator(eng, "dijkstra_hold", refresh_rate=0 if name == "free_flow" else 10, trip_reward=True, **kw)
                res = ev.run(T)
                if res.domain_exit:
                    say(f"  {name:14} {'with' if route else 'without':8} DOMAIN EXIT in frames {res.domain_exit_frames}")
                    continue
                _row(name, "with" if route else "without", eng, res)
                del ev, eng
                torch.cuda.empty_cache()


def checkpoints(paths, scenario, K, frames):
    from src.agents.base import destination_set
    from src.runner import Runner, RunnerArgs
    say(f"(c) goal_mlp checkpoints on {scenario}: MODE under --policy-hold and --route-departures, K = {K} environments, {frames} "
        f"frames, mean +- se")
    for path in paths:
        r = Runner(RunnerArgs(algo="mpnn", scenario=scenario, mode="eval", policy_head="goal_mlp", checkpoint=path))
        r.setup()
        eng = r._eval_engine(r.env.simulator, r.policy_net.agent_features, K)
        dests = destination_set(eng.agents, eng.N) if r.policy_net.resolve_prior_method() != "all_pairs" else None
        ev = VecEvaluator.from_policy_net(eng, r.policy_net, prior_dests=dests, policy_hold=True, route_departures=True,
                                          trip_reward=True)
        res = ev.run(frames)
        if res.domain_exit:
            say(f"  {path}: DOMAIN EXIT in frames {res.domain_exit_frames}")
            continue
        _row(os.path.basename(os.path.dirname(path)) or path, "", eng, res)


def ppo_after_cloning(K, bc_iterations, ppo_iterations):
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import synth
    from tarl_hip.imitation import BCTrainer
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(8, 8)
    N, Nmax, T = net.num_roads, net.Nmax, 300
    pop = synth.population(128, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    engine = lambda B, seed: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, Nmax, pop.cuda(),        # noqa: E731
                                       congestion_constant=net.congestion_constant, num_envs=B, seed=seed)
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]].cuda().contiguous()
    say(f"(d) PPO after cloning, 8 x 8 torus, 128 agents bound anywhere: goal_mlp head, {bc_iterations} DAgger iterations, then "
        f"{ppo_iterations} PPO iterations of {T} frames x {K} environments under policy_hold and route_departures; MODE evaluation "
        f"under both rules, K = {K}, {T} frames, mean +- se")
    for reward in ("queue", "trip"):
        torch.manual_seed(1)
        pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
        pol.prior_method = "all_pairs"
        pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * Nmax:]))
        val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
        l, gm = val.final_mlp, pol.goal_mlp
        tr = VecPPOTrainer(engine(K, 5), pol.nodes_embedding.weight,
                           [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias], rollout_steps=T,
                           extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")],
                           policy="goal_mlp", goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias],
                           prior_table=pol.dist_matrix, policy_hold=True, route_departures=True, reward=reward)
        bc = BCTrainer(tr, engine(16, 11), expert="dijkstra", driver="dagger", frames=T, samples=512, epochs=4, batch=64, lr=1e-2)
        for _ in range(bc_iterations):
            r = bc.iterate()
            say(f"    [bc {r['iteration']}] {r['driver']:6} loss {r['loss_first']:.4f} -> {r['loss_last']:.4f}  accuracy "
                f"{r['accuracy_before']:.3f} -> {r['accuracy_after']:.3f}  arrivals {r['arrivals']:.1f}")

        def evaluate(tag):
            eng = engine(K, 3)
            res = VecEvaluator.from_policy_net(eng, pol, policy_hold=True, route_departures=True, trip_reward=True).run(T)
            if res.domain_exit:
                say(f"  reward {reward}: {tag} DOMAIN EXIT in frames {res.domain_exit_frames}")
            else:
                _row(f"reward {reward}", tag, eng, res)
        evaluate("cloned")
        for it in range(ppo_iterations):
            tr.collect()
            out = tr.update().tolist()
            say(f"    [ppo {it}] mean collected reward per frame {float(tr.reward.mean()):10.3f}   objective {out[0]:.4f}  value loss "
                f"{out[1]:.4f}  kl {out[4]:.5f}")
        tr.check_flags()
        evaluate("+ ppo")
        del tr, bc, pol
        torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,4096")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--table-envs", type=int, default=64)
    ap.add_argument("--table-frames", type=int, default=256)
    ap.add_argument("--ppo", action="store_true")
    ap.add_argument("--bc-iterations", type=int, default=2)
    ap.add_argument("--ppo-iterations", type=int, default=10)
    ap.add_argument("--checkpoints", default="")
    ap.add_argument("--scenario", default="synthetic-256-128")
    ap.add_argument("--ckpt-frames", type=int, default=300)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "trip_reward_time.log"))
    a = ap.parse_args()
    LOG = open(a.log, "a")
    envs = [int(v) for v in a.envs.split(",") if v]
    if envs or a.table:
        engine = config4()
        if envs:
            time_launches(engine, envs, a.frames, a.reps, a.launches, a.split)
        if a.table:
            table(engine, a.table_envs, a.table_frames)
    if a.ppo:
        ppo_after_cloning(a.table_envs, a.bc_iterations, a.ppo_iterations)
    if a.checkpoints:
        checkpoints(a.checkpoints.split(","), a.scenario, a.table_envs, a.ckpt_frames)
    LOG.close()


if __name__ == "__main__":
    main()
