#!/usr/bin/env python3
"""Developer tool for DESIGN 4.26: per-decision PPO credit (``--credit decision``). Everything printed also goes to --log
(default profiles/decision_credit_time.log).

  (a) cost, with HIP events, median of --reps with min - max: tarl_fused_head_rows for the kept pairs of one frame; one
      ``collect()`` with and without the capture (variants alternating, per frame); and the stages of one minibatch step
      (``decision_ppo`` beside ``graphdist_bwd`` and ``actor_logits_bwd`` at the same M), on the 8 x 8 torus and on the geometry
      of BASELINE config 4 (25 x 25 torus, 2 500 roads, 16 384 agents), goal_mlp head, --envs environments.
  (b) with --ppo: the experiment of DESIGN 4.24 part 3 again. 8 x 8 torus, 128 agents bound anywhere, the goal_mlp head, two
      DAgger iterations (expert dijkstra, 16 environments, 512 samples, 4 epochs of minibatches of 64, lr 0.01), then
      --ppo-iterations PPO iterations of 300 frames x --envs environments under policy_hold and route_departures, from the
      same cloned weights, credit "joint" against "decision", per schedule of --schedules (epochs:minibatch:lr); MODE
      evaluation under both rules over --envs environments before and after.
  --credit-baseline learned: the rows of the learned per-decision critic instead. (a) then times the stages of
      a step of VecPPOTrainer(credit_baseline="learned") — ``decision_critic`` beside ``decision_ppo`` and
      ``actor_logits_bwd`` — and the critic's forward over all kept rows, once per update; (b) runs the same experiment with
      credit "decision" and the learned baseline (rows "learned", with the critic's explained variance per iteration).

  --credit-scope due / --credit-horizon bootstrap: the rows of the narrowed credit instead. (a) then times
      tarl_fused_head_rows_due beside tarl_fused_head_rows, tarl_fused_agent_roads (once per segment) and one ``collect()``
      with the flags against one without; (b) runs the same experiment with credit "decision" and the flags given (rows "due",
      "bootstrap", "due+boot"; with --credit-baseline learned "due+boot+L"), with the headed and bootstrapped counts per
      iteration.

    python tools/time_decision_credit.py [--envs 64] [--reps 5] [--ppo] [--ppo-iterations 10] [--schedules 1:32:1e-3,...]
                                         [--credit-baseline {free_flow,learned}] [--credit-scope {headed,due}]
                                         [--credit-horizon {charge,bootstrap}]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from tarl_hip import ops, synth  # noqa: E402
from tarl_hip.engine import EPISODE_START, SimEngine  # noqa: E402
from tarl_hip.evaluator import VecEvaluator  # noqa: E402
from tarl_hip.trainer import StageTimer, VecPPOTrainer  # noqa: E402

LOG = None


def say(text=""):
    print(text, flush=True)
    if LOG is not None:
        LOG.write(text + "\n")
        LOG.flush()


def med(v, unit="us"):
    return f"{statistics.median(v):10.2f} {unit} ({min(v):.2f} - {max(v):.2f})"


def _mean_se(v):
    v = [float(x) for x in v]
    n = len(v)
    m = sum(v) / n
    return m, (math.sqrt(sum((x - m) ** 2 for x in v) / (n - 1) / n) if n > 1 else float("nan"))


def trainer(net, pop, B, T, *, credit, epochs=1, M=32, lr=1e-3, seed=5, reward="trip", rules=True, baseline="free_flow",
            scope="headed", horizon="charge"):
    """``baseline`` "learned" (with ``credit`` "decision"): the learned per-decision critic of DESIGN 4.27; ``scope`` "due" /
    ``horizon`` "bootstrap": the narrowed credit of DESIGN 4.28."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    N, Nmax = net.num_roads, net.Nmax
    eng = SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, Nmax, pop.cuda(), congestion_constant=net.congestion_constant,
                    num_envs=B, seed=seed)
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]].cuda().contiguous()
    torch.manual_seed(1)
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.prior_method = "all_pairs"
    pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * Nmax:]))
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l, gm = val.final_mlp, pol.goal_mlp
    critic = ops.decision_critic_init("cuda", seed) if baseline == "learned" else []
    kw = dict(credit_baseline="learned", decision_critic_params=critic) if critic else {}
    if scope != "headed":
        kw["credit_scope"] = scope
    if horizon != "charge":
        kw["credit_horizon"] = horizon
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias],
                       rollout_steps=T, num_epochs=epochs, sub_batch_size=M, lr=lr,
                       extra_params=[p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")] + critic,
                       policy="goal_mlp", goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias],
                       prior_table=pol.dist_matrix, policy_hold=rules, route_departures=rules, reward=reward,
                       credit=credit, **kw)
    return tr, pol


def critic_cost(label, net, pop, B, T, M, reps):
    """The stages of a step under the learned baseline, and the critic's forward over all kept rows."""
    say(f"{label}: N = {net.num_roads}, B = {B}, T = {T} frames, minibatch M = {M}, goal_mlp head, credit_baseline learned")
    tr = trainer(net, pop, B, T, credit="decision", baseline="learned", M=M, rules=False, reward="queue")[0]
    stages, fwd, live = {}, [], []
    value = adv_dec = None
    for rep in range(reps + 1):                 # one warm-up round
        tr.collect()
        tr.stage = StageTimer()
        tr.update()
        dist, slot = tr._decision_dist
        if value is None:
            value, adv_dec = torch.empty_like(tr.adv_raw), torch.empty_like(tr.adv_raw)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.decision_critic_forward(tr.eng.plan, tr.obs_mb, tr.head_keep, tr.frames_left, dist, slot, tr._dcritic(),
                                    tr.adv_raw, timestep=tr.eng.timestep, delay_scale=tr.decision_delay_scale,
                                    value=value, adv_out=adv_dec)          # buffers of its own: the trainer's stay as they are
        b.record()
        torch.cuda.synchronize()
        if rep:
            fwd.append(a.elapsed_time(b) * 1e3)
            live.append(int((tr.head_keep > 0).sum()))
            for k, (v, n) in tr.stage.ms().items():
                stages.setdefault(k, []).append(v / n * 1e3)
    for k in ("actor_logits_bwd", "decision_ppo", "decision_critic"):
        say(f"  step stage {k:18} {med(stages[k])}")
    say(f"  critic forward over all {tr.head_keep.size(0)} kept rows (once per update) {med(fwd)}; live decisions "
        f"{min(live)} - {max(live)} of {tr.head_keep.numel()}")
    rows = min(M, tr.head_keep.size(0))         # the loss launch of one minibatch on its own, 50 launches per sample
    head = tr.head_keep[:rows]
    n_live = (head > 0).sum(dtype=torch.int32).reshape(1)
    grads = torch.zeros(ops.DECISION_CRITIC_PARAMS, device="cuda")
    scratch = torch.empty((ops.decision_critic_scratch_bytes(tr.eng.plan, rows) + 7) // 8, dtype=torch.float64, device="cuda")
    v = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            ops.decision_critic_loss(tr.eng.plan, tr.obs_mb[:rows], head, tr.frames_left[:rows], dist, slot, tr._dcritic(),
                                     tr.adv_raw[:rows], n_live, timestep=tr.eng.timestep, grads=grads, scratch=scratch)
        b.record()
        torch.cuda.synchronize()
        if rep:
            v.append(a.elapsed_time(b) / 50 * 1e3)
    say(f"  tarl_decision_critic_loss, {rows} rows, {int(n_live)} live decisions: {med(v)} per call (50 calls per sample)")
    tr.check_flags()


def cost(label, net, pop, B, T, M, reps):
    say(f"{label}: N = {net.num_roads}, B = {B}, T = {T} frames, minibatch M = {M}, goal_mlp head")
    trs = {c: trainer(net, pop, B, T, credit=c, M=M, rules=False, reward="queue")[0] for c in ("joint", "decision")}
    times = {c: [] for c in trs}
    stages = {}
    for rep in range(reps + 1):                 # one warm-up round, variants alternating
        for c, tr in trs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.collect()
            b.record()
            tr.stage = StageTimer()
            tr.update()
            ms = tr.stage.ms()
            if rep:
                times[c].append(a.elapsed_time(b) / T * 1e3)
                for k, (v, n) in ms.items():
                    stages.setdefault((c, k), []).append(v / n * 1e3)
    for c in trs:
        say(f"  collect, credit {c:9} {med(times[c])} per frame")
    say(f"  capture = decision - joint: {statistics.median(times['decision']) - statistics.median(times['joint']):.2f} us per "
        f"frame ({M} kept pairs over {T} frames: {M / T:.2f} head-row launches per frame)")
    for k in ("graphdist_bwd", "actor_logits_bwd", "decision_ppo", "ppo_loss"):
        for c in trs:
            if (c, k) in stages:
                say(f"  step stage {k:18} credit {c:9} {med(stages[(c, k)])}")
    tr = trs["decision"]
    eng = tr.eng
    n = max(1, M // T)
    env = torch.zeros(n, dtype=torch.int32, device="cuda")
    slot = torch.arange(n, dtype=torch.int32, device="cuda")
    v = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            ops.fused_head_rows(eng.plan, eng.fs, env, slot, tr.head_keep)
        b.record()
        torch.cuda.synchronize()
        if rep:
            v.append(a.elapsed_time(b) / 50 * 1e3)
    say(f"  tarl_fused_head_rows, {n} pair(s): {med(v)} per launch (50 launches per sample)")
    tr.check_flags()


def _per_call(fn, reps, calls=50):
    v = []
    for r in range(reps + 1):                   # one warm-up round
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            v.append(a.elapsed_time(b) / calls * 1e3)
    return v


def scope_cost(label, net, pop, B, T, M, reps, scope, horizon):
    """The launches of DESIGN 4.28 beside the one they replace, and a ``collect()`` frame with and without the flags."""
    say(f"{label}: N = {net.num_roads}, B = {B}, T = {T} frames, minibatch M = {M}, goal_mlp head, credit_scope {scope}, "
        f"credit_horizon {horizon}")
    trs = {"decision": trainer(net, pop, B, T, credit="decision", M=M, rules=False, reward="queue")[0],
           "narrowed": trainer(net, pop, B, T, credit="decision", M=M, rules=False, reward="queue", scope=scope,
                               horizon=horizon)[0]}
    times = {c: [] for c in trs}
    for r in range(reps + 1):                   # one warm-up round, variants alternating
        for c, tr in trs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.collect()
            b.record()
            torch.cuda.synchronize()
            if r:
                times[c].append(a.elapsed_time(b) / T * 1e3)
    for c in trs:
        say(f"  collect, {c:9} {med(times[c])} per frame")
    tr = trs["narrowed"]
    eng = tr.eng
    n = max(1, M // T)
    env = torch.zeros(n, dtype=torch.int32, device="cuda")
    slot = torch.arange(n, dtype=torch.int32, device="cuda")
    hk = torch.empty_like(tr.head_keep)
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    clock = float(eng.time)
    v = _per_call(lambda: ops.fused_head_rows(eng.plan, eng.fs, env, slot, hk), reps)
    say(f"  tarl_fused_head_rows,     {n} pair(s): {med(v)} per launch (50 launches per sample)")
    v = _per_call(lambda: ops.fused_head_rows(eng.plan, eng.fs, env, slot, hk, t=clock, counts=counts), reps)
    say(f"  tarl_fused_head_rows_due, {n} pair(s): {med(v)} per launch (50 launches per sample)")
    road = torch.empty((eng.B, eng.A), dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    v = _per_call(lambda: ops.fused_agent_roads(eng.plan, eng.fs, eng.Nmax, out=road, bad=bad), reps)
    say(f"  tarl_fused_agent_roads (fill + kernel, once per segment), {int((road >= 0).sum())} of {road.numel()} agents queued: "
        f"{med(v)} per call (50 calls per sample)")
    tr.check_flags()


VARIANTS = {"joint": {}, "decision": {}, "learned": dict(baseline="learned"), "due": dict(scope="due"),
            "bootstrap": dict(horizon="bootstrap"), "due+boot": dict(scope="due", horizon="bootstrap"),
            "due+boot+L": dict(scope="due", horizon="bootstrap", baseline="learned"),
            "due+L": dict(scope="due", baseline="learned"), "bootstrap+L": dict(horizon="bootstrap", baseline="learned")}


def ppo_after_cloning(K, bc_iterations, ppo_iterations, schedules, credits=("joint", "decision")):
    from tarl_hip.imitation import BCTrainer
    net = synth.torus_network(8, 8)
    T = 300
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    engine = lambda B, seed: SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),        # noqa: E731
                                       congestion_constant=net.congestion_constant, num_envs=B, seed=seed)
    say(f"(b) PPO after cloning, 8 x 8 torus, 128 agents bound anywhere: goal_mlp head, {bc_iterations} DAgger iterations, then "
        f"{ppo_iterations} PPO iterations of {T} frames x {K} environments under policy_hold and route_departures (reward trip); "
        f"MODE evaluation under both rules, K = {K}, {T} frames, mean +- se")
    for epochs, M, lr in schedules:
        say(f"schedule: {epochs} epoch(s) of one minibatch of {M} frames per iteration, lr {lr:g}")
        for credit in credits:
            tr, pol = trainer(net, pop, K, T, credit="joint" if credit == "joint" else "decision", epochs=epochs, M=M, lr=lr,
                              **VARIANTS[credit])
            bc = BCTrainer(tr, engine(16, 11), expert="dijkstra", driver="dagger", frames=T, samples=512, epochs=4, batch=64,
                           lr=1e-2)
            acc = [bc.iterate()["accuracy_after"] for _ in range(bc_iterations)]

            def evaluate(tag):
                eng = engine(K, 3)
                res = VecEvaluator.from_policy_net(eng, pol, policy_hold=True, route_departures=True, trip_reward=True).run(T)
                if res.domain_exit:
                    say(f"  credit {credit:9} {tag:8} DOMAIN EXIT in frames {res.domain_exit_frames}")
                    return
                lost = (eng.agents[:, :, 7].sum(1) - eng.x[:, :, 3 * eng.Nmax + 1].sum(1)).tolist()
                (am, ase), (lm, _), (tm, tse) = _mean_se(res.arrived), _mean_se(lost), _mean_se(res.trip_return)
                say(f"  credit {credit:9} {tag:8} arrivals {am:7.2f} +- {ase:.2f}   agents lost {lm:5.2f}   trip return {tm:10.1f} +- "
                    f"{tse:.1f}")
            say(f"  credit {credit:9} cloned: accuracy on the store {' -> '.join(f'{a:.3f}' for a in acc)}")
            evaluate("cloned")
            for it in range(ppo_iterations):
                tr.collect()
                on_way = float(tr.eng.agents[:, :, 7].sum()) / K
                queued = float(tr.eng.x[:, :, 3 * net.Nmax + 1].sum()) / K
                out = tr.update().tolist()
                line = f"    [ppo {it}] collected reward per frame {float(tr.reward.mean()):9.3f}  joint kl {out[4]:.5f}"
                d = {}                       # the joint row has no per-decision figures
                if credit != "joint":
                    d = {k: float(v) for k, v in tr.last["decision"].items() if not isinstance(v, str)}
                    line += (f"  decisions {int(d['decisions'])}  delay {d['delay_frames']:.2f} frames  truncated "
                             f"{d['truncated']:.3f}  objective {d['objective']:.4f}  clip {d['clip_fraction']:.3f}  kl {d['kl']:.5f}")
                if "decisions_headed" in d:
                    line += f"  headed {int(d['decisions_headed'])}"
                if "bootstrapped" in d:      # ... and who is left when the segment ends: ON_WAY agents against queued ones
                    line += (f"  bootstrapped {d['bootstrapped']:.3f}  on the way {on_way:.1f} of which queued {queued:.2f} per "
                             f"environment")
                if "critic_loss" in d:
                    line += (f"  critic loss {d['critic_loss']:.4f}  explained variance {d['explained_variance']:.3f}  value mean "
                             f"{d['value_mean']:.3f}")
                say(line)
            tr.check_flags()
            evaluate("+ ppo")
            del tr, bc, pol
            torch.cuda.empty_cache()


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--ppo", action="store_true")
    ap.add_argument("--bc-iterations", type=int, default=2)
    ap.add_argument("--ppo-iterations", type=int, default=10)
    ap.add_argument("--schedules", default="1:32:1e-3,4:256:1e-3,8:512:3e-3")
    ap.add_argument("--credit-baseline", choices=("free_flow", "learned"), default="free_flow")
    ap.add_argument("--credit-scope", choices=("headed", "due"), default="headed")
    ap.add_argument("--credit-horizon", choices=("charge", "bootstrap"), default="charge")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "decision_credit_time.log"))
    a = ap.parse_args()
    LOG = open(a.log, "a")
    shown, skip = [], False       # the command line without where the log goes
    for arg in sys.argv[1:]:
        if skip or arg == "--log":
            skip = not skip
            continue
        if not arg.startswith("--log="):
            shown.append(arg)
    learned = a.credit_baseline == "learned"
    narrowed = a.credit_scope != "headed" or a.credit_horizon != "charge"
    say(f"# tools/time_decision_credit.py {' '.join(shown)}   (MI355X; DESIGN "
        f"{'4.28' if narrowed else '4.27' if learned else '4.26'})")
    cost_fn = critic_cost if learned else cost
    if narrowed:
        cost_fn = lambda *args: scope_cost(*args, a.credit_scope, a.credit_horizon)      # noqa: E731
    if not a.no_cost:
        say("(a) cost: HIP events, median (min - max) of the repetitions after one warm-up round")
        net = synth.torus_network(8, 8)
        pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
        cost_fn("8 x 8 torus", net, pop, a.envs, 64, 32, a.reps)
        cost_fn("8 x 8 torus", net, pop, a.envs, 64, 512, a.reps)
        net = synth.torus_network(25, 25)
        pop = synth.population(16384, net.num_roads, seed=0)
        cost_fn("config-4 geometry (25 x 25 torus, 16 384 agents)", net, pop, a.envs, 32, 32, a.reps)
    if a.ppo:
        sched = [(int(e), int(m), float(lr)) for e, m, lr in (s.split(":") for s in a.schedules.split(","))]
        row = "+".join(n for n, on in (("due", a.credit_scope == "due"), ("boot", a.credit_horizon == "bootstrap")) if on)
        row = {"due": "due", "boot": "bootstrap"}.get(row, row) + ("+L" if learned else "")
        ppo_after_cloning(a.envs, a.bc_iterations, a.ppo_iterations, sched,
                          (row,) if narrowed else ("learned",) if learned else ("joint", "decision"))
    LOG.close()


if __name__ == "__main__":
    main()
