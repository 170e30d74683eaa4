"""Timings of the goal-conditioned policy head (policy_head "goal_mlp", csrc/goal_mlp.hip) at BASELINE config 4 (25 x 25
torus, N = 2 500 roads, E = 10 000, 16 384 agents), median and min - max of five, HIP events on the launch stream:

  1. the fused logits launch (tarl_fused_goal_mlp_logits) at B in {64, 4 096} after 20 live frames, beside
     tarl_fused_prior_logits on the same state and beside its byte bound (packed word + head's destination per (env, road),
     one logit per (env, edge));
  2. the collect loop at B = 4 096 in env-steps/s: goal_mlp beside embedding_dijkstra and edge_mlp_bf16, same session;
  3. the backward (tarl_policy_goal_mlp_bwd) at M = 32 and 4 096, beside the forward from observations.

    python tools/time_goal_mlp.py [--envs 4096] [--frames 64] [--skip-collect]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import ops, synth  # noqa: E402
from tarl_hip.engine import SimEngine  # noqa: E402
from tarl_hip.trainer import VecPPOTrainer  # noqa: E402
from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple  # noqa: E402


def five(fn, inner=10):
    """median and (min, max) in microseconds of five timings of ``inner`` back-to-back calls"""
    fn()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:.1f} us ({t[1]:.1f} - {t[2]:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    net = synth.torus_network(25, 25)
    N, E, Nmax = net.num_roads, net.edge_index.size(1), net.Nmax
    torch.manual_seed(0)
    ff = net.x[:, 3 * Nmax + 2][net.edge_index[1]].cuda()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    S = ops.goal_time_scale(net.x[:, 3 * Nmax:])
    pol.use_goal_mlp(S)
    gm, mm = pol.goal_mlp, pol.edge_mlp
    goal_params = [gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias]
    table = pol.dist_matrix
    emb = pol.nodes_embedding.weight.detach().reshape(-1).contiguous()
    print(f"config-4: N={N} E={E}, time_scale {S:.4f}")
    # 1. the fused logits launch beside the prior's
    for B in (64, args.envs):
        pops = synth.population_batch(16384, N, B, seed=21, device="cuda")
        eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, Nmax, pops,
                        congestion_constant=net.congestion_constant, seed=29)
        eng.reset()
        eng.prepare_policy(emb)
        for _ in range(20):
            eng.frame_fused()
        w = ops.GoalMlpWeights(*(p.data for p in goal_params))
        logits = torch.empty((B, E), device="cuda")
        nbytes = B * (N * 12 + E * 4)
        tg = five(lambda: ops.fused_goal_mlp_logits(eng.plan, eng.fs, eng._x, Nmax, eng.agents, w, table, S, out=logits))
        tp = five(lambda: ops.fused_prior_logits(eng.plan, eng.fs, eng._x, Nmax, eng.agents, emb, table, 1.0, out=logits))
        print(f"B={B}: tarl_fused_goal_mlp_logits {fmt(tg)}, tarl_fused_prior_logits {fmt(tp)}: {tg[0] / tp[0]:.2f}x; byte bound "
              f"{nbytes / 1e6:.1f} MB -> goal {nbytes / tg[0] / 1e6:.2f} TB/s, prior {nbytes / tp[0] / 1e6:.2f} TB/s", flush=True)
        # 3. forward and backward from observations
        if B == args.envs:
            obs_all = ops.fused_obs16(eng.plan, eng.fs, eng._x, Nmax, eng.agents)
            for M in (32, min(4096, B)):
                obs = obs_all[:M].contiguous()
                gl = torch.randn((M, E), device="cuda")
                grads = torch.zeros(ops.GOAL_MLP_PARAMS, device="cuda")
                scratch = torch.empty(ops.goal_mlp_bwd_scratch_floats(eng.plan, M), device="cuda")
                out = torch.empty((M, E), device="cuda")
                tf = five(lambda: ops.policy_goal_mlp(eng.plan, obs, w, table, S, out=out))
                tb = five(lambda: ops.policy_goal_mlp_bwd(eng.plan, obs, w, table, S, gl, grads, scratch=scratch))
                print(f"M={M}: tarl_policy_goal_mlp_fwd {fmt(tf)}, tarl_policy_goal_mlp_bwd {fmt(tb)} "
                      f"({scratch.numel() // ops.GOAL_MLP_PARAMS} partitions)", flush=True)
        del eng
        torch.cuda.empty_cache()
    if args.skip_collect:
        return
    # 2. the collect loop
    B, T = args.envs, args.frames
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    pops = synth.population_batch(16384, N, B, seed=21, device="cuda")
    for head in ("goal_mlp", "embedding_dijkstra", "edge_mlp_bf16"):
        eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, Nmax,
                        pops.clone(), congestion_constant=net.congestion_constant, seed=29)
        kw = dict(policy="goal_mlp", prior_table=table, goal_mlp_params=goal_params)
        if head == "embedding_dijkstra":
            kw = dict(policy="embedding_dijkstra", prior_table=table, prior_weight=1.0)
        elif head == "edge_mlp_bf16":
            kw = dict(policy="edge_mlp", policy_precision="bf16",
                      edge_mlp_params=[mm[0].weight, mm[0].bias, mm[2].weight, mm[2].bias, mm[4].weight, mm[4].bias])
        tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, sub_batch_size=32, extra_params=extra, **kw)
        tr.collect()
        tr.check_flags()
        rates = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.collect()
            torch.cuda.synchronize()
            rates.append(T * B / (time.perf_counter() - t0) / 1e6)
        tr.check_flags()
        print(f"collect B={B} T={T} {head} (rollout {tr.rollout}): {statistics.median(rates):.2f} M env-steps/s "
              f"({min(rates):.2f} - {max(rates):.2f})", flush=True)
        del tr, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
