"""Collect-loop throughput of the graph-transformer head at BASELINE config 4 (25 x 25 torus, N = 2 500 roads, E = 10 000,
16 384 agents), B = 4 096 environments, T frames per collect, against ``embedding_dijkstra`` and bf16 ``edge_mlp``;
env-steps/s = T * B / seconds of one VecPPOTrainer.collect(). Then the head's forward alone (tarl_policy_gt_fwd on the
B observations of one frame) with HIP events, and its fraction of the fp32 vector peak (157 TFLOP/s) at the head's
arithmetic (multiply-adds per environment-frame counted below). A kernel breakdown comes from running this under
``rocprofv3 --kernel-trace --stats -- python tools/time_gt.py``.

    python tools/time_gt.py [--envs 4096] [--frames 16] [--reps 2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import ops, synth  # noqa: E402
from tarl_hip.engine import SimEngine  # noqa: E402
from tarl_hip.trainer import VecPPOTrainer  # noqa: E402
from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple  # noqa: E402
from src.transformer import laplacian_pe  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--agents", type=int, default=16384)
    args = ap.parse_args()
    B, T = args.envs, args.frames
    net = synth.torus_network(25, 25)
    N, E = net.num_roads, net.edge_index.size(1)
    torch.manual_seed(0)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.use_graph_transformer(laplacian_pe(net.edge_index, N, N))
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l, mm = val.final_mlp, pol.edge_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    pops = synth.population_batch(args.agents, N, B, seed=21, device="cuda")
    tt = pol.transformer.kernel_tensors()
    for head in ("graph_transformer", "embedding_dijkstra", "edge_mlp_bf16"):
        eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                        pops.clone(), congestion_constant=net.congestion_constant, seed=29)
        if head == "graph_transformer":
            kw = dict(policy="graph_transformer", gt_params=tt, gt_pe=pol.gt_pe, temperature=500.0)
        elif head == "embedding_dijkstra":
            kw = dict(policy="embedding_dijkstra", prior_table=pol.dist_matrix, prior_weight=1.0)
        else:
            kw = dict(policy="edge_mlp", policy_precision="bf16",
                      edge_mlp_params=[mm[0].weight, mm[0].bias, mm[2].weight, mm[2].bias, mm[4].weight, mm[4].bias])
        tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, sub_batch_size=32, extra_params=extra,
                           **kw)
        tr.collect()
        tr.check_flags()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            tr.collect()
        torch.cuda.synchronize()
        s = (time.perf_counter() - t0) / args.reps
        tr.check_flags()
        print(f"config-4 B={B} T={T} {head} (rollout {tr.rollout}): {T * B / s / 1e6:.3f} M env-steps/s "
              f"({s / T * 1e3:.3f} ms per frame)", flush=True)
        if head == "graph_transformer":
            obs = ops.fused_obs16(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents)
            w = ops.GtWeights(tt)
            logits = torch.empty((B, E), device="cuda")
            ops.policy_gt_logits(eng.plan, obs, eng.ec, pol.gt_pe, w, out=logits)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                ops.policy_gt_logits(eng.plan, obs, eng.ec, pol.gt_pe, w, out=logits)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 5
            # multiply-adds per environment-frame: nodes 5 x 256 (node_emb, WQ, WK, WV, n_gate) + attention + 4 x 256 (WO,
            # FFN) + 2 x 256 (WQ2, WK2); edges 2 x 3 x 256 (WOe, FFN_e per layer) + 256 (WE2) + 16 (edge_linear)
            macs = N * (5 * 256 + 4 * 256 + 2 * 256) + E * (2 * 3 * 256 + 256 + 16)
            flop = 2.0 * macs * B
            print(f"  tarl_policy_gt_fwd: {ms:.3f} ms per frame, {flop / 1e9:.0f} GFLOP -> {flop / ms / 1e9:.1f} TFLOP/s "
                  f"({flop / ms / 1e9 / 157.0 * 100:.1f} % of the fp32 vector peak)", flush=True)
        del tr, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
