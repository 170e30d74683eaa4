"""Timing of the graph-transformer critic at BASELINE config 4 (25 x 25 torus, N = 2 500 roads, E = 10 000, 16 384 agents),
B = 4 096 environments, T frames per collect, under the graph-transformer policy head: the critic's forward on one frame's
B observations (tarl_value_gt_fwd, HIP events) and its fraction of the fp32 vector peak (157 TFLOP/s); the all-frames critic
pass over the (T + 1) * B stored observations; one minibatch step; one training iteration (collect + update) against the
same run with the simple critic. A kernel breakdown comes from running this under
``rocprofv3 --kernel-trace --stats -- python tools/time_gt_value.py``.

    python tools/time_gt_value.py [--envs 4096] [--frames 8] [--reps 3]
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
from src.agents.transformer_agent import ValueNet  # noqa: E402
from src.transformer import laplacian_pe  # noqa: E402


def _events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--agents", type=int, default=16384)
    args = ap.parse_args()
    B, T, reps = args.envs, args.frames, args.reps
    net = synth.torus_network(25, 25)
    N = net.num_roads
    torch.manual_seed(0)
    pe = laplacian_pe(net.edge_index, N, N)
    pol = MPNNPolicyNet(net.edge_index, N, None, device="cuda")
    pol.use_graph_transformer(pe)
    simple = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    gtv = ValueNet(net.edge_index, N, "cuda", pe)
    l = simple.final_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    pops = synth.population_batch(args.agents, N, B, seed=21, device="cuda")
    kw = dict(rollout_steps=T, sub_batch_size=32, extra_params=extra, num_epochs=2 * reps + 4, policy="graph_transformer",
              gt_params=pol.transformer.kernel_tensors(), gt_pe=pol.gt_pe, temperature=500.0)
    for value in ("simple", "graph_transformer"):
        eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                        pops.clone(), congestion_constant=net.congestion_constant, seed=29)
        if value == "simple":
            tr = VecPPOTrainer(eng, pol.nodes_embedding.weight,
                               [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias], **kw)
        else:
            tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, list(gtv.transformer.parameters()), value=value,
                               gt_value_params=gtv.kernel_tensors(), gt_value_pe=gtv.gt_pe, **kw)
        tr.collect()
        adv, tgt = tr.advantages()
        tr.minibatch_step(adv, tgt)
        torch.cuda.synchronize()
        if value == "graph_transformer":
            w = ops.GtValueWeights(gtv.kernel_tensors())
            obs = tr.obs_all[0].contiguous()
            out = torch.empty(B, device="cuda")
            scratch = torch.empty(ops.value_gt_fwd_scratch_bytes(eng.plan, B) // 4, device="cuda")
            ms = _events_ms(lambda: ops.value_gt_forward(eng.plan, obs, gtv.gt_pe, w, out=out, scratch=scratch), 5)
            # multiply-adds per environment-frame: per node node_emb + 2 layers x (WQ, WK, WV, n_gate, WO, 2 FFN) = 15 x 256,
            # the attention (score + message: 2 x 16 per in-edge and layer), pe_emb hoisted; mu_mlp per sample
            macs = N * 15 * 256 + net.edge_index.size(1) * 2 * 2 * 16 + 272
            flop = 2.0 * macs * B
            print(f"config-4 B={B}: tarl_value_gt_fwd {ms:.3f} ms per frame, {flop / 1e9:.0f} GFLOP -> "
                  f"{flop / ms / 1e9:.1f} TFLOP/s ({flop / ms / 1e9 / 157.0 * 100:.1f} % of the fp32 vector peak)", flush=True)
            ms = _events_ms(tr._gt_value_all_frames, reps)
            print(f"  all-frames critic pass, (T + 1) * B = {(T + 1) * B} observations: {ms:.2f} ms", flush=True)
        ms = _events_ms(lambda: tr.minibatch_step(adv, tgt), reps)
        print(f"config-4 B={B} T={T} value={value}: one minibatch step {ms:.2f} ms", flush=True)
        tr._epoch = 0
        tr.train_iteration()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            tr.num_epochs = 1
            tr.train_iteration()
        torch.cuda.synchronize()
        s = (time.perf_counter() - t0) / reps
        tr.check_flags()
        print(f"config-4 B={B} T={T} value={value}: one training iteration (collect + 1 epoch) {s * 1e3:.1f} ms "
              f"({T * B / s / 1e6:.3f} M env-steps/s)", flush=True)
        del tr, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
