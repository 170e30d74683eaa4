"""Collect-loop throughput of the three policy heads at BASELINE config 4 (25 x 25 torus, N = 2 500 roads, E = 10 000,
16 384 agents; --torus / --agents for other sizes), B = 4 096 environments, T = 64 frames per collect: ``embedding``
(state-independent tables, the trainer's default four-launch rollout), ``embedding_dijkstra`` (tarl_fused_rollout_prior:
per-frame prior logits from the packed state) and ``edge_mlp`` with bf16 logits (tarl_fused_rollout_policy). env-steps/s
= T * B / seconds of one VecPPOTrainer.collect(). Then the prior kernel alone (tarl_fused_prior_logits) and the sampler it feeds
(tarl_graphdist_rollout), timed with HIP events on the launch stream, against the prior kernel's compulsory bytes.

    python tools/time_prior.py [--envs 4096] [--frames 64] [--reps 3] [--prior-method all_pairs|per_destination|both]
                               [--torus 25x25] [--agents 16384] [--heads embedding,embedding_dijkstra,edge_mlp_bf16]

--prior-method picks where the prior head's distances come from (MPNNPolicyNet.prior_method); "both" runs the prior head
once per method in the same session. Each method first reports its table build (tarl_apsp's N x N table or
tarl_prior_dest_table's N x D table over the population's destinations) with its time and the peak device memory of the
build. --torus W x H sets the graph (config 5: 25x250 with --agents 262144).
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
from src.agents.base import destination_set  # noqa: E402
from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple  # noqa: E402


def event_ms(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def build_table(method, plan, ff, agents):
    """-> (table, dest_slot) of one prior method, with its build time and peak device memory printed."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    if method == "all_pairs":
        table, slot = ops.all_pairs_shortest_paths(plan, ff, want_next_hop=False, want_dist=True)[1][0], None
    else:
        dests, slot = destination_set(agents, plan.num_nodes)
        table = ops.prior_dest_table(plan, ff, dests)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    print(f"  {method} table {tuple(table.shape)}: built in {s * 1e3:.1f} ms, peak device memory {peak / 2**20:.0f} MiB "
          f"(table {table.numel() * 4 / 2**20:.0f} MiB)", flush=True)
    return table, slot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--agents", type=int, default=16384)
    ap.add_argument("--prior-method", choices=("all_pairs", "per_destination", "both"), default="all_pairs")
    ap.add_argument("--torus", default="25x25", help="W x H of the heterogeneous torus (N = 4 W H roads)")
    ap.add_argument("--heads", default="embedding,embedding_dijkstra,edge_mlp_bf16")
    args = ap.parse_args()
    B, T = args.envs, args.frames
    W, H = (int(v) for v in args.torus.lower().split("x"))
    net = synth.torus_network(W, H)
    N, E = net.num_roads, net.edge_index.size(1)
    torch.manual_seed(0)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l, mm = val.final_mlp, pol.edge_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    pops = synth.population_batch(args.agents, N, B, seed=21, device="cuda")
    methods = ("all_pairs", "per_destination") if args.prior_method == "both" else (args.prior_method,)
    runs = [(h, m) for h in args.heads.split(",") for m in (methods if h == "embedding_dijkstra" else (None,))]
    name = "config-4" if (W, H) == (25, 25) else f"{W}x{H} torus (N={N})"
    for head, method in runs:
        eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                        pops.clone(), congestion_constant=net.congestion_constant, seed=29)
        kw = dict(policy="embedding")
        slot = None
        if head == "embedding_dijkstra":
            table, slot = build_table(method, eng.plan, ff, eng.agents)
            kw = dict(policy="embedding_dijkstra", prior_table=table, prior_weight=1.0)
            if slot is not None:       # the trainer builds (and checks the size of) its own table
                kw = dict(policy="embedding_dijkstra", prior_free_flow=ff, prior_dests=destination_set(eng.agents, N))
        elif head == "edge_mlp_bf16":
            kw = dict(policy="edge_mlp", policy_precision="bf16",
                      edge_mlp_params=[mm[0].weight, mm[0].bias, mm[2].weight, mm[2].bias, mm[4].weight, mm[4].bias])
        tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, sub_batch_size=32, extra_params=extra,
                           **kw)
        if slot is not None:
            del table
            table, slot = tr.prior_table, tr.prior_dest_slot
        tr.collect()
        tr.check_flags()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            tr.collect()
        torch.cuda.synchronize()
        s = (time.perf_counter() - t0) / args.reps
        tr.check_flags()
        label = head if method is None else f"{head} [{method}]"
        print(f"{name} B={B} T={T} {label} (rollout {tr.rollout}): {T * B / s / 1e6:.2f} M env-steps/s "
              f"({s / T * 1e3:.3f} ms per frame)", flush=True)
        if head == "embedding_dijkstra":
            emb = pol.nodes_embedding.weight.detach().reshape(-1).contiguous()
            logits = torch.empty((B, E), device="cuda")
            ms = event_ms(lambda: ops.fused_prior_logits(eng.plan, eng.fs, eng._x, net.Nmax, eng.agents, emb, table, 1.0,
                                                         out=logits, dest_slot=slot), 20)
            nbytes = B * (N * 12 + E * 4)      # packed word + head's destination per (env, road), one logit per (env, edge)
            kname = "tarl_fused_prior_logits" + ("" if slot is None else "_dest")
            print(f"  {kname}: {ms * 1e3:.1f} us per frame, compulsory {nbytes / 1e6:.0f} MB -> {nbytes / ms / 1e9:.2f} TB/s",
                  flush=True)
            c8 = torch.empty((B, N), dtype=torch.uint8, device="cuda")
            scratch = torch.empty((int(ops._lib.load().tarl_graphdist_rollout_scratch_bytes(eng.plan.handle, B)) + 7) // 8,
                                  dtype=torch.float64, device="cuda")
            sel = eng.fs.sel8.clone()
            ms_s = event_ms(lambda: ops.graphdist_rollout(eng.plan, logits, 1.0, seed=1, counter=1, choice8=c8, sel8=sel,
                                                          scratch=scratch), 20)
            print(f"  tarl_graphdist_rollout (sample + log-prob of those logits): {ms_s * 1e3:.1f} us per frame", flush=True)
        del tr, eng
        table = slot = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
