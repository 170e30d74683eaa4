"""Time one next-hop refresh of the classical dijkstra agent (DijkstraAgents.choice at count % refresh_rate == 0):
tarl_edge_travel_time plus either the all-pairs table (tarl_apsp) or one reverse tree per distinct destination of the
population (tarl_dest_trees), on BASELINE config 4's and config 5's graphs and two sizes between them (heterogeneous
torus, a population of 6.5 agents per road; 10.5 at config 5). The trees are timed on a congested state and at free
flow, the all-pairs table on the congested state. Also the per-step select kernel of each method, and the implied
refresh time of one simulated day (86 400 steps, a refresh every 10 steps).

All-pairs at config 5 runs only with --all-pairs-c5: its extract-min scans every node once per settled node, O(N^2) per
source and O(N^3) per table, with 16 B of state per node outside the LDS at N = 25 000."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import ops, synth  # noqa: E402

STEPS_PER_DAY, REFRESH_RATE = 86_400, 10


def timed(fn, reps, warm=True):
    if warm:
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all-pairs-c5", action="store_true", help="also time the all-pairs table at N = 25 000")
    args = ap.parse_args()
    cases = (("config-4 (25x25 torus, N=2500)", (25, 25), 16_384, True),
             ("25x50 torus (N=5000)", (25, 50), 32_768, True),
             ("25x100 torus (N=10000)", (25, 100), 65_536, True),
             ("config-5 (25x250 torus, N=25000)", (25, 250), 262_144, args.all_pairs_c5))
    for name, (W, H), agents, all_pairs in cases:
        net = synth.torus_network(W, H, heterogeneous=True, seed=1)
        N, Nmax = net.num_roads, net.Nmax
        plan = ops.Plan(net.edge_index, N)
        states = {"congested": synth.random_state(net, seed=7, fill=0.5).cuda(), "free flow": net.x.clone().cuda()}
        cc = net.congestion_constant.cuda()
        ag = synth.population(agents, N, seed=5).cuda()
        dests = torch.unique(ag[:, 1].to(torch.int64))                    # every row, dummy row 0 included
        slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        slot[dests] = torch.arange(dests.numel(), dtype=torch.int32, device="cuda")
        runs = [("per_destination", st) for st in states] + ([("all_pairs", "congested")] if all_pairs else [])
        out = {}
        for m, st in runs:
            x = states[st]
            if m == "per_destination":
                def refresh():
                    w = ops.edge_travel_time(plan, x, Nmax, cc)
                    out[m, st] = ops.destination_trees(plan, w[0], dests)[0]
                reps = 3
            else:
                def refresh():
                    w = ops.edge_travel_time(plan, x, Nmax, cc)
                    out[m, st] = ops.all_pairs_shortest_paths(plan, w)[0][0]
                reps = 3 if N <= 5_000 else 1
            ms = timed(refresh, reps, warm=reps > 1)          # the kernels are loaded by the smaller graphs already
            if m == "per_destination":
                sel = timed(lambda: ops.select_next_hop_dest(x, Nmax, ag, slot, out[m, st]), 20)
            else:
                sel = timed(lambda: ops.select_next_hop(x, Nmax, ag, out[m, st]), 20)
            day = ms * STEPS_PER_DAY / REFRESH_RATE / 1e3
            print(f"{name} {m} ({st}): {ms:.2f} ms per refresh (destinations {dests.numel()}, edges "
                  f"{net.edge_index.size(1)}); select {sel * 1e3:.1f} us per step; refreshes of one simulated day: "
                  f"{day:.1f} s", flush=True)
        if ("all_pairs", "congested") in out:   # the two tables on the same weights (heterogeneous torus: no ties expected)
            same = torch.equal(out["per_destination", "congested"].to(torch.int64),
                               out["all_pairs", "congested"][:, dests].t())
            print(f"{name}: per-destination rows == all-pairs columns: {same}", flush=True)
        del out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
