"""Time one MSA iteration's all-or-nothing assignment (per-origin trees, tarl_msa_assign_sssp) on BASELINE config 4's and
config 5's graphs, and the all-pairs path (tarl_apsp_f64 + tarl_msa_assign) at config 4 for comparison. Free-flow costs,
heterogeneous torus; the OD demand is built the way run_msa builds it."""
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

from tarl_hip import ops, synth  # noqa: E402
from src.algorithms.user_equilibrium_msa import build_demand  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for name, (W, H), agents, methods in (("config-4 (25x25 torus, N=2500)", (25, 25), 16_384, ("per_origin", "all_pairs")),
                                      ("config-5 (25x250 torus, N=25000)", (25, 250), 262_144, ("per_origin",))):
    net = synth.torus_network(W, H, heterogeneous=True, seed=1)
    N, E = net.num_roads, net.edge_index.size(1)
    plan = ops.Plan(net.edge_index, N)
    w = net.x[:, 3 * net.Nmax + 2].to(torch.float64)[net.edge_index[1]].contiguous().cuda()
    ag = types.SimpleNamespace(agent_features=synth.population(agents, N, seed=5).cuda(), ORIGIN=0, DESTINATION=1)
    od_o, od_d, od_vol = build_demand(ag, N)
    origins, per = torch.unique_consecutive(od_o, return_counts=True)
    od_ptr = torch.zeros(origins.numel() + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(per, 0, out=od_ptr[1:])
    road = torch.ones(N, dtype=torch.uint8, device="cuda")
    aux = torch.zeros(N, dtype=torch.float64, device="cuda")
    for m in methods:
        if m == "per_origin":
            def step():
                aux.zero_()
                ops.msa_assign_trees(plan, w, origins, od_ptr, od_d, od_vol, road, aux)
        else:
            def step():
                aux.zero_()
                nh = ops.all_pairs_shortest_paths(plan, w)[0][0]
                ops.msa_assign(nh, od_o, od_d, od_vol, road, aux)
        ms = timed(step, 5)
        relax = E * origins.numel() if m == "per_origin" else E * N
        print(f"{name} {m}: {ms:.2f} ms per iteration (sources {origins.numel()}, pairs {od_d.numel()}, "
              f"edges x sources {relax:.3g}, assigned volume {float(aux.sum()):.0f})", flush=True)
    # per-phase split of the per-origin kernel: the trees alone (distances + predecessors, no walk)
    d_only = timed(lambda: ops.shortest_path_trees(plan, w, origins, want_dist=False, want_pred=True), 3)
    print(f"{name} trees only (no OD walk, pred written out): {d_only:.2f} ms", flush=True)
