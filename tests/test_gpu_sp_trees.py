"""GPU: the shared core of the shortest-path tree kernels (csrc/sp_trees.h). The per-origin and the per-destination trees
are one algorithm with the two adjacencies swapped, so a tree from r on a graph G and a tree towards r on its transpose
must be the same tree bit for bit; and the shared launcher raises the dynamic-LDS limit once the bitmaps pass 64 KB,
which only a graph of more than 131 072 nodes reaches."""
import pytest
import torch

from tree_restatement import adjacency, check_table, check_tree, cpu_dijkstra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def _torus_case(W, H, het, roots):
    from tarl_hip import synth
    net = synth.torus_network(W, H, heterogeneous=het, seed=4)
    x = synth.random_state(net, seed=2) if het else net.x
    return net.edge_index, net.num_roads, x, net.Nmax, net.congestion_constant, roots(net.num_roads)


def _matsim_case(tmp_path):
    from src.matsim_io import build_network
    from tarl_hip import synth
    synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 5, 4, seed=2, heterogeneous=True)
    graph, Nmax = build_network(str(tmp_path / "network"))
    N = graph.x.size(0)
    return graph.edge_index.cpu(), N, graph.x, Nmax, graph.congestion_constant, torch.arange(N, dtype=torch.int64)


@pytest.mark.parametrize("case", ["torus_6x5_het", "torus_12x9_hom", "matsim_5x4_src_dest"])
def test_forward_and_reverse_trees_are_mirror_images(ops, tmp_path, case):
    """shortest_path_trees on G against destination_trees on G transposed (edge_index.flip(0): the same edge ids, the same
    weight order), weights as DijkstraAgents routes on them (tarl_edge_travel_time, fp32): both accumulate fp64 from the
    root outwards, so dist is equal bit for bit, and pred == next_hop except at the root (-1 against the root itself)."""
    if case == "torus_6x5_het":
        ei, N, x, Nmax, cc, roots = _torus_case(6, 5, True, lambda n: torch.arange(n, dtype=torch.int64))
    elif case == "torus_12x9_hom":            # nearly every pair ties: the tie rule decides
        ei, N, x, Nmax, cc, roots = _torus_case(12, 9, False, lambda n: torch.arange(0, n, 7, dtype=torch.int64))
    else:
        ei, N, x, Nmax, cc, roots = _matsim_case(tmp_path)
    plan = ops.Plan(ei, N)
    w = ops.edge_travel_time(plan, x.cuda(), Nmax, cc.cuda())[0]
    if case == "torus_12x9_hom":
        assert bool((w == w[0]).all())
    roots = roots.cuda()
    dist, pred = ops.shortest_path_trees(plan, w.double(), roots)
    next_hop, dist_t = ops.destination_trees(ops.Plan(ei.flip(0).contiguous(), N), w, roots, want_dist=True)
    assert torch.equal(dist, dist_t), "distances"
    at_root = torch.zeros_like(pred, dtype=torch.bool)
    at_root[torch.arange(roots.numel(), device="cuda"), roots] = True
    assert bool((pred[at_root] == -1).all()) and torch.equal(next_hop[at_root], roots.to(torch.int32))
    assert torch.equal(pred[~at_root], next_hop[~at_root]), "links"
    assert bool((pred[~at_root] >= 0).any())
    if case == "matsim_5x4_src_dest":          # SRC / DEST pseudo-nodes: pairs no path joins
        assert bool(torch.isinf(dist).any()) and bool((pred[~at_root] == -1).any())


def test_launch_above_64k_of_lds(ops):
    """182 x 182 heterogeneous torus: N = 132 496 roads, 66 256 B of LDS for the four bitmaps of the tree kernels, above the
    64 KB a launch gets without raising the limit. One source (tarl_sssp_f64) and one destination (tarl_dest_trees) at
    free flow against the CPU Dijkstra. The same destination through tarl_prior_dest_table, whose two bitmaps (33 128 B)
    stay below the limit: its column is the fp32 rounding of the CPU's fp64 distances."""
    from tarl_hip import synth
    net = synth.torus_network(182, 182, heterogeneous=True, seed=1)
    ei, N = net.edge_index, net.num_roads
    assert 16 * ((N + 31) // 32) > 64 * 1024
    w = net.x[:, 3 * net.Nmax + 2][ei[1]].contiguous()                     # fp32: an edge costs what its head node costs
    w64 = w.double()
    plan = ops.Plan(ei, N)
    src = torch.tensor([N // 3], dtype=torch.int64)
    dst = torch.tensor([2 * N // 3 + 1], dtype=torch.int64)

    dist, pred = ops.shortest_path_trees(plan, w64.cuda(), src.cuda())
    dc, _ = cpu_dijkstra(adjacency(ei, w64, N), N, int(src))
    assert torch.equal(dist[0].cpu(), torch.tensor(dc, dtype=torch.float64)), "distances from the source"
    check_tree(ei, w64, N, src, dist, pred)

    next_hop, dist_d = ops.destination_trees(plan, w.cuda(), dst.cuda(), want_dist=True)
    dc, _ = cpu_dijkstra(adjacency(ei, w64, N, reverse=True), N, int(dst), reverse=True)
    dc = torch.tensor(dc, dtype=torch.float64)
    assert torch.equal(dist_d[0].cpu(), dc), "distances to the destination"
    check_table(ei, w, N, dst, dist_d, next_hop)

    table = ops.prior_dest_table(plan, w.cuda(), dst.cuda())
    assert table.shape == (N, 1) and torch.equal(table[:, 0].cpu(), dc.to(torch.float32))
