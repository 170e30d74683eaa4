"""CPU: the inputs of tests/test_gpu_irregular.py reach the branches they are there for, and a kernel that got those
branches wrong could not pass. Everything here runs the CPU oracle alone (tests/irregular_graphs.py): the degree sets and
plan facts of the two graphs, a census of a run per graph (how often an in-edge of in-rank >= 4 is admissible, races, wins,
Response messages on out-edges of out-rank >= 4, gridlock-relief admissions), and three replays of the same inputs with one
deliberate restriction each, which must leave the true trajectory within the run. The thresholds are conditions on the
INPUTS, fixed before any kernel ran on them; the measured figures are printed (pytest -s) and recorded in DESIGN.md."""
import pytest
import torch

import irregular_graphs as ig
from oracle import sim

CENSUS_SEED, POP_SEED = 2, 1
GRAPHS = ("MIXED", "HUB126")      # the sibling graphs of the same module: tests/test_sibling_graphs_host.py


@pytest.fixture(scope="module")
def runs():
    """The census run of each graph, computed once: name -> (net, population, frames, counters)."""
    out = {}
    for name in GRAPHS:
        cfg = ig.CENSUS[name]
        net = ig.graph(name)
        pop = ig.population(net, cfg["per_road"], seed=POP_SEED)
        frames, counters = ig.census(net, pop, cfg["T"], seed=CENSUS_SEED)
        print(f"\ncensus {name}: N={net.num_roads} E={net.edge_index.size(1)} Nmax={net.Nmax} {counters}")
        out[name] = (net, pop, frames, counters)
    return out


def test_degree_sets_and_plan_facts():
    mixed, hub = ig.graph("MIXED"), ig.graph("HUB126")
    din, dout = ig.degrees(mixed)
    assert ig.MIXED_DEGREES <= set(din.tolist()) and ig.MIXED_DEGREES <= set(dout.tolist())
    assert 70 <= mixed.num_roads <= 90 and 350 <= mixed.edge_index.size(1) <= 430
    hin, hout = ig.degrees(hub)
    assert int(hin.max()) == 126 and int(hout.max()) == 126 and 0 in hin.tolist() and 0 in hout.tolist()
    assert 256 < hub.num_roads <= 512 and 17000 <= hub.edge_index.size(1) <= 18500      # two roads per thread of the LDS rollout
    for net in (mixed, hub):
        assert ig.ops.fused_path_supported(net.edge_index, net.Nmax) and net.Nmax <= 127
        f = ig.plan_facts(net)
        assert not f["src_sorted"] and not f["dst_sorted"] and not f["siblings4"]
        # rows group by their out-lists in groups of mixed size, some of them no multiple of four: partial chunks, and the
        # row pass walks the chunk table (few enough chunks) on both graphs
        assert len(set(f["group_sizes"])) > 3 and any(s % 4 for s in f["group_sizes"]) and any(s > 4 for s in f["group_sizes"])
        assert f["num_row_chunks"] > net.num_roads // 4 and f["row_siblings"]
        # a road's own out-list is in ascending edge id AND ascending target order; the in-lists are not source-ordered
        assert all(l == sorted(l) for l in ig.out_lists(net))
    fm = ig.plan_facts(mixed)
    assert fm["max_in"] == 9 and fm["max_out"] == 9 and {5, 8, 9} <= set(fm["group_sizes"])      # chunks 4+1, 4+4, 4+4+1
    assert ig.plan_facts(hub)["max_in"] == 126 and 126 in ig.plan_facts(hub)["group_sizes"]
    # the plan records only N and E on the host side (tests/fake_plan.py): the rest of these facts is what
    # tarl_plan_create derives, restated in ig.plan_facts and compared with the real plan by the GPU suite
    from fake_plan import fake_plan
    p = fake_plan(mixed.num_roads, mixed.edge_index.size(1))
    assert (p.N, p.E) == (mixed.num_roads, mixed.edge_index.size(1))


def test_random_state_is_consistent_on_any_degree():
    for name in GRAPHS:
        net = ig.graph(name)
        c = sim.Cols(net.Nmax)
        lists = ig.out_lists(net)
        x = ig.random_state(net, seed=3, t=200.0)
        n = x[:, c.N].long()
        assert int(n.min()) >= 0 and bool((n < x[:, c.MAXN].long()).all()) and int((n == 0).sum()) > 0
        ids = x[:, :net.Nmax][torch.arange(net.Nmax).unsqueeze(0) < n.unsqueeze(1)]
        assert ids.numel() == ids.unique().numel() and float(ids.min()) >= 1
        sel = x[:, c.SEL].long().tolist()
        with_out = [r for r in range(net.num_roads) if lists[r]]
        neighbour = sum(sel[r] in lists[r] for r in with_out)
        assert 0.8 * len(with_out) <= neighbour < len(with_out)                # most select a neighbour, some do not
        assert all(sel[r] == 0 for r in range(net.num_roads) if not lists[r])  # roads without out-edges keep theirs
        static = [c.MAXN, c.FF, c.LEN, c.MAXFLOW, c.ROAD]
        assert torch.equal(x[:, static], net.x[:, static])


@pytest.mark.parametrize("name", ["MIXED", "HUB126"])
def test_census_conditions(runs, name):
    net, _, _, c = runs[name]
    for k in ("a_tail_admissible", "b_tail_in_race", "c_tail_wins", "d_tail_response"):
        assert c[k] >= 50, (k, c)
    if name == "MIXED":
        assert c["e_relief_admissions"] >= 50, c
    assert c["max_count"] < net.Nmax and c["done"] > 0, c


@pytest.mark.parametrize("name", ["MIXED", "HUB126"])
def test_a_kernel_that_drops_the_tails_would_be_noticed(runs, name):
    """(i) no in-edge of in-rank >= 4 in the Direction message, (ii) no out-edge of out-rank >= 4 in the Response message:
    each replay leaves the true trajectory within the run."""
    net, pop, frames, _ = runs[name]
    T = ig.CENSUS[name]["T"]
    first_in = ig.replay_restricted(net, pop, T, CENSUS_SEED, frames, drop_in_tail=True)
    first_out = ig.replay_restricted(net, pop, T, CENSUS_SEED, frames, drop_out_tail=True)
    print(f"\nfirst differing frame {name}: (i) in-tail dropped {first_in}, (ii) out-tail dropped {first_out}")
    assert first_in is not None and first_out is not None
    # (the unrestricted restatement IS the oracle: ig.census asserts that against sim.env_step frame by frame)


def test_a_kernel_with_the_wrong_tie_order_would_be_noticed(runs):
    """(iii) last maximum instead of first. Natural noise never ties (the replay of the census run stays on the true
    trajectory), so a handful of crafted frames follow: bit-equal scores on in-ranks 3 and 4 of a nine-edge race."""
    net, pop, frames, _ = runs["MIXED"]
    T = ig.CENSUS["MIXED"]["T"]
    assert ig.replay_restricted(net, pop, T, CENSUS_SEED, frames, last_max=True) is None
    gen = torch.Generator().manual_seed(5)
    first = None
    for k in range(4):
        t = 200.0 + k
        x = ig.random_state(net, seed=40 + k, t=t)
        ea, e3, e4, road = ig.tie_case(net, x, t)
        u = ig.tie_uniform(torch.rand(net.edge_index.size(1), generator=gen), net, road, e3, e4)
        irank, _ = ig.edge_ranks(net.edge_index, net.num_roads)
        assert int(irank[e3]) == 3 and int(irank[e4]) == 4 and int(ig.degrees(net)[0][road]) == 9
        xa, xb, xc = x.clone(), x.clone(), x.clone()
        ig.core_step_counted(xa, net, t, u, ig.new_counters(), edge_attr=ea)
        ig.core_step_counted(xb, net, t, u, ig.new_counters(), edge_attr=ea, last_max=True)
        sim.core_step(xc, net.edge_index, ea, t, net.Nmax, uniform=u, congestion_constant=net.congestion_constant)
        assert torch.equal(xa, xc)
        # the true run admits the head of rank 3's road, the last-maximum run the head of rank 4's
        n0 = int(x[road, 3 * net.Nmax + 1])
        j3, j4 = int(net.edge_index[0, e3]), int(net.edge_index[0, e4])
        assert x[j3, 0] != x[j4, 0] and not bool((x[road, :n0 + 1] == x[j3, 0]).any() | (x[road, :n0 + 1] == x[j4, 0]).any())
        assert bool((xa[road, :n0 + 1] == x[j3, 0]).any()) and not bool((xa[road, :n0 + 1] == x[j4, 0]).any())
        assert bool((xb[road, :n0 + 1] == x[j4, 0]).any()) and not bool((xb[road, :n0 + 1] == x[j3, 0]).any())
        if first is None and not torch.equal(xa, xb):
            first = T + k
    print(f"\nfirst differing frame MIXED: (iii) last maximum {first} (crafted frames start at {T})")
    assert first == T
