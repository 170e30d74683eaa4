"""CPU: the inputs of tests/test_gpu_sibling_graphs.py reach the branches they are there for. SIBS and SIBS_TAILS
(tests/irregular_graphs.py) are the two graphs off the torus on which the plan sets ``siblings4`` — the Direction gather
then fetches the first four upstream rows once per chunk of four rows — and on which every road has out-edges and the road
count is a multiple of four — the action draw then takes its quad form. Everything here runs the CPU oracle alone: the
plan facts and degree sets of both graphs, a census of a run per graph (the counters of tests/test_irregular_host.py and
the admissions into roads of in-degree 1 to 3, whose embedded in-edge records end in padding), replays of the same inputs
with one deliberate restriction each — among them the one that tells SIBS_TAILS from SIBS: in-edges of in-rank >= 4
evaluated on sibling 0's sources — and a count of the seeded action draws by out-degree and out-rank. The thresholds are
conditions on the INPUTS, fixed before any kernel ran on them; the measured figures are printed (pytest -s) and recorded
in DESIGN.md."""
import pytest
import torch

import irregular_graphs as ig
from oracle import sim

CENSUS_SEED, POP_SEED = 2, 1
GRAPHS = ("SIBS", "SIBS_TAILS")


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


def in_lists(net):
    """Every road's in-edge sources in ascending edge id (the plan's CSC order)."""
    lists = [[] for _ in range(net.num_roads)]
    for s, d in net.edge_index.t().tolist():
        lists[d].append(s)
    return lists


def test_plan_facts_and_degree_sets():
    sibs, tails = ig.graph("SIBS"), ig.graph("SIBS_TAILS")
    for net in (sibs, tails):
        N = net.num_roads
        din, dout = ig.degrees(net)
        assert (N, net.edge_index.size(1), net.Nmax) == (56, 272, 41)
        assert ig.ops.fused_path_supported(net.edge_index, net.Nmax)
        f = ig.plan_facts(net)
        assert f["siblings4"] and not f["src_sorted"] and not f["dst_sorted"] and f["max_in"] == 9
        assert set(din.tolist()) == {0, 1, 2, 3, 4, 5, 8, 9}
        # the in-degrees differ from chunk to chunk and are equal inside every chunk
        assert din.view(-1, 4).tolist() == [[d] * 4 for v, d in enumerate(ig.SIBS_IN) for _ in range(ig.SIBS_OUT[v] // 4)]
        # the quad draw's condition: every road draws an action, and the roads make whole quads
        assert int(dout.min()) > 0 and N % 4 == 0
        assert all(s != d for s, d in net.edge_index.t().tolist())
    ins, ins_t = in_lists(sibs), in_lists(tails)
    fs, ft = ig.plan_facts(sibs), ig.plan_facts(tails)
    # SIBS: siblings share their whole in-list, in one order; every out-list is in ascending target order; rows group by
    # their out-lists as the intersections they enter, and the row pass walks the chunk table
    assert all(ins[r] == ins[r - r % 4] for r in range(56))
    assert all(l == sorted(l) for l in ig.out_lists(sibs))
    assert set(ig.degrees(sibs)[1].tolist()) == {4, 8} and fs["max_out"] == 8
    assert fs["group_sizes"] == [1, 2, 3, 4, 4, 4, 5, 8, 8, 8, 9] and fs["num_row_chunks"] == 17 and fs["row_siblings"]
    assert torch.equal(ig.sibling0_tail_edges(sibs.edge_index, 56), sibs.edge_index)      # the restriction is the identity
    # SIBS_TAILS: the same first four sources, and in every chunk of in-degree above four each of the siblings 1 .. 3
    # differs from sibling 0 in exactly one source of in-rank >= 4; the same edge ids, so the same in-ranks
    assert torch.equal(tails.edge_index[1], sibs.edge_index[1])
    assert int((tails.edge_index[0] != sibs.edge_index[0]).sum()) == ig.SIBS_TAILS_MOVED
    for r in range(56):
        differs = [q for q in range(len(ins_t[r])) if ins_t[r][q] != ins_t[r - r % 4][q]]
        assert ins_t[r][:4] == ins[r][:4]
        assert len(differs) == (1 if r % 4 and len(ins_t[r]) > 4 else 0) and all(q >= 4 for q in differs)
        assert len(set(ins_t[r])) == len(ins_t[r])
    assert not ft["row_siblings"]
    assert set(ig.degrees(tails)[1].tolist()) == set(range(1, 10)) and ft["max_out"] == 9      # every out-degree from 1 to 9
    moved = ig.sibling0_tail_edges(tails.edge_index, 56)[0] != tails.edge_index[0]
    assert int(moved.sum()) == ig.SIBS_TAILS_MOVED
    assert bool((ig.edge_ranks(tails.edge_index, 56)[0][moved] >= 4).all()) and bool((tails.edge_index[1][moved] % 4 != 0).all())
    # edge_attr is a distribution over every road's out-edges on both graphs
    for net in (sibs, tails):
        total = torch.zeros(56, dtype=torch.float64).index_add_(0, net.edge_index[0], net.edge_attr.view(-1).double())
        assert torch.allclose(total, torch.ones(56, dtype=torch.float64), atol=1e-6)


def test_random_state_and_tie_case_on_a_non_zero_sibling():
    """The random state the GPU cases start from is consistent on these degrees, and the crafted tie sits on sibling 1 of
    the nine-in-edge chunk: a row whose first four upstream words come from sibling 0's gather."""
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
        neighbour = sum(sel[r] in lists[r] for r in range(net.num_roads))
        assert 0.8 * net.num_roads <= neighbour < net.num_roads
        ea, e3, e4, road = ig.tie_case(net, x, 200.0, in_degree=9, which=ig.TIE_WHICH[name])
        irank, _ = ig.edge_ranks(net.edge_index, net.num_roads)
        assert road % 4 != 0 and int(ig.degrees(net)[0][road]) == 9 and int(irank[e3]) == 3 and int(irank[e4]) == 4
        u = ig.tie_uniform(torch.rand(net.edge_index.size(1), generator=torch.Generator().manual_seed(5)), net, road, e3, e4)
        xa, xb, xc = x.clone(), x.clone(), x.clone()
        ig.core_step_counted(xa, net, 200.0, u, ig.new_counters(), edge_attr=ea)
        ig.core_step_counted(xb, net, 200.0, u, ig.new_counters(), edge_attr=ea, last_max=True)
        sim.core_step(xc, net.edge_index, ea, 200.0, net.Nmax, uniform=u, congestion_constant=net.congestion_constant)
        assert torch.equal(xa, xc) and not torch.equal(xa, xb)      # the tie order decides this frame
        assert ig.tie_case(net, x.clone(), 200.0)[3] == road - road % 4      # the default stays the first road


@pytest.mark.parametrize("name", GRAPHS)
def test_census_conditions(runs, name):
    net, _, _, c = runs[name]
    for k in ig.COUNTERS + (ig.SHORT_IN,):
        assert c[k] >= 50, (k, c)
    # the rollouts carry a count byte per road, and the quad draw takes every road: nobody may be left out
    assert c["max_count"] < net.Nmax and c["done"] > 0, c
    assert int(ig.degrees(net)[1].min()) > 0 and net.num_roads % 4 == 0


@pytest.mark.parametrize("name", GRAPHS)
def test_a_kernel_that_drops_the_tails_would_be_noticed(runs, name):
    net, pop, frames, _ = runs[name]
    T = ig.CENSUS[name]["T"]
    first_in = ig.replay_restricted(net, pop, T, CENSUS_SEED, frames, drop_in_tail=True)
    first_out = ig.replay_restricted(net, pop, T, CENSUS_SEED, frames, drop_out_tail=True)
    print(f"\nfirst differing frame {name}: in-tail dropped {first_in}, out-tail dropped {first_out}")
    assert first_in is not None and first_out is not None


def test_a_kernel_that_shares_the_whole_in_list_would_be_noticed_on_sibs_tails_only(runs):
    """In-edges of in-rank >= 4 into siblings 1 .. 3 evaluated on sibling 0's sources: the true trajectory on SIBS, where
    siblings share everything, and a departure from it on SIBS_TAILS."""
    first = {}
    for name in GRAPHS:
        net, pop, frames, _ = runs[name]
        first[name] = ig.replay_restricted(net, pop, ig.CENSUS[name]["T"], CENSUS_SEED, frames, sibling0_tail=True)
    print(f"\nfirst differing frame, tails from sibling 0: {first}")
    assert first["SIBS"] is None and first["SIBS_TAILS"] is not None


def test_the_seeded_draws_cover_every_out_degree(runs):
    """The census run's actions on SIBS_TAILS: how often a road picks an out-edge of out-rank >= 4 (the quad draw's walk
    beyond its four embedded thresholds), and how often a road of out-degree 1 to 3 picks at all (thresholds padded beyond
    the degree). Every road with out-edges picks once per frame, so the inputs reach both counts hundreds of times."""
    net = runs["SIBS_TAILS"][0]
    _, orank = ig.edge_ranks(net.edge_index, net.num_roads)
    dout = ig.degrees(net)[1]
    high = short = 0
    by_degree = torch.zeros(10, dtype=torch.int64)
    for action, _ in ig.census_inputs(net, ig.CENSUS["SIBS_TAILS"]["T"], CENSUS_SEED):
        e = torch.nonzero(action).view(-1)
        assert e.numel() == net.num_roads
        high += int((orank[e] >= 4).sum())
        short += int((dout[net.edge_index[0][e]] < 4).sum())
        by_degree += torch.bincount(orank[e], minlength=10)
    print(f"\ndraws SIBS_TAILS: out-rank >= 4 {high}, on roads of out-degree 1 to 3 {short}, by out-rank {by_degree.tolist()}")
    assert high >= 50 and short >= 50
    assert int(by_degree[:9].min()) > 0      # every out-rank up to the largest out-degree is drawn
