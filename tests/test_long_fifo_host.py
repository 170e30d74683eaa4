"""CPU: the inputs of tests/test_gpu_long_fifo.py reach the FIFO-length limit of the packed path (Nmax = 127: a seven-bit
count beside HD_DIRTY, a seven-bit ring offset, one wrap of phys()), and a kernel that kept those fields in six bits could
not pass. Everything here runs the CPU oracle alone (tests/irregular_graphs.py): LONG127 and LONGMIX (16 roads of a 2 x 2
torus, 940 m each: MAX_NUMBER_OF_AGENT 126, Nmax 127; on LONGMIX every third road holds at most 14), 150 agents per road
due within 30 s — or all at once — and 300 frames. The thresholds are conditions on the INPUTS, fixed before any kernel ran
on them; the measured figures are printed (pytest -s) and recorded in DESIGN.md."""
import pytest
import torch

import irregular_graphs as ig
from oracle import sim

CENSUS_SEED, POP_SEED = 2, 1
RUNS = (("LONG127", 130), ("LONGMIX", 130), ("LONGMIX", 100))


@pytest.fixture(scope="module")
def runs():
    """The counted run of each (graph, last departure), computed once: -> (net, population, frames, counters)."""
    out = {}
    for name, t1 in RUNS:
        cfg = ig.CENSUS[name]
        net = ig.graph(name)
        pop = ig.population(net, cfg["per_road"], seed=POP_SEED, t1=t1)
        frames, counters = ig.long_fifo_counters(net, pop, cfg["T"], CENSUS_SEED, t1)
        shown = dict(counters, rings_wrapped=f"{int(counters['rings_wrapped'].sum())} of {net.num_roads}")
        print(f"\nlong FIFO run {name} t1={t1}: N={net.num_roads} E={net.edge_index.size(1)} Nmax={net.Nmax} {shown}")
        out[name, t1] = (net, pop, frames, counters)
    return out


def test_the_two_networks():
    for name in ig.LONG_GRAPHS:
        net = ig.graph(name)
        c = sim.Cols(net.Nmax)
        assert (net.num_roads, net.edge_index.size(1), net.Nmax) == (16, 64, 127)
        assert ig.ops.fused_path_supported(net.edge_index, net.Nmax)
        f = ig.plan_facts(net)
        assert f["siblings4"] and f["src_sorted"] and f["max_in"] == 4 and f["max_out"] == 4
        din, dout = ig.degrees(net)
        assert set(din.tolist()) == {4} and set(dout.tolist()) == {4}
        assert bool((net.x[:, c.FF] == 10.0).all())
        short = torch.zeros(16, dtype=torch.bool)
        short[::3] = name == "LONGMIX"
        assert bool((net.x[short, c.MAXN] == 14).all()) and bool((net.x[~short, c.MAXN] == 126).all())
        crit, cong = sim.congestion_constants(net.x, net.Nmax)
        assert torch.equal(net.critical_number, crit) and torch.equal(net.congestion_constant, cong)


@pytest.mark.parametrize("name", ig.LONG_GRAPHS)
def test_counters_reach_the_second_half_of_every_field(runs, name):
    net, _, _, c = runs[name, 130]
    c_maxn = net.x[:, 3 * net.Nmax]
    assert c["count_ge64"] >= 1000 and c["offset_ge64"] >= 500, c
    assert c["insert_frames_ge64"] >= 100 and c["insert_pos_ge64"] >= c["insert_frames_ge64"], c
    assert c["withdraw_ge2"] >= 50 and c["e_relief_admissions"] >= 200 and c["done"] >= 100, c
    assert c["max_count"] < net.Nmax, c
    assert bool(c["rings_wrapped"][c_maxn == 126].all()), c      # every ring of a MAX-126 road wraps (all 16 on LONG127)
    if name == "LONGMIX":
        assert c["at_max"] >= 10 and c["at_last_slot"] >= 1, c    # count == Nmax - 1: the packed row turns DIRTY


def test_backlog_of_a_whole_population_in_frame_0(runs):
    """Every agent due in frame 0: more than INS_CAP ready agents (the insert's ordered global-scratch path), and one road
    takes 100 or more of them in that frame."""
    net, pop, _, c = runs["LONGMIX", 100]
    assert c["due_frame0"] == pop.size(0) - 1 > ig.INS_CAP, c
    assert c["max_inserted_frame0"] >= 100 and c["max_count"] < net.Nmax and c["done"] >= 100, c


@pytest.mark.parametrize("name", ig.LONG_GRAPHS)
def test_a_kernel_with_six_bit_counts_would_be_noticed(runs, name):
    """(i) the Direction and Response messages read the counts through ``& 63``, (ii) the insert computes its capacity from
    ``count & 63``: each replay leaves the true trajectory within the run; with a mask that hides nothing both are the
    oracle."""
    net, pop, frames, _ = runs[name, 130]
    T = ig.CENSUS[name]["T"]
    assert ig.replay_long_restricted(net, pop, T, CENSUS_SEED, frames, message_mask=-1) is None
    assert ig.replay_long_restricted(net, pop, T, CENSUS_SEED, frames, capacity_mask=-1) is None
    first_msg = ig.replay_long_restricted(net, pop, T, CENSUS_SEED, frames, message_mask=63)
    first_cap = ig.replay_long_restricted(net, pop, T, CENSUS_SEED, frames, capacity_mask=63)
    print(f"\nfirst differing frame {name}: (i) messages read count & 63: {first_msg}, (ii) insert capacity from count & 63: {first_cap}")
    assert first_msg is not None and first_cap is not None


def test_random_state_fills_the_long_fifos():
    for name in ig.LONG_GRAPHS:
        net = ig.graph(name)
        c = sim.Cols(net.Nmax)
        lists = ig.out_lists(net)
        seen = 0
        for seed in range(3, 7):
            x = ig.random_state(net, seed=seed, t=200.0)
            n = x[:, c.N].long()
            assert int(n.min()) >= 0 and bool((n < x[:, c.MAXN].long()).all())
            seen = max(seen, int(n.max()))
            ids = x[:, :net.Nmax][torch.arange(net.Nmax).unsqueeze(0) < n.unsqueeze(1)]
            assert ids.numel() == ids.unique().numel() and float(ids.min()) >= 1
            sel = x[:, c.SEL].long().tolist()
            assert sum(sel[r] in lists[r] for r in range(net.num_roads)) >= 0.75 * net.num_roads      # 10 % are bogus on purpose
            static = [c.MAXN, c.FF, c.LEN, c.MAXFLOW, c.ROAD]
            assert torch.equal(x[:, static], net.x[:, static])
        assert seen == 125, seen      # MAX - 1: the fullest state the reference's domain has
