"""CPU: the cases of tests/test_gpu_sp_irregular.py can see the faults they are there to catch. Everything here runs the
CPU restatements alone (tests/sp_cases.py, oracle/routing.py, tests/tree_restatement.py): the golden from real networkx
against the graphs and the oracle, a census of the two graphs, and the restatements with one deliberate restriction each —
weights fetched in list position instead of by edge id, lists cut after four entries, the rank lookup confined to the four
embedded out-edges, the other family's tie rule — each of which must fail the check the GPU test applies to the kernel.
The thresholds are conditions on the INPUTS; the measured figures are printed (pytest -s) and recorded in DESIGN.md."""
import pytest
import torch

import irregular_graphs as ig
import sp_cases as S

CASES = [(n, t) for n in S.NAMES for t in S.WEIGHTS]


def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# ---- A. the golden ---------------------------------------------------------------------------------------------------------
def test_golden_holds_the_graphs_and_the_oracle_reproduces_networkx():
    g = S.golden()
    have = set()
    for name in S.NAMES:
        c = S.case(name)
        assert torch.equal(g[f"{name}__edge_index"], ig.graph(name).edge_index), f"{name}: the graph left its golden"
        for tag in S.WEIGHTS:
            if f"{name}__next_hop_{tag}" not in g:
                continue
            have.add((name, tag))
            assert torch.equal(g[f"{name}__w_{tag}"], c.w[tag]) and g[f"{name}__w_{tag}"].dtype == torch.float32
            nh, dist = S.all_pairs(name, tag)
            assert g[f"{name}__next_hop_{tag}"].dtype == torch.int16
            assert torch.equal(nh.to(torch.int16), g[f"{name}__next_hop_{tag}"]), f"{name}/{tag}: oracle against networkx"
            S.check_all_pairs(name, tag, nh, dist)
    assert have == {("MIXED", "ff"), ("MIXED", "r5"), ("HUB126", "r5")}
    assert torch.equal(S.case("MIXED").w["r5"].unique(), torch.tensor([5.0, 10.0, 15.0]))


# ---- census ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_census(name):
    c = S.case(name)
    din, dout = ig.degrees(c.net)
    assert int(din.max()) == S.MAX_DEGREE[name] and int(dout.max()) == S.MAX_DEGREE[name]
    assert int((dout == 0).sum()) == 2 and int((din == 0).sum()) == 2          # two dead ends, two roads nobody can enter
    ident = torch.arange(c.E)
    assert not torch.equal(c.out_eid, ident) and not torch.equal(c.in_eid, ident)
    # networkx's DiGraph and the kernel's edge list are the same graph: no parallel dual edges, no self-loops
    key = c.ei[0] * c.N + c.ei[1]
    assert key.unique().numel() == c.E and not bool((c.ei[0] == c.ei[1]).any())
    for tag in S.WEIGHTS:
        nh, dist = S.all_pairs(name, tag)
        assert int((nh < 0).sum()) == S.UNREACHABLE[name] and int(torch.isinf(dist).sum()) == S.UNREACHABLE[name]
        for reverse in (True, False):
            assert int(torch.isinf(S.trees(name, tag, reverse)[0]).sum()) == S.UNREACHABLE[name]
    assert (c.N + 31) // 32 == {"MIXED": 3, "HUB126": 9}[name] and c.N % 32 != 0      # bitmaps end in a partial word
    assert c.E % 64 != 0
    print(f"\ncensus {name}: N={c.N} E={c.E} max degree {int(dout.max())}, unreachable pairs {S.UNREACHABLE[name]} of {c.N * c.N}")


def test_the_restatements_without_a_restriction_are_the_references():
    """The list walk of k_apsp and the rounds of spt_distances, restated, give what the oracle and the heap Dijkstra give."""
    for name, tag in CASES:
        c = S.case(name)
        nh, dist = S.all_pairs_lists(c, c.w[tag])
        S.check_all_pairs(name, tag, nh, dist)
        for reverse in (True, False):
            assert torch.equal(S.tree_distances_rounds(c, c.w[tag], reverse), S.trees(name, tag, reverse)[0])


# ---- identity edge ids -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES)
def test_weights_in_list_position_would_be_noticed(name, tag):
    """``w[k]`` for ``w[out_eid[k]]`` (k_apsp's relaxation, the pull of the per-destination trees) and for ``w[in_eid[k]]``
    (the pull of the per-origin trees)."""
    c = S.case(name)
    w_out, w_in = S.positional_weights(c, c.w[tag], "out"), S.positional_weights(c, c.w[tag], "in")
    assert not torch.equal(w_out, c.w[tag]) and not torch.equal(w_in, c.w[tag])
    nh, dist = S.all_pairs_lists(c, w_out)
    nh_o, dist_o = S.all_pairs(name, tag)
    assert not torch.equal(nh, nh_o) and not torch.equal(dist, dist_o)
    _fails(S.check_all_pairs, name, tag, nh, dist)
    _fails(S.check_all_pairs, name, tag, nh_o, dist)          # each table alone fails the check
    _fails(S.check_all_pairs, name, tag, nh, dist_o)
    for reverse, w_seen in ((True, w_out), (False, w_in)):
        d, l = S.trees_of(c.ei, w_seen, c.N, reverse)
        d_ref, l_ref = S.trees(name, tag, reverse)
        assert not torch.equal(d, d_ref) and not torch.equal(l, l_ref)
        _fails(S.check_trees, name, tag, reverse, d, l_ref)
        _fails(S.check_trees, name, tag, reverse, d_ref, l)
    print(f"\nidentity edge ids {name}/{tag}: {int((nh != nh_o).sum())} next hops and {int((dist != dist_o).sum())} distances "
          f"of the all-pairs table differ")


def test_weights_in_list_position_change_nothing_on_a_torus():
    """The reason these cases exist: synth.torus_network emits a source-sorted edge list, so ``out_eid`` is the identity
    and the restricted fetch IS the correct one — on every graph the shortest-path kernels had run on."""
    c = S.torus_case()
    assert torch.equal(c.out_eid, torch.arange(c.E))
    w = c.w["ff"]
    assert torch.equal(S.positional_weights(c, w, "out"), w)
    from oracle import routing
    nh, dist = S.all_pairs_lists(c, S.positional_weights(c, w, "out"))
    nh_o, dist_o = routing.all_pairs(c.ei, w, c.N)
    assert torch.equal(nh, nh_o) and torch.equal(dist, dist_o)
    d, l = S.trees_of(c.ei, S.positional_weights(c, w, "out"), c.N, True)
    d_ref, l_ref = S.trees_of(c.ei, w, c.N, True)
    assert torch.equal(d, d_ref) and torch.equal(l, l_ref)


# ---- truncated lists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES)
def test_lists_cut_after_four_entries_would_be_noticed(name, tag):
    c = S.case(name)
    w = c.w[tag]
    nh, dist = S.all_pairs_lists(c, w, cut=True)                 # k_apsp's relaxation loop
    assert not torch.equal(dist, S.all_pairs(name, tag)[1])
    _fails(S.check_all_pairs, name, tag, nh, dist)
    changed = {}
    for reverse in (True, False):
        d_ref, l_ref = S.trees(name, tag, reverse)
        for kind in ("cut_pull", "cut_mark"):
            d = S.tree_distances_rounds(c, w, reverse, **{kind: True})
            changed[(reverse, kind)] = int((d != d_ref).sum())
            assert changed[(reverse, kind)] > 0, (reverse, kind)
            _fails(S.check_trees, name, tag, reverse, d, l_ref)
        # a pull confined to four entries is the correct algorithm on the graph without the other edges
        keep = (c.out_rank if reverse else c.in_rank) < 4
        ei4, w4 = S.subgraph(c, w, keep)
        assert torch.equal(S.tree_distances_rounds(c, w, reverse, cut_pull=True), S.trees_of(ei4, w4, c.N, reverse)[0])
    print(f"\ntruncated lists {name}/{tag}: distances changed {changed}")


# ---- first-four ranks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES)
def test_a_rank_lookup_among_four_out_edges_would_be_noticed(name, tag):
    c = S.case(name)
    _, nh = S.trees(name, tag, True)
    codes = S.rank_codes(c, nh)
    beyond = S.check_ranks(c, nh, codes)
    short = S.rank_codes(c, nh, first_four=True)
    affected = int(((short == S.SEL_RAW) & (codes >= 4) & (codes != S.SEL_RAW)).sum())
    assert affected == beyond > 0
    _fails(S.check_ranks, c, nh, short)
    print(f"\nranks {name}/{tag}: the next hop sits at out-rank >= 4 on {beyond} of {c.N * c.N} (road, destination) pairs")


# ---- tie rules -------------------------------------------------------------------------------------------------------------
def test_the_two_tie_rules_differ_on_mixed_r5():
    """networkx's heap order (k_apsp) against (distance, hops, smallest id) (the trees), all 80 destinations of MIXED with
    the rounded weights: at least 100 (road, destination) pairs on which the two pick different next hops, so neither
    kernel passes with the other's rule. On HUB126 the two rules agree on every pair (nearly every shortest path there runs
    through the one hub); the count is printed, and the tie discrimination rests on MIXED."""
    nh_nx, dist_nx = S.all_pairs("MIXED", "r5")
    d_tree, nh_tree = S.trees("MIXED", "r5", True)
    assert torch.equal(d_tree.t().to(torch.float32), dist_nx)             # the same distances: only the ties differ
    differ = int((nh_tree.t().to(torch.int64) != nh_nx).sum())
    assert differ >= 100, differ
    _fails(S.check_all_pairs, "MIXED", "r5", nh_tree.t().to(torch.int64), dist_nx)
    _fails(S.check_trees, "MIXED", "r5", True, d_tree, nh_nx.t().to(torch.int32))
    hub = int((S.trees("HUB126", "r5", True)[1].t().to(torch.int64) != S.all_pairs("HUB126", "r5")[0]).sum())
    untied = int((S.trees("MIXED", "ff", True)[1].t().to(torch.int64) != S.all_pairs("MIXED", "ff")[0]).sum())
    print(f"\ntie rules: MIXED/r5 {differ} pairs differ, MIXED/ff {untied}, HUB126/r5 {hub}")
