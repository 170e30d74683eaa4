"""CPU: the exact draw checks of tests/draw_check.py (used by the oracle replays of the live-policy rollouts) on the
GraphDistribution goldens. The rank-from-thresholds replica must BE ``GraphDist.sample`` (the reference's strict
``s < cumsum`` rule, ties included) when fed the oracle's own table, and the checks must tell a one-ulp threshold rounding
from a wrong draw."""
import pytest
import torch

from conftest import load_golden
from draw_check import CARRIED, DrawCheck, code_rank, ranks
from oracle import dist

INF = float("inf")


def _setup(name):
    g = load_golden(name)
    ei = g["edge_index"]
    gd = dist.GraphDist(g["logits"], ei)
    src = ei[0]
    N = gd.nb_nodes
    ptr = torch.zeros(N + 1, dtype=torch.long)
    ptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    out_eid = torch.argsort(src, stable=True)
    return g, gd, ptr, out_eid


def _onehot(r, ptr, out_eid, E):
    """Device-style code ranks -> the one-hot action (a node with rank == degree draws nothing)."""
    deg = ptr[1:] - ptr[:-1]
    drew = r < deg
    a = torch.zeros(E, dtype=torch.long)
    a[out_eid[ptr[:-1][drew] + r[drew]]] = 1
    return a


def _codes(r, deg):
    return torch.where(r < deg, r, torch.full_like(r, CARRIED)).to(torch.uint8)


@pytest.mark.parametrize("name", ["dist_small", "dist_mid"])
def test_rank_replica_is_graphdist_sample_at_and_around_every_threshold(name):
    g, gd, ptr, out_eid = _setup(name)
    E, N = out_eid.numel(), gd.nb_nodes
    deg = ptr[1:] - ptr[:-1]
    cs = gd.cumsum
    cases = [g[f"u{k}"] for k in range(4)]
    for q in range(int(deg.max())):
        k = ptr[:-1] + torch.minimum(torch.full_like(deg, q), deg - 1)
        at = cs[k].clone()
        cases += [at, torch.nextafter(at, torch.full_like(at, -INF)), torch.nextafter(at, torch.full_like(at, INF))]
    for u in cases:
        r = ranks(u, cs, ptr)
        assert torch.equal(_onehot(r, ptr, out_eid, E), gd.sample(u)), "rank replica != GraphDist.sample"
        chk = DrawCheck(gd, cs, ptr)
        assert chk.max_ulps == 0.0 and chk.a2_ok()
        assert chk.frame(u, _codes(r, deg)) == 0
    # u exactly AT a threshold is past it (s < cumsum is strict): the rank counts that boundary
    k0 = ptr[:-1] + 1
    u = cs[k0].clone()
    assert bool((ranks(u, cs, ptr) >= 2).all())


@pytest.mark.parametrize("name", ["dist_small", "dist_mid"])
def test_one_ulp_gap_explains_a_flip_and_nothing_else(name):
    _, gd, ptr, _ = _setup(name)
    N = gd.nb_nodes
    deg = ptr[1:] - ptr[:-1]
    cs = gd.cumsum.clone()
    i, q = N // 2, 2
    k = int(ptr[i]) + q
    thr = cs.clone()
    thr[k] = torch.nextafter(cs[k], torch.tensor(INF))             # the device rounded boundary q one ulp up
    chk = DrawCheck(gd, thr, ptr)
    assert 0 < chk.max_ulps <= 1.0 and chk.a2_ok()
    # u inside the gap [cs[k], thr[k]): the oracle counts boundary q, the device does not -> one flip, explained
    u = cs[ptr[:-1]].clone() * 0.5
    u[i] = cs[k]
    r_dev = ranks(u, thr, ptr)
    assert int(r_dev[i]) == q and int(ranks(u, cs, ptr)[i]) == q + 1
    code = _codes(r_dev, deg)
    assert chk.a1_mismatches(u, code).numel() == 0
    flipped, unexplained = chk.explain(u, code)
    assert flipped.tolist() == [i] and unexplained.numel() == 0
    assert chk.frame(u, code) == 1 and chk.report()["flipped_nodes"] == 1
    # the same gap with u OUTSIDE it (one step below both tables) and the code still claiming the flip: A1 and A3 both fail
    u_out = u.clone()
    u_out[i] = torch.nextafter(cs[k], torch.tensor(-INF))
    assert int(ranks(u_out, thr, ptr)[i]) == q == int(ranks(u_out, cs, ptr)[i])
    wrong = code.clone()
    wrong[i] = q + 1
    assert chk.a1_mismatches(u_out, wrong).tolist() == [i]
    assert chk.explain(u_out, wrong)[1].tolist() == [i]
    with pytest.raises(AssertionError, match="A1"):
        DrawCheck(gd, thr, ptr).frame(u_out, wrong)
    # a flip TWO boundaries away from the oracle's draw: only one of the two boundaries lies in a gap -> unexplained
    two = code.clone()
    two[i] = q - 1
    assert chk.explain(u, two)[1].tolist() == [i]
    assert chk.a1_mismatches(u, two).tolist() == [i]


@pytest.mark.parametrize("name", ["dist_small", "dist_mid"])
def test_draw_checks_bite(name):
    """A device table a few ulps off fails A2; a remapped code byte fails A1; a code that draws nothing where the table
    drew, or draws where the table ran out, fails A1."""
    _, gd, ptr, _ = _setup(name)
    deg = ptr[1:] - ptr[:-1]
    cs = gd.cumsum.clone()
    S = torch.cumsum(gd.proba_sort, dim=-1)
    k = int(ptr[3]) + 1
    thr = cs.clone()
    thr[k] = cs[k] + 3 * (torch.nextafter(S[k], torch.tensor(INF)) - S[k])
    assert not DrawCheck(gd, thr, ptr).a2_ok()
    u = torch.full((gd.nb_nodes,), 0.5)
    r = ranks(u, cs, ptr)
    chk = DrawCheck(gd, cs, ptr)
    code = _codes(r, deg)
    remap = code.clone()
    remap[5] = (int(r[5]) + 1) % int(deg[5])
    assert chk.a1_mismatches(u, remap).tolist() == [5]
    carried = code.clone()
    carried[7] = CARRIED | int(r[7])
    assert chk.a1_mismatches(u, carried).tolist() == [7]
    assert int(code_rank(carried, deg)[7]) == int(deg[7])
    # u past the node's last threshold: only a code with bit 7 set is right
    u2 = u.clone()
    u2[2] = torch.nextafter(cs[int(ptr[3]) - 1], torch.tensor(INF))
    r2 = ranks(u2, cs, ptr)
    assert int(r2[2]) == int(deg[2])
    c2 = _codes(r2, deg)
    assert chk.a1_mismatches(u2, c2).numel() == 0
    c2[2] = int(deg[2]) - 1
    assert chk.a1_mismatches(u2, c2).tolist() == [2]
