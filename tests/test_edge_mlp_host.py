"""CPU: pins tests/edge_mlp_restatement.py (the float64 reference of test_gpu_edge_mlp_bwd.py) to what the project already
trusts — float64 autograd of oracle/nets.edge_mlp_logits and the reference's golden —, checks that the emulation of the
backward's work partition (the grid and ranges of ``emr_walk``, the flat index, ``k_nt_dot``'s split ranges and stride passes)
reproduces the facts the case list is built on, so that a change of EMR_WAVES, ND_SPLIT, ND_T or the grid rule fails here
first, and checks that every GPU case is sensitive: each unit of work the kernel could lose or misplace moves every gradient
it can reach by at least 10x the tolerance the GPU test applies to it (all of it computable without a GPU).

Which gradient a unit can reach. A lost record adds nothing to any sum: all six gradients move (modelled as the sums without
those rows). A record computed from the wrong observation, or stored onto another edge's index, keeps that index's
grad_logits, and gb3 = sum(grad_logits) is read from the caller's tensor, never from the scratch: such a unit reaches five
gradients, gb3 is named as out of its reach. A single lost edge is not visible in a sum over L >= 40 000 edges; the one-hot
probes of the GPU test are for that, and their sensitivity is shown here."""
import pytest
import torch

import edge_mlp_restatement as R
from conftest import load_golden
from oracle import nets

D = torch.float64
FACTOR = 10.0
IDS = [R.case_id(c) for c in R.BWD_CASES]
CROSSING = "a range's chunks after a sample crossing read the previous sample's observation"
TAIL_LANE = "a tail lane stored onto l = m E + 0"
GB3_OUT_OF_REACH = (CROSSING, TAIL_LANE)


def _close(a, b, tol=1e-12):
    a, b = a.detach().to(D), b.detach().to(D)
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- the restatement against autograd and the golden ------------------------------------------------------------------------
@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_manual_backward_equals_float64_autograd(E, M):
    c = R.case(E, M)
    ws = [w.double().requires_grad_(True) for w in c.weights]
    logits = nets.edge_mlp_logits(c.obs.double(), c.edge_index, c.edge_attr.double().expand(M, -1, -1), *ws)
    (logits * c.grad_logits.double()).sum().backward()
    _close(c.logits64, logits)
    for name, got, w, shape in zip(R.GRAD_NAMES, c.grads64, ws, R.GRAD_SHAPES):
        assert got.dtype == D and got.shape == shape, name
        assert float(w.grad.abs().max()) > 0, name
        _close(got, w.grad.reshape(shape))


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_no_relu_layer_is_all_dead_and_the_one_hot_gradient_is_the_full_one_on_one_edge(E, M):
    c = R.case(E, M)
    rec = c.records(torch.arange(min(c.L, 4096)))
    assert bool((rec.h1 > 0).any()) and bool((rec.h2 > 0).any())
    assert bool((rec.d1 != 0).any()) and bool((rec.d2 != 0).any())
    if c.L > 1:
        assert bool((rec.h1 == 0).any()) and bool((rec.h2 == 0).any())          # and the masks mask something
    m, e = M - 1, E // 2
    onehot = torch.zeros((M, E))
    onehot[m, e] = 1.0
    for a, b in zip(c.single(m, e), R.backward64(c.obs, c.edge_index, c.edge_attr, c.weights, onehot)):
        _close(a, b)


@pytest.mark.parametrize("tag", ["ref", "biased"])
def test_backward_meets_the_golden(tag):
    """The golden's inputs and weights: the gradients the reference's module computed in fp32, at the tolerance
    test_gpu_edge_mlp.py holds the kernel to (1e-4 of each tensor's scale)."""
    g = load_golden("edge_mlp")
    obs = torch.cat((g["node_features"], g["agent_features"][g["agent_index"]]), dim=-1)
    ws = [g[f"{tag}__{k}"] for k in ("0__weight", "0__bias", "2__weight", "2__bias", "4__weight", "4__bias")]
    _close(R.logits64(obs, g["edge_index"], g["edge_attr"], ws), g[f"{tag}__logits"], R.TOL)
    got = R.backward64(obs, g["edge_index"], g["edge_attr"], ws, g["coef"])
    for gr, name in zip(got, ("0__weight", "0__bias", "2__weight", "2__bias", "4__weight", "4__bias")):
        want = g[f"{tag}__grad__{name}"]
        assert float(want.abs().max()) > 0
        _close(gr.reshape(-1), want.reshape(-1), R.TOL)


# ---- the emulation reproduces the facts the case list is built on --------------------------------------------------------------
def test_the_kernel_constants_are_the_ones_emulated():
    """The four numbers the facts below follow from, read from the source: a change there must come here too."""
    import os
    import re
    from conftest import PKG
    src = open(os.path.join(PKG, "csrc", "edge_mlp.hip")).read()
    assert int(re.search(r"#define EMR_WAVES (\d+)", src).group(1)) == R.EMR_WAVES
    assert int(re.search(r"#define ND_SPLIT (\d+)", src).group(1)) == R.ND_SPLIT
    assert int(re.search(r"#define ND_T (\d+)", src).group(1)) == R.ND_T
    bwd = src[src.index('extern "C" int tarl_policy_edge_mlp_bwd('):]
    rule = re.search(r"blocks = ceil_div\(chunks, \(int64_t\)EMR_WAVES \* (\d+)\);\s*if \(blocks > (\d+)\) blocks = (\d+);", bwd)
    assert rule and [int(v) for v in rule.groups()] == [R.CHUNKS_PER_WAVE, R.MAX_BLOCKS, R.MAX_BLOCKS]
    assert R.SCRATCH_ROWS == 225


def test_case_list_reaches_what_it_says():
    w = {c: R.case(*c).walk for c in R.BWD_CASES}
    s = {c: R.case(*c).split for c in R.BWD_CASES}
    facts = {c: (w[c].CH, w[c].total, w[c].blocks, w[c].uncapped_blocks, w[c].per, len(w[c].active), w[c].idle, s[c].span)
             for c in R.BWD_CASES}
    #                  CH  chunks  grid uncapped per active idle  span
    assert facts == {(1, 1): (1, 1, 1, 1, 1, 1, 3, 1),
                     (32, 3): (1, 3, 1, 1, 1, 3, 1, 2),
                     (33, 7): (2, 14, 1, 1, 4, 4, 0, 4),
                     (185, 5): (6, 30, 2, 2, 4, 8, 0, 15),
                     (1, 4097): (1, 4097, 256, 257, 5, 820, 204, 65),
                     (400, 100): (13, 1300, 82, 82, 4, 325, 3, 625),
                     (185, 700): (6, 4200, 256, 263, 5, 840, 184, 2024)}
    # the grid is capped exactly in the two capped cases
    assert [c for c in R.BWD_CASES if w[c].uncapped_blocks > w[c].blocks] == [(1, 4097), (185, 700)]
    # a second stride pass exactly where stated
    passes = {c: s[c].pass_sizes(0) for c in R.BWD_CASES}
    assert [c for c in R.BWD_CASES if len(passes[c]) >= 2] == [(400, 100), (185, 700)]
    assert passes[(400, 100)] == [256, 256, 113] and passes[(185, 700)] == [256] * 7 + [232]
    assert len(s[(1, 1)].nonempty()) == 1 and all(len(s[c].nonempty()) >= 48 for c in R.BWD_CASES[1:])
    assert R.SCRATCH_ROWS * 4 * R.case(185, 700).L == 116_550_000                 # 117 MB
    # tail lanes: none at E = 32, ONE live lane at E = 33
    assert len(w[(32, 3)].lanes(0)) == 32 and len(w[(33, 7)].lanes(1)) == 1 and len(w[(185, 5)].lanes(5)) == 25
    # partial last waves, ranges that start mid-sample, ranges that cross a sample
    assert {c: w[c].partial_last_wave() for c in R.BWD_CASES} == {(1, 1): None, (32, 3): None, (33, 7): 3, (185, 5): 7,
                                                                  (1, 4097): 819, (400, 100): None, (185, 700): None}
    assert w[(33, 7)].ranges[3] == (12, 14) and w[(1, 4097)].ranges[819] == (4095, 4097)
    assert {c: (len(w[c].mid_sample_starts()), len(w[c].crossings())) for c in R.BWD_CASES} == {
        (1, 1): (0, 0), (32, 3): (0, 0), (33, 7): (0, 3), (185, 5): (5, 2), (1, 4097): (0, 3277), (400, 100): (300, 75),
        (185, 700): (700, 560)}
    # (185, 5): the eight ranges by the samples they touch; (1, 4097): every full range spans five samples
    touched = [sorted({w[(185, 5)].m[g] for g in range(*w[(185, 5)].ranges[gw])}) for gw in range(8)]
    assert touched == [[0], [0, 1], [1], [2], [2, 3], [3], [4], [4]]
    assert all(len({w[(1, 4097)].m[g] for g in range(*w[(1, 4097)].ranges[gw])}) == 5 for gw in range(819))
    # a capped range that starts mid-sample AND crosses: (185, 700)
    both = [gw for gw in w[(185, 700)].mid_sample_starts() if gw in {x for x, _ in w[(185, 700)].crossings()}]
    assert len(both) == 560
    # the irregular case's edge list is in no order
    ei = R.case(400, 100).edge_index
    assert not bool((ei[0][1:] >= ei[0][:-1]).all()) and not bool((ei[1][1:] >= ei[1][:-1]).all())


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_every_chunk_and_every_element_has_exactly_one_owner(E, M):
    c = R.case(E, M)
    w, s = c.walk, c.split
    assert all(len(o) == 1 for o in w.owner)                                        # every chunk: one wave
    assert all((w.m[g], w.c[g]) == divmod(g, w.CH) for g in range(w.total))         # the carried (m, c) is the chunk's own
    flat = [l for g in range(w.total) for l in w.flat(g)]
    assert flat == list(range(c.L))                                                 # live lanes: every l once, in order
    owners = s.owners()
    assert all(len(o) == 1 for o in owners)                                         # every l: one (range, pass, thread)
    step = max(1, c.L // 997)
    assert all(owners[l][0] == s.where(l) for l in list(range(0, c.L, step)) + [c.L - 1])
    assert sum(sum(s.pass_sizes(z)) for z in range(R.ND_SPLIT)) == c.L


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
ABSENT = {
    (1, 1): {"the partial last wave", "after the first stride pass of one range", CROSSING, TAIL_LANE},
    (32, 3): {"the partial last wave", "the tail chunk of one sample", "after the first stride pass of one range", CROSSING,
              TAIL_LANE},
    (33, 7): {"after the first stride pass of one range"},
    (185, 5): {"after the first stride pass of one range"},
    (1, 4097): {"after the first stride pass of one range", TAIL_LANE},
    (400, 100): {"the partial last wave"},
    (185, 700): {"the partial last wave"},
}
UNITS = ("one wave's whole range", "the partial last wave", "the tail chunk of one sample", "one split range",
         "after the first stride pass of one range", CROSSING, TAIL_LANE)


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_cases_notice_every_unit_the_kernel_could_lose_or_misplace(E, M):
    c = R.case(E, M)
    units = c.units()
    assert tuple(units) == UNITS
    assert {name for name, u in units.items() if u is None} == ABSENT[(E, M)]        # skipped by name, never silently
    bound = c.bounds()
    for name, unit in units.items():
        if unit is None:
            continue
        assert len(unit[0]) > 0, name
        moved = c.moved(unit)
        for i, gname in enumerate(R.GRAD_NAMES):
            if gname == "gb3" and name in GB3_OUT_OF_REACH:
                assert moved[i] == 0.0
                continue
            assert moved[i] >= FACTOR * bound[i], (name, gname, moved[i], bound[i], moved[i] / bound[i])
    # reduce overwriting instead of adding: the result minus G0 is then short of G0
    for gname, g0, b in zip(R.GRAD_NAMES, c.G0, bound):
        assert float(g0.abs().min()) >= 4.0 and float(g0.abs().max()) >= FACTOR * b, (gname, b)


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_probes_sit_where_the_emulation_says_and_a_dropped_edge_would_show(E, M):
    c = R.case(E, M)
    w, s = c.walk, c.split
    probes = c.probes()
    assert 1 <= len(probes) <= 12 and len(set(probes.values())) == len(probes)
    for what, (m, e) in probes.items():
        assert 0 <= m < M and 0 <= e < E, what
        # a kernel that dropped this one (m, e) would return zeros where float64 gives a non-zero gradient, in all six
        for gname, g in zip(R.GRAD_NAMES, c.single(m, e)):
            assert float(g.abs().max()) > 0 and bool(torch.isfinite(g).all()), (what, gname)
    chunk = lambda m, e: m * w.CH + e // R.LANES
    flat = lambda m, e: m * E + e
    if "last live lane of a tail chunk" in probes:
        m, e = probes["last live lane of a tail chunk"]
        assert e == E - 1 and E % R.LANES and w.lanes(chunk(m, e))[-1] == e
    if "first chunk of a range that starts mid-sample" in probes:
        g = chunk(*probes["first chunk of a range that starts mid-sample"])
        assert g in [r[0] for r in w.ranges] and w.c[g] != 0
    if "first chunk after a sample crossing" in probes:
        g = chunk(*probes["first chunk after a sample crossing"])
        assert w.c[g] == 0 and w.owner[g] == w.owner[g - 1] and w.m[g - 1] == w.m[g] - 1
    for what, zpt in (("l = span - 1", (0, (s.span - 1) // R.ND_T, (s.span - 1) % R.ND_T)), ("l = span", (1, 0, 0)),
                      ("l = 63 span", (63, 0, 0))):
        if what in probes:
            assert s.where(flat(*probes[what])) == zpt, what
    if s.span > R.ND_T:
        z, p, t = s.where(flat(*probes["256th element of a range"]))
        assert (p, t) == (0, R.ND_T - 1) and s.where(flat(*probes["257th element of a range"])) == (z, 1, 0)
    # which kinds each case has
    kinds = {"tail": "last live lane of a tail chunk" in probes, "mid": "first chunk of a range that starts mid-sample" in probes,
             "cross": "first chunk after a sample crossing" in probes, "pass2": "257th element of a range" in probes}
    assert kinds == {"tail": E % 32 != 0 and (M // 2, E - 1) not in ((0, E - 1), (M - 1, E - 1)),
                     "mid": (E, M) in ((185, 5), (400, 100), (185, 700)), "cross": (E, M) not in ((1, 1), (32, 3)),
                     "pass2": (E, M) in ((400, 100), (185, 700))}
