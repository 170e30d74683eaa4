"""CPU: what the sharp cases of test_gpu_gt_head.py / test_gpu_gt_value.py can see. For each of them and for both heads,
from the float64 and fp32 restatements alone: the inputs meet the census conditions (the attention is neither uniform nor
one-hot); every wrong variant of gt_mutants.py that is not the identity on the case's graph moves the output by at least
10 x the tolerance the GPU test applies, and a layer-0 WQ / WK / WV gradient by at least 10 x its elementwise allowance
somewhere. And the reason the sharp cases exist: on an old random case, uniform attention passes."""
import sys

import pytest
import torch

from conftest import PKG

sys.path.insert(0, PKG)
import gt_cases as H  # noqa: E402
import gt_mutants as MU  # noqa: E402

MARGIN = 10.0
HEADS = [False, True]                     # critic?
L0_ATTENTION = tuple(f"gt_layers.0.{w}.weight" for w in ("WQ", "WK", "WV"))


@pytest.fixture(scope="module")
def proof(tmp_path_factory):
    """(kind, M, weights, critic) -> the case, its references and, per variant, how far it moves the output and the
    layer-0 attention gradients (largest ratio to the elementwise allowance); computed once per case."""
    cache = {}

    def get(kind, M, weights, critic):
        key = (kind, M, weights, critic)
        if key not in cache:
            c = H.case_inputs(kind, M, weights, critic, tmp_path_factory.mktemp("g"))
            ref64, ref32, g64, g32, S = H.references(c)
            allow = {k: H.grad_allowance(k, g64, g32, S, c) for k in L0_ATTENTION}
            moved = {}
            for name in MU.NAMES:
                with MU.mutant(name):
                    out, p = H.restate(c, torch.float64)
                    (c.coef.double() * out).sum().backward()
                moved[name] = (float((out.detach() - ref64).abs().max()),
                               max(float(((p[k].grad - g64[k]).abs() / allow[k].clamp(min=1e-300)).max()) for k in L0_ATTENTION))
            cache[key] = (c, ref64, ref32, moved)
        return cache[key]
    return get


@pytest.mark.parametrize("critic", HEADS)
@pytest.mark.parametrize("kind,M", H.SHARP_CASES)
def test_sharp_inputs_keep_the_attention_between_uniform_and_one_hot(kind, M, critic, proof):
    c = proof(kind, M, "sharp", critic)[0]
    census = H.attention_census(c.sd, c.obs, c.ei, c.pe, critic, edge_attr=c.ea)
    print(kind, M, "critic" if critic else "policy", census)
    assert [f["layer"] for f in census] == ([0, 1] if critic else [0])
    H.check_census(census, critic)


@pytest.mark.parametrize("critic", HEADS)
@pytest.mark.parametrize("kind,M", H.SHARP_CASES)
def test_every_wrong_attention_is_ten_tolerances_away(kind, M, critic, proof):
    c, ref64, ref32, moved = proof(kind, M, "sharp", critic)
    tol = H.sharp_tolerance(ref64, ref32)
    required = [n for n in MU.REQUIRED if not MU.is_identity(n, c.ei, c.N)]
    assert "uniform" in required and "reversed" in required
    if kind in H.IRREGULAR_MAX_DEGREE:
        assert required == list(MU.REQUIRED)
    print(f"{kind} M={M} {'critic' if critic else 'policy'}: tolerance {tol:.3g} "
          f"(16 x fp32 distance {16 * float((ref32 - ref64).abs().max()):.3g}); moved by / tolerance, worst gradient / allowance:")
    for name in MU.NAMES:
        out, grad = moved[name]
        print(f"  {name:14s} {out / tol:10.3g} {grad:10.3g}{'' if name in required else '   (not required)'}")
    for name in required:
        out, grad = moved[name]
        assert out >= MARGIN * tol, (name, out, tol)
        assert grad >= MARGIN, (name, grad)


@pytest.mark.parametrize("critic", HEADS)
def test_an_old_random_case_cannot_see_uniform_attention(critic, proof):
    """("torus8", 1, "random"): the scores are so small that ignoring them moves the output by less than the tolerance that
    case applies (1e-4 of its scale) — a kernel with wrong scores, maxima or denominators passes it."""
    c, ref64, _, moved = proof("torus8", 1, "random", critic)
    assert moved["uniform"][0] < 1e-4 * max(float(ref64.abs().max()), 1.0), moved["uniform"]
    assert MU.is_identity("tail4", c.ei, c.N) and MU.is_identity("k_by_position", c.ei, c.N)
    assert moved["tail4"] == (0.0, 0.0) and moved["k_by_position"] == (0.0, 0.0)


def test_variants_leave_the_restatement_as_it_was():
    import gt_restatement as R
    for name in MU.NAMES:
        with MU.mutant(name):
            assert (R._segment_softmax, R._gather_k) != (MU._TRUE_SOFTMAX, MU._TRUE_GATHER)
        assert R._segment_softmax is MU._TRUE_SOFTMAX and R._gather_k is MU._TRUE_GATHER and R._SCORES is None


def test_irregular_graphs_have_another_edge_order_with_the_same_segments():
    """The GPU tests' second edge order of MIXED: not the identity, every node's in- and out-edges in their old order."""
    ei = H._graph("MIXED", None)[0]
    order = H.order_preserving_shuffle(ei, seed=1)
    assert sorted(order.tolist()) == list(range(ei.size(1))) and int((order != torch.arange(ei.size(1))).sum()) > ei.size(1) // 2
    mx_in, mx_out, in0, out0, src_sorted = H.graph_facts(ei, 80)
    assert (mx_in, mx_out) == (9, 9) and in0 > 0 and out0 > 0 and not src_sorted
