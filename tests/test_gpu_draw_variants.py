"""GPU: every launch shape of the rollout's action draw (tarl_graphdist_rollout: twelve register-resident instantiations
k_graphdist_rollout_reg<J, D, SORTED> and the generic kernel with more than one 1 024-group chunk), each against

  * the oracle, integers exact: oracle.dist.GraphDist on the device's probabilities and the same uniforms (host uniforms,
    device Philox noise read back through tarl_noise_export, and uniforms placed on the thresholds) — edge ids, rank bytes
    and SELECTED_ROAD bytes; the graph with nodes without out-edges, outside the oracle's domain, against the per-node
    restatement of the same lines that test_update_host.py pins to the oracle;
  * the three-launch chain softmax -> sample -> apply_choice -> log_prob, bits exact;
  * TARL_GRAPHDIST_REG=0 (the generic kernel on the register cases), bits exact;
  * the float64 log-prob of tests/update_restatement.py, within max(8 e32, 2^-22 scale), never above the existing test's
    2e-2 absolute / 1e-5 relative.

Every case first asserts, from the plan, the numbers that decide the dispatch."""
import ctypes
import math

import pytest
import torch

import update_restatement as R
from oracle import dist

pytestmark = pytest.mark.gpu
SEED, COUNTER = 5, 17


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


_CASES = {}


def _case(ops, name):
    """Plan, inputs, the device's probabilities and the float64 distribution of a case: built once per module."""
    if name not in _CASES:
        ei, N, logits, u, prev = R.draw_inputs(name)
        plan = ops.Plan(ei, N)
        p = ops.graphdist_softmax(plan, logits.cuda(), R.DRAW_T)
        _CASES[name] = dict(ei=ei, N=N, logits=logits, u=u, prev=prev, plan=plan, po=R.PlanOrder(ei, N), p=p, p_cpu=p.cpu(),
                            d64=R.segment_dist(logits.double(), ei, R.DRAW_T, N))
    return _CASES[name]


def _assert_dispatch(name, plan):
    N, D, srt, holes, kernel = R.DRAW_CASES[name]
    assert plan.num_nodes == N and plan.max_out == D and plan.src_sorted == srt
    assert (plan.num_groups == N) == (not holes)
    assert R.draw_dispatch(plan.num_nodes, plan.num_groups, plan.max_out, plan.src_sorted) == kernel
    if kernel == "generic":
        assert plan.num_groups > 1024                  # more than one chunk: the cross-chunk running sum is exercised


def _oracle_pick(c, b, u_b):
    """(choice (N,), rank (N,)) of environment b from the oracle on the device's probabilities."""
    if c["po"].G == c["N"]:
        d = dist.GraphDist(c["logits"][b], c["ei"], R.DRAW_T, proba=c["p_cpu"][b])
        return R.choice_from_onehot(d.sample(u_b), c["po"])
    return R.sample_choice(c["p_cpu"][b], c["po"], u_b)


def _thresholds(c, b):
    """The oracle's own rebased cumulative sums (sorted order) of environment b."""
    if c["po"].G == c["N"]:
        return dist.GraphDist(c["logits"][b], c["ei"], R.DRAW_T, proba=c["p_cpu"][b]).cumsum
    return R.rebased_cumsum(c["p_cpu"][b], c["po"])


def _uniforms(ops, c, noise):
    """(uniform argument of the launch or None, the same numbers on the host (B, G))."""
    if noise == "device":
        return None, ops.noise_export(c["plan"], "uniform", SEED, COUNTER, range(R.DRAW_B)).cpu()
    u = c["u"].clone()
    if noise == "edges":
        po = c["po"]
        u[:, ::5] = 0.0                      # the first edge with a positive rebased cumulative sum
        u[:, ::7] = 0.99999994               # the largest fp32 below 1: may be beyond a rounded-down cumulative sum
        for b in range(R.DRAW_B):            # exactly on the first threshold: the comparison is strict
            u[b, ::11] = _thresholds(c, b)[po.start[po.nodes[::11]]]
    return u.cuda(), u


def _one_launch(ops, c, uniform):
    B, N = R.DRAW_B, c["N"]
    ch = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    c8 = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    sel = c["prev"].cuda()
    lp = ops.graphdist_rollout(c["plan"], c["logits"].cuda(), R.DRAW_T, uniform=uniform, seed=SEED, counter=COUNTER, choice=ch,
                               choice8=c8, sel8=sel)
    return ch, c8, sel, lp


@pytest.mark.parametrize("noise", ["host", "device", "edges"])
@pytest.mark.parametrize("name", list(R.DRAW_CASES))
def test_draw_variant(ops, monkeypatch, name, noise):
    c = _case(ops, name)
    plan, N, B, po = c["plan"], c["N"], R.DRAW_B, c["po"]
    _assert_dispatch(name, plan)
    uniform, u_host = _uniforms(ops, c, noise)
    monkeypatch.delenv("TARL_GRAPHDIST_REG", raising=False)
    ch, c8, sel, lp = _one_launch(ops, c, uniform)

    # the oracle decides: edge ids, rank bytes (0x80 | previous rank where nothing was drawn), their transpose
    picks = [_oracle_pick(c, b, u_host[b]) for b in range(B)]
    ch_ref = torch.stack([p[0] for p in picks])
    rank_ref = torch.stack([p[1] for p in picks])
    assert torch.equal(ch.cpu().long(), ch_ref)
    c8_ref = torch.where(ch_ref >= 0, rank_ref, 0x80 | (c["prev"].t().long() & 0x7F)).to(torch.uint8)
    if po.G != N:                            # a node without out-edges draws nothing either
        assert bool((ch_ref[:, po.deg == 0] == -1).all())
    assert torch.equal(c8.cpu(), c8_ref)
    assert torch.equal(sel.cpu(), c8_ref.t())
    drew_nothing = bool((ch_ref[:, po.deg > 0] < 0).any())
    if noise == "edges":
        assert drew_nothing                  # (a degree-1 node whose u sits on its only threshold)
        assert bool(((c8.cpu() & 0x80) != 0).any())

    # the chain, bits exact
    _, ch_chain = ops.graphdist_sample(plan, c["p"], uniform=uniform, seed=SEED, counter=COUNTER, want_onehot=False,
                                       want_choice=True)
    lp_chain, _ = ops.graphdist_logprob_entropy(plan, c["p"], choice=ch_chain, want_entropy=False)
    sel_chain = c["prev"].cuda()
    from tarl_hip import lib as _lib
    f = _lib.FusedStruct()                   # tarl_fused_apply_choice only touches sel8: drive it through its C entry
    f.sel8 = sel_chain.data_ptr()
    _lib.check(_lib.load().tarl_fused_apply_choice(plan.handle, ctypes.byref(f), B, ch_chain.data_ptr(), _lib.current_stream()))
    assert torch.equal(ch, ch_chain) and torch.equal(lp, lp_chain)
    assert torch.equal(sel, sel_chain) and torch.equal(c8, sel_chain.t())

    # the knob: the generic kernel on the same inputs gives the same bits
    if R.DRAW_CASES[name][4] != "generic":
        monkeypatch.setenv("TARL_GRAPHDIST_REG", "0")
        ch0, c80, sel0, lp0 = _one_launch(ops, c, uniform)
        monkeypatch.delenv("TARL_GRAPHDIST_REG")
        assert torch.equal(ch0, ch) and torch.equal(c80, c8) and torch.equal(sel0, sel) and torch.equal(lp0, lp)

    # log-prob against float64 on the same (fp32) logits and the same action
    ref = c["d64"].log_prob(ch_ref)
    lp_cpu = lp.cpu().double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lp_cpu), fin) and bool((lp_cpu[~fin] == -math.inf).all())
    if po.G == N:
        lp32 = torch.stack([dist.GraphDist(c["logits"][b], c["ei"], R.DRAW_T).log_prob(c["d64"].onehot(ch_ref[b]))
                            for b in range(B)]).double()
    else:
        lp32 = R.segment_dist(c["logits"], c["ei"], R.DRAW_T, N).log_prob(ch_ref).double()
    if fin.any():
        e32 = R.max_err(lp32[fin], ref[fin])
        bound = min(R.tensor_bound(e32, ref[fin]), 2e-2, 1e-5 * float(ref[fin].abs().min()))
        err = R.max_err(lp_cpu[fin], ref[fin])
        print(f"DRAW {name:7s} {noise:6s} lp: e32 {e32:.3e} bound {bound:.3e} gpu {err:.3e}")
        assert err <= bound
    else:
        print(f"DRAW {name:7s} {noise:6s} lp: -inf in every environment (u on the only threshold of a degree-1 node)")
    if noise != "edges":
        assert bool(fin.all()) or drew_nothing


def test_rank_byte_guard(ops):
    """A node with 127 out-edges has no rank byte (bit 7 is SEL_CARRIED): the call that asks for rank bytes is refused
    before any launch, with tarl_graphdist_mode_rollout's words; the int32 edge ids alone have no such limit."""
    from tarl_hip import lib as _lib
    ei, N = R.star_graph(127)
    assert N == 130
    plan = ops.Plan(ei, N)
    assert plan.max_out == 127 and plan.num_groups == N
    gen = torch.Generator().manual_seed(3)
    B = 2
    logits = torch.randn((B, ei.size(1)), generator=gen) * 3
    u = torch.rand((B, N), generator=gen)
    for kw in (dict(choice8=torch.zeros((B, N), dtype=torch.uint8, device="cuda")),
               dict(sel8=torch.zeros((N, B), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(_lib.TarlError, match="out-degree above 126 has no rank byte"):
            ops.graphdist_rollout(plan, logits.cuda(), R.DRAW_T, uniform=u.cuda(), **kw)
        assert int(next(iter(kw.values())).sum()) == 0
    ch = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    lp = ops.graphdist_rollout(plan, logits.cuda(), R.DRAW_T, uniform=u.cuda(), choice=ch)
    p = ops.graphdist_softmax(plan, logits.cuda(), R.DRAW_T).cpu()
    po = R.PlanOrder(ei, N)
    for b in range(B):
        want, _ = R.choice_from_onehot(dist.GraphDist(logits[b], ei, R.DRAW_T, proba=p[b]).sample(u[b]), po)
        assert torch.equal(ch[b].cpu().long(), want)
    assert bool(torch.isfinite(lp).all())
    # a hub of 126 still has its rank byte
    ei2, N2 = R.star_graph(126)
    plan2 = ops.Plan(ei2, N2)
    c8 = torch.zeros((1, N2), dtype=torch.uint8, device="cuda")
    u2 = torch.full((1, N2), 0.99, device="cuda")
    flat = torch.zeros((1, ei2.size(1)), device="cuda")
    ops.graphdist_rollout(plan2, flat, 1.0, uniform=u2, choice8=c8)
    assert int(c8[0, 0]) == 124              # uniform hub: the first k with 0.99 < fl((k + 1) / 126) is k = 124
