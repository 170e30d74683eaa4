"""GPU: the gradients and the ordered fp64 sums of the goal head and the per-decision family (csrc/goal_mlp.hip,
csrc/decision_critic.hip, csrc/decision_credit.hip) give the BITS recorded in tests/golden/decision_bits.npz. The file was
written by tools/make_decision_bits.py from the library as it stood before these kernels were rebuilt on csrc/mlp8.h and
csrc/tile_sums.h: the other GPU tests hold these outputs to float64 within a tolerance, which a reordered addition passes;
here it fails. Stored: the 161-word gradients of tarl_policy_goal_mlp_bwd and tarl_decision_critic_loss, out5 (M, 5), out4
(M, 4) with grad_logits, stats3 — fp32 words as int32, fp64 words as int64. Every gradient goes onto a non-zero starting
buffer from a NaN-filled scratch.

Inputs: the builders of test_gpu_goal_mlp.py, test_gpu_decision_critic.py and test_gpu_decision_credit.py. Cases:
  goal backward (random and sharp weights x all-pairs and per-destination tables): the torus at M = 1 (four full tiles);
    the shortest tails the builders allow — every graph of theirs has an even edge count (1 024, 400, 17 852), so
    M * E = 1 mod 256 has no solution: MIXED at M = 9 (14 tiles and a tail of 16 lanes, the shortest at a small size) and
    HUB126 at M = 15 (a tail of 4 lanes, the shortest there is); HUB126 at M = 17 (more than 1 024 tiles: a partition
    owns two).
  critic loss: torus8x8 M = 1; torus9x8 M = 3 (a nearly empty second tile); MIXED M = 3; every road live on torus8x8;
    HUB126 at M = 1027 (runs of three (row, tile) pairs that cross rows); n_live = 0.
  decision PPO: torus6x5 and torus9x8 at M = 3 (source-sorted edge lists) and MIXED at M = 3 (not source-sorted).
  decision statistics: 240 elements (one block, no second turn of the grid-stride loop) and HUB126's 1027 kept rows (more
    than 256 x 256 elements)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
NAN = float("nan")
GOAL_CASES = (("torus", 1), ("MIXED", 9), ("HUB126", 15), ("HUB126", 17))
CRITIC_CASES = ("torus8x8-M1", "torus9x8-M3", "MIXED-M3", "torus8x8-dense", "HUB126-M1027", "torus9x8-L0")
PPO_CASES = ("torus6x5", "torus9x8", "MIXED")
STATS_CASES = ("one-block", "grid-stride")


def _start(n, seed=99):
    """The non-zero buffer a gradient is accumulated onto."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32)).cuda()


def _words(out):
    ints = {torch.float32: torch.int32, torch.float64: torch.int64}
    return {k: v.detach().cpu().contiguous().view(ints[v.dtype]).reshape(-1) for k, v in out.items()}


def goal_bits(name, M):
    import test_gpu_goal_mlp as TG
    from tarl_hip import ops
    c = TG._graph_case(name)
    E = c["ei"].shape[1]
    assert M * E % 256 == {("MIXED", 9): 16, ("HUB126", 15): 4}.get((name, M), M * E % 256)
    obs = c["live"][:M].contiguous()
    obs_np = obs.cpu().numpy()
    gl = torch.from_numpy(np.random.default_rng(M).standard_normal((M, E)).astype(np.float32)).cuda()
    need = ops.goal_mlp_bwd_scratch_floats(c["plan"], M)
    assert (-(-M * E // 256) > 1024) == (name == "HUB126")
    out = {}
    for kind in ("all_pairs", "per_destination"):
        tab, slot, _, _ = TG._tables(c, obs_np, kind)
        for sharp in (False, True):
            _, w = TG._weights(31 + M, sharp)
            scratch = torch.full((need,), NAN, device="cuda")
            out[f"{kind}/{'sharp' if sharp else 'random'}"] = TG._bwd(ops, c, obs, w, tab, slot, gl, init=_start(161),
                                                                      scratch=scratch)
    return _words(out)


def _critic_case(tag):
    """-> (the case's dict, n_live)"""
    import test_gpu_decision_critic as TC
    if tag == "HUB126-M1027":
        c = TC._hub_case()
    elif tag == "torus8x8-dense":      # test_loss_on_dense_tiles' case
        c = dict(TC._inputs("torus8x8", 3, "packed"))
        head = np.full((3, c["N"]), 9, dtype=np.int32)
        adv = (np.random.default_rng(3).normal(size=head.shape) * 24.0 - 4.0).astype(np.float32)
        c.update(head=head, live=head > 0, adv=adv)
    else:
        name, m = tag.split("-")
        c = TC._inputs(name, 1 if m == "M1" else 3, "packed")
    return c, 0 if tag.endswith("L0") else int(c["live"].sum())


def critic_bits(tag):
    import decision_critic_restatement as C
    import test_gpu_decision_critic as TC
    from tarl_hip import ops
    c, L = _critic_case(tag)
    M = c["head"].shape[0]
    need = ops.decision_critic_scratch_bytes(c["plan"], M)
    scratch = torch.full(((need + 7) // 8,), NAN, dtype=torch.float64, device="cuda")
    out5, grads = TC._run_loss(ops, c, C.weights(23 + M), L, grads=_start(161), scratch=scratch)
    assert tuple(out5.shape) == (M, 5)
    return _words(dict(out5=out5, grads=grads))


def ppo_bits(name):
    import decision_credit_restatement as DC
    import test_gpu_decision_credit as TD
    from tarl_hip import ops
    M = 3
    c = TD._loss_inputs(name, M)
    plan = ops.Plan(c["net"].edge_index, c["N"])
    assert plan.src_sorted == (name != "MIXED") == bool((np.diff(c["ei"][0]) >= 0).all())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    head = dev(np.where(c["live"], 5, 0).astype(np.int32))
    n_live = torch.tensor([int(c["live"].sum())], dtype=torch.int32).cuda()
    need = ops._lib.load().tarl_graphdist_decision_ppo_scratch_bytes(plan.handle, M)
    scratch = torch.full(((need + 7) // 8,), NAN, dtype=torch.float64, device="cuda")
    g = _start(M * c["E"]).view(M, c["E"])
    out4 = ops.graphdist_decision_ppo(plan, dev(c["logits"]), dev(c["choice"]), head, dev(c["lp_old"]), dev(c["adv"]),
                                      dev(DC.decision_stats(c["adv"], c["live"])), n_live, clip_epsilon=0.2,
                                      temperature=c["T"], grad_scale=0.5, grad_logits=g, scratch=scratch)
    assert tuple(out4.shape) == (M, 4)
    return _words(dict(out4=out4, grad_logits=g))


def stats_bits(tag):
    import test_gpu_decision_credit as TD
    import test_gpu_decision_critic as TC
    from tarl_hip import ops
    if tag == "one-block":
        c = TD._loss_inputs("torus6x5", 3)
        adv, head = c["adv"][:2], np.where(c["live"][:2], 5, 0).astype(np.int32)
        assert adv.size <= 256
    else:
        c = TC._hub_case()
        adv, head = c["adv"], c["head"]
        assert adv.size > 256 * 256
    st = ops.decision_stats(torch.from_numpy(np.ascontiguousarray(adv)).cuda(), torch.from_numpy(np.ascontiguousarray(head)).cuda())
    assert float(st[2]) == int((head > 0).sum()) > 0
    return _words(dict(stats3=st))


CASES = ([(f"goal_bwd/{n}-M{M}", goal_bits, (n, M)) for n, M in GOAL_CASES] +
         [(f"critic_loss/{t}", critic_bits, (t,)) for t in CRITIC_CASES] +
         [(f"decision_ppo/{n}-M3", ppo_bits, (n,)) for n in PPO_CASES] +
         [(f"decision_stats/{t}", stats_bits, (t,)) for t in STATS_CASES])


@pytest.mark.parametrize("case,fn,args", CASES, ids=[c[0] for c in CASES])
def test_the_bits_are_the_recorded_ones(case, fn, args):
    gold = load_golden("decision_bits")
    got = fn(*args)
    assert sorted(f"{case}/{k}" for k in got) == sorted(k for k in gold if k.startswith(case + "/"))
    bad = []
    for name, bits in got.items():
        want = gold[f"{case}/{name}"]
        assert want.dtype == bits.dtype and want.shape == bits.shape, name
        floats = bits.view(torch.float32 if bits.dtype == torch.int32 else torch.float64)
        assert bool(torch.isfinite(floats).all()), name
        if not torch.equal(bits, want):
            bad.append((name, int((bits != want).sum()), bits.numel()))
    assert not bad, bad
