"""GPU: tarl_policy_edge_mlp_bwd (csrc/edge_mlp.hip: k_edge_mlp_bwd_edges -> k_nt_dot -> k_nt_reduce) at every launch shape of
tests/edge_mlp_restatement.py's ``BWD_CASES`` — one edge, full and ragged chunks, wave ranges that start mid-sample and cross
samples, the capped grid, two to eight stride passes of the split reduction — against the float64 backward written out by hand
there (pinned to float64 autograd and the golden by test_edge_mlp_host.py, which also shows that every case notices each unit
of work the kernel could lose by 10x the tolerance used here).

Every call gets a caller-owned scratch filled with NaN immediately before it: an element the reduction reads and stage 1 never
wrote poisons a gradient (a scratch from the allocator hands a second call of one shape the first call's values back). The
gradient buffers start from a non-zero G0: the kernels accumulate. Tolerance: 1e-4 * max(1, scale) per tensor, what
test_gpu_edge_mlp.py applies to this kernel; the one-hot probes 1e-4 of the single-edge gradient's own scale. Each test prints
its largest err / scale per tensor before it asserts."""
import pytest
import torch

import edge_mlp_restatement as R

pytestmark = pytest.mark.gpu
IDS = [R.case_id(c) for c in R.BWD_CASES]
NAN = float("nan")


class Dev:
    """One case's inputs on the device."""

    def __init__(self, c):
        from tarl_hip import ops
        self.c = c
        self.plan = ops.Plan(c.edge_index, c.N)
        self.ec = ops.EdgeConst(c.edge_attr, "cuda")
        self.w = ops.EdgeMlpWeights(*[t.cuda() for t in c.weights])
        self.obs = c.obs.cuda()
        self.need = ops.edge_mlp_bwd_scratch_floats(self.plan, c.M)
        assert self.need == R.SCRATCH_ROWS * c.L + R.ND_SPLIT * R.H1 * R.H1

    def bwd(self, grad_logits, grads, scratch):
        from tarl_hip import ops
        scratch.fill_(NAN)
        ops.policy_edge_mlp_bwd(self.plan, self.obs, self.ec, self.w, grad_logits, grads, scratch=scratch)
        return grads


def dev(E, M):
    return Dev(R.case(E, M))               # (the case and its float64 reference are cached; the upload is a few MB at most)


def _shaped(grads):
    return [g.detach().cpu().double().reshape(s) for g, s in zip(grads, R.GRAD_SHAPES)]


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_full_gradient_accumulates_onto_g0_from_a_nan_scratch(E, M):
    """result - G0 == the float64 gradient; and the accumulate contract with the sum's determinism, bit for bit: with s what a
    call adds to zeroed buffers, the call on G0 returns fl(G0 + s) and a second call on that result fl(fl(G0 + s) + s) — both
    calls added the same bits, each from a scratch that held nothing but NaN."""
    d = dev(E, M)
    c = d.c
    scratch = torch.empty(d.need, device="cuda")
    gl = c.grad_logits.cuda()
    s = d.bwd(gl, [torch.zeros(sh, device="cuda") for sh in R.GRAD_SHAPES], scratch)
    g0 = [t.cuda() for t in c.G0]
    r1 = d.bwd(gl, [t.clone() for t in g0], scratch)
    r2 = d.bwd(gl, [t.clone() for t in r1], scratch)
    worst = []
    for name, got, start, want in zip(R.GRAD_NAMES, _shaped(r1), c.G0, c.grads64):
        scale = max(1.0, float(want.abs().max()))
        err = float((got - start.double() - want).abs().max())
        worst.append((name, err / scale))
    print(f"\nedge_mlp_bwd {R.case_id((E, M))} err/scale: " + " ".join(f"{n}={v:.2e}" for n, v in worst))
    for t in list(s) + list(r1) + list(r2):
        assert bool(torch.isfinite(t).all())
    for name, v in worst:
        assert v <= R.TOL, (name, v)
    for name, a, b, inc, start in zip(R.GRAD_NAMES, r1, r2, s, g0):
        assert torch.equal(a, start + inc), name
        assert torch.equal(b, a + inc), name
        assert float(inc.abs().max()) > 0, name


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_one_hot_probes_return_the_single_edge_gradient(E, M):
    """grad_logits zero except a single 1.0 at (m, e), at the positions the emulation names (corners, the last live lane of a
    tail chunk, the first chunk of a range that starts mid-sample, the first chunk after a sample crossing, the edges of the
    split ranges, the 256th / 257th element of a range): all six gradients are that edge's float64 gradient and finite. A sum
    over L >= 40 000 edges would not show ONE lost or misplaced edge; this does. The scratch is allocated once and refilled."""
    d = dev(E, M)
    c = d.c
    scratch = torch.empty(d.need, device="cuda")
    gl = torch.zeros((M, E), device="cuda")
    worst = 0.0
    fails = []
    for what, (m, e) in c.probes().items():
        gl[m, e] = 1.0
        got = _shaped(d.bwd(gl, [torch.zeros(sh, device="cuda") for sh in R.GRAD_SHAPES], scratch))
        gl[m, e] = 0.0
        for name, a, want in zip(R.GRAD_NAMES, got, c.single(m, e)):
            scale = float(want.abs().max())
            assert scale > 0
            err = float((a - want).abs().max()) if bool(torch.isfinite(a).all()) else float("inf")
            worst = max(worst, err / scale)
            if not err <= R.TOL * scale:
                fails.append((what, (m, e), name, err, scale))
    print(f"\nedge_mlp_bwd probes {R.case_id((E, M))}: {len(c.probes())} probes, worst err/scale {worst:.2e}")
    assert not fails, fails


@pytest.mark.parametrize("E,M", R.BWD_CASES, ids=IDS)
def test_fp32_forward_of_the_same_case(E, M):
    """The forward twin: fp32 MFMA logits into a NaN-prefilled ``out`` against float64 within 1e-5 of the logits' scale (the
    contract of test_edge_mlp_chunk_walk_edge_cases_all_precisions, at shapes that test does not have: the capped grid with
    several chunks per sample, E = 32)."""
    from tarl_hip import ops
    d = dev(E, M)
    c = d.c
    out = torch.full((M, E), NAN, device="cuda")
    ops.policy_edge_mlp(d.plan, d.obs, d.ec, d.w, precision="fp32", out=out)
    ref = c.logits64
    scale = float(ref.abs().max())
    err = float((out.cpu().double() - ref).abs().max())
    print(f"\nedge_mlp fwd fp32 {R.case_id((E, M))}: err/scale {err / scale:.2e}")
    assert err <= R.FWD_TOL * scale, (err, scale)           # (a NaN left in `out` = a chunk nobody wrote)


def test_scratch_keyword_refuses_what_the_kernel_cannot_use():
    from tarl_hip import ops
    d = dev(33, 7)
    c = d.c
    gl = c.grad_logits.cuda()
    zeros = lambda: [torch.zeros(sh, device="cuda") for sh in R.GRAD_SHAPES]
    for bad in (torch.empty(d.need - 1, device="cuda"), torch.empty(d.need, device="cuda", dtype=torch.float64),
                torch.empty(2 * d.need, device="cuda")[::2], torch.empty(d.need)):
        with pytest.raises(ValueError):
            ops.policy_edge_mlp_bwd(d.plan, d.obs, d.ec, d.w, gl, zeros(), scratch=bad)
    # None: allocated per call, as before; a larger caller-owned buffer is fine — the same bits either way
    a = zeros()
    ops.policy_edge_mlp_bwd(d.plan, d.obs, d.ec, d.w, gl, a)
    b = d.bwd(gl, zeros(), torch.empty(d.need + 1000, device="cuda"))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
