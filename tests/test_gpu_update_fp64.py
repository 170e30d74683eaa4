"""GPU: the PPO update arithmetic (csrc/ppo.hip, the distribution forward / backward of csrc/dist.hip, k_rollout_gather, the
uint8 row-major critic) at every launch shape — below, at and above one workgroup, one wave, the grid-stride threshold —
against the float64 restatement of tests/update_restatement.py on the fp32-rounded inputs.

Tolerances (none taken from a kernel): tensors max(8 e32, 2^-22 scale) with e32 the error of the same arithmetic in fp32 on
the CPU, capped by what the older test of the kernel allows; the six reduced loss scalars the depth bound of the reduction,
(ceil(M / 256) + 16) 2^-24 mean|term|. test_update_host.py checks that each case here would notice a lost row or wave.
Every case prints its e32, bound and observed error."""
import math

import pytest
import torch

import update_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.cuda()


def _check_tensor(what, got, ref, f32, atol_cap, rtol_cap, relative_scale=False):
    """|got - ref| <= min(max(8 e32, 2^-22 scale), atol_cap + rtol_cap |ref|) element by element."""
    ref = ref.detach().double()
    e32 = R.max_err(f32.detach(), ref)
    bound = R.tensor_bound(e32, ref, relative_scale)
    err = (got.detach().cpu().double() - ref).abs()
    print(f"UPD {what}: e32 {e32:.3e} bound {bound:.3e} gpu {float(err.max()) if err.numel() else 0.0:.3e}")
    assert bool((err <= torch.clamp(atol_cap + rtol_cap * ref.abs(), max=bound)).all()), what
    return e32, bound, float(err.max())


# ---- tarl_ppo_loss ------------------------------------------------------------------------------------------------------
NAMES6 = ("objective", "critic", "entropy", "clip_frac", "kl", "ess")


def _ppo_compare(ops, what, ins, coefs):
    M = ins[0].numel()
    lo, hi = R.clip_thresholds32(coefs.get("clip_epsilon", 0.2), device="cuda")
    ref, g_lp, g_ent, g_val, mean_abs = R.ppo_loss64(*(t.double() for t in ins), **coefs, lo=lo, hi=hi)
    _, e_lp, e_ent, e_val, _ = R.ppo_loss64(*ins, **coefs, lo=lo, hi=hi)              # the same arithmetic in fp32
    out, glp, gent, gval = ops.ppo_loss(*(dev(t) for t in ins), **coefs)
    out_ng, a, b, c = ops.ppo_loss(*(dev(t) for t in ins), **coefs, want_grads=False)
    assert a is None and b is None and c is None and torch.equal(out_ng, out)
    o = out.cpu().double()
    for i, name in enumerate(NAMES6):
        bound = R.scalar_bound(M, mean_abs[i], ess=(i == 5))
        err = abs(float(o[i] - ref[i]))
        print(f"UPD {what} {name}: ref {float(ref[i]):+.9e} bound {bound:.3e} gpu {err:.3e}")
        assert err <= bound, (name, err, bound)
    _check_tensor(f"{what} g_lp", glp, g_lp, e_lp, 1e-6, 1e-4, relative_scale=True)
    _check_tensor(f"{what} g_val", gval, g_val, e_val, 1e-6, 1e-4, relative_scale=True)
    _check_tensor(f"{what} g_ent", gent, g_ent, e_ent, 1e-7, 1e-4, relative_scale=True)
    return out, glp, gent, gval


@pytest.mark.parametrize("coefs", R.PPO_COEFS, ids=["default", "custom"])
@pytest.mark.parametrize("M", R.PPO_SIZES)
def test_ppo_loss_all_outputs_and_seeds(ops, M, coefs):
    _ppo_compare(ops, f"ppo M={M} {'custom' if coefs else 'default'}", R.ppo_inputs(M), coefs)


def test_ppo_loss_rows_on_the_clip_and_on_the_huber_knee(ops):
    """Log-ratio exactly log1p(+-eps) (inside the clip: the gradient flows, whatever the sign of the advantage) and
    |value - target| exactly 1 (the linear branch: loss 1/2, gradient the sign), in a batch of ordinary rows; expectations
    from autograd of the float64 restatement with the kernel's fp32 thresholds."""
    M = 70
    lp_new, lp_old, adv, value, target, ent = (t.clone() for t in R.ppo_inputs(M, seed=1))
    lo, hi = (torch.tensor(x, dtype=torch.float64).float() for x in R.clip_thresholds32(0.2, device="cuda"))
    rows = [3, 4, 66, 67]
    lp_old[rows] = 0.0
    lp_new[rows] = torch.stack([hi, hi, lo, lo])
    adv[rows] = torch.tensor([1.5, -1.5, 0.75, -0.75])
    value[[5, 68]] = torch.tensor([2.0, -0.25])
    target[[5, 68]] = torch.tensor([1.0, 0.75])
    out, glp, gent, gval = _ppo_compare(ops, "ppo edges", (lp_new, lp_old, adv, value, target, ent), {})
    r = torch.stack([hi, hi, lo, lo]).double().exp()
    want = -(r * adv[rows].double()) / M
    assert float((glp[rows].cpu().double() - want).abs().max()) <= 4 * R.U24 * float(want.abs().max())
    assert bool((glp[rows] != 0).all())
    assert gval[5].item() == pytest.approx(1.0 / M, rel=1e-6) and gval[68].item() == pytest.approx(-1.0 / M, rel=1e-6)


def test_ppo_loss_row_with_infinite_log_probs(ops):
    """One row with lp_new = lp_old = -inf (an impossible action under both policies; lw = nan). Asserted: every other
    row's three seeds are bit-identical to the same batch with a finite row in its place, and that row's g_lp is 0.
    Not asserted, observed in the float64 reference arithmetic (torch, CPU) for this batch: loss_objective, kl and ESS are
    nan (nan propagates through min / the sums); loss_critic and loss_entropy are finite and unchanged; the clip fraction
    counts the row as inside, since both comparisons with nan are false (k_ppo_loss tests `inside` = lw >= lo && lw <= hi,
    false for nan, and so counts it as clipped)."""
    M, row = 257, 200
    ins = [t.clone() for t in R.ppo_inputs(M, seed=2)]
    ref = [dev(t) for t in ins]
    ref[0][row], ref[1][row] = -5.0, -5.25
    bad = [t.clone() for t in ref]
    bad[0][row] = bad[1][row] = -math.inf
    _, glp_r, gent_r, gval_r = ops.ppo_loss(*ref)
    _, glp_b, gent_b, gval_b = ops.ppo_loss(*bad)
    keep = torch.arange(M, device="cuda") != row
    assert torch.equal(glp_b[keep], glp_r[keep]) and glp_b[row].item() == 0.0 and glp_r[row].item() != 0.0
    assert torch.equal(gent_b, gent_r) and torch.equal(gval_b, gval_r)
    assert bool(torch.isfinite(glp_b).all())


# ---- tarl_gae -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.GAE_T)
@pytest.mark.parametrize("B", R.GAE_B)
def test_gae_sizes_masks_and_discounts(ops, B, T):
    worst = [0.0, 0.0, 0.0]
    for masks in R.GAE_MASKS:
        for gl in R.GAE_GL:
            r, v, nv, done, term = R.gae_inputs(B, T, masks)
            gl32 = tuple(float(torch.tensor(x, dtype=torch.float32)) for x in gl)     # the kernel's scalar arguments
            a64, t64 = R.gae64(r.double(), v.double(), nv.double(), done, term, *gl32)
            a32, t32 = R.gae64(r, v, nv, done, term, *gl)
            adv, tgt = ops.gae(dev(r), dev(v), dev(nv), done=dev(done), terminated=dev(term), gamma=gl[0], lmbda=gl[1])
            for got, ref, f32 in ((adv, a64, a32), (tgt, t64, t32)):
                e32 = R.max_err(f32, ref)
                bound = R.tensor_bound(e32, ref)
                err = (got.cpu().double() - ref).abs()
                worst = [max(worst[0], e32), max(worst[1], bound), max(worst[2], float(err.max()))]
                assert bool((err <= torch.clamp(1e-4 + 1e-5 * ref.abs(), max=bound)).all()), (masks, gl)
    print(f"UPD gae B={B} T={T} (12 mask/discount settings, worst): e32 {worst[0]:.3e} bound {worst[1]:.3e} gpu {worst[2]:.3e}")


# ---- tarl_advantage_stats / tarl_advantage_normalize ------------------------------------------------------------------
@pytest.mark.parametrize("n", R.STATS_N)
def test_advantage_stats_and_normalize(ops, n):
    for kind in ("wide", "narrow"):
        a = R.stats_inputs(n, kind)
        s = ops.advantage_stats(dev(a)).cpu()
        ref = R.adv_stats64(a)
        rel = [abs(float(s[i]) - ref[k]) / abs(ref[k]) for i, k in enumerate(("sum", "sumsq", "n"))]
        print(f"UPD stats n={n} {kind}: relative error sum {rel[0]:.2e} sumsq {rel[1]:.2e} n {rel[2]:.1e} (bound 1e-12)")
        assert max(rel) <= 1e-12
    a = R.stats_inputs(n, "wide")
    x = dev(a.clone())
    ops.advantage_normalize_(x, ops.advantage_stats(x))
    _check_tensor(f"normalize n={n}", x, R.normalize64(a.double()), R.normalize64(a, R.adv_stats64(a)), 1e-4, 1e-4)
    c = dev(R.stats_inputs(n, "const"))
    ops.advantage_normalize_(c, ops.advantage_stats(c))
    assert bool((c == 0).all())                        # std falls to the floor, (a - mean) is exactly zero


# ---- tarl_adam_step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_hyperparameters_scale_and_resume(ops, n):
    h = R.ADAM_HYPER
    p0, grad, m0, v0 = R.adam_inputs(n)
    for step, (m_in, v_in) in ((1, (torch.zeros(n), torch.zeros(n))), (5000, (m0, v0))):
        p = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
        if step > 1:
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m_in.clone(), "exp_avg_sq": v_in.clone()}
        p.grad = grad * 0.5
        opt.step()
        q, m, v = dev(p0.clone()), dev(m_in.clone()), dev(v_in.clone())
        ops.adam_step_(q, dev(grad), m, v, step, grad_scale=0.5, **h)
        st = opt.state[p]
        p64, m64, v64 = R.adam64(p0.double(), grad.double(), m_in.double(), v_in.double(), step, grad_scale=0.5, **h)
        for name, got, t32, t64 in (("param", q, p.detach(), p64), ("exp_avg", m, st["exp_avg"], m64),
                                    ("exp_avg_sq", v, st["exp_avg_sq"], v64)):
            assert torch.allclose(got.cpu(), t32, rtol=1e-6, atol=1e-7), (name, step)
            assert torch.allclose(got.cpu().double(), t64, rtol=1e-6, atol=1e-7), (name, step, "float64")
            print(f"UPD adam n={n} step={step} {name}: vs torch.optim {R.max_err(got.cpu(), t32):.3e} vs float64 "
                  f"{R.max_err(got.cpu(), t64):.3e} (bound 1e-7 + 1e-6 |x|)")


# ---- distribution forward and backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.DIST_T)
@pytest.mark.parametrize("name", list(R.DIST_GRAPHS))
def test_graphdist_forward_backward_vs_float64_autograd(ops, name, T):
    ei, N, logits, choice, w_lp, w_ent = R.dist_inputs(name)
    b = R.dist_reference(ei, N, logits, choice, w_lp, w_ent, T)
    plan = ops.Plan(ei, N)
    spec = R.DIST_GRAPHS[name]
    assert plan.max_out == spec["D"] and plan.src_sorted == spec["sorted"] and (plan.num_groups != N) == spec["holes"]
    d32 = R.segment_dist(logits, ei, T, N)
    p = ops.graphdist_softmax(plan, dev(logits), T)
    tag = f"dist {name} T={T}"
    _check_tensor(f"{tag} proba", p, b["ref_proba"], d32.proba, 1e-6, 1e-5)
    ch = dev(choice.to(torch.int32))
    lp, ent = ops.graphdist_logprob_entropy(plan, p, choice=ch)
    lp_oh, ent_oh = ops.graphdist_logprob_entropy(plan, p, action_onehot=dev(d32.onehot(choice)))
    assert torch.equal(lp_oh, lp) and torch.equal(ent_oh, ent)
    _check_tensor(f"{tag} log_prob", lp, b["ref_lp"], d32.log_prob(choice), min(2e-2, 1e-5 * float(b["ref_lp"].abs().min())), 0.0)
    _check_tensor(f"{tag} entropy", ent, b["ref_ent"], d32.entropy(), min(2e-2, 1e-5 * float(b["ref_ent"].abs().min())), 0.0)
    # backward: the three configurations of the trainer's call
    g = ops.graphdist_logprob_entropy_bwd(plan, p, T, choice=ch, grad_log_prob=dev(w_lp))
    g_oh = ops.graphdist_logprob_entropy_bwd(plan, p, T, action_onehot=dev(d32.onehot(choice)), grad_log_prob=dev(w_lp))
    assert torch.equal(g, g_oh)
    _grad_check(f"{tag} grad(log_prob)", g, b, "grad_lp")
    g = ops.graphdist_logprob_entropy_bwd(plan, p, T, grad_entropy=dev(w_ent))
    _grad_check(f"{tag} grad(entropy)", g, b, "grad_ent")
    bad = dev(b["bad"].to(torch.int32))
    lp_bad, _ = ops.graphdist_logprob_entropy(plan, p, choice=bad)
    assert lp_bad[1].item() == -math.inf and torch.equal(torch.isfinite(lp_bad).cpu(), torch.isfinite(b["lp_bad"]))
    g = ops.graphdist_logprob_entropy_bwd(plan, p, T, choice=bad, grad_log_prob=dev(w_lp), grad_entropy=dev(w_ent),
                                          log_prob_fwd=lp_bad)
    _grad_check(f"{tag} grad(both, row 1 impossible)", g, b, "grad_both")
    if plan.num_groups != N:                            # edges are all owned by a node with out-edges: every entry written
        assert bool(torch.isfinite(g).all())


def _grad_check(what, got, b, key):
    """As _check_tensor (cap: the golden test's 1e-4 absolute), with the e32 that dist_reference measured."""
    ref = b["ref_" + key].double()
    err = (got.cpu().double() - ref).abs()
    print(f"UPD {what}: e32 {b['e32_' + key]:.3e} bound {b[key]:.3e} gpu {float(err.max()):.3e}")
    assert float(err.max()) <= min(b[key], 1e-4), what


# ---- tarl_rollout_gather ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_minor", [False, True])
def test_rollout_gather_both_layouts(ops, env_minor):
    T, B, N = 3, 5, 70
    ei = R.ring_graph(N, 4, sorted=False, seed=9)
    plan, po = ops.Plan(ei, N), R.PlanOrder(ei, N)
    gen = torch.Generator().manual_seed(12)
    rank = (torch.rand((T, B, N), generator=gen) * po.deg).long()
    carried = torch.rand((T, B, N), generator=gen) < 0.2
    byte = (rank | torch.where(carried, 0x80, 0)).to(torch.uint8)                # [T][B][N]
    cnt = torch.randint(0, 256, (T, B, N), generator=gen).to(torch.uint8)
    cnt[0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    want_c = torch.where(carried, torch.full_like(rank, -1), po.order[po.start + rank]).view(T * B, N)
    want_f = cnt.float().view(T * B, N)
    lay = (lambda t: t.permute(0, 2, 1).contiguous()) if env_minor else (lambda t: t.contiguous())
    cb, fb = dev(lay(byte)), dev(lay(cnt))
    for idx in (None, torch.tensor([14, 14, 13, 9, 9, 3, 0, 0])):
        rows = slice(None) if idx is None else idx
        ce, cf = ops.rollout_gather(plan, T, B, env_minor, dev(idx), choice=cb, counts=fb)
        assert ce.dtype == torch.int32 and torch.equal(ce.cpu().long(), want_c[rows])
        assert cf.dtype == torch.float32 and torch.equal(cf.cpu(), want_f[rows])
        ce1, none = ops.rollout_gather(plan, T, B, env_minor, dev(idx), choice=cb)
        none2, cf1 = ops.rollout_gather(plan, T, B, env_minor, dev(idx), counts=fb)
        assert none is None and none2 is None and torch.equal(ce1, ce) and torch.equal(cf1, cf)
    assert bool((want_c == -1).any()) and bool((want_c >= 0).any())


# ---- uint8 row-major critic --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 24), (129, 31), (300, 77)])
def test_critic_uint8_rows_and_accumulating_backward(ops, M, N):
    gen = torch.Generator().manual_seed(M + N)
    torch.manual_seed(M * 3 + N)
    lin = [torch.nn.Linear(N + 1, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1)]
    params = [p.detach() for l in lin for p in (l.weight, l.bias)]
    flat = [dev((p.reshape(-1) if i == 4 else p).contiguous()) for i, p in enumerate(params)]
    cw = ops.CriticWeights(*flat)
    counts = torch.randint(0, 256, (M, N), generator=gen).to(torch.uint8)
    counts.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    times = dev(torch.rand(M, generator=gen) * 10 + 21.54)
    big8 = torch.zeros((M, N + 12), dtype=torch.uint8, device="cuda")       # row stride != N
    big8[:, :N] = dev(counts)
    bigf = torch.full((M, N + 12), 7.0, device="cuda")
    bigf[:, :N] = dev(counts.float())
    v8, h18, h28 = ops.critic_forward(cw, big8[:, :N], times, keep_hidden=True)
    vf, h1f, h2f = ops.critic_forward(cw, bigf[:, :N], times, keep_hidden=True)
    assert big8[:, :N].stride(0) == N + 12
    assert torch.equal(v8, vf) and torch.equal(h18, h1f) and torch.equal(h28, h2f)
    v8n, _, _ = ops.critic_forward(cw, big8[:, :N], times)
    assert torch.equal(v8n, vf)
    # backward adds to what the gradient buffers hold
    gv = dev(torch.randn(M, generator=gen))
    zero = [torch.zeros_like(t) for t in flat]
    ops.critic_backward(cw, bigf[:, :N], times, 1, h1f, h2f, gv, zero)
    prior = [dev(torch.randn(t.shape, generator=gen)) for t in flat]
    acc = [t.clone() for t in prior]
    ops.critic_backward(cw, bigf[:, :N], times, 1, h1f, h2f, gv, acc)
    for i, (a, p0, g0) in enumerate(zip(acc, prior, zero)):
        s = p0 + g0
        ulp = torch.nextafter(s.abs(), torch.full_like(s, math.inf)) - s.abs()
        assert float(g0.abs().max()) > 0 and bool(((a - s).abs() <= ulp).all()), f"grad {i}"
