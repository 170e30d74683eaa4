"""CPU: pins tests/update_restatement.py (the float64 reference of the GPU update / draw tests) to what the project already
trusts — oracle/dist.py, oracle/ppo.py, the reference's golden vectors — and checks that every GPU case of
test_gpu_update_fp64.py is sensitive: with one row / element, or one wave's worth (64 consecutive), lost, every compared
output moves by more than 10x the tolerance the GPU test applies (all of it computable without a GPU)."""
import math

import pytest
import torch

import update_restatement as R
from conftest import load_golden
from oracle import dist, ppo

D = torch.float64


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=D).detach(), torch.as_tensor(b, dtype=D).detach()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin) and torch.equal(a[~fin], b[~fin])
    assert float((a[fin] - b[fin]).abs().max() if fin.any() else 0.0) <= tol * max(1.0, float(b[fin].abs().max() if fin.any() else 0.0))


# ---- the restatement against the oracle and the goldens -------------------------------------------------------------
@pytest.mark.parametrize("N,Dg,srt", [(40, 4, True), (1030, 4, False), (300, 9, False)])
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_segment_dist_equals_graphdist_in_float64(N, Dg, srt, T):
    ei = R.ring_graph(N, Dg, srt, seed=1)
    gen = torch.Generator().manual_seed(N)
    l1 = (torch.randn((3, ei.size(1)), generator=gen) * 6).double().requires_grad_(True)
    l2 = l1.detach().clone().requires_grad_(True)
    a, b = R.segment_dist(l1, ei, T, N), dist.GraphDist(l2, ei, T)
    po = R.PlanOrder(ei, N)
    choice = po.order[po.start + (torch.rand((3, N), generator=gen) * po.deg).long()]
    choice[1, 7] = -1                                             # an impossible action
    onehot = a.onehot(choice)
    assert int(onehot.sum()) == 3 * N - 1
    _close(a.proba, b.proba)
    _close(a.log_prob(choice), b.log_prob(onehot))
    _close(a.log_prob(onehot=onehot), b.log_prob(onehot))
    assert a.log_prob(choice)[1].item() == -math.inf
    _close(a.entropy(), b.entropy().view(3))
    w = torch.randn(3, generator=gen).double()
    fin = torch.tensor([True, False, True])
    ((a.log_prob(choice)[fin] * w[fin]).sum() + (a.entropy() * w).sum()).backward()
    ((b.log_prob(onehot)[fin] * w[fin]).sum() + (b.entropy().view(3) * w).sum()).backward()
    _close(l1.grad, l2.grad)
    lt, et = a.node_terms(choice)
    _close(et.sum(-1), a.entropy())
    _close(lt.sum(-1)[fin], a.log_prob(choice)[fin])


@pytest.mark.parametrize("name", ["dist_small", "dist_mid"])
def test_segment_dist_equals_the_golden_vectors(name):
    """float64 on the golden's fp32 logits against the reference's fp32 results, at the tolerances the GPU golden test
    applies to the kernels (probabilities 1e-6 + 1e-5 relative, everything else 1e-4)."""
    g = load_golden(name)
    ei = g["edge_index"]
    N = int(ei.max()) + 1
    d = R.segment_dist(g["logits"].double(), ei, 1.0, N)
    assert int(d.has_out.sum()) == g["nb_nodes"]
    assert torch.allclose(d.proba.float(), g["proba"], atol=1e-6, rtol=1e-5)
    assert abs(d.entropy().item() - float(g["entropy"])) < 1e-4
    po = R.PlanOrder(ei, N)
    for k in range(4):
        assert abs(d.log_prob(onehot=g[f"a{k}"]).item() - float(g[f"lp{k}"])) < 1e-4
        ch, _ = R.choice_from_onehot(g[f"a{k}"], po)
        assert torch.equal(d.onehot(ch), g[f"a{k}"]) and d.log_prob(ch).item() == d.log_prob(onehot=g[f"a{k}"]).item()
    assert d.log_prob(onehot=g["bad"]).item() == -math.inf
    lb = g["logits_b"].double().requires_grad_(True)
    db = R.segment_dist(lb, ei, 1.0, N)
    lp, ent = db.log_prob(onehot=g["acts_b"]), db.entropy()
    assert torch.allclose(db.proba.float(), g["proba_b"], atol=1e-6, rtol=1e-5)
    assert torch.allclose(lp.float(), g["lp_b"], atol=1e-4, rtol=0) and torch.allclose(ent.float(), g["ent_b"], atol=1e-4, rtol=0)
    g_lp, = torch.autograd.grad((lp * g["w_b"].double()).sum(), lb, retain_graph=True)
    g_en, = torch.autograd.grad((ent * g["w_b"].double()).sum(), lb)
    assert torch.allclose(g_lp.float(), g["grad_lp_b"], atol=1e-4, rtol=0)
    assert torch.allclose(g_en.float(), g["grad_ent_b"], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["r1x4s", "r2x4u", "g9"])
def test_sample_restatement_equals_graphdist_sample(name):
    """The per-node draw used where the oracle cannot go (sources that are not compact): same thresholds, bit for bit,
    and same picks as GraphDist on graphs where both apply — also with u on a threshold, at 0 and just below 1."""
    ei, N, logits, u, _ = R.draw_inputs(name)
    po = R.PlanOrder(ei, N)
    assert po.G == N
    for b in range(2):
        p = dist.segment_softmax(logits[b] / R.DRAW_T, ei[0], N)
        d = dist.GraphDist(logits[b], ei, proba=p)
        cum = R.rebased_cumsum(p, po)
        assert torch.equal(cum, d.cumsum)
        ub = u[b].clone()
        ub[::5] = 0.0
        ub[::7] = 0.99999994
        ub[::11] = cum[po.start[::11]]
        ch, rk = R.sample_choice(p, po, ub)
        ch2, rk2 = R.choice_from_onehot(d.sample(ub), po)
        assert torch.equal(ch, ch2) and torch.equal(rk, rk2)
        assert bool((ch[::11][po.deg[::11] == 1] == -1).all())        # strict comparison: a degree-1 node draws nothing


def test_ring_graph_family():
    for N, Dg in ((40, 4), (1025, 8), (1500, 9), (300, 12)):
        ei = R.ring_graph(N, Dg)
        deg = torch.bincount(ei[0], minlength=N)
        assert torch.equal(deg, 1 + torch.arange(N) % Dg) and int(deg.max()) == Dg
        assert bool((ei[0][1:] >= ei[0][:-1]).all())
        k = torch.arange(ei.size(1)) - (torch.cumsum(deg, 0) - deg)[ei[0]]
        assert torch.equal(ei[1], (ei[0] + torch.tensor(R.RING_OFFSETS)[k]) % N)
        eu = R.ring_graph(N, Dg, sorted=False, seed=4)
        assert not bool((eu[0][1:] >= eu[0][:-1]).all())
        assert torch.equal(torch.sort(eu[0] * N + eu[1])[0], torch.sort(ei[0] * N + ei[1])[0])
        assert torch.equal(eu, R.ring_graph(N, Dg, sorted=False, seed=4))
    eh = R.ring_graph(1500, 4, sorted=False, holes=True, seed=2)
    deg = torch.bincount(eh[0], minlength=1500)
    assert bool((deg[torch.arange(1500) % 17 == 5] == 0).all()) and int((deg == 0).sum()) == 88 and int(deg.max()) == 4
    for name, (N, Dg, srt, holes, kernel) in R.DRAW_CASES.items():     # every row of the table reaches its kernel
        deg = 1 + torch.arange(N) % Dg
        G = N - (int((torch.arange(N) % 17 == 5).sum()) if holes else 0)
        assert R.draw_dispatch(N, G, Dg, srt) == kernel, name
    reached = {v[4] for v in R.DRAW_CASES.values()}
    assert reached == {f"reg<{j},{d},{s}>" for j, d in ((1, 4), (2, 4), (3, 4), (4, 4), (1, 8), (2, 8))
                       for s in ("sorted", "unsorted")} | {"generic"}


@pytest.mark.parametrize("M", [1, 257, 4133])
@pytest.mark.parametrize("coefs", R.PPO_COEFS)
def test_ppo_loss64_equals_the_oracle_in_float64(M, coefs):
    ins = [t.double() for t in R.ppo_inputs(M)]
    out, g_lp, g_ent, g_val, mean_abs = R.ppo_loss64(*ins, **coefs)
    lp_new, value, ent = (ins[i].clone().requires_grad_(True) for i in (0, 3, 5))
    kw = {k: v for k, v in coefs.items() if k != "grad_scale"}
    ref = ppo.clip_ppo_loss(lp_new, ins[1], ins[2], value, ins[4], ent, **kw)
    ((ref["loss_objective"] + ref["loss_critic"] + ref["loss_entropy"]) * coefs.get("grad_scale", 1.0)).backward()
    for i, k in enumerate(("loss_objective", "loss_critic", "loss_entropy")):
        _close(out[i], ref[k].detach())
    _close(g_lp, lp_new.grad)
    _close(g_ent, ent.grad)
    _close(g_val, value.grad)
    lw = ins[0] - ins[1]
    eps = coefs.get("clip_epsilon", 0.2)
    _close(out[3], ((lw < math.log1p(-eps)) | (lw > math.log1p(eps))).double().mean())
    _close(out[4], (-lw).mean())
    _close(out[5], lw.exp().sum() ** 2 / (2 * lw).exp().sum())
    assert mean_abs.shape == (6,) and bool((mean_abs >= out.abs() - 1e-15).all())
    if M > 1:
        assert 0.0 < float(out[3]) < 1.0                    # log-ratios on both sides of the clip
        d = (ins[3] - ins[4]).abs()
        assert bool((d < 1).any()) and bool((d > 1).any())


@pytest.mark.parametrize("masks", R.GAE_MASKS)
@pytest.mark.parametrize("gl", R.GAE_GL)
def test_gae64_equals_the_oracle_in_float64(masks, gl):
    r, v, nv, done, term = R.gae_inputs(37, 50, masks)
    z = torch.zeros_like(r, dtype=torch.uint8)
    a, t = R.gae64(r.double(), v.double(), nv.double(), done, term, *gl)
    a2, t2 = ppo.gae(r.double(), v.double(), nv.double(), z if done is None else done, z if term is None else term, *gl,
                     average_gae=False)
    _close(a, a2)
    _close(t, t2)
    an, _ = ppo.gae(r.double(), v.double(), nv.double(), z if done is None else done, z if term is None else term, *gl)
    _close(R.normalize64(a), an, 1e-11)
    s = R.adv_stats64(a.float())
    _close(s["sum"], a.float().double().sum(), 1e-13)
    _close(s["sumsq"], (a.float().double() ** 2).sum(), 1e-13)
    assert s["n"] == a.numel()


@pytest.mark.parametrize("step", [1, 5000])
def test_adam64_equals_the_oracle_in_float64(step):
    p, g, m, v = (t.double() for t in R.adam_inputs(257))
    h = R.ADAM_HYPER
    p1, m1, v1 = R.adam64(p, g, m, v, step, grad_scale=0.5, **h)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ppo.adam_step(p2, g * 0.5, m2, v2, step, h["lr"], h["beta1"], h["beta2"], h["eps"])
    _close(p1, p2)
    _close(m1, m2)
    _close(v1, v2)


# ---- sensitivity of the GPU cases -------------------------------------------------------------------------------------
def _lost(ref, tol, what):
    """Per-element outputs: a kernel that loses an element leaves it unwritten — the output then differs from the
    reference by that element. The last element, and the largest of the last 64, must stand out of the tolerance."""
    flat = ref.detach().double().reshape(-1)
    assert abs(float(flat[-1])) > 10 * tol, (what, "last element", float(flat[-1]), tol)
    assert float(flat[-64:].abs().max()) > 10 * tol, (what, "last wave", tol)


@pytest.mark.parametrize("M", R.PPO_SIZES)
@pytest.mark.parametrize("coefs", R.PPO_COEFS)
def test_ppo_cases_notice_a_lost_row_and_a_lost_wave(M, coefs):
    """Six scalars: the reference with the last row, and with the last 64 rows, removed (where that leaves a row) must
    differ from the full reference by more than 10x the depth bound. Seeds: the lost rows' own seeds against their bound."""
    ins = [t.double() for t in R.ppo_inputs(M)]
    lo, hi = R.clip_thresholds32(coefs.get("clip_epsilon", 0.2))
    out, g_lp, g_ent, g_val, mean_abs = R.ppo_loss64(*ins, **coefs, lo=lo, hi=hi)
    tol = [R.scalar_bound(M, mean_abs[i], ess=(i == 5)) for i in range(6)]
    for k in (1, 64):
        if M - k < 1:
            continue
        out_k = R.ppo_loss64(*(t[:M - k] for t in ins), **coefs, lo=lo, hi=hi)[0]
        for i in range(6):
            assert abs(float(out_k[i] - out[i])) > 10 * tol[i], (M, k, i, float(out_k[i] - out[i]), tol[i])
    ins32 = R.ppo_inputs(M)
    _, e_lp, e_ent, e_val, _ = R.ppo_loss64(*ins32, **coefs, lo=lo, hi=hi)       # the same arithmetic in fp32
    for name, ref, f32 in (("g_lp", g_lp, e_lp), ("g_ent", g_ent, e_ent), ("g_val", g_val, e_val)):
        tol_t = R.tensor_bound(R.max_err(f32, ref), ref, relative_scale=True)
        assert float(ref[-64:].abs().max()) > 10 * tol_t, (name, M)
        if name != "g_lp":                                   # (a clipped row's g_lp is 0: the wave has unclipped rows)
            assert abs(float(ref[-1])) > 10 * tol_t, (name, M)


@pytest.mark.parametrize("B", R.GAE_B)
@pytest.mark.parametrize("T", R.GAE_T)
def test_gae_cases_notice_a_lost_element(B, T):
    for masks in R.GAE_MASKS:
        for gl in R.GAE_GL:
            r, v, nv, done, term = R.gae_inputs(B, T, masks)
            gl32 = tuple(float(torch.tensor(x, dtype=torch.float32)) for x in gl)
            a, t = R.gae64(r.double(), v.double(), nv.double(), done, term, *gl32)
            a32, t32 = R.gae64(r, v, nv, done, term, *gl)
            for ref, f32, what in ((a, a32, "adv"), (t, t32, "target")):
                tol = R.tensor_bound(R.max_err(f32, ref), ref)
                for row in range(T):                                             # the last thread's element of every frame
                    _lost(ref[row], tol, (what, B, T, masks, gl))


@pytest.mark.parametrize("n", R.STATS_N)
def test_stats_cases_notice_a_lost_element(n):
    for kind in ("wide", "narrow"):
        a = R.stats_inputs(n, kind)
        s = R.adv_stats64(a)
        for k in (1, 64):
            if n - k < 1:
                continue
            sk = R.adv_stats64(a[:n - k])
            for key in ("sum", "sumsq", "n"):
                assert abs(sk[key] - s[key]) > 10 * 1e-12 * abs(s[key]), (n, kind, k, key)
    a = R.stats_inputs(n, "wide")
    ref = R.normalize64(a.double())
    tol = R.tensor_bound(R.max_err(R.normalize64(a, R.adv_stats64(a)), ref), ref)
    # a lost element stays un-normalised
    d = (a.double() - ref).abs()
    assert float(d[-1]) > 10 * tol and float(d[-64:].max()) > 10 * tol
    assert abs(float(a.double().mean())) <= 10 * float(a.double().std())


@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_cases_notice_a_lost_element(n):
    """A lost element keeps its old parameter / moments: the update must exceed 10x (1e-7 + 1e-6 |x|)."""
    p, g, m, v = R.adam_inputs(n)
    for step, (m0, v0) in ((1, (torch.zeros(n), torch.zeros(n))), (5000, (m, v))):
        new = R.adam64(p.double(), g.double(), m0.double(), v0.double(), step, grad_scale=0.5, **R.ADAM_HYPER)
        for old, x in zip((p, m0, v0), new):
            d = (x - old.double()).abs() - 10 * (1e-7 + 1e-6 * x.abs())
            assert float(d[-1]) > 0 and float(d[-64:].max()) > 0, (n, step)


@pytest.mark.parametrize("name", list(R.DIST_GRAPHS))
@pytest.mark.parametrize("T", R.DIST_T)
def test_dist_cases_notice_a_lost_node(name, T):
    """log-prob and entropy are sums over the nodes: the last node with out-edges, and the last 64 together, contribute
    more than 10x the tolerance; probabilities and gradients are per edge (the lost edge keeps a zero)."""
    ei, N, logits, choice, w_lp, w_ent = R.dist_inputs(name)
    b = R.dist_reference(ei, N, logits, choice, w_lp, w_ent, T)
    d = R.segment_dist(logits.double(), ei, T, N)
    assert bool((d.proba < 1e-8).any())                     # the epsilon matters
    lt, et = d.node_terms(choice)
    nodes = torch.nonzero(d.has_out).view(-1)
    for terms, tol, what in ((lt, b["lp"], "lp"), (et, b["ent"], "ent")):
        assert float(terms[:, nodes[-1]].abs().min()) > 10 * tol, (what, "node")
        assert float(terms[:, nodes[-64:]].sum(-1).abs().min()) > 10 * tol, (what, "wave")
    last = R.PlanOrder(ei, N).order[-64:]                   # the last node's edges, the last wave of nodes' edges
    assert float(d.proba[:, last].max()) > 10 * b["proba"]
    for key in ("grad_lp", "grad_ent", "grad_both"):
        assert float(b["ref_" + key][:, last].abs().max()) > 10 * b[key], key
