"""GPU: the learned per-decision critic — tarl_decision_critic_features / _fwd against the fp32 restatement bit
for bit and within ``update_restatement.tensor_bound`` of float64 (packed random states and states after 40 frames of the
holding router; the torus at, below and above one tile of 256 roads and both irregular graphs; M in {1, 3, 65}; random and
sharp weights; outputs between guard bands in NaN-filled buffers), tarl_decision_critic_loss against float64 (sums, gradient,
accumulation, scratch from NaN, reproducibility, L = 0, one-hot probes at the tile and partition edges), the trainer, the
learning case that fails without the feature, and the CLI."""
import json
import math

import numpy as np
import pytest
import torch

import decision_critic_restatement as C
import update_restatement as R

pytestmark = pytest.mark.gpu

GRAPHS = ["torus8x8", "torus6x5", "torus9x8", "MIXED", "HUB126"]
DELAY_SCALE = 16.0
MAX_LIVE = 2500      # the restatement loops over the live decisions in Python: larger masks are thinned (the mask is an input)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _net(name):
    import test_gpu_decision_credit as TD
    return TD._net(name)


def _packed(ops, net, B, t=200.0):
    """B random mid-simulation states packed -> (plan, fs, x on the device, agent tables on the device)."""
    import irregular_graphs as ig
    from tarl_hip import synth
    Nmax, N = net.Nmax, net.num_roads
    x = torch.stack([ig.random_state(net, seed=300 + b, t=t) for b in range(B)])
    A = int(x[:, :, :Nmax].max()) + 2
    ag = torch.stack([synth.population(A - 1, N, seed=b, t0=100, t1=130) for b in range(B)]).cuda()
    plan = ops.Plan(net.edge_index, N)
    fs = ops.FusedState(plan, B, A, "cuda", Nmax)
    xd = x.cuda()
    ops.fused_pack(plan, fs, xd, Nmax, ag, net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    fs.check_flags()
    return plan, fs, xd, ag


_INPUTS = {}


def _inputs(name, M, kind):
    """Observations (ops.fused_obs16) and heads (ops.fused_head_rows) of one state of M environments; the free-flow table
    to every destination of the agent tables (ops.destination_trees); random frames_left and raw advantages.
    -> dict of host arrays and the plan (computed once per case)."""
    key = (name, M, kind)
    if key in _INPUTS:
        return _INPUTS[key]
    import test_gpu_decision_credit as TD
    from tarl_hip import ops
    from tarl_hip.evaluator import VecEvaluator
    net = _net(name)
    N = net.num_roads
    if kind == "packed":
        plan, fs, xd, ag = _packed(ops, net, M)
        Nmax, tau = net.Nmax, 0.25
    else:
        _, eng, _ = TD._live_case(M, name)
        VecEvaluator(eng, "dijkstra_hold").run(40)
        eng.check_flags()
        plan, fs, xd, ag, Nmax, tau = eng.plan, eng.fs, eng._x, eng.agents, eng.Nmax, 1.0
    obs = ops.fused_obs16(plan, fs, xd, Nmax, ag)
    rows = torch.arange(M, dtype=torch.int32, device="cuda")
    head = ops.fused_head_rows(plan, fs, rows, rows, torch.zeros((M, N), dtype=torch.int32, device="cuda"))
    d = torch.unique(ag[..., 1].reshape(-1).to(torch.int64))
    d = d[(d >= 0) & (d < N)].contiguous()
    slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    slot[d] = torch.arange(d.numel(), dtype=torch.int32, device="cuda")
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous().cuda()
    dist = ops.destination_trees(plan, ff, d, want_next_hop=False, want_dist=True)[1]
    rng = np.random.default_rng(17 * M + len(name))
    head = head.cpu().numpy()
    n_heads = int((head > 0).sum())
    assert n_heads > 0
    if n_heads > MAX_LIVE:
        head = np.where(rng.random(head.shape) < MAX_LIVE / n_heads, head, 0).astype(np.int32)
    frames_left = rng.integers(0, 600, M).astype(np.int32)
    adv = np.where(head > 0, rng.normal(size=head.shape) * 24.0 - 4.0, 0.0).astype(np.float32)
    c = dict(plan=plan, ei=net.edge_index.numpy(), N=N, obs=obs.cpu().numpy(), head=head, live=head > 0,
             frames_left=frames_left, dist=dist.cpu().numpy().astype(np.float64), slot=slot.cpu().numpy(), adv=adv, timestep=tau)
    c["f32"] = C.features(c["ei"], N, c["obs"], head, frames_left, c["dist"], c["slot"], tau, np.float32)
    c["f64"] = C.features(c["ei"], N, c["obs"], head, frames_left, c["dist"], c["slot"], tau, np.float64)
    _INPUTS[key] = c
    return c


def _dev(c):
    """The case's device tensors: obs, head, frames_left, dist, slot (positional arguments of the ops after the plan)."""
    return (torch.from_numpy(c["obs"]).cuda(), torch.from_numpy(c["head"]).cuda(), torch.from_numpy(c["frames_left"]).cuda(),
            torch.from_numpy(c["dist"]).cuda(), torch.from_numpy(c["slot"]).cuda())


def _guarded(shape, dtype=torch.float32, pad=64):
    """A NaN-filled buffer with guard bands -> (whole, view)."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
    return big, big[pad:pad + n].view(shape)


def _guards_intact(big, n, pad=64):
    return bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n:]).all())


def _weights(ops, w):
    return ops.DecisionCriticWeights(flat=torch.from_numpy(np.asarray(w, dtype=np.float32)).cuda())


# ---- 1. features and value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_features_and_value_against_the_restatement(name, M):
    from tarl_hip import ops
    for kind in ("packed", "live"):
        c = _inputs(name, M, kind)
        N, live = c["N"], c["live"]
        args = _dev(c)
        big, feats = _guarded((M, N, 8))
        ops.decision_critic_features(c["plan"], *args, timestep=c["timestep"], out=feats)
        torch.cuda.synchronize()
        assert _guards_intact(big, M * N * 8)
        got = feats.cpu().numpy()
        assert np.array_equal(got, c["f32"]), (kind, int((got != c["f32"]).sum()))           # bit for bit (no NaN is left)
        assert not got[~live].any()
        b = R.tensor_bound(R.max_err(_t(c["f32"]), _t(c["f64"])), _t(c["f64"]))
        assert R.max_err(_t(got), _t(c["f64"])) <= b
        assert got[live][:, 0].max() > 0 and got[live][:, 2:5].any()
        adv = torch.from_numpy(c["adv"]).cuda()
        for sharp in (False, True):
            w = C.weights(11 + M, sharp)
            v32, a32 = C.forward(w, c["f32"], live, c["adv"], DELAY_SCALE, np.float32)
            v64, a64 = C.forward(w.astype(np.float64), c["f64"], live, c["adv"], DELAY_SCALE, np.float64)
            bv, value = _guarded((M, N))
            ba, adv_out = _guarded((M, N))
            ops.decision_critic_forward(c["plan"], *args, _weights(ops, w), adv, timestep=c["timestep"],
                                        delay_scale=DELAY_SCALE, value=value, adv_out=adv_out)
            torch.cuda.synchronize()
            assert _guards_intact(bv, M * N) and _guards_intact(ba, M * N)
            gv, ga = value.cpu().numpy(), adv_out.cpu().numpy()
            assert np.array_equal(gv, v32) and np.array_equal(ga, a32), (kind, sharp)
            assert not gv[~live].any() and not ga[~live].any()
            assert np.array_equal(ga, (c["adv"] + np.float32(DELAY_SCALE) * gv).astype(np.float32))
            assert R.max_err(_t(gv), _t(v64)) <= R.tensor_bound(R.max_err(_t(v32), _t(v64)), _t(v64))
            assert R.max_err(_t(ga), _t(a64)) <= R.tensor_bound(R.max_err(_t(a32), _t(a64)), _t(a64))
            v2, none = ops.decision_critic_forward(c["plan"], *args, _weights(ops, w), adv, timestep=c["timestep"],
                                                   delay_scale=DELAY_SCALE, want_adv=False)
            assert none is None and torch.equal(v2, value)
        # the initialisation: a zero last layer gives value 0 and the raw advantage, bit for bit
        v0, a0 = ops.decision_critic_forward(c["plan"], *args, _weights(ops, C.init_weights()), adv, timestep=c["timestep"])
        assert not bool(v0.any()) and torch.equal(a0, adv)


# ---- 2. the loss ----------------------------------------------------------------------------------------------------------------
def _loss_bounds(r32, r64, N):
    g64 = _t(r64["grads"])
    b_g = R.tensor_bound(R.max_err(_t(r32["grads"]), g64), g64, relative_scale=True)
    o64 = _t(r64["out5"])
    # out5: fp32 terms (the restatement's, to within the kernel's own order) summed in fp64 through a six-level shuffle tree,
    # four waves and ceil(N / 256) tiles in order: depth (6 + 4 + tiles) of 2^-53 relative to the sum of the magnitudes
    depth = 6 + 4 + math.ceil(N / 256)
    b_o = R.tensor_bound(R.max_err(_t(r32["out5"]), o64), o64) + depth * 2.0 ** -53 * float(o64.abs().max()) * N
    return b_g, b_o


def _run_loss(ops, c, w, n_live, coef=0.75, grad_scale=0.5, grads=None, scratch=None):
    args = _dev(c)
    adv = torch.from_numpy(c["adv"]).cuda()
    nl = torch.tensor([n_live], dtype=torch.int32, device="cuda")
    if grads is None:
        grads = torch.zeros(161, device="cuda")
    out5 = ops.decision_critic_loss(c["plan"], *args, _weights(ops, w), adv, nl, timestep=c["timestep"],
                                    delay_scale=DELAY_SCALE, coef=coef, grad_scale=grad_scale, grads=grads, scratch=scratch)
    return out5, grads


@pytest.mark.parametrize("M", [1, 3, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_loss_against_float64(name, M):
    from tarl_hip import ops
    c = _inputs(name, M, "packed")
    N, live = c["N"], c["live"]
    L = int(live.sum())
    for sharp in (False, True):
        w = C.weights(23 + M, sharp)
        r64 = C.critic_loss(w.astype(np.float64), c["f64"], live, c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float64)
        r32 = C.critic_loss(w, c["f32"], live, c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float32)
        need = ops.decision_critic_scratch_bytes(c["plan"], M)
        scratch = torch.full(((need + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
        out5, grads = _run_loss(ops, c, w, L, scratch=scratch)
        b_g, b_o = _loss_bounds(r32, r64, N)
        e_o, e_g = R.max_err(out5.cpu(), _t(r64["out5"])), R.max_err(grads.cpu(), _t(r64["grads"]))
        print(f"[decision critic loss {name} M={M} sharp={sharp}] L={L}, out5 err {e_o:.3e} (bound {b_o:.3e}), "
              f"grads err {e_g:.3e} (bound {b_g:.3e})")
        assert e_o <= b_o and e_g <= b_g and float(np.abs(r64["grads"]).max()) > 0
        assert torch.equal(out5[:, 1].cpu(), _t(live.sum(1)))
        # two runs are bit-identical; pre-filled grads receive exactly what zeros received
        out5b, gradsb = _run_loss(ops, c, w, L, scratch=scratch)
        assert torch.equal(out5, out5b) and torch.equal(grads, gradsb)
        fill = torch.from_numpy(C.weights(99).copy()).cuda()
        _, filled = _run_loss(ops, c, w, L, grads=fill.clone())
        assert torch.equal(filled, fill + grads)
        # a short scratch is refused; without grads the sums are the same
        if need >= 16:
            with pytest.raises(ValueError, match="scratch holds"):
                _run_loss(ops, c, w, L, scratch=torch.empty(need // 8 - 1, dtype=torch.float64, device="cuda"))
        args = _dev(c)
        nl = torch.tensor([L], dtype=torch.int32, device="cuda")
        out5c = ops.decision_critic_loss(c["plan"], *args, _weights(ops, w), torch.from_numpy(c["adv"]).cuda(), nl,
                                         timestep=c["timestep"], delay_scale=DELAY_SCALE, coef=0.75, grad_scale=0.5)
        assert torch.equal(out5c, out5)
    # L = 0 adds nothing, whatever the mask says
    _, g0 = _run_loss(ops, c, w, 0, grads=fill.clone())
    assert torch.equal(g0, fill)


def test_loss_on_dense_tiles():
    """Every road of every tile live (the compaction fills all 256 rows, every wave's ballot is full), at small M: the torus
    at exactly one tile and above it, and HUB126."""
    from tarl_hip import ops
    for name in ("torus8x8", "torus9x8", "HUB126"):
        c = dict(_inputs(name, 3, "packed"))
        M, N = 3, c["N"]
        rng = np.random.default_rng(3)
        head = np.full((M, N), 9, dtype=np.int32)
        c.update(head=head, live=head > 0, adv=(rng.normal(size=(M, N)) * 24.0 - 4.0).astype(np.float32))
        L = M * N
        f64 = C.features(c["ei"], N, c["obs"], head, c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float64)
        f32 = C.features(c["ei"], N, c["obs"], head, c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float32)
        feats = ops.decision_critic_features(c["plan"], *_dev(c), timestep=c["timestep"])
        assert np.array_equal(feats.cpu().numpy(), f32)
        w = C.weights(41)
        r64 = C.critic_loss(w.astype(np.float64), f64, c["live"], c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float64)
        r32 = C.critic_loss(w, f32, c["live"], c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float32)
        out5, grads = _run_loss(ops, c, w, L)
        b_g, b_o = _loss_bounds(r32, r64, N)
        e_o, e_g = R.max_err(out5.cpu(), _t(r64["out5"])), R.max_err(grads.cpu(), _t(r64["grads"]))
        print(f"[decision critic dense {name}] L={L}, out5 err {e_o:.3e} (bound {b_o:.3e}), grads err {e_g:.3e} (bound {b_g:.3e})")
        assert e_o <= b_o and e_g <= b_g and float(out5[:, 1].sum()) == L
        out5b, gradsb = _run_loss(ops, c, w, L)
        assert torch.equal(out5, out5b) and torch.equal(grads, gradsb)


_BIG = {}


def _hub_case(M=1027):
    """HUB126 (two tiles of 256 roads) at M = 1027: 2054 (row, tile) pairs in 685 runs of three, so that a run crosses rows."""
    if not _BIG:
        c = _inputs("HUB126", 65, "packed")
        rows = np.arange(M) % 65
        rng = np.random.default_rng(5)
        head = np.where(rng.random((M, c["N"])) < 0.02, c["head"][rows], 0).astype(np.int32)
        _BIG.update(c, obs=c["obs"][rows], head=head, live=head > 0, frames_left=c["frames_left"][rows],
                    adv=np.where(head > 0, c["adv"][rows], 0).astype(np.float32), M=M)
        _BIG.pop("f32"), _BIG.pop("f64")
    return _BIG


def test_loss_where_a_partition_holds_several_tiles():
    from tarl_hip import ops
    c = _hub_case()
    M, N, live = c["M"], c["N"], c["live"]
    assert ops.decision_critic_scratch_bytes(c["plan"], M) == 2054 * 40 + 685 * 161 * 4
    L = int(live.sum())
    assert 300 < L <= MAX_LIVE
    f64 = C.features(c["ei"], N, c["obs"], c["head"], c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float64)
    f32 = C.features(c["ei"], N, c["obs"], c["head"], c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float32)
    w = C.weights(31)
    r64 = C.critic_loss(w.astype(np.float64), f64, live, c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float64)
    r32 = C.critic_loss(w, f32, live, c["adv"], L, DELAY_SCALE, 0.75, 0.5, np.float32)
    out5, grads = _run_loss(ops, c, w, L)
    b_g, b_o = _loss_bounds(r32, r64, N)
    assert R.max_err(out5.cpu(), _t(r64["out5"])) <= b_o and R.max_err(grads.cpu(), _t(r64["grads"])) <= b_g
    out5b, gradsb = _run_loss(ops, c, w, L)
    assert torch.equal(out5, out5b) and torch.equal(grads, gradsb)


def test_one_hot_probes_at_the_tile_and_partition_edges():
    """A single live decision: at the first and the last node of the first and the last tile of the first and the last row,
    and on both sides of the edges of a run of three (row, tile) pairs (pairs 2 | 3 and 5 | 6)."""
    from tarl_hip import ops
    c = dict(_hub_case())
    M, N = c["M"], c["N"]
    assert 256 < N <= 512
    w = C.weights(37)
    probes = [(0, 0), (0, 255), (0, 256), (0, N - 1), (M - 1, 0), (M - 1, 255), (M - 1, 256), (M - 1, N - 1),
              (1, 0), (1, 255), (1, 256), (2, N - 1), (3, 0)]
    for m, u in probes:
        head = np.zeros((M, N), dtype=np.int32)
        head[m, u] = 5
        adv = np.zeros((M, N), dtype=np.float32)
        adv[m, u] = -9.0 - m % 7
        c.update(head=head, live=head > 0, adv=adv)
        f64 = np.zeros((M, N, 8))
        f64[m, u] = C.decision_features(c["ei"], N, c["obs"], m, u, c["frames_left"], c["dist"], c["slot"], c["timestep"],
                                        np.float64)
        r64 = C.critic_loss(w.astype(np.float64), f64[m:m + 1], c["live"][m:m + 1], adv[m:m + 1], 1, DELAY_SCALE, 1.0, 1.0)
        r32 = C.critic_loss(w, f64[m:m + 1].astype(np.float32), c["live"][m:m + 1], adv[m:m + 1], 1, DELAY_SCALE, 1.0, 1.0,
                            np.float32)
        out5, grads = _run_loss(ops, c, w, 1, coef=1.0, grad_scale=1.0)
        o = out5.cpu()
        assert float(o[m, 1]) == 1.0 and float(o[:, 1].sum()) == 1.0, (m, u)
        rest = torch.ones(M, dtype=torch.bool)
        rest[m] = False
        assert not bool(o[rest].any()), (m, u)
        b_g, b_o = _loss_bounds(r32, r64, N)
        assert R.max_err(o[m], _t(r64["out5"][0])) <= b_o, (m, u)
        assert R.max_err(grads.cpu(), _t(r64["grads"])) <= b_g and float(np.abs(r64["grads"]).max()) > 0, (m, u)


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------------------
def _trainer(baseline=None, credit="decision", epochs=2, B=3, T=24, M=8, seed=0, critic=None, **more):
    """test_gpu_decision_credit's trainer (8 x 8 torus, B = 3, the goal-conditioned head, T = 24, minibatches of 8) with the
    critic's arguments. ``critic``: (161,) values set by hand (default: the initialisation)."""
    from src.agents.mpnn_agent import MPNNPolicyNet, MPNNValueNetSimple
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    from tarl_hip.trainer import VecPPOTrainer
    net = synth.torus_network(8, 8)
    N = net.num_roads
    pops = torch.stack([synth.population(128, N, seed=40 + b, t0=21540, t1=21545) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=9)
    torch.manual_seed(1)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].cuda().contiguous()
    pol = MPNNPolicyNet(net.edge_index, N, ff, device="cuda")
    pol.prior_method = "all_pairs"
    pol.use_goal_mlp(ops.goal_time_scale(net.x[:, 3 * net.Nmax:]))
    with torch.no_grad():
        pol.goal_mlp[0].bias.uniform_(-0.3, 0.3)
        pol.goal_mlp[0].weight.uniform_(-1.0, 1.0)
    val = MPNNValueNetSimple(net.edge_index, N, device="cuda")
    l = val.final_mlp
    crit = [l[0].weight, l[0].bias, l[2].weight, l[2].bias, l[4].weight, l[4].bias]
    gm = pol.goal_mlp
    extra = [p for n, p in pol.named_parameters() if not n.startswith("nodes_embedding")]
    kw = dict(more)
    if baseline is not None:
        kw["credit_baseline"] = baseline
    if baseline == "learned":
        cp = ops.decision_critic_init("cuda", seed=5)
        if critic is not None:
            flat = torch.from_numpy(np.asarray(critic, dtype=np.float32)).cuda()
            cp = [flat[:128].view(16, 8).clone(), flat[128:144].clone(), flat[144:160].view(1, 16).clone(), flat[160:].clone()]
        extra = extra + cp
        kw["decision_critic_params"] = cp
    tr = VecPPOTrainer(eng, pol.nodes_embedding.weight, crit, rollout_steps=T, num_epochs=epochs, sub_batch_size=M,
                       extra_params=extra, policy="goal_mlp", temperature=2.0, seed=seed, credit=credit,
                       goal_mlp_params=[gm[0].weight, gm[0].bias, gm[2].weight, gm[2].bias], prior_table=pol.dist_matrix, **kw)
    tr.keep_grad = True
    return tr, net


def test_free_flow_baseline_is_bit_identical_to_the_default():
    a, _ = _trainer("free_flow")
    b, _ = _trainer(None)
    a.train_iteration()
    b.train_iteration()
    assert a.credit_baseline == b.credit_baseline == "free_flow" and set(a.last["decision"]) == set(b.last["decision"])
    assert "critic_loss" not in a.last["decision"]
    assert torch.equal(a.last_grad, b.last_grad) and torch.equal(a.flat.flat, b.flat.flat)
    assert torch.equal(a.adv_raw, b.adv_raw) and torch.equal(a.last["losses"], b.last["losses"])


def test_zero_initialised_critic_leaves_the_first_iteration_as_it_is_and_its_gradient_is_the_restated_one():
    """Under ``"learned"`` with w2 = b2 = 0 the first iteration's ``adv_dec``, statistics and actor gradient ``==`` those of
    ``"free_flow"``; per epoch the critic parameters' gradient is the restatement's (float64, ``tensor_bound``) at the
    parameters in front of that epoch's Adam step; the report is built from the last epoch's sums."""
    import test_gpu_decision_credit as TD
    from tarl_hip import ops
    tl, net = _trainer("learned")
    tf, _ = _trainer("free_flow")
    snaps_l, g_l = TD._record_steps(tl)
    snaps_f, g_f = TD._record_steps(tf)
    tl.train_iteration()
    tf.train_iteration()
    tl.check_flags()
    N, M = tl.eng.N, tl.M
    assert torch.equal(tl.adv_dec, tf.adv_raw) and torch.equal(tl.adv_raw, tf.adv_raw) and not bool(tl.value_old.any())
    assert torch.equal(tl._decision_stats, tf._decision_stats) and torch.equal(tl.head_keep, tf.head_keep)
    n_f = tf.flat.flat.numel()
    off = tl._dcritic_off
    assert tl.flat.flat.numel() == n_f + 161 and off == n_f
    for e in range(2):
        assert torch.equal(g_l[e], g_f[e])                                          # the logits' gradient, both epochs
        assert torch.equal(snaps_l[e][1][:n_f], snaps_f[e][1])                      # every other parameter's gradient
        assert torch.equal(snaps_l[e][0][:n_f], snaps_f[e][0])
    assert bool(snaps_l[0][1][off:off + 161].any())
    # frames_left: t_end - t of every kept row (one segment of T frames)
    frames = torch.tensor(tl._keep[0], dtype=torch.int32)
    slot = tl._keep[2].cpu().long()
    assert torch.equal(tl.frames_left.cpu()[slot], tl.T - frames)
    ei = net.edge_index.numpy()
    dist, dslot = (t.cpu().numpy() for t in tl._decision_dist)
    hk, adv, fl, obs = tl.head_keep.cpu().numpy(), tl.adv_raw.cpu().numpy(), tl.frames_left.cpu().numpy(), tl.obs_mb.cpu().numpy()
    f64 = C.features(ei, N, obs, hk, fl, dist, dslot, tl.eng.timestep, np.float64)
    f32 = f64.astype(np.float32)
    last = None
    for e in range(2):
        sl = slice(e * M, (e + 1) * M)
        w = snaps_l[e][0][off:off + 161].cpu().numpy()
        live = hk[sl] > 0
        L = int(live.sum())
        r64 = C.critic_loss(w.astype(np.float64), f64[sl], live, adv[sl], L, 16.0, 1.0, 1.0)
        r32 = C.critic_loss(w, f32[sl], live, adv[sl], L, 16.0, 1.0, 1.0, np.float32)
        got = snaps_l[e][1][off:off + 161].cpu()
        b = R.tensor_bound(R.max_err(_t(r32["grads"]), _t(r64["grads"])), _t(r64["grads"]), relative_scale=True)
        err = R.max_err(got, _t(r64["grads"]))
        print(f"[decision critic trainer epoch {e}] L={L}, critic gradient err {err:.3e} (bound {b:.3e})")
        assert L > 0 and err <= b and float(np.abs(r64["grads"]).max()) > 0
        last = r64
    assert not bool(snaps_l[0][0][off + 144:off + 161].any()) and bool(snaps_l[1][0][off + 144:off + 161].any())
    rep = {k: float(v) for k, v in tl.last["decision"].items()}
    assert abs(rep["critic_loss"] - last["loss"]) <= 1e-5 * max(1.0, abs(last["loss"]))
    assert abs(rep["explained_variance"] - last["explained_variance"]) <= 1e-4 * max(1.0, abs(last["explained_variance"]))
    assert rep["value_mean"] == 0.0                                                # the values the advantages were formed with
    assert all(isinstance(tl.last["decision"][k], torch.Tensor) and tl.last["decision"][k].dim() == 0
               for k in ("critic_loss", "explained_variance", "value_mean"))


def test_a_hand_set_critic_shifts_the_advantage_the_policy_term_reads():
    """A non-zero critic: ``adv_dec == adv_raw + delay_scale * value`` with the value of the rollout's parameters, the
    statistics are those of ``adv_dec``, and the logits' gradient of every epoch ``==`` the entropy term's plus
    ops.graphdist_decision_ppo called on that ``adv_dec``."""
    import test_gpu_decision_credit as TD
    from tarl_hip import ops
    w0 = C.weights(7)
    tr, net = _trainer("learned", critic=w0)
    snaps, g_seen = TD._record_steps(tr)
    tr.train_iteration()
    eng, N, M, T = tr.eng, tr.eng.N, tr.M, tr.temperature
    off = tr._dcritic_off
    assert torch.equal(snaps[0][0][off:off + 161].cpu(), torch.from_numpy(w0))
    dist, dslot = tr._decision_dist
    value, adv_dec = ops.decision_critic_forward(eng.plan, tr.obs_mb, tr.head_keep, tr.frames_left, dist, dslot,
                                                 _weights(ops, w0), tr.adv_raw, timestep=eng.timestep, delay_scale=16.0)
    assert bool(value.any()) and torch.equal(value, tr.value_old) and torch.equal(adv_dec, tr.adv_dec)
    assert torch.equal(tr.adv_dec, tr.adv_raw + 16.0 * tr.value_old) and not torch.equal(tr.adv_dec, tr.adv_raw)
    stats = ops.decision_stats(tr.adv_dec, tr.head_keep)
    assert torch.equal(stats, tr._decision_stats)
    for e, idx in enumerate(tr._mb_idx):
        sl = slice(e * M, (e + 1) * M)
        params = snaps[e][0]
        w = ops.GoalMlpWeights(flat=params[tr._goal_off:tr._goal_off + ops.GOAL_MLP_PARAMS].clone())
        logits = ops.policy_goal_mlp(eng.plan, tr.obs_mb[sl], w, tr.prior_table, tr.goal_scale, dest_slot=tr.prior_dest_slot)
        choice, _ = ops.rollout_gather(eng.plan, tr.T, eng.B, False, idx, choice=tr.choice)
        proba = ops.graphdist_softmax(eng.plan, logits, T)
        g_ent = torch.full((M,), -tr.entropy_coef / M, device="cuda")
        g = ops.graphdist_logprob_entropy_bwd(eng.plan, proba, T, choice=choice, grad_log_prob=torch.zeros(M, device="cuda"),
                                              grad_entropy=g_ent)
        head = tr.head_keep[sl]
        n_live = (head > 0).sum(dtype=torch.int32).reshape(1)
        ops.graphdist_decision_ppo(eng.plan, logits, choice, head, tr.lp_old_node[sl], tr.adv_dec[sl], stats, n_live,
                                   clip_epsilon=tr.clip_epsilon, temperature=T, grad_scale=1.0, grad_logits=g)
        edge_live = (head > 0)[:, net.edge_index[0].cuda()]
        assert torch.equal(g_seen[e][edge_live], g[edge_live]) and bool(g[edge_live].any())
    assert float(tr.last["decision"]["value_mean"]) != 0.0


def test_the_trainer_refusals():
    with pytest.raises(ValueError, match="needs credit='decision'"):
        _trainer("learned", credit="joint")
    with pytest.raises(ValueError, match="credit_baseline must be"):
        _trainer("other")
    with pytest.raises(ValueError, match="decision_critic_coef"):
        _trainer("learned", decision_critic_coef=-1.0)


# ---- 4. THE TEST THAT FAILS WITHOUT THE FEATURE -----------------------------------------------------------------------------------
def test_the_critic_learns_the_learning_case_on_the_device():
    """The learning case (the spread case's last 30 frames of a segment that ends at frame 120), 200 full-batch Adam steps at
    lr 0.01 from the zero-initialised last layer, on the device: explained variance >= 0.9 EV64 and final loss <= 1.5 times
    the float64 figure (goal_mlp's rule). On the parent commit there is no critic to call."""
    from tarl_hip import ops
    c = C.learning_case()
    N, live = c["N"], c["live"]
    L = int(live.sum())
    f64 = C.features(c["ei"], N, c["obs"], c["head"], c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float64)
    _, r64 = C.adam_fit(C.init_weights(), f64, live, c["adv"], C.LEARN_STEPS, C.LEARN_LR)
    assert r64["explained_variance"] >= 0.3
    plan = ops.Plan(c["net"].edge_index, N)
    args = _dev(c)
    adv = torch.from_numpy(c["adv"]).cuda()
    nl = torch.tensor([L], dtype=torch.int32, device="cuda")
    flat = torch.from_numpy(C.init_weights().astype(np.float32)).cuda()
    grad, m, v = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    w = ops.DecisionCriticWeights(flat=flat)
    scratch = torch.empty((ops.decision_critic_scratch_bytes(plan, live.shape[0]) + 7) // 8, dtype=torch.float64, device="cuda")
    kw = dict(timestep=c["timestep"], delay_scale=16.0, coef=1.0, grad_scale=1.0, scratch=scratch)
    first = None
    for step in range(1, C.LEARN_STEPS + 1):
        grad.zero_()
        out5 = ops.decision_critic_loss(plan, *args, w, adv, nl, grads=grad, **kw)
        first = out5.sum(0).cpu() if first is None else first
        ops.adam_step_(flat, grad, m, v, step, lr=C.LEARN_LR)
    s = ops.decision_critic_loss(plan, *args, w, adv, nl, **kw).sum(0).cpu()
    den = float(s[3] - s[2] * s[2] / s[1])
    ev, loss = 1.0 - float(s[4]) / den, float(s[0] / s[1])
    print(f"[decision critic learning case] device EV {ev:.4f} (float64 {r64['explained_variance']:.4f}), loss "
          f"{float(first[0] / first[1]):.5f} -> {loss:.5f} (float64 {r64['loss']:.5f})")
    assert float(s[1]) == L
    assert ev >= 0.9 * r64["explained_variance"]
    assert loss <= 1.5 * r64["loss"]


# ---- 5. CLI end to end ----------------------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-300"
NEW_KEYS = {"train/credit_baseline", "train/decision_critic_loss", "train/decision_explained_variance",
            "train/decision_value_mean"}


def _main(argv):
    import importlib
    importlib.import_module("main").main(argv)


def test_cli_train_end_to_end(tmp_path):
    run, ref = tmp_path / "run", tmp_path / "ref"
    base = ["--algo", "mpnn+ppo", "--mode", "train", "--scenario", SCENARIO, "--policy-head", "goal_mlp", "--policy-hold",
            "--route-departures", "--rollout-steps", "256", "--iterations", "2", "--steps", "5", "--credit", "decision"]
    _main(base + ["--credit-baseline", "learned", "--credit-critic-coef", "0.5", "--output-dir", str(run)])
    _main(base + ["--output-dir", str(ref)])
    logs = [json.loads(l) for l in open(run / "train_log.jsonl")]
    old = [json.loads(l) for l in open(ref / "train_log.jsonl")]
    assert len(logs) == 2 and len(old) == 2
    assert set(logs[0]) - set(old[0]) == NEW_KEYS and set(old[0]) <= set(logs[0])
    for rec, o in zip(logs, old):
        assert NEW_KEYS <= set(rec) and not NEW_KEYS & set(o)
        assert rec["train/credit_baseline"] == "learned" and rec["train/credit"] == "decision"
        assert all(np.isfinite(rec[k]) for k in NEW_KEYS - {"train/credit_baseline"})
        assert rec["train/decision_critic_loss"] >= 0.0 and rec["train/decision_explained_variance"] <= 1.0
    # iteration 0: the same frames, and with the zero-initialised last layer the same update of the policy
    for k in ("PPO/avg_episode_return", "train/held", "train/decisions", "train/decision_delay_frames", "train/decision_kl",
              "train/decision_clip_fraction"):
        assert logs[0][k] == old[0][k], k
    assert logs[0]["train/decision_value_mean"] == 0.0
    a, b = torch.load(run / "policy.pt", map_location="cpu"), torch.load(ref / "policy.pt", map_location="cpu")
    assert list(a) == list(b)                                                      # the critic is not saved, as no critic is


def test_cli_refusals():
    for argv, msg in ((["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit-baseline", "learned"],
                       "needs credit decision"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit-critic-coef", "0.5"],
                       "needs credit decision"),
                      (["--algo", "mpnn+ppo", "--mode", "train", "--credit", "decision", "--credit-baseline", "learned"],
                       "state-dependent head"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--credit", "decision", "--credit-baseline",
                        "learned"], "mode 'train'")):
        with pytest.raises(ValueError, match=msg):
            _main(argv + ["--scenario", SCENARIO])
