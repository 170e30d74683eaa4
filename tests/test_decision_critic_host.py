"""CPU: the learned per-decision critic on its restatement — the float64 backward against torch autograd, the
crafted cases by hand on the torus, MIXED and HUB126, every named defect against ten times the tolerance the GPU tests
use, the learning case in float64 (EV64), the host checks of the four entry points, the scratch-size rule, and the argument
rules of the layers."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import decision_critic_restatement as C
import update_restatement as R
from fake_plan import fake_plan as _plan

GRAPHS = {"torus8": (), "MIXED": (4, 8), "HUB126": (0, 70, 125)}


def _net(name):
    if name == "torus8":
        from tarl_hip import synth
        return synth.torus_network(8, 8)
    import irregular_graphs
    return irregular_graphs.graph(name)


_CASES = {}


def _case(name):
    if name not in _CASES:
        net = _net(name)
        _CASES[name] = C.crafted_case(net.edge_index.numpy(), net.num_roads, seed=len(name), hub_ranks=GRAPHS[name])
    return _CASES[name]


def _feats(c, dtype=np.float64, defect=None, mask=None):
    return C.features(c["ei"], c["N"], c["obs"], c["head"], c["frames_left"], c["dist"], c["slot"], c["timestep"], dtype, mask,
                      defect)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---- 1. the backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharp", [False, True])
def test_float64_backward_matches_autograd(sharp):
    c = _case("MIXED")
    f = _feats(c)
    w = C.weights(3, sharp).astype(np.float64)
    L = int(c["live"].sum())
    r = C.critic_loss(w, f, c["live"], c["adv"], L, 16.0, 0.75, 0.5)
    wt = _t(w).requires_grad_(True)
    ft, live = _t(f), torch.from_numpy(c["live"])
    pre = ft @ wt[:128].view(16, 8).t() + wt[128:144]
    val = pre.clamp(min=0) @ wt[144:160] + wt[160]
    y = -_t(c["adv"]) / 16.0
    e = val - y
    sl1 = torch.where(e.abs() < 1, 0.5 * e * e, e.abs() - 0.5)
    loss = 0.75 / L * sl1[live].sum()
    (0.5 * loss).backward()
    assert abs(float(loss.detach()) - r["loss"]) < 1e-12
    assert float((wt.grad - _t(r["grads"])).abs().max()) < 1e-12
    e_np = (r["value"] - r["y"])[c["live"]]
    assert (np.abs(e_np) > 1).any() and (sharp or (np.abs(e_np) < 1).any())     # both branches of the loss
    pre_live = pre.detach().numpy()[c["live"]]
    assert (pre_live > 0).any() and (pre_live < 0).any()                        # both sides of the ReLU


# ---- 2. the crafted cases by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_crafted_cases_by_hand(name):
    c = _case(name)
    f = _feats(c)
    f32 = _feats(c, np.float32)
    nm, nb, obs = c["named"], c["nbrs"], c["obs"]
    fill = lambda m, v: float(obs[m, v, 1]) / float(obs[m, v, 0]) if obs[m, v, 0] > 0 else 0.0      # noqa: E731
    m, u = nm["tie"]
    assert f[m, u, 3] == fill(m, nb[u][0]) != fill(m, nb[u][-1])                # the first in CSR order wins
    m, u = nm["none"]
    assert f[m, u, 3] == f[m, u, 4] == f[m, u, 5] == 0.0
    m, u = nm["one"]
    assert f[m, u, 3] == f[m, u, 4] == fill(m, nb[u][1]) and f[m, u, 5] == 1.0 and fill(m, nb[u][0]) != fill(m, nb[u][1])
    m, u = nm["maxn0"]
    assert obs[m, u, 0] == 0 and obs[m, nb[u][0], 0] == 0 and f[m, u, 2] == 0.0 and f[m, u, 3] == 0.0
    assert [float(f[nm[k]][6]) for k in ("nff_below", "nff_equal", "nff_above")] == [0.0, 0.0, 1.0]
    assert [float(f[nm[k]][0]) * 64 for k in ("nff_below", "nff_equal", "nff_above")] == [39.0, 40.0, 41.0]
    m, u = nm["big"]
    assert f[m, u, 0] == 8.0 and f[m, u, 1] == 8.0 and f[m, u, 6] == 1.0       # both clamped at 512, 800 > 600
    assert float(f[..., 7].max()) == 8.0 and 0 < float(f[..., 7][c["live"]].min()) < 8.0       # FF / timestep passes 64
    for r in GRAPHS[name]:
        m, u = nm[f"hub_rank_{r}"]
        assert u == c["hub"] and f[m, u, 3] == 0.9 == fill(m, nb[u][r])
    assert not f[~c["live"]].any() and f32.dtype == np.float32
    assert float(np.abs(f32 - f).max()) < 1e-6
    if name == "HUB126":
        assert len(nb[c["hub"]]) == 126
    if name == "MIXED":
        assert len(nb[c["hub"]]) == 9


def test_zero_last_layer_gives_zero_value_and_the_raw_advantage():
    c = _case("torus8")
    f32 = _feats(c, np.float32)
    w0 = C.init_weights()
    val, adv = C.forward(w0, f32, c["live"], c["adv"])
    assert not val.any() and (adv == c["adv"]).all()
    r = C.critic_loss(w0, f32, c["live"], c["adv"], 0)                          # L = 0: nothing is added
    assert not r["grads"].any() and r["loss"] == 0.0


# ---- 3. the named defects -------------------------------------------------------------------------------------------------------
FEATURE_DEFECTS = {"vstar_first_four": ("MIXED", "hub_rank_8"), "vstar_inf_wins": ("torus8", "none"),
                   "tie_last": ("torus8", "tie"), "mean_over_all": ("torus8", "one"), "dest_of_v": ("torus8", "one"),
                   "dist_transposed": ("torus8", "nff_above"), "slot_ignored": ("torus8", "nff_above"),
                   "frames_left_next_row": ("torus8", "nff_equal")}
LOSS_DEFECTS = ("target_sign", "sl1_switch", "relu_mask_no_bias", "loss_over_mn", "count_nonlive")


@pytest.mark.parametrize("defect", list(FEATURE_DEFECTS))
def test_each_feature_defect_moves_its_named_case(defect):
    """The GPU test asks the features to equal the fp32 restatement bit for bit and to lie within ``tensor_bound`` of
    float64: each defect moves a feature of its named decision by at least ten times that bound."""
    graph, nm = FEATURE_DEFECTS[defect]
    c = _case(graph)
    good, bad, f32 = _feats(c), _feats(c, defect=defect), _feats(c, np.float32)
    bound = R.tensor_bound(R.max_err(_t(f32), _t(good)), _t(good))
    moved = float(np.abs(good[c["named"][nm]] - bad[c["named"][nm]]).max())
    print(f"[decision critic defect {defect}] {graph}/{nm} moved {moved:.3g}, bound {bound:.3g}")
    assert moved >= 10 * bound


def _loss(c, w, dtype=np.float64, defect=None):
    mask = None
    live = c["live"]
    if defect == "count_nonlive":
        mask = np.array([[len(c["nbrs"][u]) > 0 for u in range(c["N"])]] * live.shape[0])
        live = mask
    f = _feats(c, dtype, mask=mask)
    return C.critic_loss(w, f, live, c["adv"], int(c["live"].sum()), 16.0, 1.0, 0.5, dtype, defect)


@pytest.mark.parametrize("defect", LOSS_DEFECTS)
def test_each_loss_defect_moves_the_gradient_or_the_sums(defect):
    c = _case("torus8")
    w = C.weights(5)
    good, bad, r32 = _loss(c, w), _loss(c, w, defect=defect), _loss(c, w, np.float32)
    b_g = R.tensor_bound(R.max_err(_t(r32["grads"]), _t(good["grads"])), _t(good["grads"]), relative_scale=True)
    b_o = R.tensor_bound(R.max_err(_t(r32["out5"]), _t(good["out5"])), _t(good["out5"]))
    moved_g = float(np.abs(good["grads"] - bad["grads"]).max())
    moved_o = float(np.abs(good["out5"] - bad["out5"]).max())
    print(f"[decision critic defect {defect}] grads moved {moved_g:.3g} (bound {b_g:.3g}), out5 moved {moved_o:.3g} "
          f"(bound {b_o:.3g})")
    assert moved_g >= 10 * b_g
    if defect in ("target_sign", "sl1_switch", "count_nonlive"):
        assert moved_o >= 10 * b_o


def test_delay_scale_missing_from_the_advantage():
    c = _case("torus8")
    w = C.weights(5)
    f32 = _feats(c, np.float32)
    _, good = C.forward(w, f32, c["live"], c["adv"], 16.0, np.float64)
    _, a32 = C.forward(w, f32, c["live"], c["adv"], 16.0, np.float32)
    _, bad = C.forward(w, f32, c["live"], c["adv"], 16.0, np.float64, "adv_no_delay_scale")
    bound = R.tensor_bound(R.max_err(_t(a32), _t(good)), _t(good))
    assert float(np.abs(good - bad).max()) >= 10 * bound


def test_every_defect_is_covered_and_unknown_ones_are_refused():
    assert set(FEATURE_DEFECTS) | set(LOSS_DEFECTS) | {"adv_no_delay_scale"} == set(C.DEFECTS)
    with pytest.raises(ValueError, match="unknown defect"):
        _feats(_case("torus8"), defect="other")


# ---- 4. the learning case ---------------------------------------------------------------------------------------------------------
EV64_FLOOR = 0.3


def test_learning_case_in_float64():
    """The spread case on the CPU oracle, the last 30 frames of a segment that ends at frame 120: 200 full-batch Adam steps
    at lr 0.01 from the zero-initialised last layer. EV64 = 0.362, final loss 0.01351."""
    c = C.learning_case()
    L = int(c["live"].sum())
    assert L == 110 and c["truncated"] == 30                                    # a substantial share is truncated
    f = C.features(c["ei"], c["N"], c["obs"], c["head"], c["frames_left"], c["dist"], c["slot"], c["timestep"], np.float64)
    r0 = C.critic_loss(C.init_weights(), f, c["live"], c["adv"], L)
    w, r = C.adam_fit(C.init_weights(), f, c["live"], c["adv"], C.LEARN_STEPS, C.LEARN_LR)
    print(f"[decision critic learning case] EV64 {r['explained_variance']:.4f}, loss {r0['loss']:.5f} -> {r['loss']:.5f}")
    assert r["explained_variance"] >= EV64_FLOOR
    assert r["loss"] < 0.5 * r0["loss"]


# ---- 5. the host side ---------------------------------------------------------------------------------------------------------------
NEW = ("tarl_decision_critic_features", "tarl_decision_critic_fwd", "tarl_decision_critic_loss_scratch_bytes",
       "tarl_decision_critic_loss")


def test_entry_points_are_bound_and_nothing_moved():
    from tarl_hip import lib
    L = lib.load()
    assert all(n in lib.SIGNATURES and hasattr(L, n) for n in NEW)
    assert L.tarl_abi_version() == 5
    assert lib.FusedStruct._fields_[-1][0] == "policy_held"                     # tarl_fused did not grow


def _refused(L, entry, ok, nulls, bads):
    for i in nulls:
        args = list(ok)
        args[i] = None
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in bads:
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, bad, L.tarl_last_error())


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake, odd = None, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    pp = ctypes.byref(_plan(100, 400))
    common = [(2, 0, b"bad sizes"), (2, 1 << 24, b"too many"), (7, 0, b"bad sizes"), (8, 0.0, b"timestep"),
              (8, -1.0, b"timestep"), (8, float("inf"), b"timestep"), (1, odd, b"obs16")]
    # plan, obs16, M, head, frames_left, dist, dest_slot, D, timestep, feats, stream
    ok = [pp, fake, 3, fake, fake, fake, fake, 4, 1.0, fake, null]
    _refused(L, L.tarl_decision_critic_features, ok, (0, 1, 3, 4, 5, 6, 9), common + [(9, odd, b"feats")])
    # ..., timestep, weights, delay_scale, adv_raw, value, adv_out, stream
    a, b, c = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000), ctypes.c_void_p(0x4000)
    ok = [pp, fake, 3, fake, fake, fake, fake, 4, 1.0, fake, 16.0, a, b, c, null]
    _refused(L, L.tarl_decision_critic_fwd, ok, (0, 1, 3, 4, 5, 6, 9, 11, 12),
             common + [(10, 0.0, b"delay_scale"), (10, -2.0, b"delay_scale"), (10, float("nan"), b"delay_scale"),
                       (10, float("inf"), b"delay_scale"), (12, a, b"alias"), (13, a, b"alias"), (13, b, b"alias")])
    # ..., timestep, weights, delay_scale, adv_raw, n_live, coef, grad_scale, out5, grads, scratch, stream
    ok = [pp, fake, 3, fake, fake, fake, fake, 4, 1.0, fake, 16.0, fake, fake, 1.0, 1.0, fake, fake, fake, null]
    _refused(L, L.tarl_decision_critic_loss, ok, (0, 1, 3, 4, 5, 6, 9, 11, 12, 15, 17),
             common + [(10, 0.0, b"delay_scale"), (10, float("nan"), b"delay_scale"), (13, -0.5, b"coef"),
                       (13, float("nan"), b"coef"), (17, odd, b"scratch")])


def test_scratch_size_rule():
    """40 bytes per (row, tile of 256 roads) pair and 161 floats per run of ceil(pairs / 1024) pairs."""
    from tarl_hip import lib
    L = lib.load()
    size = L.tarl_decision_critic_loss_scratch_bytes
    assert size(None, 2) == -1 and size(ctypes.byref(_plan(100, 400)), 0) == -1
    assert size(ctypes.byref(_plan(100, 400)), 1 << 24) == -1
    for N, M in ((100, 1), (100, 3), (256, 65), (257, 3), (300, 1024), (300, 1025), (72, 5000)):
        pairs = M * -(-N // 256)
        per = -(-pairs // 1024)
        assert size(ctypes.byref(_plan(N, 4 * N)), M) == pairs * 40 + -(-pairs // per) * 161 * 4, (N, M)


class _P:
    num_nodes, num_edges, handle = 4, 8, None


def test_the_ops_refuse_host_tensors_and_bad_arguments():
    from tarl_hip import lib, ops
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    obs, d64 = torch.zeros(2, 4, 16), torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.decision_critic_features(_P(), obs, i32(2, 4), i32(2), d64, i32(4), timestep=1.0)
    cp = ops.decision_critic_init(seed=3)
    assert [tuple(t.shape) for t in cp] == [(16, 8), (16,), (1, 16), (1,)] and not any(bool(t.any()) for t in cp[1:])
    assert 0.05 < float(cp[0].abs().max()) < 0.1 and torch.equal(cp[0], ops.decision_critic_init(seed=3)[0])
    with pytest.raises(ValueError, match="8 -> 16 -> 1"):
        ops.DecisionCriticWeights(torch.zeros(16, 7), torch.zeros(16), torch.zeros(1, 16), torch.zeros(1))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.DecisionCriticWeights(*cp)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.decision_critic_forward(_P(), obs, i32(2, 4), i32(2), d64, i32(4), None, torch.zeros(2, 4), timestep=1.0)
    assert ops.DECISION_CRITIC_PARAMS == 161 and ops.DECISION_CRITIC_FEATURES == 8


# ---- 6. argument rules ----------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="goal_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules():
    assert _args().credit_baseline is None and _args().credit_critic_coef is None
    assert _args(credit="decision").credit_baseline is None
    assert _args(credit="decision", credit_baseline="learned", credit_critic_coef=0.5).credit_critic_coef == 0.5
    assert _args(credit="decision", credit_baseline="free_flow").credit_baseline == "free_flow"
    assert _args(credit="decision", credit_baseline="learned", reward="trip", policy_hold=True, route_departures=True,
                 pretrain_bc=2).credit_baseline == "learned"
    for kw in (dict(credit_baseline="learned"), dict(credit_baseline="free_flow"), dict(credit_critic_coef=1.0)):
        with pytest.raises(ValueError, match="needs credit decision"):
            _args(**kw)
    with pytest.raises(ValueError, match="credit_baseline must be"):
        _args(credit="decision", credit_baseline="other")
    for kw in (dict(), dict(credit_baseline="free_flow")):             # a coefficient with nothing to weigh is refused, not ignored
        with pytest.raises(ValueError, match="needs credit_baseline learned"):
            _args(credit="decision", credit_critic_coef=0.5, **kw)
    for coef in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="credit_critic_coef must be"):
            _args(credit="decision", credit_baseline="learned", credit_critic_coef=coef)
    with pytest.raises(ValueError, match="state-dependent head"):          # the refusals of credit decision stand
        _args(credit="decision", credit_baseline="learned", policy_head="embedding")


def test_parser_flags():
    import importlib
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.credit_baseline is None and ns.credit_critic_coef is None
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit",
                                         "decision", "--credit-baseline", "learned", "--credit-critic-coef", "0.25"])
    a = RunnerArgs(**vars(ns))
    assert a.credit_baseline == "learned" and a.credit_critic_coef == 0.25
    for extra in (["--credit-baseline", "learned"], ["--credit-critic-coef", "0.5"]):
        ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train"] + extra)
        with pytest.raises(ValueError, match="needs credit decision"):
            RunnerArgs(**vars(ns))
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--credit-baseline", "other"])


def test_the_layers_take_the_arguments():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.trainer import VecPPOTrainer
    p = inspect.signature(VecPPOTrainer.__init__).parameters
    assert p["credit_baseline"].default == "free_flow" and p["decision_critic_params"].default is None
    assert p["decision_critic_coef"].default == 1.0 and p["decision_delay_scale"].default == 16.0
    p = inspect.signature(ppo_train).parameters
    assert p["credit_baseline"].default == "free_flow" and p["decision_critic_coef"].default == 1.0
    with pytest.raises(ValueError, match="needs credit decision"):
        ppo_train(None, None, None, credit_baseline="learned")
    with pytest.raises(ValueError, match="credit_baseline must be"):
        ppo_train(None, None, None, credit="decision", credit_baseline="other")


def test_trainer_refusals_without_a_device():
    from tarl_hip import ops
    from tarl_hip.trainer import VecPPOTrainer
    t = VecPPOTrainer.__new__(VecPPOTrainer)
    t.decision_critic_coef, t.decision_delay_scale = 1.0, 16.0
    cp = ops.decision_critic_init()
    other = [torch.zeros(3)]
    with pytest.raises(ValueError, match="needs credit='decision'"):
        t._check_decision_critic("joint", cp, other + cp)
    with pytest.raises(ValueError, match="8 -> 16 -> 1"):
        t._check_decision_critic("decision", None, other)
    with pytest.raises(ValueError, match="8 -> 16 -> 1"):
        t._check_decision_critic("decision", cp[:3], other + cp)
    with pytest.raises(ValueError, match="part of extra_params"):
        t._check_decision_critic("decision", cp, other)
    with pytest.raises(ValueError, match="part of extra_params"):
        t._check_decision_critic("decision", cp, [cp[0], cp[1], other[0], cp[2], cp[3]])
    assert t._check_decision_critic("decision", cp, other + cp) == cp
    t.decision_critic_coef = -1.0
    with pytest.raises(ValueError, match="decision_critic_coef"):
        t._check_decision_critic("decision", cp, other + cp)
    t.decision_critic_coef, t.decision_delay_scale = 1.0, 0.0
    with pytest.raises(ValueError, match="decision_delay_scale"):
        t._check_decision_critic("decision", cp, other + cp)


def test_policy_state_keys_do_not_depend_on_the_flag():
    """The critic lives beside the policy, as every critic does: MPNNPolicyNet (what policy.pt saves) has no key of it."""
    from src.agents.mpnn_agent import MPNNPolicyNet
    from tarl_hip import synth
    net = synth.torus_network(4, 4)
    keys = set(MPNNPolicyNet(net.edge_index, net.num_roads, None, device="cpu").state_dict())
    assert keys and not any("critic" in k or "decision" in k for k in keys)
