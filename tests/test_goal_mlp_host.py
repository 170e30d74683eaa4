"""CPU: the goal-conditioned policy head (policy_head = "goal_mlp", csrc/goal_mlp.hip) — its features, forward and backward
restated (``goal_mlp_restatement``), the float64 backward against torch autograd, what each named defect would do instead on
a crafted case, the conditions the crafted inputs must meet, and the host side: the C-ABI entry points (bound, validated
before any HIP call, ABI number unchanged) and the wrapper's refusals that need no device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import goal_mlp_restatement as G
import irregular_graphs as IG
from fake_plan import fake_plan as _plan
from update_restatement import tensor_bound

GRAPHS = ("torus", "MIXED", "HUB126")


def _net(name):
    from tarl_hip import synth
    return synth.torus_network(8, 8) if name == "torus" else IG.graph(name)


@pytest.fixture(scope="module")
def cases():
    """Per graph: net, all-pairs table, S, observations (M = 3), weights; the torus is homogeneous (ties in c abound)."""
    out = {}
    for i, name in enumerate(GRAPHS):
        net = _net(name)
        table, S = G.free_flow_table(net)
        ei = net.edge_index.numpy()
        obs, table, u0, u1 = G.craft(ei, G.random_obs(net, 3, seed=10 + i), table)
        out[name] = types.SimpleNamespace(net=net, ei=ei, table=table, S=S, obs=obs, w=G.weights(20 + i), u0=u0, u1=u1)
    return out


def _hub(cs, deg):
    dout = np.bincount(cs.ei[0], minlength=cs.net.num_roads)
    return int(np.nonzero(dout == deg)[0][0])


# ---- 1. the crafted inputs meet their conditions ----------------------------------------------------------------------------
def test_crafted_cases_hold_what_they_claim(cases):
    t, m, h = cases["torus"], cases["MIXED"], cases["HUB126"]
    assert not bool((m.ei[0][1:] >= m.ei[0][:-1]).all())                                  # unsorted edge list
    dout = {k: np.bincount(c.ei[0], minlength=c.net.num_roads) for k, c in cases.items()}
    assert 9 in dout["MIXED"] and 126 in dout["HUB126"] and 0 in dout["MIXED"]            # hubs and dead ends
    for name, cs in cases.items():
        g, reach = G.features(cs.obs, cs.ei, cs.table, cs.S)
        assert np.isfinite(g).all() and g.dtype == np.float32
        pre = G.hidden(g, cs.w, np.float32)
        assert (pre > 1e-3).any() and (pre < -1e-3).any()                                 # pre-activations on both sides of 0
        assert (cs.obs[..., 1] == 0).any() and (g[..., 6] == 1).any()                     # an empty source road
    # ties in c: a homogeneous torus with equal counts has candidates of equal cost that are both the minimum
    obs = t.obs.copy()
    obs[..., 1] = 2.0
    g, reach = G.features(obs, t.ei, t.table, t.S)
    zeros = np.zeros((3, t.net.num_roads))
    np.add.at(zeros, (np.repeat(np.arange(3), t.ei.shape[1]), np.tile(t.ei[0], 3)), (g[..., 0] == 0).reshape(-1))
    assert (zeros >= 2).any()
    # every graph: a node whose candidates are all unreachable, and one with exactly one reachable candidate (its g0 = 0)
    for cs in cases.values():
        g, reach = G.features(cs.obs, cs.ei, cs.table, cs.S)
        assert not reach[:, cs.ei[0] == cs.u0].any() and (reach[:, cs.ei[0] == cs.u1].sum(1) == 1).all()
        assert (g[:, cs.ei[0] == cs.u0, 0] == 8).all() and (g[:, cs.ei[0] == cs.u1, 0][reach[:, cs.ei[0] == cs.u1]] == 0).all()
        l = G.forward(cs.obs, cs.ei, cs.table, cs.S, cs.w)
        assert (l[~reach] == G.UNREACHABLE).all() and np.isfinite(l).all() and (np.abs(l[reach]) < 1e3).all()


def test_a_destination_without_a_column_is_unreachable(cases):
    for name, cs in cases.items():
        tab, slot = G.per_destination(cs.table, cs.obs)
        full = G.forward(cs.obs, cs.ei, cs.table, cs.S, cs.w)
        assert np.array_equal(G.forward(cs.obs, cs.ei, tab, cs.S, cs.w, slot=slot), full)
        gone = int(cs.obs[0, cs.ei[0][0], 8])
        tab2, slot2 = G.per_destination(cs.table, cs.obs, drop=(gone,))
        l = G.forward(cs.obs, cs.ei, tab2, cs.S, cs.w, slot=slot2)
        hit = cs.obs[:, cs.ei[0], 8].astype(np.int64) == gone
        assert hit.any() and (l[hit] == G.UNREACHABLE).all() and np.array_equal(l[~hit], full[~hit])


# ---- 2. the float64 backward is the gradient -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_float64_backward_equals_autograd(cases, name):
    cs = cases[name]
    gl = np.random.default_rng(3).standard_normal((3, cs.ei.shape[1]))
    got = G.backward(cs.obs, cs.ei, cs.table, cs.S, cs.w, gl)
    ref = G.torch_backward(cs.obs, cs.ei, cs.table, cs.S, cs.w, gl)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # fp32 and float64 agree to fp32 accuracy
    l32, l64 = G.forward(cs.obs, cs.ei, cs.table, cs.S, cs.w), G.forward(cs.obs, cs.ei, cs.table, cs.S, cs.w, dt=np.float64)
    ok = l32 != G.UNREACHABLE
    assert np.array_equal(ok, l64 != np.float64(G.UNREACHABLE)) and np.abs(l32[ok] - l64[ok]).max() < 1e-4


# ---- 3. one defect at a time ---------------------------------------------------------------------------------------------------
def _nan_cost_case(cs):
    """An out-edge whose cost is NaN (0 / 0 in the congestion time): NUMBER_OF_AGENT = MAXN + 10 and MAX_FLOW such that
    MAX_FLOW * FF / 3600 = MAXN + 10 exactly (FF = 3600 / 64 s is a power-of-two fraction of 3600)."""
    obs = cs.obs.copy()
    u = _hub(cs, 9) if 9 in np.bincount(cs.ei[0]) else int(cs.ei[0][0])
    v = int(cs.ei[1][np.nonzero(cs.ei[0] == u)[0][1]])
    obs[:, v, 0], obs[:, v, 1], obs[:, v, 2], obs[:, v, 4] = 6.0, 16.0, 56.25, 1024.0
    obs[:, u, 1], obs[:, u, 8] = 1.0, float(cs.ei[1][np.nonzero(cs.ei[0] == u)[0][0]])
    return obs, u


FEATURE_DEFECTS = {"cmin_first4": "MIXED", "cmin_tile64": "HUB126", "cmin_unreachable": "MIXED", "dest_of_v": "torus",
                   "table_transposed": "torus", "slot_ignored": "MIXED", "g3_g4_swapped": "torus"}


@pytest.mark.parametrize("defect,name", sorted(FEATURE_DEFECTS.items()))
def test_each_feature_defect_changes_its_named_case(cases, defect, name):
    """The device test demands equality of the features and logits, so any change is seen; each defect moves a feature by
    more than 1e-3 on the rows the case was made for."""
    cs = cases[name]
    obs, slot, table = cs.obs, None, cs.table
    rows = np.ones(cs.ei.shape[1], dtype=bool)
    if defect == "cmin_first4":          # the 9-hub: make one of its out-edges of rank >= 4 the cheapest (the destination itself)
        obs = obs.copy()
        u = _hub(cs, 9)
        outs = np.nonzero(cs.ei[0] == u)[0]
        obs[:, u, 1], obs[:, u, 8] = 1.0, float(cs.ei[1][outs[6]])
        rows = cs.ei[0] == u
    elif defect == "cmin_tile64":        # the 126-hub: its list straddles a 64-position tile whatever its start
        obs = obs.copy()
        u = _hub(cs, 126)
        outs = np.nonzero(cs.ei[0] == u)[0]
        obs[:, u, 1] = 1.0
        obs[0, u, 8], obs[1, u, 8], obs[2, u, 8] = (float(cs.ei[1][outs[k]]) for k in (0, 70, 125))
        rows = cs.ei[0] == u
    elif defect == "cmin_unreachable":
        obs, u = _nan_cost_case(cs)
        rows = cs.ei[0] == u
    elif defect == "slot_ignored":
        table, slot = G.per_destination(cs.table, obs)
    good, reach = G.features(obs, cs.ei, table, cs.S, slot)
    bad, _ = G.features(obs, cs.ei, table, cs.S, slot, defect=defect)
    assert np.isfinite(good).all()
    with np.errstate(invalid="ignore"):
        diff = np.abs(good[:, rows] - bad[:, rows])
    assert np.nanmax(np.where(np.isnan(diff), np.inf, diff)) > 1e-3, defect
    if defect == "cmin_tile64":          # every sample's minimum lies in one tile, so the other tile's edges are wrong in each
        assert all(np.abs(good[m, rows] - bad[m, rows]).max() > 1e-3 for m in range(3))


def test_unreachable_edges_carry_the_sentinel_exactly(cases):
    cs = cases["MIXED"]
    good = G.forward(cs.obs, cs.ei, cs.table, cs.S, cs.w)
    bad = G.forward(cs.obs, cs.ei, cs.table, cs.S, G.weights(1, sharp=True) * 1e10, defect="unreachable_mlp_minus_1e20")
    ref = G.forward(cs.obs, cs.ei, cs.table, cs.S, G.weights(1, sharp=True) * 1e10)
    un = good == G.UNREACHABLE
    assert un.any() and (ref[un] == G.UNREACHABLE).all() and (bad[un] != G.UNREACHABLE).any()


BACKWARD_DEFECTS = ("unreachable_grad_counted", "relu_mask_no_bias", "dw1_per_sample_mean")


@pytest.mark.parametrize("defect", BACKWARD_DEFECTS)
@pytest.mark.parametrize("name", ("MIXED", "HUB126"))
def test_each_backward_defect_exceeds_ten_times_the_device_bound(cases, defect, name):
    """The device test compares with the float64 gradient within tensor_bound(e32, ref, relative_scale=True), e32 the error
    of the fp32 restatement: each defect moves the gradient by at least ten times that."""
    cs = cases[name]
    gl = np.random.default_rng(4).standard_normal((3, cs.ei.shape[1]))
    ref = G.backward(cs.obs, cs.ei, cs.table, cs.S, cs.w, gl)
    r32 = G.backward(cs.obs, cs.ei, cs.table, cs.S, cs.w, gl, dt=np.float32)
    bound = tensor_bound(np.abs(r32.astype(np.float64) - ref).max(), torch.tensor(ref), relative_scale=True)
    bad = G.backward(cs.obs, cs.ei, cs.table, cs.S, cs.w, gl, defect=defect)
    assert np.abs(bad - ref).max() >= 10 * bound, (defect, np.abs(bad - ref).max(), bound)


# ---- 4. the host side ----------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host():
    from tarl_hip import lib
    L = lib.load()
    null = None
    assert L.tarl_abi_version() == 5
    p = _plan(300, 1200)
    P = ctypes.byref(p)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a16 = (a + 15) // 16 * 16
    # null arguments
    assert L.tarl_policy_goal_features(null, a16, 1, a16, 300, null, 1.0, a16, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_policy_goal_features(P, a16, 1, null, 300, null, 1.0, a16, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_policy_goal_features(P, a16, 1, a16, 300, null, 1.0, null, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_policy_goal_mlp_fwd(P, a16, 1, a16, 300, null, 1.0, null, a16, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_policy_goal_mlp_bwd(P, a16, 1, a16, 300, null, 1.0, a16, a16, a16, null, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_fused_goal_mlp_logits(P, null, a16, 1, 0, 52, 15, a16, 1, 9, a16, 300, null, 1.0, a16, a16, null) == -1
    assert b"null" in L.tarl_last_error()
    # sizes, the time scale, the table's columns
    assert L.tarl_policy_goal_mlp_fwd(P, a16, 0, a16, 300, null, 1.0, a16, a16, null) == -1 and b"bad sizes" in L.tarl_last_error()
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert L.tarl_policy_goal_mlp_fwd(P, a16, 1, a16, 300, null, s, a16, a16, null) == -1
        assert b"time_scale" in L.tarl_last_error()
    assert L.tarl_policy_goal_mlp_fwd(P, a16, 1, a16, 299, null, 1.0, a16, a16, null) == -1 and b"N x N" in L.tarl_last_error()
    assert L.tarl_policy_goal_mlp_fwd(P, a16, 1, a16, 0, a16, 1.0, a16, a16, null) == -1 and b"column" in L.tarl_last_error()
    # alignment
    assert L.tarl_policy_goal_mlp_fwd(P, a16 + 4, 1, a16, 300, null, 1.0, a16, a16, null) == -1
    assert b"obs16 must be 16-byte aligned" in L.tarl_last_error()
    assert L.tarl_policy_goal_mlp_bwd(P, a16, 1, a16, 300, null, 1.0, a16, a16, a16, a16 + 4, null) == -1
    assert b"scratch must be 16-byte aligned" in L.tarl_last_error()
    assert L.tarl_policy_goal_features(P, a16, 1, a16, 300, null, 1.0, a16 + 8, null) == -1 and b"feats" in L.tarl_last_error()
    # too many pairs / tiles for a grid dimension
    assert L.tarl_policy_goal_mlp_fwd(P, a16, 1 << 40, a16, 300, null, 1.0, a16, a16, null) == -1 and b"grid" in L.tarl_last_error()
    assert L.tarl_fused_goal_mlp_logits(P, a16, a16, 65536 * 64, 0, 52, 15, a16, 1, 9, a16, 300, null, 1.0, a16, a16, null) == -1
    assert b"grid" in L.tarl_last_error()
    # the rollout entry point checks the same
    args = [P, null, 1, 15, 1, null, 0.0, a16, 0, 52, a16, 1, 9, null, null, 0.0, 0, a16, 300, null, 1.0, a16, 1.0, 0, 0, 0, 0]
    assert L.tarl_fused_rollout_goal(*args, *([null] * 12)) == -1 and b"null" in L.tarl_last_error()
    # the scratch size: 161 floats per partition, partitions = tiles of 256 pairs up to 1024, then equal runs of tiles
    q = L.tarl_policy_goal_mlp_bwd_scratch_floats
    assert q(null, 1) == -1 and q(P, 0) == -1 and q(P, 1 << 50) == -1
    assert q(P, 1) == 5 * 161 and q(P, 3) == 15 * 161                                     # 1200 pairs: 5 tiles
    assert q(P, 1000) == 938 * 161                                                        # 4688 tiles: 5 per partition
    assert not any(buf)                                                                   # a refused call writes nothing


def test_wrapper_sizes_and_refusals_without_a_device():
    from tarl_hip import lib, ops
    p = _plan(300, 1200)
    plan = types.SimpleNamespace(handle=ctypes.byref(p), num_nodes=300, num_edges=1200)
    L = lib.load()
    for M in (1, 3, 64, 65, 1000, 4096):
        assert ops.goal_mlp_bwd_scratch_floats(plan, M) == L.tarl_policy_goal_mlp_bwd_scratch_floats(plan.handle, M)
    with pytest.raises(ValueError):
        ops.goal_mlp_bwd_scratch_floats(plan, 0)
    assert ops.GOAL_MLP_PARAMS == G.NW == 161
    assert ops.GOAL_MLP_KEYS == ("goal_mlp.0.weight", "goal_mlp.0.bias", "goal_mlp.2.weight", "goal_mlp.2.bias")
    with pytest.raises(ValueError, match="8 -> 16 -> 1"):
        ops.GoalMlpWeights(torch.zeros(16, 9), torch.zeros(16), torch.zeros(1, 16), torch.zeros(1))
    # the time scale: the float64 mean of FREE_FLOW rounded to fp32
    x = torch.zeros(5, 7)
    x[:, 2] = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.7])
    assert ops.goal_time_scale(x) == float(np.float32(x[:, 2].double().mean().item()))
    assert ops.goal_time_scale(x.unsqueeze(0).repeat(2, 1, 1)) == ops.goal_time_scale(x)
    with pytest.raises(ValueError, match="finite and > 0"):
        ops.goal_time_scale(torch.zeros(5, 7))
    # no CPU fall-back: host tensors are refused
    with pytest.raises(lib.TarlError):
        ops.policy_goal_mlp(plan, torch.zeros(1, 300, 16), None, torch.zeros(300, 300), 1.0)


# ---- 5. the Python layers ------------------------------------------------------------------------------------------------------
def test_parser_and_argument_rules():
    import importlib
    main = importlib.import_module("main")
    from src.runner import RunnerArgs
    from tarl_hip import evaluator
    p = main.build_parser()
    assert p.parse_args([]).policy_head == "embedding"
    for method in ("all_pairs", "per_destination", "auto"):
        ns = p.parse_args(["--algo", "mpnn+ppo", "--policy-head", "goal_mlp", "--prior-method", method])
        a = RunnerArgs(**vars(ns))
        assert a.policy_head == "goal_mlp" and a.prior_method == method
    with pytest.raises(SystemExit):
        p.parse_args(["--policy-head", "goal"])
    assert "goal_mlp" in evaluator.HEADS and "goal_mlp" not in evaluator.ROUTER_HEADS + evaluator.PLAN_HEADS
    # a state-dependent head: accepted by --policy-hold in training and by the graph-transformer critic
    RunnerArgs(algo="mpnn+ppo", scenario="synthetic-64-16", mode="train", policy_head="goal_mlp", policy_hold=True)
    RunnerArgs(algo="mpnn+ppo", scenario="synthetic-64-16", mode="train", policy_head="goal_mlp", value_head="graph_transformer")
    with pytest.raises(ValueError, match="goal_mlp"):
        RunnerArgs(algo="mpnn+ppo", scenario="synthetic-64-16", mode="train", policy_head="embedding", policy_hold=True)


def test_state_dict_is_unchanged_without_the_head():
    from src.agents.mpnn_agent import MPNNPolicyNet
    from tarl_hip import ops, synth
    net = synth.torus_network(3, 3)
    pol = MPNNPolicyNet(net.edge_index, net.num_roads, None, device="cpu")
    today = ["nodes_embedding.weight"] + [f"edge_mlp_test.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")] + \
        [f"edge_mlp.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")]
    assert list(pol.state_dict()) == today and not hasattr(pol, "goal_mlp") and not hasattr(pol, "goal_scale")
    S = ops.goal_time_scale(net.x[:, 3 * net.Nmax:])
    pol.use_goal_mlp(S)
    assert sorted(pol.state_dict()) == sorted(today + list(ops.GOAL_MLP_KEYS) + ["goal_scale"])
    assert [n for n, _ in pol.named_parameters()] == today + list(ops.GOAL_MLP_KEYS)      # one run of the flat buffer
    assert pol.policy_head == "goal_mlp" and float(pol.goal_scale) == S
    assert sum(pol.state_dict()[k].numel() for k in ops.GOAL_MLP_KEYS) == ops.GOAL_MLP_PARAMS
    m = pol.goal_mlp
    assert float(m[0].weight.detach().abs().max()) <= 0.1 and float(m[2].weight.detach().abs().max()) <= 0.1
    assert not bool(m[0].bias.any()) and not bool(m[2].bias.any())
    fresh = MPNNPolicyNet(net.edge_index, net.num_roads, None, device="cpu")
    with pytest.raises(RuntimeError):
        fresh.load_state_dict(pol.state_dict())                                  # a checkpoint of another head is refused
    for bad in (0.0, float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError, match="time_scale"):
            fresh.use_goal_mlp(bad)


def test_the_loop_learns_the_router_where_agents_are_bound_anywhere():
    """The case DESIGN 4.21 reports at chance: destinations over all roads, ``free_flow`` expert, ``expert`` driver, 60
    frames, K = 3, 50 full-batch float64 Adam steps at lr 0.05. The goal head: nll 1.4057 -> 0.3743, accuracy on the 8 851
    labelled rows 0.945; the embedding head under the same loop (the control): 1.6697 -> 1.0275, accuracy 0.503. The device
    test takes its thresholds (0.9 x accuracy, 1.5 x nll) from this run."""
    r = G.anywhere_run()
    goal, emb = r["goal"], r["embedding"]
    print(f"[goal bc anywhere, float64] {goal['labelled']} labelled rows; goal nll {goal['nll'][0]:.4f} -> {goal['nll'][-1]:.4f}, "
          f"accuracy {goal['acc'][0]:.3f} -> {goal['acc'][-1]:.3f}; embedding nll {emb['nll'][0]:.4f} -> {emb['nll'][-1]:.4f}, "
          f"accuracy {emb['acc'][0]:.3f} -> {emb['acc'][-1]:.3f}; expert arrivals {r['arrivals']}")
    assert goal["labelled"] == emb["labelled"] > 5000
    assert goal["acc"][-1] >= 0.9 and goal["nll"][-1] <= 0.5 * goal["nll"][0]
    assert goal["acc"][-1] >= emb["acc"][-1] + 0.3                               # well above the control
    assert emb["acc"][-1] <= 0.6
