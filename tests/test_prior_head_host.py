"""CPU: the shortest-path prior head (policy_head = "embedding_dijkstra", csrc/prior.hip) at the interfaces — CLI flags,
C-ABI symbols, host-side argument checks (before any HIP call) and the Python layers' refusal of host tensors. No GPU
compute happens here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import PKG, ROOT
from fake_plan import fake_plan as _plan

NEW = ("tarl_policy_prior_logits", "tarl_fused_prior_logits", "tarl_fused_rollout_prior")


@pytest.fixture(scope="module")
def L():
    from tarl_hip import lib
    return lib.load()


def test_cli_accepts_the_prior_head():
    import sys
    sys.path.insert(0, PKG)
    import main
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--policy-head", "embedding_dijkstra", "--prior-weight", "0.5"])
    assert ns.policy_head == "embedding_dijkstra" and ns.prior_weight == 0.5
    assert main.build_parser().parse_args([]).prior_weight == 1.0
    from src.runner import RunnerArgs
    a = RunnerArgs(**vars(ns))
    assert a.policy_head == "embedding_dijkstra" and a.prior_weight == 0.5


def test_new_entry_points_are_declared_exported_and_bound():
    from tarl_hip import lib
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in lib.SIGNATURES, name
    assert re.search(r"#define TARL_ABI_VERSION 5\b", header)


def test_observation_entry_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    ok = [pp, fake, 4, fake, 100, fake, 100, ctypes.c_float(1.0), fake, null]
    for i in (0, 1, 3, 5, 8):
        args = list(ok)
        args[i] = null
        assert L.tarl_policy_prior_logits(*args) == -1, i
        assert b"null" in L.tarl_last_error(), i
    for i, v, msg in ((2, 0, b"bad sizes"), (4, 0, b"bad sizes"), (6, 99, b"not N x N"), (6, 101, b"not N x N"),
                      (7, ctypes.c_float(-0.5), b"prior_weight"), (7, ctypes.c_float(float("inf")), b"prior_weight"),
                      (7, ctypes.c_float(float("nan")), b"prior_weight"), (1, ctypes.c_void_p(0x1004), b"aligned")):
        args = list(ok)
        args[i] = v
        assert L.tarl_policy_prior_logits(*args) == -1, (i, v)
        assert msg in L.tarl_last_error(), (i, L.tarl_last_error())


def test_fused_entries_reject_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    w = ctypes.c_float(1.0)
    # plan, f, x, B, x_bstride, ldx, Nmax, ag, A, a_bstride, emb, M, dist, dist_n, w, logits, stream
    ok = [pp, fake, fake, 8, 0, 0, 15, fake, 50, 450, fake, 100, fake, 100, w, fake, null]
    for i in (0, 1, 2, 7, 10, 12, 15):
        args = list(ok)
        args[i] = null
        assert L.tarl_fused_prior_logits(*args) == -1, i
        assert b"null" in L.tarl_last_error(), i
    for i, v, msg in ((13, 64, b"not N x N"), (3, 0, b"bad sizes"), (8, 0, b"bad sizes"), (14, ctypes.c_float(-1), b"prior_weight")):
        args = list(ok)
        args[i] = v
        assert L.tarl_fused_prior_logits(*args) == -1, i
        assert msg in L.tarl_last_error(), i
    times = (ctypes.c_float * 4)(1, 2, 3, 4)
    # plan, f, B, Nmax, T, times, prev, x, xbs, ldx, ag, A, abs, ea, lea, log_eps, use_cong, emb, M, dist, dist_n, w, temp,
    # pseed, pc0, seed, c0, keep_ptr, keep_env, keep_slot, obs_keep, logits_scratch, dist_scratch, ins_scratch, choice8,
    # log_prob, reward, counts, stream
    ok = [pp, fake, 8, 15, 4, times, ctypes.c_float(0), fake, 0, 0, fake, 50, 450, fake, fake, ctypes.c_float(0), 1, fake,
          100, fake, 100, w, ctypes.c_float(1), 0, 0, 0, 0, null, null, null, null, fake, fake, fake, null, null, null, null,
          null]
    for i, v, msg in ((19, null, b"null"), (20, 99, b"not N x N"), (17, null, b"null"), (0, null, b"null")):
        args = list(ok)
        args[i] = v
        assert L.tarl_fused_rollout_prior(*args) == -1, i
        assert msg in L.tarl_last_error(), i


def test_python_layer_refuses_host_tensors():
    from tarl_hip import lib, ops

    class _P:
        num_nodes, num_edges, handle = 4, 8, None
    obs = torch.zeros((1, 4, 16))
    emb = torch.zeros(4)
    table = torch.zeros((4, 4))
    with pytest.raises(lib.TarlError):
        ops.policy_prior_logits(_P(), obs, emb, table)
    with pytest.raises(lib.TarlError):
        ops.fused_prior_logits(_P(), None, obs, 1, None, emb, table)


def test_trainer_and_dispatch_know_the_head():
    import inspect
    from tarl_hip.trainer import VecPPOTrainer
    sig = inspect.signature(VecPPOTrainer.__init__)
    assert sig.parameters["prior_weight"].default == 1.0 and sig.parameters["prior_table"].default is None
    import sys
    sys.path.insert(0, PKG)
    from src.agents.mpnn_agent import MPNNPolicyNet
    assert MPNNPolicyNet.policy_head == "embedding" and MPNNPolicyNet.prior_weight == 1.0
    src = inspect.getsource(__import__("src.rl.ppo_trainer", fromlist=["ppo_train"]).ppo_train)
    assert "embedding_dijkstra" in src and "prior_table" in src


def test_trainer_refuses_lazy_log_prob_for_state_dependent_heads():
    """lazy_log_prob re-evaluates the embedding head's tables at update time: both state-dependent heads refuse it up
    front (checked before the engine is touched, so a stand-in engine suffices)."""
    import types
    from tarl_hip.trainer import VecPPOTrainer
    eng = types.SimpleNamespace(fs=object(), N=4)
    mlp = [torch.zeros(1) for _ in range(6)]
    for kw in (dict(policy="edge_mlp", edge_mlp_params=mlp, extra_params=mlp),
               dict(policy="embedding_dijkstra", prior_table=torch.zeros(4, 4))):
        with pytest.raises(ValueError, match="lazy_log_prob"):
            VecPPOTrainer(eng, torch.zeros(4, 1), [], rollout_steps=4, lazy_log_prob=True, **kw)
