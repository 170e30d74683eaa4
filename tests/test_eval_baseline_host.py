"""CPU: the host side of the vectorised shortest-path baseline — the argument rules of ``--eval-baseline`` and
``--dijkstra-envs``, ``paired_report`` against numpy on hand-made results, the new C-ABI entry points (bound, validated
before any HIP call, ABI number unchanged) and the host-side argument checks of the new ops."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from fake_plan import fake_plan as _plan


# ---- argument rules ----------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules_and_defaults():
    a = _args()
    assert a.eval_baseline == "none" and a.dijkstra_envs == 0 and a.eval_envs == 0
    assert _args(eval_envs=4, eval_baseline="dijkstra").eval_baseline == "dijkstra"
    assert _args(algo="mpnn", mode="eval", eval_envs=4, eval_baseline="dijkstra").eval_envs == 4
    assert _args(algo="dijkstra", mode="eval", dijkstra_envs=8).dijkstra_envs == 8
    with pytest.raises(ValueError, match="eval_envs"):
        _args(eval_baseline="dijkstra")                                   # no eval_envs
    for algo in ("dijkstra", "random"):
        with pytest.raises(ValueError):
            _args(algo=algo, mode="eval", eval_baseline="dijkstra")
        with pytest.raises(ValueError):                                   # the existing refusal of eval_envs stays
            _args(algo=algo, mode="eval", eval_envs=4, eval_baseline="dijkstra")
        with pytest.raises(ValueError):
            _args(algo=algo, mode="eval", eval_envs=4)
    for bad in ("astar", "random", "", None):
        with pytest.raises(ValueError, match="eval_baseline"):
            _args(eval_envs=4, eval_baseline=bad)
    for bad in (dict(algo="mpnn", mode="eval", dijkstra_envs=4), dict(dijkstra_envs=4), dict(algo="random", mode="eval", dijkstra_envs=4),
                dict(algo="dijkstra", mode="train", dijkstra_envs=4), dict(algo="dijkstra", mode="eval", dijkstra_envs=-1)):
        with pytest.raises(ValueError, match="dijkstra_envs"):
            _args(**bad)


def test_parser_flags():
    main = importlib.import_module("main")
    from src.runner import RunnerArgs
    ns = main.build_parser().parse_args([])
    assert ns.eval_baseline == "none" and ns.dijkstra_envs == 0
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "8", "--eval-baseline", "dijkstra"])
    assert RunnerArgs(**vars(ns)).eval_baseline == "dijkstra"
    ns = main.build_parser().parse_args(["--algo", "dijkstra", "--mode", "eval", "--dijkstra-envs", "16"])
    assert RunnerArgs(**vars(ns)).dijkstra_envs == 16
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--eval-baseline", "astar"])


def test_ppo_train_takes_the_baseline_argument():
    import inspect
    from src.rl.ppo_trainer import ppo_train
    assert inspect.signature(ppo_train).parameters["eval_baseline"].default == "none"


# ---- paired_report -----------------------------------------------------------------------------------------------------
def _result(head, ret, arrived, avg, p50, p95, *, seed=3, env_base=0, frames=120, bin_width=10.0, num_bins=720, exit_=False):
    from tarl_hip.evaluator import EvalResult
    K = len(ret)
    settings = dict(bin_width=bin_width, num_bins=num_bins, seed=seed, env_base=env_base, temperature=1.0, poll_frames=64)
    if exit_:
        return EvalResult(envs=K, head=head, deterministic=True, frames_run=64, domain_exit=True, domain_exit_frames=(0, 64),
                          settings=settings)
    return EvalResult(envs=K, head=head, deterministic=True, frames_run=frames, episode_return=list(ret),
                      arrived=list(arrived), avg_travel_time=list(avg), p50_travel_time=list(p50), p95_travel_time=list(p95),
                      settings=settings)


A = dict(ret=[-100.0, -140.5, -90.0, -120.0, -101.0], arrived=[5, 0, 7, 6, 4], avg=[50.0, None, 61.5, 47.0, 52.0],
         p50=[50.0, None, 60.0, 40.0, 50.0], p95=[90.0, None, 110.0, 80.0, 70.0])
B = dict(ret=[-80.0, -100.0, -95.5, -70.0, -88.0], arrived=[9, 3, 8, 0, 6], avg=[40.0, 45.0, 44.5, None, 39.0],
         p50=[40.0, 40.0, 50.0, None, 40.0], p95=[60.0, 70.0, 90.0, None, 50.0])


def _stats(d):
    d = np.asarray(d, dtype=np.float64)
    se = d.std(ddof=1) / math.sqrt(d.size)
    return d.mean(), d.std(ddof=1), se, (d.mean() - 1.96 * se, d.mean() + 1.96 * se)


def test_paired_report_against_numpy():
    from tarl_hip.evaluator import PAIRED_METRICS, paired_lines, paired_report, paired_scalars
    assert [n for n, _ in PAIRED_METRICS] == ["episode_return", "arrivals", "mean_travel_time", "p50_travel_time",
                                              "p95_travel_time"]
    rep = paired_report(_result("embedding", **A), _result("dijkstra", **B))
    assert rep["available"] and rep["envs"] == 5 and rep["a"] == "embedding" and rep["b"] == "dijkstra"
    m = rep["metrics"]
    mean, std, se, ci = _stats(np.asarray(A["ret"]) - np.asarray(B["ret"]))
    assert m["episode_return"] == dict(n=5, dropped=0, mean=mean, std=std, se=se, ci95=ci,
                                       ci95_kind="normal approximation, mean -+ 1.96 se")
    mean, std, se, ci = _stats(np.asarray(A["arrived"]) - np.asarray(B["arrived"]))
    assert (m["arrivals"]["n"], m["arrivals"]["mean"], m["arrivals"]["se"]) == (5, mean, se)
    # travel times: environments 1 (no arrival in a) and 3 (none in b) are dropped pairwise; n is reported
    for name, key in (("mean_travel_time", "avg"), ("p50_travel_time", "p50"), ("p95_travel_time", "p95")):
        d = [A[key][i] - B[key][i] for i in (0, 2, 4)]
        mean, std, se, ci = _stats(d)
        assert m[name]["n"] == 3 and m[name]["dropped"] == 2
        assert (m[name]["mean"], m[name]["std"], m[name]["se"], m[name]["ci95"]) == (mean, std, se, ci)
        assert "normal" in m[name]["ci95_kind"]
    text = "\n".join(paired_lines(rep))
    assert "episode_return" in text and "normal approx." in text and "n 3" in text and "2 environments without" in text
    flat = paired_scalars(rep)
    assert flat["available"] == 1 and flat["mean_travel_time/n"] == 3 and flat["episode_return/mean"] == m["episode_return"]["mean"]


def test_paired_report_small_samples():
    from tarl_hip.evaluator import paired_lines, paired_report
    one = paired_report(_result("embedding", [-10.0], [2], [30.0], [30.0], [40.0]),
                        _result("dijkstra", [-4.0], [3], [20.0], [20.0], [20.0]))
    for m in one["metrics"].values():                       # n = 1: a difference, no spread, no interval
        assert m["n"] == 1 and m["std"] is None and m["se"] is None and m["ci95"] is None
    assert one["metrics"]["episode_return"]["mean"] == -6.0 and one["metrics"]["mean_travel_time"]["mean"] == 10.0
    # one usable travel-time pair of two environments; none at all
    two = paired_report(_result("embedding", [-1.0, -2.0], [1, 0], [30.0, None], [30.0, None], [30.0, None]),
                        _result("dijkstra", [-3.0, -1.0], [1, 1], [10.0, 20.0], [10.0, 20.0], [10.0, 20.0]))
    assert two["metrics"]["episode_return"]["n"] == 2 and two["metrics"]["episode_return"]["ci95"] is not None
    assert two["metrics"]["mean_travel_time"]["n"] == 1 and two["metrics"]["mean_travel_time"]["ci95"] is None
    none = paired_report(_result("embedding", [-1.0, -2.0], [0, 0], [None, None], [None, None], [None, None]),
                         _result("dijkstra", [-3.0, -1.0], [1, 1], [10.0, 20.0], [10.0, 20.0], [10.0, 20.0]))
    tm = none["metrics"]["p95_travel_time"]
    assert tm["n"] == 0 and tm["mean"] is None and tm["ci95"] is None
    assert any("no usable pair" in line for line in paired_lines(none))


def test_paired_report_refusals_and_domain_exit():
    from tarl_hip.evaluator import paired_lines, paired_report, paired_scalars
    a = _result("embedding", **A)
    for kw, what in ((dict(seed=4), "seed"), (dict(env_base=8), "env_base"), (dict(frames=121), "frames"),
                     (dict(bin_width=5.0), "bin_width"), (dict(num_bins=360), "num_bins")):
        with pytest.raises(ValueError, match=what):
            paired_report(a, _result("dijkstra", **B, **kw))
    with pytest.raises(ValueError, match="envs"):
        paired_report(a, _result("dijkstra", [-1.0], [1], [1.0], [10.0], [10.0]))
    for x, y in ((a, _result("dijkstra", **B, exit_=True)), (_result("embedding", **A, exit_=True), _result("dijkstra", **B)),
                 (_result("embedding", **A, exit_=True), _result("dijkstra", **B, exit_=True))):
        rep = paired_report(x, y)
        assert rep["available"] is False and "domain exit" in rep["reason"] and "metrics" not in rep
        assert not any(isinstance(v, float) for v in rep.values())
        assert paired_lines(rep)[0].startswith("not available") and paired_scalars(rep) == {"available": 0}
    with pytest.raises(ValueError, match="seed"):              # a mismatch is refused before the domain exit is looked at
        paired_report(a, _result("dijkstra", **B, seed=4, exit_=True))


# ---- library loading -----------------------------------------------------------------------------------------------------
NEW = ("tarl_fused_edge_travel_time", "tarl_dest_trees_batched", "tarl_dest_trees_batched_scratch_bytes",
       "tarl_fused_select_next_hop_dest")


def test_entry_points_are_bound_and_the_abi_number_stays():
    from tarl_hip import lib
    L = lib.load()
    for name in NEW:
        assert name in lib.SIGNATURES and getattr(L, name) is not None
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    for name in NEW:
        assert name + "(" in header


def test_batched_scratch_query():
    from tarl_hip import lib
    L = lib.load()
    p = _plan(25_000, 100_000)
    pp = ctypes.byref(p)
    assert L.tarl_dest_trees_batched_scratch_bytes(None, 1, 4) == -1
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 0, 4) == -1 and L.tarl_dest_trees_batched_scratch_bytes(pp, -2, 4) == -1
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 1, -1) == -1
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 3, 0) == 0
    one = L.tarl_dest_trees_scratch_bytes(pp, 1)
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 1, 7) == L.tarl_dest_trees_scratch_bytes(pp, 7) == 7 * one
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 3, 5) == 15 * one
    # O(min(B D, 1024) x N), never O(B x D x N)
    assert L.tarl_dest_trees_batched_scratch_bytes(pp, 64, 3000) == 1024 * one == L.tarl_dest_trees_batched_scratch_bytes(pp, 10**4, 10**5)


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    need = L.tarl_dest_trees_batched_scratch_bytes(pp, 2, 4)
    ok = [pp, fake, 2, 400, fake, 4, fake, need, fake, null]
    for i in (0, 1, 4, 8):
        args = list(ok)
        args[i] = null
        assert L.tarl_dest_trees_batched(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad in ((2, 0), (5, -1), (3, -1), (3, 399)):
        args = list(ok)
        args[i] = bad
        assert L.tarl_dest_trees_batched(*args) == -1 and b"bad sizes" in L.tarl_last_error(), i
    args = list(ok)
    args[7] = need - 1
    assert L.tarl_dest_trees_batched(*args) == -1 and b"scratch too small" in L.tarl_last_error()
    big = _plan(400_000, 1_600_000)
    assert L.tarl_dest_trees_batched(ctypes.byref(big), fake, 1, 0, fake, 1, fake, 1 << 40, fake, null) == -1
    assert b"too large" in L.tarl_last_error()
    assert L.tarl_dest_trees_batched(pp, fake, 2, 0, fake, 0, null, 0, fake, null) == 0       # nothing to do: no launch
    assert L.tarl_fused_edge_travel_time(null, fake, 1, fake, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_fused_edge_travel_time(pp, fake, 1, null, null) == -1 and b"null" in L.tarl_last_error()
    assert L.tarl_fused_select_next_hop_dest(pp, null, 1, 15, 4, fake, fake, 0, 2, null, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_fused_select_next_hop_dest(pp, fake, 1, 15, 4, null, fake, 0, 2, null, null) == -1
    assert b"null" in L.tarl_last_error()


# ---- host argument checks of the ops ------------------------------------------------------------------------------------
class _P:
    num_nodes, num_edges, handle = 4, 4, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)
    sel8 = torch.zeros((4, 2), dtype=torch.uint8)


def test_ops_refuse_host_tensors():
    from tarl_hip import lib, ops
    w = torch.zeros((2, 4), dtype=torch.float32)
    dests = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.destination_trees_batched(_P(), w, dests)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_edge_travel_time(_P(), _FS())
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_select_next_hop_dest(_P(), _FS(), torch.zeros(4, dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32))


def test_evaluator_head_rules_without_a_device():
    from tarl_hip import lib
    from tarl_hip.evaluator import HEADS, VecEvaluator

    class _Unfused:
        fs = None
    assert "dijkstra" in HEADS
    with pytest.raises(lib.TarlError, match="fused"):
        VecEvaluator(_Unfused(), "dijkstra")

    class _Fused:
        fs = object()
    with pytest.raises(ValueError, match="emb"):                # every policy head still needs its embedding
        VecEvaluator(_Fused(), "embedding")
    with pytest.raises(ValueError, match="refresh_rate"):
        VecEvaluator(_Fused(), "dijkstra", refresh_rate=0)
