"""CPU: the host side of the vectorised evaluation — CLI flags and RunnerArgs checks, the checkpoint key mapping, the
aggregate over environments, percentiles from a histogram, and the two new C-ABI entry points' argument validation."""
import importlib
import math

import numpy as np
import pytest
import torch


def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train")
    base.update(kw)
    return RunnerArgs(**base)


def test_parser_defaults_and_flags():
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.eval_envs == 0 and ns.eval_sampled is False and ns.iterations == 1 and ns.checkpoint is None
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "8", "--eval-sampled", "--iterations", "3",
                                         "--checkpoint", "runs/policy.pt"])
    assert (ns.eval_envs, ns.eval_sampled, ns.iterations, ns.checkpoint) == (8, True, 3, "runs/policy.pt")
    from src.runner import RunnerArgs
    a = RunnerArgs(**vars(ns))          # every parsed flag is a RunnerArgs field
    assert a.eval_envs == 8 and a.eval_sampled and a.iterations == 3 and a.checkpoint == "runs/policy.pt"


def test_runner_args_defaults_refusals_and_total_frames():
    a = _args()
    assert a.eval_envs == 0 and a.eval_sampled is False and a.iterations == 1 and a.checkpoint is None
    assert a.total_frames == a.rollout_steps == 32            # the default trains one collector batch, as before
    assert _args(iterations=5, rollout_steps=48).total_frames == 240
    assert _args(eval_envs=16, algo="mpnn", mode="eval").eval_envs == 16
    for bad in (dict(eval_envs=4, algo="random"), dict(eval_envs=4, algo="dijkstra"), dict(eval_envs=-1),
                dict(iterations=0), dict(iterations=-2)):
        with pytest.raises(ValueError):
            _args(**bad)
    with pytest.raises(ValueError, match="eval_envs"):
        _args(eval_sampled=True)
    with pytest.raises(ValueError, match="checkpoint"):
        _args(algo="dijkstra", checkpoint="policy.pt")


def test_checkpoint_key_mapping():
    from src.runner import CHECKPOINT_PREFIX, checkpoint_state
    own = {"nodes_embedding.weight": torch.zeros(6, 1), "edge_mlp.0.weight": torch.zeros(64, 33),
           "edge_mlp.0.bias": torch.zeros(64), "gt_pe": torch.zeros(6, 16)}
    file = {CHECKPOINT_PREFIX + k: torch.full_like(v, float(i + 1)) for i, (k, v) in enumerate(own.items())}
    got = checkpoint_state(file, own)
    assert sorted(got) == sorted(own)
    for i, k in enumerate(own):
        assert torch.equal(got[k], torch.full_like(own[k], float(i + 1)))
    # a shape that does not match, a key the network lacks, a key the file lacks, a foreign prefix: each names the key
    bad = dict(file)
    bad[CHECKPOINT_PREFIX + "nodes_embedding.weight"] = torch.zeros(7, 1)
    with pytest.raises(ValueError, match="nodes_embedding.weight.*\\(7, 1\\)"):
        checkpoint_state(bad, own)
    extra = dict(file)
    extra[CHECKPOINT_PREFIX + "transformer.WQ.weight"] = torch.zeros(2)
    with pytest.raises(ValueError, match="transformer.WQ.weight"):
        checkpoint_state(extra, own)
    short = {k: v for k, v in file.items() if not k.endswith("gt_pe")}
    with pytest.raises(ValueError, match="gt_pe"):
        checkpoint_state(short, own)
    with pytest.raises(ValueError, match="other.weight"):
        checkpoint_state({"other.weight": torch.zeros(1)}, own)


def test_aggregate_against_numpy():
    from tarl_hip.evaluator import aggregate
    v = [3.0, -1.5, 8.25, 0.0, 4.0]
    g = aggregate(v)
    a = np.asarray(v)
    se = a.std(ddof=1) / math.sqrt(a.size)
    assert g["n"] == 5 and g["missing"] == 0
    assert g["mean"] == a.mean() and g["std"] == a.std(ddof=1) and g["se"] == se
    assert g["min"] == -1.5 and g["max"] == 8.25
    assert g["ci95"] == (a.mean() - 1.96 * se, a.mean() + 1.96 * se) and "normal" in g["ci95_kind"]
    one = aggregate([7.0])                    # K = 1: a mean, no spread, no interval
    assert one["mean"] == 7.0 and one["std"] is None and one["se"] is None and one["ci95"] is None and one["n"] == 1
    # environments without an arrival have no travel time: left out, and counted
    g = aggregate([None, 120.0, None, 80.0])
    assert g["n"] == 2 and g["missing"] == 2 and g["mean"] == 100.0
    assert g["std"] == np.std([120.0, 80.0], ddof=1)
    none = aggregate([None, None])
    assert none["n"] == 0 and none["missing"] == 2 and none["mean"] is None and none["ci95"] is None


def test_summarise_environments_without_arrivals():
    from tarl_hip.evaluator import summarise
    counts = np.array([[2, 1, 0], [0, 3, 0]], dtype=np.int32)
    sums = np.array([[50.0, 1700.0, 40.0], [0.0, 0.0, 0.0]])
    hist = np.zeros((2, 8), dtype=np.int32)
    hist[0, 1] = 1      # tt = 10
    hist[0, 4] = 1      # tt = 40
    per, agg, missing = summarise(counts, sums, np.array([-12.0, -30.0]), hist, 25, 10.0)
    assert per["avg_travel_time"] == [25.0, None] and per["max_travel_time"] == [40.0, None]
    assert per["std_travel_time"][0] == 15.0 and per["p50_travel_time"] == [20.0, None] and per["p95_travel_time"] == [50.0, None]
    assert per["arrived"] == [2, 0] and per["on_way"] == [1, 3] and per["frames"] == [25, 25]
    assert missing == 1 and agg["avg_travel_time"]["n"] == 1 and agg["avg_travel_time"]["missing"] == 1
    assert agg["avg_travel_time"]["ci95"] is None and agg["episode_return"]["mean"] == -21.0


@pytest.mark.parametrize("seed,n", [(0, 1), (1, 20), (2, 37), (3, 400), (4, 1001)])
def test_percentiles_from_a_histogram_against_numpy(seed, n):
    """Integer data, unit bins: value v lies in bin v, whose upper edge is v + 1 — the histogram percentile is numpy's
    inverted-CDF percentile plus one bin width."""
    from tarl_hip.evaluator import hist_percentile
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 50, size=n)
    hist = np.bincount(data, minlength=64)
    for q in (0.5, 0.95, 0.25, 1.0):
        want = float(np.percentile(data, 100 * q, method="inverted_cdf")) + 1.0
        assert hist_percentile(hist, q, 1.0) == want, (q, n)
    # bins of width 10: the upper edge of the bin of the same sample
    hist10 = np.bincount(data // 10, minlength=8)
    for q in (0.5, 0.95):
        want = (float(np.percentile(data, 100 * q, method="inverted_cdf")) // 10 + 1) * 10.0
        assert hist_percentile(hist10, q, 10.0) == want
    assert hist_percentile(np.zeros(8, dtype=np.int64), 0.5, 10.0) is None


def test_new_entry_points_are_bound_and_validate_on_the_host():
    from tarl_hip import lib
    assert "tarl_graphdist_mode_rollout" in lib.SIGNATURES and "tarl_episode_summary" in lib.SIGNATURES
    L = lib.load()
    null = None
    assert L.tarl_graphdist_mode_rollout(null, null, 1, 1.0, null, null, null, null, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_episode_summary(null, 1, 1, 9, null, 0, 10.0, 720, null, null, null, null, null) == -1
    assert b"null" in L.tarl_last_error()
    # sizes are checked before anything is launched: a buffer address is never dereferenced on these paths
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert L.tarl_episode_summary(p, 0, 1, 9, null, 0, 10.0, 720, p, p, null, null, null) == -1
    assert L.tarl_episode_summary(p, 1, 2, 9, null, 0, 10.0, 720, p, p, null, null, null) == -1      # tables overlap
    assert L.tarl_episode_summary(p, 1, 1, 9, null, 5, 10.0, 720, p, p, p, null, null) == -1          # frames, no rewards
    assert L.tarl_episode_summary(p, 1, 1, 9, null, 0, 10.0, 0, p, p, null, p, null) == -1            # no bins
    assert L.tarl_episode_summary(p, 1, 1, 9, null, 0, 0.0, 8, p, p, null, p, null) == -1             # zero bin width
    assert b"bin_width" in L.tarl_last_error()


def test_evaluator_refuses_an_unfused_engine_and_unknown_heads():
    from tarl_hip import lib
    from tarl_hip.evaluator import VecEvaluator

    class _Eng:
        fs = None
    with pytest.raises(lib.TarlError, match="fused"):
        VecEvaluator(_Eng(), "embedding", emb=torch.zeros(4))
