"""CPU: ``bench.py --dump-outputs DIR`` writes what the last timed PPO iteration left its caller as DIR/<name>.npy — float32,
finite, small arrays whole, large ones as a seeded sample of flat positions that depends on the element count alone (so two
builds are compared position for position), and never more than 64 MB in all. The real run is in
tests/test_gpu_bench_contract.py::test_bench_line_contract."""
import importlib
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_sample_is_whole_or_fixed_positions():
    bench = _bench()
    small = torch.arange(12, dtype=torch.uint8).view(3, 4)
    assert np.array_equal(bench.dump_sample(small), np.arange(12, dtype=np.float32))
    big = torch.arange(5000, dtype=torch.int32).view(50, 100)
    a = bench.dump_sample(big, k=300)
    b = bench.dump_sample(big.float() * 2, k=300)
    assert a.dtype == np.float32 and a.shape == (300,)
    assert np.all(np.diff(a) >= 0) and a.max() < 5000                  # sorted flat positions of the array
    assert np.array_equal(b, 2 * a)                                      # the same positions for the same element count


def test_dump_writes_every_output_within_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    names = {"params", "losses", "reward", "log_prob", "log_prob_infeasible", "values", "times", "counts", "choice", "leg",
             "state", "agents"}
    assert len(names) * bench.DUMP_SAMPLE * 4 <= bench.DUMP_BYTES == 64 << 20     # the bench's default sample fits the budget
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    T, B, N = 6, 40, 30
    g = torch.Generator().manual_seed(0)
    trainer = SimpleNamespace(flat=SimpleNamespace(flat=torch.randn(500, generator=g)), last={"losses": torch.randn(6, generator=g)},
                              reward=torch.randn(T, B, generator=g), logp=torch.randn(T, B, generator=g),
                              values=torch.randn(T + 1, B, generator=g), times=torch.arange(T + 1, dtype=torch.float32),
                              counts=torch.randint(0, 16, (T + 1, N, B), dtype=torch.uint8, generator=g),
                              choice=torch.randint(0, 4, (T, N, B), dtype=torch.uint8, generator=g),
                              leg=torch.randint(0, 9, (T, B, 2), dtype=torch.int32, generator=g))
    engine = SimpleNamespace(x=torch.randn(B, N, 52, generator=g), agents=torch.randn(B, 7, 9, generator=g))
    sizes = bench.dump_outputs(str(tmp_path / "out"), trainer, engine)
    assert set(sizes) == names and {p.name for p in (tmp_path / "out").iterdir()} == {n + ".npy" for n in names}
    for n in names:
        a = np.load(tmp_path / "out" / (n + ".npy"))
        assert a.dtype == np.float32 and a.size == sizes[n] <= 1000
    assert np.array_equal(np.load(tmp_path / "out" / "reward.npy"), trainer.reward.reshape(-1).numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "losses.npy"), trainer.last["losses"].numpy())
    assert not np.load(tmp_path / "out" / "log_prob_infeasible.npy").any()


def _outputs(logp):
    T, B = logp.shape
    trainer = SimpleNamespace(flat=SimpleNamespace(flat=torch.zeros(8)), last={"losses": torch.zeros(6)}, reward=torch.zeros(T, B),
                              logp=logp, values=torch.zeros(T + 1, B), times=torch.zeros(T + 1), counts=torch.zeros(T + 1, 3, B),
                              choice=torch.zeros(T, 3, B), leg=torch.zeros(T, B, 2))
    return trainer, SimpleNamespace(x=torch.zeros(B, 3, 4), agents=torch.zeros(B, 2, 9))


def test_infeasible_log_prob_is_written_as_a_mask(tmp_path):
    """An infeasible action's log-probability is -inf (the reference's GraphDistribution.log_prob): the file holds 0 there and
    log_prob_infeasible marks it, so every file stays finite."""
    bench = _bench()
    logp = torch.tensor([[-3.5, -float("inf")], [-float("inf"), -0.25]])
    bench.dump_outputs(str(tmp_path), *_outputs(logp))
    assert np.array_equal(np.load(tmp_path / "log_prob.npy"), np.array([-3.5, 0.0, 0.0, -0.25], dtype=np.float32))
    assert np.array_equal(np.load(tmp_path / "log_prob_infeasible.npy"), np.array([0, 1, 1, 0], dtype=np.float32))
    assert all(np.isfinite(np.load(p)).all() for p in tmp_path.iterdir())


def test_non_finite_outputs_are_refused(tmp_path):
    """A NaN anywhere (or an infinity other than an infeasible log-probability) is an error, not a file."""
    bench = _bench()
    trainer, engine = _outputs(torch.zeros(2, 2))
    trainer.values[1, 0] = float("nan")
    with pytest.raises(AssertionError, match="values"):
        bench.dump_outputs(str(tmp_path / "out"), trainer, engine)
    assert not (tmp_path / "out").exists()
