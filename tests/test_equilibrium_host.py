"""CPU: the equilibrium-metric entry points (csrc/equilibrium.hip, csrc/msa.hip) are declared, exported and bound, they and
their Python wrappers refuse bad arguments before any HIP call, the CLI carries the new flags with defaults that leave
RunnerArgs as before, and the numpy restatement the GPU tests compare against solves the closed-form four-road case."""
import ctypes
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import equilibrium_restatement as R
from fake_plan import fake_plan

NEW = ("tarl_msa_assign_sssp_gap", "tarl_msa_assign_gap", "tarl_bpr_step")


@pytest.fixture(scope="module")
def L():
    from tarl_hip import lib
    return lib.load()


def test_entry_points_declared_exported_and_bound(L):
    from tarl_hip import lib
    hdr = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} not declared"
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert int(re.search(r"#define TARL_ABI_VERSION (\d+)", hdr).group(1)) == 5       # additions only
    for k in ("TARL_BPR_UE = 0", "TARL_BPR_SO = 1", "TARL_BPR_MSA = 0", "TARL_BPR_FW = 1", "TARL_BPR_CFW = 2",
              "TARL_BPR_EVAL = 3"):
        assert k in code
    from tarl_hip import ops
    assert ops.BPR_OBJECTIVES == {"ue": 0, "so": 1} and ops.BPR_RULES == {"msa": 0, "fw": 1, "cfw": 2, "eval": 3}


def test_bpr_step_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    ok = [fake, fake, fake, fake, fake, fake, 16, 0, 1, 0.0, 2, fake, fake, null]
    for i in (0, 1, 2, 3, 4, 5, 11, 12):
        args = list(ok)
        args[i] = null
        assert L.tarl_bpr_step(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((7, 2, b"objective"), (7, -1, b"objective"), (8, 4, b"rule"), (8, -1, b"rule"),
                        (6, -1, b"bad sizes")):
        args = list(ok)
        args[i] = bad
        assert L.tarl_bpr_step(*args) == -1 and msg in L.tarl_last_error(), (i, bad)
    args = list(ok)
    args[8], args[9] = 0, 1.5
    assert L.tarl_bpr_step(*args) == -1 and b"msa_step" in L.tarl_last_error()


def test_assign_gap_entry_points_reject_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)
    ok = [fake, 8, fake, fake, fake, 3, fake, fake, fake, fake, null]
    for i in (0, 2, 3, 4, 6, 7, 8, 9):
        args = list(ok)
        args[i] = null
        assert L.tarl_msa_assign_gap(*args) == -1 and b"null" in L.tarl_last_error(), i
    args = list(ok)
    args[1] = 0
    assert L.tarl_msa_assign_gap(*args) == -1 and b"bad sizes" in L.tarl_last_error()
    args = list(ok)
    args[5] = 0
    assert L.tarl_msa_assign_gap(*args) == 0                    # nothing to do: no launch
    p = fake_plan(100, 400)
    pp = ctypes.byref(p)
    need = L.tarl_msa_scratch_bytes(pp, 3)
    ok = [pp, fake, fake, 3, fake, fake, fake, fake, fake, need, fake, fake, fake, null]
    for i in (0, 1, 2, 4, 5, 6, 7, 10, 11, 12):
        args = list(ok)
        args[i] = null
        assert L.tarl_msa_assign_sssp_gap(*args) == -1 and b"null" in L.tarl_last_error(), i
    args = list(ok)
    args[9] = need - 8
    assert L.tarl_msa_assign_sssp_gap(*args) == -1 and b"scratch too small" in L.tarl_last_error()


def test_wrappers_refuse_host_tensors_dtypes_and_sizes():
    from tarl_hip import lib, ops

    class _P:
        num_nodes, num_edges, handle = 4, 4, None
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)      # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)        # noqa: E731
    u8 = lambda n: torch.ones(n, dtype=torch.uint8)          # noqa: E731
    with pytest.raises(lib.TarlError):
        ops.bpr_step(f64(4), f64(4), f64(4), f64(4), f64(4), u8(4))
    with pytest.raises(lib.TarlError):
        ops.bpr_step(f64(4), None, None, f64(4), f64(4), u8(4), rule="eval")
    with pytest.raises(lib.TarlError):
        ops.msa_assign_gap(torch.zeros((4, 4), dtype=torch.int64), i64(2), i64(2), f64(2), u8(4), f64(4), f64(4))
    with pytest.raises(lib.TarlError):
        ops.msa_assign_trees_gap(_P(), f64(4), i64(1), i64(2), i64(1), f64(1), u8(4), f64(4))
    with pytest.raises(ValueError, match="objective"):
        ops.bpr_step(f64(4), f64(4), f64(4), f64(4), f64(4), u8(4), objective="nash")
    with pytest.raises(ValueError, match="rule"):
        ops.bpr_step(f64(4), f64(4), f64(4), f64(4), f64(4), u8(4), rule="newton")
    with pytest.raises(ValueError, match="msa_step"):
        ops.bpr_step(f64(4), f64(4), f64(4), f64(4), f64(4), u8(4), rule="msa", msa_step=2.0)


def test_wrappers_check_dtypes_and_sizes_before_any_hip_call(monkeypatch):
    """With the device check taken out (this test runs without a GPU) and the library replaced by one that fails on any call, a
    wrong dtype or size must still be refused: the checks run before the first HIP call."""
    from tarl_hip import ops

    def dtype_only(t, dtype, name):
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}")

    def no_library():
        raise AssertionError("a HIP call was reached")
    monkeypatch.setattr(ops, "_check_dev", dtype_only)
    monkeypatch.setattr(ops._lib, "load", no_library)

    class _P:
        num_nodes, num_edges, handle = 4, 6, None
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)      # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)        # noqa: E731
    u8 = lambda n: torch.ones(n, dtype=torch.uint8)          # noqa: E731
    good = dict(flow=f64(4), aon_flow=f64(4), target_prev=f64(4), free_flow=f64(4), capacity=f64(4), is_road=u8(4))
    for key in good:
        bad = dict(good)
        bad[key] = torch.zeros(4, dtype=torch.float32)
        with pytest.raises(TypeError, match=key):
            ops.bpr_step(**bad)
        bad[key] = good[key][:3].clone()
        if key != "flow":
            with pytest.raises(ValueError, match=key):
                ops.bpr_step(**bad)
        bad[key] = torch.zeros(8, dtype=good[key].dtype)[::2]
        with pytest.raises(ValueError, match="contiguous"):
            ops.bpr_step(**bad)
    with pytest.raises(ValueError, match="record"):
        ops.bpr_step(**good, record=f64(6))
    with pytest.raises(ValueError, match="cost_out"):
        ops.bpr_step(**good, cost_out=f64(5))
    with pytest.raises(AssertionError, match="HIP call"):          # the well-formed call is the one that gets through
        ops.bpr_step(**good, cost_out=f64(4), record=f64(8))

    nh = torch.zeros((4, 4), dtype=torch.int64)
    with pytest.raises(TypeError, match="node_cost"):
        ops.msa_assign_gap(nh, i64(2), i64(2), f64(2), u8(4), torch.zeros(4), f64(4))
    with pytest.raises(TypeError, match="next_hop"):
        ops.msa_assign_gap(nh.to(torch.int32), i64(2), i64(2), f64(2), u8(4), f64(4), f64(4))
    with pytest.raises(ValueError, match="per pair"):
        ops.msa_assign_gap(nh, i64(2), i64(3), f64(2), u8(4), f64(4), f64(4))
    with pytest.raises(ValueError, match="per node"):
        ops.msa_assign_gap(nh, i64(2), i64(2), f64(2), u8(4), f64(5), f64(4))
    with pytest.raises(ValueError, match="pair_cost"):
        ops.msa_assign_gap(nh, i64(2), i64(2), f64(2), u8(4), f64(4), f64(4), pair_cost=f64(3))
    with pytest.raises(ValueError, match=r"\(N, N\)"):
        ops.msa_assign_gap(torch.zeros((4, 5), dtype=torch.int64), i64(2), i64(2), f64(2), u8(4), f64(4), f64(4))

    args = lambda **kw: {**dict(plan=_P(), weights=f64(6), origins=i64(2), od_ptr=i64(3), od_dest=i64(5),   # noqa: E731
                                od_volume=f64(5), is_road=u8(4), aux_flow=f64(4)), **kw}
    with pytest.raises(TypeError, match="od_volume"):
        ops.msa_assign_trees_gap(**args(od_volume=torch.zeros(5)))
    with pytest.raises(ValueError, match="weights"):
        ops.msa_assign_trees_gap(**args(weights=f64(4)))
    with pytest.raises(ValueError, match="od_ptr"):
        ops.msa_assign_trees_gap(**args(od_ptr=i64(2)))
    with pytest.raises(ValueError, match="per node"):
        ops.msa_assign_trees_gap(**args(aux_flow=f64(3)))
    with pytest.raises(ValueError, match="sptt_part"):
        ops.msa_assign_trees_gap(**args(sptt_part=f64(3), unrouted_part=f64(2)))
    with pytest.raises(AssertionError, match="HIP call"):
        ops.msa_assign_trees_gap(**args(sptt_part=f64(2), unrouted_part=f64(2)))


def test_solver_argument_checks():
    from src.algorithms import equilibrium as eq
    sig = inspect.signature(eq.solve_assignment)
    want = dict(objective="ue", solver="cfw", gap_tol=1e-4, max_iter=500, method="auto", check_every=1)
    for k, v in want.items():
        assert sig.parameters[k].default == v, k
    with pytest.raises(ValueError, match="objective"):
        eq.solve_assignment(None, None, objective="nash")
    with pytest.raises(ValueError, match="solver"):
        eq.solve_assignment(None, None, solver="bush")
    with pytest.raises(ValueError, match="objective"):
        eq.assignment_gap(None, None, None, objective="x")
    with pytest.raises(ValueError, match="max_iter"):
        eq.solve_assignment(None, None, max_iter=0)
    assert callable(eq.equilibrium_report)


def test_cli_flags_and_runner_defaults():
    sys.path.insert(0, PKG)
    import main
    from src.runner import RunnerArgs
    p = main.build_parser()
    ns = p.parse_args([])
    assert ns.equilibrium_metrics is False and ns.equilibrium_gap == 1e-4 and ns.equilibrium_max_iter == 500
    ns = p.parse_args(["--algo", "random", "--equilibrium-metrics", "--equilibrium-gap", "1e-3",
                       "--equilibrium-max-iter", "40"])
    assert ns.equilibrium_metrics is True and ns.equilibrium_gap == 1e-3 and ns.equilibrium_max_iter == 40
    a = RunnerArgs(algo="random", scenario="synthetic-64-10", mode="eval")         # existing constructions keep working
    assert a.equilibrium_metrics is False and a.equilibrium_gap == 1e-4 and a.equilibrium_max_iter == 500
    assert RunnerArgs(**vars(ns)).equilibrium_max_iter == 40
    names = {f.name for f in dataclasses.fields(RunnerArgs)}
    assert {"equilibrium_metrics", "equilibrium_gap", "equilibrium_max_iter"} <= names


# ---- the restatement itself -------------------------------------------------------------------------------------------------
def test_restatement_closed_form():
    cf = R.four_road_closed_form()
    assert abs(cf["ue"][0] - 1.488) < 1e-3 and abs(cf["ue"][1] - 13.512) < 1e-3
    assert abs(cf["so"][0] - 5.964) < 1e-3 and abs(cf["so"][1] - 9.036) < 1e-3
    assert abs(cf["tstt_ue"] / cf["tstt_so"] - 1.1223) < 1e-4
    m = R.four_road_model()
    for objective in ("ue", "so"):
        for solver in ("fw", "cfw"):
            trace, flows = m.solve(objective, solver, 3)
            assert abs(flows[-1][1] - cf[objective][0]) < 1e-13 and abs(flows[-1][2] - cf[objective][1]) < 1e-13
            assert flows[-1][3] == 19.0 and flows[-1][0] == 0.0         # D carries both demands, the origin nothing
            assert abs(trace[-1][0]) < 1e-14 and trace[0][1] == 1.0
        ev = m.evaluate(flows[-1], objective)
        assert abs(ev["gap"]) < 1e-14
    # the lower bound from the UE flows, through their marginal-cost gap, stays below the optimum
    _, ue = m.solve("ue", "fw", 3)
    assert m.evaluate(ue[-1], "so")["lower_bound"] <= cf["tstt_so"] <= m.tstt(ue[-1])


def test_restatement_corner_equilibrium():
    cf = R.four_road_closed_form(13.0)
    assert cf["ue"] == (0.0, 13.0) and cf["so"][0] > 0.0
    m = R.four_road_model(13.0)
    trace, flows = m.solve("ue", "cfw", 3)
    assert np.array_equal(flows[-1], np.array([0.0, 0.0, 13.0, 17.0]))
    assert -1e-15 < trace[-1][0] <= 1e-15                               # may come out a few ulps below zero


def test_restatement_step_properties():
    rng = np.random.default_rng(0)
    N = 50
    ff, cap = rng.uniform(5, 20, N), rng.uniform(5, 30, N)
    road = rng.uniform(size=N) > 0.2
    f, y, sp = rng.uniform(0, 40, N), rng.uniform(0, 40, N), rng.uniform(0, 40, N)
    for objective in ("ue", "so"):
        r = R.step(f, y, sp, ff, cap, road, objective, "fw", 5)
        d = r["s"] - f
        g = lambda l: float(np.sum(d * R.bpr(ff, cap, road, f + l * d, R.C_OF[objective])))     # noqa: E731
        if r["g1"] > 0:
            assert 0.0 < r["lam"] < 1.0 and abs(g(r["lam"])) <= 1e-9 * np.sum(np.abs(d) * R.bpr(ff, cap, road, f + d, 0.75))
        assert R.step(f, f.copy(), sp, ff, cap, road, objective, "fw", 5)["lam"] == 1.0              # y = f: g == 0
        assert np.array_equal(R.step(f, f.copy(), sp, ff, cap, road, objective, "fw", 5)["f"], f)
        assert R.step(f, y, f.copy(), ff, cap, road, objective, "cfw", 5)["alpha"] == 0.0            # Dn = 0
        a = R.step(f, y, sp, ff, cap, road, objective, "cfw", 5)["alpha"]
        assert 0.0 <= a <= 0.99
        assert R.step(f, y, sp, ff, cap, road, objective, "cfw", 1)["lam"] == 1.0                    # the first load
        assert R.step(f, y, sp, ff, cap, road, objective, "msa", 4, msa_step=0.25)["lam"] == 0.25
        assert np.all(R.step(f, y, sp, ff, cap, road, objective, "fw", 5)["cost"][~road] == 0.0)
