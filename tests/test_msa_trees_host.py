"""CPU: the per-origin shortest-path tree entry points (csrc/msa.hip) validate their arguments on the host, before any
HIP call, and the Python layers refuse what the device path cannot take. No GPU compute happens here."""
import ctypes
import inspect

import pytest
import torch

from fake_plan import fake_plan as _plan


@pytest.fixture(scope="module")
def L():
    from tarl_hip import lib
    return lib.load()


def test_scratch_query(L):
    assert L.tarl_msa_scratch_bytes(None, 4) == -1
    p = _plan(25_000, 100_000)
    assert L.tarl_msa_scratch_bytes(ctypes.byref(p), -1) == -1
    assert L.tarl_msa_scratch_bytes(ctypes.byref(p), 0) == 0
    one = L.tarl_msa_scratch_bytes(ctypes.byref(p), 1)
    assert one >= 12 * 25_000                                   # one fp64 distance + one int32 predecessor per node
    assert L.tarl_msa_scratch_bytes(ctypes.byref(p), 10) == 10 * one
    # bounded by the resident workgroups, never O(sources x N)
    assert L.tarl_msa_scratch_bytes(ctypes.byref(p), 25_000) == L.tarl_msa_scratch_bytes(ctypes.byref(p), 10**9)
    assert L.tarl_msa_scratch_bytes(ctypes.byref(p), 25_000) < 25_000 * one


def test_sssp_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    assert L.tarl_sssp_f64(null, fake, fake, 1, fake, 1 << 20, fake, fake, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_sssp_f64(pp, null, fake, 1, fake, 1 << 20, fake, fake, null) == -1
    assert L.tarl_sssp_f64(pp, fake, null, 1, fake, 1 << 20, fake, fake, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_sssp_f64(pp, fake, fake, -3, fake, 1 << 20, fake, fake, null) == -1
    assert b"bad sizes" in L.tarl_last_error()
    need = L.tarl_msa_scratch_bytes(pp, 4)
    assert L.tarl_sssp_f64(pp, fake, fake, 4, fake, need - 1, fake, fake, null) == -1
    assert b"scratch too small" in L.tarl_last_error()
    assert L.tarl_sssp_f64(pp, fake, fake, 4, null, need, fake, fake, null) == -1
    assert b"scratch too small" in L.tarl_last_error()
    big = _plan(400_000, 1_600_000)                             # beyond the LDS bitmaps
    assert L.tarl_sssp_f64(ctypes.byref(big), fake, fake, 1, fake, 1 << 40, fake, fake, null) == -1
    assert b"too large" in L.tarl_last_error()
    assert L.tarl_sssp_f64(pp, fake, fake, 0, null, 0, null, null, null) == 0        # nothing to do: no launch


def test_msa_assign_sssp_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    need = L.tarl_msa_scratch_bytes(pp, 3)
    ok = [pp, fake, fake, 3, fake, fake, fake, fake, fake, need, fake, null]
    for i in (0, 1, 2, 4, 5, 6, 7, 10):                         # every pointer argument the call needs
        args = list(ok)
        args[i] = null
        assert L.tarl_msa_assign_sssp(*args) == -1, i
        assert b"null" in L.tarl_last_error(), i
    args = list(ok)
    args[9] = need - 8
    assert L.tarl_msa_assign_sssp(*args) == -1 and b"scratch too small" in L.tarl_last_error()
    args = list(ok)
    args[3] = -1
    assert L.tarl_msa_assign_sssp(*args) == -1 and b"bad sizes" in L.tarl_last_error()


def test_ops_refuse_cpu_tensors():
    from tarl_hip import lib, ops

    class _P:
        num_nodes, num_edges, handle = 4, 4, None
    w = torch.zeros(4, dtype=torch.float64)
    src = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(lib.TarlError):
        ops.shortest_path_trees(_P(), w, src)
    with pytest.raises(lib.TarlError):
        ops.msa_assign_trees(_P(), w, src, torch.zeros(2, dtype=torch.int64), src, torch.ones(1, dtype=torch.float64),
                             torch.ones(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.shortest_path_trees(_P(), w, src, want_dist=False, want_pred=False)


def test_run_msa_method_argument():
    from src.algorithms import user_equilibrium_msa as msa
    sig = inspect.signature(msa.run_msa)
    assert sig.parameters["method"].default == "auto"
    assert sig.parameters["tol"].default == 1e-5 and sig.parameters["max_iter"].default == 1000
    with pytest.raises(ValueError, match="method"):
        msa.run_msa(None, None, method="bellman")
