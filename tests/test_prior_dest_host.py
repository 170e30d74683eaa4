"""CPU: the per-destination prior table (MPNNPolicyNet.prior_method) — CLI and RunnerArgs plumbing, the auto rule, the
new C-ABI symbols, argument checks on the host, and the destination set / slot map the table is built over."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT
from fake_plan import fake_plan as _plan

NEW = ("tarl_prior_dest_table_scratch_bytes", "tarl_prior_dest_table", "tarl_policy_prior_logits_dest",
       "tarl_fused_prior_logits_dest", "tarl_fused_rollout_prior_dest")


@pytest.fixture(scope="module")
def L():
    from tarl_hip import lib
    return lib.load()


def test_cli_prior_method_parsing_and_default():
    sys.path.insert(0, PKG)
    import main
    p = main.build_parser()
    assert p.parse_args([]).prior_method == "all_pairs"
    for m in ("all_pairs", "per_destination", "auto"):
        assert p.parse_args(["--prior-method", m]).prior_method == m
    with pytest.raises(SystemExit):
        p.parse_args(["--prior-method", "nope"])
    from src.runner import RunnerArgs
    ns = p.parse_args(["--policy-head", "embedding_dijkstra", "--prior-method", "per_destination"])
    assert RunnerArgs(**vars(ns)).prior_method == "per_destination"


def test_runner_args_reject_unknown_prior_method():
    sys.path.insert(0, PKG)
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-64", mode="train", policy_head="embedding_dijkstra")
    assert RunnerArgs(**base).prior_method == "all_pairs"
    with pytest.raises(ValueError, match="prior_method"):
        RunnerArgs(prior_method="dense", **base)


@pytest.mark.parametrize("N,want", [(4096, "all_pairs"), (4097, "per_destination")])
def test_auto_resolves_by_the_all_pairs_limit(N, want):
    sys.path.insert(0, PKG)
    from src.agents.mpnn_agent import MPNNPolicyNet
    pol = MPNNPolicyNet.__new__(MPNNPolicyNet)          # the rule reads num_nodes and prior_method only
    torch.nn.Module.__init__(pol)
    pol.num_nodes = N
    pol.prior_method = "auto"
    assert pol.resolve_prior_method() == want
    for m in ("all_pairs", "per_destination"):
        pol.prior_method = m
        assert pol.resolve_prior_method() == m
    pol.prior_method = "nope"
    with pytest.raises(ValueError):
        pol.resolve_prior_method()


def test_new_entry_points_are_declared_exported_and_bound():
    from tarl_hip import lib
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert re.search(rf" T {name}$", syms, re.M), name
        assert name in lib.SIGNATURES, name
    assert re.search(r"#define TARL_ABI_VERSION 5\b", header)
    assert lib.load().tarl_abi_version() == 5


def test_entry_points_reject_bad_arguments_on_the_host(L):
    null, fake = None, ctypes.c_void_p(0x1000)           # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    assert L.tarl_prior_dest_table_scratch_bytes(None, 4) == -1
    assert L.tarl_prior_dest_table_scratch_bytes(pp, -1) == -1
    assert L.tarl_prior_dest_table_scratch_bytes(pp, 3) > 0
    # plan, weights, dests, D, scratch, scratch_bytes, table, stream
    ok = [pp, fake, fake, 3, fake, 1 << 30, fake, null]
    for i in (0, 1, 2, 6):
        args = list(ok)
        args[i] = null
        assert L.tarl_prior_dest_table(*args) == -1 and b"null" in L.tarl_last_error(), i
    args = list(ok)
    args[5] = 8
    assert L.tarl_prior_dest_table(*args) == -1 and b"scratch" in L.tarl_last_error()
    # plan, obs16, M, emb, num_emb, table, D, dest_slot, w, logits, stream
    ok = [pp, fake, 4, fake, 100, fake, 7, fake, ctypes.c_float(1.0), fake, null]
    for i in (0, 5, 7):
        args = list(ok)
        args[i] = null
        assert L.tarl_policy_prior_logits_dest(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, v, msg in ((6, 0, b"column"), (2, 0, b"bad sizes"), (8, ctypes.c_float(-1.0), b"prior_weight")):
        args = list(ok)
        args[i] = v
        assert L.tarl_policy_prior_logits_dest(*args) == -1 and msg in L.tarl_last_error(), i
    # plan, f, x, B, x_bstride, ldx, Nmax, ag, A, a_bstride, emb, M, table, D, dest_slot, w, logits, stream
    w = ctypes.c_float(1.0)
    ok = [pp, fake, fake, 8, 0, 0, 15, fake, 50, 450, fake, 100, fake, 7, fake, w, fake, null]
    for i, v, msg in ((12, null, b"null"), (14, null, b"null"), (13, 0, b"column"), (16, null, b"null")):
        args = list(ok)
        args[i] = v
        assert L.tarl_fused_prior_logits_dest(*args) == -1 and msg in L.tarl_last_error(), i


def test_destination_set_and_slot_map():
    """Dummy row 0 is a destination (empty rows read agent 0); ids outside [0, N) are dropped; B environments' tables
    share one set; the slot map inverts it."""
    sys.path.insert(0, PKG)
    from src.agents.base import destination_set
    N = 10
    ag = torch.zeros((5, 9))
    ag[:, 1] = torch.tensor([4.0, 7.0, 4.0, 12.0, -1.0])        # row 0 heads for 4; 12 and -1 are out of range
    d, slot = destination_set(ag, N)
    assert d.dtype == torch.int64 and slot.dtype == torch.int32 and slot.shape == (N,)
    assert d.tolist() == [4, 7]
    assert slot[4] == 0 and slot[7] == 1 and int((slot >= 0).sum()) == 2
    ag[0, 1] = 2.0
    d, slot = destination_set(ag, N)
    assert d.tolist() == [2, 4, 7]                           # the dummy row's own destination counts
    batch = torch.zeros((3, 4, 9))
    batch[0, :, 1] = torch.tensor([0.0, 1.0, 1.0, 9.0])
    batch[1, :, 1] = torch.tensor([0.0, 5.0, 10.0, 3.0])
    batch[2, :, 1] = torch.tensor([6.0, 6.0, 6.0, 6.0])
    d, slot = destination_set(batch, N)
    assert d.tolist() == [0, 1, 3, 5, 6, 9]
    assert torch.equal(slot[d], torch.arange(d.numel(), dtype=torch.int32))
    assert int((slot >= 0).sum()) == d.numel()


def test_dijkstra_agents_share_the_destination_set():
    sys.path.insert(0, PKG)
    from src.agents.base import DijkstraAgents, destination_set
    ag = torch.zeros((6, 9))
    ag[:, 1] = torch.tensor([3.0, 8.0, 1.0, 8.0, 40.0, 2.0])
    a = DijkstraAgents("cpu", method="per_destination")
    a.agent_features = ag
    a._build_destinations(20)
    d, slot = destination_set(ag, 20)
    assert torch.equal(a.destinations, d) and torch.equal(a.dest_slot, slot)
