"""CPU: the per-destination tree entry points (csrc/dest_trees.hip) validate their arguments on the host, before any HIP
call; the Python layers refuse what the device path cannot take; ``DijkstraAgents(method=...)``, the ``--dijkstra-method``
flag and ``RunnerArgs.dijkstra_method`` at the interfaces. No GPU compute happens here."""
import ctypes
import dataclasses

import pytest
import torch

from fake_plan import fake_plan as _plan


@pytest.fixture(scope="module")
def L():
    from tarl_hip import lib
    return lib.load()


def test_scratch_query(L):
    assert L.tarl_dest_trees_scratch_bytes(None, 4) == -1
    p = _plan(25_000, 100_000)
    assert L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), -1) == -1
    assert L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 0) == 0
    one = L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 1)
    assert one >= 12 * 25_000                                   # one fp64 distance + one int32 next hop per node
    assert L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 10) == 10 * one
    # bounded by the resident workgroups, never O(destinations x N)
    assert L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 25_000) == L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 10**9)
    assert L.tarl_dest_trees_scratch_bytes(ctypes.byref(p), 25_000) == 1024 * one


def test_dest_trees_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    need = L.tarl_dest_trees_scratch_bytes(pp, 4)
    assert L.tarl_dest_trees(null, fake, fake, 4, fake, need, fake, fake, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, null, fake, 4, fake, need, fake, fake, null) == -1
    assert L.tarl_dest_trees(pp, fake, null, 4, fake, need, fake, fake, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, fake, fake, 4, fake, need, null, null, null) == -1
    assert b"no output" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, fake, fake, -3, fake, need, fake, fake, null) == -1
    assert b"bad sizes" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, fake, fake, 4, fake, need - 1, fake, null, null) == -1
    assert b"scratch too small" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, fake, fake, 4, null, need, null, fake, null) == -1
    assert b"scratch too small" in L.tarl_last_error()
    big = _plan(400_000, 1_600_000)                             # beyond the LDS bitmaps
    assert L.tarl_dest_trees(ctypes.byref(big), fake, fake, 1, fake, 1 << 40, fake, fake, null) == -1
    assert b"too large" in L.tarl_last_error()
    assert L.tarl_dest_trees(pp, fake, fake, 0, null, 0, fake, null, null) == 0        # nothing to do: no launch


def test_select_next_hop_dest_rejects_bad_arguments(L):
    null, fake = None, ctypes.c_void_p(0x1000)
    ok = [fake, 1, 0, 52, 15, 4, fake, 1, 9, fake, fake, 2, null]
    for i in (0, 6, 9, 10):                                     # every pointer argument the call needs
        args = list(ok)
        args[i] = null
        assert L.tarl_select_next_hop_dest(*args) == -1, i
        assert b"null" in L.tarl_last_error(), i
    for i, bad in ((1, 0), (3, 51), (4, 0), (7, 0), (5, -1), (11, -1)):
        args = list(ok)
        args[i] = bad
        assert L.tarl_select_next_hop_dest(*args) == -1, i
        assert b"bad shape" in L.tarl_last_error(), i
    args = list(ok)
    args[5] = 0
    assert L.tarl_select_next_hop_dest(*args) == 0                                      # no rows: no launch


def test_ops_refuse_cpu_tensors():
    from tarl_hip import lib, ops

    class _P:
        num_nodes, num_edges, handle = 4, 4, None
    w = torch.zeros(4, dtype=torch.float32)
    dests = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(lib.TarlError):
        ops.destination_trees(_P(), w, dests)
    with pytest.raises(ValueError):
        ops.destination_trees(_P(), w, dests, want_next_hop=False, want_dist=False)
    x = torch.zeros(4, 52)
    with pytest.raises(lib.TarlError):
        ops.select_next_hop_dest(x, 15, torch.zeros(2, 9), torch.zeros(4, dtype=torch.int32),
                                 torch.zeros(1, 4, dtype=torch.int32))


def test_dijkstra_agents_method_argument():
    from src.agents.base import DijkstraAgents
    from src.algorithms import user_equilibrium_msa as msa
    assert DijkstraAgents.METHODS == ("all_pairs", "per_destination", "auto")
    ag = DijkstraAgents("cpu")
    assert ag.method == "all_pairs" and ag.next_hop_tensor is None and ag.dest_next_hop is None
    with pytest.raises(ValueError, match="method"):
        DijkstraAgents("cpu", method="bellman_ford")
    # "auto": all-pairs up to run_msa's size limit, per-destination above (one constant for both)
    auto = DijkstraAgents("cpu", method="auto")
    cap = msa.ALL_PAIRS_MAX_NODES
    assert cap == 4096
    assert auto.resolve_method(cap) == "all_pairs" and auto.resolve_method(cap + 1) == "per_destination"
    assert auto.resolve_method(124) == "all_pairs" and auto.resolve_method(25_000) == "per_destination"
    for m in ("all_pairs", "per_destination"):
        assert DijkstraAgents("cpu", method=m).resolve_method(10) == m
        assert DijkstraAgents("cpu", method=m).resolve_method(10**6) == m


def test_cli_flag_and_runner_args():
    import main
    from src.runner import RunnerArgs
    p = main.build_parser()
    assert p.parse_args([]).dijkstra_method == "all_pairs"
    for m in ("all_pairs", "per_destination", "auto"):
        ns = p.parse_args(["--algo", "dijkstra", "--dijkstra-method", m])
        assert ns.dijkstra_method == m
        assert RunnerArgs(**vars(ns)).dijkstra_method == m
    with pytest.raises(SystemExit):
        p.parse_args(["--dijkstra-method", "floyd"])
    # RunnerArgs built without the new field keep working, with the old behaviour
    a = RunnerArgs(algo="dijkstra", scenario="Easy", mode="eval")
    assert a.dijkstra_method == "all_pairs"
    assert {f.name for f in dataclasses.fields(RunnerArgs)} >= {"algo", "scenario", "mode", "value_head", "dijkstra_method"}
    with pytest.raises(ValueError, match="dijkstra_method"):
        RunnerArgs(algo="dijkstra", scenario="Easy", mode="eval", dijkstra_method="floyd")


def test_runner_hands_the_method_to_the_agent(monkeypatch):
    """Runner.setup builds DijkstraAgents(method=args.dijkstra_method); the simulator's own I/O is stubbed out."""
    from src import runner as rmod
    from src import transportation_simulator as ts
    from src.agents.base import Agents, DijkstraAgents
    monkeypatch.setattr(ts.TransportationSimulator, "load_network", lambda self, scenario: None)
    monkeypatch.setattr(ts.TransportationSimulator, "config_parameters", lambda self, **kw: None)
    monkeypatch.setattr(Agents, "load", lambda self, scenario: None)
    for algo, m in (("dijkstra", "per_destination"), ("dijkstra", "auto"), ("dijkstra", "all_pairs"), ("random", "auto")):
        r = rmod.Runner.__new__(rmod.Runner)
        r.args, r.device = rmod.RunnerArgs(algo=algo, scenario="synthetic-1024-8", mode="eval", dijkstra_method=m), "cpu"
        r.setup()
        if algo == "dijkstra":
            assert isinstance(r.agent, DijkstraAgents) and r.agent.method == m
        else:
            assert type(r.agent) is Agents
        assert r.simulator.agent is r.agent
