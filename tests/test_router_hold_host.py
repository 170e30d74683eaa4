"""CPU: the shortest-path router that holds one road short of its destination (head "dijkstra_hold") — the rule
on the CPU oracle (``router_hold_restatement``) on the two torus cases of the design note, what the rule does and what each
of four defects would do instead, the static (free-flow) router, and the host side: the argument rules of
``--eval-baseline`` / ``--dijkstra-router``, the new C-ABI entry point (bound, validated before any HIP call, ABI number
unchanged) and the evaluator's refusals."""
import ctypes
import importlib
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from fake_plan import fake_plan as _plan

FEW_DESTS = [3, 17, 40, 66, 90, 101, 120, 127]


# ---- the two cases ---------------------------------------------------------------------------------------------------------
def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


def _gumbel(E, frames):
    """Seeded torch noise (NOT the device's streams): -log(-log(u)), u clamped away from 0."""
    g = torch.Generator().manual_seed(1)
    vals = [-torch.log(-torch.log(torch.rand(E, generator=g).clamp_min(1e-12))) for _ in range(frames)]
    return lambda t: vals[t]


def _case(name):
    """-> (net, population, frames). "spread": 128 agents bound anywhere, 300 frames; "few": 500 agents bound for eight roads,
    120 frames. Both leave within 40 s of the episode's start."""
    import baseline_restatement as BR
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = _torus8()
    if name == "spread":
        return net, synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40), 300
    return net, BR.few_destination_population(500, net.num_roads, FEW_DESTS, seed=7, t0=EPISODE_START,
                                              t1=EPISODE_START + 40), 120


def _replay(name, **kw):
    import router_hold_restatement as H
    from tarl_hip.engine import EPISODE_START
    net, pop, T = _case(name)
    kw.setdefault("refresh_rate", 10)
    T = kw.pop("frames", T)
    return H.replay(net, pop, T, kw.pop("refresh_rate"), _gumbel(net.edge_index.size(1), T), EPISODE_START, **kw)


@pytest.fixture(scope="module")
def replays():
    """{(case, hold)}: the reference-order replay and the hold replay of both cases, computed once."""
    return {(name, hold): _replay(name, hold=hold) for name in ("spread", "few") for hold in (False, True)}


def test_reference_replay_is_the_baseline_restatement(replays):
    """``hold=False`` is baseline_restatement.replay: the same frames, rewards and tables."""
    import baseline_restatement as BR
    from tarl_hip.engine import EPISODE_START
    net, pop, T = _case("few")
    want = BR.replay(net, pop, T, 10, _gumbel(net.edge_index.size(1), T), EPISODE_START)
    got = replays[("few", False)]
    assert torch.equal(got["sel"], want["sel"]) and got["reward"] == want["reward"]
    assert torch.equal(got["x"], want["x"]) and torch.equal(got["agents"], want["agents"])
    assert got["acted"] == 0


def test_the_hold_router_delivers_where_the_reference_order_strands(replays):
    """The finding of DESIGN 4.13 and its remedy. Under this noise: spread 0 -> 105 arrivals (return -27 924 -> -6 770), few
    372 -> 461 (return -34 361 -> -28 494); the test prints what it sees."""
    net = _torus8()
    for name in ("spread", "few"):
        ref, hold = replays[(name, False)], replays[(name, True)]
        print(f"[hold] {name}: arrivals {ref['arrivals']} -> {hold['arrivals']}, return {sum(ref['reward']):.0f} -> "
              f"{sum(hold['reward']):.0f}, peak count {ref['max_count']:.0f} / {hold['max_count']:.0f} of {net.Nmax}")
        assert ref["error"] is None and hold["error"] is None
        assert hold["arrivals"] > ref["arrivals"]
        assert ref["max_count"] < net.Nmax and hold["max_count"] < net.Nmax
    assert replays[("spread", False)]["arrivals"] == 0


def test_what_the_rule_does(replays):
    """The rule acts, agents enter through holding origin rows, and the core never carries an agent onto the road it is bound
    for (which the reference order does: that is how its agents strand). Both stated populations reach every case."""
    for name in ("spread", "few"):
        ref, hold = replays[(name, False)], replays[(name, True)]
        print(f"[hold] {name}: rule acted {hold['acted']} times ({hold['acted_occupied']} on occupied rows), "
              f"{hold['origin_hold']} agents entered through a holding origin row ({hold['origin_self']} through a row that "
              f"selects itself), core onto the destination road {ref['core_onto_dest']} -> {hold['core_onto_dest']}")
        assert hold["acted"] > 0 and hold["acted_occupied"] > 0
        assert hold["origin_hold"] > 0 and hold["origin_self"] >= hold["origin_hold"]
        assert hold["core_onto_dest"] == 0
        assert ref["core_onto_dest"] > 0 and ref["acted"] == 0
    # a holding row names itself, and only rows the reference rule sent to the head's destination hold
    hold = replays[("few", True)]
    ref_first = replays[("few", False)]["sel"][0]
    changed = hold["sel"][0] != ref_first          # frame 0: both replays start from the same state
    assert bool(changed.any())
    assert torch.equal(hold["sel"][0][changed], torch.arange(ref_first.numel(), dtype=ref_first.dtype)[changed])


@pytest.mark.parametrize("defect", ["minus_one", "two_short", "due_only", "slot_float"])
def test_each_defect_changes_the_outcome(replays, defect):
    """One wrong rule at a time on the few-destination case: the final agent table or a reward differs from the hold replay.
    (-1 as the hold value leaves the oracle's domain as soon as an agent enters through such a row: its insert raises.)"""
    good = replays[("few", True)]
    bad = _replay("few", hold=True, defect=defect)
    differs = bad["reward"] != good["reward"] or not torch.equal(bad["agents"], good["agents"])
    print(f"[hold] defect {defect}: arrivals {bad['arrivals']} (hold {good['arrivals']}), return {sum(bad['reward']):.0f}, "
          f"error {bad['error']}")
    assert differs
    if defect == "minus_one":
        assert bad["error"] is not None and len(bad["reward"]) < len(good["reward"])
    else:
        assert bad["error"] is None


def test_unknown_defect_is_refused():
    with pytest.raises(ValueError, match="defect"):
        _replay("few", hold=True, defect="other", frames=1)


def test_refresh_rate_zero_is_the_table_of_the_empty_network():
    """``refresh_rate=0`` == a replay that is handed, for every frame, the table built once from the state after the reset
    (every count 0: the free-flow router under the router's own weight expression); and it is not the refreshing router."""
    import baseline_restatement as BR
    from oracle import routing
    net, pop, _ = _case("few")
    N, Nmax = net.num_roads, net.Nmax
    T = 60
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, 3 * Nmax + 1] = 0
    w = routing.edge_travel_time(x, net.edge_index, net.congestion_constant, Nmax)
    assert torch.equal(w, net.x[:, 3 * Nmax + 2][net.edge_index[0]])          # the empty network: free-flow times
    table = BR.destination_columns(net.edge_index, w, N, sorted(set(FEW_DESTS)))
    static = _replay("few", hold=True, refresh_rate=0, frames=T)
    handed = _replay("few", hold=True, table=table, frames=T)
    assert len(static["tables"]) == 1 and handed["tables"] == []
    assert torch.equal(static["sel"], handed["sel"]) and static["reward"] == handed["reward"]
    assert torch.equal(static["x"], handed["x"]) and torch.equal(static["agents"], handed["agents"])
    live = _replay("few", hold=True, frames=T)
    assert len(live["tables"]) == 6 and not torch.equal(live["sel"], static["sel"])


def test_hold_choice_is_dijkstra_choice_plus_the_rule():
    """A hand-made state on a 3-road ring 0 -> 1 -> 2 -> 0: heads bound for the next road, the road after it and the road
    itself."""
    import router_hold_restatement as H
    from oracle import routing
    Nmax = 2
    col = 3 * Nmax + 5
    x = torch.zeros((3, 3 * Nmax + 7))
    x[:, 0] = torch.tensor([1.0, 2.0, 3.0])                      # heads: agents 1, 2, 3
    x[:, 3 * Nmax + 1] = 1.0
    ag = torch.zeros((4, 9))
    ag[1:, 1] = torch.tensor([1.0, 0.0, 2.0])                    # row 0 -> road 1 (next), row 1 -> road 0 (two on), row 2 -> itself
    table = torch.tensor([[0, 1, 1], [2, 1, 2], [0, 0, 2]])      # [row][destination]
    ref, _ = routing.dijkstra_choice(x, ag, None, None, Nmax, next_hop=table)
    assert ref[:, col].tolist() == [1.0, 2.0, 2.0]
    got = H.hold_choice(x, ag, table, Nmax)
    assert got[:, col].tolist() == [0.0, 2.0, 2.0]               # row 0 holds, row 1 moves on, row 2 is where it was
    assert H.holding_rows(x, ag, table, Nmax).tolist() == [True, False, True]
    assert H.hold_choice(x, ag, table, Nmax, defect="minus_one")[:, col].tolist() == [-1.0, 2.0, -1.0]
    assert H.hold_choice(x, ag, table, Nmax, defect="two_short")[:, col].tolist() == [0.0, 1.0, 2.0]
    got[:, col] = ref[:, col]
    assert torch.equal(got, ref)                                 # nothing else is touched


# ---- argument rules --------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules_for_the_new_values():
    assert _args().dijkstra_router == "reference"
    for name in ("dijkstra", "dijkstra_hold", "free_flow"):
        assert _args(eval_envs=4, eval_baseline=name).eval_baseline == name
        assert _args(algo="mpnn", mode="eval", eval_envs=4, eval_baseline=name).eval_baseline == name
        with pytest.raises(ValueError, match="eval_envs"):
            _args(eval_baseline=name)                                          # no eval_envs
        with pytest.raises(ValueError):
            _args(algo="dijkstra", mode="eval", eval_baseline=name)
    for bad in ("astar", "random", "", None, "hold", "reference"):
        with pytest.raises(ValueError, match="eval_baseline"):
            _args(eval_envs=4, eval_baseline=bad)
    for name in ("reference", "hold", "free_flow"):
        assert _args(algo="dijkstra", mode="eval", dijkstra_envs=2, dijkstra_router=name).dijkstra_router == name
    for bad in ("dijkstra_hold", "", None, "static"):
        with pytest.raises(ValueError, match="dijkstra_router"):
            _args(algo="dijkstra", mode="eval", dijkstra_envs=2, dijkstra_router=bad)
    for kw in (dict(algo="dijkstra", mode="eval"), dict(), dict(algo="mpnn", mode="eval", eval_envs=4)):
        for name in ("hold", "free_flow"):
            with pytest.raises(ValueError, match="dijkstra_router"):           # refused without dijkstra_envs
                _args(dijkstra_router=name, **kw)


def test_parser_flags():
    main = importlib.import_module("main")
    from src.runner import RunnerArgs
    ns = main.build_parser().parse_args([])
    assert ns.eval_baseline == "none" and ns.dijkstra_router == "reference"
    for name in ("dijkstra_hold", "free_flow"):
        ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "8", "--eval-baseline", name])
        assert RunnerArgs(**vars(ns)).eval_baseline == name
    for name in ("reference", "hold", "free_flow"):
        ns = main.build_parser().parse_args(["--algo", "dijkstra", "--mode", "eval", "--dijkstra-envs", "4",
                                             "--dijkstra-router", name])
        assert RunnerArgs(**vars(ns)).dijkstra_router == name
    ns = main.build_parser().parse_args(["--algo", "dijkstra", "--mode", "eval", "--dijkstra-router", "hold"])
    with pytest.raises(ValueError, match="dijkstra_router"):
        RunnerArgs(**vars(ns))
    for flag, bad in (("--eval-baseline", "hold"), ("--dijkstra-router", "dijkstra_hold")):
        with pytest.raises(SystemExit):
            main.build_parser().parse_args([flag, bad])


def test_the_names_map_onto_heads():
    from src.rl import ppo_trainer
    from src.rl.ppo_trainer import ppo_train
    from src import runner
    from tarl_hip.evaluator import DIJKSTRA_ROUTERS, EVAL_BASELINES, HEADS, ROUTER_HEADS
    assert inspect.signature(ppo_train).parameters["eval_baseline"].default == "none"
    assert EVAL_BASELINES == {"dijkstra": ("dijkstra", {}), "dijkstra_hold": ("dijkstra_hold", {}),
                              "free_flow": ("dijkstra_hold", {"refresh_rate": 0})}
    assert DIJKSTRA_ROUTERS == {"reference": ("dijkstra", None), "hold": ("dijkstra_hold", None),
                                "free_flow": ("dijkstra_hold", 0)}
    assert runner.EVAL_BASELINE_NAMES == ppo_trainer.EVAL_BASELINE_NAMES == ("none",) + tuple(EVAL_BASELINES)
    assert runner.DIJKSTRA_ROUTER_NAMES == tuple(DIJKSTRA_ROUTERS)
    assert ROUTER_HEADS == ("dijkstra", "dijkstra_hold") and all(h in HEADS for h in ROUTER_HEADS)


# ---- library loading -------------------------------------------------------------------------------------------------------
NEW = "tarl_fused_select_next_hop_hold"


def test_entry_point_is_bound_and_the_abi_number_stays():
    from tarl_hip import lib
    L = lib.load()
    assert NEW in lib.SIGNATURES and getattr(L, NEW) is not None
    assert lib.SIGNATURES[NEW] == lib.SIGNATURES["tarl_fused_select_next_hop_dest"]        # the same arguments
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert NEW + "(" in header


def test_entry_point_validates_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)                 # never dereferenced: validation fails first
    p = _plan(100, 400)
    pp = ctypes.byref(p)
    for entry in (L.tarl_fused_select_next_hop_hold, L.tarl_fused_select_next_hop_dest):      # the same host checks
        ok = [pp, fake, 1, 15, 4, fake, fake, 0, 2, null, null]
        for i in (0, 1, 5, 6):
            args = list(ok)
            args[i] = null
            assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i


# ---- host argument checks ----------------------------------------------------------------------------------------------------
class _P:
    num_nodes, num_edges, handle = 4, 4, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)
    sel8 = torch.zeros((4, 2), dtype=torch.uint8)


def test_the_op_takes_hold_and_refuses_host_tensors():
    from tarl_hip import lib, ops
    assert inspect.signature(ops.fused_select_next_hop_dest).parameters["hold"].default is False
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_select_next_hop_dest(_P(), _FS(), torch.zeros(4, dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32),
                                       hold=True)


def test_evaluator_head_rules_without_a_device():
    from tarl_hip import lib
    from tarl_hip.evaluator import HEADS, VecEvaluator

    class _Unfused:
        fs = None
    assert "dijkstra_hold" in HEADS
    with pytest.raises(lib.TarlError, match="fused"):
        VecEvaluator(_Unfused(), "dijkstra_hold")

    class _Fused:
        fs = object()
    for head in ("dijkstra_hold", "dijkstra"):
        with pytest.raises(ValueError, match="refresh_rate"):
            VecEvaluator(_Fused(), head, refresh_rate=-1)
    with pytest.raises(ValueError, match="refresh_rate"):           # the policy heads and the reference router keep >= 1
        VecEvaluator(_Fused(), "embedding", emb=torch.zeros(4), refresh_rate=0)
    with pytest.raises(ValueError, match="head"):
        VecEvaluator(_Fused(), "free_flow")                         # a name of the flags, not a head
