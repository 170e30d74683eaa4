"""CPU: the hold rule on a policy's action (``--policy-hold``) — the rule on the CPU oracle
(``policy_hold_restatement``) on crafted states of the torus and both irregular graphs and in a closed-loop replay on the
torus, what the rule does and what each of six defects would do instead, the conditions the chosen inputs must meet (enough
holds on occupied rows, every "leave alone" reason present), and the host side: the new C-ABI entry points (bound,
validated before any HIP call, ABI number unchanged), the parser, the argument rules and the head rules."""
import ctypes
import importlib
import inspect
import os
import re

import pytest
import torch

import policy_hold_restatement as PH
from conftest import ROOT
from fake_plan import fake_plan as _plan

GRAPHS = ("torus", "MIXED", "HUB126")
K = 3


# ---- 1. crafted states ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    return {name: PH.crafted(name, K) for name in GRAPHS}


def _classify(cr, b, **kw):
    return PH.classify(PH.with_selected_road(cr, b), cr.ag[b], cr.succ, cr.deg, cr.Nmax, code=cr.code[b], **kw)


@pytest.mark.parametrize("name", GRAPHS)
def test_the_rule_on_crafted_rows(crafted, name):
    """Conditions on the inputs (checked here, on the CPU: the GPU tests run the same cases): >= 20 holds on occupied rows
    and >= 1 of every "leave alone" reason per graph; the named rows behave as :func:`policy_hold_restatement.crafted` says;
    ranks >= 4 and the last rank of the largest out-list are held off the torus."""
    cr = crafted[name]
    rows = cr.rows
    col_n = 3 * cr.Nmax + 1
    total = {k: 0 for k in PH.REASONS}
    for b in range(K):
        hold, why = _classify(cr, b)
        for w in why:
            total[w] += 1
        assert bool((cr.x[b, hold, col_n] > 0).all())                      # a hold is a hold on an occupied row
        want = dict(near="hold", far="hold", raw="raw", carried="carried", head_hi="head_range", other_road="other_road",
                    empty="empty", stale="empty", own="other_road")
        if "rank4" in rows:
            want["rank4"] = "hold"
        for r, w in want.items():
            assert why[rows[r]] == w, (name, b, r, why[rows[r]])
        # without the bytes, from x alone, the raw and the carried row could not be told from a rank
        blind, _ = PH.classify(PH.with_selected_road(cr, b), cr.ag[b], cr.succ, cr.deg, cr.Nmax)
        assert bool(blind[rows["raw"]]) and bool(blind[rows["carried"]])
        s8, sel, held = PH.expected_bytes(PH.with_selected_road(cr, b), cr.ag[b], cr.succ, cr.deg, cr.Nmax, cr.code[b], cr.sel[b])
        assert held == int(hold.sum())
        assert bool((s8[hold] == PH.SEL_RAW).all()) and torch.equal(sel[hold], torch.nonzero(hold).view(-1).float())
        assert torch.equal(s8[~hold], cr.code[b][~hold]) and torch.equal(sel[~hold], cr.sel[b][~hold])
    print(f"[policy hold, crafted {name}] {total}")
    assert total["hold"] >= 20 and all(total[k] >= 1 for k in PH.REASONS), total
    assert int(cr.code[0, rows["far"]]) == int(cr.deg[rows["far"]]) - 1
    if name != "torus":
        assert "rank4" in rows and int(cr.deg[rows["far"]]) - 1 >= 4
    if name == "HUB126":
        assert int(cr.code[0, rows["far"]]) == 125


@pytest.mark.parametrize("name", GRAPHS)
def test_each_defect_changes_a_named_crafted_row(crafted, name):
    cr = crafted[name]
    rows = cr.rows
    for b in range(K):
        x = PH.with_selected_road(cr, b)
        true, _ = _classify(cr, b)
        # holds empty rows too, reading agent 0: the clean empty row, whose choice leads to agent 0's destination
        d, _ = _classify(cr, b, defect="empty_rows")
        assert bool(d[rows["empty"]]) and not bool(true[rows["empty"]])
        # holds when ANY out-target is the destination: the road that chose another one
        d, _ = _classify(cr, b, defect="any_target")
        assert bool(d[rows["other_road"]]) and not bool(true[rows["other_road"]])
        # holds only when the head is due: `near` leaves at t + 50, `far` at t - 5
        d, _ = _classify(cr, b, defect="due_only", t=cr.t)
        assert not bool(d[rows["near"]]) and bool(d[rows["far"]]) and bool(true[rows["near"]]) and bool(true[rows["far"]])
        # compares floats against the destination's slot: one road is nobody's destination, so behind it slot != id
        slot_of = PH.slots_of(cr.ag[b], cr.N)
        d, _ = _classify(cr, b, defect="slot_float", slot_of=slot_of)
        named = [r for r in ("near", "far", "rank4") if r in rows and bool(true[rows[r]]) and not bool(d[rows[r]])]
        assert named, (name, b)
        # writes -1
        xm, xt = x.clone(), x.clone()
        PH.apply_rule(xm, cr.ag[b], cr.succ, cr.deg, cr.Nmax, code=cr.code[b], defect="minus_one")
        PH.apply_rule(xt, cr.ag[b], cr.succ, cr.deg, cr.Nmax, code=cr.code[b])
        col = 3 * cr.Nmax + 5
        assert xm[rows["near"], col] == -1.0 and xt[rows["near"], col] == float(rows["near"])
        assert torch.equal(xm[~true], xt[~true]) and torch.equal(xt[~true], x[~true])      # every other row: as written


# ---- 2. closed-loop replay on the torus ------------------------------------------------------------------------------------------
def _gumbel(E, frames):
    g = torch.Generator().manual_seed(1)
    vals = [-torch.log(-torch.log(torch.rand(E, generator=g).clamp_min(1e-12))) for _ in range(frames)]
    return lambda t: vals[t]


T_REPLAY = 200


@pytest.fixture(scope="module")
def torus_case():
    """128 agents bound anywhere on the 8 x 8 torus (the "spread" case of DESIGN 4.13a), and a deterministic policy that
    needs no device: every road picks the free-flow next hop towards its head agent's destination (an empty road reads
    agent 0), recorded frame by frame along the run WITHOUT the rule and along the run WITH it."""
    from baseline_restatement import destination_columns
    from oracle import sim
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    N, Nmax, ei = net.num_roads, net.Nmax, net.edge_index
    pop = synth.population(128, N, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    succ, deg, orank = PH.out_table(ei, N)
    ff = net.x[:, 3 * Nmax + 2][ei[0]]
    dests = sorted({int(d) for d in pop[:, 1].tolist() if 0 <= d < N})
    table = destination_columns(ei, ff, N, dests)
    adj = net.dense_adjacency()
    gum = _gumbel(ei.size(1), T_REPLAY)
    no_action = torch.zeros(ei.size(1), dtype=torch.long)

    def record(hold):
        c = sim.Cols(Nmax)
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pop.clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        acts = []
        for t in range(T_REPLAY):
            d = ag[x[:, 0].long(), 1].long()
            code = PH.codes_of(table[torch.arange(N), d].float(), succ)
            code = torch.where(code == PH.SEL_RAW, torch.full_like(code, PH.SEL_CARRIED), code)      # "no draw": keep the byte
            acts.append(code.to(torch.uint8))
            sim.apply_action(x, ei, PH.onehot_of_bytes(code, ei, orank), Nmax)
            if hold:
                PH.apply_rule(x, ag, succ, deg, Nmax)
            sim.env_step(x, ag, ei, net.edge_attr, adj, no_action, float(EPISODE_START + t), Nmax, gumbel=gum(t),
                         congestion_constant=net.congestion_constant)
        return torch.stack(acts)

    return dict(net=net, pop=pop, gum=gum, t0=EPISODE_START, acts={h: record(h) for h in (False, True)})


def test_the_rule_delivers_where_the_policy_alone_strands(torus_case):
    c = torus_case
    plain = PH.replay(c["net"], c["pop"], c["acts"][False], c["gum"], c["t0"], hold=False)
    held = PH.replay(c["net"], c["pop"], c["acts"][True], c["gum"], c["t0"], hold=True)
    print(f"[policy hold, torus replay] arrivals {plain['arrivals']} -> {held['arrivals']}, holds {sum(held['held'])}, "
          f"reasons {held['reasons']}")
    assert plain["error"] is None and held["error"] is None
    assert held["arrivals"] > plain["arrivals"] and held["arrivals"] >= 20
    assert sum(held["held"]) >= 20 and sum(plain["held"]) == 0
    assert sum(held["reward"]) > sum(plain["reward"])
    assert torch.equal(held["stored"], c["acts"][True].long())              # the stored action is the policy's own
    assert held["reasons"]["empty"] > 0 and held["reasons"]["other_road"] > 0


REPLAY_DEFECTS = tuple(d for d in PH.DEFECTS if d not in ("minus_one", "any_target"))


@pytest.mark.parametrize("defect", REPLAY_DEFECTS)
def test_each_defect_changes_the_replay(torus_case, defect):
    """Four of the six defects show in this replay. The other two cannot, and the crafted rows name them instead: the
    recorded policy always picks the destination road where one leads there (so "any target" is "the chosen target"), and no
    agent enters through a holding origin row before the row's head leaves (so -1 is never read as a road)."""
    c = torus_case
    true = PH.replay(c["net"], c["pop"], c["acts"][True], c["gum"], c["t0"], hold=True)
    bad = PH.replay(c["net"], c["pop"], c["acts"][True], c["gum"], c["t0"], hold=True, defect=defect)
    same_run = bad["error"] is None and bad["reward"] == true["reward"] and torch.equal(bad["x"], true["x"]) and \
        torch.equal(bad["agents"], true["agents"]) and bad["held"] == true["held"]
    if defect == "rewrite_action":          # the environment is the same; what the update would read is not
        assert same_run and not torch.equal(bad["stored"], true["stored"])
        assert int((bad["stored"] == PH.SEL_RAW).sum()) == sum(true["held"])
    else:
        assert not same_run, defect
        assert torch.equal(bad["stored"], true["stored"])


# ---- 3. library loading, refusals before any HIP call ---------------------------------------------------------------------------
NEW = ("tarl_fused_hold_policy_actions", "tarl_fused_set_policy_hold")


def test_entry_points_are_bound_and_the_abi_number_stays():
    from tarl_hip import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    for n in NEW:
        assert n in lib.SIGNATURES and getattr(L, n) is not None and n + "(" in header
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert "src/reinforcement_learning.py:222-309" in header and "src/agents/base.py:334-403" in header
    names = [f[0] for f in lib.FusedStruct._fields_]
    assert names[-3:] == ["policy_hold", "bufs_dev", "policy_held"]         # appended / the reserved word: nothing moved
    kernel = open(os.path.join(ROOT, "tarl-simulator_amd", "csrc", "policy_hold.hip")).read()
    assert "k_fused_hold_policy_actions" in kernel and "EMPTY row is never touched" in kernel


def _fake_fused(lib):
    f = lib.FusedStruct()
    for name, typ in lib.FusedStruct._fields_:
        if typ is ctypes.c_void_p and name != "policy_held":
            setattr(f, name, 0x1000)                                        # never dereferenced: validation fails first
    f.ld_slots, f.acc_slots = 48, 1
    return f


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    pp = ctypes.byref(_plan(100, 400))
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    entry = L.tarl_fused_hold_policy_actions
    ok = [pp, fp, 2, 15, fake, 4, 36, null, null, null]
    for i in (0, 1, 4):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    # the host checks of tarl_fused_select_next_hop_dest on the handle and the sizes
    for i, bad, msg in ((2, 0, b"bad sizes"), (3, 128, b"Nmax"), (2, 1 << 31, b"bad sizes")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    empty = lib.FusedStruct()
    assert entry(pp, ctypes.byref(empty), 2, 15, fake, 4, 36, null, null, null) == -1 and b"buffers missing" in L.tarl_last_error()
    # its own: the agent table
    for i, bad, msg in ((5, 0, b"bad sizes"), (5, (1 << 24) + 1, b"bad sizes"), (6, 35, b"agent stride")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    # the switch
    setter = L.tarl_fused_set_policy_hold
    assert setter(null, 1, null) == -1 and b"null" in L.tarl_last_error()
    assert setter(fp, 2, null) == -1 and setter(fp, -1, null) == -1
    assert setter(fp, 0, fake) == -1 and b"without the switch" in L.tarl_last_error()
    assert f.policy_hold == 0 and not f.policy_held                        # a refused call changes nothing
    assert setter(fp, 1, fake) == 0 and f.policy_hold == 1 and f.policy_held == 0x1000
    assert setter(fp, 0, null) == 0 and f.policy_hold == 0 and not f.policy_held
    assert lib.FusedStruct().policy_hold == 0                               # off by default


class _P:
    num_nodes, num_edges, handle = 4, 4, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)
    sel8 = torch.zeros((4, 2), dtype=torch.uint8)


def test_the_ops_refuse_host_tensors():
    from tarl_hip import lib, ops
    sig = inspect.signature(ops.fused_hold_policy_actions).parameters
    assert list(sig) == ["plan", "fs", "agent_features", "choice8", "held"] and sig["choice8"].default is None and \
        sig["held"].default is None
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_hold_policy_actions(_P(), _FS(), torch.zeros((2, 3, 9)))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_set_policy_hold(_FS(), True, torch.zeros(2, dtype=torch.int32))


# ---- 4. parser, argument rules, head rules ----------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="edge_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_parser_flag_and_runner_rules():
    main = importlib.import_module("main")
    from src.runner import RunnerArgs
    assert main.build_parser().parse_args([]).policy_hold is False and _args().policy_hold is False
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--policy-hold"])
    assert RunnerArgs(**vars(ns)).policy_hold is True
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "edge_mlp", "--policy-hold"])
    assert RunnerArgs(**vars(ns)).policy_hold is True
    with pytest.raises(ValueError, match="eval_envs"):                      # eval mode without --eval-envs
        _args(algo="mpnn", mode="eval", policy_hold=True)
    with pytest.raises(ValueError, match="embedding"):                      # train mode with the embedding head
        _args(algo="mpnn+ppo", mode="train", policy_head="embedding", policy_hold=True)
    for algo in ("random", "dijkstra"):
        with pytest.raises(ValueError, match="policy_hold"):
            _args(algo=algo, mode="eval", policy_hold=True)
    _args(algo="mpnn", mode="eval", eval_envs=2, policy_head="embedding", policy_hold=True)       # evaluated: per-frame path
    for head in ("edge_mlp", "edge_mlp_bf16", "embedding_dijkstra", "graph_transformer"):
        _args(algo="mpnn+ppo", mode="train", policy_head=head, policy_hold=True)
    help_text = main.build_parser().format_help()
    assert "--policy-hold" in help_text and "empty road" in " ".join(help_text.split())


def test_defaults_are_off_everywhere():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.evaluator import EvalResult, VecEvaluator
    from tarl_hip.trainer import VecPPOTrainer
    for fn in (ppo_train, VecEvaluator.__init__, VecPPOTrainer.__init__):
        assert inspect.signature(fn).parameters["policy_hold"].default is False
    res = EvalResult(envs=1, head="embedding", deterministic=True, frames_run=1)
    assert res.held is None and "held" not in res.to_dict() and "policy_hold" not in res.settings


def test_evaluator_and_trainer_head_rules_without_a_device():
    from tarl_hip.evaluator import PLAN_HEADS, ROUTER_HEADS, VecEvaluator
    from tarl_hip.trainer import VecPPOTrainer

    class _Fused:
        fs = object()
    for head in ROUTER_HEADS + PLAN_HEADS:
        with pytest.raises(ValueError, match="policy_hold"):
            VecEvaluator(_Fused(), head, routes=(None, None) if head in PLAN_HEADS else None, policy_hold=True)
    with pytest.raises(ValueError, match="policy_hold is not available for policy='embedding'"):
        VecPPOTrainer(_Fused(), None, [], rollout_steps=4, policy="embedding", policy_hold=True)
