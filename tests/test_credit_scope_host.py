"""CPU: credit scope "due" and the horizon bootstrap of the per-decision PPO credit — the premise on the CPU
oracle (the draw of a road whose head is not due changes nothing), ``credit_scope_restatement`` on hand-made cases, the ten
named defects (each moves its case by at least ten times the GPU tolerance or flips an integer), and the host side: the new
C-ABI entry points (bound, validated before any HIP call, ABI number unchanged, tarl_fused not grown), the setter's state
rules, the ops', the parser's, the argument rules' and the trainer's refusals."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import credit_scope_restatement as CS
import decision_credit_restatement as DC
import update_restatement as R
from conftest import ROOT
from fake_plan import fake_plan as _plan


# ---- 1. the premise ------------------------------------------------------------------------------------------------------------
def test_the_draw_of_a_road_whose_head_is_not_due_changes_nothing():
    """The spread case of test_router_hold_host (8 x 8 torus, 128 agents, 300 frames, holding router, refresh 10): the
    selection of every headed-but-not-due road re-drawn, every frame leaves the FIFOs below the count, the counts and the
    agent table ``==``. Under this noise 4 734 headed (frame, road) decisions, 790 of them due."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    g = torch.Generator().manual_seed(1)
    vals = [-torch.log(-torch.log(torch.rand(net.edge_index.size(1), generator=g).clamp_min(1e-12))) for _ in range(300)]
    r = CS.premise_replay(net, pop, 300, 10, lambda t: vals[t], EPISODE_START)
    print(f"[credit scope premise] headed {r['headed']}, due {r['due']} ({100.0 * r['due'] / r['headed']:.1f} %), "
          f"{r['redrawn']} selections re-drawn, {len(r['differing'])} differing frames, {r['twice']} ids queued twice")
    assert r["differing"] == [] and r["redrawn"] > r["headed"] // 2
    assert 0 < r["due"] < r["headed"] / 2
    assert r["twice"] == 0
    # where everybody stands in the end: arrived and lost agents nowhere, the queued ones on the road that holds them
    x, ag = r["x"].numpy(), r["agents"].numpy()
    Nmax = net.Nmax
    for a in range(1, ag.shape[0]):
        where = [u for u in range(net.num_roads) if a in x[u, :int(x[u, 3 * Nmax + 1])].astype(np.int64)]
        assert ([int(r["road"][a])] if r["road"][a] >= 0 else []) == where, a
        if ag[a, DC.DONE] == 1:
            assert r["road"][a] == -1
    assert int(ag[1:, DC.DONE].sum()) > 50 and (r["road"][1:] >= 0).any()


# ---- 2. hand-made cases -----------------------------------------------------------------------------------------------------------
NMAX = 4


def _state():
    """One environment, five roads, Nmax 4 (F = 19), the clock of the frame 100: road 0 headed and due exactly at the clock,
    road 1 headed and due one ulp above it, road 2 empty with a stale id and a stale, early dep word, road 3 headed and long
    due with two queued, road 4 headed and due at the NEXT clock."""
    x = np.zeros((1, 5, 3 * NMAX + 7), dtype=np.float32)
    x[0, :, 0] = [7, 8, 9, 3, 5]
    x[0, 3, 1] = 4
    x[0, 3, 2] = 6                                             # the slot AT the count of road 3: a pending garbage id
    x[0, :, 2 * NMAX] = [100.0, np.nextafter(np.float32(100.0), np.float32(200.0)), 50.0, 20.0, 101.0]
    x[0, :, 3 * NMAX + 1] = [1, 1, 0, 2, 1]
    return x


def test_due_heads_by_hand():
    x = _state()
    heads, headed, due = CS.due_heads(x, NMAX, 100.0)
    assert heads.tolist() == [[7, 0, 0, 3, 0]]
    assert headed.tolist() == [[True, True, False, True, True]] and due.tolist() == [[True, False, False, True, False]]
    assert CS.due_heads(x, NMAX, 100.0, defect="strict_less")[0].tolist() == [[0, 0, 0, 3, 0]]
    assert CS.due_heads(x, NMAX, 100.0, next_clock=101.0, defect="next_clock")[0].tolist() == [[7, 8, 0, 3, 5]]
    assert CS.due_heads(x, NMAX, 100.0, defect="empty_dep_believed")[0].tolist() == [[7, 0, 9, 3, 0]]
    # one ulp below the head's dep: not due; the headed heads are DC.heads'
    below = np.nextafter(np.float32(100.0), np.float32(0.0))
    assert CS.due_heads(x, NMAX, below)[0].tolist() == [[0, 0, 0, 3, 0]]
    assert DC.heads(x, NMAX).tolist() == [[7, 8, 0, 3, 5]]


def test_agent_roads_by_hand():
    """Ids queued on a road map to it, lost agents to -1, agents that have left a road do not map to it; the ring offset and
    the garbage slot."""
    x = _state()
    count = x[..., 3 * NMAX + 1]
    road, bad, twice = CS.agent_roads(x[..., :NMAX].astype(np.int64), count, 10)
    assert road.tolist() == [[-1, -1, -1, 3, 3, 4, -1, 0, 1, -1]] and bad == 0 and twice == 0      # 9: left road 2; 6: garbage
    assert CS.agent_roads(x[..., :NMAX].astype(np.int64), count, 10, defect="garbage_slot_read")[0][0, 6] == 3
    hoff = np.array([[0, 3, 1, 3, 2]])
    rg = CS.ring(x, NMAX, hoff)
    assert rg[0, 3].tolist() == [4, 6, 0, 3]                   # logical 0, 1, 2 at physical 3, 0, 1
    assert np.array_equal(CS.agent_roads(rg, count, 10, hoff)[0], road)
    wrong = CS.agent_roads(rg, count, 10, hoff, defect="hoff_ignored")[0]
    assert wrong[0, 3] == -1 and wrong[0, 6] == 3 and not np.array_equal(wrong, road)
    assert CS.agent_roads(x[..., :NMAX].astype(np.int64), count, 8)[1] == 1                          # id 8 outside [1, 8)


def _torus_case():
    """The 8 x 8 torus (free flow 10 s per road, timestep 1): the rows decide in frames 2 and 5 of a segment that ends after
    frame 11. Agent 1 is queued two roads short of its destination, agent 2 is lost (queued nowhere, never DONE), agent 3
    arrived at clock 107. dist[s][v] = 10 s x the roads from v to the destination (a breadth-first search of the graph)."""
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    N, ei = net.num_roads, net.edge_index.numpy()
    assert net.x[:, 3 * net.Nmax + 2].unique().tolist() == [10.0]
    lists = DC.out_lists(ei, N)
    nbr = [[int(ei[1][e]) for e in ls] for ls in lists]
    dests = [40, 90, 200]
    dist = np.full((3, N), np.inf)
    for s, d in enumerate(dests):
        dist[s, d], frontier = 0.0, [d]
        rev = [[v for v in range(N) if u in nbr[v]] for u in range(N)]
        while frontier:
            nxt = []
            for u in frontier:
                for v in rev[u]:
                    if not np.isfinite(dist[s, v]):
                        dist[s, v] = dist[s, u] + 10.0
                        nxt.append(v)
            frontier = nxt
    slot = np.full(N, -1, dtype=np.int64)
    slot[dests] = np.arange(3)
    two_short = next(v for v in range(N) if dist[0, v] == 20.0)
    far = next(v for v in range(N) if dist[0, v] == 60.0 and dist[1, v] != 60.0)
    A = 5
    ag = np.zeros((1, A, 9), dtype=np.float32)
    ag[0, 1:4, DC.DESTINATION] = dests
    ag[0, 1, DC.ON_WAY] = ag[0, 2, DC.ON_WAY] = 1.0
    ag[0, 3, [DC.ARRIVAL_TIME, DC.DONE]] = [107.0, 1.0]
    road = np.full((1, A), -1, dtype=np.int64)
    road[0, 1] = two_short
    head = np.zeros((2, N), dtype=np.int64)
    head[0, far], head[0, 5], head[0, 9] = 1, 2, 3             # frame 2: the three travellers at the heads of three roads
    head[1, far] = 1                                           # frame 5: agent 1 again
    times = np.arange(100, 113, dtype=np.float32)
    return dict(N=N, deg=np.full(N, 4), dist=dist, slot=slot, ag=ag, road=road, head=head, frame=[2, 5], env=[0, 0],
                times=times, t_end=12, far=far, two_short=two_short)


def _boot(c, bootstrap=True, defect=None, gamma=1.0):
    return CS.decision_advantage_boot(c["head"], c["frame"], c["env"], c["ag"], c["times"], c["t_end"], c["dist"], c["slot"],
                                      c["deg"], c["road"], bootstrap, 1.0, gamma, defect)


def test_the_bootstrapped_n_by_hand():
    c = _torus_case()
    out = _boot(c)
    far = c["far"]
    # agent 1, frame 2: 10 frames to the horizon + 2 roads x 10 frames; frame 5: 7 + 20. Free flow from `far`: 60 frames
    assert out["n"][0, far] == 30.0 and out["n"][1, far] == 27.0
    assert out["adv"][0, far] == 60.0 - 30.0 and out["adv"][1, far] == 60.0 - 27.0
    # agent 2 is lost: charged the 10 frames to the horizon, truncated; agent 3 arrived at clock 107: frames 2 .. 6 owed
    assert out["n"][0, 5] == 10.0 and out["n"][0, 9] == 5.0
    assert (out["bootstrapped"], out["truncated"], out["bad"]) == (2, 1, 0) and int(out["live"].sum()) == 4
    g = _boot(c, gamma=0.99)
    assert abs(g["adv"][0, far] - ((1 - 0.99 ** 60.0) / 0.01 - (1 - 0.99 ** 30.0) / 0.01)) < 1e-12
    # a segment that ends with the episode keeps the charge: the plain rule, bit for bit
    from tarl_hip.engine import EPISODE_END
    assert CS.segment_bootstrap(EPISODE_END, EPISODE_END) and not CS.segment_bootstrap(EPISODE_END + 1.0, EPISODE_END)
    end = _boot(c, bootstrap=CS.segment_bootstrap(EPISODE_END + 1.0, EPISODE_END))
    plain = DC.decision_advantage(c["head"], c["frame"], c["env"], c["ag"], c["times"], c["t_end"], c["dist"], c["slot"],
                                  c["deg"])
    assert np.array_equal(end["adv"], plain["adv"]) and end["n"][0, far] == 10.0
    assert (end["bootstrapped"], end["truncated"]) == (0, 3) and plain["truncated"] == 3


# ---- 3. the named defects --------------------------------------------------------------------------------------------------------
def test_each_defect_moves_its_case():
    """The raw advantage is compared on the GPU within ``tensor_bound`` of its fp32 rounding, integers ``==``: each defect
    moves an element of a crafted case by whole frames, at least ten times that bound, or flips an integer."""
    c = _torus_case()
    ref = _boot(c)
    a64 = torch.from_numpy(ref["adv"])
    bound = R.tensor_bound(R.max_err(a64.float(), a64), a64)
    seen = set()
    for defect in ("bootstrap_from_u", "dist_transposed", "lost_bootstrapped", "bootstrapped_also_truncated",
                   "bootstrap_at_episode_end"):
        if defect == "bootstrap_at_episode_end":
            from tarl_hip.engine import EPISODE_END
            got = _boot(c, bootstrap=CS.segment_bootstrap(EPISODE_END + 1.0, EPISODE_END, defect))
            want = _boot(c, bootstrap=CS.segment_bootstrap(EPISODE_END + 1.0, EPISODE_END))
        else:
            got, want = _boot(c, defect=defect), ref
        moved = float(np.abs(got["adv"] - want["adv"]).max())
        ints = (got["truncated"], got["bootstrapped"]) != (want["truncated"], want["bootstrapped"])
        print(f"[credit scope defect {defect}] moved {moved:.3g} (bound {bound:.3g}), integers differ: {ints}")
        assert moved >= 10.0 * bound or ints, defect
        if defect in ("bootstrap_from_u", "dist_transposed", "lost_bootstrapped", "bootstrap_at_episode_end"):
            assert moved >= 10.0 * bound, defect       # whole frames
        if defect in ("lost_bootstrapped", "bootstrapped_also_truncated"):
            assert ints, defect
        seen.add(defect)
    # the integer ones: test_due_heads_by_hand and test_agent_roads_by_hand show the flipped entries
    x = _state()
    good = CS.due_heads(x, NMAX, 100.0)[0]
    for defect in ("strict_less", "next_clock", "empty_dep_believed"):
        assert not np.array_equal(CS.due_heads(x, NMAX, 100.0, next_clock=101.0, defect=defect)[0], good), defect
        seen.add(defect)
    count, hoff = x[..., 3 * NMAX + 1], np.array([[0, 3, 1, 3, 2]])
    rg = CS.ring(x, NMAX, hoff)
    good = CS.agent_roads(rg, count, 10, hoff)[0]
    for defect in ("garbage_slot_read", "hoff_ignored"):
        assert not np.array_equal(CS.agent_roads(rg, count, 10, hoff, defect=defect)[0], good), defect
        seen.add(defect)
    assert seen == set(CS.DEFECTS)
    with pytest.raises(ValueError, match="unknown defect"):
        CS.due_heads(x, NMAX, 100.0, defect="other")
    with pytest.raises(ValueError, match="unknown defect"):
        _boot(c, defect="other")


# ---- 4. the host side --------------------------------------------------------------------------------------------------------------
NEW = ("tarl_fused_head_rows_due", "tarl_fused_set_head_capture_scope", "tarl_fused_agent_roads",
       "tarl_decision_advantage_boot")


def _fake_fused(lib):
    f = lib.FusedStruct()
    for name, typ in lib.FusedStruct._fields_:
        if typ is ctypes.c_void_p and name != "policy_held":
            setattr(f, name, 0x1000)                                        # never dereferenced: validation fails first
    f.ld_slots, f.acc_slots = 48, 1
    return f


def test_entry_points_are_bound_and_nothing_moved():
    from tarl_hip import lib
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert all(n in lib.SIGNATURES and hasattr(L, n) and n + "(" in header for n in NEW)
    assert re.search(r"#define TARL_ABI_VERSION (\d+)", header).group(1) == "5" and L.tarl_abi_version() == 5
    assert lib.FusedStruct._fields_[-1][0] == "policy_held"                  # tarl_fused did not grow
    # the boot form takes the plain form's arguments plus three in front of the stream
    plain, boot = lib.SIGNATURES["tarl_decision_advantage"][1], lib.SIGNATURES["tarl_decision_advantage_boot"][1]
    assert boot[:len(plain) - 1] == plain[:-1] and len(boot) == len(plain) + 3


def test_entry_points_validate_before_any_hip_call():
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    pp = ctypes.byref(_plan(100, 400))
    f = _fake_fused(lib)
    fp = ctypes.byref(f)
    # plan, f, B, t_clock, env, slot, n, head_keep, counts2, stream
    entry, ok = L.tarl_fused_head_rows_due, [pp, fp, 2, 100.0, fake, fake, 3, fake, null, null]
    for i in (0, 1, 4, 5, 7):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad in ((2, 0), (2, 1 << 31), (6, -1), (6, 1 << 24)):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1, (i, bad)
    for bad in (float("inf"), float("nan")):
        args = list(ok)
        args[3] = bad
        assert entry(*args) == -1 and b"t_clock" in L.tarl_last_error()
    assert entry(pp, fp, 2, 100.0, null, null, 0, null, null, null) == 0        # nothing to do: no launch, no pointer needed
    # plan, f, B, A, Nmax, agent_road, bad, stream
    entry, ok = L.tarl_fused_agent_roads, [pp, fp, 2, 5, 15, fake, fake, null]
    for i in (0, 1, 5, 6):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad in ((2, 0), (3, 0), (3, (1 << 24) + 1), (4, 128), (4, 1), (4, 17)):      # 17: ld_slots 48 < 3 * 17
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1, (i, bad)
    # the plain form's arguments and refusals, then agent_road, bootstrap, bootstrapped, stream
    entry = L.tarl_decision_advantage_boot
    ok = [pp, fake, fake, fake, fake, 3, 2, fake, 5, 45, fake, 11, 10, fake, fake, 4, 1.0, 1.0, fake, fake, fake, fake, 1, fake,
          null]
    for i in (0, 1, 2, 3, 4, 7, 10, 13, 14, 18, 19, 20):
        args = list(ok)
        args[i] = null
        assert entry(*args) == -1 and b"null" in L.tarl_last_error(), i
    for i, bad, msg in ((5, -1, b"bad sizes"), (9, 44, b"a_bstride"), (12, 12, b"t_end"), (16, 0.0, b"timestep"),
                        (17, 1.5, b"decision_gamma"), (5, 1 << 24, b"too many"), (22, 2, b"bootstrap must"),
                        (22, -1, b"bootstrap must"), (21, null, b"bootstrap needs"), (23, null, b"bootstrap needs")):
        args = list(ok)
        args[i] = bad
        assert entry(*args) == -1 and msg in L.tarl_last_error(), (i, L.tarl_last_error())
    args = list(ok)
    args[5], args[21], args[22], args[23] = 0, null, 0, null                   # no rows, no bootstrap: nothing to do
    assert entry(*args) == 0


def test_the_scope_setter_state_rules():
    """Refused unless the capture is on for that handle; switching the capture off clears it (and on starts from headed);
    the word of the four switches is the capture setter's alone."""
    from tarl_hip import lib
    L = lib.load()
    null, fake = None, ctypes.c_void_p(0x1000)
    f, g = _fake_fused(lib), _fake_fused(lib)
    fp, gp = ctypes.byref(f), ctypes.byref(g)
    cap, scope = L.tarl_fused_set_head_capture, L.tarl_fused_set_head_capture_scope
    assert scope(null, 1, null) == -1 and b"null" in L.tarl_last_error()
    assert scope(fp, 1, null) == -1 and b"capture is off" in L.tarl_last_error()      # never switched on
    assert scope(fp, 0, null) == -1 and f.policy_hold == 0
    assert cap(fp, 1, fake) == 0 and f.policy_hold == 8
    assert scope(gp, 1, null) == -1 and b"capture is off" in L.tarl_last_error()      # on for another handle only
    assert scope(fp, 2, null) == -1 and scope(fp, -1, null) == -1 and b"scope must" in L.tarl_last_error()
    assert scope(fp, 0, fake) == -1 and b"counts2" in L.tarl_last_error()
    for s, c in ((1, null), (1, fake), (0, null), (1, fake)):
        assert scope(fp, s, c) == 0 and f.policy_hold == 8
    assert cap(fp, 0, null) == 0 and f.policy_hold == 0
    assert scope(fp, 1, null) == -1 and b"capture is off" in L.tarl_last_error()      # the switch cleared it
    assert L.tarl_fused_set_policy_hold(fp, 1, null) == 0 and f.policy_hold == 1
    assert scope(fp, 1, null) == -1                                                   # another switch's bit is not this one's
    assert cap(fp, 1, fake) == 0 and scope(fp, 1, fake) == 0 and f.policy_hold == 9
    assert cap(fp, 0, null) == 0 and L.tarl_fused_set_policy_hold(fp, 0, null) == 0 and f.policy_hold == 0


class _P:
    num_nodes, num_edges, handle = 4, 8, None


class _FS:
    B, N, A, Nmax, ref = 2, 4, 3, 15, None
    hdp = torch.zeros((4, 2, 2), dtype=torch.int32)


def test_the_ops_refuse_host_tensors_and_bad_arguments():
    from tarl_hip import lib, ops
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    p = inspect.signature(ops.fused_head_rows).parameters
    assert p["t"].default is None and p["counts"].default is None
    p = inspect.signature(ops.fused_set_head_capture).parameters
    assert p["scope"].default == "headed" and p["counts"].default is None
    p = inspect.signature(ops.decision_advantage).parameters
    assert p["agent_road"].default is None and p["bootstrap"].default is False and p["bootstrapped"].default is None
    assert list(inspect.signature(ops.fused_agent_roads).parameters) == ["plan", "fs", "Nmax", "out", "bad"]
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_head_rows(_P(), _FS(), i32(2), i32(2), i32(2, 4), t=100.0)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_agent_roads(_P(), _FS(), 15)
    with pytest.raises(ValueError, match="scope must be"):
        ops.fused_set_head_capture(_FS(), True, i32(2, 4), scope="other")
    with pytest.raises(ValueError, match="switched-on capture"):
        ops.fused_set_head_capture(_FS(), False, scope="due")
    with pytest.raises(ValueError, match="belongs to scope 'due'"):
        ops.fused_set_head_capture(_FS(), True, i32(2, 4), counts=i32(2))
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.fused_set_head_capture(_FS(), True, i32(2, 4), scope="due", counts=i32(2))
    kw = dict(B=2, timestep=1, adv_raw=torch.zeros(2, 4), truncated=i32(1), bad=i32(1))
    args = (_P(), i32(2, 4), i32(2), i32(2), i32(2), torch.zeros(2, 3, 9), torch.zeros(5), 4,
            torch.zeros(2, 4, dtype=torch.float64), i32(4))
    with pytest.raises(ValueError, match="bootstrap needs"):
        ops.decision_advantage(*args, bootstrap=True, **kw)
    with pytest.raises(lib.TarlError, match="GPU"):
        ops.decision_advantage(*args, agent_road=i32(2, 3), bootstrap=True, bootstrapped=i32(1), **kw)


# ---- 5. argument rules -----------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn+ppo", scenario="synthetic-1024-1024", mode="train", policy_head="goal_mlp")
    base.update(kw)
    return RunnerArgs(**base)


def test_runner_args_rules():
    assert _args().credit_scope is None and _args().credit_horizon is None
    a = _args(credit="decision", credit_scope="due", credit_horizon="bootstrap", credit_baseline="learned", credit_gamma=0.99)
    assert (a.credit_scope, a.credit_horizon) == ("due", "bootstrap")
    assert _args(credit="decision", credit_scope="headed", credit_horizon="charge").credit_scope == "headed"
    for kw in (dict(credit_scope="due"), dict(credit_horizon="bootstrap"), dict(credit_scope="headed"),
               dict(credit_horizon="charge")):
        with pytest.raises(ValueError, match="needs credit decision"):       # the refusals of credit_gamma
            _args(**kw)
    with pytest.raises(ValueError, match="credit_scope must be"):
        _args(credit="decision", credit_scope="other")
    with pytest.raises(ValueError, match="credit_horizon must be"):
        _args(credit="decision", credit_horizon="other")
    with pytest.raises(ValueError, match="mode 'train'"):
        _args(credit="decision", credit_scope="due", mode="eval", algo="mpnn", eval_envs=2)
    with pytest.raises(ValueError, match="state-dependent head"):
        _args(credit="decision", credit_horizon="bootstrap", policy_head="embedding")


def test_parser_flags():
    from src.runner import RunnerArgs
    main = importlib.import_module("main")
    ns = main.build_parser().parse_args([])
    assert ns.credit_scope is None and ns.credit_horizon is None
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", "--credit",
                                         "decision", "--credit-scope", "due", "--credit-horizon", "bootstrap"])
    a = RunnerArgs(**vars(ns))
    assert (a.credit_scope, a.credit_horizon) == ("due", "bootstrap")
    for flag, value in (("--credit-scope", "due"), ("--credit-horizon", "bootstrap")):
        ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "goal_mlp", flag, value])
        with pytest.raises(ValueError, match="needs credit decision"):
            RunnerArgs(**vars(ns))
        with pytest.raises(SystemExit):
            main.build_parser().parse_args([flag, "other"])


def test_the_layers_take_the_arguments():
    from src.rl.ppo_trainer import ppo_train
    from tarl_hip.trainer import VecPPOTrainer
    for fn in (ppo_train, VecPPOTrainer.__init__):
        p = inspect.signature(fn).parameters
        assert p["credit_scope"].default == "headed" and p["credit_horizon"].default == "charge"
    with pytest.raises(ValueError, match="credit_scope narrows the per-decision credit: it needs credit decision"):
        ppo_train(None, None, None, credit_scope="due")
    with pytest.raises(ValueError, match="credit_horizon closes the per-decision return: it needs credit decision"):
        ppo_train(None, None, None, credit_horizon="bootstrap")


def test_trainer_refusals_without_a_device():
    from tarl_hip.trainer import VecPPOTrainer
    check = VecPPOTrainer._check_credit_scope
    check("joint", "headed", "charge")
    check("decision", "due", "bootstrap")
    with pytest.raises(ValueError, match="credit_scope narrows the per-decision credit: it needs credit decision"):
        check("joint", "due", "charge")
    with pytest.raises(ValueError, match="credit_horizon closes the per-decision return: it needs credit decision"):
        check("joint", "headed", "bootstrap")
    with pytest.raises(ValueError, match="credit_scope must be"):
        check("decision", "other", "charge")
    with pytest.raises(ValueError, match="credit_horizon must be"):
        check("decision", "due", "other")
