"""GPU: the accumulator banks of the fused frame (csrc/fused_insert.hip: acc_lp / acc_n / acc_w, ``FusedState(acc_slots=...)``).

The insert launch reads the log-prob banks only where a log-prob is asked for, re-arms a bank only where it does not
already hold zero, and the number of banks is a constructor argument. None of this may change a result: the banks hold
exact sums (small integers in fp32, fixed-point log-probs in int64), so every output is compared bit for bit — across bank
counts, across the three rollout modes (TARL_ROLLOUT_MERGE, read once per process: a child process each), against the
one-wave-per-environment insert kernel on a backlog that overflows the packed kernel's candidate list, and across
consecutive calls on one engine. After every call all bank arrays must hold zero bits.

Run as a script (``python tests/test_gpu_insert_banks.py <scenario> <out.pt>``) this file computes one scenario under the
knobs of its environment and saves the outputs; the tests start it for the knobs that are fixed per process."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 21540            # the clock of the first frame after a reset
INS_CAP = 192         # csrc/fused_common.h: candidate list of an insert workgroup (shared by the environments of a wave)


def banks_are_zero(fs):
    """All three bank arrays (and the second log-prob buffer of the merged launch) hold zero bits."""
    arrays = {"acc_lp": fs.acc_lp, "acc_n": fs.acc_n.view(torch.int32), "acc_w": fs.acc_w.view(torch.int32)}
    if getattr(fs, "acc_scratch", None) is not None:
        arrays["acc_scratch"] = fs.acc_scratch
    bad = {k: int(v.ne(0).sum()) for k, v in arrays.items() if bool(v.ne(0).any())}
    assert not bad, f"banks not zero after the call: {bad}"


def make_engine(B, A, window, acc_slots=None, torus=3):
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    net = synth.torus_network(torus, torus, heterogeneous=True, seed=3)
    N = net.num_roads
    pops = torch.stack([synth.population(A, N, seed=b, t0=T0, t1=T0 + window) for b in range(B)])
    e = SimEngine(net.x.unsqueeze(0).repeat(B, 1, 1).cuda(), net.edge_index, net.edge_attr, net.Nmax, pops.cuda(),
                  congestion_constant=net.congestion_constant, seed=9, acc_slots=acc_slots)
    e.reset()
    e.prepare_policy(torch.randn(N, generator=torch.Generator().manual_seed(5)).cuda())
    return e


def rollout(e, T, want_lp=True):
    """One rollout_fused call -> its outputs on the host; the banks are checked right after it."""
    N, B = e.N, e.B
    ch = torch.zeros((T, N, B), dtype=torch.uint8, device="cuda")
    lp = torch.zeros((T, B), device="cuda") if want_lp else None
    rw = torch.zeros((T, B), device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    leg = torch.zeros((T, B, 2), dtype=torch.int32, device="cuda")
    e.rollout_fused(T, choice=ch, log_prob=lp, reward=rw, counts=ct, leg=leg)
    banks_are_zero(e.fs)
    out = {"choice": ch.cpu(), "reward": rw.cpu(), "counts": ct[1:].cpu(), "leg": leg.cpu()}
    if want_lp:
        out["log_prob"] = lp.cpu()
    return out


def final_state(e):
    """Exported state, agent tables and the packed records a later frame reads."""
    fs = e.fs
    return {"x": e.x.cpu(), "agents": e.agents.cpu(), "count": fs.count.cpu(), "sel8": fs.sel8.cpu(),
            "a_status": fs.a_status.cpu(), "cur_lo": fs.cur_lo.cpu()}


def same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{what}: {k} differs"


def cat(outs):
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


# ---- scenarios (also run in child processes) ---------------------------------------------------------------------------
def scenario_modes():
    """B = 13, 300 agents due in the first 8 s, T = 12. One engine takes three calls with a log-prob buffer, a second one
    the same three calls with the buffer only in the middle one."""
    T = 12
    e_with, e_mixed = make_engine(13, 300, 8), make_engine(13, 300, 8)
    res = {}
    for c in range(3):
        a = rollout(e_with, T, True)
        b = rollout(e_mixed, T, c == 1)
        for k, v in a.items():
            res[f"with{c}.{k}"] = v
        for k, v in b.items():
            res[f"mixed{c}.{k}"] = v
    for k, v in final_state(e_with).items():
        res["with.final." + k] = v
    for k, v in final_state(e_mixed).items():
        res["mixed.final." + k] = v
    return res


def scenario_backlog():
    """B = 9 (the last wave of the eight- and of the four-environment kernel holds one environment), 180 agents per environment (fewer
    than the whole list holds) all due in the first second, T = 16, for the default bank count and for 3 banks."""
    res = {}
    for acc in (None, 3):
        e = make_engine(9, 180, 0, acc_slots=acc)
        for k, v in rollout(e, 16, True).items():
            res[f"acc{acc}.{k}"] = v
        for k, v in final_state(e).items():
            res[f"acc{acc}.final.{k}"] = v
    return res


SCENARIOS = {"modes": scenario_modes, "backlog": scenario_backlog}


def children(scenario, tmp_path, knob, values):
    """One child process per value of the knob, side by side -> {value: the scenario's outputs}."""
    procs = {}
    for v in values:
        out = os.path.join(str(tmp_path), f"{scenario}_{knob}_{v}.pt")
        procs[v] = (out, subprocess.Popen([sys.executable, os.path.abspath(__file__), scenario, out],
                                          env=dict(os.environ, **{knob: v}), stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True))
    res = {}
    for v, (out, p) in procs.items():
        log = p.communicate(timeout=300)[0]
        assert p.returncode == 0, f"{knob}={v}: " + log[-3000:]
        res[v] = torch.load(out)
    return res


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [13, 64])
def test_bank_count_does_not_matter(B):
    """acc_slots in {1, 3, 8, 32}: reward, leg, log-prob, counts, actions, final packed state and agent tables identical,
    banks zero after the call (checked in rollout()). 300 agents due within 10 s on 36 roads of 6 .. 15 s: the 16 frames
    admit agents and withdraw the first arrivals, so acc_n AND acc_w are filled — asserted from the leg histogram."""
    T = 16
    ref = ref_state = None
    for acc in (32, 1, 3, 8):
        e = make_engine(B, 300, 10, acc_slots=acc)
        assert e.fs.acc_slots == acc and tuple(e.fs.acc_n.shape) == (acc, B)
        out, st = rollout(e, T), final_state(e)
        if ref is None:
            ref, ref_state = out, st
            leg = out["leg"]
            print(f"B={B}: departed {int(leg[..., 0].sum())}, arrived {int(leg[..., 1].sum())} in "
                  f"{int((leg[..., 1] > 0).any(dim=1).sum())} of {T} frames")
            assert int(leg[..., 0].sum()) > 0, "nobody was admitted: the test would pass on zeros"
            assert int(leg[..., 1].sum()) > 0, "nobody was withdrawn: acc_w stayed zero in every frame"
            assert bool(((leg[..., 0] > 0).any(dim=1) & (leg[..., 1] > 0).any(dim=1)).any()), \
                "no frame both admits and withdraws"
            assert float(out["reward"].abs().sum()) > 0 and bool(torch.isfinite(out["log_prob"]).any())
        else:
            same(out, ref, f"acc_slots={acc} against 32")
            same(st, ref_state, f"acc_slots={acc} against 32 (final state)")


def test_rollout_modes_agree(tmp_path):
    """TARL_ROLLOUT_MERGE = 0, 1, 2 in a child process each: identical outputs (log-probs bit for bit, -inf at the same
    places), and in every mode a call without a log-prob buffer before or after a call with one changes nothing."""
    res = children("modes", tmp_path, "TARL_ROLLOUT_MERGE", ("2", "1", "0"))
    ref = res["2"]
    assert float(ref["with0.reward"].abs().sum()) > 0
    lp = ref["with1.log_prob"]
    assert bool(torch.isfinite(lp).any()) and float(lp[torch.isfinite(lp)].abs().sum()) > 0
    for m, r in res.items():
        assert r.keys() == ref.keys()
        for k in ref:
            if ref[k].is_floating_point():
                assert torch.equal(torch.isneginf(r[k]), torch.isneginf(ref[k])), f"mode {m} against mode 2: -inf of {k}"
            assert torch.equal(r[k], ref[k]), f"mode {m} against mode 2: {k} differs"
        # the engine whose first and third call had no log-prob buffer against the one that always had it
        for c in range(3):
            for k in ("choice", "reward", "counts", "leg"):
                assert torch.equal(r[f"mixed{c}.{k}"], r[f"with{c}.{k}"]), f"mode {m}, call {c}: {k} differs"
        assert torch.equal(r["mixed1.log_prob"], r["with1.log_prob"]), f"mode {m}: log-probs after a call without buffer"
        for k in ("x", "agents", "count", "sel8", "a_status", "cur_lo"):
            assert torch.equal(r["mixed.final." + k], r["with.final." + k]), f"mode {m}: final {k}"


def test_long_backlog_falls_back_to_one_environment_body(tmp_path):
    """Every agent due in the first second: with eight environments per wave (TARL_INSERT_EPW=8) an environment's share of
    the candidate list is 24 entries, with four (TARL_INSERT_EPW=4) 48, and an environment that admits more than its share
    in a frame had more candidates than that — it sat the packed part out and went through the one-environment body.
    (The 180 agents of an environment are all candidates of the first frame; on the CPU, from the origins and the roads'
    capacities, that frame admits 132 or more of them in every environment under any of 2 000 random actions.) Against the
    one-wave-per-environment kernel (TARL_INSERT_EPW=1): identical, for 32 banks and for 3."""
    res = children("backlog", tmp_path, "TARL_INSERT_EPW", ("8", "4", "1"))
    single = res["1"]
    departed = single["accNone.leg"][..., 0]                     # [T][B]
    for epw in (8, 4):
        over = departed > INS_CAP // epw
        n_env, n_frames = int(over.any(dim=0).sum()), int(over.sum())
        print(f"EPW {epw}: {n_env} of {departed.size(1)} environments overflowed their share of the list ({n_frames} (frame, "
              f"environment) pairs; most admitted in one frame: {int(departed.max())})")
        assert n_env >= 2, f"EPW {epw}: no wave had several environments over their share: the fall-back was not exercised"
        assert bool(over[:, 8].any()), f"EPW {epw}: the environment alone in the last wave did not overflow"
    assert int(single["accNone.leg"][..., 1].sum()) > 0, "nobody was withdrawn"
    for epw in ("8", "4"):
        packed = res[epw]
        assert packed.keys() == single.keys()
        for k in single:
            assert torch.equal(packed[k], single[k]), f"EPW {epw} against EPW 1: {k} differs"
    for k in single:
        if k.startswith("accNone."):
            assert torch.equal(single["acc3." + k[8:]], single[k]), f"3 banks against 32: {k[8:]} differs"


def test_consecutive_collects_and_reset():
    """Two rollouts back to back (7 + 9 frames: an episode end splits a collector batch at any length) == one rollout of
    16 == 16 calls of frame_fused; then reset + rollout == reset + frame loop. Banks zero after every call."""
    B, T1, T2 = 13, 7, 9
    T = T1 + T2
    e_split, e_one, e_loop = (make_engine(B, 300, 10) for _ in range(3))
    N = e_loop.N

    def frame_loop(n):
        ch, lp = torch.zeros((n, N, B), dtype=torch.int32, device="cuda"), torch.zeros((n, B), device="cuda")
        rw, ct = torch.zeros((n, B), device="cuda"), torch.zeros((n, N, B), device="cuda")
        for t in range(n):
            e_loop.frame_fused(choice=ch[t], log_prob=lp[t], reward=rw[t], counts=ct[t])
            banks_are_zero(e_loop.fs)
        return {"reward": rw.cpu(), "log_prob": lp.cpu(), "counts": ct.to(torch.uint8).cpu()}

    split = cat([rollout(e_split, T1), rollout(e_split, T2)])
    one = rollout(e_one, T)
    loop = frame_loop(T)
    assert float(one["reward"].abs().sum()) > 0 and int(one["leg"][..., 1].sum()) > 0
    same(split, one, "7 + 9 frames against 16")
    same(final_state(e_split), final_state(e_one), "7 + 9 frames against 16 (final state)")
    for k in loop:
        assert torch.equal(loop[k], one[k]), f"frame loop against rollout: {k} differs"
    assert torch.equal(e_loop.x, e_one.x) and torch.equal(e_loop.agents, e_one.agents)
    # a reset between rollouts: the banks are zero when it comes, and the sums of the next episode are complete
    e_one.reset()
    e_loop.reset()
    banks_are_zero(e_one.fs)
    again, loop = rollout(e_one, T1), frame_loop(T1)
    assert float(again["reward"].abs().sum()) > 0
    for k in loop:
        assert torch.equal(loop[k], again[k]), f"after reset, frame loop against rollout: {k} differs"
    assert torch.equal(e_loop.x, e_one.x) and torch.equal(e_loop.agents, e_one.agents)


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tarl-simulator_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.save(SCENARIOS[sys.argv[1]](), sys.argv[2])
