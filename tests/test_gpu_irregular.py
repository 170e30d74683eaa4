"""GPU: the frame and rollout kernels on irregular road graphs (tests/irregular_graphs.py: hubs with up to nine, and with
126, in- and out-edges, dead ends, feeder links, an edge list in no order). One comparison chain, bit-exact throughout
(log-probs to fp32 rounding): CPU oracle -> per-op kernels (sim.hip, agents.hip) -> fused frame (fused_*.hip) -> one-call
rollouts (fused_rollout.hip's launcher, rollout_env.hip's LDS-resident workgroup). tests/test_irregular_host.py shows on the CPU
that these inputs drive traffic through in-edges of in-rank >= 4 and out-edges of out-rank >= 4 hundreds of times, and that
an implementation which dropped them, or broke ties the other way, would leave the oracle's trajectory.
The MIXED tests come first in the file, the HUB126 tests last."""
import os
import subprocess
import sys

import pytest
import torch

import irregular_graphs as ig
from test_gpu_fused import LP_RTOL, fused_vs_unfused_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


def plan_of(ops, net):
    """The device plan, checked against the host restatement the CPU suite reasons about."""
    plan = ops.Plan(net.edge_index, net.num_roads)
    f = ig.plan_facts(net)
    assert (plan.src_sorted, plan.siblings4, plan.row_siblings, plan.num_row_chunks, plan.max_in, plan.max_out) == \
        (f["src_sorted"], f["siblings4"], f["row_siblings"], f["num_row_chunks"], f["max_in"], f["max_out"])
    assert plan.num_groups == int((ig.degrees(net)[1] > 0).sum())      # the roads that draw an action
    return plan


def core_step_case(ops, name):
    """B = 3 random mid-simulation states in one launch (strided views), five steps of tarl_core_step against
    sim.core_step: state, per-edge delta_travel_time and the pop mask. Environment 0 starts with a crafted tie: bit-equal
    maximal scores on in-ranks 3 and 4 of the longest race (the oracle's first-maximum rule decides). On the long-FIFO
    graphs (LONG127, LONGMIX: every in-degree four) the tie sits on in-ranks 2 and 3, and the random states hold up to 125
    agents per road: the per-op kernels on counts, shifts and slot indices beyond 63."""
    from oracle import sim
    net = ig.graph(name)
    R, F, E, Nmax = net.num_roads, net.F, net.edge_index.size(1), net.Nmax
    B, t0 = 3, 200.0
    long_fifo = name in ig.LONG_GRAPHS
    xs = [ig.random_state(net, seed=100 + b, t=t0) for b in range(B)]
    ea, e3, e4, road = ig.tie_case(net, xs[0], t0, in_degree=int(ig.degrees(net)[0].max()), which=ig.TIE_WHICH.get(name, 0),
                                   ranks=(2, 3) if long_fifo else (3, 4))
    top = max(int(xb[:, 3 * Nmax + 1].max()) for xb in xs)
    plan = plan_of(ops, net)
    ec = ops.EdgeConst(ea, "cuda")
    cc = dev(net.congestion_constant)
    big = torch.zeros((B, R + 3, F + 5), device="cuda")        # odd env / row strides on purpose
    x = big[:, :R, :F]
    x.copy_(torch.stack(xs))
    gen = torch.Generator().manual_seed(7)
    counters, total_pops = ig.new_counters(), 0
    for s in range(5):
        t = t0 + s
        u = torch.rand((B, E), generator=gen)
        if s == 0:
            u[0] = ig.tie_uniform(u[0], net, road, e3, e4)
        dtt, popped = ops.core_step(plan, x, Nmax, ec, t, congestion_constant=cc, gumbel=dev(ops.gumbel_from_uniform_cpu(u)))
        for b in range(B):
            shadow = xs[b].clone()
            ig.core_step_counted(shadow, net, t, u[b], counters, edge_attr=ea)
            _, dref, pref = sim.core_step(xs[b], net.edge_index, ea, t, Nmax, uniform=u[b],
                                          congestion_constant=net.congestion_constant)
            assert torch.equal(shadow, xs[b])
            assert torch.equal(x[b].cpu(), xs[b]), f"env {b} step {s}"
            assert torch.equal(dtt[b].cpu(), dref) and torch.equal(popped[b].cpu().bool(), pref), f"env {b} step {s}"
            total_pops += int(pref.sum())
            top = max(top, int(xs[b][:, 3 * Nmax + 1].max()))
    print(f"\ncore step {name}: pops {total_pops} largest count {top} {counters}")
    assert total_pops > 0
    if long_fifo:
        assert 120 <= top < Nmax      # (relief admissions on these graphs: env_chain_case)
    else:
        assert counters["a_tail_admissible"] > 0 and counters["d_tail_response"] > 0 and counters["e_relief_admissions"] > 0
        assert counters["c_tail_wins"] > 0
    assert float(big[:, R:, :].abs().sum()) == 0 and float(big[:, :, F:].abs().sum()) == 0      # padding untouched


def test_core_step_vs_oracle_mixed(ops):
    core_step_case(ops, "MIXED")


def env_chain_case(ops, name, frames, t1=130):
    """apply_action, core_step, withdraw_step, insert_step against sim.env_step: B = 3, the census population of the graph
    (MIXED: 40 agents per road due within 30 s: backlog, relief admissions; LONGMIX: 150 per road due by ``t1``, FIFOs of
    up to 126), uniform random valid actions; state, agents and reward per environment and frame."""
    from oracle import sim
    net = ig.graph(name)
    N, Nmax, E = net.num_roads, net.Nmax, net.edge_index.size(1)
    adj = net.dense_adjacency()
    B = 3
    plan = plan_of(ops, net)
    ec = ops.EdgeConst(net.edge_attr, "cuda")
    cc = dev(net.congestion_constant)
    pops = [ig.population(net, ig.CENSUS[name]["per_road"], seed=20 + b, t1=t1) for b in range(B)]
    xs = [net.x.clone() for _ in range(B)]
    x, ag = dev(torch.stack(xs)), dev(torch.stack(pops))
    reward = torch.empty(B, device="cuda")
    gen = torch.Generator().manual_seed(3)
    counters, top, most_inserted = ig.new_counters(), 0, 0
    for s in range(frames):
        t = 100 + s
        before = [float(p[:, sim.ON_WAY].sum() + p[:, sim.DONE].sum()) for p in pops]
        choice = ig.random_actions(net, gen, B)
        u = torch.rand((B, E), generator=gen)
        ops.apply_action(plan, x, Nmax, choice=dev(choice))
        ops.core_step(plan, x, Nmax, ec, t, congestion_constant=cc, gumbel=dev(ops.gumbel_from_uniform_cpu(u)))
        ops.withdraw_step(plan, x, Nmax, ag, t)
        ops.insert_step(x, Nmax, ag, t, congestion_constant=cc, reward=reward)
        for b in range(B):
            onehot = ig.onehot_of(choice[b], E)
            shadow_x, shadow_a = xs[b].clone(), pops[b].clone()
            ig.env_step_counted(shadow_x, shadow_a, net, adj, onehot, t, u[b], counters)
            out = sim.env_step(xs[b], pops[b], net.edge_index, net.edge_attr, adj, onehot, t, Nmax, uniform=u[b],
                               congestion_constant=net.congestion_constant)
            assert torch.equal(shadow_x, xs[b]) and torch.equal(shadow_a, pops[b])
            assert torch.equal(x[b].cpu(), xs[b]), f"env {b} step {s}"
            assert torch.equal(ag[b].cpu(), pops[b]), f"agents env {b} step {s}"
            assert reward[b].item() == out["reward"].item()
            top = max(top, int(xs[b][:, 3 * Nmax + 1].max()))
            most_inserted = max(most_inserted, int(pops[b][:, sim.ON_WAY].sum() + pops[b][:, sim.DONE].sum() - before[b]))
    print(f"\nenv chain {name}: largest count {top}, most agents inserted in one frame {most_inserted}, {counters}")
    assert sum(float(p[:, sim.DONE].sum()) for p in pops) > 0
    if name in ig.LONG_GRAPHS:
        assert counters["e_relief_admissions"] > 0 and 100 <= top < Nmax
    else:
        assert min(counters[k] for k in ig.COUNTERS) > 0
    return top, most_inserted


def test_env_step_chain_vs_oracle(ops):
    env_chain_case(ops, "MIXED", 40)


def fused_frame_case(ops, name, B, frames, *, t1=130, visit=None, repack_at=None):
    """The frame loop of test_fused_equals_unfused_frame_by_frame on the irregular graphs, host-supplied noise. On MIXED,
    at frame 30 (traffic is flowing) two upstream rows of the nine-in-edge road get a raw SELECTED_ROAD — a road that is
    none of their neighbours — on both sides, the fused state is packed again, and five frames run without the choice phase:
    the Direction gather's exact ``redo`` pass then walks a nine-entry in-list. On the sibling graphs (SIBS, SIBS_TAILS) the
    nine-in-edge road is a non-zero sibling, and road 0 gets a raw code too: road 0 is what the padding records of a short
    in-list name, so the sibling gather repeats the pass of chunks that did not need it — which must change nothing. The
    long-FIFO graphs (LONG127, LONGMIX) are 2 x 2 tori: every degree four, the sibling gather and the quad draw; ``t1`` is
    the last departure of the populations, ``visit`` / ``repack_at`` are handed to the frame loop."""
    net = ig.graph(name)
    plan = plan_of(ops, net)
    raw_sel, pop_seed = None, 40
    if name in ("MIXED", "SIBS", "SIBS_TAILS"):
        sibs = name != "MIXED"
        assert plan.max_in == 9 and plan.siblings4 == sibs
        assert plan.num_groups == net.num_roads if sibs else plan.num_row_chunks > net.num_roads // 4
        road = int(torch.nonzero(ig.degrees(net)[0] == 9)[ig.TIE_WHICH.get(name, 0)])
        ups = net.edge_index[0][net.edge_index[1] == road][[2, 6]].tolist()      # one embedded record, one of the tail
        lists = ig.out_lists(net)
        far = [next(c for c in order if c not in lists[j] and c != road)      # two different roads, no neighbours
               for j, order in zip(ups, (range(net.num_roads), reversed(range(net.num_roads))))]
        if sibs and 0 not in ups:
            assert road % 4 != 0 and int((ig.degrees(net)[0] < 4).sum()) > 0
            ups, far = ups + [0], far + [next(c for c in range(1, net.num_roads) if c not in lists[0])]
        raw_sel = (30, 5, ups, far)
    elif name in ig.LONG_GRAPHS:
        assert plan.siblings4 and plan.max_in == 4 and plan.max_out == 4 and net.Nmax == 127
        assert plan.num_groups == net.num_roads and net.num_roads % 4 == 0      # the quad draw
        pop_seed = LONG_POP_SEED
    else:
        assert plan.max_in == 126 and plan.max_out == 126
    pops = torch.stack([ig.population(net, ig.CENSUS[name]["per_road"], seed=pop_seed + b, t1=t1) for b in range(B)])
    events, a1 = fused_vs_unfused_frames(ops, net, plan, pops, frames, raw_sel=raw_sel, visit=visit, repack_at=repack_at)
    assert events > 0 and float(a1[:, :, 8].sum()) > 0


def test_fused_frame_vs_per_op_kernels_mixed(ops):
    fused_frame_case(ops, "MIXED", 5, 60)


def fused_tie_case(ops, name):
    """Crafted ties across the 4 / 5 boundary of the longest race (equal turn probability and equal Gumbel noise on
    in-ranks 3 and 4, both admissible, every other in-edge behind): packed, one fused frame without the choice phase
    against core_step + withdraw + insert on the reference layout — which test_core_step_vs_oracle pins to the oracle's
    first-maximum rule on the same construction."""
    net = ig.graph(name)
    N, Nmax, E = net.num_roads, net.Nmax, net.edge_index.size(1)
    B, t = 4, 200.0
    xs, us = [], torch.rand((B, E), generator=torch.Generator().manual_seed(9))
    for b in range(B):
        xb = ig.random_state(net, seed=60 + b, t=t)
        ea, e3, e4, road = ig.tie_case(net, xb, t, in_degree=int(ig.degrees(net)[0].max()), which=ig.TIE_WHICH.get(name, 0))
        us[b] = ig.tie_uniform(us[b], net, road, e3, e4)
        xs.append(xb)
    A = int(torch.stack(xs)[:, :, :Nmax].max()) + 2
    ag = torch.zeros((B, A, 9))
    ag[:, :, 1] = torch.randint(0, N, (B, A), generator=torch.Generator().manual_seed(4)).float()
    ag[:, :, 2] = 48 * 3600.0        # nobody is waiting to be inserted
    ag[:, 1:, 7] = 1.0               # everybody queued is on the way
    plan = plan_of(ops, net)
    ec = ops.EdgeConst(ea, "cuda")
    cc = dev(net.congestion_constant)
    x1, a1 = dev(torch.stack(xs)), dev(ag)
    x2, a2 = x1.clone(), a1.clone()
    j3 = int(net.edge_index[0, e3])
    head3 = x1[:, j3, 0].clone()
    n0 = x1[:, road, 3 * Nmax + 1].long()
    fs = ops.FusedState(plan, B, A, "cuda", Nmax)
    ops.fused_pack(plan, fs, x2, Nmax, a2, cc, ec=ec)
    gum = dev(ops.gumbel_from_uniform_cpu(us))
    r1, r2 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    dtt2 = torch.empty((B, E), device="cuda")
    pop2 = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    dtt1, pop1 = ops.core_step(plan, x1, Nmax, ec, t, congestion_constant=cc, gumbel=gum)
    admitted = torch.stack([(x1[b, road, :int(n0[b]) + 1] == head3[b]).any() for b in range(B)])
    ops.withdraw_step(plan, x1, Nmax, a1, t)
    ops.insert_step(x1, Nmax, a1, t, congestion_constant=cc, reward=r1)
    ops.fused_frame(plan, fs, None, a2, ec, t, use_cong=True, prev_time=t - 1, gumbel=gum, dtt=dtt2, popped=pop2, reward=r2)
    ops.fused_export(plan, fs, x2, Nmax, t)
    assert bool(admitted.all())              # rank 3's head went in: the first maximum
    assert torch.equal(x1, x2) and torch.equal(a1, a2) and torch.equal(r1, r2)
    assert torch.equal(dtt1, dtt2) and torch.equal(pop1, pop2)


def test_fused_frame_breaks_ties_like_the_per_op_kernels_mixed(ops):
    fused_tie_case(ops, "MIXED")


# The long-FIFO graphs run next to the edge of the reference's domain: the insert fills a road to MAX - 3, three relief
# admissions take it to MAX = Nmax - 1 (the DIRTY transition these tests are after), a fourth to Nmax — outside the domain,
# flagged, and no subject of a parity test. How often that happens is a property of the inputs: with the policy embedding
# the other graphs use (seed 5) some environment of 130 left the domain within 300 frames under every one of 1 500 engine
# seeds (LONGMIX, also at 120 agents per road); with seed 7, at 150 agents per road and the engine seed unchanged, all of
# B = 5 and 130 on both graphs stay inside (13 of 20 engine seeds do at LONGMIX / 130, 19 or 20 elsewhere). Host noise: the
# populations 40 + b take one of 130 LONGMIX environments to Nmax in frame 42, the populations 1000 + b none.
LONG_EMB_SEED, LONG_POP_SEED = 7, 1000


def _engines(net, B, per_road, kinds, emb_seed=5):
    from tarl_hip.engine import SimEngine
    N = net.num_roads
    pops = torch.stack([ig.population(net, per_road, seed=b, t0=21540, t1=21570) for b in range(B)])
    emb = torch.randn(N, generator=torch.Generator().manual_seed(emb_seed)).cuda()
    out = []
    for fused in kinds:
        e = SimEngine(dev(net.x.unsqueeze(0).repeat(B, 1, 1)), net.edge_index, net.edge_attr, net.Nmax, dev(pops.clone()),
                      congestion_constant=net.congestion_constant, seed=9, fused=fused)
        e.reset()
        if fused:
            e.prepare_policy(emb)
        out.append(e)
    return emb, out


def rollout_case(ops, setenv, name, B, T):
    """Device Philox noise everywhere, the same seeds on every engine: T calls of frame_fused (the reference of this
    case, itself compared with the per-op engine frame by frame), SimEngine.rollout_fused with TARL_ROLLOUT_MERGE 1 and 2,
    SimEngine.rollout_env; a second rollout from the state the first left; five frames of frame_fused after rollout_env.
    The first two environments keep the per-node series (dtt_node, events). On the long-FIFO graphs the uint8 count
    buffers of every rollout are read as bytes: some reach 64, none reaches Nmax = 127, and every reward is minus their
    sum. Returns (count bytes >= 64 seen, the largest count byte)."""
    net = ig.graph(name)
    N, E, M = net.num_roads, net.edge_index.size(1), 2
    emb, (e0, e1, m1, m2, ev) = _engines(net, B, ig.CENSUS[name]["per_road"], [False, True, True, True, True],
                                         emb_seed=LONG_EMB_SEED if name in ig.LONG_GRAPHS else 5)
    plan_of(ops, net)
    assert ev.env_rollout_supported and (name != "HUB126" or 256 < N <= 512)
    src = net.edge_index[0].cuda()
    has_out = dev(ig.degrees(net)[1] > 0)
    ch1, lp1, rw1 = (torch.zeros((T, N, B), dtype=torch.int32, device="cuda"), torch.zeros((T, B), device="cuda"),
                     torch.zeros((T, B), device="cuda"))
    ct1 = torch.zeros((T + 1, N, B), device="cuda")
    dtt, pop, wd = (torch.empty((B, E), device="cuda"), torch.empty((B, N), dtype=torch.uint8, device="cuda"),
                    torch.empty((B, N), dtype=torch.uint8, device="cuda"))
    _, orank = (r.cuda() for r in ig.edge_ranks(net.edge_index, N))
    short_out = dev((ig.degrees(net)[1] > 0) & (ig.degrees(net)[1] < 4))
    high_picks, short_picks = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    bufs, bytes_ge64, top_byte = {}, 0, 0
    for key, env_minor in (("m1", True), ("m2", True), ("env", False)):
        shp = (lambda t, k: (t, N, k)) if env_minor else (lambda t, k: (t, k, N))
        bufs[key] = dict(choice=torch.zeros(shp(T, B), dtype=torch.uint8, device="cuda"),
                         log_prob=torch.zeros((T, B), device="cuda"), reward=torch.zeros((T, B), device="cuda"),
                         counts=torch.zeros(shp(T + 1, B), dtype=torch.uint8, device="cuda"),
                         dtt_node=torch.full(shp(T, M), -1.0, device="cuda"),
                         events=torch.full(shp(T, M), 255, dtype=torch.uint8, device="cuda"))
    for rep in range(2):
        dtt_ref, ev_ref = [], []
        for t in range(T):
            s = rep * T + t
            # the per-op engine: the action chain of test_fused_equals_unfused_on_a_matsim_graph_with_pseudo_nodes
            logits = ops.policy_edge_logits(e0.plan, e0.node_features, emb)
            p = ops.graphdist_softmax(e0.plan, logits)
            _, ch0 = ops.graphdist_sample(e0.plan, p, seed=e1.seed ^ 0x5DEECE66D, counter=s + 1, want_onehot=False,
                                          want_choice=True)
            lp0, _ = ops.graphdist_logprob_entropy(e0.plan, p, choice=ch0, want_entropy=False)
            high_picks += ((ch0 >= 0) & (orank[ch0.long().clamp(min=0)] >= 4)).sum(1)
            short_picks += ((ch0 >= 0) & short_out).sum(1)
            e0.step(choice=ch0)
            e1.frame_fused(choice=ch1[t], log_prob=lp1[t], reward=rw1[t], counts=ct1[t + 1], dtt=dtt, popped=pop, withdrawn=wd)
            assert torch.equal(ch0, ch1[t].t()), f"actions frame {s}"
            assert torch.allclose(lp0, lp1[t], rtol=LP_RTOL, atol=1e-5), f"log-prob frame {s}"
            assert torch.equal(e0.reward, rw1[t]) and torch.equal(e0.counts, ct1[t + 1].t()), f"reward / counts frame {s}"
            assert torch.equal(e0.agents, e1.agents), f"agents frame {s}"
            if s % 10 == 0 or t == T - 1:
                assert torch.equal(e0.x, e1.x), f"state frame {s}"
            node_d = torch.zeros((M, N), device="cuda")
            node_d.scatter_reduce_(1, src.expand(M, -1), dtt[:M], "amax", include_self=False)
            assert torch.equal(node_d[:, src], dtt[:M])      # delta_travel_time is a property of the edge's SOURCE road
            dtt_ref.append(node_d)
            ev_ref.append((pop | (wd << 1))[:M].clone())
        dtt_ref, ev_ref = torch.stack(dtt_ref), torch.stack(ev_ref)      # (T, M, N)
        series = {}
        for key, eng, merge in (("m1", m1, "1"), ("m2", m2, "2"), ("env", ev, None)):
            b = bufs[key]
            if merge is not None:
                setenv("TARL_ROLLOUT_MERGE", merge)
            times = (eng.rollout_env if merge is None else eng.rollout_fused)(T, metrics_envs=M, **b)
            assert len(times) == T + 1 and eng.time == e1.time
            chd, ctd = eng.decode_rollout(merge is not None, choice=b["choice"], counts=b["counts"])
            assert torch.equal(ch1.permute(0, 2, 1), chd), f"actions ({key}, rollout {rep})"
            assert torch.equal(lp1, b["log_prob"]) and torch.equal(rw1, b["reward"]), f"log-prob / reward ({key}, rollout {rep})"
            assert torch.equal(ct1[1:].permute(0, 2, 1), ctd[1:]), f"counts ({key}, rollout {rep})"
            if name in ig.LONG_GRAPHS:
                cb = b["counts"][1:]                  # (T, N, B) or (T, B, N) raw bytes, as the reward and the critic read them
                assert int(cb.max()) < net.Nmax == 127, f"count byte ({key}, rollout {rep})"
                assert torch.equal(b["reward"], -cb.sum(1 if merge is not None else 2, dtype=torch.float32)), f"reward ({key}, rollout {rep})"
                bytes_ge64, top_byte = bytes_ge64 + int((cb >= 64).sum()), max(top_byte, int(cb.max()))
            assert torch.equal(e1.x, eng.x) and torch.equal(e1.agents, eng.agents), f"state / agents ({key}, rollout {rep})"
            dn, evs = b["dtt_node"], b["events"]
            series[key] = (dn.permute(0, 2, 1), evs.permute(0, 2, 1)) if merge is not None else (dn, evs)
            assert torch.equal(series[key][1], ev_ref), f"pop / withdraw masks ({key}, rollout {rep})"
            assert torch.equal(series[key][0][:, :, has_out], dtt_ref[:, :, has_out]), f"delta_travel_time ({key}, rollout {rep})"
        for key in ("m2", "env"):      # the two rollouts against each other, roads without out-edges included
            assert torch.equal(series["m1"][0], series[key][0]) and torch.equal(series["m1"][1], series[key][1])
        assert int(ev_ref.sum()) > 0
    assert float(rw1.abs().sum()) > 0 and float(e1.agents[:, :, 8].sum()) > 0
    if name == "SIBS_TAILS":      # the reference side's draws reached what the quad draw does off the torus, in every environment
        assert int(high_picks.min()) > 0 and int(short_picks.min()) > 0, (high_picks, short_picks)
    ca, cb = torch.zeros_like(ch1[0]), torch.zeros_like(ch1[0])
    ra, rb = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    for t in range(5):      # hand the state back to the four-launch path
        e1.frame_fused(choice=ca, reward=ra)
        ev.frame_fused(choice=cb, reward=rb)
        assert torch.equal(ca, cb) and torch.equal(ra, rb)
    assert torch.equal(e1.x, ev.x) and torch.equal(e1.agents, ev.agents)
    return bytes_ge64, top_byte


@pytest.mark.parametrize("B,T", [(5, 40), (130, 40)])
def test_rollouts_equal_the_frame_loop_mixed(ops, monkeypatch, B, T):
    rollout_case(ops, monkeypatch.setenv, "MIXED", B, T)


@pytest.mark.parametrize("knob", ["TARL_ROWS_SIBLINGS=0", "TARL_ADDR32=0"])
def test_rollouts_under_developer_knobs(ops, monkeypatch, knob):
    """Consecutive row chunks instead of the chunk table (MIXED's table has partial chunks of every size) and 64-bit
    addresses in the frame kernels: the knobs are read once per process, so the MIXED rollout case runs in a child — after
    the same case has passed here."""
    rollout_case(ops, monkeypatch.setenv, "MIXED", 5, 40)
    env = dict(os.environ)
    k, v = knob.split("=")
    env[k] = v
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                        os.path.abspath(__file__) + "::test_rollouts_equal_the_frame_loop_mixed", "-k", "5-40"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the hub at the degree limit: 126 in, 126 out, 280 roads (two per thread of the LDS-resident rollout) ---------------------
def test_core_step_vs_oracle_hub126(ops):
    core_step_case(ops, "HUB126")


def test_fused_frame_vs_per_op_kernels_hub126(ops):
    fused_frame_case(ops, "HUB126", 3, 30)


def test_fused_frame_breaks_ties_like_the_per_op_kernels_hub126(ops):
    fused_tie_case(ops, "HUB126")


def test_rollouts_equal_the_frame_loop_hub126(ops, monkeypatch):
    rollout_case(ops, monkeypatch.setenv, "HUB126", 3, 25)
