"""GPU: day-to-day replanning — tarl_td_routes against ``replan_restatement.routes`` with == (the 8 x 8 torus
under uniform road times, where every tie is live, and both irregular graphs; one bin and four with a slow bin before a fast
one; one and three environments; max_hops at the longest route and one below it; more searches than workgroups; garbage-filled
outputs, the dummy row, ids out of range), tarl_fused_select_route against ``replan_restatement.select_rule`` on the exported
state (after the reset and on a live state, 1 to 65 environments, a shared plan and one per environment), the Replanner against
the restated day loop on the CPU oracle day by day, and the CLI. Every comparison is == except the relative gap (1e-12, the
tolerance of test_gpu_dynamic_gap for the same fp64 reduction).

No improvement assertion: on the CPU oracle no small two-route network showed the last day's travel time below day 0's by a
clear margin (a fork 0 -> 1 -> {2, 3} -> 4 -> 5 with 40 to 150 agents: 52.0 s -> 50.6 s at best, under 3 %, and no switch at all
once the roads are long). A FIFO releases one head per frame, so a road's density — the only congestion the road times see —
stays far below the level at which the alternative is quicker; the queueing delay sits on the shared upstream road."""
import importlib
import json

import numpy as np
import pytest
import torch

import dynamic_gap_restatement as G
import irregular_graphs as ig
import replan_restatement as R
import sp_cases as S

pytestmark = pytest.mark.gpu

SEL_RAW = 0x7F
SENTINEL = -7.0
GUARD = 64                      # int32 words in front of and behind the routes of the guarded calls


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _torus8():
    from tarl_hip import synth
    return synth.torus_network(8, 8)


# ---- 1. the routes -----------------------------------------------------------------------------------------------------------------
def _tables(kind, K, H, N, bs, fb, seed):
    """tau fp32 (K, H, N) and its envelope. "uniform": 10 s everywhere (every tie is live), with H = 4 bin 1 slow (90 s) and bin
    2 fast (5 s) so that waiting for the bin edge wins, and from the second environment on a few roads slower by multiples of
    5 s. "random": dynamic_gap_restatement.random_tau (fractional, +inf and NaN entries) with its zeros raised to 0.25 s —
    tau >= FF > 0 is the contract of the walk."""
    if kind == "uniform":
        tau = np.full((K, H, N), 10.0, np.float32)
        if H >= 4:
            tau[:, 1, :], tau[:, 2, :] = 90.0, 5.0
        rng = np.random.default_rng(seed)
        for k in range(1, K):
            slow = rng.choice(N, size=max(N // 5, 1), replace=False)
            tau[k][:, slow] += (5.0 * rng.integers(1, 4, size=slow.size)).astype(np.float32)[None, :]
    else:
        tau = G.random_tau(K, H, N, seed)
        tau[tau == 0.0] = 0.25
    return tau, G.envelope(tau, bs, fb)


def _run_routes(plan, tau, env, ag, bs, fb, max_hops, fill=-77):
    """ops.td_routes into garbage-filled outputs, the routes between two guard bands -> (best, routes, route_len) on the host;
    asserts that the guards and every word from a route's length on kept their fill."""
    from tarl_hip import ops
    K, A = ag.shape[:2]
    flat = torch.full((2 * GUARD + K * A * max_hops,), fill, dtype=torch.int32, device="cuda")
    out = (torch.full((K, A), float("nan"), dtype=torch.float64, device="cuda"),
           flat[GUARD:GUARD + K * A * max_hops].view(K, A, max_hops),
           torch.full((K, A), fill, dtype=torch.int32, device="cuda"))
    best, rt, ln = ops.td_routes(plan, _cuda(tau), _cuda(env), _cuda(ag), bin_seconds=bs, first_bin=fb, max_hops=max_hops, out=out)
    assert best is out[0] and rt is out[1] and ln is out[2]
    flat_h = flat.cpu()
    assert bool((flat_h[:GUARD] == fill).all()) and bool((flat_h[-GUARD:] == fill).all()), "a write outside the routes"
    best, rt, ln = best.cpu().numpy(), rt.cpu().numpy(), ln.cpu().numpy()
    assert not np.isnan(best).any() and not (ln == fill).any()                  # every best and route_len entry written
    tail = np.arange(max_hops)[None, None, :] >= np.maximum(ln, 0)[..., None]
    assert (rt[tail] == fill).all(), "words from the length on (a whole row without a route) are left as allocated"
    return best, rt, ln


def _assert_routes(plan, edges, N, tau, env, ag, bs, fb, max_hops, full=None):
    """``full``: the restatement's result at max_hops = N, computed once by the caller; what it gives at a smaller max_hops
    follows from it (a longer route keeps its best and gets the negative length; test_replan_host checks the restatement's own
    overflow branch)."""
    if full is None:
        want_best, want_rt, want_ln = R.routes(edges, N, tau, env, ag, bs, fb, max_hops)
    else:
        want_best, want_rt = full[0], full[1][..., :max_hops]
        want_ln = np.where(full[2] > max_hops, -full[2], full[2])
    best, rt, ln = _run_routes(plan, tau, env, ag, bs, fb, max_hops)
    assert _same_bits(best, want_best), np.argwhere(best != want_best)[:5]
    assert np.array_equal(ln, want_ln), np.argwhere(ln != want_ln)[:5]
    live = np.arange(max_hops)[None, None, :] < np.maximum(ln, 0)[..., None]
    assert np.array_equal(rt[live], want_rt[live])
    return best, rt, ln


def _graph(name):
    if name == "torus":
        net = _torus8()
    else:
        net = ig.graph(name)
    return net.num_roads, net.edge_index.numpy()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("name,kind", [("torus", "uniform"), ("MIXED", "random"), ("HUB126", "random"), ("HUB126", "uniform")])
def test_routes_equal_the_restatement(name, kind, H, K):
    """== on best, route_len and routes[:len], at max_hops = the longest route and one below it (that route then has a negative
    length and nothing outside its row is written); best == ops.td_hindsight wherever DONE == 1; the dummy row and the two
    agents with an id out of range have length 0 and best +inf; a second run gives the same bits."""
    from tarl_hip import ops
    N, edges = _graph(name)
    bs, fb, A = 40, 11, 40
    tau, env = _tables(kind, K, H, N, bs, fb, 300 + N + H)
    ag = G.random_agents(K, A, N, H, bs, fb, 300 + N)
    plan = ops.Plan(torch.from_numpy(edges), N)
    full = R.routes(edges, N, tau, env, ag, bs, fb, N)
    ln_all = full[2]
    longest = int(ln_all.max())
    assert longest >= 3 and (name == "torus" or (ln_all[:, 1:] == 0).any())          # dead ends: agents without a route
    best, rt, ln = _assert_routes(plan, edges, N, tau, env, ag, bs, fb, longest, full)
    assert (ln >= 0).all() and int(ln.max()) == longest
    assert (ln[:, 0] == 0).all() and np.isinf(best[:, 0]).all() and (ln[:, 2:4] == 0).all() and np.isinf(best[:, 2:4]).all()
    hs = ops.td_hindsight(plan, _cuda(tau), _cuda(env), _cuda(ag), bin_seconds=bs, first_bin=fb).cpu().numpy()
    done = ag[:, :, G.DONE] == 1.0
    done[:, 0] = False
    assert _same_bits(best[done], hs[done]) and done.any() and (~done[:, 1:]).any()
    b2, r2, l2 = _run_routes(plan, tau, env, ag, bs, fb, longest)
    assert _same_bits(b2, best) and np.array_equal(l2, ln) and np.array_equal(r2, rt)
    if longest >= 2:
        sbest, _, sln = _assert_routes(plan, edges, N, tau, env, ag, bs, fb, longest - 1, full)
        assert (sln[ln_all == longest] == -longest).all() and _same_bits(sbest, best)
    if kind == "uniform" and name == "torus":
        # the ties are live: some road on some route has two tight in-edges, and the smaller id was taken
        ins, outs = R.in_lists(edges, N), G.out_lists(edges, N)
        ties = 0
        for a in range(4, A):
            if ln[0, a] >= 2:
                o, t0 = int(ag[0, a, 0]), float(ag[0, a, 2])
                L = R.labels(outs, tau[0], env[0], o, t0, bs, fb)
                for u, v in zip(rt[0, a, :ln[0, a] - 1], rt[0, a, 1:ln[0, a]]):
                    tight = [s for s in ins[v] if G.leave(tau[0], env[0], v, L[s], bs, fb) == L[v]]
                    ties += len(tight) >= 2
                    assert u == min(tight)
        assert ties > 0


def test_waiting_for_the_faster_bin_wins_on_the_torus():
    """H = 4, bin 1 slow and bin 2 fast: some route's arrival is the envelope's (left at the bin edge), found from the tables."""
    N, edges = _graph("torus")
    bs, fb = 40, 11
    tau, env = _tables("uniform", 1, 4, N, bs, fb, 5)
    ag = G.random_agents(1, 40, N, 4, bs, fb, 300 + N)
    flags = set()
    _, rt, ln = R.routes(edges, N, tau, env, ag, bs, fb, N)
    for a in range(4, 40):
        t = float(ag[0, a, 2])
        for n in rt[0, a, :max(int(ln[0, a]), 0)]:
            t = G.leave(tau[0], env[0], int(n), t, bs, fb, flags=flags)
    assert "envelope" in flags


def test_more_searches_than_workgroups():
    """K A = 3 x 400 = 1 200 searches on the 21-road graph of test_gpu_dynamic_gap: the grid stride runs and every workgroup
    reuses its label row — and walks it again."""
    import occupancy_restatement as O
    from tarl_hip import ops
    net = O.small_graph()
    N, K, A, H, bs = net.num_roads, 3, 400, 5, 60
    edges = net.edge_index.numpy()
    tau, env = _tables("random", K, H, N, bs, 11, 77)
    ag = G.random_agents(K, A, N, H, bs, 11, 77)
    _, _, ln = _assert_routes(ops.Plan(torch.from_numpy(edges), N), edges, N, tau, env, ag, bs, 11, N)
    assert int((ln > 0).sum()) > 600


def test_refused_calls_write_nothing():
    from tarl_hip import lib, ops
    N, edges = _graph("torus")
    plan = ops.Plan(torch.from_numpy(edges), N)
    tau, env = _tables("uniform", 1, 1, N, 40, 11, 1)
    ag = _cuda(G.random_agents(1, 8, N, 1, 40, 11, 1))
    out = (torch.full((1, 8), -77.0, dtype=torch.float64, device="cuda"), torch.full((1, 8, 4), -77, dtype=torch.int32, device="cuda"),
           torch.full((1, 8), -77, dtype=torch.int32, device="cuda"))
    with pytest.raises(lib.TarlError, match="scratch"):
        ops.td_routes(plan, _cuda(tau), _cuda(env), ag, bin_seconds=40, first_bin=11, max_hops=4, out=out,
                      scratch=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.td_routes(plan, _cuda(tau), _cuda(env), ag, bin_seconds=40, first_bin=11, max_hops=5, out=out)
    torch.cuda.synchronize()
    assert all(bool((t == -77).all()) for t in out)


# ---- 2. the select kernel ----------------------------------------------------------------------------------------------------------
def _select_case(name):
    from test_gpu_router_hold import _case
    return _case(name)


def _population(c, name):
    import baseline_restatement as BR
    from tarl_hip.engine import EPISODE_START
    from test_gpu_eval_baseline import IRREGULAR_LOAD as LOAD
    if name == "torus":
        from test_gpu_router_hold import _few_population
        return _few_population(c.net), 40
    _, dout = ig.degrees(c.net)
    leads_on = torch.nonzero(dout > 0).view(-1)
    pop = BR.few_destination_population(LOAD["agents"], c.N, LOAD["dests"], seed=7, t0=EPISODE_START, t1=EPISODE_START + LOAD["span"])
    pop[:, 0] = leads_on[pop[:, 0].long() % leads_on.numel()].float()
    return pop, LOAD["frames"]


def _crafted_plans(c, x, A, L, per_env, seed):
    """Plans made from the exported state ``x`` (B, N, F), whatever the quickest routes would be: for every row with a head the
    head agent's plan is drawn from six kinds — through the row (a random walk that passes it), ending on it (the destination
    row), one short of its end (the holding row), elsewhere (off its route), none (length 0), overflowing (negative length).
    A shared plan takes the kinds from environment 0's rows; the same agent then stands on other rows elsewhere. Agent 0, whom
    every clean empty row reads, has no route in the shared plan and in environment 0, and a long walk from the second
    environment on. -> (routes int32 (P, A, L), route_len (P, A), kinds {(p, agent): kind})."""
    rng = np.random.default_rng(seed)
    B, N = x.shape[0], c.N
    outl = ig.out_lists(c.net)
    ins = R.in_lists(c.ei.numpy(), N)
    P = B if per_env else 1
    rt = rng.integers(-5, N + 5, size=(P, A, L)).astype(np.int32)          # garbage beyond the lengths
    ln = np.zeros((P, A), np.int32)
    kinds = {}

    def forward(start, steps):
        path = [start]
        for _ in range(steps):
            if not outl[path[-1]]:
                break
            path.append(int(rng.choice(outl[path[-1]])))
        return path

    for p in range(P):
        heads = x[p, :, 0].numpy().astype(np.int64)
        counts = x[p, :, 3 * c.Nmax + 1].numpy()
        for i in np.nonzero((counts > 0) | (heads != 0))[0]:      # (an empty row with a head: DIRTY, a stale slot)
            h = int(heads[i])
            if not 1 <= h < A or (p, h) in kinds:
                continue
            kind = ("through", "destination", "holding", "elsewhere", "none", "overflow")[int(rng.integers(0, 6))]
            back = [int(rng.choice(ins[i]))] if ins[i] and rng.random() < 0.5 else []
            if kind == "through":
                path = back + forward(int(i), 3)
            elif kind == "destination":
                path = back + [int(i)]
            elif kind == "holding":
                path = back + forward(int(i), 1)
            elif kind == "elsewhere":
                path = [v for v in forward(int(rng.integers(0, N)), 3) if v != i] or [int((i + 1) % N)]
            else:
                path = forward(int(i), 2)
            path = path[:L]
            rt[p, h, :len(path)] = path
            ln[p, h] = {"none": 0, "overflow": -len(path)}.get(kind, len(path))
            kinds[(p, h)] = kind
        if per_env and p >= 1:
            walk = forward(int(rng.integers(0, N)), L - 1)
            rt[p, 0, :len(walk)], ln[p, 0] = walk, len(walk)
    return rt, ln, kinds


def _expected_select(c, x_b, rt_p, ln_p):
    """One environment -> (sel8, sel) as the kernel must leave them from (SEL_RAW, SENTINEL) everywhere, and the written rows."""
    written, value = R.select_rule(x_b.numpy(), rt_p, ln_p)
    written, value = torch.from_numpy(written), torch.from_numpy(value).float()
    hit = S.out_table(c).float() == value.unsqueeze(1)
    code = torch.where(hit.any(1), torch.argmax(hit.to(torch.int8), dim=1), torch.full((c.N,), SEL_RAW))
    sel8 = torch.where(written, code, torch.full((c.N,), SEL_RAW)).to(torch.uint8)
    sel = torch.where(written & (code == SEL_RAW), value, torch.full((c.N,), SENTINEL))
    return sel8, sel, written


@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("name", ["torus", "MIXED"])
def test_select_route_equals_the_rule_on_the_exported_state(name, B):
    """After the reset (every row empty and clean: agent 0 is read) and after the hold router has run the engine into a live
    state (empty rows, DIRTY rows, ranks above 3 on MIXED): sel8 / sel / choice8 == the rule on the exported x for a shared
    plan and for one plan per environment; sentinel-filled outputs untouched on the rows the kernel must leave alone; the
    kinds of :func:`_crafted_plans` all occur."""
    from tarl_hip import ops
    from tarl_hip.evaluator import VecEvaluator
    from test_gpu_router_hold import _engine
    c = _select_case(name)
    pop, frames = _population(c, name)
    eng = _engine(c.net, pop, B)
    A, L, plan, fs = eng.A, 6, eng.plan, eng.fs
    seen, wrote_raw, high_rank, dirty_rows = set(), 0, 0, 0
    for live in (False, True):
        if live:
            VecEvaluator(eng, "dijkstra_hold").run(frames)
            # a run from the reset seldom leaves a DIRTY row: three empty rows per environment get a stale slot 0 (an old
            # agent id with its clocks, as test_gpu_router_hold crafts it) and the state is packed again
            xd = eng.x
            empty = xd[:, :, 3 * c.Nmax + 1] == 0
            for b in range(B):
                for q, r in enumerate(torch.nonzero(empty[b]).view(-1)[:3].tolist()):
                    xd[b, r, 0], xd[b, r, c.Nmax], xd[b, r, 2 * c.Nmax] = float(20 + q), 150.0, 160.0
            eng._packed_stale = True
            eng.resync()
            eng._x_stale = True                 # what the kernel sees: the export of the packed state
        else:
            eng.reset()
        x = eng.x.cpu()
        dirty = ((fs.hdp[..., 0] & 0xFF) == 0x80).t().cpu()
        dirty_rows += int(dirty.sum())
        assert not live or int((x[:, :, 0][dirty] >= 20.0).sum()) == 3 * B      # the crafted rows, exported with their stale ids
        for per_env in (False, True):
            rt, ln, kinds = _crafted_plans(c, x, A, L, per_env, 40 + B + live)
            seen |= set(kinds.values()) if live else set()
            fs.sel8.fill_(SEL_RAW)
            fs.sel.fill_(SENTINEL)
            c8 = torch.full((B, c.N), 0x55, dtype=torch.uint8, device="cuda")
            rt_d, ln_d = _cuda(rt if per_env else rt[0]), _cuda(ln if per_env else ln[0])
            assert ops.fused_select_route(plan, fs, rt_d, ln_d, choice8=c8) is c8
            fs.check_flags()
            sel8, sel, c8 = fs.sel8.t().cpu(), fs.sel.t().cpu(), c8.cpu()
            any_written = 0
            for b in range(B):
                p = b if per_env else 0
                w8, wsel, written = _expected_select(c, x[b], rt[p], ln[p])
                assert torch.equal(sel8[b], w8), f"sel8, environment {b}, live={live}, per_env={per_env}"
                assert torch.equal(sel[b], wsel), f"sel, environment {b}, live={live}, per_env={per_env}"
                any_written += int(written.sum())
                wrote_raw += int((written & (w8 == SEL_RAW)).sum())
                high_rank += int(((w8 >= 4) & (w8 < SEL_RAW)).sum())
            assert torch.equal(c8, sel8)
            assert any_written > 0 or not live and (not per_env or B == 1)
    assert seen == {"through", "destination", "holding", "elsewhere", "none", "overflow"}
    assert wrote_raw > 0 and dirty_rows > 0 and (name == "torus" or high_rank > 0)


# ---- 3. the episode ----------------------------------------------------------------------------------------------------------------
def test_the_replanner_equals_the_restated_day_loop():
    """8 x 8 torus, 128 agents, 60 frames, K = 2, three days, fraction 0.5, bins of 20 s, max_hops 16: the plan of every day, the
    switch masks, the agent tables and the returns == the restatement's loop on oracle.sim.env_step under the exported Gumbel
    values (the same on every day); the relative gap within 1e-12."""
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.replanning import Replanner
    from test_gpu_router_hold import _engine
    net = _torus8()
    K, T, days = 2, 60, 3
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    eng = _engine(net, pop, K)
    noise0 = eng.noise_counter + 1
    rp = Replanner(eng, days=days, fraction=0.5, max_hops=16, link_bin_seconds=20, seed=0, keep=True)
    res = rp.run(T)
    assert res.domain_exit_day is None and len(res.days) == days and res.last.head == "routes" and res.last.frames_run == T
    assert res.last.settings["max_hops"] == 16 and res.last.settings["agents_without_route"] == 0
    noise = {}

    def gumbel_of(b, t):
        if (b, t) not in noise:
            noise[(b, t)] = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
        return noise[(b, t)]

    want = R.day_loop(net, pop, K, T, days, 0.5, 16, 20, 0, gumbel_of, EPISODE_START)
    for day, (w, h, rec) in enumerate(zip(want, rp.history, res.days)):
        ln = h["route_len"].cpu().numpy()
        assert np.array_equal(ln, w["route_len"]), f"route_len, day {day}"
        live = np.arange(16)[None, None, :] < np.maximum(ln, 0)[..., None]
        assert np.array_equal(h["routes"].cpu().numpy()[live], w["routes"][live]), f"routes, day {day}"
        assert (w["mask"] is None) == (h["mask"] is None) == (day == days - 1)
        if w["mask"] is not None:
            assert np.array_equal(h["mask"].cpu().numpy(), w["mask"]), f"switch mask, day {day}"
        assert np.array_equal(h["agents"].cpu().numpy(), w["agents"]), f"agent tables, day {day}"
        assert rec["per_env"]["episode_return"] == w["returns"] and rec["per_env"]["arrived"] == w["arrived"], f"day {day}"
        assert rec["differs"] == int(w["differs"][:, 1:].sum())
        assert rec["switched"] == (None if w["mask"] is None else int((w["mask"] & w["differs"])[:, 1:].sum()))
        for got, rg in zip(rec["per_env"]["relative_gap"], w["rg"]):
            assert (got is None) == (rg is None) and (got is None or abs(got - rg) <= 1e-12), (day, got, rg)
        print(f"[replan] day {day}: arrivals {w['arrived']}, travel time {w['travel_time']}, RG {w['rg']}, differs {rec['differs']}, "
              f"switched {rec['switched']}")
    assert min(want[-1]["arrived"]) > 0 and res.days[0]["differs"] > 0 and res.days[0]["switched"] > 0
    assert torch.equal(res.routes, rp.history[-1]["routes"]) and torch.equal(res.route_len, rp.history[-1]["route_len"])


def test_the_shared_plan_the_reports_and_the_fallback():
    """per_env=False: one plan (1, A, L) planned on the sum over the environments, followed by both. Every report flag runs
    with the head and perturbs nothing. Without the fallback the select kernel alone strands the population on the torus (the
    origin rows are empty: the dummy agent has no route, the stale byte decides) — the finding the fallback answers."""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import VecEvaluator
    from tarl_hip.replanning import Replanner, replan_lines, replan_report
    from test_gpu_router_hold import _engine
    net = _torus8()
    pop = synth.population(128, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + 40)
    kw = dict(days=2, fraction="msa", max_hops=16, link_bin_seconds=60)
    shared = Replanner(_engine(net, pop, 2), per_env=False, **kw).run(120)
    assert shared.routes.shape == (1, 129, 16) and shared.last.settings["routes_per_env"] is False
    assert shared.days[0]["switch_probability"] == 0.5 and shared.days[0]["agents"] == 128
    plain = Replanner(_engine(net, pop, 2), **kw).run(120)
    full = Replanner(_engine(net, pop, 2), link_counts=True, trips=True, turns=True, **kw).run(120)
    assert full.last.episode_return == plain.last.episode_return and full.last.arrived == plain.last.arrived
    assert torch.equal(full.routes, plain.routes) and full.last.link_counts is not None and full.last.turn_counts is not None
    assert full.last.occupancy is not None and full.last.dynamic_gap is not None and int(full.last.trips["n_done"].sum()) > 0
    rep = replan_report(plain)
    assert len(rep["rows"]) == 2 and rep["rows"][1]["switched_share"] is None and len(replan_lines(rep)) == 5
    assert min(plain.last.arrived) > 0
    ev = VecEvaluator(_engine(net, pop, 2), "routes", routes=(plain.routes, plain.route_len), route_fallback=False)
    bare = ev.run(120)
    assert bare.settings["route_fallback"] is False and max(bare.arrived) < min(plain.last.arrived)
    with pytest.raises(ValueError, match="sampled"):
        ev.run(8, deterministic=False)
    r2 = Replanner(_engine(net, pop, 2), **kw).run(120)
    assert r2.last == plain.last and torch.equal(r2.routes, plain.routes)          # two runs are bit-identical


# ---- 4. CLI end to end ---------------------------------------------------------------------------------------------------------------
def test_cli_replanning_end_to_end(tmp_path, capsys):
    """--replan-days 2 --replan-envs 2 writes its files next to the evaluation's; the same run without the flags writes none of
    them, and the evaluation's own tables are byte-identical between the two runs."""
    main = importlib.import_module("main").main
    common = ["--algo", "mpnn", "--mode", "eval", "--scenario", "synthetic-1024-300", "--steps", "120", "--eval-envs", "2",
              "--eval-trips"]
    with_, without = tmp_path / "with", tmp_path / "without"
    main(common + ["--replan-days", "2", "--replan-envs", "2", "--output-dir", str(with_)])
    text = capsys.readouterr().out
    assert "=== Replanning (2 days, 2 environments) ===" in text and "routes, last day) ===" in text
    assert "=== Policy \u2212 replanned (paired) ===" in text
    for f in ("replan_days.csv", "replan_envs.json", "replan_envs.csv", "replan_trips.csv"):
        assert (with_ / f).exists(), f
    doc = json.load(open(with_ / "replan_envs.json"))
    assert doc["routes"]["head"] == "routes" and len(doc["days"]) == 2 and doc["settings"]["days"] == 2
    assert doc["paired"]["b"] == "routes" and doc["settings"]["shared_noise"] is True
    assert len(open(with_ / "replan_days.csv").read().splitlines()) == 3
    main(common + ["--output-dir", str(without)])
    assert "Replanning" not in capsys.readouterr().out
    names = {p.name for p in without.iterdir()}
    assert not any(n.startswith("replan") for n in names)
    assert names == {p.name for p in with_.iterdir() if not p.name.startswith("replan")}
    same = [f for f in ("eval_envs.csv", "eval_trips.csv", "eval_trips_by_departure.csv", "msa_expected_flows.csv") if f in names]
    assert "eval_envs.csv" in same and "eval_trips.csv" in same
    for f in same:
        assert (with_ / f).read_bytes() == (without / f).read_bytes(), f


@pytest.mark.parametrize("algo", ["dijkstra", "random"])
def test_cli_replanning_with_the_classical_agents(tmp_path, capsys, algo):
    """--replan-days goes with any --algo: the loop needs the network and the population, not a policy; no paired block."""
    main = importlib.import_module("main").main
    out = tmp_path / algo
    main(["--algo", algo, "--mode", "eval", "--scenario", "synthetic-1024-300", "--steps", "60", "--replan-days", "2",
          "--replan-fraction", "msa", "--replan-max-hops", "64", "--output-dir", str(out)])
    text = capsys.readouterr().out
    assert "=== Replanning (2 days, 1 environments) ===" in text and "(paired)" not in text
    doc = json.load(open(out / "replan_envs.json"))
    assert doc["settings"]["fraction"] == "msa" and doc["settings"]["max_hops"] == 64 and doc["settings"]["envs"] == 1
    assert doc["days"][0]["switch_probability"] == 0.5 and doc["routes"]["settings"]["max_hops"] == 64
    assert (out / "replan_days.csv").exists() and (out / "replan_envs.csv").exists()
