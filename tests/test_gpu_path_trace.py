"""GPU: the per-agent path trace — tarl_path_trace_reset and tarl_fused_path_trace against
``path_trace_restatement`` on the packed words of live frames (the 8 x 8 torus and both irregular graphs, the sampled embedding
head, which wanders), tarl_path_agent_stats against a numpy restatement that sums in the same order, the evaluator on the
free-flow hold router (the test that fails without the feature: every delivered trip follows its tree, excess exactly 0), the
cross-check against the turn counts, the command line end to end and the refusals. Every comparison is ``==``, fp64 included."""
import numpy as np
import pytest
import torch

import path_trace_restatement as P
import sp_cases as S

pytestmark = pytest.mark.gpu

GRAPHS = ["torus", "MIXED", "HUB126"]
CHECKPOINTS = (1, 20, 60)
FILL = 0x7F
STATE = ("hdp", "tl", "gc8", "post", "slots", "sel8", "sel", "a_origin", "a_dest", "a_dep", "a_status", "a_order", "a_dep_sorted",
         "cur_lo", "a_win", "a_ins", "a_rank", "acc_lp", "acc_n", "acc_w", "flags", "st0", "node_rec", "in_rec", "out_pad")
NAMES = ("last_road", "roads", "revisits", "off_tree", "path_cost", "excess", "route", "bad")


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _net(name):
    from tarl_hip import synth
    return synth.torus_network(8, 8) if name == "torus" else S.case(name).net


def _population(net, agents, t1=4):
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    return synth.population(agents, net.num_roads, seed=7, t0=EPISODE_START, t1=EPISODE_START + t1)


def _engine(net, pop, K, seed=3):
    from tarl_hip.engine import SimEngine
    return SimEngine(net.x.cuda(), net.edge_index, net.edge_attr, net.Nmax, pop.cuda(),
                     congestion_constant=net.congestion_constant, num_envs=K, seed=seed)


def _emb(net):
    return torch.randn(net.num_roads, generator=torch.Generator().manual_seed(11)).cuda()


_LIVE = {}


def _live(name, B, A, frames=60):
    """``frames`` live frames of the sampled embedding head on B environments of A - 1 agents that all depart within 4 s
    -> (net, engine, the packed hdp words after every frame). Computed once per shape and left unchanged."""
    key = (name, B, A)
    if key not in _LIVE:
        net = _net(name)
        eng = _engine(net, _population(net, A - 1), B)
        eng.reset()
        eng.prepare_policy(_emb(net), 1.0)
        reward = torch.zeros(B, device="cuda")
        snaps = []
        for _ in range(frames):
            eng.frame_fused(reward=reward)
            snaps.append(eng.fs.hdp.clone())
        eng.fs.check_flags()
        _LIVE.clear()       # one shape's engine at a time
        _LIVE[key] = (net, eng, snaps)
    return _LIVE[key]


def _tables(net, eng, drop_every=5):
    """Random positive weights, the distances to every destination of the agent tables but every fifth (no slot: off-tree)."""
    from tarl_hip import ops
    N, E = net.num_roads, net.edge_index.size(1)
    w = (torch.rand(E, generator=torch.Generator().manual_seed(5)) * 9 + 1).to(torch.float32).cuda()
    d = torch.unique(eng.agents[..., 1].reshape(-1).to(torch.int64))
    d = d[(d >= 0) & (d < N)]
    keep = torch.ones(d.numel(), dtype=torch.bool, device=d.device)
    keep[::drop_every] = d.numel() < 2
    d = d[keep].contiguous()
    slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    slot[d] = torch.arange(d.numel(), dtype=torch.int32, device="cuda")
    _, dist = ops.destination_trees(eng.plan, w, d, want_next_hop=False, want_dist=True)
    return w, dist, slot


def _guarded_state(ops, B, A, L):
    """A PathTraceState whose tensors lie in the middle of 0x7F-filled buffers -> (state, check): ``check()`` asserts that
    the bands on both sides of every array still hold the fill."""
    st = ops.path_trace_state(B, A, L, "cuda")
    bufs = []
    for name, t in st.tensors().items():
        nbytes = t.numel() * t.element_size()
        buf = torch.full((nbytes + 512,), FILL, dtype=torch.uint8, device="cuda")
        setattr(st, name, buf[256:256 + nbytes].view(t.dtype).view(t.shape))
        bufs.append((name, buf, nbytes))

    def check():
        for name, buf, nbytes in bufs:
            assert bool((buf[:256] == FILL).all()) and bool((buf[256 + nbytes:] == FILL).all()), f"guard band of {name}"
    return st, check


def _host(st):
    return {k: v.cpu().numpy() for k, v in st.tensors().items()}


def _equal(got, want, where):
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k)


# ---- 1. the sighting pass on live frames -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("name", GRAPHS)
def test_trace_of_live_frames(name, B):
    """After 1, 20 and 60 live frames, A in {2, 129}, L in {0, 1, 3, 64}, with and without weights: every state array equals
    the restatement, from 0x7F-filled arrays between guard bands after the reset; a second launch on the same packed state
    changes nothing; the packed state and its export stay as they were."""
    from tarl_hip import ops
    for A in (2, 129):
        net, eng, snaps = _live(name, B, A)
        plan, fs, N = eng.plan, eng.fs, net.num_roads
        graph = P.csr(net.edge_index.numpy(), N)
        tables = _tables(net, eng)
        host_tables = dict(a_dest=fs.a_dest.cpu().numpy(), weights=tables[0].cpu().numpy(), dist=tables[1].cpu().numpy(),
                           dest_slot=tables[2].cpu().numpy())
        words = [s[..., 0].cpu().numpy() for s in snaps]
        final = snaps[-1].clone()
        for L in (0, 1, 3, 64):
            for with_w in (False, True):
                st, bands = _guarded_state(ops, B, A, L)
                ops.path_trace_reset(st)
                want = P.new_state(B, A, L)
                _equal(_host(st), P.arrays(want), (A, L, with_w, "reset"))
                dev_kw = dict(zip(("weights", "dist", "dest_slot"), tables)) if with_w else {}
                for f, snap in enumerate(snaps):
                    fs.hdp.copy_(snap)
                    ops.fused_path_trace(plan, fs, st, **dev_kw)
                    P.sighting_pass(want, words[f], graph, **(host_tables if with_w else {}))
                    if f + 1 in CHECKPOINTS:
                        got = _host(st)
                        _equal(got, P.arrays(want), (A, L, with_w, f + 1))
                        ops.fused_path_trace(plan, fs, st, **dev_kw)      # the same packed state again: nothing new
                        _equal(_host(st), got, (A, L, with_w, f + 1, "second launch"))
                bands()
                w = P.arrays(want)
                assert w["bad"].sum() == 0 and (A == 2 or (w["roads"][:, 1:] > 0).any())
                if A == 129 and L == 3:
                    assert (w["roads"] > L).any(), "the wandering head truncates a trace of three roads"
                if A == 129:
                    print(f"[path trace] {name} B={B} L={L}: truncated {int((w['roads'] > L).sum())}, with a loop "
                          f"{int((w['revisits'] > 0).sum())} of {B * 128} traces")
                if A == 129 and L == 64:
                    assert (w["revisits"] > 0).any(), "the wandering head loops"
                if A == 129 and with_w:
                    assert (w["path_cost"] > 0).any() and (w["excess"] > 0).any() and (w["off_tree"] > 0).any()
                if not with_w:
                    assert not w["path_cost"].any() and not w["excess"].any() and not w["off_tree"].any()
        # the packed state and its export are not written
        fs.hdp.copy_(final)
        x_before, x_after = eng._x.clone(), eng._x.clone()
        ops.fused_export(plan, fs, x_before, net.Nmax, float(eng.time))      # (the export refreshes words of its own: first)
        before = {k: getattr(fs, k).clone() for k in STATE}
        st = ops.path_trace_state(B, A, 3, "cuda")
        ops.path_trace_reset(st)
        ops.fused_path_trace(plan, fs, st, *tables)
        changed = [k for k in STATE if not torch.equal(before[k], getattr(fs, k))]
        assert not changed, changed
        ops.fused_export(plan, fs, x_after, net.Nmax, float(eng.time))
        assert torch.equal(x_before.view(torch.int32), x_after.view(torch.int32))      # bit for bit


# ---- 2. the per-agent reduction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 65])
def test_agent_stats_equal_the_restatement(K):
    """Random state arrays and DONE flags, A = 129 (three workgroups' worth of lanes, the last partial), with and without the
    second run: every count and every fp64 sum equals the numpy restatement that adds the environments in the same order."""
    from tarl_hip import ops
    A, L = 129, 3
    g = torch.Generator().manual_seed(K)

    def run():
        st = ops.path_trace_state(K, A, L, "cuda")
        ops.path_trace_reset(st)
        st.roads.copy_(torch.randint(0, 9, (K, A), generator=g).to(torch.int32))
        st.revisits.copy_(torch.randint(0, 3, (K, A), generator=g).to(torch.int32))
        st.off_tree.copy_(torch.randint(0, 2, (K, A), generator=g).to(torch.int32))
        st.path_cost.copy_(torch.rand((K, A), generator=g, dtype=torch.float64) * 1e3)
        ex = torch.rand((K, A), generator=g, dtype=torch.float64) * 7
        st.excess.copy_(torch.where(torch.rand((K, A), generator=g) < 0.3, torch.zeros_like(ex), ex))
        ag = torch.zeros((K, A, 9))
        ag[:, :, 8] = (torch.rand((K, A), generator=g) < 0.6).float()
        return st, ag.cuda()

    (sa, aa), (sb, ab) = run(), run()
    ha, hb = _host(sa), _host(sb)
    da, db = aa[:, :, 8].cpu().numpy() == 1, ab[:, :, 8].cpu().numpy() == 1
    for pair in (False, True):
        got = ops.path_agent_stats(sa, aa, *((sb, ab) if pair else ()))
        want = P.agent_stats(ha, da, L, *((hb, db) if pair else ()))
        assert set(got) == set(want)
        for k, v in want.items():
            assert np.array_equal(got[k].cpu().numpy(), v), (pair, k)
        assert int(got["n_done"][1:].sum()) > 0 and got["n_done"][0] == 0
    with pytest.raises(ValueError, match="come together"):
        ops.path_agent_stats(sa, aa, state_b=sb)


# ---- 3. the evaluator: the test that fails without the feature -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def torus_runs():
    """The torus "spread" case (128 agents, K = 3, 300 frames): the free-flow hold router with the first-hop rule, traced
    under the travel times its table was built from, with the turn counts beside it; and the sampled embedding head."""
    from tarl_hip import ops
    from tarl_hip.evaluator import VecEvaluator
    net = _net("torus")
    pop = _population(net, 128, t1=40)
    eng = _engine(net, pop, 3)
    eng.reset()
    if eng._packed_stale:
        eng.resync()
    w = ops.fused_edge_travel_time(eng.plan, eng.fs)[0].clone()      # what the router reads at frame 0: the empty network
    router = VecEvaluator(eng, "dijkstra_hold", refresh_rate=0, paths=True, route_departures=True, path_weights=w, turns=True)
    r = router.run(300)
    assert torch.equal(router.weights[0], w)
    wander = VecEvaluator(_engine(net, pop, 3), "embedding", emb=_emb(net), paths=True, path_weights=w)
    return net, r, wander.run(300, deterministic=False)


def test_the_free_flow_router_follows_its_tree(torus_runs):
    net, r, s = torus_runs
    p, done = r.paths, r.paths["done"].copy()
    done[:, 0] = False
    assert done.sum() > 0.9 * 3 * 128 and r.path_meta["weights"] and r.path_meta["note"] is None
    assert (p["excess"][done] == 0.0).all() and (p["off_tree"][done] == 0).all()
    assert (p["path_cost"][:, 1:] > 0).any() and (p["roads"][done] >= 1).all()
    edges = set(map(tuple, net.edge_index.t().tolist()))
    routes, length = r.path_routes
    assert np.array_equal(length, np.minimum(p["roads"], 64))
    dest = r.path_meta["destination"]
    for k in range(3):
        for a in range(1, 129):
            way = routes[k, a, :length[k, a]].tolist()
            assert all(e in edges for e in zip(way, way[1:])), (k, a, way)
            if done[k, a]:
                assert way[-1] == dest[a] or (way[-1], int(dest[a])) in edges, (k, a, way)
    st = r.path_stats
    assert np.array_equal(st["n_done"][1:], done[:, 1:].sum(axis=0)) and np.array_equal(st["n_zero_excess"], st["n_done"])
    assert not st["excess_sum"].any()      # (run() raises where `bad` is not all zero: a result means it was)
    # the wandering head pays for its detours, in every environment
    assert (s.paths["excess"].sum(axis=1) > p["excess"].sum(axis=1)).all() and (s.paths["excess"].sum(axis=1) > 0).all()


def test_moves_are_bounded_by_the_turn_counts(torus_runs):
    """An independent kernel: every hop the trace saw crossed a route edge the turn counts counted; movements into a queue
    whose agent never reached its head, and Q24 losses, account for the difference."""
    _, r, _ = torus_runs
    moves = np.maximum(r.paths["roads"][:, 1:] - 1, 0).sum(axis=1)
    turns = r.turn_counts.sum(axis=(1, 2))
    assert (moves <= turns).all() and (moves > 0).all()


def test_report_of_the_runs(torus_runs):
    from tarl_hip.evaluator import path_lines, path_report, path_summary
    _, r, s = torus_runs
    rep, rep_s = path_report(r), path_report(s)
    assert rep["available"] and len(rep["rows"]) == 128 and rep["summary"]["trips"] == int(r.path_stats["n_done"].sum())
    assert rep["summary"]["weights"]["mean_excess"] == 0.0 and rep["summary"]["weights"]["share_zero_excess"] == 1.0
    assert rep_s["available"] and rep_s["summary"]["open"]["traces"] > 0
    text = "\n".join(path_lines(rep))
    assert "definition:" in text and "mean excess:" in text and "By departure time" in text
    import json
    json.dumps(path_summary(rep))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from tarl_hip import lib, ops
    from tarl_hip.evaluator import VecEvaluator
    net = _net("torus")
    eng = _engine(net, _population(net, 8), 2)
    for kw, msg in ((dict(path_max_hops=8), "need paths=True"), (dict(path_weights=torch.ones(4)), "need paths=True"),
                    (dict(paths=True, path_max_hops=4097), "path_max_hops must be"),
                    (dict(paths=True, path_weights=torch.ones(4)), "one weight per edge")):
        with pytest.raises(ValueError, match=msg):
            VecEvaluator(eng, "dijkstra_hold", refresh_rate=0, **kw)
    with pytest.raises(ValueError, match="needs paths=True"):
        VecEvaluator(eng, "dijkstra_hold", refresh_rate=0).run(2, path_pair=(None, eng.agents))
    st = ops.path_trace_state(3, 9, 2, "cuda")
    with pytest.raises(ValueError, match="state is for"):
        ops.fused_path_trace(eng.plan, eng.fs, st)
    st = ops.path_trace_state(2, 9, 2, "cuda")
    with pytest.raises(ValueError, match="come together"):
        ops.fused_path_trace(eng.plan, eng.fs, st, weights=torch.ones(net.edge_index.size(1), device="cuda"))
    with pytest.raises(TypeError):
        ops.fused_path_trace(eng.plan, eng.fs, st, weights=torch.ones(net.edge_index.size(1), device="cuda"),
                             dist=torch.zeros((1, net.num_roads), device="cuda"),
                             dest_slot=torch.zeros(net.num_roads, dtype=torch.int32, device="cuda"))
    st.roads = st.roads.to(torch.int64)
    with pytest.raises(TypeError):
        ops.path_trace_reset(st)
    assert isinstance(lib.TarlError("x"), RuntimeError)


def test_memory_limits(monkeypatch):
    """A route array beyond half the free device memory is refused with its size; a distance table beyond half of what is
    left beside the state is dropped, the weights with it, and the run reports roads and loops only."""
    from tarl_hip import lib
    from tarl_hip.evaluator import VecEvaluator, path_lines, path_report
    net = _net("torus")
    eng = _engine(net, _population(net, 8), 2)
    ff = net.x[:, 3 * net.Nmax + 2][net.edge_index[1]].contiguous()
    total = torch.cuda.mem_get_info()[1]
    need = 4 * 2 * 9 * 64      # K x A x L int32
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (2 * need - 2, total))
    with pytest.raises(lib.TarlError, match=r"route array \(0\.00 GiB for K = 2 environments x A = 9 agents x path_max_hops = 64\)"):
        VecEvaluator(eng, "embedding", emb=_emb(net), paths=True, path_weights=ff)
    answers = iter([(total, total), (1024, total)])      # room for the routes, then none for 8 x D x 256 bytes of distances
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: next(answers))
    ev = VecEvaluator(eng, "embedding", emb=_emb(net), paths=True, path_weights=ff)
    monkeypatch.undo()
    assert ev.path_w is None and ev.path_dist is None and ev.path_note.startswith("path cost and excess not available: the distance")
    res = ev.run(40, deterministic=False)
    assert res.path_meta["weights"] is False and not res.paths["path_cost"].any() and (res.paths["roads"] > 0).any()
    assert any("path cost and excess not available" in line for line in path_lines(path_report(res)))


# ---- 5. the command line, end to end -------------------------------------------------------------------------------------------------
SCENARIO = "synthetic-1024-300"


def _main(argv):
    import importlib
    importlib.import_module("main").main(argv)


def _files(d):
    return {p.name: p.read_bytes() for p in d.iterdir() if p.is_file()}


def test_cli_eval_envs_with_a_baseline(tmp_path, capsys):
    import json
    base = ["--algo", "mpnn", "--mode", "eval", "--scenario", SCENARIO, "--steps", "60", "--eval-envs", "2", "--eval-trips",
            "--eval-baseline", "free_flow"]
    _main(base + ["--output-dir", str(tmp_path / "off")])
    capsys.readouterr()
    _main(base + ["--eval-paths", "--eval-paths-max-hops", "8", "--eval-paths-routes", "1", "--output-dir", str(tmp_path / "on")])
    text = capsys.readouterr().out
    assert "=== Paths ===" in text and "=== Paths: baseline (dijkstra_hold) ===" in text and "definition:" in text
    off, on = _files(tmp_path / "off"), _files(tmp_path / "on")
    new = {"eval_paths.csv", "eval_paths_by_departure.csv", "eval_paths_baseline.csv", "eval_paths_routes.csv"}
    assert set(on) - set(off) == new
    doc_on, doc_off = json.loads(on["eval_envs.json"]), json.loads(off["eval_envs.json"])
    assert doc_on["paths"]["available"] and doc_on["paths"]["baseline"]["available"] and "paired" in doc_on["paths"]["summary"]
    for k in ("mode", "baseline"):      # the settings name the trace; nothing else of the old keys changes
        assert doc_on[k]["settings"].pop("paths") is True and doc_on[k]["settings"].pop("path_max_hops") == 8
        doc_on[k].pop("computation_time_ms"), doc_off[k].pop("computation_time_ms")
    doc_on.pop("paths")
    assert doc_on == doc_off
    # (computation_time.png plots wall-clock times: it differs between any two runs, with or without the flag)
    for name in set(off) - {"eval_envs.json", "computation_time.png"}:
        assert on[name] == off[name], name
    header = on["eval_paths.csv"].decode().splitlines()[0]
    assert "excess_mean" in header and "paired_excess_diff_mean" in header and "moves_ci95_hi" in header
    assert on["eval_paths_routes.csv"].decode().splitlines()[0] == "env,agent,roads,truncated,route"


def _without_wall_times(doc, dropped):
    """A JSON document without its wall-clock fields (keys ending in ``_ms``) and without the two settings the trace adds
    (counted in ``dropped``): what must be equal between a run with and a run without the flag."""
    if isinstance(doc, dict):
        out = {}
        for k, v in doc.items():
            if k.endswith("_ms"):
                continue
            if k == "settings" and isinstance(v, dict):
                dropped.append(sum(1 for key in ("paths", "path_max_hops") if key in v))
                v = {key: val for key, val in v.items() if key not in ("paths", "path_max_hops")}
            out[k] = _without_wall_times(v, dropped)
        return out
    if isinstance(doc, list):
        return [_without_wall_times(v, dropped) for v in doc]
    return doc


def _csv_without_wall_times(raw):
    import csv
    import io
    rows = list(csv.reader(io.StringIO(raw.decode())))
    keep = [j for j, name in enumerate(rows[0]) if not name.endswith("_ms")]
    return [[r[j] for j in keep] for r in rows]


def test_cli_dijkstra_envs_and_replan_days(tmp_path, capsys):
    """--dijkstra-envs and --replan-days 2 in one run, with and without the flag: the new files and keys are there, every old
    file is byte-identical — but the wall-clock plot, and the wall-clock columns (``*_ms``) of replan_days.csv, which differ
    between any two runs — and the old JSON keys are equal apart from the wall times and the two new settings."""
    import json
    base = ["--algo", "dijkstra", "--dijkstra-method", "per_destination", "--mode", "eval", "--scenario", SCENARIO,
            "--dijkstra-envs", "2", "--dijkstra-router", "free_flow", "--route-departures", "--eval-trips", "--replan-days", "2",
            "--replan-envs", "2", "--steps", "40"]
    _main(base + ["--output-dir", str(tmp_path / "off")])
    capsys.readouterr()
    _main(base + ["--eval-paths", "--output-dir", str(tmp_path / "on")])
    assert capsys.readouterr().out.count("=== Paths ===") == 2
    off, on = _files(tmp_path / "off"), _files(tmp_path / "on")
    assert set(on) - set(off) == {"dijkstra_paths.csv", "dijkstra_paths_by_departure.csv", "replan_paths.csv",
                                  "replan_paths_by_departure.csv"}
    for name in sorted(set(off) - {"computation_time.png"}):
        if name.endswith(".json"):
            doc_on, doc_off = json.loads(on[name]), json.loads(off[name])
            assert doc_on.pop("paths")["available"] and "paths" not in doc_off, name
            d_on, d_off = [], []
            assert _without_wall_times(doc_on, d_on) == _without_wall_times(doc_off, d_off), name
            assert sum(d_on) >= 2 and sum(d_off) == 0, name      # the evaluator's settings name the trace, and only they
        elif name.endswith(".csv") and b"_ms" in off[name].splitlines()[0]:
            assert _csv_without_wall_times(on[name]) == _csv_without_wall_times(off[name]), name
        else:
            assert on[name] == off[name], name
    assert {"dijkstra_envs.json", "dijkstra_envs.csv", "replan_days.csv", "replan_envs.json", "replan_envs.csv",
            "dijkstra_trips.csv", "replan_trips.csv"} <= set(off)


def test_cli_refusals():
    for argv, msg in ((["--algo", "mpnn", "--mode", "eval", "--eval-paths"], "eval_envs > 0 or dijkstra_envs > 0"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--eval-paths-max-hops", "4"], "needs that flag"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--eval-paths-routes", "1"], "needs that flag"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--eval-paths", "--eval-paths-max-hops", "0",
                        "--eval-paths-routes", "1"], "none is kept"),
                      (["--algo", "mpnn", "--mode", "eval", "--eval-envs", "2", "--eval-paths", "--eval-paths-max-hops", "5000"],
                       "in \\[0, 4096\\]")):
        with pytest.raises(ValueError, match=msg):
            _main(argv + ["--scenario", SCENARIO])
