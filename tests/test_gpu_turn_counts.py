"""GPU: per-turn movement counts — tarl_turn_counts_accumulate against the numpy restatement, frames composed by hand and
VecEvaluator(turns=True) against the CPU oracle's own choice (Direction's Gumbel race, replayed with the exported noise), and
the CLI end to end. Every comparison is ==."""
import csv
import importlib
import json

import numpy as np
import pytest
import torch

import link_counts_restatement as LR
import turn_counts_restatement as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.crafted_cases()}
_PLANS = {}


# ---- 1. the accumulate kernel ----------------------------------------------------------------------------------------------------
def _device_accumulate(call, tables, case):
    from tarl_hip import ops
    if case["name"] not in _PLANS:
        _PLANS[case["name"]] = ops.Plan(torch.from_numpy(case["edge_index"]), case["N"])
    plan = _PLANS[case["name"]]
    dev = [torch.from_numpy(t).cuda() for t in tables]
    prev = None if call["prev"] is None else torch.from_numpy(call["prev"]).cuda()
    ops.turn_counts_accumulate(plan, torch.from_numpy(call["popped"]).cuda(), torch.from_numpy(call["sel8"]).cuda(),
                               torch.from_numpy(call["counts"]).cuda(), *dev, prev_counts=prev, t0=call["t0"],
                               timestep=case["timestep"], bin_seconds=case["bin_seconds"], first_bin=case["first_bin"])
    return tuple(t.cpu().numpy() for t in dev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_equals_the_restatement(name):
    case = CASES[name]
    want = R.run_case(case)
    got = R.run_case(case, accumulate_fn=_device_accumulate)
    for g, w, table in zip(got, want, ("turns", "lost", "unresolved")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, table)
    assert sum(int(g.sum()) for g in got) == R.popped_bits(case) > 0      # every popped bit in exactly one table
    assert not got[0][:, 0].any() and not got[0][:, -1].any() and not got[1][:, 0].any() and not got[1][:, -1].any()


def test_accumulate_takes_a_prefix_of_the_rings_and_unaligned_bases():
    """``frames``: only the first frames of the rings are read (the evaluator's partial last block); byte rings that start
    1 - 3 bytes into an allocation and float rings that start one float into theirs; the bytes around them are ones (a read
    outside the prefix or the ring would count)."""
    from tarl_hip import ops
    F, K, N, use = 9, 3, 67, 6
    ei = R.crafted_graph(N, 13)
    plan = ops.Plan(torch.from_numpy(ei), N)
    p, s, c = R._rings(ei, N, F, K, 300)
    prev = R.COUNT_VALUES[np.random.default_rng(301).integers(0, R.COUNT_VALUES.size, size=(N, K))]
    E = ei.shape[1]
    want = (np.zeros((K, 2, E), np.int32), np.zeros((K, 2, N), np.int32), np.zeros(K, np.int32))
    R.accumulate(ei, N, p[:use], s[:use], c[:use], prev, *want, 96, 1, 100, 0)
    assert all(int(w.sum()) > 0 for w in want) and int(want[0][:, 0].sum()) > 0 and int(want[0][:, 1].sum()) > 0
    n = F * K * N
    for shift in (0, 1, 2, 3):
        raw_p, raw_s = (torch.full((n + 8,), 1, dtype=torch.uint8, device="cuda") for _ in range(2))
        raw_c, raw_v = torch.ones(n + 2, device="cuda"), torch.ones(N * K + 2, device="cuda")
        dp, ds = raw_p[shift:shift + n].view(F, K, N), raw_s[shift:shift + n].view(F, N, K)
        dc, dv = raw_c[shift % 2:shift % 2 + n].view(F, N, K), raw_v[shift % 2:shift % 2 + N * K].view(N, K)
        for d, h in ((dp, p), (ds, s), (dc, c), (dv, prev)):
            d.copy_(torch.from_numpy(h))
        got = (torch.zeros((K, 2, E), dtype=torch.int32, device="cuda"), torch.zeros((K, 2, N), dtype=torch.int32, device="cuda"),
               torch.zeros(K, dtype=torch.int32, device="cuda"))
        ops.turn_counts_accumulate(plan, dp, ds, dc, *got, prev_counts=dv, t0=96, timestep=1, bin_seconds=100, first_bin=0,
                                   frames=use)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w), shift


def test_a_call_that_would_reach_bin_H_is_refused_and_leaves_the_tables_untouched():
    from tarl_hip import lib, ops
    F, K, N, H = 8, 2, 5, 2
    ei = R.crafted_graph(N, 11)
    E = ei.shape[1]
    plan = ops.Plan(torch.from_numpy(ei), N)
    popped = torch.ones((F, K, N), dtype=torch.uint8, device="cuda")
    sel8 = torch.zeros((F, N, K), dtype=torch.uint8, device="cuda")
    counts = torch.ones((F, N, K), device="cuda")
    tables = (torch.full((K, H, E), 7, dtype=torch.int32, device="cuda"), torch.full((K, H, N), 7, dtype=torch.int32, device="cuda"),
              torch.full((K,), 7, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="bin out of range"):            # the last frame starts at 200: bin 2 of 2
        ops.turn_counts_accumulate(plan, popped, sel8, counts, *tables, t0=193, timestep=1, bin_seconds=100, first_bin=0)
    L = lib.load()
    ptrs = [t.data_ptr() for t in tables]
    rc = L.tarl_turn_counts_accumulate(plan.handle, popped.data_ptr(), sel8.data_ptr(), counts.data_ptr(), None, F, K, 193, 1, 100,
                                       0, H, *ptrs, lib.current_stream())
    assert rc == -1 and b"bin >= H" in L.tarl_last_error()
    rc = L.tarl_turn_counts_accumulate(plan.handle, popped.data_ptr(), sel8.data_ptr(), counts.data_ptr(), None, F, K, 193, 1, 100,
                                       2, H, *ptrs, lib.current_stream())
    assert rc == -1 and b"below first_bin" in L.tarl_last_error()
    rc = L.tarl_turn_counts_accumulate(plan.handle, popped.data_ptr(), None, counts.data_ptr(), None, F, K, 192, 1, 100, 0, H,
                                       *ptrs, lib.current_stream())
    assert rc == -1 and b"null" in L.tarl_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in tables)
    ops.turn_counts_accumulate(plan, popped, sel8, counts, *tables, t0=192, timestep=1, bin_seconds=100, first_bin=0)
    # one second earlier fits. Frame 0 sees empty roads (no prev): K N phantom pops in bin 1; the other 7 frames move over rank 0
    # where the road has an out-edge (roads 0, 1, 3, 4) and are unresolved on road 2, which has none
    turns, lost, unres = (t.cpu().numpy() for t in tables)
    out_ptr, out_eid = R.csr(ei, N)
    first = [int(out_eid[out_ptr[u]]) for u in (0, 1, 3, 4)]
    assert bool((turns[:, 0] == 7).all()) and bool((lost[:, 0] == 7).all())
    assert bool((lost[:, 1] == 8).all()) and unres.tolist() == [7 + 7] * K
    assert bool((turns[:, 1, first] == 14).all()) and int((turns[:, 1] - 7).sum()) == K * 4 * 7


# ---- 2. frames composed by hand against the oracle's own choice ---------------------------------------------------------------------
def _replay(net, pop, eng, noise0, T, clock0, choices_of, b):
    from tarl_hip import ops
    return R.oracle_replay(net, pop, T, clock0, choices_of,
                           lambda f: dict(gumbel=ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + f, [b])[0].cpu()))


def _hand_composed(net, pop, K, T, BIN, seed):
    """T frames of frame_fused(action=<host-drawn random out-edge per road>, popped=, counts=) with the SELECTED_ROAD bytes
    copied after every frame, one accumulate launch over the rings, and per environment the oracle replay."""
    import irregular_graphs as ig
    from tarl_hip import ops
    from tarl_hip.engine import EPISODE_START
    N, E = net.num_roads, net.edge_index.size(1)
    eng = LR.engine_of(net, pop, K, seed=seed)
    eng.reset()
    gen = torch.Generator().manual_seed(seed)
    actions = torch.stack([ig.random_actions(net, gen, B=K) for _ in range(T)])              # (T, K, N) int32
    popped = torch.zeros((T, K, N), dtype=torch.uint8, device="cuda")
    sel8 = torch.zeros((T, N, K), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((T, N, K), device="cuda")
    reward = torch.zeros((T, K), device="cuda")
    noise0 = eng.noise_counter + 1
    for t in range(T):
        eng.frame_fused(action=actions[t].cuda(), popped=popped[t], counts=counts[t], reward=reward[t])
        sel8[t].copy_(eng.fs.sel8)
    eng.check_flags()
    first_bin = EPISODE_START // BIN
    H = (EPISODE_START + T - 1) // BIN - first_bin + 1
    tables = (torch.zeros((K, H, E), dtype=torch.int32, device="cuda"), torch.zeros((K, H, N), dtype=torch.int32, device="cuda"),
              torch.zeros(K, dtype=torch.int32, device="cuda"))
    ops.turn_counts_accumulate(eng.plan, popped, sel8, counts, *tables, t0=EPISODE_START, bin_seconds=BIN)
    turns, lost, unres = (t.cpu().numpy() for t in tables)
    stats = []
    for b in range(K):
        o = _replay(net, pop, eng, noise0, T, EPISODE_START, lambda f: actions[f, b].numpy(), b)
        assert torch.equal(o["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        assert np.array_equal(o["reward"], reward[:, b].cpu().numpy()), f"rewards of environment {b}"
        assert np.array_equal(o["popped"][:, 0], popped[:, b].cpu().numpy() & 1), f"popped masks of environment {b}"
        assert np.array_equal(o["sel8"][:, :, 0], sel8[:, :, b].cpu().numpy() & 0x7F), f"rank bytes of environment {b}"
        want = R.moved_binned(o["moved"], EPISODE_START, BIN)
        assert np.array_equal(turns[b], want), f"turns of environment {b}"
        assert int(unres[b]) == 0 and int(lost[b].sum()) == o["unqueued"] == int(o["accepted"].sum()) - int(o["moved"].sum())
        used = want.sum(axis=0) > 0
        two = int((np.bincount(net.edge_index[0].numpy(), weights=used, minlength=N) >= 2).sum())
        last_clock = [min((first_bin + h + 1) * BIN, EPISODE_START + T) - 1 for h in range(H)]
        assert all(int(want[h].sum()) > 0 for h in range(H) if last_clock[h] > 21560), want.sum(axis=1)
        assert o["max_count"] < net.Nmax
        stats.append(dict(moved=want.sum(axis=1).tolist(), phantom=int(lost[b].sum()), used=int(used.sum()), two=two,
                          max_count=o["max_count"]))
        print(f"[hand composed] environment {b}: {stats[-1]}")
    return stats


def test_hand_composed_frames_on_the_torus():
    """8 x 8 torus, the population of the link-count tests, K = 2, T = 300, bins of 100 s, random actions drawn on the host.
    Guards from the oracle's own replay: every bin holds movements, at least one phantom pop, at least 100 roads use two of
    their out-edges, no count reaches Nmax. (CPU oracle under torch's own noise, seeds 0 - 2: 123 - 127 phantom pops, 438 -
    492 of 1 024 edges used, 141 - 171 roads with two out-edges in use, largest queue 3. Under device noise, engine seed 3,
    environments 0 / 1: movements per bin [84, 280, 257, 22] / [89, 304, 275, 12], 123 / 126 phantom pops, 489 / 493 edges used,
    170 / 161 roads with two out-edges in use, largest count 3.)"""
    from tarl_hip import synth
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    pop = LR.deliverable_population(net, LR.oracle_mode(net, emb)[2])
    for s in _hand_composed(net, pop, 2, 300, 100, seed=3):
        assert s["phantom"] >= 1 and s["two"] >= 100


def test_hand_composed_frames_on_the_small_graph():
    """21 roads, 49 edges in no order, 63 agents, K = 2, T = 200, bins of 50 s. (CPU oracle, torch noise: all 49 edges used, 4
    and 0 phantom pops with seeds 0 and 1, largest queue 10 - 12 of 15. Under device noise, engine seed 11, environments 0 / 1:
    movements per bin [0, 65, 190, 204, 148] / [0, 64, 198, 218, 160] (the first bin ends at 21 549 s), 7 / 4 phantom pops, all 49
    edges used, largest count 11 / 10.)"""
    net = LR.small_graph()
    _hand_composed(net, LR.small_population(net), 2, 200, 50, seed=11)


# ---- 3. the evaluator ------------------------------------------------------------------------------------------------------------
def _check_run(ev, res, net, pop, noise0, T, BIN, choices_of):
    """``res`` of ``ev`` against the oracle replay of every environment; ``choices_of(b)`` -> the frame -> action map."""
    from tarl_hip.engine import EPISODE_START
    eng = ev.eng
    assert not res.domain_exit and res.frames_run == T
    K, H, E = res.turn_counts.shape
    assert res.turn_counts.dtype == np.int32 and res.turn_lost.shape == (K, H, net.num_roads)
    assert res.turn_meta["first_bin"] == EPISODE_START // BIN and res.turn_meta["bin_seconds"] == BIN
    assert int(ev.turn_acc["unresolved"].sum()) == 0
    out = []
    for b in range(K):
        o = _replay(net, pop, eng, noise0, T, EPISODE_START, choices_of(b), b)
        assert np.array_equal(o["reward"], ev.reward[:T, b].cpu().numpy()), f"rewards of environment {b}"
        assert torch.equal(o["agents"], eng.agents[b].cpu()), f"agent table of environment {b}"
        assert np.array_equal(res.turn_counts[b], R.moved_binned(o["moved"], EPISODE_START, BIN)), f"turns of environment {b}"
        lost = R.binned(net.edge_index.numpy(), net.num_roads, o["popped"], o["sel8"], o["counts"], EPISODE_START, 1, BIN)[2]
        assert np.array_equal(res.turn_lost[b], lost[0]), f"lost of environment {b}"
        assert int(res.turn_lost[b].sum()) == o["unqueued"] == res.on_way[b] - int(-o["reward"][-1])
        out.append(o)
    LR.assert_stats_equal({k: res.turn_stats["turns"][k] for k in ("sum", "sumsq", "min", "max")}, LR.stats(res.turn_counts))
    LR.assert_stats_equal({k: res.turn_stats["lost"][k] for k in ("sum", "sumsq", "min", "max")}, LR.stats(res.turn_lost))
    return out


def test_evaluator_turns_replayed_by_the_oracle():
    """The 8 x 8 torus MODE recipe of the link-count tests, K = 2, T = 300, bins of 100 s, ``turn_block`` = 300 so that the
    SELECTED_ROAD ring holds the whole run. MODE: the oracle's movements differ from its acceptances (18 phantom pops under
    torch's noise), so the naive rule would fail here. Sampled: the actions are decoded from the evaluator's own ring,
    replayed by the oracle, and the per-frame rewards must agree: the ring holds the action the device used. Then both runs
    again with ``turn_block`` = 7 (block edges inside bins, the carry of the counts between blocks): identical tables.
    (Measured under device noise, engine seed 3: MODE movements per bin [85, 495, 686, 255] / [85, 495, 680, 248], acceptances -
    movements 18 / 18; sampled [74, 343, 370, 73] / [90, 327, 306, 53], 114 / 118 agents lost, 558 edges used.)"""
    from tarl_hip import synth
    from tarl_hip.evaluator import turn_report
    net = synth.torus_network(8, 8)
    N, K, T, BIN = net.num_roads, 2, 300, 100
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    _, action, succ = LR.oracle_mode(net, emb)
    pop = LR.deliverable_population(net, succ)
    mode_choice = np.full(N, -1, dtype=np.int64)
    chosen = action.nonzero().view(-1)
    mode_choice[net.edge_index[0, chosen].numpy()] = chosen.numpy()
    ev, _ = LR.embedding_evaluator(net, pop, K, turns=True, link_bin_seconds=BIN, turn_block=T)
    assert ev.turn_sel.shape == (T, N, K) and ev.turn_popped.shape == (T, K, N) and ev.turn_ring.shape == (T, N, K)
    noise0 = ev.eng.noise_counter + 1
    res = ev.run(T)
    mode = _check_run(ev, res, net, pop, noise0, T, BIN, lambda b: (lambda f: mode_choice))
    gap = [int(o["accepted"].sum()) - int(o["moved"].sum()) for o in mode]
    print(f"[evaluator MODE] movements per bin {res.turn_counts.sum(axis=2).tolist()}, acceptances - movements {gap}")
    assert all(g > 0 for g in gap)                              # the naive rule is wrong on this very run
    rep = turn_report(res)
    assert rep["summary"]["identity"]["holds"] and rep["summary"]["lost_per_env"] == gap
    assert rep["rows"][0]["policy_prob"] is not None
    tables = {True: (res.turn_counts, res.turn_lost)}
    # (a fresh engine: a reset keeps the ARRIVAL_TIME column of the run before, which the replay from the population lacks)
    ev, _ = LR.embedding_evaluator(net, pop, K, turns=True, link_bin_seconds=BIN, turn_block=T)
    noise0 = ev.eng.noise_counter + 1
    res = ev.run(T, deterministic=False)
    ring = ev.turn_sel.cpu().numpy()                                                # (T, N, K): the run's action bytes
    _check_run(ev, res, net, pop, noise0, T, BIN, lambda b: (lambda f: R.choice_of_ranks(net, ring[f, :, b])))
    used = res.turn_counts.sum(axis=(0, 1)) > 0
    print(f"[evaluator sampled] movements per bin {res.turn_counts.sum(axis=2).tolist()}, lost {res.turn_lost.sum(axis=(1, 2)).tolist()}, "
          f"edges used {int(used.sum())}")
    tables[False] = (res.turn_counts, res.turn_lost)
    for det in (True, False):      # (fresh engines again: the same noise counters as the runs above)
        small, _ = LR.embedding_evaluator(net, pop, K, turns=True, link_bin_seconds=BIN, turn_block=7)
        again = small.run(T, deterministic=det)
        assert np.array_equal(again.turn_counts, tables[det][0]) and np.array_equal(again.turn_lost, tables[det][1]), det


def test_turn_counting_shares_the_rings_and_does_not_perturb_the_run():
    """With link counts and occupancy on, the frames write one popped and one counts slice: the turn rings get theirs by
    sharing (equal blocks) or by a copy (unequal blocks); the tables, and everything else, equal those of a run with turns alone."""
    from tarl_hip import synth
    from tarl_hip.evaluator import PER_ENV_KEYS
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    pop = LR.deliverable_population(net, LR.oracle_mode(net, emb)[2])
    alone, _ = LR.embedding_evaluator(net, pop, 3, turns=True)
    r0 = alone.run(200)
    off, _ = LR.embedding_evaluator(net, pop, 3)
    assert not off.turns and not hasattr(off, "turn_popped")              # no buffers without the flag
    r_off = off.run(200)
    assert r_off.turn_counts is None and r_off.turn_meta is None
    for kw in (dict(), dict(turn_block=5)):
        both, _ = LR.embedding_evaluator(net, pop, 3, turns=True, link_counts=True, occupancy=True, **kw)
        assert (both.turn_ring is both.occ_ring) == (not kw)
        r1 = both.run(200)
        assert np.array_equal(r1.turn_counts, r0.turn_counts) and np.array_equal(r1.turn_lost, r0.turn_lost)
        assert int(r1.link_counts.sum()) > 0 and r1.occupancy is not None
        for k in PER_ENV_KEYS:
            assert getattr(r0, k) == getattr(r1, k) == getattr(r_off, k), k
    assert int(r0.turn_counts.sum()) > 0 and "turn_counts" not in r0.to_dict(per_env=True)
    with pytest.raises(ValueError, match="turn_block"):
        LR.embedding_evaluator(net, pop, 3, turns=True, turn_block=0)
    with pytest.raises(ValueError, match="turn_block"):
        LR.embedding_evaluator(net, pop, 3, turn_block=4)


# ---- 4. CLI end to end ------------------------------------------------------------------------------------------------------------
def test_cli_turns_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-300"
    on = tmp_path / "on"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--eval-turns", "--eval-baseline", "dijkstra",
          "--steps", "120", "--output-dir", str(on)])
    text = capsys.readouterr().out
    assert "=== Turns ===" in text and text.index("=== Turns ===") > text.index("=== Vectorised evaluation (4")
    assert "agents lost (Q24)" in text and "policy - dijkstra" in text
    doc = json.load(open(on / "eval_envs.json"))
    assert not doc["mode"]["domain_exit"], "the synthetic scenario left the domain under MODE"
    rows = list(csv.DictReader(open(on / "eval_turns.csv")))
    t = doc["turns"]
    s = t["summary"]
    assert t["available"] and "rows" not in t and "lost_rows" not in t and t["columns"] == list(rows[0])
    assert len(rows) == s["edges"] == 1024 and [int(r["edge"]) for r in rows] == list(range(1024))
    assert list(rows[0])[:3] == ["edge", "from_road", "to_road"] and "policy_prob" in rows[0] and "paired_diff_mean" in rows[0]
    assert s["envs"] == 4 and s["frames_run"] == 120 and s["identity"]["holds"]
    total = sum(s["movements_per_env"])
    assert total > 0 and abs(sum(float(r["mean"]) for r in rows) * 4 - total) < 1e-6 * total
    assert abs(sum(float(r[b]) for r in rows for b in t["bins"]) * 4 - total) < 1e-6 * total
    assert abs(sum(s["movements_per_bin"]) * 4 - total) < 1e-6 * total
    lost_rows = list(csv.DictReader(open(on / "eval_turns_lost.csv")))
    assert len(lost_rows) == s["roads_with_a_loss"] and abs(sum(float(r["mean"]) for r in lost_rows) * 4 - sum(s["lost_per_env"])) < 1e-9
    assert s["paired"]["available"] and s["paired"]["baseline_head"] == "dijkstra"
    assert "turns" not in doc["mode"] and "turns" not in doc["baseline"]
    # the router alone
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--mode", "eval", "--scenario", scenario, "--dijkstra-envs", "4", "--eval-turns",
          "--eval-link-counts", "--steps", "60", "--start-end-time", "21540", "21600", "--output-dir", str(dj)])
    text = capsys.readouterr().out
    assert "=== Turns ===" in text and text.index("=== Turns ===") > text.index("=== Link counts ===")
    rows = list(csv.DictReader(open(dj / "dijkstra_turns.csv")))
    assert len(rows) == 1024 and "policy_prob" not in rows[0] and "paired_diff_mean" not in rows[0]
    assert (dj / "dijkstra_turns_lost.csv").exists()
    assert json.load(open(dj / "dijkstra_envs.json"))["turns"]["summary"]["envs"] == 4
    # without the flag: none of it
    off = tmp_path / "off"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--steps", "40",
          "--output-dir", str(off)])
    assert "Turns" not in capsys.readouterr().out
    assert not (off / "eval_turns.csv").exists() and set(json.load(open(off / "eval_envs.json"))) == {"mode"}
