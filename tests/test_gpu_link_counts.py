"""GPU: per-road link counts — tarl_link_counts_accumulate and tarl_link_count_stats against the numpy restatement with ==,
VecEvaluator(link_counts=True) against the CPU oracle and against frames composed by hand, and the CLI end to end."""
import csv
import functools
import importlib
import json

import numpy as np
import pytest
import torch

import link_counts_restatement as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.crafted_cases()}


# ---- 1. the accumulate kernel ----------------------------------------------------------------------------------------------------
def _device_accumulate(call, counts, case):
    from tarl_hip import ops
    dev = torch.from_numpy(counts).cuda()
    ops.link_counts_accumulate(torch.from_numpy(call["popped"]).cuda(), torch.from_numpy(call["withdrawn"]).cuda(), dev,
                               t0=call["t0"], timestep=case["timestep"], bin_seconds=case["bin_seconds"],
                               first_bin=case["first_bin"])
    return dev.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_equals_the_restatement(name):
    case = CASES[name]
    want = R.run_case(case)
    got = R.run_case(case, accumulate_fn=_device_accumulate)
    assert got.dtype == np.int32 and np.array_equal(got, want), name
    assert int(want.sum()) > 0 and not want[:, 0].any() and not want[:, -1].any()      # the bins on either side stay empty
    if name == "all-ones-max-F-twice":
        first = R.run_case(dict(case, calls=case["calls"][:1]), accumulate_fn=_device_accumulate)
        assert first[:, 1, :].tolist() == [[2 * R.MAX_FRAMES] * 5]             # one call at the declared maximum: exactly 2 F
        assert got[:, 1, :].tolist() == [[4 * R.MAX_FRAMES] * 5]


def test_accumulate_takes_a_prefix_of_the_ring_and_unaligned_slices():
    """``frames``: only the first frames of a ring are read (the evaluator's partial last block); a ring that starts one
    byte into an allocation, so that no slice is word-aligned."""
    from tarl_hip import ops
    F, B, N = 9, 3, 5
    p, w = R._masks(F, B, N, seed=9)
    want = np.zeros((B, 2, N), dtype=np.int32)
    R.accumulate(p[:6], w[:6], want, 96, 1, 100, 0)
    for shift in (0, 1, 2, 3):
        raw_p, raw_w = (torch.full((F * B * N + 8,), 1, dtype=torch.uint8, device="cuda") for _ in range(2))
        dp, dw = (r[shift:shift + F * B * N].view(F, B, N) for r in (raw_p, raw_w))
        dp.copy_(torch.from_numpy(p))
        dw.copy_(torch.from_numpy(w))
        counts = torch.zeros((B, 2, N), dtype=torch.int32, device="cuda")
        ops.link_counts_accumulate(dp, dw, counts, t0=96, timestep=1, bin_seconds=100, first_bin=0, frames=6)
        assert np.array_equal(counts.cpu().numpy(), want), shift


def test_a_call_that_would_reach_bin_H_is_refused_and_leaves_counts_untouched():
    from tarl_hip import lib, ops
    F, B, N, H = 8, 2, 5, 2
    ones = torch.ones((F, B, N), dtype=torch.uint8, device="cuda")
    counts = torch.full((B, H, N), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="bin out of range"):            # the last frame starts at 200: bin 2 of 2
        ops.link_counts_accumulate(ones, ones, counts, t0=193, timestep=1, bin_seconds=100, first_bin=0)
    L = lib.load()
    rc = L.tarl_link_counts_accumulate(ones.data_ptr(), ones.data_ptr(), F, B, N, 193, 1, 100, 0, H, counts.data_ptr(),
                                       lib.current_stream())
    assert rc == -1 and b"bin >= H" in L.tarl_last_error()
    rc = L.tarl_link_counts_accumulate(ones.data_ptr(), ones.data_ptr(), F, B, N, 193, 1, 100, 2, H, counts.data_ptr(),
                                       lib.current_stream())
    assert rc == -1 and b"below first_bin" in L.tarl_last_error()
    torch.cuda.synchronize()
    assert bool((counts == 7).all())
    ops.link_counts_accumulate(ones, ones, counts, t0=192, timestep=1, bin_seconds=100, first_bin=0)       # one second earlier fits
    assert counts.cpu()[:, 1].tolist() == [[7 + 2 * F] * N] * B and bool((counts[:, 0] == 7).all())


# ---- 2. the statistics kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 64, 65])
def test_stats_equal_numpy_int64(K):
    from tarl_hip import ops
    rng = np.random.default_rng(K)
    for H in (1, 3):
        for N in (1, 21, 257):
            a = rng.integers(0, 7201, size=(K, H, N)).astype(np.int32)
            b = rng.integers(0, 7201, size=(K, H, N)).astype(np.int32)
            a[0, 0, 0], b[0, 0, 0] = 7200, 0
            da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            R.assert_stats_equal(ops.link_count_stats(da), R.stats(a))
            R.assert_stats_equal(ops.link_count_stats(da, db), R.stats(a, b))
            out = {k: torch.empty((H + 1, N), dtype=dt, device="cuda")
                   for k, dt in (("sum", torch.int64), ("sumsq", torch.int64), ("min", torch.int32), ("max", torch.int32))}
            assert ops.link_count_stats(db, da, out=out) is out
            R.assert_stats_equal(out, R.stats(b, a))
            if K >= 64 and H == 3:      # totals near 10 800: 64 squares of them pass 2^31, the sums need their 64 bits
                assert int(R.stats(a)["sumsq"].max()) > 2 ** 31


# ---- 3. oracle replay ---------------------------------------------------------------------------------------------------------------
def test_link_counts_replayed_by_the_oracle():
    """The 8 x 8 torus MODE recipe of test_mode_evaluation_replayed_by_the_oracle (128 agents, every other one bound three
    MODE steps from its origin, embedding seed 0, engine seed 3), K = 2, T = 300, bins of 100 s: the clock starts at 21 540, so
    bin edges fall at frames 60, 160 and 260; with the default block of 64 frames the blocks 0, 2 and 4 straddle an edge and
    the last block (frames 256 - 299) is partial. oracle.sim.env_step replays every environment with the exported Gumbel
    values; its popped and withdrawn masks, summed per bin, must equal res.link_counts with ==. Guards, from the oracle's own
    masks: every bin holds pops, at least two bins hold a withdrawal, at least one (road, frame) holds both, no count reaches
    Nmax. (CPU oracle under torch's own noise, seeds 0 - 2: 94 pops and no withdrawal in the first 60 frames, 1 434 - 1 436
    pops and 12 - 13 withdrawals in the other 240, 6 double events, largest count 11 of 15.)"""
    from oracle import sim
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import link_moments
    net = synth.torus_network(8, 8)
    N, Nmax, K, T, BIN = net.num_roads, net.Nmax, 2, 300, 100
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    _, action, succ = R.oracle_mode(net, emb)
    pop = R.deliverable_population(net, succ)
    ev, _ = R.embedding_evaluator(net, pop, K, link_counts=True, link_bin_seconds=BIN)
    assert ev.link_block == 64 and ev.link_popped.shape == (64, K, N)
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    assert res.link_first_bin == EPISODE_START // BIN == 215 and res.link_bin_seconds == BIN
    assert res.link_counts.shape == (K, 4, N) and res.link_counts.dtype == np.int32
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    popped, withdrawn = np.zeros((T, K, N), dtype=np.uint8), np.zeros((T, K, N), dtype=np.uint8)
    for b in range(K):
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pop.clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        max_count = 0.0
        for t in range(T):
            g = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
            out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, float(EPISODE_START + t), Nmax, gumbel=g,
                               congestion_constant=net.congestion_constant)
            popped[t, b] = out["popped"].reshape(-1).numpy().astype(bool)
            withdrawn[t, b] = out["withdrawn"].reshape(-1).numpy().astype(bool)
            max_count = max(max_count, float(x[:, c.N].max()))
        assert torch.equal(ag, eng.agents[b].cpu()), f"agent table of environment {b}"
        first, want = R.binned(popped[:, b:b + 1], withdrawn[:, b:b + 1], EPISODE_START, 1, BIN)
        pops = [int(popped[t0:t1, b].sum()) for t0, t1 in ((0, 60), (60, 160), (160, 260), (260, 300))]
        wds = [int(withdrawn[t0:t1, b].sum()) for t0, t1 in ((0, 60), (60, 160), (160, 260), (260, 300))]
        both = int((popped[:, b] & withdrawn[:, b]).sum())
        print(f"[link replay] environment {b}: pops per bin {pops}, withdrawals per bin {wds}, {both} double events, "
              f"largest count {max_count:.0f} of {Nmax}, largest link count {int(want.max())}")
        assert first == 215 and min(pops) > 0 and sum(1 for v in wds if v > 0) >= 2 and both >= 1 and max_count < Nmax
        assert np.array_equal(res.link_counts[b], want[0]), f"link counts of environment {b}"
    R.assert_stats_equal({k: res.link_stats[k] for k in ("sum", "sumsq", "min", "max")}, R.stats(res.link_counts))
    R.assert_moments_close(res.link_stats, R.moments(res.link_counts), K)
    R.assert_moments_close(link_moments(R.stats(res.link_counts), K), R.moments(res.link_counts), K)


# ---- 4. the evaluator against frames composed by hand, K N = 63 ----------------------------------------------------------------
T_HAND, K_HAND, SEED_HAND = 130, 3, 11


@functools.lru_cache(maxsize=None)
def _hand_composed():
    """The masks of 130 sampled frames of the embedding head on the 21-road graph, from frame_fused one frame at a time:
    (popped, withdrawn) uint8 (T, K, N) on the host, computed once and left unchanged."""
    net = R.small_graph()
    eng = R.engine_of(net, R.small_population(net), K_HAND, seed=SEED_HAND)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0)).cuda()
    eng.reset()
    eng.prepare_policy(emb, 1.0)
    p = torch.zeros((T_HAND, K_HAND, net.num_roads), dtype=torch.uint8, device="cuda")
    w = torch.zeros_like(p)
    rw = torch.zeros((T_HAND, K_HAND), device="cuda")
    for t in range(T_HAND):
        eng.frame_fused(reward=rw[t], popped=p[t], withdrawn=w[t])
    eng.check_flags()
    return p.cpu(), w.cpu(), eng.agents.cpu()


@pytest.mark.parametrize("bin_seconds", [3600, 25])
@pytest.mark.parametrize("link_block", [1, 7, 64])
def test_evaluator_equals_frames_composed_by_hand(link_block, bin_seconds):
    """(CPU oracle, random actions, this graph and population: 67 pops in the first 60 frames, 286 in the next 70, largest
    count 10 of 40, every road counted.) The expected value sums the masks with torch. Every road's total over the three
    environments must be > 0; under the sampled embedding policy one road of one environment can stay at 0 (printed)."""
    from tarl_hip.engine import EPISODE_START
    p, w, agents = _hand_composed()
    net = R.small_graph()
    N = net.num_roads
    assert (K_HAND * N) % 4 == 3
    ev, _ = R.embedding_evaluator(net, R.small_population(net), K_HAND, seed=SEED_HAND, link_counts=True,
                                  link_bin_seconds=bin_seconds, link_block=link_block)
    res = ev.run(T_HAND, deterministic=False)
    assert not res.domain_exit and torch.equal(ev.eng.agents.cpu(), agents)
    bins = (EPISODE_START + torch.arange(T_HAND)) // bin_seconds
    first = int(bins[0])
    H = int(bins[-1]) - first + 1
    want = torch.zeros((K_HAND, H, N), dtype=torch.int32)
    want.index_add_(1, bins - first, (p.to(torch.int32) + w.to(torch.int32)).permute(1, 0, 2).contiguous())
    assert H == (2 if bin_seconds == 3600 else 6) and res.link_first_bin == first      # the clock passes 6 h at frame 60
    assert torch.equal(torch.from_numpy(res.link_counts), want)
    total = want.sum(dim=1)
    print(f"[hand composed] block {link_block}, bins of {bin_seconds} s: {int(p.sum())} pops, {int(w.sum())} withdrawals, "
          f"smallest road total per environment {int(total.min())}, over the environments {int(total.sum(dim=0).min())}, "
          f"largest {int(total.max())}")
    assert int(total.sum(dim=0).min()) > 0                            # every road's total > 0
    R.assert_stats_equal({k: res.link_stats[k] for k in ("sum", "sumsq", "min", "max")}, R.stats(want.numpy()))


def test_default_block_respects_the_ring_budget_and_the_declared_maximum():
    from tarl_hip import ops
    from tarl_hip.evaluator import LINK_RING_BYTES
    net = R.small_graph()
    pop = R.small_population(net)
    assert R.embedding_evaluator(net, pop, 2, link_counts=True, poll_frames=500)[0].link_block == ops.LINK_COUNTS_MAX_FRAMES
    assert R.embedding_evaluator(net, pop, 2, link_counts=True, poll_frames=5)[0].link_block == 5
    assert LINK_RING_BYTES == 256 << 20
    for bad in (0, ops.LINK_COUNTS_MAX_FRAMES + 1):
        with pytest.raises(ValueError, match="link_block"):
            R.embedding_evaluator(net, pop, 2, link_counts=True, link_block=bad)
    off = R.embedding_evaluator(net, pop, 2)[0]
    assert not off.link_counts and not hasattr(off, "link_popped")      # no buffers without the flag


# ---- 5. counting does not perturb the run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["embedding", "dijkstra"])
def test_link_counting_does_not_perturb_the_run(head):
    from tarl_hip import synth
    from tarl_hip.evaluator import PER_ENV_KEYS, VecEvaluator
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    pop = R.deliverable_population(net, R.oracle_mode(net, emb)[2])
    runs = []
    for flag in (False, True):
        if head == "embedding":
            ev, _ = R.embedding_evaluator(net, pop, 4, link_counts=flag)
        else:
            ev = VecEvaluator(R.engine_of(net, pop, 4), "dijkstra", link_counts=flag)
        runs.append((ev, ev.run(200)))
    (e0, r0), (e1, r1) = runs
    assert not r0.domain_exit and not r1.domain_exit and r0.frames_run == r1.frames_run == 200
    for k in PER_ENV_KEYS:
        assert getattr(r0, k) == getattr(r1, k), k
    assert r0.aggregate == r1.aggregate and r0.settings == r1.settings
    assert torch.equal(e0.reward[:200], e1.reward[:200]) and float(e0.reward.abs().sum()) > 0
    assert torch.equal(e0.eng.x, e1.eng.x) and torch.equal(e0.eng.agents, e1.eng.agents)
    assert r0.link_counts is None and r0.link_stats is None and r0.link_first_bin is None
    assert r1.link_counts.shape == (4, 2, net.num_roads) and int(r1.link_counts.sum()) > 0      # 200 frames: 5 h and 6 h
    assert "link_counts" not in r1.to_dict(per_env=True)               # the tensor never enters the JSON document


# ---- 6. domain exit -----------------------------------------------------------------------------------------------------------------
def test_a_domain_exit_returns_no_link_counts_and_leaves_the_engine_usable():
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import link_count_report
    net = synth.torus_network(8, 8)
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    ev, _ = R.embedding_evaluator(net, pop, 2, link_counts=True)
    res = ev.run(256)
    assert res.domain_exit and res.aggregate is None
    assert res.link_counts is None and res.link_stats is None and res.link_first_bin is None and res.link_bin_seconds is None
    assert not link_count_report(res)["available"]
    ev.eng.reset()
    ev.eng.check_flags()
    again = ev.run(8, deterministic=False)
    assert not again.domain_exit and again.frames_run == 8
    assert again.link_counts.shape == (2, 1, net.num_roads) and again.link_first_bin == 5
    assert 0 <= int(again.link_counts.min()) and int(again.link_counts.max()) <= 2 * 8      # only these eight frames were counted


# ---- 7. CLI end to end ----------------------------------------------------------------------------------------------------------
BASE_COLUMNS = ["road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max", "count_5h"]      # + count_6h from frame 60 on
EXPECTED_COLUMNS = ["expected_msa", "diff_msa", "geh_msa", "ue_flow", "diff_ue", "geh_ue", "so_flow", "diff_so", "geh_so"]
PAIRED_COLUMNS = ["baseline_mean", "paired_diff_mean", "paired_diff_se", "paired_diff_ci95_lo", "paired_diff_ci95_hi"]


def test_cli_link_counts_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-300"
    on = tmp_path / "on"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--eval-link-counts",
          "--eval-baseline", "dijkstra", "--equilibrium-metrics", "--steps", "120", "--output-dir", str(on)])
    text = capsys.readouterr().out
    assert "=== Link counts ===" in text and text.index("=== Link counts ===") > text.index("=== Vectorised evaluation (4")
    assert "vs msa:" in text and "vs ue:" in text and "vs so:" in text and "part of the demand" in text
    roads = len(list(csv.DictReader(open(on / "msa_expected_flows.csv"))))
    doc = json.load(open(on / "eval_envs.json"))
    assert not doc["mode"]["domain_exit"], "the synthetic scenario left the domain under MODE"
    rows = list(csv.DictReader(open(on / "eval_link_counts.csv")))
    assert list(rows[0]) == BASE_COLUMNS + ["count_6h"] + EXPECTED_COLUMNS + PAIRED_COLUMNS
    assert len(rows) == roads and [int(r["road"]) for r in rows] == list(range(roads))
    assert sum(float(r["mean"]) for r in rows) > 0
    lc = doc["link_counts"]
    assert lc["available"] and "rows" not in lc and lc["bins"] == ["count_5h", "count_6h"] and lc["columns"] == list(rows[0])
    s = lc["summary"]
    assert s["envs"] == 4 and s["roads"] == roads and s["frames_run"] == 120 and set(s["expected"]) == {"msa", "ue", "so"}
    assert s["paired"]["available"] and s["paired"]["baseline_head"] == "dijkstra"
    assert "link_counts" not in doc["mode"] and "link_counts" not in doc["baseline"]
    # the router alone
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--mode", "eval", "--scenario", scenario, "--dijkstra-envs", "4", "--eval-link-counts",
          "--steps", "60", "--start-end-time", "21540", "21600", "--output-dir", str(dj)])
    assert "=== Link counts ===" in capsys.readouterr().out
    rows = list(csv.DictReader(open(dj / "dijkstra_link_counts.csv")))
    assert len(rows) == roads and list(rows[0]) == BASE_COLUMNS + EXPECTED_COLUMNS[:3]
    assert json.load(open(dj / "dijkstra_envs.json"))["link_counts"]["summary"]["envs"] == 4
    # without the flag: none of it
    off = tmp_path / "off"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--steps", "40",
          "--output-dir", str(off)])
    assert "Link counts" not in capsys.readouterr().out
    assert not (off / "eval_link_counts.csv").exists() and set(json.load(open(off / "eval_envs.json"))) == {"mode"}
