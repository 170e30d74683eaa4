"""GPU: per-road occupancy — tarl_occupancy_accumulate against the numpy restatement with == on all three accumulators,
tarl_link_count_stats on them, VecEvaluator(occupancy=True) against the CPU oracle and against frames composed by hand, and
the CLI end to end."""
import csv
import functools
import importlib
import json

import numpy as np
import pytest
import torch

import occupancy_restatement as R

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.crafted_cases()}
ACC = ("veh", "full", "peak")


# ---- 1. the accumulate kernel ----------------------------------------------------------------------------------------------------
def _device_accumulate(call, acc, case):
    from tarl_hip import ops
    dev = [torch.from_numpy(a).cuda() for a in acc]
    out = ops.occupancy_accumulate(torch.from_numpy(call["ring"]).cuda(), torch.from_numpy(case["thr"]).cuda(), *dev,
                                   t0=call["t0"], timestep=case["timestep"], bin_seconds=case["bin_seconds"],
                                   first_bin=case["first_bin"])
    assert all(o is d for o, d in zip(out, dev))
    return tuple(d.cpu().numpy() for d in dev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_equals_the_restatement(name):
    """Every crafted case, the two with several calls into one set of accumulators included."""
    case = CASES[name]
    want = R.run_case(case)
    got = R.run_case(case, accumulate_fn=_device_accumulate)
    for key, g, w in zip(ACC, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (name, key)
    assert int(want[0].sum()) > 0 and int(want[1].sum()) > 0 and int(want[2].max()) == 127
    for a in got[:2]:
        assert not a[:, 0].any() and not a[:, -1].any()                # the bins on either side stay empty


def test_accumulate_takes_a_prefix_of_the_ring():
    """``frames``: only the first frames of a ring are read (the evaluator's partial last block); the rest holds values that
    would show."""
    from tarl_hip import ops
    case = CASES["65x63x9-no-edge"]
    ring, thr = case["ring"].copy(), case["thr"]
    ring[6:] = 200.0
    K, N = case["K"], case["N"]
    want = (np.zeros((K, 2, N), np.int32), np.zeros((K, 2, N), np.int32), np.zeros((K, 1, N), np.int32))
    R.accumulate(ring[:6], thr, *want, 96, 1, 100, 0)
    dev = [torch.zeros(a.shape, dtype=torch.int32, device="cuda") for a in want]
    ops.occupancy_accumulate(torch.from_numpy(ring).cuda(), torch.from_numpy(thr).cuda(), *dev, t0=96, timestep=1,
                             bin_seconds=100, first_bin=0, frames=6)
    for key, d, w in zip(ACC, dev, want):
        assert np.array_equal(d.cpu().numpy(), w), key
    assert want[0][:, 0].any() and want[0][:, 1].any() and int(want[2].max()) == 127


def test_a_call_that_would_reach_bin_H_is_refused_and_leaves_the_accumulators_untouched():
    from tarl_hip import lib, ops
    F, K, N, H = 8, 2, 5, 2
    ring = torch.full((F, N, K), 4.0, device="cuda")
    thr = torch.full((N,), 3, dtype=torch.int32, device="cuda")
    veh, full = (torch.full((K, H, N), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    peak = torch.full((K, 1, N), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="bin out of range"):            # the last frame starts at 200: bin 2 of 2
        ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=193, timestep=1, bin_seconds=100, first_bin=0)
    L = lib.load()
    ptrs = (veh.data_ptr(), full.data_ptr(), peak.data_ptr(), lib.current_stream())
    rc = L.tarl_occupancy_accumulate(ring.data_ptr(), thr.data_ptr(), F, K, N, 193, 1, 100, 0, H, *ptrs)
    assert rc == -1 and b"bin >= H" in L.tarl_last_error()
    rc = L.tarl_occupancy_accumulate(ring.data_ptr(), thr.data_ptr(), F, K, N, 193, 1, 100, 2, H, *ptrs)
    assert rc == -1 and b"below first_bin" in L.tarl_last_error()
    torch.cuda.synchronize()
    assert bool((veh == 7).all()) and bool((full == 7).all()) and bool((peak == 7).all())
    ops.occupancy_accumulate(ring, thr, veh, full, peak, t0=192, timestep=1, bin_seconds=100, first_bin=0)   # one second earlier fits
    assert veh.cpu()[:, 1].tolist() == [[7 + 4 * F] * N] * K and bool((veh[:, 0] == 7).all())
    assert full.cpu()[:, 1].tolist() == [[7 + F] * N] * K and bool((full[:, 0] == 7).all())
    assert bool((peak == 7).all())                                         # max-merged: 4 < 7 stays


def test_foreign_values_change_only_their_own_elements():
    """NaN, -1 and 300 in single elements: NaN and -1 count 0, 300 counts 255, and every other element is as without them."""
    from tarl_hip import ops
    case = CASES["65x63x9-no-edge"]
    K, N, H = case["K"], case["N"], 1
    thr = torch.from_numpy(case["thr"]).cuda()
    clean = case["ring"].copy()
    spots = ((2, 5, 7, np.nan), (3, 62, 64, -1.0), (4, 40, 0, 300.0), (0, 0, 1, -np.inf), (8, 1, 33, np.inf))
    for f, n, k, _ in spots:
        clean[f, n, k] = 0.0
    dirty = clean.copy()
    for f, n, k, v in spots:
        dirty[f, n, k] = v
    out = {}
    for name, ring in (("clean", clean), ("dirty", dirty)):
        dev = [torch.zeros(s, dtype=torch.int32, device="cuda") for s in ((K, H, N), (K, H, N), (K, 1, N))]
        ops.occupancy_accumulate(torch.from_numpy(ring).cuda(), thr, *dev, t0=0, timestep=1, bin_seconds=3600)
        out[name] = [d.cpu().numpy() for d in dev]
    want = (np.zeros((K, H, N), np.int32), np.zeros((K, H, N), np.int32), np.zeros((K, 1, N), np.int32))
    R.accumulate(dirty, case["thr"], *want, 0, 1, 3600, 0)
    for key, d, w in zip(ACC, out["dirty"], want):
        assert np.array_equal(d, w), key
    differs = out["dirty"][0] != out["clean"][0]
    assert sorted(zip(*np.nonzero(differs))) == [(0, 0, 40), (33, 0, 1)]       # only the two that count 255
    assert out["dirty"][0][0, 0, 40] - out["clean"][0][0, 0, 40] == 255 and out["dirty"][2][0, 0, 40] == 255


# ---- 2. the statistics kernel on the three accumulators -----------------------------------------------------------------------
def test_link_count_stats_serves_the_three_accumulators():
    from tarl_hip import ops
    case = CASES["130x70x5-skipping"]
    veh, full, peak = R.run_case(case)
    other = R.run_case(CASES["130x70x5-no-edge"])
    for key, a in zip(ACC, (veh, full, peak)):
        R.assert_stats_equal(ops.link_count_stats(torch.from_numpy(a).cuda()), R.stats(a))
    b = np.roll(veh, 1, axis=0)                                                # the paired form, same shape
    R.assert_stats_equal(ops.link_count_stats(torch.from_numpy(veh).cuda(), torch.from_numpy(b).cuda()), R.stats(veh, b))
    R.assert_stats_equal(ops.link_count_stats(torch.from_numpy(peak).cuda(), torch.from_numpy(other[2]).cuda()),
                         R.stats(peak, other[2]))
    assert peak.shape[1] == 1 and int(R.stats(veh)["sumsq"].max()) > 0


# ---- 3. oracle replay ---------------------------------------------------------------------------------------------------------------
def test_occupancy_replayed_by_the_oracle():
    """The 8 x 8 torus recipe of test_link_counts_replayed_by_the_oracle (128 agents, every other one bound three MODE steps
    from its origin, embedding seed 0, engine seed 3), K = 2, T = 300, bins of 100 s: the clock starts at 21 540, so bin edges
    fall at frames 60, 160 and 260; with the default block of 64 frames the blocks 0, 2 and 4 straddle an edge and the last
    block (frames 256 - 299) is partial. oracle.sim.env_step replays every environment with the exported Gumbel values; its
    NUMBER_OF_AGENT column after each step, accumulated by numpy, must equal all three arrays with ==. Guards, from the
    oracle's own counts: every bin holds vehicle-frames, at least two bins hold a (road, frame) at capacity, at least one
    road's peak exceeds thr, no count reaches Nmax. (CPU oracle under torch's own noise, seeds 0 - 2: MAX = 14, thr = 11,
    largest count 12 of 15; vehicle-frames per bin 1 093 / 6 186 / 10 034 - 10 165 / 3 884 - 3 928; (road, frame) pairs at
    capacity per bin 0 / 2 / 115 - 132 / 62 - 71, on 4 - 5 roads.) The identity -episode_return[b] == veh[b].sum() is checked
    on the same run."""
    from oracle import sim
    from tarl_hip import ops, synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import capacity_threshold, link_moments, occupancy_report
    net = synth.torus_network(8, 8)
    N, Nmax, K, T, BIN = net.num_roads, net.Nmax, 2, 300, 100
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    _, action, succ = R.oracle_mode(net, emb)
    pop = R.deliverable_population(net, succ)
    ev, _ = R.embedding_evaluator(net, pop, K, occupancy=True, link_bin_seconds=BIN)
    assert ev.occupancy_block == 64 and ev.occ_ring.shape == (64, N, K) and ev.occ_ring.dtype == torch.float32
    eng = ev.eng
    noise0 = eng.noise_counter + 1
    res = ev.run(T)
    assert not res.domain_exit and res.frames_run == T
    assert res.occupancy_meta["first_bin"] == EPISODE_START // BIN == 215 and res.occupancy_meta["bin_seconds"] == BIN
    assert res.occupancy_frames_per_bin == [60, 100, 100, 40]
    assert res.occupancy["veh"].shape == res.occupancy["full"].shape == (K, 4, N) and res.occupancy["peak"].shape == (K, 1, N)
    assert all(res.occupancy[k].dtype == np.int32 for k in ACC)
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    thr = capacity_threshold(net.x[:, c.MAXN].numpy())
    assert np.array_equal(thr, res.occupancy_meta["thr"]) and np.array_equal(thr, R.threshold(net.x[:, c.MAXN].numpy()))
    for b in range(K):
        x = net.x.clone()
        x[:, :3 * Nmax] = 0
        x[:, c.N] = 0
        ag = pop.clone()
        ag[:, sim.ON_WAY] = 0
        ag[:, sim.DONE] = 0
        counts = np.zeros((T, N, 1), dtype=np.float32)
        ret = 0.0
        for t in range(T):
            g = ops.noise_export(eng.plan, "gumbel", eng.seed, noise0 + t, [b])[0].cpu()
            out = sim.env_step(x, ag, net.edge_index, net.edge_attr, adj, action, float(EPISODE_START + t), Nmax, gumbel=g,
                               congestion_constant=net.congestion_constant)
            counts[t, :, 0] = x[:, c.N].numpy()
            ret += float(out["reward"])
        assert torch.equal(ag, eng.agents[b].cpu()), f"agent table of environment {b}"
        first, veh, full, peak = R.binned(counts, thr, EPISODE_START, 1, BIN)
        per_bin, at_cap = veh[0].sum(axis=1).tolist(), full[0].sum(axis=1).tolist()
        roads = int((full[0].sum(axis=0) > 0).sum())
        print(f"[occupancy replay] environment {b}: MAX {float(net.x[:, c.MAXN].max()):.0f}, thr {int(thr.max())}, vehicle-frames "
              f"per bin {per_bin}, (road, frame) pairs at capacity per bin {at_cap} on {roads} roads, largest count "
              f"{int(peak.max())} of {Nmax}, return {ret:.0f}")
        assert first == 215 and min(per_bin) > 0 and sum(1 for v in at_cap if v > 0) >= 2
        assert bool((peak[0, 0] > thr).any()) and int(peak.max()) < Nmax
        for key, want in zip(ACC, (veh, full, peak)):
            assert np.array_equal(res.occupancy[key][b], want[0]), f"{key} of environment {b}"
        assert -res.episode_return[b] == float(res.occupancy["veh"][b].astype(np.int64).sum()) == -ret      # the identity
    for key in ACC:
        R.assert_stats_equal({k: res.occupancy_stats[key][k] for k in ("sum", "sumsq", "min", "max")}, R.stats(res.occupancy[key]))
        R.assert_moments_close(res.occupancy_stats[key], R.moments(res.occupancy[key]), K)
        R.assert_moments_close(link_moments(R.stats(res.occupancy[key]), K), R.moments(res.occupancy[key]), K)
    rep = occupancy_report(res)
    assert rep["summary"]["identity"]["holds"] and rep["bins"] == ["occ_bin215", "occ_bin216", "occ_bin217", "occ_bin218"]


# ---- 4. the evaluator against frames composed by hand, K N = 63 ----------------------------------------------------------------
T_HAND, K_HAND, SEED_HAND = 130, 3, 11


@functools.lru_cache(maxsize=None)
def _hand_composed():
    """The counts of 130 sampled frames of the embedding head on the 21-road graph, from frame_fused one frame at a time:
    (counts fp32 (T, N, K), rewards (T, K), agents) on the host, computed once and left unchanged."""
    net = R.small_graph()
    eng = R.engine_of(net, R.small_population(net), K_HAND, seed=SEED_HAND)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0)).cuda()
    eng.reset()
    eng.prepare_policy(emb, 1.0)
    cnt = torch.zeros((T_HAND, net.num_roads, K_HAND), dtype=torch.float32, device="cuda")
    rw = torch.zeros((T_HAND, K_HAND), device="cuda")
    for t in range(T_HAND):
        eng.frame_fused(reward=rw[t], counts=cnt[t])
    eng.check_flags()
    return cnt.cpu(), rw.cpu(), eng.agents.cpu(), eng.static_node_features[0, :, 0].cpu().numpy()


@pytest.mark.parametrize("bin_seconds", [3600, 25])
@pytest.mark.parametrize("occupancy_block", [1, 7, 64])
def test_evaluator_equals_frames_composed_by_hand(occupancy_block, bin_seconds):
    """The expected value bins the hand-composed counts with torch. thr comes from the graph's own MAX column; the frames at
    capacity and the peaks are printed (this graph's roads hold up to 40, so few frames are at capacity)."""
    from tarl_hip.engine import EPISODE_START
    cnt, rw, agents, cap = _hand_composed()
    net = R.small_graph()
    N = net.num_roads
    ev, _ = R.embedding_evaluator(net, R.small_population(net), K_HAND, seed=SEED_HAND, occupancy=True,
                                  link_bin_seconds=bin_seconds, occupancy_block=occupancy_block)
    assert ev.occ_ring.shape == (occupancy_block, N, K_HAND)
    res = ev.run(T_HAND, deterministic=False)
    assert not res.domain_exit and torch.equal(ev.eng.agents.cpu(), agents)
    thr = torch.from_numpy(R.threshold(cap).astype(np.int64))
    bins = (EPISODE_START + torch.arange(T_HAND)) // bin_seconds
    first = int(bins[0])
    H = int(bins[-1]) - first + 1
    c = cnt.to(torch.int32).permute(2, 0, 1).contiguous()                     # (K, T, N)
    assert torch.equal(c.to(torch.float32), cnt.permute(2, 0, 1))             # the counts are whole numbers
    veh, full = torch.zeros((K_HAND, H, N), dtype=torch.int32), torch.zeros((K_HAND, H, N), dtype=torch.int32)
    veh.index_add_(1, bins - first, c)
    full.index_add_(1, bins - first, (c >= thr[None, None, :]).to(torch.int32))
    peak = c.max(dim=1, keepdim=True).values
    assert H == (2 if bin_seconds == 3600 else 6) and res.occupancy_meta["first_bin"] == first
    assert res.occupancy_frames_per_bin == torch.bincount(bins - first, minlength=H).tolist()
    assert torch.equal(torch.from_numpy(res.occupancy["veh"]), veh)
    assert torch.equal(torch.from_numpy(res.occupancy["full"]), full)
    assert torch.equal(torch.from_numpy(res.occupancy["peak"]), peak)
    print(f"[hand composed] block {occupancy_block}, bins of {bin_seconds} s: {int(veh.sum())} vehicle-frames, "
          f"{int(full.sum())} (road, frame) pairs at capacity, largest count {int(peak.max())}, thr {thr.tolist()}")
    assert int(veh.sum()) > 0 and int(veh.sum(dim=(0, 1)).min()) >= 0
    assert [-float(x) for x in rw.to(torch.float64).sum(dim=0)] == [float(x) for x in veh.to(torch.int64).sum(dim=(1, 2))]
    assert [-x for x in res.episode_return] == [float(x) for x in veh.to(torch.int64).sum(dim=(1, 2))]
    for key, want in zip(ACC, (veh, full, peak)):
        R.assert_stats_equal({k: res.occupancy_stats[key][k] for k in ("sum", "sumsq", "min", "max")}, R.stats(want.numpy()))


def test_default_block_respects_the_ring_budget(monkeypatch):
    from tarl_hip import evaluator as E
    net = R.small_graph()
    pop = R.small_population(net)
    N = net.num_roads
    assert E.OCCUPANCY_RING_BYTES == 256 << 20
    assert R.embedding_evaluator(net, pop, 2, occupancy=True, poll_frames=500)[0].occupancy_block == 500      # no cap of 127
    assert R.embedding_evaluator(net, pop, 2, occupancy=True, poll_frames=5)[0].occupancy_block == 5
    monkeypatch.setattr(E, "OCCUPANCY_RING_BYTES", 4 * 2 * N * 9 + 3)          # room for 9 frames and a little
    ev = R.embedding_evaluator(net, pop, 2, occupancy=True)[0]
    assert ev.occupancy_block == 9 and ev.occ_ring.numel() * 4 <= E.OCCUPANCY_RING_BYTES
    monkeypatch.setattr(E, "OCCUPANCY_RING_BYTES", 5)                           # not even one frame: at least 1
    assert R.embedding_evaluator(net, pop, 2, occupancy=True)[0].occupancy_block == 1
    with pytest.raises(ValueError, match="occupancy_block"):
        R.embedding_evaluator(net, pop, 2, occupancy=True, occupancy_block=0)
    off = R.embedding_evaluator(net, pop, 2)[0]
    assert not off.occupancy and not hasattr(off, "occ_ring") and not hasattr(off, "occ_thr")      # no buffers without the flag


# ---- 5. accumulating does not perturb the run ------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["embedding", "dijkstra"])
def test_accumulating_does_not_perturb_the_run(head):
    from tarl_hip import synth
    from tarl_hip.evaluator import PER_ENV_KEYS, VecEvaluator
    net = synth.torus_network(8, 8)
    emb = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(0))
    pop = R.deliverable_population(net, R.oracle_mode(net, emb)[2])
    runs = []
    for flag in (False, True):
        if head == "embedding":
            ev, _ = R.embedding_evaluator(net, pop, 4, occupancy=flag, link_counts=True)
        else:
            ev = VecEvaluator(R.engine_of(net, pop, 4), "dijkstra", occupancy=flag, link_counts=True)
        runs.append((ev, ev.run(200)))
    (e0, r0), (e1, r1) = runs
    assert not r0.domain_exit and not r1.domain_exit and r0.frames_run == r1.frames_run == 200
    for k in PER_ENV_KEYS:
        assert getattr(r0, k) == getattr(r1, k), k
    assert r0.aggregate == r1.aggregate and r0.settings == r1.settings
    assert torch.equal(e0.reward[:200], e1.reward[:200]) and float(e0.reward.abs().sum()) > 0
    assert torch.equal(e0.eng.x, e1.eng.x) and torch.equal(e0.eng.agents, e1.eng.agents)
    assert np.array_equal(r0.link_counts, r1.link_counts) and int(r0.link_counts.sum()) > 0
    assert r0.occupancy is None and r0.occupancy_stats is None and r0.occupancy_frames_per_bin is None and r0.occupancy_meta is None
    assert r1.occupancy["veh"].shape == (4, 2, net.num_roads) and r1.occupancy_frames_per_bin == [60, 140]      # 5 h and 6 h
    assert [-x for x in r1.episode_return] == [float(v) for v in r1.occupancy["veh"].astype(np.int64).sum(axis=(1, 2))]
    assert "occupancy" not in r1.to_dict(per_env=True)                 # the tensors never enter the JSON document


# ---- 6. domain exit -----------------------------------------------------------------------------------------------------------------
def test_a_domain_exit_returns_no_occupancy_and_leaves_the_engine_usable():
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    from tarl_hip.evaluator import occupancy_report
    net = synth.torus_network(8, 8)
    pop = synth.population(1024, net.num_roads, seed=7, t1=EPISODE_START + 120)
    ev, _ = R.embedding_evaluator(net, pop, 2, occupancy=True)
    res = ev.run(256)
    assert res.domain_exit and res.aggregate is None
    assert res.occupancy is None and res.occupancy_stats is None and res.occupancy_frames_per_bin is None
    assert res.occupancy_meta is None and not occupancy_report(res)["available"]
    ev.eng.reset()
    ev.eng.check_flags()
    again = ev.run(8, deterministic=False)
    assert not again.domain_exit and again.frames_run == 8
    assert again.occupancy["veh"].shape == (2, 1, net.num_roads) and again.occupancy_meta["first_bin"] == 5
    assert again.occupancy_frames_per_bin == [8]
    assert [-x for x in again.episode_return] == [float(v) for v in again.occupancy["veh"].astype(np.int64).sum(axis=(1, 2))]
    assert 0 <= int(again.occupancy["full"].min()) and int(again.occupancy["full"].max()) <= 8      # only these eight frames


# ---- 7. CLI end to end ----------------------------------------------------------------------------------------------------------
BASE_COLUMNS = ["road", "max_agents", "thr", "veh_seconds_mean", "veh_seconds_sd", "veh_seconds_se", "veh_seconds_ci95_lo",
                "veh_seconds_ci95_hi", "veh_seconds_min", "veh_seconds_max", "occ_5h"]                  # + occ_6h from frame 60 on
TAIL_COLUMNS = ["vc_mean", "peak_mean", "peak_max", "full_frames_mean", "full_frames_min", "full_frames_max", "full_share"]
PAIRED_COLUMNS = ["baseline_veh_seconds_mean", "paired_veh_seconds_mean", "paired_veh_seconds_se", "paired_veh_seconds_ci95_lo",
                  "paired_veh_seconds_ci95_hi", "baseline_full_frames_mean", "paired_full_frames_mean", "paired_full_frames_se",
                  "paired_full_frames_ci95_lo", "paired_full_frames_ci95_hi"]


def test_cli_occupancy_end_to_end(tmp_path, capsys):
    main = importlib.import_module("main").main
    scenario = "synthetic-1024-300"
    on = tmp_path / "on"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--eval-occupancy",
          "--eval-link-counts", "--eval-baseline", "dijkstra", "--steps", "120", "--output-dir", str(on)])
    text = capsys.readouterr().out
    assert "=== Occupancy ===" in text and text.index("=== Occupancy ===") > text.index("=== Link counts ===")
    block = text[text.index("=== Occupancy ==="):]
    assert "vehicle-hours:" in block and "policy - dijkstra:" in block and "v/c occ_5h:" in block and "v/c occ_6h:" in block
    assert "in every environment: yes" in block and "roads with the most frames at capacity" in block
    assert len([line for line in block.splitlines() if line.startswith("  road")]) == 10
    roads = len(list(csv.DictReader(open(on / "msa_expected_flows.csv"))))
    doc = json.load(open(on / "eval_envs.json"))
    assert not doc["mode"]["domain_exit"], "the synthetic scenario left the domain under MODE"
    rows = list(csv.DictReader(open(on / "eval_occupancy.csv")))
    assert list(rows[0]) == BASE_COLUMNS + ["occ_6h"] + TAIL_COLUMNS + PAIRED_COLUMNS
    assert len(rows) == roads and [int(r["road"]) for r in rows] == list(range(roads))
    assert sum(float(r["veh_seconds_mean"]) for r in rows) > 0
    oc = doc["occupancy"]
    assert oc["available"] and "rows" not in oc and oc["bins"] == ["occ_5h", "occ_6h"] and oc["columns"] == list(rows[0])
    s = oc["summary"]
    assert s["envs"] == 4 and s["roads"] == roads and s["frames_run"] == 120 and s["frames_per_bin"] == [60, 60]
    assert s["identity"]["holds"] and s["vehicle_hours"]["n"] == 4 and len(s["vc_mean_per_bin"]) == 2
    assert s["paired"]["available"] and s["paired"]["baseline_head"] == "dijkstra"
    assert len(json.dumps(oc)) < 20000                                   # the summary only, never the K x H x N tensors
    assert "occupancy" not in doc["mode"] and "occupancy" not in doc["baseline"] and doc["link_counts"]["available"]
    vh = sum(float(r["veh_seconds_mean"]) for r in rows) / 3600.0
    assert abs(vh - s["vehicle_hours"]["mean"]) <= 1e-9 * max(1.0, vh)
    # the router alone
    dj = tmp_path / "dj"
    main(["--algo", "dijkstra", "--mode", "eval", "--scenario", scenario, "--dijkstra-envs", "4", "--eval-occupancy",
          "--steps", "60", "--start-end-time", "21540", "21600", "--output-dir", str(dj)])
    out = capsys.readouterr().out
    assert "=== Occupancy ===" in out and "Link counts" not in out
    rows = list(csv.DictReader(open(dj / "dijkstra_occupancy.csv")))
    assert len(rows) == roads and list(rows[0]) == BASE_COLUMNS + TAIL_COLUMNS
    assert json.load(open(dj / "dijkstra_envs.json"))["occupancy"]["summary"]["envs"] == 4
    # without the flag: none of it
    off = tmp_path / "off"
    main(["--algo", "mpnn", "--mode", "eval", "--scenario", scenario, "--eval-envs", "4", "--steps", "40",
          "--output-dir", str(off)])
    assert "Occupancy" not in capsys.readouterr().out
    assert not (off / "eval_occupancy.csv").exists() and set(json.load(open(off / "eval_envs.json"))) == {"mode"}
