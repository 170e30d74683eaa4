"""CPU: per-turn movement counts — the numpy restatement by hand, its crafted cases and defects, the rule against the oracle's
own choice (Direction's Gumbel race) on the 8 x 8 torus under random actions, the reports on a seeded result against a
recorded snapshot, the flags, and the host-side checks of the entry point and its wrapper."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import link_counts_restatement as LR
import turn_counts_restatement as R
from fake_plan import fake_plan

CASES = R.crafted_cases()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turn_reports_snapshot.json")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_accumulate_restatement_by_hand():
    """Three roads, edges in the order (1 -> 2), (0 -> 1), (0 -> 2), (2 -> 0): road 0's out-list is [edge 1, edge 2]. One
    environment, frames at the clocks 9, 10 with bins of 10 s. Frame 0 (bin 0): road 0 popped, empty before (after a reset):
    lost. Frame 1 (bin 1): road 0 popped, held 2 after frame 0, rank 1 with bit 7 set -> edge 2; road 1 popped, held 1, code
    0x7F -> unresolved; road 2 not popped (byte 0x02)."""
    ei = np.array([[1, 0, 0, 2], [2, 1, 2, 0]])
    popped = np.array([[[1, 0, 0]], [[3, 0xFF, 0x02]]], dtype=np.uint8)
    sel8 = np.array([[[0], [0], [0]], [[0x81], [0x7F], [0]]], dtype=np.uint8)
    counts = np.array([[[2], [1], [5]], [[0], [0], [0]]], dtype=np.float32)
    turns, lost, unres = np.zeros((1, 2, 4), np.int32), np.zeros((1, 2, 3), np.int32), np.zeros(1, np.int32)
    R.accumulate(ei, 3, popped, sel8, counts, None, turns, lost, unres, 9, 1, 10, 0)
    assert turns.tolist() == [[[0, 0, 0, 0], [0, 0, 1, 0]]] and lost.tolist() == [[[1, 0, 0], [0, 0, 0]]] and unres.tolist() == [1]
    out_ptr, out_eid = R.csr(ei, 3)
    assert out_ptr.tolist() == [0, 2, 3, 4] and out_eid.tolist() == [1, 2, 0, 3]


def test_crafted_cases_cover_what_the_issue_lists():
    names = {c["name"] for c in CASES}
    for K in (1, 3, 64, 65):
        for N in (1, 5, 64, 67):
            assert f"K{K}-N{N}" in names
    by = {c["name"]: c for c in CASES}
    assert len(by["one-frame"]["calls"]) == 1 and by["one-frame"]["calls"][0]["popped"].shape[0] == 1
    c = by["three-bins-one-call"]
    assert len(c["calls"]) == 1 and c["H"] == 5
    turns, lost, _ = R.run_case(c)
    assert all(int(turns[:, h].sum()) + int(lost[:, h].sum()) > 0 for h in (1, 2, 3))      # one call, three bins
    assert by["first-call-with-prev"]["calls"][0]["prev"] is not None and by["K3-N5"]["calls"][0]["prev"] is None
    assert by["K3-N5"]["calls"][1]["prev"] is not None and len(by["K3-N5"]["calls"]) == 3
    deg = np.bincount(by["K3-N67"]["edge_index"][0], minlength=67)
    assert {0, 1, 5, 126} <= set(deg.tolist()) and deg[3] == 126
    for c in CASES:
        if c["N"] > 1:
            assert not np.array_equal(R.csr(c["edge_index"], c["N"])[1], np.arange(c["E"])), c["name"]      # eid != CSR position
    seen_p, seen_c, seen_s = set(), set(), set()
    rank125 = False
    for c in CASES:
        for call in c["calls"]:
            seen_p |= set(np.unique(call["popped"]).tolist())
            seen_s |= set(np.unique(call["sel8"]).tolist())
            v = call["counts"]
            seen_c |= {"nan" if np.isnan(x) else ("-0" if x == 0 and np.signbit(x) else float(x)) for x in np.unique(v)}
            seen_c |= {"-0"} if bool((np.signbit(v) & (v == 0)).any()) else set()
            if c["N"] >= 5:
                rank125 |= bool(((call["sel8"][:, 3, :] & 0x7F) == 125).any())
    assert {0x02, 0xFE, 0x03, 0xFF, 0, 1} <= seen_p and {"nan", "-0", 0.0, 1.0, 14.0} <= seen_c
    assert {0x7F, 0x7E, 0xFF, 0xFE} <= seen_s and any(s & 0x80 and (s & 0x7F) < 0x7E for s in seen_s) and rank125
    # the two-call case: the second call's frame 0 holds one genuine movement and one phantom pop of environment 1
    c = by["two-calls-prev-decides"]
    turns, lost, unres = R.run_case(c)
    e = R.csr(c["edge_index"], 5)[1][4]                                  # road 0's out-edge of rank 4
    assert turns[1, :, e].sum() == 1 and lost[1, :, 1].sum() == 1 and lost[1, :, 0].sum() == 0
    assert turns[1].sum() - 1 == sum(int(turns[1, :, x].sum()) for x in range(c["E"]) if c["edge_index"][0][x] not in (0, 1))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_popped_bit_lands_in_exactly_one_table(case):
    turns, lost, unres = R.run_case(case)
    assert int(turns.sum()) + int(lost.sum()) + int(unres.sum()) == R.popped_bits(case) > 0
    assert not turns[:, 0].any() and not turns[:, -1].any() and not lost[:, 0].any() and not lost[:, -1].any()
    if case["name"] not in ("one-frame", "two-calls-prev-decides") and case["K"] * case["N"] >= 15:
        assert int(turns.sum()) > 0 and int(lost.sum()) > 0 and int(unres.sum()) > 0, case["name"]


NOTICED_BY = {"ignore_n_pre": "K3-N5", "same_frame_counts": "two-calls-prev-decides", "sel_of_next_frame": "K3-N67",
              "csr_position": "K3-N5", "no_mask_7f": "K3-N5", "bin_of_frame_end": "three-bins-one-call",
              "popped_untransposed": "K3-N5"}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_noticed_by_the_crafted_cases(defect):
    assert set(NOTICED_BY) == set(R.DEFECTS)
    by = {c["name"]: c for c in CASES}
    true, bad = R.run_case(by[NOTICED_BY[defect]]), R.run_case(by[NOTICED_BY[defect]], defect=defect)
    assert any(not np.array_equal(a, b) for a, b in zip(true, bad)), defect
    changed = [c["name"] for c in CASES
               if any(not np.array_equal(a, b) for a, b in zip(R.run_case(c), R.run_case(c, defect=defect)))]
    print(f"[defect {defect}] changes {len(changed)} of {len(CASES)} cases")
    assert len(changed) >= 1


# ---- the rule against the oracle's own choice ----------------------------------------------------------------------------------------
def test_rule_equals_directions_choice_on_the_torus_under_random_actions():
    """8 x 8 torus (256 roads, 1 024 edges), the population of tests/link_counts_restatement.py, one uniformly random out-edge
    per road per frame, 300 frames from 21 540 s, torch's own noise (seed 0), bins of 100 s. The oracle truth is the in-edge
    Direction's Gumbel race chose for every road with P > 0 whose agent id is not 0; the rule reads only the popped mask, the
    rank byte and the counts of the frame before. (Recorded with seeds 0 - 2: 123 - 127 phantom pops, 438 - 492 of 1 024 edges
    used, 141 - 171 roads that use at least two out-edges, largest queue 3.)"""
    from tarl_hip import synth
    from tarl_hip.engine import EPISODE_START
    net = synth.torus_network(8, 8)
    N, E, T, BIN = net.num_roads, net.edge_index.size(1), 300, 100
    emb = torch.randn(N, generator=torch.Generator().manual_seed(0))
    pop = LR.deliverable_population(net, LR.oracle_mode(net, emb)[2])
    choices = R.random_choices(net, 0, T)
    gen = torch.Generator().manual_seed(1000)
    o = R.oracle_replay(net, pop, T, EPISODE_START, lambda f: choices[f], lambda f: dict(uniform=torch.rand(E, generator=gen)))
    ei = net.edge_index.numpy()
    first, turns, lost, unres = R.binned(ei, N, o["popped"], o["sel8"], o["counts"], EPISODE_START, 1, BIN)
    want = R.moved_binned(o["moved"], EPISODE_START, BIN)
    assert first == 215 and turns.shape == (1, 4, E)
    assert np.array_equal(turns[0], want) and int(unres[0]) == 0                     # every frame's bin, every edge
    # frame by frame as well: one frame per bin
    _, per_frame, lost_f, _ = R.binned(ei, N, o["popped"], o["sel8"], o["counts"], 0, 1, 1)
    assert np.array_equal(per_frame[0].astype(bool), o["moved"])
    phantom = int(lost.sum())
    used = want.sum(axis=0) > 0
    two = int((np.bincount(ei[0], weights=used, minlength=N) >= 2).sum())
    print(f"[oracle torus random] moved per bin {want.sum(axis=1).tolist()}, accepted {int(o['accepted'].sum())}, phantom pops "
          f"{phantom}, edges used {int(used.sum())}, roads using two out-edges {two}, largest count {o['max_count']:.0f}")
    assert phantom >= 1 and two >= 100 and o["max_count"] < net.Nmax
    assert phantom == o["unqueued"] == int(o["accepted"].sum()) - int(o["moved"].sum())
    # the naive rule (popped and SELECTED_ROAD points there) books the phantom pops as movements
    _, naive, naive_lost, _ = R.binned(ei, N, o["popped"], o["sel8"], o["counts"], EPISODE_START, 1, BIN, defect="ignore_n_pre")
    assert not np.array_equal(naive[0], want) and int(naive.sum()) == int(want.sum()) + phantom and int(naive_lost.sum()) == 0


# ---- the reports ----------------------------------------------------------------------------------------------------------------------
N_R, E_R, H_R = 5, 9, 2
EDGES = np.array([[0, 0, 1, 2, 2, 2, 3, 4, 4], [1, 2, 2, 0, 3, 4, 4, 0, 1]])


def _result(K, seed, head, prob=True, empty=False):
    """An EvalResult as VecEvaluator(turns=True).run() leaves it, seeded; edge 4 (2 -> 3) and so road 3 are never used."""
    from tarl_hip.evaluator import EvalResult, link_moments
    rng = np.random.default_rng(seed)
    res = EvalResult(envs=K, head=head, deterministic=True, frames_run=100, settings=dict(seed=3, env_base=0))
    res.turn_counts = rng.integers(0, 30, size=(K, H_R, E_R)).astype(np.int32) * (0 if empty else 1)
    res.turn_counts[:, :, 4] = 0
    res.turn_counts[:, :, 6] = 0
    res.turn_lost = (rng.random((K, H_R, N_R)) < 0.3).astype(np.int32) * rng.integers(1, 3, size=(K, H_R, N_R)).astype(np.int32)
    res.turn_lost[:, :, 1] = 0
    res.turn_stats = {"turns": link_moments(LR.stats(res.turn_counts), K), "lost": link_moments(LR.stats(res.turn_lost), K)}
    lost = res.turn_lost.astype(np.int64).sum(axis=(1, 2))
    queued = rng.integers(0, 20, size=K)
    p = np.array([0.25, 0.75, 1.0, 0.5, 0.25, 0.25, 1.0, 0.125, 0.875]) if prob and head == "embedding" else None
    res.turn_meta = dict(first_bin=5, bin_seconds=3600, edge_index=EDGES.copy(), on_way=[int(x) for x in queued + lost],
                         queued=[int(x) for x in queued], policy_prob=p)
    return res


def _table(rows):
    keys = list(rows[0]) if rows else []
    assert all(list(r) == keys for r in rows)
    return {"keys": keys, "values": [list(r.values()) for r in rows]}


def build_snapshot():
    from tarl_hip import evaluator as E
    out = {}
    for K in (1, 4):
        res, base = _result(K, 30 + K, "embedding"), _result(K, 40 + K, "dijkstra")
        lacking = E.EvalResult(envs=K, head="dijkstra", deterministic=True, frames_run=100, settings=dict(seed=3, env_base=0))
        gone = E.EvalResult(envs=K, head="embedding", deterministic=True, frames_run=64, domain_exit=True,
                            domain_exit_frames=(0, 64), settings=dict(seed=3, env_base=0))
        reports = {"alone": E.turn_report(res), "router-alone": E.turn_report(base), "baseline": E.turn_report(res, baseline=base),
                   "baseline-lacking": E.turn_report(res, baseline=lacking), "domain-exit": E.turn_report(gone),
                   "nothing-moved": E.turn_report(_result(K, 50 + K, "embedding", empty=True))}
        for name, rep in reports.items():
            slim = {k: v for k, v in rep.items() if k not in ("rows", "lost_rows")}
            assert json.dumps(E.turn_summary(rep), allow_nan=False) == json.dumps(slim), name
            rep, text = dict(rep), E.turn_lines(rep)
            for table in ("rows", "lost_rows"):
                if table in rep:
                    rep[table] = _table(rep[table])
            out[f"K{K}/{name}"] = {"report": rep, "lines": text}
    return out


def test_the_turn_reports_equal_the_recorded_snapshot(monkeypatch):
    """tests/golden/turn_reports_snapshot.json was recorded by :func:`build_snapshot` (both sides compared as JSON text: every
    float64 bit and the order of the keys, the columns of the CSV files)."""
    from tarl_hip import eval_reports, evaluator as E
    monkeypatch.setattr(eval_reports, "_paired_moments", lambda a, b, K: E.link_moments(LR.stats(a, b), K))
    got = build_snapshot()
    with open(GOLDEN) as f:
        snapshot = json.load(f)
    assert sorted(got) == sorted(snapshot) and len(got) == 12
    for name, want in snapshot.items():
        for part in want:
            assert json.dumps(got[name][part]) == json.dumps(want[part]), (name, part)


def test_turn_report_against_numpy(monkeypatch):
    from tarl_hip import eval_reports, evaluator as E
    monkeypatch.setattr(eval_reports, "_paired_moments", lambda a, b, K: E.link_moments(LR.stats(a, b), K))
    K = 4
    res, base = _result(K, 34, "embedding"), _result(K, 44, "dijkstra")
    rep = E.turn_report(res, baseline=base)
    tot = res.turn_counts.astype(np.float64).sum(axis=1)                 # (K, E)
    assert [r["edge"] for r in rep["rows"]] == list(range(E_R)) and len(rep["rows"]) == E_R
    assert rep["columns"][:10] == ["edge", "from_road", "to_road", "mean", "sd", "se", "ci95_lo", "ci95_hi", "min", "max"]
    assert rep["columns"][10:] == ["turns_5h", "turns_6h", "share", "policy_prob", "share_minus_prob", "baseline_mean",
                                   "paired_diff_mean", "paired_diff_se", "paired_diff_ci95_lo", "paired_diff_ci95_hi"]
    m = LR.moments(res.turn_counts)
    d = LR.moments(res.turn_counts, base.turn_counts)
    for e, r in enumerate(rep["rows"]):
        assert (r["from_road"], r["to_road"]) == (EDGES[0, e], EDGES[1, e])
        assert r["mean"] == tot[:, e].mean() and np.isclose(r["se"], m["se"][H_R, e], rtol=1e-12, atol=1e-12)
        assert r["min"] == tot[:, e].min() and r["max"] == tot[:, e].max()
        assert r["turns_5h"] == res.turn_counts[:, 0, e].mean() and r["turns_6h"] == res.turn_counts[:, 1, e].mean()
        out_of = tot[:, EDGES[0] == EDGES[0, e]].sum()
        assert r["share"] == (tot[:, e].sum() / out_of if out_of > 0 else None)
        assert r["paired_diff_mean"] == d["mean"][H_R, e] and np.isclose(r["paired_diff_se"], d["se"][H_R, e], rtol=1e-12)
    assert rep["rows"][6]["share"] is None and rep["rows"][6]["share_minus_prob"] is None      # nothing left road 3
    assert np.isclose(sum(r["share"] for r in rep["rows"] if r["from_road"] == 2), 1.0)
    s = rep["summary"]
    assert s["movements_per_env"] == [int(x) for x in tot.sum(axis=1)] and s["turns_used"] == 7 and s["edges"] == E_R
    assert s["lost_per_env"] == [int(x) for x in res.turn_lost.sum(axis=(1, 2))] and s["identity"]["holds"]
    assert [r["road"] for r in rep["lost_rows"]] == [int(n) for n in np.nonzero(res.turn_lost.sum(axis=(0, 1)))[0]]
    assert 1 not in [r["road"] for r in rep["lost_rows"]] and s["roads_with_a_loss"] == len(rep["lost_rows"])
    assert s["paired"]["available"] and s["paired"]["baseline_head"] == "dijkstra"
    assert "policy_prob" not in E.turn_report(base)["columns"]                       # the router has no policy probability
    text = "\n".join(E.turn_lines(rep))
    assert "agents lost (Q24)" in text and "busiest turns" in text and "policy - dijkstra" in text and "yes" in text
    broken = _result(K, 34, "embedding")
    broken.turn_meta["on_way"][0] += 1
    assert not E.turn_report(broken)["summary"]["identity"]["holds"] and "NO" in "\n".join(E.turn_lines(E.turn_report(broken)))
    other = _result(K, 44, "dijkstra")
    other.turn_meta["edge_index"] = EDGES[:, ::-1].copy()
    with pytest.raises(ValueError, match="same frames, bins and edges"):
        E.turn_report(res, baseline=other)


def test_without_the_flag_nothing_changes():
    from tarl_hip import evaluator as E
    res = E.EvalResult(envs=2, head="embedding", deterministic=True, frames_run=10, settings=dict(seed=3, env_base=0))
    assert res.turn_counts is None and res.turn_lost is None and res.turn_stats is None and res.turn_meta is None
    assert set(res.to_dict(per_env=True)) == {"envs", "head", "deterministic", "frames_run", "domain_exit", "domain_exit_frames",
                                              "aggregate", "envs_without_arrival", "settings", "computation_time_ms", "per_env"}
    on = _result(2, 1, "embedding")
    assert not any(k.startswith("turn") for k in on.to_dict(per_env=True))      # the tables never enter the JSON document
    rep = E.turn_report(res)
    assert rep == {"available": False, "reason": "the run did not count turns"}
    assert E.turn_lines(rep) == ["not available: the run did not count turns"] and E.turn_summary(rep) == rep


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from src.runner import RunnerArgs
    base = dict(algo="mpnn", scenario="synthetic-1024-1024", mode="eval")
    base.update(kw)
    return RunnerArgs(**base)


def test_flag_defaults_and_refusals():
    main = importlib.import_module("main")
    assert main.build_parser().parse_args([]).eval_turns is False
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--eval-envs", "4", "--eval-turns", "--eval-link-bin", "900"])
    from src.runner import RunnerArgs
    a = RunnerArgs(**vars(ns))
    assert a.eval_turns and a.eval_link_bin == 900 and not a.eval_link_counts and not a.eval_occupancy
    assert _args().eval_turns is False
    assert _args(eval_envs=4, eval_turns=True).eval_turns
    assert _args(algo="dijkstra", dijkstra_envs=4, eval_turns=True).eval_turns
    with pytest.raises(ValueError, match="eval_turns"):
        _args(eval_turns=True)
    with pytest.raises(ValueError, match="eval_turns"):
        _args(algo="dijkstra", eval_turns=True)
    with pytest.raises(ValueError, match="eval_link_bin"):
        _args(eval_envs=4, eval_turns=True, eval_link_bin=0)


# ---- the entry point and its wrapper validate on the host ------------------------------------------------------------------------
def test_entry_point_validation():
    import ctypes
    from tarl_hip import lib, ops
    assert "tarl_turn_counts_accumulate" in lib.SIGNATURES
    L = lib.load()
    null = None
    buf = torch.zeros(64)
    p = buf.data_ptr()      # sizes and bins are checked before anything is launched: the address is never dereferenced
    plan = fake_plan(5, 9)
    pl = ctypes.addressof(plan)
    acc = L.tarl_turn_counts_accumulate
    #    plan popped sel8 counts prev F  K  t0 step bin first H  turns lost unresolved stream
    for i in (0, 1, 2, 3, 12, 13, 14):
        a = [pl, p, p, p, null, 1, 1, 0, 1, 10, 0, 1, p, p, p, null]
        a[i] = null
        assert acc(*a) == -1 and b"null" in L.tarl_last_error(), i
    tail = (p, p, p, null)
    assert acc(pl, p, p, p, null, 0, 1, 0, 1, 10, 0, 1, *tail) == -1 and b"F must be" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, ops.TURN_COUNTS_MAX_FRAMES + 1, 1, 0, 0, 10, 0, 1, *tail) == -1 and b"F must be" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 0, 0, 1, 10, 0, 1, *tail) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 1, 0, 1, 10, 0, 0, *tail) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 1 << 40, 0, 1, 10, 0, 1, *tail) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 1 << 20, 0, 1, 10, 0, 1 << 20, *tail) == -1 and b"bad sizes" in L.tarl_last_error()
    assert acc(ctypes.addressof(fake_plan(5, 0)), p, p, p, null, 1, 1, 0, 1, 10, 0, 1, *tail) == -1 and b"no edge" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 1, 0, 1, 0, 0, 1, *tail) == -1 and b"bin_seconds" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 1, 1, 0, -1, 10, 0, 1, *tail) == -1 and b"clock" in L.tarl_last_error()
    assert acc(pl, p, p, p, null, 2, 1, 9, 1, 10, 0, 1, *tail) == -1 and b"bin >= H" in L.tarl_last_error()      # frame 1 in bin 1
    assert acc(pl, p, p, p, null, 2, 1, 9, 1, 10, 1, 1, *tail) == -1 and b"below first_bin" in L.tarl_last_error()


class _Plan:
    num_nodes, num_edges, handle = 3, 4, None


def test_ops_wrapper_refuses_bad_arguments():
    from tarl_hip import lib, ops
    F, N, K, H, E = 4, 3, 2, 2, 4
    popped, sel8, counts = torch.zeros((F, K, N), dtype=torch.uint8), torch.zeros((F, N, K), dtype=torch.uint8), torch.zeros((F, N, K))
    turns, lost = torch.zeros((K, H, E), dtype=torch.int32), torch.zeros((K, H, N), dtype=torch.int32)
    unres = torch.zeros(K, dtype=torch.int32)
    ok = dict(t0=100, timestep=1, bin_seconds=3600, first_bin=0)
    call = lambda *a, **kw: ops.turn_counts_accumulate(_Plan, *a, **{**ok, **kw})      # noqa: E731
    with pytest.raises(lib.TarlError, match="GPU"):                      # everything else in order: a host tensor is refused
        call(popped, sel8, counts, turns, lost, unres)
    with pytest.raises(TypeError, match="popped"):
        call(popped.to(torch.int32), sel8, counts, turns, lost, unres)
    with pytest.raises(TypeError, match="counts"):
        call(popped, sel8, counts.to(torch.float64), turns, lost, unres)
    with pytest.raises(ValueError, match="sel8"):                        # env-minor: (F, N, K), not (F, K, N)
        call(popped, sel8.transpose(1, 2).contiguous(), counts, turns, lost, unres)
    with pytest.raises(ValueError, match="popped"):                      # not this plan's roads
        call(popped[:, :, :2].contiguous(), sel8, counts, turns, lost, unres)
    with pytest.raises(ValueError, match="turns"):                       # one column per EDGE
        call(popped, sel8, counts, lost.clone(), lost, unres)
    with pytest.raises(ValueError, match="lost"):
        call(popped, sel8, counts, turns, turns.clone(), unres)
    with pytest.raises(ValueError, match="unresolved"):
        call(popped, sel8, counts, turns, lost, unres[:1])
    with pytest.raises(ValueError, match="prev_counts"):
        call(popped, sel8, counts, turns, lost, unres, prev_counts=torch.zeros((K, N)))
    with pytest.raises(ValueError, match="contiguous"):
        call(popped, sel8, counts.transpose(1, 2).contiguous().transpose(1, 2), turns, lost, unres)
    with pytest.raises(ValueError, match="bin out of range"):           # frames 2, 3 reach bin 2 of the 2 stored
        call(popped, sel8, counts, turns, lost, unres, t0=7198)
    with pytest.raises(ValueError, match="frames"):
        call(popped, sel8, counts, turns, lost, unres, frames=5)
