"""GPU: the shortest-path family on the irregular road graphs of tests/irregular_graphs.py — k_apsp, the travel-time,
select and assignment kernels of csrc/routing.hip, the three tree kernels of csrc/sp_trees.h, csrc/dest_trees.hip's select,
csrc/baseline.hip and the per-edge logits of csrc/prior.hip. MIXED (80 roads, degrees 0 - 9) and HUB126 (280 roads, one hub
with 126 in- and out-edges): edge lists in no order (``out_eid`` and ``in_eid`` are no identity), lists far longer than the
four of a torus, dead ends and roads nobody can enter (pairs without a path), ties that no lattice symmetry makes. The
references are real networkx (tests/golden/routing_irregular.npz), the oracle's heap replay and tree_restatement's Dijkstra
and tie rule, all from tests/sp_cases.py, computed once; tests/test_sp_irregular_host.py shows on the CPU that a kernel
wrong in any of these respects fails the checks used here. Everything is integer- or bit-exact but the fp64 atomics of the
assignment (rtol 1e-9, as tests/test_gpu_routing.py)."""
import pytest
import torch

import irregular_graphs as ig
import sp_cases as S
from tree_restatement import check_table, check_tree

pytestmark = pytest.mark.gpu

CASES = [(n, t) for n in S.NAMES for t in S.WEIGHTS]
APSP_LDS_WAVES, APSP_SCRATCH_WAVES, SPT_MAX_WG = 65536, 4096, 1024       # the launch caps of routing.hip and sp_trees.h


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def _plan(ops, c):
    plan = ops.Plan(c.ei, c.N)
    assert not plan.src_sorted and plan.max_out == S.MAX_DEGREE[c.name] and plan.max_in == S.MAX_DEGREE[c.name]
    return plan


# ---- 1. all pairs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lds", "scratch", "f64"])
@pytest.mark.parametrize("name,tag", CASES)
def test_all_pairs_against_networkx_and_the_oracle(ops, monkeypatch, name, tag, variant):
    """tarl_apsp with its per-wave state in LDS and in the global scratch row, and tarl_apsp_f64 (double weights, the
    entry run_msa reaches): next hops equal to real networkx's and the oracle's, distances to the oracle's fp32 table bit
    for bit, -1 / +inf on the pairs no path joins."""
    from tarl_hip import lib
    if variant == "scratch":
        monkeypatch.setenv("TARL_APSP_LDS_MAX", "0")
    c = S.case(name)
    plan = _plan(ops, c)
    assert (int(lib.load().tarl_apsp_scratch_bytes(plan.handle, 1)) > 0) == (variant == "scratch")
    w = c.w[tag].cuda()
    nh, dist = ops.all_pairs_shortest_paths(plan, w.double() if variant == "f64" else w, want_dist=True)
    assert nh.shape == (1, c.N, c.N) and nh.dtype == torch.int64
    S.check_all_pairs(name, tag, nh[0].cpu(), dist[0].cpu())


# ---- 2. the job loop of k_apsp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,B,cap", [("scratch", 52, APSP_SCRATCH_WAVES), ("lds", 820, APSP_LDS_WAVES)])
def test_all_pairs_job_loop_wraps(ops, monkeypatch, variant, B, cap):
    """More (weight set, source) jobs than the launch has waves: a wave re-initialises its state and takes a second job.
    The weight sets cycle through four vectors, so every table must equal the first one of its vector."""
    from oracle import routing
    if variant == "scratch":
        monkeypatch.setenv("TARL_APSP_LDS_MAX", "0")
    c = S.case("MIXED")
    N = c.N
    assert B * N > cap and (B - 1) * N < cap + N * 4 and B % 4 == 0        # the loop wraps, and only just
    vectors = [c.w["ff"], c.w["r5"], S.random_weights(c.E, 31), S.random_weights(c.E, 32)]
    w = torch.stack([vectors[b % 4] for b in range(B)]).cuda()
    nh, dist = ops.all_pairs_shortest_paths(_plan(ops, c), w, want_dist=True)
    assert nh.shape == (B, N, N)
    assert bool((nh.view(B // 4, 4, N, N) == nh[:4]).all()), "a later table differs from the first of its vector"
    assert bool((dist.view(B // 4, 4, N, N).view(torch.int32) == dist[:4].view(torch.int32)).all())
    assert not torch.equal(nh[0], nh[1]) and not torch.equal(nh[2], nh[3])
    for k, v in enumerate(vectors):
        nh_o, dist_o = S.all_pairs("MIXED", ("ff", "r5")[k]) if k < 2 else routing.all_pairs(c.ei, v, N)
        for b in (k, B - 4 + k):
            assert torch.equal(nh[b].cpu(), nh_o) and torch.equal(dist[b].cpu(), dist_o), f"table {b}"


# ---- 3. the tree core ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", CASES)
def test_trees_from_and_towards_every_road(ops, name, tag):
    """tarl_dest_trees, tarl_sssp_f64 and tarl_prior_dest_table with all N roots: distances and links against the heap
    Dijkstra and the tie rule, the tables walked, the mirror image on the transposed graph, and the all-pairs table
    wherever the first hop is not tied."""
    c = S.case(name)
    N, w = c.N, c.w[tag]
    plan = _plan(ops, c)
    roots = torch.arange(N, dtype=torch.int64)
    nh, dist = ops.destination_trees(plan, w.cuda(), roots.cuda(), want_dist=True)
    S.check_trees(name, tag, True, dist.cpu(), nh.cpu())
    check_table(c.ei, w, N, roots, dist.cpu(), nh.cpu(), walks=4)
    dist_f, pred = ops.shortest_path_trees(plan, w.double().cuda(), roots.cuda())
    S.check_trees(name, tag, False, dist_f.cpu(), pred.cpu())
    check_tree(c.ei, w.double(), N, roots, dist_f.cpu(), pred.cpu())
    # the prior head's table: the fp32 rounding, candidate-major, +inf where the reverse tree does not reach
    table = ops.prior_dest_table(plan, w.cuda(), roots.cuda())
    d_ref = S.trees(name, tag, True)[0]
    assert table.shape == (N, N) and torch.equal(table.t().cpu(), d_ref.to(torch.float32))
    assert int(torch.isinf(table).sum()) == S.UNREACHABLE[name]
    assert int(torch.isinf(table).sum(0).max()) == N - 1 and int(torch.isinf(table).sum(1).max()) == N - 1
    # (the column of a road nobody can enter, the row of a dead end)
    # mirror image: the same trees with the two adjacencies swapped
    plan_t = ops.Plan(c.ei.flip(0).contiguous(), N)
    nh_t, dist_t = ops.destination_trees(plan_t, w.cuda(), roots.cuda(), want_dist=True)
    dist_ft, pred_t = ops.shortest_path_trees(plan_t, w.double().cuda(), roots.cuda())
    at_root = torch.eye(N, dtype=torch.bool, device="cuda")
    assert torch.equal(dist_t, dist_f) and torch.equal(dist_ft, dist)
    assert torch.equal(nh_t[~at_root], pred[~at_root]) and torch.equal(pred_t[~at_root], nh[~at_root])
    assert bool((pred[at_root] == -1).all()) and torch.equal(nh[at_root], roots.to(torch.int32).cuda())
    # against k_apsp's table: the distances everywhere, the next hops wherever u has at most one tight out-edge towards d
    nh_ap, d_ap = ops.all_pairs_shortest_paths(plan, w.cuda(), want_dist=True)
    assert torch.equal(dist.t().to(torch.float32), d_ap[0])
    src, dst = c.ei[0].cuda(), c.ei[1].cuda()
    tight = (w.cuda().double()[None, :] + dist[:, dst]) == dist[:, src]                  # [d][e]; inf == inf counts
    tight &= torch.isfinite(dist[:, src])
    ntight = torch.zeros((N, N), dtype=torch.int32, device="cuda").index_add_(1, src, tight.to(torch.int32))
    untied = (ntight <= 1).t()                                                           # [u][d]
    assert torch.equal(nh.t().to(torch.int64)[untied], nh_ap[0][untied])
    assert int((nh_ap[0][untied] == -1).sum()) == S.UNREACHABLE[name]                    # unreachable entries included
    print(f"\ntrees {name}/{tag}: {int((~untied).sum())} of {N * N} pairs with a tied first hop")
    if tag == "ff":
        assert int((~untied).sum()) == 0


# ---- 4. batched trees past the workgroup cap -------------------------------------------------------------------------------
def test_batched_trees_stride_over_their_scratch_rows(ops):
    c = S.case("MIXED")
    N, B = c.N, 16
    assert B * N > SPT_MAX_WG and (N + 31) // 32 == 3 and N % 32 != 0
    plan = _plan(ops, c)
    sets = [c.w["ff"], c.w["r5"]] + [S.random_weights(c.E, 40 + k) for k in range(B - 2)]
    sets[3], sets[9] = torch.round(sets[3]), torch.round(sets[9] / 4) * 4 + 1            # tied sets among the untied
    w = torch.stack(sets).cuda()
    dests = torch.arange(N, dtype=torch.int64, device="cuda")
    nh = ops.destination_trees_batched(plan, w, dests)
    assert nh.shape == (B, N, N)
    for b in range(B):
        assert torch.equal(nh[b], ops.destination_trees(plan, w[b].contiguous(), dests)[0]), f"weight set {b}"
    S.check_trees("MIXED", "ff", True, S.trees("MIXED", "ff", True)[0], nh[0].cpu())
    S.check_trees("MIXED", "r5", True, S.trees("MIXED", "r5", True)[0], nh[1].cpu())
    assert not torch.equal(nh[0], nh[2])


# ---- loaded states ---------------------------------------------------------------------------------------------------------
def _loaded(c, B, seed, spare=4):
    """B random mid-simulation states (ig.random_state: consistent FIFOs, stale dead slots, counts up to MAX - 1) and an
    agent table that holds every id of theirs plus ``spare`` ids nobody carries; destinations uniform over the roads."""
    x = torch.stack([ig.random_state(c.net, seed=seed + b, t=200.0) for b in range(B)])
    A = int(x[:, :, :c.Nmax].max()) + 1 + spare
    ag = torch.zeros((B, A, 9))
    ag[:, :, 1] = torch.randint(0, c.N, (B, A), generator=torch.Generator().manual_seed(seed)).float()
    ag[:, :, 2] = 48 * 3600.0
    ag[:, 1:, 7] = 1.0
    return x, ag, A


def _pack(ops, plan, c, x, ag):
    fs = ops.FusedState(plan, x.size(0), ag.size(1), "cuda", c.Nmax)
    ops.fused_pack(plan, fs, x, c.Nmax, ag, c.net.congestion_constant.cuda(), ec=ops.EdgeConst(c.net.edge_attr, "cuda"))
    fs.check_flags()
    return fs


def _export(ops, plan, fs, x, Nmax):
    """The packed state in the reference's layout: static columns from ``x``, dynamic ones from the export."""
    out = x.clone()
    out[:, :, :3 * Nmax] = -3.0
    out[:, :, 3 * Nmax + 1] = -3.0
    out[:, :, 3 * Nmax + 5] = -3.0
    ops.fused_export(plan, fs, out, Nmax, 200.0)
    return out


# ---- 5. travel times -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("name", S.NAMES)
def test_travel_times_on_loaded_states(ops, name, B):
    from oracle import routing
    c = S.case(name)
    assert c.E % 64 != 0 and (B % 64 != 0)                                   # ragged 64-edge and 64-environment tiles
    plan = _plan(ops, c)
    x, ag, _ = _loaded(c, B, seed=300)
    cc = c.net.congestion_constant
    want = torch.stack([routing.edge_travel_time(x[b], c.ei, cc, c.Nmax) for b in range(B)])
    got = ops.edge_travel_time(plan, x.cuda(), c.Nmax, cc.cuda())
    assert torch.equal(got.cpu(), want)
    ff = x[0, :, 3 * c.Nmax + 2][c.ei[0]]
    assert bool((want[0] > ff).any()) and bool((want[0] == ff).any()) and not bool(torch.isnan(want).any())
    fs = _pack(ops, plan, c, x.cuda(), ag.cuda())
    fused = ops.fused_edge_travel_time(plan, fs)
    assert torch.equal(fused, got)
    assert torch.equal(fused, ops.edge_travel_time(plan, _export(ops, plan, fs, x.cuda(), c.Nmax), c.Nmax, cc.cuda()))


# ---- 6. the select kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_select_kernels_on_a_loaded_state(ops, name):
    """B = 3 loaded states routed on the travel times of the first. tarl_select_next_hop (all-pairs table) and
    tarl_select_next_hop_dest (the same table by destination) against oracle.routing.dijkstra_choice; the fused kernel
    against the unfused one through the export, its rank bytes against the out-lists. Then the documented guards: a head
    agent index out of range, a destination out of range, a destination without a tree — each leaves its row untouched."""
    from oracle import routing
    c = S.case(name)
    N, Nmax, B = c.N, c.Nmax, 3
    col = 3 * Nmax + 5
    plan = _plan(ops, c)
    x, ag, A = _loaded(c, B, seed=500)
    cc = c.net.congestion_constant
    w = ops.edge_travel_time(plan, x[:1].cuda(), Nmax, cc.cuda())[0]
    assert torch.equal(w.cpu(), routing.edge_travel_time(x[0], c.ei, cc, Nmax))
    nh_o, _ = routing.all_pairs(c.ei, w.cpu(), N)
    nh_ap = ops.all_pairs_shortest_paths(plan, w)[0]                                   # (1, N, N), shared
    assert torch.equal(nh_ap[0].cpu(), nh_o)
    table = nh_ap[0].t().to(torch.int32).contiguous()                                  # [d][u]
    slot = torch.arange(N, dtype=torch.int32, device="cuda")
    want = torch.stack([routing.dijkstra_choice(x[b], ag[b], c.ei, cc, Nmax, next_hop=nh_o)[0] for b in range(B)])
    assert torch.equal(want[0], routing.dijkstra_choice(x[0], ag[0], c.ei, cc, Nmax)[0])       # the oracle's own table
    assert not torch.equal(want[:, :, col], x[:, :, col]) and bool((want[:, :, col] == -1).any())
    a = x.clone().cuda()
    ops.select_next_hop(a, Nmax, ag.cuda(), nh_ap)
    assert torch.equal(a.cpu(), want)
    b_ = x.clone().cuda()
    ops.select_next_hop_dest(b_, Nmax, ag.cuda(), slot, table)
    assert torch.equal(b_.cpu(), want)
    # fused: through the export, against the unfused kernel on the export
    fs = _pack(ops, plan, c, x.cuda(), ag.cuda())
    before = _export(ops, plan, fs, x.cuda(), Nmax)
    unfused = before.clone()
    ops.select_next_hop_dest(unfused, Nmax, ag.cuda(), slot, table)
    assert torch.equal(unfused[:, :, col].cpu(), want[:, :, col])                      # pack and export keep what it reads
    c8 = torch.full((B, N), 0x55, dtype=torch.uint8, device="cuda")
    ops.fused_select_next_hop_dest(plan, fs, slot, table, choice8=c8)
    assert torch.equal(_export(ops, plan, fs, x.cuda(), Nmax), unfused)
    assert torch.equal(c8, fs.sel8.t().contiguous())
    # the rank bytes: every row was written (heads, destinations and slots all in range)
    codes, value = c8.cpu().long(), want[:, :, col].long()                             # [b][u]
    raw = codes == S.SEL_RAW
    assert torch.equal(raw, (value == -1) | (value == torch.arange(N))), "SEL_RAW exactly at -1 and on the destination"
    t = S.out_table(c)
    named = t[torch.arange(N).unsqueeze(0).expand(B, -1), codes.clamp(max=t.size(1) - 1)]
    assert torch.equal(named[~raw], value[~raw]), "a rank byte names another out-edge"
    beyond = int(((codes >= 4) & ~raw).sum())
    print(f"\nselect {name}: {beyond} of {B * N} rank bytes >= 4, {int(raw.sum())} raw")
    assert beyond > 0 and int(raw.sum()) > 0

    # ---- the guards ----
    xg, agg = x.clone(), ag.clone()
    rows = torch.nonzero((x[:, :, 3 * Nmax + 1] > 0).all(0) & (ig.degrees(c.net)[1] > 0)).view(-1)[:5].tolist()
    assert len(rows) == 5
    bound_for = torch.gather(ag[:, :, 1].long(), 1, x[:, :, 0].long())                 # [b][u]: the head's destination
    bound_for[:, rows] = -1
    no_tree = int(torch.mode(bound_for[bound_for >= 0]).values)    # the destination most heads have: its tree is withdrawn
    slot2 = slot.clone()
    slot2[no_tree] = -1
    xg[:, rows[0], 0], xg[:, rows[1], 0] = float(A), float(A + 40)                     # head ids at and above A
    xg[:, rows[2], 0], agg[:, A - 1, 1] = float(A - 1), float(N + 3)                   # destinations out of range
    xg[:, rows[3], 0], agg[:, A - 2, 1] = float(A - 2), -1.0
    xg[:, rows[4], 0], agg[:, A - 3, 1] = float(A - 3), float(no_tree)                 # a destination without a tree
    xg[:, rows, col] = -5.0                                                            # what an untouched row keeps
    expect = torch.stack([routing.dijkstra_choice(x[b], ag[b], c.ei, cc, Nmax, next_hop=nh_o)[0] for b in range(B)])
    expect[:, rows, :] = xg[:, rows, :]
    a = xg.clone().cuda()
    ops.select_next_hop(a, Nmax, agg.cuda(), nh_ap)
    exp_ap = expect.clone()
    exp_ap[:, rows[4], col] = nh_o[rows[4], no_tree].float()                           # (the all-pairs table has no slots)
    assert torch.equal(a.cpu(), exp_ap)
    gone = bound_for == no_tree                                                        # the other rows bound for no_tree
    assert int(gone.sum()) >= 2
    expect[:, :, col] = torch.where(gone, x[:, :, col], expect[:, :, col])
    b_ = xg.clone().cuda()
    ops.select_next_hop_dest(b_, Nmax, agg.cuda(), slot2, table)
    assert torch.equal(b_.cpu(), expect)
    fs = _pack(ops, plan, c, xg.cuda(), agg.cuda())
    before = _export(ops, plan, fs, xg.cuda(), Nmax)
    assert torch.equal(before[:, :, col].cpu(), xg[:, :, col])
    ops.fused_select_next_hop_dest(plan, fs, slot2, table)
    after = _export(ops, plan, fs, xg.cuda(), Nmax)
    assert torch.equal(after[:, :, col].cpu(), expect[:, :, col])
    assert torch.equal(after[:, rows].cpu(), before[:, rows].cpu())


# ---- 7. the prior head -----------------------------------------------------------------------------------------------------
def test_prior_logits_from_both_tables(ops):
    """The per-edge logits of csrc/prior.hip on MIXED, observation and packed-state kernels, from the all-pairs table and
    from the per-destination table, against the restatement of tests/test_gpu_prior_head.py on the oracle's distances.
    Agent 0 — whom every empty row reads — is bound for a road nobody can enter: all candidates of such a row are
    unreachable. The two dead ends have no candidate at all; the roads upstream of one get the same destination in a
    crafted observation."""
    from src.agents.base import destination_set
    from tarl_hip.engine import SimEngine
    from test_gpu_prior_head import UNREACHABLE, restated_logits
    c = S.case("MIXED")
    net, N, B = c.net, c.N, 3
    din, dout = ig.degrees(net)
    nobody_enters, dead_end = int(torch.nonzero(din == 0)[0]), int(torch.nonzero(dout == 0)[0])
    dist_ref = S.all_pairs("MIXED", "ff")[1]
    assert bool(torch.isinf(dist_ref[torch.arange(N) != nobody_enters, nobody_enters]).all())
    pops = torch.stack([ig.population(net, 12, seed=70 + b, t0=21540, t1=21570) for b in range(B)])
    pops[:, 0, 1] = float(nobody_enters)
    eng = SimEngine(net.x.unsqueeze(0).repeat(B, 1, 1).contiguous().cuda(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.cuda(), congestion_constant=net.congestion_constant, seed=5)
    eng.reset()
    emb = torch.randn(N, generator=torch.Generator().manual_seed(1))
    eng.prepare_policy(emb.cuda())
    for _ in range(12):
        eng.frame_fused()
    eng.check_flags()
    plan = eng.plan
    ff = c.w["ff"].cuda()
    table_ap = ops.all_pairs_shortest_paths(plan, ff, want_next_hop=False, want_dist=True)[1][0]
    assert torch.equal(table_ap.cpu(), dist_ref)
    dests, slot = destination_set(eng.agents, N)
    table_pd = ops.prior_dest_table(plan, ff, dests)
    assert torch.equal(table_pd.cpu(), dist_ref[:, dests.cpu()])
    obs = ops.fused_obs16(plan, eng.fs, eng._x, net.Nmax, eng.agents)
    assert float(obs[..., 1].sum()) > 0 and bool((obs[..., 1] == 0).any())
    crafted = obs.clone()
    upstream = c.ei[0][c.ei[1] == dead_end]
    crafted[:, upstream.cuda(), 8] = float(nobody_enters)
    src = c.ei[0]
    for w in (1.0, 0.37):
        ref = restated_logits(obs.cpu(), c.ei, dist_ref, emb, w)
        for table, sl in ((table_ap, None), (table_pd, slot)):
            assert torch.equal(ops.policy_prior_logits(plan, obs, emb.cuda(), table, w, dest_slot=sl).cpu(), ref)
            assert torch.equal(ops.fused_prior_logits(plan, eng.fs, eng._x, net.Nmax, eng.agents, emb.cuda(), table, w,
                                                      dest_slot=sl).cpu(), ref)
            got = ops.policy_prior_logits(plan, crafted, emb.cuda(), table, w, dest_slot=sl).cpu()
            assert torch.equal(got, restated_logits(crafted.cpu(), c.ei, dist_ref, emb, w))
            on_upstream = torch.isin(src, upstream)
            assert bool(on_upstream.any()) and torch.equal(got[:, on_upstream], (emb[c.ei[1]] + UNREACHABLE)[on_upstream].expand(B, -1))
        empty = (obs[..., 1] == 0).cpu()[:, src]                         # [b][e]: the edge leaves an empty row
        assert bool(empty.any()) and torch.equal(ref[empty], (emb[c.ei[1]] + UNREACHABLE).expand(B, -1)[empty])
        assert bool(torch.isfinite(ref).all()) and bool((ref > -1e19).any())
    assert not bool((src == dead_end).any())                             # a road without a candidate: no logit to write


# ---- 8. assignment ---------------------------------------------------------------------------------------------------------
def test_assignment_along_the_table_and_along_the_trees(ops):
    """tarl_msa_assign on the all-pairs table and tarl_msa_assign_sssp on per-origin trees, MIXED at free flow (no tied
    first hop: the two path sets agree): a seeded OD list with unreachable pairs, zero volumes and an origin that is its
    own destination, against a host walk of the oracle's table."""
    c = S.case("MIXED")
    N = c.N
    plan = _plan(ops, c)
    nh_o, _ = S.all_pairs("MIXED", "ff")
    gen = torch.Generator().manual_seed(8)
    P = 600
    o = torch.randint(0, N, (P,), generator=gen)
    d = torch.randint(0, N, (P,), generator=gen)
    vol = torch.rand(P, generator=gen, dtype=torch.float64) * 9 + 0.5
    vol[torch.rand(P, generator=gen) < 0.1] = 0.0
    d[:3] = o[:3]
    order = torch.argsort(o, stable=True)
    o, d, vol = o[order].contiguous(), d[order].contiguous(), vol[order].contiguous()
    unreachable = nh_o[o, d] < 0
    assert int(unreachable.sum()) >= 10 and int((vol == 0).sum()) >= 10 and int((unreachable & (vol > 0)).sum()) > 0
    is_road = torch.ones(N, dtype=torch.uint8)
    is_road[torch.randperm(N, generator=gen)[:6]] = 0
    want = torch.zeros(N, dtype=torch.float64)
    for oo, dd, vv in zip(o.tolist(), d.tolist(), vol.tolist()):
        if vv > 0 and nh_o[oo, dd] >= 0:
            node = oo
            while node != dd:
                node = int(nh_o[node, dd])
                if is_road[node]:
                    want[node] += vv
    assert float(want.sum()) > 0
    w32 = c.w["ff"].cuda()
    nh = ops.all_pairs_shortest_paths(plan, w32.double())[0][0]
    a = torch.zeros(N, dtype=torch.float64, device="cuda")
    ops.msa_assign(nh, o.cuda(), d.cuda(), vol.cuda(), is_road.cuda(), a)
    origins = torch.unique(o)
    od_ptr = torch.searchsorted(o, torch.cat([origins, torch.tensor([N])])).to(torch.int64)
    assert int(od_ptr[-1]) == P
    b = torch.zeros(N, dtype=torch.float64, device="cuda")
    ops.msa_assign_trees(plan, w32.double(), origins.cuda(), od_ptr.cuda(), d.cuda(), vol.cuda(), is_road.cuda(), b)
    assert torch.allclose(a.cpu(), want, rtol=1e-9, atol=0) and torch.allclose(b.cpu(), want, rtol=1e-9, atol=0)
    assert torch.allclose(a, b, rtol=1e-9, atol=0)
    assert bool((want[is_road == 0] == 0).all()) and bool((a.cpu()[is_road == 0] == 0).all())
