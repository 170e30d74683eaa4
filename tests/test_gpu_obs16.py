"""GPU: the four observation builders of csrc/edge_mlp.hip — k_obs16_packed and k_obs16_packed_bf16 (tiles of 8 roads x 64
environments), k_obs16_rows and k_obs16_cat (256-thread blocks) — against the exported state, bit for bit, at the shapes
where their tiles end: B in {1, 63, 64, 65, 130} (below, at and above one environment tile, three tiles), N = 36 (a half road
tile), 288 (more than one 256-thread block), 80 on MIXED (out-degrees up to 9: SELECTED_ROAD rank bytes above 3 go through
out_dst[out_ptr[i] + rank]), 37 on a small hub graph (N % 8 odd) and 16 on LONGMIX (FIFOs of up to 126 in 127-slot rings: count
features beyond 100, heads read at ring offsets beyond 63); every B on the 36-road torus, every graph at B = 65.
Twice per engine: straight after reset() and after 25 frames (LONGMIX: 150), when counts, ON_WAY flags and rank bytes are live.

The reference is ``eng.x`` as test_fused_obs16_matches_the_exported_state builds it (the bf16 builder: ``ref.to(bfloat16)``).
The export turns the SELECTED_ROAD byte into a road through the same device function the builders use, so that column is
checked once more against the rank bytes decoded on the host from the edge list. Output buffers go in filled with NaN: a
row nobody wrote shows. The graphs come from ``irregular_graphs.road_network``, which asserts ``fused_path_supported``."""
import pytest
import torch

import irregular_graphs as ig

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEL_RAW = 0x7F
FRAMES = 25


def _net(name):
    from tarl_hip import synth
    if name == "torus3x3":
        return synth.torus_network(3, 3, heterogeneous=True, seed=1)           # 36 roads: four road tiles and a half
    if name == "torus9x8":
        return synth.torus_network(9, 8, heterogeneous=True, seed=2)           # 288 roads: two blocks of k_obs16_rows
    if name in ("MIXED", "LONGMIX"):
        return ig.graph(name)
    return ig.road_network(ig.hub_links([(6, 5), (3, 3)], 10, 4), 4)            # "HUBS37": 37 roads


CASES = [("torus3x3", B) for B in (1, 63, 64, 65, 130)] + [(g, 65) for g in ("torus9x8", "MIXED", "HUBS37", "LONGMIX")]


def _engine(net, B, per_road=3, window=20):
    from tarl_hip import synth
    from tarl_hip.engine import SimEngine
    N = net.num_roads
    pops = torch.stack([synth.population(per_road * N, N, seed=b, t0=21540, t1=21540 + window) for b in range(B)])
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax, pops.cuda(),
                    congestion_constant=net.congestion_constant, seed=4)
    eng.reset()
    return eng


def _codes_of(net, sel_value):
    """fused_pack's rule on the host: the rank of the out-edge whose target is ``sel_value[i]``, SEL_RAW when there is none."""
    return torch.tensor([lst.index(int(v)) if int(v) in lst else SEL_RAW for lst, v in zip(ig.out_lists(net), sel_value.tolist())],
                        dtype=torch.uint8)


def _check(eng, net, what):
    """All four packed-state builders against the exported state. Returns (ref, rank bytes (N, B))."""
    from tarl_hip import ops
    B, N = eng.B, eng.N
    full = lambda shape, dtype=torch.float32: torch.full(shape, NAN, dtype=dtype, device="cuda")
    obs = ops.fused_obs16(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, out=full((B, N, 16)))
    ob = ops.fused_obs16_bf16(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, out=full((B, N, 16), torch.bfloat16))
    assert bool(torch.isnan(full((2,), torch.bfloat16)).all())
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    env, slot = [B - 1, 0, B // 2, 0, B - 1], [3, 0, 4, 1, 2]      # repeated environments, the first and the last, slots in no order
    rows = ops.fused_obs16_rows(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, i32(env), i32(slot), full((5, N, 16)))
    one = ops.fused_obs16_rows(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, i32([B - 1]), i32([0]), full((1, N, 16)))
    code = (eng.fs.sel8 & SEL_RAW).cpu()                             # (N, B), before the export below refreshes fs.sel
    raw = eng.fs.sel.cpu()
    x = eng.x                                                        # exports the packed state
    nf = x[:, :, 3 * eng.Nmax:]
    head = x[:, :, 0].long()
    ref = torch.cat((nf, torch.gather(eng.agents, 1, head.unsqueeze(-1).expand(B, N, 9))), dim=-1)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(obs, ref), what
    assert ob.dtype == torch.bfloat16 and torch.equal(ob, ref.to(torch.bfloat16)), what
    for e, s in zip(env, slot):
        assert torch.equal(rows[s], ref[e]), (what, e, s)
    assert torch.equal(one[0], ref[B - 1]), what
    # SELECTED_ROAD from the rank bytes, decoded on the host: target of the out-edge with that rank in ascending edge id
    lists = ig.out_lists(net)
    width = max(len(l) for l in lists)
    table = torch.tensor([l + [-1] * (width - len(l)) for l in lists], dtype=torch.float32)
    ranked = torch.gather(table, 1, code.long().clamp(max=width - 1))
    assert bool(((code == SEL_RAW) | (code.long() < torch.tensor([len(l) for l in lists]).unsqueeze(1))).all()), what
    want_sel = torch.where(code == SEL_RAW, raw, ranked).t()         # (B, N)
    assert torch.equal(obs[:, :, 5].cpu(), want_sel), what
    return ref, code


@pytest.mark.parametrize("graph,B", CASES, ids=[f"{g}-B{b}" for g, b in CASES])
def test_packed_state_builders_match_the_exported_state(graph, B):
    net = _net(graph)
    N = net.num_roads
    assert N == {"torus3x3": 36, "torus9x8": 288, "MIXED": 80, "HUBS37": 37, "LONGMIX": 16}[graph]
    long_fifo = graph == "LONGMIX"
    eng = _engine(net, B, ig.CENSUS[graph]["per_road"], 30) if long_fifo else _engine(net, B)
    # straight after reset(): the SELECTED_ROAD bytes are what fused_pack made of the network's column (all zero: the rank of
    # road 0 where a road leads there, SEL_RAW with the raw value 0.0 everywhere else — reset leaves them alone)
    ref, code = _check(eng, net, "after reset")
    sel0 = net.x[:, 3 * net.Nmax + 5]
    assert float(sel0.abs().max()) == 0.0
    want = _codes_of(net, sel0)
    assert torch.equal(eng.fs.sel8.cpu(), want.unsqueeze(1).expand(N, B)) and torch.equal(code, want.unsqueeze(1).expand(N, B))
    assert int((want == SEL_RAW).sum()) >= N - 9 and int((want != SEL_RAW).sum()) >= 1
    assert float(ref[:, :, 1].abs().sum()) == 0.0 and float(ref[:, :, 5].abs().sum()) == 0.0        # empty roads, SELECTED_ROAD 0
    assert torch.equal(ref[:, :, 7:], eng.agents[:, :1].expand(B, N, 9))                            # nobody: the dummy's row
    # live state
    eng.prepare_policy(torch.randn(N, generator=torch.Generator().manual_seed(1)).cuda())
    for _ in range(150 if long_fifo else FRAMES):
        eng.frame_fused()
    if long_fifo:      # before the builders run: rows at ring offsets beyond 63, and the run stayed inside the domain
        eng.check_flags()
        assert int(((eng.fs.tl >> 1) & 127).max()) >= 64
    ref, code = _check(eng, net, "after frames")
    assert float(ref[:, :, 1].sum()) > 0 and float(ref[:, :, 14].sum()) > 0                         # counts and ON_WAY flags
    ranks = code[code != SEL_RAW]
    assert ranks.numel() > 0 and int(ranks.max()) >= 1
    if graph == "MIXED":
        assert int(ranks.max()) > 3, int(ranks.max())               # beyond the four targets a node record embeds
        assert bool((ref[:, :, 1] == 0).any())                      # some road is empty (its head is the dummy, agent row 0)
        assert bool((code == SEL_RAW).any())                        # a road without out-edges keeps its raw value
    if graph.startswith("torus"):
        assert int(ranks.max()) == 3 and not bool((code == SEL_RAW).any())
    if long_fifo:
        assert 100 <= float(ref[:, :, 1].max()) < net.Nmax and int(ranks.max()) == 3      # the count feature of a long queue


def _poison(shape):
    """What the next allocation of this size gets back from the caching allocator: NaN (policy_obs16 allocates its result)."""
    t = torch.full(shape, NAN, device="cuda")
    del t


@pytest.mark.parametrize("M,N,per_sample", [(3, 100, False), (3, 100, True), (1, 300, False), (2, 257, True)])
def test_policy_obs16_from_a_strided_view_and_both_agent_table_shapes(M, N, per_sample):
    """k_obs16_cat with M * N above one 256-thread block, ``node_features`` a view of a wider state (row stride 22 > 7) and
    the agent table shared (A, 9) or per sample (M, A, 9); indices in range, the first and the last agent among them."""
    from tarl_hip import ops
    g = torch.Generator().manual_seed(M * 1000 + N)
    A, Nmax = 37, 5
    x = torch.randn((M, N, 3 * Nmax + 7), generator=g).cuda()
    nf = x[:, :, 3 * Nmax:]
    assert nf.stride(1) == 22 and not nf.is_contiguous() and M * N > 256
    ag = torch.randn((M, A, 9) if per_sample else (A, 9), generator=g).cuda()
    ai = torch.randint(0, A, (M, N), generator=g)
    ai[0, 0], ai[-1, -1], ai[0, -1], ai[-1, 0] = 0, A - 1, A - 1, 0
    ai = ai.cuda()
    rows = torch.gather(ag, 1, ai.unsqueeze(-1).expand(M, N, 9)) if per_sample else ag[ai]
    ref = torch.cat((nf, rows), dim=-1)
    _poison((M, N, 16))
    obs = ops.policy_obs16(nf, ai, ag)
    assert obs.shape == (M, N, 16) and torch.equal(obs, ref)
    if M == 1:                                                       # the unbatched spelling: (N, 7) and (N,)
        _poison((M, N, 16))
        assert torch.equal(ops.policy_obs16(nf[0], ai[0], ag), ref)
