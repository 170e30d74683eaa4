"""GPU: the packed simulation path at its FIFO-length limit, Nmax = 127. The packed state keeps a road's count in bits 0..6
of a byte whose bit 7 is HD_DIRTY, the ring-buffer head offset in seven bits of the tail word, and wraps phys() once
(csrc/fused_common.h); every other graph of the suite holds at most 41 agents per road, so no count byte had bit 6 set, no
offset reached 64 and no long ring wrapped in any test with traffic. LONG127 and LONGMIX (tests/irregular_graphs.py: 16
roads of a 2 x 2 torus, 940 m each, MAX_NUMBER_OF_AGENT 126 — on LONGMIX every third road 14 — 150 agents per road) fill
the FIFOs to 126; tests/test_long_fifo_host.py shows on the CPU that these inputs reach counts, offsets and insert
positions beyond 63 thousands of times and that a kernel which read a count through ``& 63`` would leave the oracle's
trajectory within 20 frames.

The cases are those of tests/test_gpu_irregular.py, bit-exact throughout (log-probs to fp32 rounding): CPU oracle -> per-op
kernels -> fused frame -> one-call rollouts; the oracle replay with the device's own noise is the one of
tests/test_gpu_bench_geometry.py. What the device's own words reached (count bytes, ring offsets, a wrap, HD_DIRTY) is
asserted from ``fs.hdp`` / ``fs.tl`` and from the rollouts' uint8 count buffers."""
import pytest
import torch

import irregular_graphs as ig
import test_gpu_irregular as tgi

pytestmark = pytest.mark.gpu
GRAPHS = ig.LONG_GRAPHS
FRAMES = 300      # a ring needs about 130 pops to wrap


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


class RingWatch:
    """What the packed state's own words held at the frames the frame loop checks its records: the count byte of ``hdp``
    (count in bits 0..6, HD_DIRTY in bit 7) and the ring offset in bits 1..7 of ``tl``. An offset only ever advances modulo
    Nmax (by the row's pops and withdrawals), so an offset that is smaller than at the visit before has wrapped."""

    def __init__(self, restart_at=None):
        self.restart_at, self.seen = restart_at, {}
        self.top_count = self.top_offset = self.wraps = self.dirty = 0
        self.prev = None

    def __call__(self, s, fs):
        byte, off = fs.hdp[..., 0] & 0xFF, (fs.tl >> 1) & 127
        count = byte & 0x7F
        self.seen[s] = (int(count.max()), int(off.max()))
        self.top_count, self.top_offset = max(self.top_count, int(count.max())), max(self.top_offset, int(off.max()))
        self.dirty += int(((byte & 0x80) != 0).sum())
        if self.prev is not None and s != self.restart_at:      # (a pack puts every offset back to 0: no wrap)
            self.wraps += int((off < self.prev).sum())
        self.prev = off.clone()

    def check(self, name, what):
        print(f"\n{what} {name}: largest count byte {self.top_count}, largest ring offset {self.top_offset}, "
              f"offsets seen smaller than ten frames before {self.wraps}, dirty rows seen {self.dirty}")
        assert 64 <= self.top_count < 127 and self.top_offset >= 64 and self.wraps > 0
        assert name != "LONGMIX" or self.dirty > 0


# ---- per-op kernels against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_core_step_vs_oracle(ops, name):
    tgi.core_step_case(ops, name)


@pytest.mark.parametrize("t1,frames", [(130, 120), (100, 40)])
def test_env_step_chain_vs_oracle(ops, t1, frames):
    """LONGMIX, 150 agents per road due within 30 s, and all of them due in frame 0 (2 400 ready agents: the insert's
    ordered path through global scratch, roads that take 100 and more agents in one frame)."""
    top, most_inserted = tgi.env_chain_case(ops, "LONGMIX", frames, t1=t1)
    assert t1 != 100 or most_inserted > ig.INS_CAP


# ---- fused frame against the per-op kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("name", GRAPHS)
def test_fused_frame_vs_per_op_kernels(ops, name, B):
    watch = RingWatch()
    tgi.fused_frame_case(ops, name, B, FRAMES, visit=watch)
    watch.check(name, f"fused frames B={B}")


@pytest.mark.parametrize("name", GRAPHS)
def test_fused_frame_with_a_backlog_of_the_whole_population(ops, name):
    """Every agent due in frame 0: the fused insert's backlog path puts 100 and more agents behind each other in one row."""
    watch = RingWatch()
    tgi.fused_frame_case(ops, name, 3, FRAMES, t1=100, visit=watch)
    assert watch.seen[0][0] >= 100, watch.seen[0]      # the count byte after the first frame
    watch.check(name, "fused frames, backlog")


@pytest.mark.parametrize("name", GRAPHS)
def test_pack_in_mid_simulation(ops, name):
    """Frame 150: rows hold 100 and more agents at ring offsets beyond 63; the state the fused side has just exported is
    packed again (every offset back to 0) and both sides go on for 50 frames."""
    watch = RingWatch(restart_at=150)
    tgi.fused_frame_case(ops, name, 5, 200, visit=watch, repack_at=150)
    print(f"\nrepack {name}: (largest count, largest offset) at frame 140 {watch.seen[140]}, 150 {watch.seen[150]}, 199 {watch.seen[199]}")
    assert watch.seen[140][0] >= 100 and watch.seen[140][1] >= 64
    assert watch.seen[150][0] >= 100 and watch.seen[150][1] < 64      # one frame after the pack
    assert watch.seen[199][1] > watch.seen[150][1]


@pytest.mark.parametrize("name", GRAPHS)
def test_pack_and_export_of_full_fifos(ops, name):
    """Random mid-simulation states with up to 125 agents per road (and stale values behind them), packed and exported
    unchanged into a tensor whose FIFO blocks, counts and SELECTED_ROAD were overwritten."""
    net = ig.graph(name)
    N, Nmax, B, t = net.num_roads, net.Nmax, 4, 200.0
    xs = torch.stack([ig.random_state(net, seed=80 + b, t=t) for b in range(B)])
    counts = xs[:, :, 3 * Nmax + 1]
    assert int(counts.max()) == 125 and int((counts >= 64).sum()) >= B
    A = int(xs[:, :, :Nmax].max()) + 2
    ag = torch.zeros((B, A, 9))
    ag[:, :, 1] = torch.randint(0, N, (B, A), generator=torch.Generator().manual_seed(4)).float()
    ag[:, :, 2] = 48 * 3600.0
    ag[:, 1:, 7] = 1.0
    plan = tgi.plan_of(ops, net)
    x, a = xs.cuda(), ag.cuda()
    fs = ops.FusedState(plan, B, A, "cuda", Nmax)
    ops.fused_pack(plan, fs, x, Nmax, a, net.congestion_constant.cuda(), ec=ops.EdgeConst(net.edge_attr, "cuda"))
    assert torch.equal((fs.hdp[..., 0] & 0x7F).t().float().cpu(), counts) and int(((fs.tl >> 1) & 127).max()) == 0
    out = x.clone()
    out[:, :, :3 * Nmax] = -3.0
    out[:, :, 3 * Nmax + 1] = -3.0
    out[:, :, 3 * Nmax + 5] = -3.0
    ops.fused_export(plan, fs, out, Nmax, t)
    fs.check_flags()
    assert torch.equal(out, x) and torch.equal(out.cpu(), xs)


# ---- one-call rollouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("name", GRAPHS)
def test_rollouts_equal_the_frame_loop(ops, monkeypatch, name, B):
    """rollout_fused (merge 1 and 2) and rollout_env (16 roads: the 256-thread kernel) with device Philox noise, 150 frames
    twice, against the frame loop and the per-op engine; the raw uint8 count buffers reach bit 6 and never Nmax."""
    bytes_ge64, top_byte = tgi.rollout_case(ops, monkeypatch.setenv, name, B, FRAMES // 2)
    print(f"\nrollouts {name} B={B}: count bytes >= 64: {bytes_ge64}, largest count byte {top_byte}")
    assert bytes_ge64 > 0 and top_byte < 127
    assert name != "LONGMIX" or top_byte == 126      # a long road at its MAX_NUMBER_OF_AGENT: one relief admission


# ---- the oracle with the device's noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "env"])
def test_rollout_replayed_by_the_oracle_with_the_device_noise(path):
    """tarl_fused_rollout and tarl_rollout_env on LONGMIX, B = 64, 300 frames, every agent due within 30 s: sim.env_step
    replays three environments from the Gumbel values and action bytes of the device (draw checks A1 - A3 on) — counts and
    reward of every frame, the final state and the agent table bit for bit."""
    from test_gpu_bench_geometry import _replay_live_policy_rollout
    net = ig.graph("LONGMIX")
    A = ig.CENSUS["LONGMIX"]["per_road"] * net.num_roads
    st = _replay_live_policy_rollout(net, B=64, A=A, T=FRAMES, probe=[0, 31, 63], window=30, pop_seed=3, eng_seed=5, emb_seed=6,
                                     min_pops=1000, want_arrivals=True, max_flips=30, path=path, min_arrivals=100)
    assert st["on_way"] > 300, st      # still loaded after 300 frames


# ---- beyond the limit: MAX_NUMBER_OF_AGENT 127, Nmax 128 ------------------------------------------------------------------------
def test_nmax_128_is_refused_by_the_packed_path_and_runs_on_the_per_op_kernels(ops):
    """948 m links: Nmax = 128. The packed path refuses the graph on the host, before any launch; an engine on the per-op
    kernels (what the trainer constructs when ``fused_path_supported`` says no) equals the oracle for 20 frames."""
    from oracle import sim
    from tarl_hip import lib, synth
    from tarl_hip.engine import SimEngine
    net = synth.torus_network(2, 2, length=948.0, freespeed=94.8)
    N, Nmax, E = net.num_roads, net.Nmax, net.edge_index.size(1)
    assert Nmax == 128 and int(net.x[:, 3 * Nmax].max()) == 127 and not ops.fused_path_supported(net.edge_index, Nmax)
    plan = ops.Plan(net.edge_index, N)
    B, per_road, frames = 2, 100, 20
    pops = [ig.population(net, per_road, seed=b, t0=21540, t1=21545) for b in range(B)]
    with pytest.raises(lib.TarlError, match="Nmax <= 127"):
        ops.FusedState(plan, B, per_road * N + 1, "cuda", Nmax)
    make = lambda **kw: SimEngine(net.x.unsqueeze(0).repeat(B, 1, 1).cuda(), net.edge_index, net.edge_attr, Nmax,
                                  torch.stack(pops).cuda(), congestion_constant=net.congestion_constant, seed=9, **kw)
    with pytest.raises(lib.TarlError, match="fused=False"):      # no quiet fall-back: the caller decides
        make()
    eng = make(fused=ops.fused_path_supported(net.edge_index, Nmax))
    assert eng.fs is None
    eng.reset()
    xs, adj = [net.x.clone() for _ in range(B)], net.dense_adjacency()
    gen = torch.Generator().manual_seed(6)
    for s in range(frames):
        t = float(eng.time)
        choice, u = ig.random_actions(net, gen, B), torch.rand((B, E), generator=gen)
        eng.step(choice=choice.cuda(), gumbel=ops.gumbel_from_uniform_cpu(u).cuda())
        for b in range(B):
            out = sim.env_step(xs[b], pops[b], net.edge_index, net.edge_attr, adj, ig.onehot_of(choice[b], E), t, Nmax,
                               uniform=u[b], congestion_constant=net.congestion_constant)
            assert torch.equal(eng.x[b].cpu(), xs[b]) and torch.equal(eng.agents[b].cpu(), pops[b]), f"env {b} frame {s}"
            assert eng.reward[b].item() == out["reward"].item()
    eng.check_flags()
    assert max(int(x[:, 3 * Nmax + 1].max()) for x in xs) >= 64 and sum(float(p[:, sim.DONE].sum()) for p in pops) > 0
