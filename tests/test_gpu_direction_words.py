"""GPU: the word table of the Direction gather (csrc/fused_direction.hip). Pass 2 — the Gumbel race of the listed pairs —
is served from what pass 1 left in LDS (the upstream words beside the list entry, the chunk's statics once per workgroup)
instead of gathering it from global memory again; a pair listed beyond the table's capacity, and every pair of a workgroup
that repeats its pass in exact form, still takes the gather path. Both paths must give the same bits, so the referee is the
per-op kernels (sim.hip, agents.hip), which know neither: ``fused_vs_unfused_frames`` of tests/test_gpu_fused.py.

The capacity is the developer knob TARL_DIR_WORDS, read once per process (unset: the compiled capacity, 0: the gather path
for everybody, n: the first n list positions of a workgroup). Every knob value therefore runs its cases (the ``case_*``
functions below, which the child collects in place of ``test_*``) in a child pytest process. With 1 and 5 both paths run
inside the same workgroups and the boundary entry is hit in every loaded frame: a torus of 100 roads is 25 workgroups per
tile column, and ``case_frames`` fails unless its last frame pops at least 20 heads per environment (a pop is a race that
was won: the listed pairs are at least the pops), i.e. far more than 5 per workgroup."""
import os
import subprocess
import sys

import pytest
import torch

import irregular_graphs as ig
import test_gpu_fused as tgf

pytestmark = pytest.mark.gpu
KNOB = "TARL_DIR_WORDS"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


class PopCounting:
    """``tarl_hip.ops`` with the pops of every ``core_step`` call (the per-op side of the frame loop) counted."""

    def __init__(self, ops):
        self._ops, self.pops = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def core_step(self, *args, **kw):
        out = self._ops.core_step(*args, **kw)
        self.pops.append(int(out[1].sum()))
        return out


def torus():
    from tarl_hip import synth
    return synth.torus_network(5, 5, heterogeneous=True, seed=3)      # 100 roads, 400 route edges, Nmax = 40


# B = 130: one workgroup column, three waves, the last one partial; B = 300: two tiles, the second with 44 lanes
@pytest.mark.parametrize("B", [130, 300])
def case_frames(ops, B):
    """The inputs of test_rollout_launcher_equals_frame_loop — 700 agents per environment leaving within 20 s of the start,
    30 frames from the start (the frame loop's clock starts at 100, so the window is 100 .. 120) — fused frame against the
    per-op kernels: state, agents, actions, rewards, counts, pop and withdraw masks bit for bit at every frame."""
    from tarl_hip import synth
    net = torus()
    N = net.num_roads
    assert (N, net.edge_index.size(1), net.Nmax) == (100, 400, 40)
    plan = ops.Plan(net.edge_index, N)
    assert plan.siblings4
    pops = torch.stack([synth.population(700, N, seed=b, t0=100, t1=120) for b in range(B)])
    counting = PopCounting(ops)
    events, _ = tgf.fused_vs_unfused_frames(counting, net, plan, pops, 30)
    print(f"\npops per frame, B = {B}: {counting.pops}")
    assert len(counting.pops) == 30 and events >= sum(counting.pops) > 0
    tiles = -(-B // 256)
    # a condition of the test: the network is loaded, every workgroup's list runs past a table of 5 entries
    assert counting.pops[29] >= 20 * B, f"frame 29 pops {counting.pops[29]} heads, fewer than 20 per environment"
    assert max(counting.pops) > 5 * 25 * tiles


def case_relabelled(ops):
    """The torus with its roads renumbered at random: the rows of a chunk are unrelated, the Direction gather runs its
    per-row (non-sibling) instantiation and the stored words are the row's own. Frame loop against the per-op kernels
    (head words as the count's source), then the rollout launcher (count byte) against the frame loop."""
    from tarl_hip import synth
    net = tgf.relabelled(torus(), seed=11)
    plan = ops.Plan(net.edge_index, net.num_roads)
    assert not plan.siblings4
    B = 130
    pops = torch.stack([synth.population(700, net.num_roads, seed=b, t0=100, t1=120) for b in range(B)])
    events, _ = tgf.fused_vs_unfused_frames(ops, net, plan, pops, 30)
    assert events > 20 * B
    tgf.test_rollout_on_a_relabelled_torus_equals_frame_loop(ops, B, 30)


def case_mixed(ops):
    """MIXED (tests/irregular_graphs.py): in-degrees 0 .. 9 and chunk remainders. A table-served pair gathers its in-edges
    of rank >= 4 one by one and ignores the padding records of a short in-list; at frame 30 two raw SELECTED_ROAD codes send
    the workgroups that see them through the exact pass (tests/test_gpu_irregular.py: fused_frame_case)."""
    net = ig.graph("MIXED")
    plan = ops.Plan(net.edge_index, net.num_roads)
    din = ig.degrees(net)[0]
    assert plan.max_in == 9 and not plan.siblings4 and int((din < 4).sum()) > 0 and int((din > 4).sum()) > 0
    B = 70
    road = int(torch.nonzero(din == 9)[0])
    ups = net.edge_index[0][net.edge_index[1] == road][[2, 6]].tolist()
    lists = ig.out_lists(net)
    far = [next(c for c in order if c not in lists[j] and c != road)
           for j, order in zip(ups, (range(net.num_roads), reversed(range(net.num_roads))))]
    pops = torch.stack([ig.population(net, ig.CENSUS["MIXED"]["per_road"], seed=40 + b) for b in range(B)])
    events, a1 = tgf.fused_vs_unfused_frames(ops, net, plan, pops, 45, raw_sel=(30, 5, ups, far))
    assert events > 5 * B and float(a1[:, :, 8].sum()) > 0


def case_exact_pass(ops):
    """Raw SELECTED_ROAD codes on half of the roads: a workgroup that repeats its pass in exact form re-lists its pairs from
    global words and serves all of them by the gather path, beside workgroups that keep their table."""
    tgf.test_raw_selected_road_codes_take_the_exact_direction_pass(ops)


def case_rollout(ops, monkeypatch):
    """The rollout launcher against the frame loop at B = 300, T = 33: the count-byte instantiation (the row's own count
    from the count slice of the frame before) for t > 0, the head-word instantiation for frame 0."""
    tgf.test_rollout_launcher_equals_frame_loop(ops, monkeypatch, 300, 33, "2")


# knob value (None: unset) -> the cases it runs, and how many they are
CHILDREN = [(None, "case_", 6), ("0", "case_frames", 2), ("1", "case_frames", 2), ("5", "case_", 6)]


@pytest.mark.parametrize("value,select,count", CHILDREN, ids=[KNOB + ("=" + v if v is not None else " unset") for v, _, _ in CHILDREN])
def test_direction_word_table(value, select, count):
    env = dict(os.environ)
    env.pop(KNOB, None)
    if value is not None:
        env[KNOB] = value
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-o", "python_functions=case_*",
                        os.path.abspath(__file__), "-k", select],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"{count} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
