"""GPU: the row pass and the insert kernels behind the pointer table (csrc/fused_rows.hip, csrc/fused_insert.hip). Everything
they reach through the table (FusedBufs in device memory) is addressed as global memory (csrc/fused_frame.h: glob / gat /
gbase): dense words, slot records, agent arrays, accumulator banks and the status word — loads, stores and atomics, with
32-bit offsets from scalar bases where the launch allows them. None of this may change a bit, so the referee is the per-op
kernels (sim.hip, agents.hip), which know no table: ``fused_vs_unfused_frames`` of tests/test_gpu_fused.py.

The cases (``case_*``, which a child pytest process collects in place of ``test_*``): a loaded 5 x 5 torus with three waves
(the last one partial) and with a second tile of 44 lanes, long event lists and withdraw scans in both; the same torus
relabelled (chunks of rows that are no neighbours in memory); MIXED, with out-lists longer than the four targets of the node
record (the rest is walked through the table's out_pad) and chunks with missing rows; the rollout launcher, i.e. the rollout
instantiation with 32-bit offsets and the count byte, and the packed insert kernel. The children repeat the loaded torus
under the developer knobs that select another instantiation, each of them read once per process, and the rollout launcher
under the two pairs of knobs that select the 64-bit-address rollout kernels on consecutive chunks."""
import os
import subprocess
import sys

import pytest
import torch

import irregular_graphs as ig
import test_gpu_fused as tgf
from test_gpu_direction_words import PopCounting, torus

pytestmark = pytest.mark.gpu
AG_DONE = 8      # column of the agent table (csrc/tarl_common.h)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


# B = 130: one workgroup column, three waves, the last one partial; B = 300: two tiles, the second with 44 lanes
@pytest.mark.parametrize("B", [130, 300])
def case_loaded_torus(ops, B):
    """100 heterogeneous roads, Nmax = 40, 700 agents per environment leaving within 20 s of the start, 30 frames: fused frame
    against the per-op kernels bit for bit at every frame. A condition of the test: the last frame pops at least 20 heads per
    environment (the event lists are long) and some agents have arrived (the withdraw scan found destinations connected)."""
    from tarl_hip import synth
    net = torus()
    N = net.num_roads
    assert (N, net.edge_index.size(1), net.Nmax) == (100, 400, 40)
    plan = ops.Plan(net.edge_index, N)
    pops = torch.stack([synth.population(700, N, seed=b, t0=100, t1=120) for b in range(B)])
    counting = PopCounting(ops)
    events, a1 = tgf.fused_vs_unfused_frames(counting, net, plan, pops, 30)
    arrived = int(a1[:, :, AG_DONE].sum())
    print(f"\nB = {B}: pops per frame {counting.pops}, agents arrived {arrived}")
    assert len(counting.pops) == 30 and events >= sum(counting.pops) > 0
    assert counting.pops[29] >= 20 * B, f"frame 29 pops {counting.pops[29]} heads, fewer than 20 per environment"
    assert arrived > 0, "nobody arrived: the withdraw scan never tested a destination"


def case_relabelled(ops):
    """The torus with its roads renumbered at random: the Direction gather runs its per-row (non-sibling) instantiation, and
    the rows of a row-pass chunk are scattered over the state — the plan still groups them by their out-edge targets, so the
    chunk table holds non-consecutive rows. Under TARL_ROWS_SIBLINGS=0 (a child below) the same case runs the row pass's
    non-sibling instantiation: consecutive chunks of unrelated rows, every row gathering its downstream post words itself."""
    from tarl_hip import synth
    net = tgf.relabelled(torus(), seed=11)
    plan = ops.Plan(net.edge_index, net.num_roads)
    assert not plan.siblings4
    # which row-pass instantiation runs here: the sibling chunk table unless the knob switches it off
    sib_rows = os.environ.get("TARL_ROWS_SIBLINGS", "1") != "0" and os.environ.get("TARL_NCHUNK", "4") == "4"
    assert plan.row_siblings and plan.num_row_chunks == net.num_roads // 4
    print(f"\nrelabelled torus: row pass on {'the sibling chunk table' if sib_rows else 'consecutive (non-sibling) chunks'}")
    B = 130
    pops = torch.stack([synth.population(700, net.num_roads, seed=b, t0=100, t1=120) for b in range(B)])
    events, a1 = tgf.fused_vs_unfused_frames(ops, net, plan, pops, 30)
    assert events > 20 * B and float(a1[:, :, AG_DONE].sum()) > 0


def case_mixed(ops):
    """MIXED (tests/irregular_graphs.py): out-lists of more than four targets (the rest of a Response test walks out_pad
    through the table) and chunks with missing rows (loaded as another row of the chunk, never used)."""
    net = ig.graph("MIXED")
    N = net.num_roads
    plan = ops.Plan(net.edge_index, N)
    dout = ig.degrees(net)[1]
    assert int(dout.max()) > 4 and plan.max_out > 4
    chunks = plan.num_row_chunks if plan.row_siblings else -(-N // 4)
    assert 4 * chunks > N, "no chunk remainder"
    B = 70
    pops = torch.stack([ig.population(net, ig.CENSUS["MIXED"]["per_road"], seed=40 + b) for b in range(B)])
    events, a1 = tgf.fused_vs_unfused_frames(ops, net, plan, pops, 45)
    assert events > 5 * B and float(a1[:, :, AG_DONE].sum()) > 0


def case_rollout(ops, monkeypatch):
    """The rollout launcher against the frame loop at B = 300, T = 33: the rollout instantiation of the row pass (no frame-API
    outputs, 32-bit offsets from scalar bases, the count byte) and the packed insert kernel."""
    tgf.test_rollout_launcher_equals_frame_loop(ops, monkeypatch, 300, 33, "2")


# knob (None: none set) -> the cases it runs, and how many they are
CHILDREN = [(None, "case_", 5), ("TARL_NCHUNK=1", "case_loaded_torus", 2), ("TARL_NCHUNK=2", "case_loaded_torus", 2),
            ("TARL_ADDR32=0", "case_loaded_torus", 2), ("TARL_ROWS_SIBLINGS=0", "case_loaded_torus or case_relabelled", 3),
            # the rollout instantiations with 64-bit addresses on consecutive chunks (four and two rows per lane): the two
            # kernels whose spilled-SGPR count is above the parent's (profiles/rows_table_kernel_resources.txt)
            ("TARL_ADDR32=0,TARL_ROWS_SIBLINGS=0", "case_rollout", 1), ("TARL_ADDR32=0,TARL_NCHUNK=2", "case_rollout", 1)]


@pytest.mark.parametrize("knob,select,count", CHILDREN, ids=[k or "no knob" for k, _, _ in CHILDREN])
def test_rows_behind_the_table(knob, select, count):
    env = dict(os.environ)
    for k, _, _ in CHILDREN:
        for kv in (k or "").split(","):
            env.pop(kv.split("=")[0], None)
    for kv in (knob or "").split(","):
        if kv:
            k, v = kv.split("=")
            env[k] = v
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-o", "python_functions=case_*",
                        os.path.abspath(__file__), "-k", select],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"{count} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
