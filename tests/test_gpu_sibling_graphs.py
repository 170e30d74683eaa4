"""GPU: the sibling Direction gather and the quad action draw off the torus. The plan sets ``siblings4`` from the topology
alone (rows 4c .. 4c+3 with equal in-degree and the same first four sources: k_fused_direction<4, SIB = true, ...>), and the
draw of a whole rollout takes its quad form whenever every road has out-edges and their number is a multiple of four
(k_fused_choice_all<true>). SIBS and SIBS_TAILS (tests/irregular_graphs.py) are the graphs on which both hold and no degree
is fixed at four: in-degrees 0 .. 9 that differ from chunk to chunk — padding records in the shared gather, the per-row
tail loop beside the shared first four — siblings that share ONLY their first four sources (SIBS_TAILS), and out-degrees
1 .. 9 under the quad draw. tests/test_sibling_graphs_host.py shows on the CPU that these inputs reach those branches
hundreds of times and that a kernel which took a sibling's tail sources from sibling 0 would leave the oracle's trajectory
on SIBS_TAILS and on SIBS would not.

The cases are those of tests/test_gpu_irregular.py, bit-exact throughout (log-probs to fp32 rounding): CPU oracle -> per-op
kernels -> fused frame -> one-call rollouts. The developer knobs are read once per process, so the B = 130 frame case and
the B = 5 rollout case of both graphs (the ``case_*`` functions, which a child collects in place of ``test_*``) run again in
child pytest processes, last in the file: the gather path alone and both paths inside one workgroup (TARL_DIR_WORDS), the
generic instantiations on the same inputs (the control that tells a kernel fault from an input fault) and 64-bit offsets."""
import os
import subprocess
import sys

import pytest
import torch

import irregular_graphs as ig
import test_gpu_irregular as tgi

pytestmark = pytest.mark.gpu
GRAPHS = ("SIBS", "SIBS_TAILS")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


@pytest.mark.parametrize("name", GRAPHS)
def test_core_step_vs_oracle(ops, name):
    tgi.core_step_case(ops, name)


# one, two and three waves (with two and three, the staging of the four rows' statics wraps around the waves), and two
# tiles, the second with 44 lanes
@pytest.mark.parametrize("B", [5, 70, 130, 300])
@pytest.mark.parametrize("name", GRAPHS)
def test_fused_frame_vs_per_op_kernels(ops, name, B):
    tgi.fused_frame_case(ops, name, B, 45)


@pytest.mark.parametrize("name", GRAPHS)
def test_fused_frame_breaks_ties_like_the_per_op_kernels(ops, name):
    tgi.fused_tie_case(ops, name)


@pytest.mark.parametrize("B", [5, 130])
@pytest.mark.parametrize("name", GRAPHS)
def test_rollouts_equal_the_frame_loop(ops, monkeypatch, name, B):
    tgi.rollout_case(ops, monkeypatch.setenv, name, B, 40)


# ---- what every child process runs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def case_frames(ops, name):
    tgi.fused_frame_case(ops, name, 130, 45)


@pytest.mark.parametrize("name", GRAPHS)
def case_rollout(ops, monkeypatch, name):
    tgi.rollout_case(ops, monkeypatch.setenv, name, 5, 40)


KNOBS = ("TARL_DIR_WORDS", "TARL_DIR_SIBLINGS", "TARL_CHOICE_QUAD", "TARL_ADDR32")
CHILDREN = ["TARL_DIR_WORDS=0", "TARL_DIR_WORDS=5", "TARL_DIR_SIBLINGS=0,TARL_CHOICE_QUAD=0", "TARL_ADDR32=0"]
CASES = 4


@pytest.mark.parametrize("knobs", CHILDREN)
def test_under_developer_knobs(knobs):
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(kv.split("=") for kv in knobs.split(","))
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-o", "python_functions=case_*",
                        os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"{CASES} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
