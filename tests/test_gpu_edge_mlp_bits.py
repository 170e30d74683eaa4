"""GPU: the edge-MLP kernels of csrc/edge_mlp.hip give the BITS recorded in tests/golden/edge_mlp_bits.npz — the four forward
paths (fp32 MFMA, x3, bf16 on fp32 rows, bf16 on bf16 rows) and the six gradients of one backward call accumulated onto G0 from
a NaN-filled scratch. The file was written by tools/make_edge_mlp_bits.py from the library as it stood before the kernels were
rebuilt from one shared core: a restructuring of that file that reorders one floating-point operation, or moves one chunk to
another lane, fails here even where it stays inside the tolerances of test_gpu_edge_mlp.py / test_gpu_edge_mlp_bwd.py.

Inputs: ``edge_mlp_restatement.case(E, M)``. Cases: one edge; a full chunk; a one-lane tail chunk; (65, 5), the one case whose
per-sample segments have odd lengths for the two-chunk gather pipeline of the bf16-observation kernel (3, 1, 2, 2, 1, 3, 3
chunks: the pipeline's dead step past the end of a segment); wave ranges that start mid-sample and cross samples."""
import pytest
import torch

import edge_mlp_restatement as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
BITS_CASES = ((1, 1), (32, 3), (33, 7), (65, 5), (185, 5))
FWD_PATHS = ("fp32", "x3", "bf16", "bf16obs")
NAN = float("nan")


def device_bits(E, M):
    """name -> int32 CPU tensor holding the fp32 bit patterns of what the kernels return for ``R.case(E, M)``."""
    from tarl_hip import ops
    c = R.case(E, M)
    plan = ops.Plan(c.edge_index, c.N)
    ec = ops.EdgeConst(c.edge_attr, "cuda")
    w = ops.EdgeMlpWeights(*[t.cuda() for t in c.weights])
    obs = c.obs.cuda()
    out = {}
    for path in FWD_PATHS:
        logits = torch.full((M, E), NAN, device="cuda")
        if path == "bf16obs":
            ops.policy_edge_mlp(plan, obs.to(torch.bfloat16), ec, w, out=logits)
        else:
            ops.policy_edge_mlp(plan, obs, ec, w, precision=path, out=logits)
        out["fwd_" + path] = logits
    grads = [t.cuda() for t in c.G0]
    scratch = torch.full((ops.edge_mlp_bwd_scratch_floats(plan, M),), NAN, device="cuda")
    ops.policy_edge_mlp_bwd(plan, obs, ec, w, c.grad_logits.cuda(), grads, scratch=scratch)
    for name, g in zip(R.GRAD_NAMES, grads):
        out["bwd_" + name] = g
    return {k: v.cpu().contiguous().view(torch.int32).reshape(-1) for k, v in out.items()}


@pytest.mark.parametrize("E,M", BITS_CASES, ids=[R.case_id(c) for c in BITS_CASES])
def test_edge_mlp_bits_are_the_recorded_ones(E, M):
    gold = load_golden("edge_mlp_bits")
    got = device_bits(E, M)
    assert len(got) == len(FWD_PATHS) + len(R.GRAD_NAMES)
    bad = []
    for name, bits in got.items():
        want = gold[f"{R.case_id((E, M))}/{name}"]
        assert want.dtype == torch.int32 and want.shape == bits.shape, name
        assert bool(torch.isfinite(bits.view(torch.float32)).all()), name
        if not torch.equal(bits, want):
            bad.append((name, int((bits != want).sum()), bits.numel()))
    assert not bad, bad
