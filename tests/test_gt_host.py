"""CPU: the graph-transformer head (policy_head = "graph_transformer") — the restatement against the reference's golden,
the positional-encoding helper, the CLI choice, the kernel-order key lists and the other heads' unchanged defaults."""
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

sys.path.insert(0, PKG)
import gt_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def g():
    z = np.load(f"{ROOT}/tests/golden/gt_policy.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _sd(g, prefix="sd/"):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def test_restatement_reproduces_the_reference_logits_and_gradients(g):
    sd = _sd(g)
    ei, ea, pe = g["edge_index"], g["edge_attr"], g["pe"]
    ls = R.gt_logits(sd, g["x_single"], ei, ea, pe)
    assert float((ls - g["logits_single"]).abs().max()) <= 1e-6 * float(g["logits_single"].abs().max())
    p = {k: (v.clone().requires_grad_(True) if "running" not in k and v.is_floating_point() else v) for k, v in sd.items()}
    lb = R.gt_logits(p, g["x_batch"], ei, ea, pe)
    assert float((lb.detach() - g["logits_batch"]).abs().max()) <= 1e-6 * float(g["logits_batch"].abs().max())
    (g["coef"] * lb).sum().backward()
    grads = _sd(g, "grad/")
    assert len(grads) == sum(1 for k in sd if "running" not in k and "num_batches" not in k)
    for k, ref in grads.items():
        mine = p[k].grad if p[k].grad is not None else torch.zeros_like(ref)
        scale = max(float(ref.abs().max()), 1.0)
        assert float((mine - ref).abs().max()) <= 1e-5 * scale, k
    # the parameters that do not reach the logits get no gradient from the reference either
    for k in ("gt_layers.1.WV.weight", "gt_layers.1.n_gate.weight", "gt_layers.0.e_gate.weight", "mu_mlp.mlp.0.weight"):
        assert float(grads[k].abs().max()) == 0.0, k


def test_kernel_order_keys_cover_exactly_the_live_tensors(g):
    from tarl_hip import ops
    sd = _sd(g)
    assert len(ops.GT_PARAM_KEYS) == 46 and len(ops.GT_BUFFER_KEYS) == 12
    assert all(k in sd for k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS)
    live = {k for k, v in _sd(g, "grad/").items() if float(v.abs().max()) > 0}
    assert live <= set(ops.GT_PARAM_KEYS)
    text = open(f"{ROOT}/include/tarl_hip.h").read()
    assert "#define TARL_GT_NUM_PARAMS 46" in text and "#define TARL_GT_NUM_TENSORS 58" in text


def test_mirror_module_matches_the_reference_tree_and_initialisation(g):
    from src.transformer import GraphTransformerNet
    torch.manual_seed(20261015)
    net = GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4, dropout=0.1)
    init = _sd(g, "init/")
    sd = net.state_dict()
    assert set(sd) == set(init)
    for k, v in init.items():
        assert torch.equal(sd[k], v), k


def _check_pe(ei, n, total):
    from src.transformer import laplacian_pe
    pe, vals = laplacian_pe(ei, n, total, return_eigvals=True)
    assert pe.shape == (total, 16) and pe.dtype == torch.float32
    pe2 = laplacian_pe(ei, n, total)
    assert torch.equal(pe, pe2)                                         # bitwise repeatable
    assert float(pe[n:].abs().max() if total > n else 0.0) == 0.0       # SRC / DEST rows
    k = vals.numel()
    V = pe[:n, :k].double()
    assert torch.allclose(V.norm(dim=0), torch.ones(k, dtype=torch.float64), atol=1e-6)
    idx = V.abs().argmax(0)
    assert bool((V[idx, torch.arange(k)] > 0).all())                    # sign rule
    from src.transformer.encoding import _laplacian
    Lm = _laplacian(ei, n)
    assert float((Lm @ V - V * vals[:k]).abs().max()) <= 1e-6     # eigen-residual of the stored (float32) columns
    return vals


def test_positional_encoding_helper(g):
    from tarl_hip import synth
    net = synth.torus_network(4, 4, heterogeneous=True, seed=2)
    _check_pe(net.edge_index, net.num_roads, net.num_roads + 3)
    vals = _check_pe(g["pe_graph_edge_index"], int(g["pe_graph_num_roads"]), 24)
    assert torch.allclose(vals, g["pe_eigvals"].double(), atol=1e-8)


def test_cli_and_runner_args_accept_the_graph_transformer_head():
    import main
    from src.runner import RunnerArgs
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "graph_transformer"])
    assert ns.policy_head == "graph_transformer"
    assert RunnerArgs(**vars(ns)).policy_head == "graph_transformer"


def test_policy_net_defaults_and_other_heads_state_dicts_unchanged():
    from src.agents.mpnn_agent import MPNNPolicyNet
    assert MPNNPolicyNet.policy_head == "embedding" and MPNNPolicyNet.prior_weight == 1.0
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    pol = MPNNPolicyNet(ei, 3, None, device="cpu")
    assert not hasattr(pol, "transformer") or pol.transformer is None
    assert sorted(pol.state_dict()) == sorted(
        ["nodes_embedding.weight"] + [f"edge_mlp_test.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
        + [f"edge_mlp.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")])


def test_sparse_positional_encoding_path_agrees_with_the_dense_one(monkeypatch):
    """Above DENSE_LIMIT roads the encoding comes from scipy's eigsh in shift-invert mode: same eigenvalues, and the same
    checks (unit columns, sign rule, residual, zero SRC / DEST rows), here with the limit lowered onto a 12 x 9 torus."""
    from src.transformer import encoding
    from tarl_hip import synth
    net = synth.torus_network(12, 9, heterogeneous=True, seed=1)
    n = net.num_roads
    _, dense = encoding.laplacian_pe(net.edge_index, n, n + 4, return_eigvals=True)
    monkeypatch.setattr(encoding, "DENSE_LIMIT", 16)
    sparse = _check_pe(net.edge_index, n, n + 4)
    assert torch.allclose(sparse, dense, atol=1e-9)


def test_positional_encoding_cache_is_keyed_by_the_graph(tmp_path):
    """A cached encoding is reused only for the graph it was computed for: another network with the same node count
    under the same scenario directory is recomputed, not served stale."""
    from src.transformer import cached_laplacian_pe, laplacian_pe
    from tarl_hip import synth
    a = synth.torus_network(6, 4, heterogeneous=True, seed=1)
    b = synth.torus_network(4, 6, heterogeneous=True, seed=1)
    assert a.num_roads == b.num_roads and not torch.equal(a.edge_index, b.edge_index)
    pa = cached_laplacian_pe(a.edge_index, a.num_roads, a.num_roads, str(tmp_path))
    assert torch.equal(cached_laplacian_pe(a.edge_index, a.num_roads, a.num_roads, str(tmp_path)), pa)
    pb = cached_laplacian_pe(b.edge_index, b.num_roads, b.num_roads, str(tmp_path))
    assert torch.equal(pb, laplacian_pe(b.edge_index, b.num_roads, b.num_roads))
    assert not torch.equal(pa, pb)


def test_term_magnitudes_bound_the_gradients(g):
    """The restatement's per-parameter sum of |terms| (the scale of a summed gradient's rounding) is >= |gradient|."""
    sd = _sd(g)
    p = {k: (v.double().requires_grad_(True) if "running" not in k and v.is_floating_point() else v.double())
         for k, v in sd.items() if "num_batches" not in k}
    cap = []
    lb = R.gt_logits(p, g["x_batch"].double(), g["edge_index"], g["edge_attr"].double(), g["pe"].double(), capture=cap)
    (g["coef"].double() * lb).sum().backward()
    S = R.term_magnitudes(cap)
    from tarl_hip import ops
    assert set(ops.GT_PARAM_KEYS) <= set(S)
    for k in ops.GT_PARAM_KEYS:
        assert bool((p[k].grad.abs() <= S[k].view_as(p[k].grad) * (1 + 1e-12)).all()), k
