"""CPU: the graph-transformer critic (value_head = "graph_transformer") — the restatement against the reference's golden,
which parameters reach the value, the unbatched call, the kernel-order key lists, and the CLI / trainer plumbing."""
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

sys.path.insert(0, PKG)
import gt_value_restatement as RV  # noqa: E402

EDGE_SIDE = ("edge_emb.", ".WE.", ".WOe.", ".ffn_e.", ".norm1e.", ".norm2e.", ".e_gate.", "edge_linear.", "log_var_mlp.")


@pytest.fixture(scope="module")
def g():
    z = np.load(f"{ROOT}/tests/golden/gt_value.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def _sd(g, prefix="sd/"):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def _params(sd, dtype=torch.float32):
    return {k: (v.to(dtype).requires_grad_(True) if "running" not in k and v.is_floating_point() else v.to(dtype))
            for k, v in sd.items() if "num_batches" not in k}


def test_restatement_reproduces_the_reference_values_and_gradients(g):
    p = _params(_sd(g))
    vb = RV.gt_value(p, g["x_batch"], g["edge_index"], g["pe"])
    assert vb.shape == g["value_batch"].shape
    assert float((vb.detach() - g["value_batch"]).abs().max()) <= 1e-5 * max(float(g["value_batch"].abs().max()), 1.0)
    (g["coef"] * vb).sum().backward()
    grads = _sd(g, "grad/")
    assert len(grads) == sum(1 for k in p if "running" not in k)
    for k, ref in grads.items():
        mine = p[k].grad if p[k].grad is not None else torch.zeros_like(ref)
        assert float((mine - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1.0), k


def test_exactly_the_edge_side_gets_zero_gradients(g):
    from tarl_hip import ops
    grads = _sd(g, "grad/")
    zero = {k for k, v in grads.items() if float(v.abs().max()) == 0.0}
    edge = {k for k in grads if any(s in "." + k for s in EDGE_SIDE)}
    assert zero == edge and len(edge) > 0
    assert set(grads) - edge == set(ops.GT_VALUE_PARAM_KEYS)


def test_kernel_order_keys_and_header(g):
    from tarl_hip import ops
    sd = _sd(g)
    assert len(ops.GT_VALUE_PARAM_KEYS) == 36 and len(ops.GT_VALUE_BUFFER_KEYS) == 8
    assert len(set(ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)) == 44
    assert all(k in sd for k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)
    assert not any(any(s in "." + k for s in EDGE_SIDE) for k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)
    text = open(f"{ROOT}/include/tarl_hip.h").read()
    assert "#define TARL_GTV_NUM_PARAMS 36" in text and "#define TARL_GTV_NUM_TENSORS 44" in text
    assert "#define TARL_ABI_VERSION 5" in text


def test_unbatched_call_is_the_batched_one_at_m1(g):
    """The reference's unbatched branch raises UnboundLocalError (edge_index / positional_embedding never bound); the
    mirror's uses the module's own edge index and encoding, i.e. the batched path with M = 1."""
    p = _params(_sd(g), torch.float64)
    x = g["x_batch"][1].double()
    single = RV.gt_value(p, x, g["edge_index"], g["pe"].double())
    batched = RV.gt_value(p, x.unsqueeze(0), g["edge_index"], g["pe"].double())
    assert single.dim() == 0 and batched.shape == (1,)
    assert torch.equal(single, batched[0])
    ref = RV.gt_value(p, g["x_batch"].double(), g["edge_index"], g["pe"].double())[1]
    assert float((single - ref).abs().detach()) <= 1e-12 * max(1.0, float(ref.abs().detach()))


def test_value_net_module_tree_and_refusals():
    from src.agents.transformer_agent import ValueNet
    from tarl_hip import ops
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    torch.manual_seed(3)
    v = ValueNet(ei, 3, "cpu", torch.zeros(3, 16))
    assert not v.training and not v.transformer.training
    sd = v.state_dict()
    assert "gt_pe" in sd and all("transformer." + k in sd for k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)
    assert set(v.kernel_tensors()) == set(ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)
    with pytest.raises(ValueError, match="pe must be"):
        ValueNet(ei, 3, "cpu", torch.zeros(4, 16))
    v.train()
    with pytest.raises(Exception):       # CPU tensors are refused before anything else; training mode on the GPU
        v(torch.zeros(3, 7), torch.zeros(3, 1), torch.zeros(3, dtype=torch.int64), torch.zeros(1))


def test_cli_parses_the_value_head_and_refuses_it_behind_the_embedding_head():
    import main
    from src.runner import RunnerArgs
    p = main.build_parser()
    ns = p.parse_args(["--algo", "mpnn+ppo", "--mode", "train"])
    assert ns.value_head == "simple" and RunnerArgs(**vars(ns)).value_head == "simple"
    assert RunnerArgs(algo="mpnn+ppo", scenario="x", mode="train").value_head == "simple"
    ns = p.parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "graph_transformer", "--value-head",
                       "graph_transformer"])
    assert RunnerArgs(**vars(ns)).value_head == "graph_transformer"
    for head in ("edge_mlp", "embedding_dijkstra"):
        assert RunnerArgs(**vars(p.parse_args(["--policy-head", head, "--value-head", "graph_transformer"]))).value_head \
            == "graph_transformer"
    with pytest.raises(SystemExit):
        p.parse_args(["--value-head", "mpnn"])
    with pytest.raises(ValueError, match="state-dependent policy head"):
        main.main(["--algo", "mpnn+ppo", "--mode", "train", "--policy-head", "embedding", "--value-head",
                   "graph_transformer"])


def _capture_trainer_args(monkeypatch, value_net):
    """ppo_train up to the trainer's construction, with the engine and the trainer replaced by recorders."""
    from src.agents.mpnn_agent import MPNNPolicyNet
    from src.rl import ppo_trainer
    from tarl_hip import engine, ops, trainer
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        raise Stop

    monkeypatch.setattr(trainer, "VecPPOTrainer", fake_trainer)
    monkeypatch.setattr(engine, "SimEngine", lambda *a, **k: types.SimpleNamespace(B=1))
    monkeypatch.setattr(ops, "fused_path_supported", lambda *a: True)
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    graph = types.SimpleNamespace(x=torch.zeros(3, 10), edge_index=ei, edge_attr=torch.ones(3, 1))
    sim = types.SimpleNamespace(graph=graph, Nmax=1, agent=types.SimpleNamespace(agent_features=None), timestep=1)
    pol = MPNNPolicyNet(ei, 3, None, device="cpu")
    with pytest.raises(Stop):
        ppo_trainer.ppo_train(types.SimpleNamespace(simulator=sim), pol, value_net)
    return seen


def test_default_critic_leaves_the_trainer_arguments_unchanged(monkeypatch):
    from src.agents.mpnn_agent import MPNNValueNetSimple
    from src.agents.transformer_agent import ValueNet
    from tarl_hip import ops
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    simple = MPNNValueNetSimple(ei, 3, device="cpu")
    seen = _capture_trainer_args(monkeypatch, simple)
    l = simple.final_mlp
    assert [id(t) for t in seen["args"][2]] == [id(t) for t in (l[0].weight, l[0].bias, l[2].weight, l[2].bias,
                                                                 l[4].weight, l[4].bias)]
    assert not {"value", "gt_value_params", "gt_value_pe"} & set(seen["kw"])
    v = ValueNet(ei, 3, "cpu", torch.zeros(3, 16))
    seen = _capture_trainer_args(monkeypatch, v)
    assert seen["kw"]["value"] == "graph_transformer" and seen["kw"]["gt_value_pe"] is v.gt_pe
    assert [id(t) for t in seen["args"][2]] == [id(t) for t in v.transformer.parameters()]
    assert set(seen["kw"]["gt_value_params"]) == set(ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS)
