"""Writes tests/golden/gt_policy.npz from the reference's own GraphTransformerNet (src/transformer/model.py, unchanged).

Runs on a development host that has the reference tree (``--ref``, default ../reference); never on the GPU machine. The
PyG symbols the model imports are registered here as plain-torch stand-ins (torch-geometric 2.5 semantics):
MessagePassing.propagate (source_to_target gathers, ``index`` passed to message, sum aggregation), utils.softmax (group
max subtracted, + 1e-16), nn.aggr.MultiAggregation(['sum']), nn.resolver.activation_resolver, data.Batch,
utils.to_scipy_sparse_matrix / degree. Content: a heterogeneous 3 x 3 torus, unbatched and batched (M = 3) inputs, random
BatchNorm statistics, gamma / beta and biases, logits, autograd gradients of sum(coef * logits) for every parameter (zeros
where autograd gives None), and the eigenvalues of the reference's positional-encoding procedure on a small irregular graph.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _register_pyg():
    import inspect

    pyg = types.ModuleType("torch_geometric")
    nn_ = types.ModuleType("torch_geometric.nn")
    aggr = types.ModuleType("torch_geometric.nn.aggr")
    resolver = types.ModuleType("torch_geometric.nn.resolver")
    utils = types.ModuleType("torch_geometric.utils")
    data = types.ModuleType("torch_geometric.data")

    class MultiAggregation(torch.nn.Module):
        def __init__(self, aggrs, mode="cat"):
            super().__init__()
            assert list(aggrs) == ["sum"]

        def forward(self, x, index=None, dim_size=None, dim=0):
            if index is None:
                return x.sum(dim=dim, keepdim=True)
            n = int(dim_size) if dim_size is not None else int(index.max()) + 1
            return torch.zeros((n,) + x.shape[1:], dtype=x.dtype).index_add(0, index, x)

    class MessagePassing(torch.nn.Module):
        def __init__(self, aggr="add", flow="source_to_target", node_dim=-2, **kw):
            super().__init__()
            self.aggr_module = aggr
            self.node_dim = node_dim

        def propagate(self, edge_index, size=None, **kwargs):
            j, i = edge_index[0], edge_index[1]
            n = None
            args = {}
            for name in inspect.signature(self.message).parameters:
                if name.endswith("_i") or name.endswith("_j"):
                    t = kwargs[name[:-2]]
                    n = t.size(0)
                    args[name] = t.index_select(0, i if name.endswith("_i") else j)
                elif name == "index":
                    args[name] = i
                elif name in kwargs:
                    args[name] = kwargs[name]
            msg = self.message(**args)
            return self.aggr_module(msg, i, dim_size=n)

    def softmax(src, index, num_nodes=None):
        n = int(num_nodes) if num_nodes is not None else int(index.max()) + 1
        shape = (n,) + src.shape[1:]
        idx = index.view((-1,) + (1,) * (src.dim() - 1)).expand_as(src)
        mx = torch.full(shape, float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src.detach(), "amax",
                                                                             include_self=True)
        out = (src - mx.index_select(0, index)).exp()
        s = torch.zeros(shape, dtype=src.dtype).index_add(0, index, out) + 1e-16
        return out / s.index_select(0, index)

    def activation_resolver(name, **kw):
        assert name == "relu"
        return torch.nn.ReLU()

    def to_scipy_sparse_matrix(edge_index, edge_attr=None, num_nodes=None):
        import scipy.sparse as sp
        ei = edge_index.numpy()
        return sp.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(num_nodes, num_nodes))

    def degree(index, num_nodes=None, dtype=None):
        return torch.zeros(num_nodes, dtype=dtype).index_add(0, index, torch.ones(index.numel(), dtype=dtype))

    class Batch:
        pass

    class Data:
        pass

    aggr.MultiAggregation = MultiAggregation
    nn_.MessagePassing = MessagePassing
    nn_.aggr, nn_.resolver = aggr, resolver
    resolver.activation_resolver = activation_resolver
    utils.softmax, utils.to_scipy_sparse_matrix, utils.degree = softmax, to_scipy_sparse_matrix, degree
    data.Batch, data.Data = Batch, Data
    pyg.nn, pyg.utils, pyg.data = nn_, utils, data
    for m in (pyg, nn_, aggr, resolver, utils, data):
        sys.modules[m.__name__] = m


def _load_reference(ref):
    pkg = types.ModuleType("reftransformer")
    pkg.__path__ = [os.path.join(ref, "src", "transformer")]
    sys.modules["reftransformer"] = pkg
    mods = {}
    for name in ("mlp", "gt_conv", "model"):
        spec = importlib.util.spec_from_file_location(f"reftransformer.{name}", os.path.join(ref, "src", "transformer",
                                                                                             name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def _reference_pe_eigvals(edge_index, num_nodes):
    """The procedure of MLAgents.compute_encodings (transformer_agent.py:165-178): eigenvalues kept."""
    from scipy.sparse import csgraph
    from scipy.sparse.linalg import eigsh
    A = sys.modules["torch_geometric.utils"].to_scipy_sparse_matrix(edge_index, None, num_nodes)
    A = (A + A.T) / 2
    L = csgraph.laplacian(A, normed=True)
    vals, _ = eigsh(L, k=min(16 + 5, num_nodes - 1), which="SM", v0=np.ones(num_nodes) / np.sqrt(num_nodes), tol=1e-12)
    vals = np.sort(vals)
    return vals[vals > 1e-5][:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "gt_policy.npz"))
    a = ap.parse_args()
    _register_pyg()
    mods = _load_reference(os.path.abspath(a.ref))
    torch.manual_seed(20261015)
    net = mods["model"].GraphTransformerNet(node_dim_in=16, edge_dim_in=1, pe_in_dim=16, hidden_dim=16, gate=True,
                                            num_gt_layers=2, num_heads=4, dropout=0.1)
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():          # non-trivial BN statistics, gamma / beta and biases
        for name, mod in net.named_modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(16, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(16, generator=g) * 1.5 + 0.25)
                mod.weight.copy_(1.0 + 0.3 * torch.randn(16, generator=g))
                mod.bias.copy_(0.2 * torch.randn(16, generator=g))
            elif isinstance(mod, torch.nn.Linear) and mod.bias is not None:
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
    net.eval()
    W = H = 3
    src, dst = [], []
    for i in range(H):
        for j in range(W):
            for di, dj in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                src.append(i * W + j)
                dst.append(((i + di) % H) * W + (j + dj) % W)
    ei = torch.tensor([src, dst], dtype=torch.int64)
    N, E, M = W * H, ei.size(1), 3
    edge_attr = (torch.rand(E, 1, generator=g) * 2.0 + 0.1)                   # heterogeneous lengths
    pe = torch.randn(N, 16, generator=g) * 0.5
    xs = torch.randn(N, 16, generator=g)
    xb = torch.randn(M, N, 16, generator=g)
    _, ls = net(x=xs, edge_index=ei, edge_attr=edge_attr, pe=pe, batch=None)
    # batched as MLAgents.forward does (transformer_agent.py:75-107): node blocks, shifted edge indices, repeated PE
    inc = (torch.arange(M).repeat_interleave(E) * N).repeat(2, 1)
    coef = torch.randn(M, E, generator=g)
    net.zero_grad()
    _, lb = net(x=xb.reshape(-1, 16), edge_index=ei.repeat(1, M) + inc, edge_attr=edge_attr.repeat(M, 1),
                pe=pe.repeat(M, 1), batch=torch.arange(M).repeat_interleave(N))
    lb = lb.view(M, E)
    (coef * lb).sum().backward()
    out = {"edge_index": ei.numpy(), "edge_attr": edge_attr.numpy(), "pe": pe.numpy(), "x_single": xs.numpy(),
           "x_batch": xb.numpy(), "logits_single": ls.detach().numpy(), "logits_batch": lb.detach().numpy(),
           "coef": coef.numpy()}
    for k, v in net.state_dict().items():
        out["sd/" + k] = v.detach().numpy()
        out["init/" + k] = init[k].numpy()
    for k, p in net.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    # the positional-encoding procedure on a small irregular graph (two roads joined by a chain and a chord)
    pe_src = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 0, 5, 9, 13, 17, 2, 20]
    pe_dst = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 12, 18, 3, 22, 7, 15, 1]
    pei = torch.tensor([pe_src, pe_dst], dtype=torch.int64)
    out["pe_graph_edge_index"] = pei.numpy()
    out["pe_graph_num_roads"] = np.array(24)
    out["pe_eigvals"] = _reference_pe_eigvals(pei, 24)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {len(out)} arrays")


if __name__ == "__main__":
    main()
