"""Writes tests/golden/gt_value.npz from the reference's own GraphTransformerNet (src/transformer/model.py, unchanged),
called as ValueNet (src/agents/transformer_agent.py:257-308) calls it: batched node blocks, the per-sample batch index and
offset edge indices, the node output ``mu_mlp(global_pool(x2, batch))`` (raw=True).

Runs on a development host that has the reference tree (``--ref``, default ../reference); never on the GPU machine. The PyG
stand-ins are those of tools/make_gt_golden.py. Content: a heterogeneous 3 x 3 torus at M = 3, random BatchNorm statistics,
gamma / beta and biases, the values, and the autograd gradients of sum(coef * value) for every parameter (zeros where
autograd gives None).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_gt_golden import _load_reference, _register_pyg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden", "gt_value.npz"))
    a = ap.parse_args()
    _register_pyg()
    mods = _load_reference(os.path.abspath(a.ref))
    torch.manual_seed(20261016)
    net = mods["model"].GraphTransformerNet(node_dim_in=16, edge_dim_in=1, pe_in_dim=16, hidden_dim=16, gate=True,
                                            num_gt_layers=2, num_heads=4, dropout=0.1)
    g = torch.Generator().manual_seed(11)
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
    edge_attr = (torch.rand(E, 1, generator=g) * 2.0 + 0.1)
    pe = torch.randn(N, 16, generator=g) * 0.5
    xb = torch.randn(M, N, 16, generator=g)
    coef = torch.randn(M, generator=g)
    # batched as ValueNet.forward does (transformer_agent.py:283-307): node blocks, shifted edge indices, repeated PE,
    # batch index per node
    inc = (torch.arange(M).repeat_interleave(E) * N).repeat(2, 1)
    net.zero_grad()
    vb, _ = net(x=xb.reshape(-1, 16), edge_index=ei.repeat(1, M) + inc, edge_attr=edge_attr.repeat(M, 1),
                pe=pe.repeat(M, 1), batch=torch.arange(M).repeat_interleave(N))
    assert tuple(vb.shape) == (M, 1)
    vb = vb.view(M)
    (coef * vb).sum().backward()
    out = {"edge_index": ei.numpy(), "edge_attr": edge_attr.numpy(), "pe": pe.numpy(), "x_batch": xb.numpy(),
           "value_batch": vb.detach().numpy(), "coef": coef.numpy()}
    for k, v in net.state_dict().items():
        out["sd/" + k] = v.detach().numpy()
    for k, p in net.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {len(out)} arrays")


if __name__ == "__main__":
    main()
