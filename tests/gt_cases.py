"""Cases shared by the GPU tests of the two graph-transformer networks (test_gpu_gt_head.py, test_gpu_gt_value.py): the
closeness check, the reference's initialisation and scaled random weights, the graphs, observations as the simulator builds
them, the kernels' summation bound and a parameter's span in the trainer's flat gradient."""
import torch


def _close(a, b, what, tol=1e-4):
    scale = max(float(b.abs().max()), 1.0)
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * scale, f"{what}: {err} > {tol} * {scale}"


def _random_state(seed, scale=0.4, critic=False):
    """Scaled random weights: random normal matrices of std 1 / fan-in (node_emb 1e-4 / fan-in: the observations carry raw
    clock times of ~2e4), random biases, BatchNorm gamma / beta and statistics; of the policy head's keys, or the critic's."""
    sd = _reference_state(seed)
    from tarl_hip import ops
    params, buffers = ((ops.GT_VALUE_PARAM_KEYS, ops.GT_VALUE_BUFFER_KEYS) if critic else
                       (ops.GT_PARAM_KEYS, ops.GT_BUFFER_KEYS))
    gen = torch.Generator().manual_seed(seed + 1)
    for k in params:
        if k.endswith("weight") and "norm" not in k:
            sd[k] = torch.randn(sd[k].shape, generator=gen) / sd[k].size(-1) * (1e-4 if k == "node_emb.weight" else 1.0)
        if k.endswith("bias") or "norm" in k:
            sd[k] = sd[k] + scale * torch.randn(sd[k].shape, generator=gen)
    for k in buffers:
        sd[k] = (torch.rand(16, generator=gen) + 0.5) if k.endswith("var") else 0.3 * torch.randn(16, generator=gen)
    return sd


def _reference_state(seed):
    """The reference's initialisation (GraphTransformerNet's construction order and reset_parameters; BatchNorm statistics
    at their defaults), seeded."""
    from src.transformer import GraphTransformerNet
    torch.manual_seed(seed)
    net = GraphTransformerNet(16, 1, 16, 16, gate=True, num_gt_layers=2, num_heads=4, dropout=0.1)
    return {k: v.clone() for k, v in net.state_dict().items()}


def _graph(kind, tmp_path):
    """(edge_index, edge_attr (E, 1), x, Nmax, num_roads, road-graph edge_index) of a torus or of a MATSim grid with SRC /
    DEST pseudo-nodes (SRC: no in-edges, DEST: no out-edges, uneven degrees)."""
    from tarl_hip import synth
    if kind == "matsim":
        from src.matsim_io import build_network
        synth.write_matsim_grid_xml(str(tmp_path / "network.xml"), 4, 6, seed=3)
        g, Nmax = build_network(str(tmp_path / "network"))
        return g.edge_index, g.edge_attr, g.x, Nmax, g.num_roads, g.edge_index_routes
    W, H = {"torus8": (8, 8), "torus16": (16, 16), "config4": (25, 25)}[kind]
    net = synth.torus_network(W, H, heterogeneous=True, seed=W)
    return net.edge_index, net.edge_attr, net.x, net.Nmax, net.num_roads, net.edge_index


def _real_obs(x, Nmax, num_roads, M, seed):
    """Observations as the simulator builds them: the static node columns, counts in [0, MAXN], the head agent's row of a
    synthetic population (raw origin / destination ids and clock-time departure columns)."""
    from tarl_hip import synth
    g = torch.Generator().manual_seed(seed)
    N = x.size(0)
    nf = x[:, 3 * Nmax:3 * Nmax + 7].clone().unsqueeze(0).repeat(M, 1, 1)
    nf[..., 1] = torch.floor(torch.rand((M, N), generator=g) * (nf[..., 0] + 1))
    pop = synth.population(4 * N, num_roads, seed=seed, t0=21540, t1=25200)
    ag = pop[torch.randint(0, pop.size(0), (M, N), generator=g)]
    ag[..., 3] = torch.where(ag[..., 2] < 23000, ag[..., 2] + 600 * torch.rand((M, N), generator=g), torch.zeros(()))
    return torch.cat((nf, ag), dim=-1).contiguous()


def _sum_bound(S, M, items_per_sample):
    """Rounding bound of the kernel's summation of a weight gradient, an fp32 sum of n terms t_i (S = sum |t_i|, from the
    float64 restatement): sequential sums of 1 024-item chunks, then the chunk partials in order, err <= (1024 + chunks) u S
    (u = 2^-24; the classical bound of recursive summation)."""
    chunks = -(-M * items_per_sample // 1024)
    return (1024 + chunks) * 2.0 ** -24 * S


def _span(tr, p):
    off, n = tr.flat.offsets[id(p)]
    return off, off + n
