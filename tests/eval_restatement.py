"""TEST INFRASTRUCTURE: numpy restatement of what ``tarl_episode_summary`` and ``tarl_hip.evaluator`` report, from plain
agent tables and per-frame rewards (reference: src/runner.py:147-150 — arrived = DONE == 1, travel time = ARRIVAL_TIME -
DEPARTURE_TIME; src/rl/ppo_trainer.py:89-127 — return = sum of the rewards), and host-side helpers to decode action bytes."""
import math

import numpy as np
import torch

ON_WAY, DONE, DEP, ARR = 7, 8, 2, 3


def summary(agents, reward, bin_width, num_bins):
    """``agents`` (B, A, 9) fp32, ``reward`` (T, B) fp32 or None -> dict of numpy arrays shaped like the kernel's outputs.
    Sums in float64 over float32 differences, the histogram bin from the float32 quotient (as the kernel forms it)."""
    ag = np.asarray(agents, dtype=np.float32)[:, 1:]                # row 0: the dummy
    B = ag.shape[0]
    counts = np.zeros((B, 3), dtype=np.int32)
    sums = np.zeros((B, 3), dtype=np.float64)
    hist = np.zeros((B, num_bins), dtype=np.int32)
    for b in range(B):
        done = ag[b, :, DONE] == 1
        way = (~done) & (ag[b, :, ON_WAY] == 1)
        counts[b] = [done.sum(), way.sum(), (~done & ~way).sum()]
        tt = (ag[b, done, ARR] - ag[b, done, DEP]).astype(np.float32)
        if tt.size:
            d = tt.astype(np.float64)
            sums[b] = [d.sum(), (d * d).sum(), d.max()]
            q = np.floor(tt / np.float32(bin_width))
            bins = np.where(q >= 0, np.minimum(q, num_bins - 1), 0).astype(np.int64)
            hist[b] = np.bincount(bins, minlength=num_bins)
    ret = (np.zeros(B) if reward is None else np.asarray(reward, dtype=np.float64).sum(axis=0))
    return {"counts": counts, "sums": sums, "hist": hist, "episode_return": ret}


def per_env(s, bin_width):
    """The per-environment figures of EvalResult from :func:`summary`'s arrays (the evaluator's own formulas restated)."""
    out = []
    for b in range(s["counts"].shape[0]):
        n = int(s["counts"][b, 0])
        row = dict(arrived=n, on_way=int(s["counts"][b, 1]), not_departed=int(s["counts"][b, 2]),
                   episode_return=float(s["episode_return"][b]), avg=None, std=None, max=None, p50=None, p95=None)
        if n:
            mean = float(s["sums"][b, 0]) / n
            cum = np.cumsum(s["hist"][b])

            def pct(q):
                rank = max(1, math.ceil(q * n - 1e-9))                # the sample of rank ceil(q n)
                return float((int(np.searchsorted(cum, rank, side="left")) + 1) * bin_width)
            row.update(avg=mean, std=math.sqrt(max(0.0, float(s["sums"][b, 1]) / n - mean * mean)),
                       max=float(s["sums"][b, 2]), p50=pct(0.5), p95=pct(0.95))
        out.append(row)
    return out


def csr(edge_index, N):
    """Host CSR of the plan: rank r of node i names edge out_eid[out_ptr[i] + r] (stable order of edge_index[0])."""
    src = edge_index[0]
    out_eid = torch.argsort(src, stable=True)
    out_ptr = torch.zeros(N + 1, dtype=torch.long)
    out_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    return out_ptr, out_eid


def rank_bytes(choice, edge_index, N):
    """Edge ids (B, N) int (-1: none) -> rank bytes (B, N) uint8, 0x80 where nothing was chosen (any device)."""
    out_ptr, out_eid = csr(edge_index.cpu(), N)
    E = edge_index.size(1)
    rank_of_edge = torch.empty(E, dtype=torch.long)
    rank_of_edge[out_eid] = torch.arange(E) - out_ptr[:-1][edge_index[0].cpu()[out_eid]]
    rank_of_edge = rank_of_edge.to(choice.device)
    c = choice.long()
    return torch.where(c >= 0, rank_of_edge[c.clamp(min=0)], torch.full_like(c, 0x80)).to(torch.uint8)


def edges_of_bytes(code, edge_index, N):
    """Rank bytes (N,) -> chosen edge ids (N,) long, -1 where bit 7 is set."""
    out_ptr, out_eid = csr(edge_index.cpu(), N)
    code = code.cpu().long()
    drew = (code & 0x80) == 0
    e = torch.full((N,), -1, dtype=torch.long)
    e[drew] = out_eid[out_ptr[:-1][drew] + code[drew]]
    return e
