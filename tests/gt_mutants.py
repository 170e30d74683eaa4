"""Wrong variants of the graph-transformer restatement (gt_restatement.py, gt_value_restatement.py), selected by name: what
a kernel with one plausible attention bug would compute. Each is a context manager that swaps the restatement's segment
softmax or its gather of K for the time of the ``with`` block; test_gt_attention_host.py measures how far each one moves the
outputs and gradients of the cases the GPU tests run, against the tolerances those tests apply. Nothing here needs a GPU.

  uniform         the scores ignored: alpha = 1 / in-degree
  tail4           the in-edges of CSC in-rank >= 4 (position among the edges with the same target, ascending edge id)
                  dropped from the maximum, the denominator and the aggregate
  reversed        alpha assigned within each segment in reverse order
  no_eps          the + 1e-16 of the denominator left out (a node without in-edges has no alpha at all, so nothing is
                  expected to see it: measured, not required)
  k_by_position   K gathered by the edge's position in source-sorted order instead of by edge_index[0]: the identity on an
                  edge list that is grouped by source, as every torus is
"""
import contextlib

import torch

import gt_restatement as R

NAMES = ("uniform", "tail4", "reversed", "no_eps", "k_by_position")
REQUIRED = ("uniform", "tail4", "reversed", "k_by_position")

_TRUE_SOFTMAX, _TRUE_GATHER = R._segment_softmax, R._gather_k


def _segments(index, N):
    """(order, rank): the edge ids sorted by segment (stable: ascending edge id inside), every edge's rank in its segment."""
    E = index.numel()
    order = torch.argsort(index, stable=True)
    start = torch.zeros(N + 1, dtype=torch.int64, device=index.device)
    start[1:] = torch.cumsum(torch.bincount(index, minlength=N), 0)
    rank = torch.empty(E, dtype=torch.int64, device=index.device)
    rank[order] = torch.arange(E, device=index.device) - start[index[order]]
    return order, rank, start


def _uniform(s, index, N):
    return _TRUE_SOFTMAX(s * 0.0, index, N)


def _tail4(s, index, N):
    _, rank, _ = _segments(index, N)
    keep = (rank < 4).view(1, -1, 1)
    return _TRUE_SOFTMAX(torch.where(keep, s, torch.full_like(s, float("-inf"))), index, N)      # exp(-inf - max) = 0


def _reversed(s, index, N):
    order, rank, start = _segments(index, N)
    mirror = torch.empty_like(order)
    mirror[order] = order[start[index[order]] + start[index[order] + 1] - 1 - torch.arange(order.numel(), device=order.device)]
    return _TRUE_SOFTMAX(s, index, N).index_select(1, mirror)


def _no_eps(s, index, N):
    M, E, H = s.shape
    idx = index.view(1, E, 1).expand(M, E, H)
    mx = torch.full((M, N, H), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(1, idx, s.detach(), "amax")
    w = torch.exp(s - mx.index_select(1, index))
    den = torch.zeros((M, N, H), dtype=s.dtype, device=s.device).index_add(1, index, w)
    return w / den.index_select(1, index)


def _k_by_position(K, u):
    return K.index_select(1, torch.sort(u).values)


_SOFTMAX = {"uniform": _uniform, "tail4": _tail4, "reversed": _reversed, "no_eps": _no_eps}


@contextlib.contextmanager
def mutant(name):
    """The restatements compute the wrong variant ``name`` inside the block."""
    assert name in NAMES, name
    try:
        if name == "k_by_position":
            R._gather_k = _k_by_position
        else:
            R._segment_softmax = _SOFTMAX[name]
        yield
    finally:
        R._segment_softmax, R._gather_k = _TRUE_SOFTMAX, _TRUE_GATHER


def is_identity(name, ei, N):
    """True where the variant is the true function by construction on this graph, so that no case on it can be required to
    see it: ``tail4`` without a node of in-degree above 4, ``k_by_position`` on a source-sorted edge list."""
    if name == "tail4":
        return int(torch.bincount(ei[1], minlength=N).max()) <= 4
    if name == "k_by_position":
        return bool((ei[0][1:] >= ei[0][:-1]).all())
    return False
