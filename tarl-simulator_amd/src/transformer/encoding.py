"""Positional encoding of MLAgents.compute_encodings (src/agents/transformer_agent.py:153-200), made deterministic.

Symmetrised road adjacency -> normalised Laplacian -> the 16 eigenvectors of smallest eigenvalue above 1e-5, each column
normalised; rows of the nodes past ``num_roads`` (SRC / DEST) are zero. On degenerate spectra (tori) the eigenvectors
depend on the solver, so the encoding is computed once per graph here (dense float64 eigh up to 8192 roads, scipy's
eigsh above), each column's sign fixed (largest-magnitude entry positive), cached, and carried in the checkpoint.

Cost: the dense path is O(n^3) (8192 roads: a few seconds). Above it, eigsh runs in shift-invert mode just below 0
(sigma = -1e-3: L - sigma I is positive definite; one sparse LU factorisation, then a few dozen solves) instead of
which='SM' on the Laplacian itself, whose iteration count is unbounded on large graphs.
"""
from __future__ import annotations

import os

import torch

DENSE_LIMIT = 8192


def _laplacian(edge_index, n):
    A = torch.zeros((n, n), dtype=torch.float64)
    ei = edge_index.to("cpu", torch.int64)
    keep = (ei[0] < n) & (ei[1] < n)
    A.index_put_((ei[0][keep], ei[1][keep]), torch.ones(int(keep.sum()), dtype=torch.float64), accumulate=True)
    A = (A + A.t()) / 2
    deg = A.sum(1)
    dinv = torch.where(deg > 0, deg.rsqrt(), torch.zeros_like(deg))
    L = -dinv[:, None] * A * dinv[None, :]
    L.diagonal().add_(torch.where(deg > 0, 1.0, 0.0).to(torch.float64))
    return L


def laplacian_pe(edge_index, num_roads, total_nodes=None, dim=16, return_eigvals=False):
    """(total_nodes, dim) float32 encoding (zero-padded columns when fewer than ``dim`` non-trivial eigenvalues)."""
    n = int(num_roads)
    total = int(total_nodes) if total_nodes is not None else n
    if n <= DENSE_LIMIT:
        vals, vecs = torch.linalg.eigh(_laplacian(edge_index, n))
    else:
        try:
            import numpy as np
            import scipy.sparse as sp
            from scipy.sparse.csgraph import laplacian
            from scipy.sparse.linalg import eigsh
        except ImportError as exc:
            raise RuntimeError(f"positional encoding of {n} roads needs scipy (dense limit {DENSE_LIMIT})") from exc
        ei = edge_index.cpu().numpy()
        keep = (ei[0] < n) & (ei[1] < n)
        A = sp.coo_matrix((np.ones(int(keep.sum())), (ei[0][keep], ei[1][keep])), shape=(n, n)).tocsr()
        Lm = laplacian((A + A.T) / 2, normed=True)
        v, w = eigsh(Lm.tocsc(), k=min(dim + 5, n - 1), sigma=-1e-3, which="LM", v0=np.ones(n) / np.sqrt(n), tol=1e-10)
        order = np.argsort(v, kind="stable")
        vals, vecs = torch.from_numpy(v[order]), torch.from_numpy(w[:, order])
    mask = vals > 1e-5
    vals, vecs = vals[mask][:dim], vecs[:, mask][:, :dim]
    vecs = (vecs / torch.linalg.norm(vecs, dim=0, keepdim=True)).to(torch.float32)
    idx = vecs.abs().argmax(0)         # on the stored float32 values: the first of tied magnitudes
    sign = torch.sign(vecs[idx, torch.arange(vecs.size(1))])
    vecs = vecs * torch.where(sign == 0, 1.0, sign)
    pe = torch.zeros((total, dim), dtype=torch.float32)
    pe[:n, :vecs.size(1)] = vecs
    return (pe, vals) if return_eigvals else pe


def graph_fingerprint(edge_index, num_roads, total_nodes, dim=16):
    """sha256 of what the encoding depends on: the edges, the road and node counts, the width."""
    import hashlib
    h = hashlib.sha256()
    h.update(f"{int(num_roads)}:{int(total_nodes)}:{int(dim)}:".encode())
    h.update(edge_index.detach().to("cpu", torch.int64).contiguous().numpy().tobytes())
    return h.hexdigest()


def cached_laplacian_pe(edge_index, num_roads, total_nodes, cache_dir=None, dim=16):
    """:func:`laplacian_pe` cached as ``<cache_dir>/gt_pe.pt`` with the :func:`graph_fingerprint` it was computed for; a
    cache made for another graph (a changed network under the same scenario name) is recomputed and overwritten."""
    path = os.path.join(cache_dir, "gt_pe.pt") if cache_dir else None
    fp = graph_fingerprint(edge_index, num_roads, total_nodes, dim)
    if path and os.path.exists(path):
        rec = torch.load(path, map_location="cpu")
        if isinstance(rec, dict) and rec.get("fingerprint") == fp:
            return rec["pe"]
    pe = laplacian_pe(edge_index, num_roads, total_nodes, dim)
    if path:
        try:
            os.makedirs(cache_dir, exist_ok=True)
            torch.save({"fingerprint": fp, "pe": pe}, path)
        except OSError:
            pass
    return pe
