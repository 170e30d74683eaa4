"""CPU restatement of the shortest-path tree kernels (csrc/sp_trees.h), shared by test_gpu_msa_trees.py (trees from an
origin), test_gpu_dest_trees.py and test_gpu_prior_dest.py (trees towards a destination) and test_gpu_sp_trees.py: a heapq
Dijkstra over an adjacency list, the documented tie rule of the links, and the checkers of a finished tree / table.

A tree towards a destination is the same computation on the REVERSED adjacency (``adjacency(..., reverse=True)``), so the
reverse variants are these functions with ``reverse=True``. That flag also keeps the sum order each side documents: an
origin's tree accumulates ``dist + w`` (Dijkstra's left-to-right sum), a destination's tree ``w + dist``
(w1 + (w2 + (...))). IEEE addition is commutative, so the two orders give the same bits; the restatement spells each
one out as its kernel's contract states it and does not lean on that."""
import heapq
import math

import torch

INF = math.inf


def adjacency(ei, w, N, reverse=False):
    """Out-edges per node, adj[u] = [(v, w(u,v)), ...]; with ``reverse`` the in-edges, adj[v] = [(u, w(u,v)), ...]."""
    adj = [[] for _ in range(N)]
    for u, v, we in zip(ei[0].tolist(), ei[1].tolist(), w.tolist()):
        if reverse:
            adj[v].append((u, we))
        else:
            adj[u].append((v, we))
    return adj


def _step(d, we, reverse):
    return we + d if reverse else d + we


def cpu_dijkstra(adj, N, root, targets=None, reverse=False):
    """(dist list, link list of the settling relaxation) from ``root`` over ``adj``. Stops early once every node of
    ``targets`` is settled."""
    dist = [INF] * N
    link = [-1] * N
    done = [False] * N
    left = set(targets) if targets is not None else None
    dist[root] = 0.0
    heap = [(0.0, root)]
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        if left is not None:
            left.discard(u)
            if not left:
                break
        for v, we in adj[u]:
            nd = _step(d, we, reverse)
            if nd < dist[v]:
                dist[v] = nd
                link[v] = u
                heapq.heappush(heap, (nd, v))
    return dist, link


def cpu_tie_rule(adj, dist, N, root, reverse=False):
    """BFS levels from ``root`` over the tight edges; link[v] = the smallest u of the previous level with a tight edge
    between u and v: the predecessor in an origin's tree, the next hop in a destination's. -1 at the root and where the BFS
    does not reach."""
    link = [-1] * N
    seen = [False] * N
    seen[root] = True
    level = [root]
    while level:
        best = {}
        for u in level:
            for v, we in adj[u]:
                if not seen[v] and dist[v] < INF and _step(dist[u], we, reverse) == dist[v]:
                    if v not in best or u < best[v]:
                        best[v] = u
        for v, u in best.items():
            seen[v] = True
            link[v] = u
        level = sorted(best)
    return link


def check_tree(ei, w, N, sources, dist, pred):
    """Every reached v != s has a tight predecessor, and the tree reaches s from every reached node within N steps."""
    src, dst = ei[0], ei[1]
    for j, s in enumerate(sources.tolist()):
        d, p = dist[j].cpu(), pred[j].cpu().to(torch.int64)
        reached = torch.isfinite(d)
        assert int(p[s]) == -1 and float(d[s]) == 0.0
        assert bool((p[~reached] == -1).all())
        tight = (p[dst] == src) & (d[src] + w == d[dst])
        has = torch.zeros(N, dtype=torch.bool).index_put_((dst,), tight, accumulate=True)
        need = reached.clone()
        need[s] = False
        assert bool(has[need].all()), f"source {s}: a reached node without a tight predecessor"
        # pointer doubling: after 2^k >= N steps every reached node must sit on s (an acyclic tree rooted at s)
        nxt = torch.where(p >= 0, p, torch.full_like(p, s))
        for _ in range(max(1, math.ceil(math.log2(N))) + 1):
            nxt = nxt[nxt]
        assert bool((nxt[reached] == s).all()), f"source {s}: predecessor walk does not reach the source"


def check_table(ei, w, N, dests, dist, nh, walks=0):
    """Every reachable u != d has its next hop on a tight edge, the table reaches d from every reachable node, and
    (for ``walks`` sampled nodes per destination) the weights collected along the walk, summed in the kernel's order,
    give dist[u] exactly."""
    src, dst = ei[0], ei[1]
    w64 = w.to(torch.float64)
    gen = torch.Generator().manual_seed(3)
    tight_w = {}
    if walks:                                  # only the walks below read it
        for u, v, we in zip(src.tolist(), dst.tolist(), w64.tolist()):
            tight_w.setdefault((u, v), []).append(we)
    steps = max(1, math.ceil(math.log2(N))) + 1
    for j, d in enumerate(dests.tolist()):
        dd, h = dist[j].cpu(), nh[j].cpu().to(torch.int64)
        reached = torch.isfinite(dd)
        assert int(h[d]) == d and float(dd[d]) == 0.0
        assert bool((h[~reached] == -1).all()) and bool((h[reached] >= 0).all())
        tight = (h[src] == dst) & (w64 + dd[dst] == dd[src])
        has = torch.zeros(N, dtype=torch.bool).index_put_((src,), tight, accumulate=True)
        need = reached.clone()
        need[d] = False
        assert bool(has[need].all()), f"destination {d}: a next hop off the tight edges"
        nxt = torch.where(h >= 0, h, torch.full_like(h, d))
        for _ in range(steps):                                 # pointer doubling: 2^steps >= N hops
            nxt = nxt[nxt]
        assert bool((nxt[reached] == d).all()), f"destination {d}: the table does not reach it"
        cand = torch.nonzero(need).view(-1)
        for u in cand[torch.randperm(cand.numel(), generator=gen)[:walks]].tolist():
            ws, node = [], u
            while node != d:
                v = int(h[node])
                ws.append(next(x for x in tight_w[(node, v)] if x + float(dd[v]) == float(dd[node])))
                node = v
            s = 0.0
            for x in reversed(ws):
                s = x + s
            assert s == float(dd[u]), f"walk {u} -> {d}"
