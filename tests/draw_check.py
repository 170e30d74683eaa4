"""Exact checks of the live policy's action draw (imported by the replay tests; not a conftest).

The device draws node i's action by inverse CDF over its fp32 threshold table (``eng.tables.thresholds``, plan CSR order,
csrc/fused_choice.hip ``k_policy_tables``): the drawn rank is the number of thresholds in the node's range at or below the
uniform u (``choice_node``: an integer count; ``fused_choice_body`` / ``rollout_env.hip``: the first threshold above u —
the same thing, the thresholds being non-decreasing). The oracle (``oracle/dist.GraphDist.sample``, the reference's
``s < cumsum`` rule) does the same with its own thresholds, computed on the CPU. The two tables are not bit-identical
(GPU ``expf`` against CPU ``exp``, a double running sum against a double cumsum rounded per element), so a uniform that
falls between the two roundings of one boundary draws different edges. Instead of counting such flips against a budget:

* A1 — the device's code byte follows from the device's OWN table and uniform, with no tolerance: rank < degree ->
  code == rank; rank == degree (u beyond the last threshold) -> bit 7 set (the node drew nothing).
* A2 — every device threshold is within ``K`` fp32 ulps of the oracle's, the ulp taken at the oracle's global running sum
  ``S`` before rebasing (the threshold is fp32(run) - fp32(base): its rounding is set by the running sum's magnitude).
* A3 — wherever the oracle's draw and the device's code disagree, every boundary between the two ranks lies between the
  two tables at that u: ``(u >= thr_dev[q]) != (u >= cs_or[q])``.

The plan's CSR order (stable sort of the edges by source) is ``GraphDist``'s sorted order, so both tables are indexed by
the same k. Every node has out-edges here (groups == nodes), as on the torus networks of the replays."""
import torch

CARRIED = 0x80      # bit 7 of a code byte: the node drew nothing and keeps its previous SELECTED_ROAD


def fp32_ulp(x):
    """Spacing of fp32 numbers at |x| (the step to the next representable value above |x|)."""
    a = x.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def ranks(u, thr, ptr):
    """rank[i] = #{q in [ptr[i], ptr[i + 1]) : u[i] >= thr[q]} for per-node uniforms ``u`` (N,) and a CSR table ``thr``."""
    deg = ptr[1:] - ptr[:-1]
    node = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    hit = (u[node] >= thr).long()
    return torch.zeros(deg.numel(), dtype=torch.long).index_add_(0, node, hit)


def code_rank(code, deg):
    """The rank a device code byte claims: the byte itself, or the out-degree where bit 7 says "drew nothing"."""
    code = code.long()
    return torch.where((code & CARRIED) != 0, deg, code)


class DrawCheck:
    """A1-A3 for one live-policy table. ``gd`` the oracle's ``GraphDist`` (unbatched), ``thr_dev`` the device's
    thresholds (E,) in CSR order, ``ptr`` the CSR offsets (N + 1,). A2 is evaluated here, once per table; :meth:`frame`
    runs A1 and A3 on one environment's frame and accumulates the counts the replay reports."""

    def __init__(self, gd, thr_dev, ptr, K=2):
        self.thr = thr_dev.detach().cpu().to(torch.float32)
        self.ptr = ptr.cpu().long()
        self.deg = self.ptr[1:] - self.ptr[:-1]
        assert gd.nb_nodes == self.deg.numel() and bool((self.deg > 0).all()), "every node must have out-edges"
        assert self.thr.shape == gd.cumsum.shape, (tuple(self.thr.shape), tuple(gd.cumsum.shape))
        self.cs = gd.cumsum.detach().to(torch.float32)
        S = torch.cumsum(gd.proba_sort.detach(), dim=-1)           # the oracle's global running sum before rebasing
        self.ulp = fp32_ulp(S)
        self.ulps = (self.thr.double() - self.cs.double()).abs() / self.ulp
        self.max_ulps = float(self.ulps.max())
        self.K = K
        self.draws = self.flips = self.unexplained = self.a1_bad = 0

    def a2_ok(self):
        return self.max_ulps <= self.K

    def a1_mismatches(self, u, code):
        """Nodes whose code byte does not follow from the device's own table at ``u`` (A1)."""
        r = ranks(u, self.thr, self.ptr)
        code = code.long()
        drew = r < self.deg
        bad = torch.where(drew, code != r, (code & CARRIED) == 0)
        return torch.nonzero(bad).flatten()

    def explain(self, u, code):
        """(flipped nodes, unexplained nodes) of A3: nodes where the oracle's rank and the code's rank differ, and those
        of them with a boundary q between the two ranks where both tables put u on the same side."""
        r_or = ranks(u, self.cs, self.ptr)
        r_dev = code_rank(code, self.deg)
        flipped = torch.nonzero(r_or != r_dev).flatten()
        unexplained = []
        for i in flipped.tolist():
            lo, hi = sorted((int(r_or[i]), int(r_dev[i])))
            k = torch.arange(int(self.ptr[i]) + lo, int(self.ptr[i]) + hi)
            if not bool(((u[i] >= self.thr[k]) != (u[i] >= self.cs[k])).all()):
                unexplained.append(i)
        return flipped, torch.tensor(unexplained, dtype=torch.long)

    def frame(self, u, code, what=""):
        """A1 and A3 on one frame of one environment: ``u`` (N,) the exported uniforms, ``code`` (N,) the code bytes."""
        u = u.cpu().to(torch.float32)
        code = code.cpu()
        bad = self.a1_mismatches(u, code)
        self.a1_bad += bad.numel()
        assert bad.numel() == 0, f"A1 {what}: nodes {bad[:8].tolist()} codes {code[bad[:8]].tolist()} do not follow " \
                                 f"from the device's own thresholds"
        flipped, unexplained = self.explain(u, code)
        self.draws += u.numel()
        self.flips += flipped.numel()
        self.unexplained += unexplained.numel()
        assert unexplained.numel() == 0, f"A3 {what}: nodes {unexplained[:8].tolist()} draw another edge than the " \
                                         f"oracle without a threshold rounding between them"
        return flipped.numel()

    def report(self):
        return {"a2_max_ulps": self.max_ulps, "draws": self.draws, "flipped_nodes": self.flips,
                "a1_mismatches": self.a1_bad, "a3_unexplained": self.unexplained}
