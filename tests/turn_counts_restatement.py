"""TEST INFRASTRUCTURE: numpy restatement of the per-turn movement counts (``tarl_turn_counts_accumulate``), the crafted
accumulate cases shared by the host and the GPU suite, the same restatement with ONE deliberate defect at a time, and the
oracle replay that yields Direction's own choice per frame and edge. Plain module: no fixtures; nothing at import time
needs a GPU.

Definition: with n_pre[u] the NUMBER_OF_AGENT of road u before frame t (the ``counts`` slice of the frame
before; ``prev_counts``, or 0, for a call's first frame), for every (t, k, u) with ``popped_t[k][u] & 1``:
    not n_pre > 0 (0, -0.0, NaN)                     -> lost[k][h_t][u] += 1          (the phantom pop of quirk Q24)
    r = sel8_t[u][k] & 0x7F < out-degree(u)          -> turns[k][h_t][eid of the r-th out-edge of u] += 1
    otherwise (0x7F, 0x7E, rank >= out-degree)       -> unresolved[k] += 1
h_t = (t0 + t * timestep) // bin_seconds - first_bin: the bin of the clock at which the frame STARTS."""
from __future__ import annotations

import numpy as np
import torch

DEFECTS = ("ignore_n_pre", "same_frame_counts", "sel_of_next_frame", "csr_position", "no_mask_7f", "bin_of_frame_end",
           "popped_untransposed")


def csr(edge_index, N):
    """(out_ptr (N + 1,), out_eid (E,)): every road's out-edges in ascending original edge id, the plan's CSR order."""
    src = np.asarray(edge_index[0], dtype=np.int64)
    out_eid = np.argsort(src, kind="stable").astype(np.int64)
    out_ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=N), out=out_ptr[1:])
    return out_ptr, out_eid


def accumulate(edge_index, N, popped, sel8, counts, prev_counts, turns, lost, unresolved, t0, timestep, bin_seconds,
               first_bin, defect=None):
    """In place: ``turns`` (K, H, E), ``lost`` (K, H, N), ``unresolved`` (K,) int32 += the events of ``popped`` (F, K, N) uint8,
    ``sel8`` (F, N, K) uint8, ``counts`` (F, N, K) fp32 and ``prev_counts`` (N, K) fp32 or None."""
    F, K, _ = popped.shape
    H = turns.shape[1]
    out_ptr, out_eid = csr(edge_index, N)
    deg = np.diff(out_ptr)
    zero = np.zeros((N, K), dtype=np.float32)
    for f in range(F):
        h = (t0 + (f + 1 if defect == "bin_of_frame_end" else f) * timestep) // bin_seconds - first_bin
        if defect == "popped_untransposed":
            pop = popped[f].reshape(-1).reshape(N, K).T & 1            # the bytes read as if they were [N][K]
        else:
            pop = popped[f] & 1                                        # (K, N)
        if defect == "same_frame_counts":
            before = counts[f]
        else:
            before = counts[f - 1] if f > 0 else (zero if prev_counts is None else prev_counts)
        with np.errstate(invalid="ignore"):
            full = (before > 0).T                                      # (K, N); NaN and -0.0 are empty
        if defect == "ignore_n_pre":
            full = np.ones_like(full)
        code = sel8[min(f + 1, F - 1) if defect == "sel_of_next_frame" else f].T.astype(np.int64)      # (K, N)
        if defect != "no_mask_7f":
            code = code & 0x7F
        if not 0 <= h < H:                                             # (only a defect can leave the stored bins)
            continue
        for k, u in zip(*np.nonzero(pop)):
            if not full[k, u]:
                lost[k, h, u] += 1
            elif code[k, u] < deg[u]:
                pos = out_ptr[u] + code[k, u]
                turns[k, h, pos if defect == "csr_position" else out_eid[pos]] += 1
            else:
                unresolved[k] += 1
    return turns, lost, unresolved


# ---- crafted cases -----------------------------------------------------------------------------------------------------------
POPPED_BYTES = np.array([0, 0, 0, 0, 1, 1, 0x02, 0xFE, 0x03, 0xFF], dtype=np.uint8)       # bit 0 alone decides
COUNT_VALUES = np.array([0.0, -0.0, np.nan, 1.0, 14.0, 1.0, 14.0], dtype=np.float32)
DEGREES = (5, 1, 0, 126, 2)       # out-degree of road u: DEGREES[u % 5], the 126 only at road 3


def crafted_graph(N, seed):
    """(2, E) int64: out-degrees 0, 1, 5 and, at road 3, 126 (parallel edges and self-loops are roads like any other to the
    accumulate kernel), the edge list shuffled: an edge's id is not its CSR position."""
    rng = np.random.default_rng(seed)
    deg = [DEGREES[u % 5] if u % 5 != 3 or u == 3 else 3 for u in range(N)]
    src = np.repeat(np.arange(N, dtype=np.int64), deg)
    ei = np.stack([src, rng.integers(0, N, size=src.size)])
    ei = ei[:, rng.permutation(src.size)]
    out_ptr, out_eid = csr(ei, N)
    assert N < 2 or not np.array_equal(out_eid, np.arange(src.size))
    return ei


def _rings(ei, N, F, K, seed):
    """Random rings: popped bytes of :data:`POPPED_BYTES`, counts of :data:`COUNT_VALUES`; SELECTED_ROAD bytes: a valid rank
    (bit 7 set on half of them), and on one byte in eight a code without an edge (0x7F, 0x7E, the out-degree itself, each
    also with bit 7)."""
    rng = np.random.default_rng(seed)
    deg = np.diff(csr(ei, N)[0])
    popped = POPPED_BYTES[rng.integers(0, POPPED_BYTES.size, size=(F, K, N))]
    counts = COUNT_VALUES[rng.integers(0, COUNT_VALUES.size, size=(F, N, K))]
    rank = (rng.random((F, N, K)) * deg[None, :, None]).astype(np.int64)
    bad = np.stack([np.full((F, N, K), 0x7F), np.full((F, N, K), 0x7E),
                    np.broadcast_to(np.minimum(deg, 0x7D)[None, :, None], (F, N, K))])
    pick = rng.integers(0, 3, size=(F, N, K))
    code = np.where(rng.random((F, N, K)) < 0.125, np.take_along_axis(bad, pick[None], 0)[0], rank)
    code = np.where(deg[None, :, None] == 0, np.where(rng.random((F, N, K)) < 0.5, 0, 0x7F), code)
    sel8 = (code | (0x80 * (rng.random((F, N, K)) < 0.5))).astype(np.uint8)
    return popped, sel8, counts


def _case(name, ei, N, popped, sel8, counts, t0, timestep, bin_seconds, block, prev_first=None):
    """A sequence of calls as the evaluator issues them: blocks of ``block`` frames, the last one perhaps partial; a call's
    ``prev`` is the last ``counts`` slice of the call before (``prev_first`` for the first: None = after a reset). One empty
    bin is stored on either side of the bins the frames reach: it must stay zero."""
    T, K, _ = popped.shape
    first_bin = t0 // bin_seconds - 1
    assert first_bin >= 0
    H = (t0 + (T - 1) * timestep) // bin_seconds - first_bin + 2
    calls = []
    for f0 in range(0, T, block):
        s = slice(f0, f0 + block)
        calls.append(dict(t0=t0 + f0 * timestep, popped=np.ascontiguousarray(popped[s]), sel8=np.ascontiguousarray(sel8[s]),
                          counts=np.ascontiguousarray(counts[s]),
                          prev=prev_first if f0 == 0 else np.ascontiguousarray(counts[f0 - 1])))
    return dict(name=name, edge_index=ei, N=N, K=K, E=int(ei.shape[1]), H=int(H), first_bin=int(first_bin), timestep=timestep,
                bin_seconds=bin_seconds, calls=calls)


KS, NS = (1, 3, 64, 65), (1, 5, 64, 67)


def crafted_cases():
    """Every accumulate case of the GPU suite. K x N over {1, 3, 64, 65} x {1, 5, 64, 67} with 9 frames in blocks of 4 (two full
    calls and a partial one, every later call's frame 0 decided by ``prev``), bins of 5 s from clock 1003: the frames span
    three bins. Then: one frame; 25 frames of one call over three bins with bins skipped between them; a first call WITH
    ``prev``; a clock that stands still; and the two consecutive calls whose second starts with one genuine movement and one
    phantom pop that only ``prev`` tells apart."""
    cases = []
    for i, K in enumerate(KS):
        for j, N in enumerate(NS):
            ei = crafted_graph(N, 10 + j)
            p, s, c = _rings(ei, N, 9, K, 100 + 4 * i + j)
            cases.append(_case(f"K{K}-N{N}", ei, N, p, s, c, 1003, 1, 5, 4))
    ei = crafted_graph(5, 11)
    p, s, c = _rings(ei, 5, 1, 3, 200)
    cases.append(_case("one-frame", ei, 5, p, s, c, 4000, 1, 3600, 1))
    ei = crafted_graph(67, 13)
    p, s, c = _rings(ei, 67, 25, 3, 201)
    cases.append(_case("three-bins-one-call", ei, 67, p, s, c, 95, 1, 10, 25))
    cases.append(_case("three-bins-skipping", ei, 67, p, s, c, 1000, 25, 10, 25))
    prev = COUNT_VALUES[np.random.default_rng(202).integers(0, COUNT_VALUES.size, size=(67, 3))]
    cases.append(_case("first-call-with-prev", ei, 67, p[:6], s[:6], c[:6], 4000, 1, 3600, 6, prev_first=prev))
    cases.append(_case("timestep-0", ei, 67, p[:7], s[:7], c[:7], 4000, 0, 3600, 7))
    # two calls of 3 frames; frame 3 = frame 0 of the second call. Roads 0 (out-degree 5) and 1 (out-degree 1) of environment 1
    # are popped there and nowhere else; road 0 held 1 agent after frame 2 (genuine: rank 4), road 1 held none (phantom).
    ei = crafted_graph(5, 11)
    p, s, c = _rings(ei, 5, 6, 2, 203)
    p[:, 1, 0:2] = 0
    p[3, 1, 0:2] = (1, 0xFF)
    c[2, 0, 1], c[2, 1, 1] = 1.0, 0.0
    c[3, 0, 1], c[3, 1, 1] = 0.0, 14.0            # the frame's own counts say the opposite
    s[3, 0, 1], s[3, 1, 1] = 0x84, 0x00
    cases.append(_case("two-calls-prev-decides", ei, 5, p, s, c, 4000, 1, 3600, 3))
    return cases


def run_case(case, defect=None, accumulate_fn=None):
    """The calls of ``case`` into zeroed tables -> (turns (K, H, E), lost (K, H, N), unresolved (K,)) int32.
    ``accumulate_fn(call, tables, case)``: the implementation under test in place of the restatement (the GPU suite)."""
    K, H, N, E = case["K"], case["H"], case["N"], case["E"]
    tables = (np.zeros((K, H, E), dtype=np.int32), np.zeros((K, H, N), dtype=np.int32), np.zeros(K, dtype=np.int32))
    for call in case["calls"]:
        if accumulate_fn is not None:
            tables = accumulate_fn(call, tables, case)
        else:
            accumulate(case["edge_index"], N, call["popped"], call["sel8"], call["counts"], call["prev"], *tables, call["t0"],
                       case["timestep"], case["bin_seconds"], case["first_bin"], defect=defect)
    return tables


def popped_bits(case):
    return sum(int((call["popped"] & 1).sum()) for call in case["calls"])


def binned(edge_index, N, popped, sel8, counts, clock0, timestep, bin_seconds, defect=None):
    """All frames at once from the empty network: rings (T, K, N) / (T, N, K) -> (first_bin, turns, lost, unresolved)."""
    T, K, _ = popped.shape
    first_bin = clock0 // bin_seconds
    H = (clock0 + (T - 1) * timestep) // bin_seconds - first_bin + 1
    E = int(np.asarray(edge_index).shape[1])
    tables = (np.zeros((K, H, E), dtype=np.int32), np.zeros((K, H, N), dtype=np.int32), np.zeros(K, dtype=np.int32))
    accumulate(edge_index, N, popped, sel8, counts, None, *tables, clock0, timestep, bin_seconds, first_bin, defect=defect)
    return (int(first_bin),) + tables


# ---- the oracle's own choice ----------------------------------------------------------------------------------------------------
def rank_bytes(net, choice):
    """(N,) uint8: the rank of edge ``choice[u]`` ((N,) edge ids, -1: none -> 0x7F) in u's CSR out-list."""
    out_ptr, out_eid = csr(net.edge_index.numpy(), net.num_roads)
    code = np.full(net.num_roads, 0x7F, dtype=np.uint8)
    pos = np.empty(out_eid.size, dtype=np.int64)
    pos[out_eid] = np.arange(out_eid.size)
    src = net.edge_index[0].numpy()
    ch = np.asarray(choice, dtype=np.int64)
    has = ch >= 0
    code[has] = (pos[ch[has]] - out_ptr[src[ch[has]]]).astype(np.uint8)
    assert np.array_equal(src[ch[has]], np.nonzero(has)[0])
    return code


def choice_of_ranks(net, code):
    """The inverse of :func:`rank_bytes` for valid ranks (bit 7 ignored): (N,) edge ids, -1 where the road has no out-edge."""
    out_ptr, out_eid = csr(net.edge_index.numpy(), net.num_roads)
    r = np.asarray(code, dtype=np.int64) & 0x7F
    deg = np.diff(out_ptr)
    assert bool(((r < deg) | (deg == 0)).all())
    return np.where(deg > 0, out_eid[np.minimum(out_ptr[:-1] + r, out_eid.size - 1)], -1)


def oracle_replay(net, pop, T, clock0, choices, noise):
    """``T`` frames of the oracle from the empty network, composed from oracle.sim's own functions in the order of
    ``sim.env_step``. ``choices(t)`` -> (N,) edge ids of the frame's action (-1: the road keeps its SELECTED_ROAD);
    ``noise(t)`` -> dict(uniform=...) or dict(gumbel=...) of (E,) values. Returns a dict: ``moved`` and ``accepted`` (T, E)
    bool (Direction's chosen in-edge with a non-zero agent id — the oracle truth — and ResponseMPNN's accepted edges),
    ``popped`` (T, 1, N) uint8, ``sel8`` and ``counts`` (T, N, 1) (the rings of one environment), ``reward`` (T,), ``x``,
    ``agents``, ``max_count`` and ``unqueued`` = the agents flagged ON_WAY but queued nowhere at the end."""
    from oracle import sim
    N, Nmax, ei, ea = net.num_roads, net.Nmax, net.edge_index, net.edge_attr
    E = ei.size(1)
    adj = net.dense_adjacency()
    c = sim.Cols(Nmax)
    x = net.x.clone()
    x[:, :3 * Nmax] = 0
    x[:, c.N] = 0
    ag = pop.clone()
    ag[:, sim.ON_WAY] = 0
    ag[:, sim.DONE] = 0
    moved, accepted = np.zeros((T, E), dtype=bool), np.zeros((T, E), dtype=bool)
    popped, sel8 = np.zeros((T, 1, N), dtype=np.uint8), np.zeros((T, N, 1), dtype=np.uint8)
    counts, reward = np.zeros((T, N, 1), dtype=np.float32), np.zeros(T, dtype=np.float32)
    code = np.full(N, 0x7F, dtype=np.uint8)
    max_count = 0.0
    for f in range(T):
        t = float(clock0 + f)
        ch = np.asarray(choices(f), dtype=np.int64)
        action = torch.zeros(E, dtype=torch.int64)
        action[torch.from_numpy(ch[ch >= 0])] = 1
        new = rank_bytes(net, ch)
        code = np.where(ch >= 0, new, code)
        sim.apply_action(x, ei, action, Nmax)
        nz = noise(f)
        gumbel = nz["gumbel"] if "gumbel" in nz else sim.gumbel_from_uniform(nz["uniform"])
        agent_id, prob, _ = sim.direction_message(x, ei, ea, t, Nmax)
        P = torch.zeros(N).index_add_(0, ei[1], prob)
        arg = sim.segment_argmax_first(torch.log(prob + sim.EPS) + gumbel, ei[1], N)
        m = torch.zeros(E, dtype=torch.bool)
        m[arg[P > 0]] = True
        moved[f] = (m & (agent_id != 0)).numpy()
        sim.direction_step(x, ei, ea, t, Nmax, gumbel=gumbel, congestion_constant=net.congestion_constant)
        accepted[f] = (sim.response_message(x, ei, Nmax) > 0).numpy()
        _, pm = sim.response_step(x, ei, Nmax)
        popped[f, 0] = pm.numpy()
        sel8[f, :, 0] = code
        sim.withdraw(x, ag, adj, t, Nmax)
        sim.insert(x, ag, t, Nmax, net.congestion_constant)
        counts[f, :, 0] = x[:, c.N].numpy()
        reward[f] = float(-x[:, c.N].sum())
        max_count = max(max_count, float(x[:, c.N].max()))
    unqueued = int((ag[:, sim.ON_WAY] == 1).sum()) - int(x[:, c.N].sum())
    return dict(moved=moved, accepted=accepted, popped=popped, sel8=sel8, counts=counts, reward=reward, x=x, agents=ag,
                max_count=max_count, unqueued=unqueued)


def moved_binned(moved, clock0, bin_seconds):
    """(T, E) bool -> (H, E) int32 by the clock at which each frame starts."""
    T = moved.shape[0]
    bins = (clock0 + np.arange(T)) // bin_seconds
    out = np.zeros((int(bins[-1] - bins[0]) + 1, moved.shape[1]), dtype=np.int32)
    np.add.at(out, bins - bins[0], moved.astype(np.int32))
    return out


def random_choices(net, seed, T):
    """``irregular_graphs.random_actions`` per frame, drawn up front: (T, N) edge ids."""
    import irregular_graphs as ig
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([ig.random_actions(net, gen) for _ in range(T)]).numpy().astype(np.int64)
