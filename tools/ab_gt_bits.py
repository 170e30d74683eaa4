"""Developer tool: bit identity of the two graph-transformer networks (csrc/gt_policy.hip, csrc/gt_value.hip, their shared
core csrc/gt_core.h) between two builds of the library with one C ABI. One process per build: it runs the cases below on
whichever library ``TARL_HIP_LIB`` names (default: the tree's own) and writes every raw output to an .npz; ``--compare``
then asserts ``numpy.array_equal`` on every array of two such files.

    TARL_HIP_LIB=tmp_ab/libtarl_hip_parent.so python tools/ab_gt_bits.py --out tmp_ab/gt_parent.npz
    python tools/ab_gt_bits.py --out tmp_ab/gt_this.npz
    python tools/ab_gt_bits.py --compare tmp_ab/gt_parent.npz tmp_ab/gt_this.npz

Cases (scaled random weights: non-trivial BatchNorm statistics and biases; observations as the simulator builds them):
torus8 M = 1 (one partial workgroup); torus16 M = 7 (several full chunks of the weight-gradient sums); the 4 x 6 MATSim
grid M = 7 (empty in- / out-segments, zero PE rows); config 4 M = 1 (N > 256: the critic's pool strides). The tool checks
that in at least one case M * N and M * E both exceed 1 024 and are a multiple of neither 1 024 nor 256, so that stage 2
adds several chunks and the last one is short: config 4 is that case (2 500 and 10 000 items). torus16 cannot be, whatever
M: its N = 1 024 and E = 4 096 are multiples of the chunk.

Per case: the policy's logits, the critic's values, every gradient of both accumulated into buffers pre-filled with a fixed
non-zero pattern, and the same again through a caller-supplied scratch buffer. Then one fused_rollout_gt of 3 frames,
B = 64, on torus8.

``--sizes`` needs no GPU: it writes what the four scratch-size queries and tarl_value_gt_bwd_max_samples return for a grid
of (N, E, M), N = 0 and M = -1 included, to an .npz that ``--compare`` takes like the others.

    TARL_HIP_LIB=tmp_ab/libtarl_hip_parent.so python tools/ab_gt_bits.py --sizes tmp_ab/sizes_parent.npz
"""
import argparse
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

CASES = [("torus8", 1), ("torus16", 7), ("matsim", 7), ("config4", 1)]


def _ragged(n):
    return n > 1024 and n % 1024 != 0 and n % 256 != 0


def _prefilled(params, seed):
    """Gradient buffers holding a fixed non-zero pattern: stage 2 accumulates with += into what the caller passes."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=gen).to(p.device) for p in params]


def _case(out, kind, M, tmp):
    import torch
    import gt_cases as G
    from src.transformer import laplacian_pe
    from tarl_hip import ops
    ei, ea, x, Nmax, R, routes = G._graph(kind, tmp)
    N, E = x.size(0), ei.size(1)
    tag = f"{kind}/M{M}"
    plan = ops.Plan(ei, N)
    ec = ops.EdgeConst(ea.reshape(-1, 1), "cuda")
    pe = laplacian_pe(routes, R, N).cuda().contiguous()
    obs = G._real_obs(x, Nmax, R, M, seed=M + 5).cuda().contiguous()
    pol = G._random_state(E + M)
    w = ops.GtWeights({k: v.cuda().float().contiguous() for k, v in pol.items()
                       if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS})
    cri = G._random_state(N + M, critic=True)
    wv = ops.GtValueWeights({k: v.cuda().float().contiguous() for k, v in cri.items()
                             if k in ops.GT_VALUE_PARAM_KEYS + ops.GT_VALUE_BUFFER_KEYS})
    out[f"{tag}/logits"] = ops.policy_gt_logits(plan, obs, ec, pe, w).cpu().numpy()
    out[f"{tag}/value"] = ops.value_gt_forward(plan, obs, pe, wv).cpu().numpy()
    coef = torch.randn(M, E, generator=torch.Generator().manual_seed(M)).cuda()
    coef_v = torch.randn(M, generator=torch.Generator().manual_seed(M + 1)).cuda()
    scratch = {"own": (None, None),
               "supplied": (torch.empty(ops.gt_bwd_scratch_bytes(plan, M) // 4 + 64, device="cuda"),
                            torch.empty(ops.value_gt_bwd_scratch_bytes(plan, M) // 4 + 64, device="cuda"))}
    for how, (sp, sv) in scratch.items():
        grads = _prefilled(w.params, 11)
        ops.policy_gt_bwd(plan, obs, ec, pe, w, coef, grads, scratch=sp)
        for k, g in zip(ops.GT_PARAM_KEYS, grads):
            out[f"{tag}/policy grad ({how} scratch)/{k}"] = g.cpu().numpy()
        grads = _prefilled(wv.params, 13)
        ops.value_gt_backward(plan, obs, pe, wv, coef_v, grads, scratch=sv)
        for k, g in zip(ops.GT_VALUE_PARAM_KEYS, grads):
            out[f"{tag}/critic grad ({how} scratch)/{k}"] = g.cpu().numpy()
    print(f"  {tag} done", flush=True)
    return tag, M * N, M * E


def _rollout(out):
    import torch
    import gt_cases as G
    from src.transformer import laplacian_pe
    from tarl_hip import ops, synth
    from tarl_hip.engine import SimEngine
    net = synth.torus_network(8, 8, heterogeneous=True, seed=8)
    N, B, T = net.num_roads, 64, 3
    pops = synth.population_batch(400, N, B, seed=21, device="cuda", t1=21580)
    eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(B, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                    pops.clone(), congestion_constant=net.congestion_constant, seed=11)
    eng.reset()
    w = ops.GtWeights({k: v.cuda().contiguous() for k, v in G._random_state(3).items()
                       if k in ops.GT_PARAM_KEYS + ops.GT_BUFFER_KEYS})
    pe = laplacian_pe(net.edge_index, N, N).cuda()
    ch = torch.zeros((T, B, N), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((T + 1, N, B), dtype=torch.uint8, device="cuda")
    lp, rw = torch.zeros((T, B), device="cuda"), torch.zeros((T, B), device="cuda")
    eng.rollout_gt(T, pe, w, temperature=50.0, policy_seed=77, policy_counter0=5, choice8=ch, log_prob=lp, reward=rw,
                   counts=ct)
    for k, v in (("choice8", ch), ("log_prob", lp), ("reward", rw), ("counts", ct)):
        out[f"rollout torus8 T{T} B{B}/{k}"] = v.cpu().numpy()
    return f"rollout torus8 T{T} B{B}"


def run(path):
    import torch
    out, tags, some_short = {}, [], False
    with tempfile.TemporaryDirectory() as tmp:
        for kind, M in CASES:
            tag, mn, me = _case(out, kind, M, pathlib.Path(tmp))
            short = _ragged(mn) and _ragged(me)
            some_short = some_short or short
            tags.append(f"{tag} (M*N = {mn}, M*E = {me}{': several chunks, the last one short' if short else ''})")
    assert some_short, "no case whose weight-gradient sums span several chunks with a short last one"
    tags.append(_rollout(out))
    torch.cuda.synchronize()
    np.savez(path, **out)
    so = os.environ.get("TARL_HIP_LIB") or "the tree's own library"
    print(f"{so}: {len(out)} arrays of {len(tags)} cases -> {path}")
    for t in tags:
        print("  " + t)


def sizes(path):
    import ctypes
    from fake_plan import fake_plan
    L = ctypes.CDLL(os.environ.get("TARL_HIP_LIB") or os.path.join(ROOT, "tarl-simulator_amd", "tarl_hip", "libtarl_hip.so"))
    names = [f"tarl_{net}_gt_{d}_scratch_floats" for net in ("policy", "value") for d in ("fwd", "bwd")]
    for n in names:
        getattr(L, n).restype, getattr(L, n).argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64]
    L.tarl_value_gt_bwd_max_samples.restype, L.tarl_value_gt_bwd_max_samples.argtypes = ctypes.c_int64, [ctypes.c_void_p]
    graphs = [(0, 0), (1, 0), (1, 1), (7, 3), (3, 7000), (124, 404), (256, 1024), (1024, 4096), (2500, 10000), (25000, 100000)]
    samples = [-1, 0, 1, 2, 7, 64, 1023, 1024, 1025, 6710, 100000]
    out = {}
    for N, E in graphs:
        p = fake_plan(N, E)
        out[f"sizes/N{N} E{E}"] = np.array([[getattr(L, n)(ctypes.byref(p), M) for n in names] for M in samples]
                                           + [[L.tarl_value_gt_bwd_max_samples(ctypes.byref(p))] * len(names)], dtype=np.int64)
    np.savez(path, **out)
    print(f"{len(graphs)} graphs x {len(samples)} sample counts x {len(names)} queries, and the sample limit -> {path}")


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    assert sorted(za.files) == sorted(zb.files), "the two files hold different arrays"
    diff = [k for k in za.files if not (za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k]))]
    cases = sorted({k.split("/")[0] + ("/" + k.split("/")[1] if k.count("/") > 1 else "") for k in za.files})
    print(f"cases: {', '.join(cases)}")
    print(f"{len(za.files)} arrays, {sum(za[k].size for k in za.files)} elements, "
          f"{sum(1 for k in za.files if np.any(za[k] != 0))} of them not all zero")
    assert not diff, f"{len(diff)} arrays differ: {diff[:8]}"
    print("all equal")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    elif args.sizes:
        sizes(args.sizes)
    else:
        run(args.out or ap.error("--out or --compare"))
