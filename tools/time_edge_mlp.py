#!/usr/bin/env python3
"""Developer tool: time the kernels of csrc/edge_mlp.hip at the bench's state-dependent-policy size (config 4: the 25 x 25
torus, 10 000 edges, --envs samples): the per-edge MLP forwards (fp32 MFMA, bf16x3, bf16 on fp32 and on bf16 rows) with their
logit error against an fp64 evaluation of the head, the backward (``ops.policy_edge_mlp_bwd``, all three stages) on a
minibatch of --sub-batch samples (the trainer's sub-batch), and the packed observation builders on a live state (all
environments in fp32 and in bf16, and the fp32 rows of --sub-batch environments).

Every figure is the median over --rounds rounds of --reps launches between two device events, after a warm-up round; the
lowest and highest round are printed beside it. ``--json`` adds one machine-readable line. To compare two builds, run the
tool once per build (TARL_HIP_LIB selects the library), alternating, and compare the medians against what alternating one
build with itself gives."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd")]
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=2048)
ap.add_argument("--sub-batch", type=int, default=32, help="samples of the backward's minibatch")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=25, help="frames simulated before the observation builders are timed")
ap.add_argument("--json", action="store_true")
a = ap.parse_args()
from tarl_hip import lib, ops, synth  # noqa: E402
from tarl_hip.engine import SimEngine  # noqa: E402


def timed(fn):
    """(median, min, max) microseconds per call of ``fn`` over the rounds."""
    per = []
    for r in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:                                      # round 0 warms up
            per.append(e0.elapsed_time(e1) / a.reps * 1e3)
    return statistics.median(per), min(per), max(per)


net = synth.torus_network(25, 25)
N, E = net.num_roads, net.edge_index.size(1)
plan = ops.Plan(net.edge_index, N)
ec = ops.EdgeConst(net.edge_attr, "cuda")
g = torch.Generator().manual_seed(1)
obs = torch.randn((a.envs, N, 16), generator=g)
obs[..., 7:] = obs[..., 7:].abs() * 2.0e4          # clock-time sized columns
obs = obs.cuda()
ws = [torch.randn(s, generator=g) * 0.2 for s in ((64, 33), (64,), (32, 64), (32,), (1, 32), (1,))]
w = ops.EdgeMlpWeights(*[t.cuda() for t in ws])
out = torch.empty((a.envs, E), device="cuda")
obs_bf = obs.to(torch.bfloat16)
res, logits = {}, {}
for prec in ("fp32", "x3", "bf16", "bf16 obs"):
    # "bf16 obs": the rollout's form, observations already bf16 (tarl_fused_obs16_bf16)
    x, prec_kw = (obs_bf, None) if prec == "bf16 obs" else (obs, prec)
    res["fwd " + prec] = timed(lambda: ops.policy_edge_mlp(plan, x, ec, w, precision=prec_kw, out=out))
    logits[prec] = out[:4].clone()

# the backward on a minibatch: scratch and gradient buffers allocated once, as the trainer keeps them
Mb = min(a.sub_batch, a.envs)
gl = torch.randn((Mb, E), generator=g).cuda()
grads = [torch.zeros(s, device="cuda") for s in ((64, 33), (64,), (32, 64), (32,), (32,), (1,))]
scratch = torch.empty(ops.edge_mlp_bwd_scratch_floats(plan, Mb), device="cuda")
obs_mb = obs[:Mb].contiguous()
res[f"bwd M={Mb}"] = timed(lambda: ops.policy_edge_mlp_bwd(plan, obs_mb, ec, w, gl, grads, scratch=scratch))

# the packed observation builders on a live state (eight populations repeated over the environments)
pops = torch.stack([synth.population(N, N, seed=b, t0=21540, t1=21560) for b in range(8)]).repeat(-(-a.envs // 8), 1, 1)
eng = SimEngine(net.x.cuda().unsqueeze(0).repeat(a.envs, 1, 1).contiguous(), net.edge_index, net.edge_attr, net.Nmax,
                pops[:a.envs].cuda(), congestion_constant=net.congestion_constant, seed=4)
eng.reset()
eng.prepare_policy(torch.randn(N, generator=g).cuda())
for _ in range(a.frames):
    eng.frame_fused()
o32 = torch.empty((a.envs, N, 16), device="cuda")
o16 = torch.empty((a.envs, N, 16), dtype=torch.bfloat16, device="cuda")
res["obs16 packed"] = timed(lambda: ops.fused_obs16(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, out=o32))
res["obs16 packed bf16"] = timed(lambda: ops.fused_obs16_bf16(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, out=o16))
env = torch.arange(Mb, dtype=torch.int32, device="cuda") * (a.envs // Mb)
slot = torch.arange(Mb, dtype=torch.int32, device="cuda")
keep = torch.empty((Mb, N, 16), device="cuda")
res[f"obs16 rows M={Mb}"] = timed(lambda: ops.fused_obs16_rows(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, env, slot, keep))
assert float(o32[:, :, 1].sum()) > 0               # roads hold agents: the builders gathered real head rows

from oracle import nets  # noqa: E402
ref = nets.edge_mlp_logits(obs[:4].cpu().double(), net.edge_index, net.edge_attr.double().expand(4, -1, -1),
                           *[t.double() for t in ws])
scale = float(ref.abs().max())
print(f"library {lib.LIB_PATH}: {a.envs} samples x {E} edges, {a.rounds} rounds of {a.reps}")
for name, (med, lo, hi) in res.items():
    line = f"{name:18s} {med:9.1f} us  [{lo:.1f} .. {hi:.1f}]"
    if name.startswith("fwd "):
        err = float((logits[name[4:]].cpu().double() - ref).abs().max())
        line += f"   per {a.envs * E / 1e6:.1f} M edges   max |err| vs fp64 {err:.3e} = {err / scale:.2e} of scale"
    print(line)
if a.json:
    print("JSON " + json.dumps({"lib": lib.LIB_PATH, "us": {k: v[0] for k, v in res.items()}}))
