"""Float64 replay of VecPPOTrainer's multi-epoch update loop (TEST INFRASTRUCTURE: plain torch on the CPU, no kernel involved).

``update()`` runs, per epoch, ``advantages()`` (the critic over all frames with the CURRENT parameters, GAE, normalisation)
and ``minibatch_step()`` (one drawn sub-batch, the clipped loss, backward, one Adam step). :func:`replay_epoch` restates one
such epoch from what exists — ``update_restatement`` (gae64, normalize64, ppo_loss64, segment_dist, adam64), ``oracle/nets.py``
in float64 and the head restatements — and returns the advantages and value targets over all T * B frames, the three loss
scalars and the gradient of EVERY parameter in the order of the trainer's flat buffer (float64 autograd; a parameter off the
live path gets exactly 0). :func:`apply_adam` is ``adam64`` on a flat buffer.

The replay is TEACHER-FORCED: every epoch starts from given parameters, moments and step number (on the GPU: the trainer's
own fp32 snapshot in front of that epoch), so that fp32 error does not compound over epochs and every epoch is held to the
tolerance of the one-epoch tests. :func:`replay_loop` chains the epochs for the host test (its "snapshots" are the clean
float64 chain's) and restates the bookkeeping between ``collect()`` and the epochs — the draws of all epochs concatenated,
the stable sort into frame order, the split of the kept rows over the episode segments, the per-epoch offset — through
:func:`kept_rows` / :func:`epoch_rows`.

``defect=`` (the project's convention, see departure_restatement.py): ONE named bug of that loop at a time —
:data:`DEFECTS`. test_update_loop_host.py shows that each moves a quantity test_gpu_update_loop.py compares by more than ten
times that quantity's tolerance, on the shapes and draws of every GPU case."""
from __future__ import annotations

import types

import numpy as np
import torch

import update_restatement as R

D = torch.float64
TOL = 1e-4          # advantages, targets, losses, gradients: TOL * max(1, scale), test_gpu_trainer_parity.py's ``close``

DEFECTS = ("obs_previous_epoch",   # epoch k >= 1 reads the kept rows of epoch k - 1 (the offset counts one draw too few)
           "obs_unsorted",         # the kept rows land in frame order instead of at their slot of the concatenated draws
           "segment_shift",        # in every episode segment after the first a kept row holds the frame before its own
           "stale_advantages",     # the critic of epoch 0 values all frames in every epoch
           "adam_step_stuck",      # the bias correction's step number stays 1
           "no_done_mask")         # GAE bootstraps and accumulates across the episode end


def _check(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")


# ---- the minibatch draw ----------------------------------------------------------------------------------------------------
def replay_draws(seed, n, M, epochs):
    """``VecPPOTrainer.draw_frames`` on rank 0, ``epochs`` times: M distinct flat indices t * B + b out of n per epoch."""
    rng = np.random.Generator(np.random.Philox(key=int(seed)))
    return [torch.from_numpy(rng.choice(n, size=min(M, n), replace=False, shuffle=True).astype("int64")) for _ in range(epochs)]


def segments(done):
    """Episode segments [(start, stop)] of the batch's frames: an episode end at frame t closes a segment after t."""
    done = [bool(d) for d in done]
    cuts = [0] + [t + 1 for t, d in enumerate(done) if d and t + 1 < len(done)] + [len(done)]
    return list(zip(cuts[:-1], cuts[1:]))


def kept_rows(draws, B, done, obs_of, defect=None):
    """The observation buffer the rollout keeps for a state-dependent head: one row per drawn (frame, environment) pair of
    ALL epochs, row j = the observation of pair cat(draws)[j] — written segment by segment, frame by frame, in stable frame
    order. ``obs_of`` (T, B, N, 16). -> (rows (sum M, N, 16), frames kept per segment)."""
    _check(defect)
    flat = torch.cat(draws)
    order = torch.argsort(flat, stable=True)
    t_sorted, env = (flat[order] // B).tolist(), (flat[order] % B).tolist()
    rows = torch.zeros((flat.numel(),) + tuple(obs_of.shape[2:]), dtype=obs_of.dtype)
    per_segment = []
    for s, (lo, hi) in enumerate(segments(done)):
        here = [p for p, t in enumerate(t_sorted) if lo <= t < hi]
        per_segment.append(len(here))
        for p in here:
            t = t_sorted[p] - 1 if (defect == "segment_shift" and s > 0) else t_sorted[p]
            rows[p if defect == "obs_unsorted" else int(order[p])] = obs_of[t, env[p]]
    return rows, per_segment


def epoch_rows(rows, draws, k, defect=None):
    """Epoch k's rows of :func:`kept_rows`' buffer: behind the draws of the epochs before it."""
    kk = k - 1 if (defect == "obs_previous_epoch" and k > 0) else k
    off = sum(d.numel() for d in draws[:kk])
    return rows[off:off + draws[k].numel()]


# ---- a case: graph, head, critic, flat-buffer layout -------------------------------------------------------------------------
def spec(*, ei, ea, N, T, B, head, critic, layout, numel, temperature=1.0, consts=None, **hyper):
    """``layout``: name -> (offset, shape) of the live parameters in the flat buffer of ``numel`` floats: "emb", "critic.0..5",
    "edge_mlp.0..5", "goal" ((161,)), "gt.<key>", "gtv.<key>". ``consts``: what the head reads besides its parameters —
    "table" (N, N) distances [candidate][destination] (+inf: unreachable) and "w" (prior), "table" / "slot" / "S" (goal),
    "gt_buffers" / "pe" (graph-transformer head), "gtv_buffers" / "gtv_pe" (its critic)."""
    h = dict(gamma=0.99, lmbda=0.95, clip_epsilon=0.2, entropy_coef=0.01, critic_coef=1.0, lr=1e-3)
    h.update(hyper)
    return types.SimpleNamespace(ei=ei, ea=ea, N=N, E=ei.size(1), T=T, B=B, head=head, critic=critic, layout=dict(layout),
                                 numel=int(numel), temperature=float(temperature), consts=dict(consts or {}), **h)


def views(sp, theta):
    return {k: theta[off:off + int(np.prod(shape))].view(shape) for k, (off, shape) in sp.layout.items()}


def live_mask(sp):
    """(numel,) bool: the elements of the flat buffer that belong to a named (live) parameter."""
    m = torch.zeros(sp.numel, dtype=torch.bool)
    for off, shape in sp.layout.values():
        m[off:off + int(np.prod(shape))] = True
    return m


def goal_logits(obs, ei, table, S, w, slot=None):
    """``goal_mlp_restatement.forward`` in float64, differentiable in ``w`` (161,): the features in numpy float64, the
    8 -> 16 -> 1 MLP in torch; an unreachable edge carries the constant -1e20."""
    import goal_mlp_restatement as G
    g, reach = G.features(np.asarray(obs, dtype=np.float32), ei.numpy(), np.asarray(table), S, slot, np.float64)
    W1, b1, w2, b2 = w[:128].view(G.NH, G.NF), w[128:144], w[144:160], w[160]
    l = torch.relu(torch.from_numpy(g).to(w.dtype) @ W1.t() + b1) @ w2 + b2
    return torch.where(torch.from_numpy(reach), l, torch.full_like(l, float(G.UNREACHABLE)))


def head_logits(sp, P, obs, M=None):
    """The policy head's logits (M, E) in the dtype of the parameters ``P`` for the observations ``obs`` (M, N, 16); the
    embedding head reads none (``obs`` None, ``M`` rows)."""
    from oracle import nets
    M = obs.size(0) if obs is not None else M
    dt = next(iter(P.values())).dtype
    if sp.head == "embedding":
        nf = torch.zeros((M, sp.N, 7), dtype=dt)
        nf[..., 6] = torch.arange(sp.N, dtype=dt)
        return nets.policy_logits(nf, sp.ei, P["emb"])
    if sp.head == "edge_mlp":
        return nets.edge_mlp_logits(obs.to(dt), sp.ei, sp.ea.to(dt).expand(M, -1, -1), *(P[f"edge_mlp.{i}"] for i in range(6)))
    if sp.head == "embedding_dijkstra":
        from test_gpu_prior_head import restated_logits
        return restated_logits(obs.to(dt), sp.ei, sp.consts["table"].to(dt), P["emb"], sp.consts["w"])
    if sp.head == "goal_mlp":
        return goal_logits(obs.float().numpy(), sp.ei, sp.consts["table"], sp.consts["S"], P["goal"], sp.consts.get("slot"))
    if sp.head == "graph_transformer":
        import gt_restatement as GT
        sd = {k: v.to(dt) for k, v in sp.consts["gt_buffers"].items()}
        sd.update({k[3:]: v for k, v in P.items() if k.startswith("gt.")})
        return GT.gt_logits(sd, obs.to(dt), sp.ei, sp.ea.to(dt), sp.consts["pe"].to(dt))
    raise ValueError(sp.head)


def critic_values(sp, P, counts, times, obs):
    """The critic's values for rows of count vectors ``counts`` (R, N) at clocks ``times`` (R,) (simple) or of observations
    ``obs`` (R, N, 16) (graph transformer)."""
    from oracle import nets
    dt = next(iter(P.values())).dtype
    if sp.critic == "simple":
        nf = torch.zeros(counts.shape + (7,), dtype=dt)
        nf[..., 1] = counts.to(dt)
        return nets.critic_value(nf, times.to(dt).view(-1, 1), *(P[f"critic.{i}"] for i in range(6))).squeeze(-1)
    import gt_value_restatement as GV
    sd = {k: v.to(dt) for k, v in sp.consts["gtv_buffers"].items()}
    sd.update({k[4:]: v for k, v in P.items() if k.startswith("gtv.")})
    pe = sp.consts["gtv_pe"].to(dt)
    return torch.cat([GV.gt_value(sd, obs[i:i + 256].to(dt), sp.ei, pe) for i in range(0, obs.size(0), 256)])


# ---- one epoch -------------------------------------------------------------------------------------------------------------
def replay_epoch(sp, ro, theta, idx, obs_mb, *, adv_theta=None, defect=None, dtype=D):
    """One epoch of ``update()`` from the parameters ``theta`` (numel,) at its start.
    ``ro``: the rollout — counts (T + 1, B, N), choice (T, B, N) edge ids (-1: none), logp (T, B) the stored behaviour
    log-prob, reward (T, B), times (T + 1,), done (T,) bool, and for the graph-transformer critic obs_all ((T + 1) * B, N, 16).
    ``idx`` (M,): the minibatch's flat indices t * B + b; ``obs_mb`` (M, N, 16): the observations of those pairs (None for
    the embedding head). ``adv_theta``: the parameters the critic of the all-frames pass uses (default ``theta``; the
    ``stale_advantages`` defect of :func:`replay_loop`). ``dtype``: float64, or float32 for the error yardstick.
    -> dict: adv, target (T, B) (adv normalised), losses (3,), grad (numel,), lp_new (M,), ratio_max."""
    _check(defect)
    T, B, N = sp.T, sp.B, sp.N
    theta = theta.detach().to(dtype).clone().requires_grad_(True)
    P = views(sp, theta)
    with torch.no_grad():
        Pa = P if adv_theta is None else views(sp, adv_theta.detach().to(dtype))
        tm = ro["times"].to(dtype).view(T + 1, 1).expand(T + 1, B).reshape(-1)
        v = critic_values(sp, Pa, ro["counts"].reshape((T + 1) * B, N), tm, ro.get("obs_all")).view(T + 1, B)
        done = None if (defect == "no_done_mask" or not bool(ro["done"].any())) else ro["done"].view(T, 1).expand(T, B)
        adv, target = R.gae64(ro["reward"].to(dtype), v[:T], v[1:], done, done, sp.gamma, sp.lmbda)
        adv = R.normalize64(adv) if dtype == D else (adv - adv.mean()) / adv.std().clamp_min(R.ADV_STD_FLOOR)
    t_idx, b_idx = idx // B, idx % B
    dist = R.segment_dist(head_logits(sp, P, obs_mb, idx.numel()), sp.ei, sp.temperature, N)
    lp_new, ent = dist.log_prob(choice=ro["choice"][t_idx, b_idx]), dist.entropy()
    value = critic_values(sp, P, ro["counts"][t_idx, b_idx], ro["times"][t_idx], obs_mb)
    lp_old = ro["logp"].to(dtype).view(-1)[idx]
    out, g_lp, g_ent, g_val, _ = R.ppo_loss64(lp_new, lp_old, adv.view(-1)[idx], value, target.view(-1)[idx], ent,
                                              clip_epsilon=sp.clip_epsilon, entropy_coef=sp.entropy_coef,
                                              critic_coef=sp.critic_coef)
    torch.autograd.backward([lp_new, ent, value], [g_lp, g_ent, g_val])
    grad = theta.grad if theta.grad is not None else torch.zeros_like(theta)
    return dict(adv=adv, target=target, losses=out[:3], grad=grad.detach(), lp_new=lp_new.detach(),
                ratio_max=float((lp_new.detach() - lp_old).abs().max()))


def apply_adam(theta, m, v, step, grad, lr=1e-3):
    """``update_restatement.adam64`` on the flat buffer: -> (theta, m, v) after the step numbered ``step`` (1-based), in the
    dtype of the inputs."""
    return R.adam64(theta, grad, m, v, step, lr=lr)


def adam_bounds(theta, m, v, step, grad, lr=1e-3):
    """The float64 result of one Adam step on the fp32 inputs and, per output, the tolerance rule of test_gpu_update_fp64.py:
    ``tensor_bound(e32, ref)`` with e32 the error of the same arithmetic in fp32 on the CPU.
    -> [(name, ref64, bound)] for param, exp_avg, exp_avg_sq."""
    a32 = [t.detach().float().cpu() for t in (theta, m, v, grad)]
    ref = apply_adam(a32[0].double(), a32[1].double(), a32[2].double(), step, a32[3].double(), lr)
    f32 = apply_adam(a32[0], a32[1], a32[2], step, a32[3], lr)
    return [(n, r, R.tensor_bound(R.max_err(f, r), r)) for n, r, f in zip(("param", "exp_avg", "exp_avg_sq"), ref, f32)]


# ---- the loop --------------------------------------------------------------------------------------------------------------
def replay_loop(sp, ro, draws, theta0, obs_of=None, defect=None):
    """All epochs. The state in front of every epoch is the CLEAN float64 chain's (parameters, moments, step: the GPU test's
    snapshots); with a ``defect`` the epoch's outputs are the defective ones computed from that clean state, as the
    teacher-forced GPU test would see them. -> list over epochs of :func:`replay_epoch`'s dict plus obs (the rows the epoch
    read), theta / m / v (after the epoch's Adam step) and theta_in / m_in / v_in / step (what that step started from)."""
    _check(defect)
    theta, m, v = theta0.double().clone(), torch.zeros(sp.numel, dtype=D), torch.zeros(sp.numel, dtype=D)
    state_dep = sp.head != "embedding"
    if state_dep and sp.critic == "simple":
        clean_rows, _ = kept_rows(draws, sp.B, ro["done"], obs_of)
        rows = kept_rows(draws, sp.B, ro["done"], obs_of, defect)[0] if defect else clean_rows
    out = []
    for k, idx in enumerate(draws):
        if not state_dep:
            obs_c = obs_d = None
        elif sp.critic == "simple":
            obs_c, obs_d = epoch_rows(clean_rows, draws, k), epoch_rows(rows, draws, k, defect)
        else:       # the observation store of the graph-transformer critic: rows t * B + b
            obs_c = obs_d = ro["obs_all"][idx]
        clean = replay_epoch(sp, ro, theta, idx, obs_c)
        e = clean if defect is None else replay_epoch(sp, ro, theta, idx, obs_d, defect=defect,
                                                      adv_theta=theta0 if defect == "stale_advantages" else None)
        e = dict(e, obs=obs_d, theta_in=theta, m_in=m, v_in=v, step=k + 1, adam_step=1 if defect == "adam_step_stuck" else k + 1)
        e["theta"], e["m"], e["v"] = apply_adam(theta, m, v, e["adam_step"], e["grad"], sp.lr)
        theta, m, v = apply_adam(theta, m, v, k + 1, clean["grad"], sp.lr)
        out.append(e)
    return out


def moved(clean, bad, sp):
    """By how many tolerances a defect moves the quantities the GPU test compares: {name: max over epochs of
    |defective - clean| / tolerance}; TOL * max(1, scale) for advantages, targets, losses and each gradient slice, the Adam
    rule for the parameters and moments, and ``rows``: 1 where a kept row differs at all (compared bit for bit), else 0."""
    ratio = {}

    def note(name, d, c, tol):
        ratio[name] = max(ratio.get(name, 0.0), R.max_err(d, c) / tol)
    for c, b in zip(clean, bad):
        for q in ("adv", "target"):
            note(q, b[q], c[q], TOL * max(1.0, float(c[q].abs().max())))
        for i, q in enumerate(("loss_objective", "loss_critic", "loss_entropy")):
            note(q, b["losses"][i], c["losses"][i], TOL * max(1.0, abs(float(c["losses"][i]))))
        for name, (off, shape) in sp.layout.items():
            sl = slice(off, off + int(np.prod(shape)))
            note("grad", b["grad"][sl], c["grad"][sl], TOL * max(1.0, float(c["grad"][sl].abs().max())))
        # the GPU test replays Adam on the GPU's own gradient of that epoch: only the step number can show there
        bounds = adam_bounds(c["theta_in"], c["m_in"], c["v_in"], c["step"], c["grad"], sp.lr)
        got = apply_adam(c["theta_in"], c["m_in"], c["v_in"], b["adam_step"], c["grad"], sp.lr)
        for (name, _, bound), d, key in zip(bounds, got, ("theta", "m", "v")):
            note(name, d, c[key], bound)
        if c["obs"] is not None:
            ratio["rows"] = max(ratio.get("rows", 0.0), 0.0 if torch.equal(c["obs"], b["obs"]) else 1.0)
    return ratio


# ---- the GPU cases (shapes, seeds, heads): shared with the host test ----------------------------------------------------------
# draw shapes: A = 300-s steps, three episode segments (13 + 13 + 2 frames), the last without a kept row;
#              B = more draws than frames: pairs drawn in two and in all three epochs, kept rows in frame 0 and frame T - 1
SHAPE_A = dict(T=28, B=4, M=6, epochs=2, seed=2, timestep=300, torus=(4, 4))
SHAPE_B = dict(T=14, B=6, M=32, epochs=3, seed=0, timestep=1, torus=(4, 4))
SHAPE_SLAB = dict(T=24, B=128, M=16, epochs=3, seed=0, timestep=1, torus=(4, 4))
SHAPE_ODD = dict(T=24, B=6, M=16, epochs=3, seed=0, timestep=300, torus=(4, 4))

CASES = {
    "emb_frames": dict(head="embedding", critic="simple", rollout="frames", **SHAPE_SLAB),
    "emb_lazy": dict(head="embedding", critic="simple", rollout="frames", lazy=True, **SHAPE_SLAB),
    "emb_env_odd": dict(head="embedding", critic="simple", rollout="env", **SHAPE_ODD),
    "edge_mlp_A": dict(head="edge_mlp", critic="simple", temperature=400.0, **SHAPE_A),
    "edge_mlp_B": dict(head="edge_mlp", critic="simple", temperature=400.0, **SHAPE_B),
    "prior_all_pairs_B": dict(head="embedding_dijkstra", critic="simple", **SHAPE_B),
    "prior_per_dest_A": dict(head="embedding_dijkstra", critic="simple", per_dest=True, **SHAPE_A),
    "goal_B": dict(head="goal_mlp", critic="simple", temperature=2.0, **SHAPE_B),
    "goal_rules_A": dict(head="goal_mlp", critic="simple", temperature=2.0, rules=True, **SHAPE_A),
    "gt_B": dict(head="graph_transformer", critic="simple", temperature=1.0, **SHAPE_B),
    "gt_gtv_B": dict(head="graph_transformer", critic="graph_transformer", temperature=1.0, **SHAPE_B),
}


def done_frames(T, timestep, start=21540.0, end=25200.0):
    """``VecPPOTrainer._segments``' episode ends: the frame whose step pushes the clock past ``end`` is an episode's last."""
    done, t, clock = [False] * T, 0, start
    while t < T:
        n = int(min(T - t, max(1, (end - clock) // timestep + 1)))
        t += n
        if clock + n * timestep > end:
            done[t - 1] = True
            clock = start
        else:
            clock += n * timestep
    return torch.tensor(done)


def applicable(name, defect):
    """Whether ``defect`` restates a bug of the code the case ``name`` runs: the observation defects need kept rows (a
    state-dependent head without the observation store), ``segment_shift`` and ``no_done_mask`` an episode end."""
    c = CASES[name]
    ends = c["timestep"] == 300
    if defect in ("obs_previous_epoch", "obs_unsorted"):
        return c["head"] != "embedding" and c["critic"] == "simple"
    if defect == "segment_shift":
        return c["head"] != "embedding" and c["critic"] == "simple" and ends
    if defect == "no_done_mask":
        return ends
    return True
