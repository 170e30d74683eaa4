"""BCTrainer — behaviour cloning of the shortest-path router into a policy head (not in the reference): a warm
start for the learned heads, which otherwise meet PPO with random weights.

One iteration = one episode prefix on K environments of a fused engine of its own, labelled frame by frame, then a few
epochs of cross-entropy on a store of sampled (environment, frame) pairs:

  reset; draw ``samples`` (environment, frame) pairs ahead (the draw does not depend on the data); per frame
    the routers' refresh (``evaluator.refresh_router_tables``: what VecEvaluator's router heads do),
    ``ops.fused_expert_labels``  — the router's pick of every occupied row as a rank byte; the packed state is not touched,
    the kept pairs' observation rows (``ops.fused_obs16_rows``) and label rows go to the store,
    the DRIVER sets SELECTED_ROAD: ``expert`` = ``ops.fused_select_next_hop_dest(hold=True)`` (the run is the
      "dijkstra_hold" evaluator's, frame for frame), ``policy`` = the head's logits, ``ops.graphdist_rollout`` (sampled),
      ``ops.fused_hold_policy_actions``; ``dagger`` = iteration 0 as ``expert``, every later one as ``policy``,
    ``frame_fused(skip_choice=True)``;
  then ``epochs`` passes over the store in minibatches of ``batch``: the head's forward (``VecPPOTrainer._actor_logits``),
  ``ops.graphdist_bc``, the head's backward (``_actor_logits_bwd``), ``ops.adam_step_``.

The head's arithmetic is the PPO trainer's, held by reference: nothing of it is written a second time. The labels are taken
BEFORE the hold — the destination road is a rank among the row's out-edges, and the hold rule turns exactly that pick into
the hold — so a head that reproduces them and runs under ``policy_hold`` behaves like "dijkstra_hold" on occupied rows.
BC keeps its own Adam moments; PPO afterwards starts with fresh ones."""
from __future__ import annotations

import time

import numpy as np
import torch

from . import dist_utils, lib as _lib, ops
from .evaluator import VecEvaluator, refresh_router_tables, router_buffers

DRIVERS = ("expert", "policy", "dagger")
EXPERTS = {"dijkstra": 10, "free_flow": 0}      # refresh_rate of the router's tables (0: built at frame 0 only)
RECORD_KEYS = ("iteration", "driver", "expert", "frames", "envs", "samples", "labelled", "labelled_share", "loss_first",
               "loss_last", "accuracy_before", "accuracy_after", "arrivals", "collect_seconds", "update_seconds")


class BCTrainer:
    def __init__(self, ppo, engine, *, expert="dijkstra", driver="dagger", frames=32, samples=256, epochs=4, batch=32,
                 lr=1e-3, seed=0, baseline_dests=None):
        """``ppo``: the :class:`VecPPOTrainer` whose head is cloned into (its flat parameter buffer, head forward and
        backward); ``engine``: a fused :class:`SimEngine` with the K environments the driver runs on (the same graph and
        population). ``baseline_dests``: as VecEvaluator's. Fused engines only."""
        if engine.fs is None or ppo.eng.fs is None:
            raise _lib.TarlError("BCTrainer needs the fused engine (ops.fused_path_supported): the packed state cannot "
                                 "represent this graph and there is no fall-back")
        if dist_utils.world()[1] > 1:
            raise ValueError("behaviour cloning runs on one GPU (one process): ranks would clone from different rollouts "
                             "without averaging their gradients")
        if expert not in EXPERTS:
            raise ValueError(f"expert must be one of {tuple(EXPERTS)}, got {expert!r}")
        if driver not in DRIVERS:
            raise ValueError(f"driver must be one of {DRIVERS}, got {driver!r}")
        if engine.N != ppo.eng.N or engine.E != ppo.eng.E:
            raise ValueError("the BC engine must run on the trainer's graph")
        for name, v in (("frames", frames), ("samples", samples), ("epochs", epochs), ("batch", batch)):
            if int(v) < 1:
                raise ValueError(f"{name} must be >= 1, got {v!r}")
        if not float(lr) > 0.0:
            raise ValueError(f"lr must be positive, got {lr!r}")
        self.ppo, self.eng = ppo, engine
        self.expert, self.driver, self.refresh_rate = expert, driver, EXPERTS[expert]
        K, N, dev = engine.B, engine.N, engine.device
        self.frames, self.epochs, self.lr = int(frames), int(epochs), float(lr)
        self.samples = min(int(samples), self.frames * K)
        self.batch = min(int(batch), self.samples)
        self.state_dep = ppo.policy != "embedding"
        store = self.samples * N * (64 + 1)
        free = int(torch.cuda.mem_get_info(dev)[0])
        if store > free // 2:
            raise ValueError(f"the behaviour-cloning store of {self.samples} samples x {N} nodes x 65 bytes "
                             f"({store / 2**30:.2f} GiB) exceeds half the free device memory ({free / 2**30:.2f} GiB free): "
                             f"at most {free // 2 // (N * 65)} samples fit")
        self.dests, self.dest_slot, self.weights, self.table, self.tree_scratch = router_buffers(engine, baseline_dests)
        self.labels = torch.empty((K, N), dtype=torch.uint8, device=dev)
        self.n_lab = torch.zeros(K, dtype=torch.int32, device=dev)
        self.reward = torch.zeros((self.frames, K), dtype=torch.float32, device=dev)
        self.obs_store = torch.empty((self.samples, N, 16), dtype=torch.float32, device=dev) if self.state_dep else None
        self.label_store = torch.empty((self.samples, N), dtype=torch.uint8, device=dev)
        need = int(_lib.load().tarl_graphdist_bc_scratch_bytes(engine.plan.handle, max(self.batch, 1)))
        self.bc_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        self._policy_ev = None          # the `policy` driver's head: a VecEvaluator over the trainer's live parameters
        # BC's own Adam moments over the trainer's flat buffer (the critic's gradient stays zero: its weights do not move)
        self.exp_avg = torch.zeros_like(ppo.flat.flat)
        self.exp_avg_sq = torch.zeros_like(ppo.flat.flat)
        self.step = 0
        self.np_rng = np.random.Generator(np.random.Philox(key=int(seed) + 104723))
        self.iteration = 0
        self.keep_idx = None            # test hook: these flat pairs t * K + b instead of a random draw
        self.frame_hook = None          # test hook: called as frame_hook(t) after the labels of frame t are written
        self.records = []

    # -- the driver's action of one frame ---------------------------------------------------------------------------------
    _EVAL_HEAD = {"x3": "edge_mlp", "fp32": "edge_mlp_fp32", "bf16": "edge_mlp_bf16"}

    def _policy_head(self):
        """The ``policy`` driver's head: a :class:`VecEvaluator` with ``policy_hold`` on this engine, over views of the trainer's
        live parameters (built once; later optimiser steps, in place, are seen). Its per-frame logits, buffers and held counter
        are the evaluator's: the dispatch from the packed state to a head's logits is written there alone."""
        if self._policy_ev is None:
            ppo = self.ppo
            kw = dict(emb=ppo._emb(), temperature=ppo.temperature, prior_weight=ppo.prior_weight, policy_hold=True)
            head = ppo.policy
            if head == "edge_mlp":
                head, kw["edge_mlp"] = self._EVAL_HEAD[ppo.policy_precision], ppo._edge_mlp()
            elif head == "embedding_dijkstra":
                kw.update(prior_table=ppo.prior_table, dest_slot=ppo.prior_dest_slot)
            elif head == "goal_mlp":
                kw.update(prior_table=ppo.prior_table, dest_slot=ppo.prior_dest_slot, goal_mlp=ppo._goal(),
                          goal_scale=ppo.goal_scale)
            elif head == "graph_transformer":
                kw.update(gt_pe=ppo.gt_pe, gt_weights=ppo._gt())
            self._policy_ev = VecEvaluator(self.eng, head, **kw)
        return self._policy_ev

    @property
    def held(self):
        """Rows the hold rule rewrote in the last policy-driven collection, per environment (None before the first)."""
        return None if self._policy_ev is None else self._policy_ev.held

    def _drive(self, driver):
        eng = self.eng
        if driver == "expert":
            ops.fused_select_next_hop_dest(eng.plan, eng.fs, self.dest_slot, self.table, hold=True)
            return
        ev = self._policy_head()
        logits = ev.logits if ev.head == "embedding" else ev._logits()
        ops.graphdist_rollout(eng.plan, logits, ev.temperature, seed=eng.seed ^ 0x5DEECE66D, counter=eng.sample_counter + 1,
                              sel8=eng.fs.sel8, log_prob=ev.log_prob, scratch=ev.dist_scratch)
        ops.fused_hold_policy_actions(eng.plan, eng.fs, eng.agents, held=ev.held)

    # -- collection ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def collect(self, driver):
        """Reset, then ``frames`` labelled frames under ``driver``; fills the store. -> (labelled rows, mean arrivals)."""
        eng, T = self.eng, self.frames
        K, N = eng.B, eng.N
        eng.fs.check_flags()
        eng.reset()
        if self.keep_idx is not None:
            flat = self.keep_idx.cpu().to(torch.int64)
        else:
            flat = torch.from_numpy(self.np_rng.choice(T * K, size=self.samples, replace=False, shuffle=True).astype("int64"))
        order = torch.argsort(flat, stable=True)
        t_sorted = torch.div(flat[order], K, rounding_mode="floor").tolist()
        keep_env = (flat[order] % K).to(torch.int32).pin_memory().to(eng.device, non_blocking=True)
        keep_slot = order.to(torch.int32).pin_memory().to(eng.device, non_blocking=True)
        bounds = np.searchsorted(np.asarray(t_sorted), np.arange(T + 1))
        self.n_lab.zero_()
        if driver == "policy":          # held <- 0; the embedding head's state-independent logits are filled once
            self._policy_head()._start(False)
        for t in range(T):
            if eng._packed_stale:
                eng.resync()
            refresh_router_tables(eng, t, self.refresh_rate, self.weights, self.dests, self.table, self.tree_scratch)
            ops.fused_expert_labels(eng.plan, eng.fs, self.dest_slot, self.table, out=self.labels, n_labelled=self.n_lab)
            lo, hi = int(bounds[t]), int(bounds[t + 1])
            if hi > lo:
                env, slot = keep_env[lo:hi], keep_slot[lo:hi]
                if self.state_dep:
                    ops.fused_obs16_rows(eng.plan, eng.fs, eng._x, eng.Nmax, eng.agents, env, slot, self.obs_store)
                self.label_store.index_copy_(0, slot.long(), self.labels.index_select(0, env.long()))
            if self.frame_hook is not None:
                self.frame_hook(t)
            self._drive(driver)
            eng.frame_fused(skip_choice=True, reward=self.reward[t])
        eng.fs.check_flags()
        arrivals = float((eng.agents[:, 1:, 8] == 1).sum(1).float().mean())
        return int(self.n_lab.sum()), arrivals

    # -- the update -----------------------------------------------------------------------------------------------------------
    def _obs(self, idx):
        if self.state_dep:
            return self.obs_store.index_select(0, idx)
        return self.ppo.eng.static_node_features[:1].expand(idx.numel(), self.eng.N, 7)

    def minibatch_step(self, idx, n_labelled):
        """One minibatch ``idx`` (store rows, device int64) with ``n_labelled`` labelled nodes in it: head forward,
        ``ops.graphdist_bc``, head backward, Adam. -> (nll (M,) fp64, n_labelled (M,), n_hit (M,)) of the forward."""
        ppo = self.ppo
        obs = self._obs(idx)
        labels = self.label_store.index_select(0, idx)
        logits = ppo._actor_logits(obs)
        nll, nl, nh, g_logits = ops.graphdist_bc(ppo.eng.plan, logits, labels, ppo.temperature,
                                                 grad_scale=1.0 / max(int(n_labelled), 1), scratch=self.bc_scratch)
        ppo.flat.zero_grad()
        ppo._actor_logits_bwd(obs, g_logits)
        self.step += 1
        ops.adam_step_(ppo.flat.flat, ppo.flat.grad, self.exp_avg, self.exp_avg_sq, self.step, lr=self.lr)
        return nll, nl, nh

    @torch.no_grad()
    def evaluate(self):
        """Forward only over the whole store -> (mean loss per labelled node, accuracy, labelled nodes)."""
        ppo = self.ppo
        tot = torch.zeros(3, dtype=torch.float64, device=self.eng.device)
        for lo in range(0, self.samples, self.batch):
            idx = torch.arange(lo, min(lo + self.batch, self.samples), device=self.eng.device)
            nll, nl, nh, _ = ops.graphdist_bc(ppo.eng.plan, ppo._actor_logits(self._obs(idx)),
                                              self.label_store.index_select(0, idx), ppo.temperature, want_grad=False,
                                              scratch=self.bc_scratch)
            tot += torch.stack([nll.sum(), nl.sum().double(), nh.sum().double()])
        s, w, h = tot.tolist()
        return (s / w if w else float("nan")), (h / w if w else float("nan")), int(w)

    @torch.no_grad()
    def update(self):
        """``epochs`` passes over the store -> (loss of the first minibatch, of the last, minibatch steps taken)."""
        per_sample = (self.label_store != ops.BC_IGNORE).sum(1).cpu()          # the expert's bytes are ranks or IGNORE
        first = last = None
        steps = 0
        for _ in range(self.epochs):
            perm = torch.from_numpy(self.np_rng.permutation(self.samples).astype("int64"))
            for lo in range(0, self.samples, self.batch):
                idx = perm[lo:lo + self.batch]
                w = int(per_sample[idx].sum())
                if w == 0:
                    continue            # nothing labelled in this minibatch: no step
                nll, _, _ = self.minibatch_step(idx.to(self.eng.device), w)
                last = (nll, w)
                first = first or last
                steps += 1
        mean = lambda p: float("nan") if p is None else float(p[0].sum()) / p[1]
        return mean(first), mean(last), steps

    def iterate(self):
        """One iteration -> its record (:data:`RECORD_KEYS`)."""
        driver = self.driver if self.driver != "dagger" else ("expert" if self.iteration == 0 else "policy")
        t0 = time.perf_counter()
        labelled, arrivals = self.collect(driver)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, acc0, _ = self.evaluate()
        first, last, _ = self.update()
        _, acc1, _ = self.evaluate()
        torch.cuda.synchronize()
        rec = {"iteration": self.iteration, "driver": driver, "expert": self.expert, "frames": self.frames, "envs": self.eng.B,
               "samples": self.samples, "labelled": labelled,
               "labelled_share": labelled / float(self.frames * self.eng.B * self.eng.N), "loss_first": first,
               "loss_last": last, "accuracy_before": acc0, "accuracy_after": acc1, "arrivals": arrivals,
               "collect_seconds": t1 - t0, "update_seconds": time.perf_counter() - t1}
        self.iteration += 1
        self.records.append(rec)
        return rec
