"""CPU: behaviour cloning of the shortest-path router (``--pretrain-bc``) — the label rule, the loss and the
update loop restated (``bc_restatement``), what each defect would do instead on a named crafted case, the conditions the
crafted inputs must meet, the realisable single-destination case the GPU test repeats on the device, and the host side: the
new C-ABI entry points (bound, validated before any HIP call, ABI number unchanged), the parser, the argument rules and the
pinned names."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import bc_restatement as BC
import policy_hold_restatement as PH
from conftest import ROOT
from fake_plan import fake_plan as _plan

GRAPHS = ("torus", "MIXED", "HUB126")
K = 3


# ---- 1. the label rule ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    return {name: BC.crafted_labels(name, K) for name in GRAPHS}


def _labels(cr, **kw):
    return BC.expert_labels_envs(cr.x, cr.ag, cr.dest_slot, cr.tables, cr.succ, cr.Nmax, **kw)


@pytest.mark.parametrize("name", GRAPHS)
def test_the_label_rule_on_crafted_rows(crafted, name):
    """>= 20 labelled rows per graph and environment, every "ignore" reason present (empty, untouched: head or slot out of
    range, raw: -1, the row itself, a foreign entry), the named rows as :func:`bc_restatement.crafted_labels` says — a label
    on the LAST rank of the hubs with 9 and 126 out-edges among them — and every label names an out-edge of its row."""
    cr = crafted[name]
    lab = _labels(cr)
    assert int((lab != BC.IGNORE).sum(1).min()) >= 20
    for r, w in cr.why.items():
        want = w if isinstance(w, list) else [w] * K
        assert lab[:, cr.rows[r]].tolist() == want, (name, r)
    on = lab != BC.IGNORE
    assert bool((lab.long()[on] < cr.deg.unsqueeze(0).expand(K, -1)[on]).all())
    assert bool((cr.x[:, :, 3 * cr.Nmax + 1][on] > 0).all())                    # a label is a label on an occupied row
    if name != "torus":
        hub = cr.rows["far"]
        assert int(cr.deg[hub]) == {"MIXED": 9, "HUB126": 126}[name] and int(lab[0, hub]) == int(cr.deg[hub]) - 1
        assert bool((lab.long()[on] >= 4).any())
    # the shared table (nh_bstride 0) is environment 0's
    shared = BC.expert_labels_envs(cr.x, cr.ag, cr.dest_slot, cr.tables[0], cr.succ, cr.Nmax)
    assert torch.equal(shared[0], lab[0]) and not torch.equal(shared[1], lab[1])


@pytest.mark.parametrize("defect,name,rows", [("empty_rows", "torus", ("empty",)), ("held_table", "torus", ("near",)),
                                               ("rank4", "MIXED", ("far", "rank4")), ("rank4", "HUB126", ("far", "rank4")),
                                               ("wrong_env", "torus", ("near",))])
def test_each_label_defect_changes_its_named_case(crafted, defect, name, rows):
    cr = crafted[name]
    good, bad = _labels(cr), _labels(cr, defect=defect)
    for r in rows:
        assert not torch.equal(good[:, cr.rows[r]], bad[:, cr.rows[r]]), (defect, name, r)


# ---- 2. the loss ---------------------------------------------------------------------------------------------------------------
def _loss_case(name, M=5, kind="sharp"):
    net = PH.network(name)
    ei, N = net.edge_index, net.num_roads
    return ei, N, BC.loss_logits(ei, N, M, kind), BC.loss_labels(ei, N, M)


@pytest.mark.parametrize("kind", ["random", "sharp", "sentinel"])
@pytest.mark.parametrize("name", GRAPHS)
def test_the_loss_restated_in_both_precisions_and_against_autograd(name, kind):
    """float64 and fp32 agree to fp32 accuracy (counts and hits exactly), the labelled nodes are those with a byte below
    min(out-degree, 0x7F), an all-ignored sample gives zeros, and the float64 gradient equals torch autograd of
    grad_scale * sum nll at 1e-12."""
    ei, N, lg, lab = _loss_case(name, kind=kind)
    T, scale = 0.7, 1.0 / 37.0
    r64, r32 = BC.bc_loss(ei, N, lg, lab, T, scale), BC.bc_loss(ei, N, lg, lab, T, scale, torch.float32)
    deg = torch.bincount(ei[0], minlength=N)
    assert torch.equal(r64["n_labelled"], (lab.long() < deg.clamp(max=0x7F)).sum(1)) and int(r64["n_labelled"][1:].min()) >= 1
    assert torch.equal(r64["n_labelled"], r32["n_labelled"]) and torch.equal(r64["n_hit"], r32["n_hit"])
    assert int(r64["n_labelled"][0]) == 0 and float(r64["nll"][0]) == 0.0 and not bool(r64["grad"][0].any())
    assert int(r64["n_labelled"][-1]) == 1
    big = max(1.0, float(r64["nll"].abs().max()))
    assert float((r64["nll"] - r32["nll"]).abs().max()) <= 1e-5 * big
    if kind != "sentinel":
        assert float((r64["grad"] - r32["grad"].double()).abs().max()) <= 1e-6
    # autograd of the same loss, written independently
    eid, dg, _ = BC.csr_edges(ei, N)
    x = lg.double().clone().requires_grad_(True)
    z = torch.where(eid >= 0, x[:, eid.clamp(min=0)] / T, torch.full((1,), float("-inf"), dtype=torch.float64))
    labelled = lab.long() < dg.clamp(max=0x7F).unsqueeze(0)
    z_lab = torch.gather(z, 2, lab.long().clamp(max=eid.size(1) - 1).unsqueeze(2)).squeeze(2)
    mx = z.detach().max(2).values        # (torch.logsumexp's own backward loses log(degree) beside a sentinel's 1e20)
    lse = mx + torch.log(torch.exp(z - mx.unsqueeze(2)).sum(2))
    per = torch.where(labelled, lse - torch.where(labelled, z_lab, torch.zeros_like(z_lab)), torch.zeros_like(z_lab))
    (scale * per.sum()).backward()
    tol = 1e-12 if kind != "sentinel" else 1e-12 * 1e20       # a sentinel label's loss is 1e20: relative there
    assert float((per.sum(1).detach() - r64["nll"]).abs().max()) <= tol * max(1.0, N)
    assert float((x.grad - r64["grad"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("defect", BC.LOSS_DEFECTS)
def test_each_loss_defect_changes_its_named_case(defect):
    """MIXED (an unsorted edge list, ties on every fifth node, T = 0.7, samples with different label counts)."""
    ei, N, lg, lab = _loss_case("MIXED")
    assert not bool((ei[0][1:] >= ei[0][:-1]).all())                              # the edge list is not source-sorted
    scale = 1.0 / float((lab.long() < torch.bincount(ei[0], minlength=N).clamp(max=0x7F)).sum())
    good, bad = BC.bc_loss(ei, N, lg, lab, 0.7, scale), BC.bc_loss(ei, N, lg, lab, 0.7, scale, defect=defect)
    if defect == "last_max":
        assert not torch.equal(good["n_hit"], bad["n_hit"]) and torch.equal(good["grad"], bad["grad"])
    else:
        assert float((good["grad"] - bad["grad"]).abs().max()) > 1e-4 * float(good["grad"].abs().max())
    if defect == "wrong_segment":
        assert float((good["nll"] - bad["nll"]).abs().max()) > 1e-3
    if defect == "ignored_grad":      # the difference sits on the edges of nodes that are not labelled
        eid, _, _ = BC.csr_edges(ei, N)
        on = good["labelled"][1]
        e_lab = eid[on][eid[on] >= 0]
        assert torch.equal(good["grad"][1, e_lab], bad["grad"][1, e_lab])


# ---- 3. the loop: the realisable single-destination case ---------------------------------------------------------------------------
def test_the_loop_learns_the_router_on_a_single_destination():
    """The expert driver with the free-flow expert labels 60 frames; the embedding head from N(0, 1), full batch, Adam at
    lr 0.05 for 50 steps: emb = -distance reproduces the router, so the loss must fall to a quarter and the accuracy on the
    labelled rows reach 0.95 (the bounds the device test repeats with a factor two of room for fp32)."""
    net, pop, t0 = BC.single_destination_case()
    run = BC.collect_expert(net, pop, BC.SINGLE["frames"], BC.SINGLE["seed"], t0)
    assert run["arrivals"] > 0 and run["dests"] == [BC.SINGLE["dest"]]
    emb0 = torch.randn(net.num_roads, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    out = BC.bc_loop_embedding(net.edge_index, net.num_roads, run["labels"], emb0, BC.SINGLE["steps"], BC.SINGLE["lr"])
    print(f"[bc host loop] {out['labelled']} labelled rows in {BC.SINGLE['frames']} frames, arrivals {run['arrivals']}, nll "
          f"{out['nll'][0]:.4f} -> {out['nll'][-1]:.4f}, accuracy {out['acc'][0]:.3f} -> {out['acc'][-1]:.3f}")
    assert out["labelled"] >= 500
    assert out["nll"][-1] <= 0.25 * out["nll"][0]
    assert out["acc"][-1] >= 0.95


# ---- 4. the host side ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host():
    from tarl_hip import lib
    L = lib.load()
    null = None
    assert L.tarl_abi_version() == 5
    assert L.tarl_fused_expert_labels(null, null, 1, 15, 1, null, null, 0, 1, null, null, null) == -1
    assert b"null" in L.tarl_last_error()
    assert L.tarl_graphdist_bc_scratch_bytes(null, 4) == -1
    p = _plan(300, 1200)
    ref = ctypes.byref(p)
    assert L.tarl_graphdist_bc_scratch_bytes(ref, 0) == -1
    assert L.tarl_graphdist_bc_scratch_bytes(ref, 4) == 4 * 2 * 16            # two tiles of 256 nodes, 16 bytes each
    assert L.tarl_graphdist_bc_scratch_bytes(ref, 1 << 31) == -1
    assert L.tarl_graphdist_bc_scratch_bytes(ref, (1 << 23) - 1) == ((1 << 24) - 2) * 16      # below 2^24 (sample, tile) pairs
    assert L.tarl_graphdist_bc_scratch_bytes(ref, 1 << 23) == -1                              # 2^24 blocks of 256: refused
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    args = lambda **kw: [kw.get("plan", ref), kw.get("logits", a), kw.get("M", 4), kw.get("T", 1.0), kw.get("labels", a), 1.0,
                         kw.get("nll", a), kw.get("nl", a), kw.get("nh", a), None, kw.get("scratch", a), None]
    for kw, msg in ((dict(plan=None), b"null"), (dict(logits=None), b"null"), (dict(labels=None), b"null"),
                    (dict(nll=None), b"null"), (dict(nl=None), b"null"), (dict(nh=None), b"null"), (dict(scratch=None), b"null"),
                    (dict(M=0), b"M must be positive"), (dict(T=0.0), b"temperature"), (dict(T=-1.0), b"temperature"),
                    (dict(scratch=a + 4), b"aligned")):
        assert L.tarl_graphdist_bc(*args(**kw)) == -1 and msg in L.tarl_last_error(), kw
    assert all(v == 0.0 for v in buf)                                         # a refused call writes nothing


def test_wrapper_refuses_a_small_scratch_before_it_looks_at_the_tensors():
    """``tarl_graphdist_bc`` takes no scratch size, so "scratch too small" is refused by ``ops.graphdist_bc``, from the shapes
    alone. Shown here without a GPU: a stand-in plan (300 nodes: two tiles), HOST tensors, and a scratch one byte short of
    ``tarl_graphdist_bc_scratch_bytes`` is refused with the numbers — while the same call with a scratch of exactly that size
    gets as far as the device check of its tensors and is refused there (no CPU fall-back). Neither writes anything."""
    import types
    from tarl_hip import lib, ops
    hdr = open(os.path.join(ROOT, "include", "tarl_hip.h")).read()
    assert re.search(r"#define TARL_BC_IGNORE 0xFFu", hdr) and ops.BC_IGNORE == 0xFF == BC.IGNORE
    p = _plan(300, 1200)
    plan = types.SimpleNamespace(handle=ctypes.byref(p), num_nodes=300, num_edges=1200)
    M = 5
    need = int(lib.load().tarl_graphdist_bc_scratch_bytes(plan.handle, M))
    assert need == M * 2 * 16
    logits, labels = torch.full((M, 1200), 0.5), torch.full((M, 300), 7, dtype=torch.uint8)
    for short in (torch.zeros(need - 1, dtype=torch.uint8), torch.zeros(need // 8 - 1, dtype=torch.float64), torch.zeros(0)):
        with pytest.raises(ValueError, match=f"scratch holds {short.numel() * short.element_size()} bytes, tarl_graphdist_bc needs {need}"):
            ops.graphdist_bc(plan, logits, labels, scratch=short)
        assert not bool(short.any())
    for enough in (torch.zeros(need, dtype=torch.uint8), torch.zeros(need // 8, dtype=torch.float64)):
        with pytest.raises(lib.TarlError, match="must live on the GPU|GPU"):
            ops.graphdist_bc(plan, logits, labels, scratch=enough)
        assert not bool(enough.any())
    assert bool((logits == 0.5).all()) and bool((labels == 7).all())
    with pytest.raises(ValueError, match="logits must be"):
        ops.graphdist_bc(plan, logits[:, :-1], labels)
    with pytest.raises(ValueError, match="temperature positive"):
        ops.graphdist_bc(plan, logits, labels, temperature=0.0)


def test_bc_trainer_refuses_an_unfused_engine():
    """``BCTrainer`` runs on the packed path only, as the evaluator does: an engine without it is refused before anything else
    is looked at (stand-in engines: the check comes first)."""
    import types
    from tarl_hip import lib
    from tarl_hip.imitation import BCTrainer
    fused, plain = types.SimpleNamespace(fs=object()), types.SimpleNamespace(fs=None)
    for ppo_eng, eng in ((fused, plain), (plain, fused), (plain, plain)):
        with pytest.raises(lib.TarlError, match="BCTrainer needs the fused engine"):
            BCTrainer(types.SimpleNamespace(eng=ppo_eng), eng)


def test_parser_and_argument_rules():
    main = importlib.import_module("main")
    from src.runner import BC_DRIVER_NAMES, BC_EXPERT_NAMES, RunnerArgs
    from tarl_hip import imitation
    assert BC_DRIVER_NAMES == imitation.DRIVERS and BC_EXPERT_NAMES == tuple(imitation.EXPERTS)
    assert imitation.EXPERTS == {"dijkstra": 10, "free_flow": 0}
    assert imitation.RECORD_KEYS == ("iteration", "driver", "expert", "frames", "envs", "samples", "labelled", "labelled_share",
                                     "loss_first", "loss_last", "accuracy_before", "accuracy_after", "arrivals",
                                     "collect_seconds", "update_seconds")
    ns = main.build_parser().parse_args(["--algo", "mpnn", "--mode", "train"])
    assert ns.pretrain_bc == 0 and all(getattr(ns, k) is None for k in ("bc_expert", "bc_driver", "bc_envs", "bc_frames",
                                                                         "bc_samples", "bc_epochs", "bc_batch", "bc_lr"))
    RunnerArgs(**vars(ns))
    ns = main.build_parser().parse_args(["--algo", "mpnn+ppo", "--mode", "train", "--pretrain-bc", "3", "--bc-expert",
                                         "free_flow", "--bc-driver", "policy", "--bc-envs", "4", "--bc-frames", "20",
                                         "--bc-samples", "64", "--bc-epochs", "2", "--bc-batch", "16", "--bc-lr", "0.01"])
    a = RunnerArgs(**vars(ns))
    assert (a.pretrain_bc, a.bc_expert, a.bc_driver, a.bc_envs, a.bc_frames, a.bc_samples, a.bc_epochs, a.bc_batch, a.bc_lr) == \
        (3, "free_flow", "policy", 4, 20, 64, 2, 16, 0.01)
    base = dict(algo="mpnn", scenario="synthetic-1024-300", mode="train")
    for flag, v in (("bc_expert", "dijkstra"), ("bc_driver", "expert"), ("bc_envs", 4), ("bc_frames", 8), ("bc_samples", 8),
                    ("bc_epochs", 1), ("bc_batch", 4), ("bc_lr", 0.1)):
        with pytest.raises(ValueError, match="needs --pretrain-bc"):
            RunnerArgs(**base, **{flag: v})
    with pytest.raises(ValueError, match="needs mode 'train'"):
        RunnerArgs(algo="mpnn", scenario="synthetic-1024-300", mode="eval", pretrain_bc=2)
    with pytest.raises(ValueError, match="needs algo mpnn or mpnn\\+ppo"):
        RunnerArgs(algo="dijkstra", scenario="synthetic-1024-300", mode="train", pretrain_bc=2)
    for flag, v in (("bc_envs", 0), ("bc_lr", 0.0), ("bc_expert", "astar"), ("bc_driver", "teacher")):
        with pytest.raises(ValueError, match=flag):
            RunnerArgs(**base, pretrain_bc=1, **{flag: v})
    with pytest.raises(ValueError, match="pretrain_bc must be >= 0"):
        RunnerArgs(**base, pretrain_bc=-1)
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--bc-driver", "teacher"])
