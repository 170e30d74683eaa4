"""Developer tool: per-call device time of the per-decision ops that tools/time_decision_credit.py reaches only inside a
trainer stage — tarl_decision_stats, tarl_decision_critic_loss at M = 1027 and tarl_graphdist_decision_ppo — on the inputs
of the GPU tests (tests/test_gpu_decision_critic.py, tests/test_gpu_decision_credit.py): median [min .. max] of 7 rounds of
50 calls after a warm-up round, HIP events. Another build of the library through TARL_HIP_LIB (profiles/decision_shared_core.txt).

    python tools/time_decision_kernels.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def rounds(fn, reps=7, calls=50):
    v = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            v.append(a.elapsed_time(b) / calls * 1e3)
    return v


def show(name, v):
    print(f"{name:34s} {statistics.median(v):8.2f} us  [{min(v):.2f} .. {max(v):.2f}]", flush=True)


def main():
    import decision_credit_restatement as DC
    import decision_critic_restatement as C
    import test_gpu_decision_credit as TD
    import test_gpu_decision_critic as TC
    from tarl_hip import lib, ops
    print(f"library {lib.LIB_PATH}")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    c = TC._hub_case()
    adv, head = dev(c["adv"]), dev(c["head"])
    show("decision_stats 1027 x 280", rounds(lambda: ops.decision_stats(adv, head)))
    M = c["M"]
    args = TC._dev(c)
    w = TC._weights(ops, C.weights(31))
    nl = torch.tensor([int(c["live"].sum())], dtype=torch.int32, device="cuda")
    grads = torch.zeros(161, device="cuda")
    scratch = torch.empty((ops.decision_critic_scratch_bytes(c["plan"], M) + 7) // 8, dtype=torch.float64, device="cuda")
    show("decision_critic_loss HUB126 M=1027", rounds(lambda: ops.decision_critic_loss(
        c["plan"], *args, w, adv, nl, timestep=c["timestep"], delay_scale=16.0, coef=0.75, grad_scale=0.5, grads=grads,
        scratch=scratch)))
    for name in ("torus9x8", "HUB126"):
        p = TD._loss_inputs(name, 65)
        plan = ops.Plan(p["net"].edge_index, p["N"])
        lg, ch, lpo, a = dev(p["logits"]), dev(p["choice"]), dev(p["lp_old"]), dev(p["adv"])
        hd = dev(np.where(p["live"], 5, 0).astype(np.int32))
        st = dev(DC.decision_stats(p["adv"], p["live"]))
        n_live = torch.tensor([int(p["live"].sum())], dtype=torch.int32).cuda()
        g = torch.zeros((65, p["E"]), device="cuda")
        need = ops._lib.load().tarl_graphdist_decision_ppo_scratch_bytes(plan.handle, 65)
        sc = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        show(f"graphdist_decision_ppo {name} M=65", rounds(lambda: ops.graphdist_decision_ppo(
            plan, lg, ch, hd, lpo, a, st, n_live, clip_epsilon=0.2, temperature=p["T"], grad_scale=0.5, grad_logits=g,
            scratch=sc)))


if __name__ == "__main__":
    main()
