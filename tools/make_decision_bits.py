#!/usr/bin/env python3
"""Developer tool: writes tests/golden/decision_bits.npz — the bit patterns the goal head's backward (csrc/goal_mlp.hip), the
decision critic's loss (csrc/decision_critic.hip) and the per-decision PPO objective and statistics
(csrc/decision_credit.hip) return for the cases of tests/test_gpu_decision_bits.py. Needs a GPU. Run it with the library
whose bits are to be pinned (the tree's own, or another build through TARL_HIP_LIB) BEFORE restructuring the kernels; the
test then holds the new code to those bits.

    python tools/make_decision_bits.py [--out tests/golden/decision_bits.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decision_bits.npz"))
    a = ap.parse_args()
    import test_gpu_decision_bits as T
    from tarl_hip import lib
    out = {}
    for case, fn, args in T.CASES:
        for name, bits in fn(*args).items():
            floats = bits.numpy().view(np.float32 if bits.numpy().dtype == np.int32 else np.float64)
            assert np.isfinite(floats).all(), (case, name)
            out[f"{case}/{name}"] = bits.numpy()
        print(f"{case}: done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} from {lib.LIB_PATH}: {len(out)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
