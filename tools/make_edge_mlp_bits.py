#!/usr/bin/env python3
"""Developer tool: writes tests/golden/edge_mlp_bits.npz — the fp32 bit patterns the edge-MLP kernels (csrc/edge_mlp.hip)
return for the cases of tests/test_gpu_edge_mlp_bits.py: the logits of the four forward paths and the six gradients of one
backward call accumulated onto G0 from a NaN-filled scratch. Needs a GPU. Run it with the library whose bits are to be pinned
(the tree's own, or another build through TARL_HIP_LIB) BEFORE restructuring the kernels; the test then holds the new code
to those bits.

    python tools/make_edge_mlp_bits.py [--out tests/golden/edge_mlp_bits.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tarl-simulator_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "edge_mlp_bits.npz"))
    a = ap.parse_args()
    import edge_mlp_restatement as R
    import test_gpu_edge_mlp_bits as T
    from tarl_hip import lib
    out = {}
    for E, M in T.BITS_CASES:
        for name, bits in T.device_bits(E, M).items():
            assert np.isfinite(bits.numpy().view(np.float32)).all(), (E, M, name)
            out[f"{R.case_id((E, M))}/{name}"] = bits.numpy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} from {lib.LIB_PATH}: {len(out)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
