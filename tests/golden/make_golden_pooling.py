#!/usr/bin/env python3
"""Generate tests/golden/avgpool_*.npz — the MaskedAveragePooling cases of tests/pooling_cases.py — from the REAL reference.

Same machinery as make_golden.py (reference imported read-only; the fixtures hold the reference's OUTPUTS only, inputs and
weights are regenerated from seeds on both sides).  Runs only where the reference is available.

    python tests/golden/make_golden_pooling.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import numpy as np
import torch

import make_golden
import pooling_cases as pc


def main():
    models, FeatureMap, seed_everything = make_golden.import_reference()
    os.makedirs("/tmp/rat_golden/models", exist_ok=True)
    torch.set_num_threads(1)          # one thread -> reproducible reduction order
    only = sys.argv[1:]
    for case in pc.CASES:
        if only and case["name"] not in only:
            continue
        out = make_golden.run_case(case, models, FeatureMap, seed_everything)
        path = os.path.join(HERE, case["name"] + ".npz")
        np.savez_compressed(path, **out)
        print("%-26s %4d arrays  %7.1f KB  params=%d" % (case["name"], len(out), os.path.getsize(path) / 1024,
                                                          int(out["param_count"])))


if __name__ == "__main__":
    main()
