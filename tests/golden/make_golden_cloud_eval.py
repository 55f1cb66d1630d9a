#!/usr/bin/env python
"""Writes tests/golden/g18_cloud_eval.npz: the cases of tests/cloud_eval_ref.py (seeded clouds and
transforms) with their fp64 nearest-neighbour answers.  Our own data: numpy only, nothing else is read.

    python tests/golden/make_golden_cloud_eval.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cloud_eval_ref as R  # noqa: E402

if __name__ == "__main__":
    z = R.build_golden()
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes; hist seed {int(z['hist/seed'])}")
