#!/usr/bin/env python
"""Writes tests/golden/g20_cloud_voxel.npz: the cases of tests/cloud_voxel_ref.py (seeded clouds, masks,
weights and a transform) with the answers of the numpy restatement.  Our own data: numpy only, nothing
else is read.

    python tests/golden/make_golden_cloud_voxel.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cloud_voxel_ref as R  # noqa: E402

if __name__ == "__main__":
    z = R.build_golden()
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes")
