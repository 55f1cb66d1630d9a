#!/usr/bin/env python
"""Writes tests/golden/g21_sparsify.npz: the cases of tests/sparsify_ref.py (seeded errors, confidences,
masks and groups) with the answers of the numpy restatement.  Our own data: numpy only, nothing else is
read.

    python tests/golden/make_golden_sparsify.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import sparsify_ref as R  # noqa: E402

if __name__ == "__main__":
    z = R.build_golden()
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes")
