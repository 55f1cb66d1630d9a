#!/usr/bin/env python
"""Writes tests/golden/g19_depth_eval.npz: the cases of tests/depth_eval_ref.py (seeded depth maps with
planted invalid pixels) with the fp64 restatement's alignments, sums, histograms and quantiles.  Our own
data: numpy only, nothing else is read.

    python tests/golden/make_golden_depth_eval.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import depth_eval_ref as R  # noqa: E402

if __name__ == "__main__":
    z = R.build_golden()
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes; seed {int(z['seed'])}, "
          f"margin {R.margins(z):.1f} ulps")
