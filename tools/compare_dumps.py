#!/usr/bin/env python
"""Compare two `bench.py --dump-outputs` directories (e.g. SR_CAMERA_ONLY=0 against =1).

    python tools/compare_dumps.py DIR_A DIR_B [bf16|fp32]

Prints one EQUIV line per array (extrinsic, intrinsic, cam_tokens): the rel-L2 of DIR_B's against
DIR_A's and its bound, goldens.parity_tol of the mode (bf16: poses 2e-3, camera tokens 1e-2).
Exit status 1 if a bound is missed.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervise-sfm_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from goldens import parity_tol, rel_l2  # noqa: E402


def main():
    a, b = sys.argv[1:3]
    mode = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    ok = True
    for k in ("extrinsic", "intrinsic", "cam_tokens"):
        x, y = np.load(os.path.join(a, k + ".npy")), np.load(os.path.join(b, k + ".npy"))
        err, tol = rel_l2(y, x), parity_tol(k, mode)
        print(f"EQUIV {k}: shape {x.shape} rel-L2 {err:.3e} (bound {tol:g}){'' if err < tol else '  MISSED'}")
        ok &= err < tol
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
