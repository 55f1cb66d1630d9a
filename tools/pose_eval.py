#!/usr/bin/env python
"""Score a predicted trajectory against ground truth: RRA / RTA / AUC and the aligned ATE.

    python tools/pose_eval.py PRED.txt GT.txt [--no-scale] [--thresholds 5 15 30]

Both files are KITTI pose files as ``save_kitti_poses`` writes them (tools/demo_imc_forward.py;
the reference's pred.txt, train/demo_imc_forward.py:118-128): one line per frame, the 3x4 top of the
camera-to-world pose, row-major, 12 numbers.  They are inverted to world-to-camera in fp64 on the
host and handed to ``sailrecon_amd.utils.pose_eval.evaluate_poses``, which runs on the device; one
JSON line of its result is printed.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervise-sfm_amd"))


def load_kitti_w2c(path: str) -> np.ndarray:
    """[N, 4, 4] fp32 world-to-camera poses from a KITTI camera-to-world file (inverted in fp64)."""
    rows = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                v = [float(x) for x in line.split()]
            except ValueError:
                raise ValueError(f"{path}:{n}: not a line of numbers") from None
            if len(v) != 12:
                raise ValueError(f"{path}:{n}: {len(v)} numbers, a KITTI pose line has 12")
            rows.append(v)
    if not rows:
        raise ValueError(f"{path}: no poses")
    c2w = np.tile(np.eye(4), (len(rows), 1, 1))
    c2w[:, :3, :4] = np.asarray(rows, dtype=np.float64).reshape(-1, 3, 4)
    return np.linalg.inv(c2w).astype(np.float32)


def jsonable(res: dict) -> dict:
    out = {}
    for k, v in res.items():
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        out[k] = v.tolist() if isinstance(v, np.ndarray) else v
    return out


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", help="predicted poses, KITTI format (camera-to-world)")
    ap.add_argument("gt", help="ground-truth poses, KITTI format (camera-to-world)")
    ap.add_argument("--no-scale", action="store_true", help="rigid alignment (scale 1) for the ATE")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[5, 15, 30], help="degrees")
    a = ap.parse_args(argv)
    from sailrecon_amd.utils.pose_eval import evaluate_poses
    pred, gt = load_kitti_w2c(a.pred), load_kitti_w2c(a.gt)
    if len(pred) != len(gt):
        raise ValueError(f"{a.pred} has {len(pred)} poses, {a.gt} has {len(gt)}")
    res = evaluate_poses(pred, gt, thresholds=tuple(a.thresholds), with_scale=not a.no_scale)
    print(json.dumps(jsonable(res)))
    return res


if __name__ == "__main__":
    main()
