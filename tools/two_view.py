#!/usr/bin/env python3
"""Two-view relative poses from stored correspondences (sr_two_view): what pose do the matches of every pair
imply, how many of them agree with it, and -- with --poses -- how far are the given poses from it.

    tools/two_view.py CORRES.npz --intrinsics K.txt|fx,fy,cx,cy [--poses PRED.txt] [--threshold 2.0]
                      [--hypotheses 1024] [--refine 8] [--seed 0]

CORRES.npz holds src_coords / dst_coords [P, K, 2] (pixels), src_idx / dst_idx [P] and optionally valid [P, K].
K.txt has one row of 9 numbers per view (row-major 3 x 3); PRED.txt one row of 12 or 16 per view (camera from
world).  Prints one JSON object.  Needs the GPU: there is no CPU path.
"""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervise-sfm_amd"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("corres")
    ap.add_argument("--intrinsics", required=True, help="K.txt (9 numbers per view) or fx,fy,cx,cy for every view")
    ap.add_argument("--poses", help="PRED.txt: 12 or 16 numbers per view, camera from world")
    ap.add_argument("--threshold", type=float, default=2.0, help="inlier threshold on the Sampson distance, pixels")
    ap.add_argument("--hypotheses", type=int, default=1024)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def load_intrinsics(spec: str, n_views: int) -> np.ndarray:
    if os.path.exists(spec):
        k = np.loadtxt(spec, dtype=np.float64, ndmin=2)
        if k.shape[1] != 9:
            raise SystemExit(f"{spec}: 9 numbers per view expected, got {k.shape[1]}")
        return k.reshape(-1, 3, 3).astype(np.float32)
    try:
        fx, fy, cx, cy = (float(v) for v in spec.split(","))
    except ValueError:
        raise SystemExit(f"--intrinsics {spec!r} is neither a file nor fx,fy,cx,cy") from None
    return np.tile(np.float32([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), (n_views, 1, 1))


def load_poses(path: str) -> np.ndarray:
    e = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if e.shape[1] not in (12, 16):
        raise SystemExit(f"{path}: 12 or 16 numbers per view expected, got {e.shape[1]}")
    return e.reshape(len(e), -1, 4)[:, :3, :].astype(np.float32)


def main(argv=None):
    a = parse_args(argv)
    z = np.load(a.corres)
    si, di = np.asarray(z["src_idx"]).reshape(-1), np.asarray(z["dst_idx"]).reshape(-1)
    poses = load_poses(a.poses) if a.poses else None
    n_views = len(poses) if poses is not None else int(max(si.max(), di.max())) + 1
    k = load_intrinsics(a.intrinsics, n_views)
    from sailrecon_amd.utils.two_view import estimate_two_view
    o = estimate_two_view(z["src_coords"], z["dst_coords"], k, si, di, valid=z["valid"] if "valid" in z.files else None,
                          threshold_px=a.threshold, hypotheses=a.hypotheses, refine_iters=a.refine, seed=a.seed,
                          init_extrinsic=poses, ref_extrinsic=poses)
    host = {n: v.cpu().numpy() for n, v in o.items()}
    K = host["inlier_mask"].shape[1]
    pairs = []
    for p in range(len(si)):
        r = {"src": int(si[p]), "dst": int(di[p]), "status": int(host["status"][p]), "inliers": int(host["n_inliers"][p]),
             "inlier_ratio": float(host["n_inliers"][p]) / K, "in_front": int(host["n_front"][p]),
             "cost": float(host["cost"][p]), "R": host["R"][p].tolist(), "t": host["t"][p].tolist()}
        if poses is not None:
            r["rot_err_deg"], r["trans_err_deg"] = (float(v) for v in host["pose_err"][p])
            r["given_pose_cost"] = float(host["init_cost"][p])
        pairs.append(r)
    out = {"n_pairs": len(pairs), "n_estimated": int((host["status"] == 0).sum()), "threshold_px": a.threshold,
           "hypotheses": a.hypotheses, "pairs": pairs}
    if poses is not None:
        e = host["pose_err"]
        for t in (5, 15, 30):
            out[f"rra@{t}"] = float((e[:, 0] < t).mean())
            out[f"rta@{t}"] = float((e[:, 1] < t).mean())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
