#!/usr/bin/env python
"""Score a predicted point cloud against a ground-truth one: accuracy, completeness, Chamfer distance
and precision / recall / F-score at distance thresholds.

    python tools/cloud_eval.py PRED.ply GT.ply [--pred-poses P.txt --gt-poses G.txt] [--no-scale]
                               [--thresholds 0.01 0.02 0.05] [--bin-len 0.001] [--voxel 0.01]

The PLY files are read by the small reader below (``binary_little_endian`` and ``ascii``; the ``x y z``
properties of the ``vertex`` element, whatever else it carries), which reads what ``save_pointcloud_ply``
of tools/demo_imc_forward.py writes (the reference's pred.ply, train/train_imc.py:301-317).  With the
two KITTI pose files (tools/pose_eval.py) the predicted cloud is first brought into the ground-truth
frame by the similarity fit of the camera centres, which stays on the device.  The scores come from
``sailrecon_amd.utils.cloud_eval``, which runs on the device; one JSON line of the result is printed.
With ``--voxel V`` both clouds are first reduced to one point per voxel of edge V (the ground truth in
its frame, the prediction after the fit), as the published accuracy / completeness protocols do.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervise-sfm_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from pose_eval import jsonable, load_kitti_w2c  # noqa: E402

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_xyz(path: str) -> np.ndarray:
    """[N, 3] fp32: the x, y, z properties of a PLY file's vertex element."""
    return read_ply_columns(path, ("x", "y", "z"))


def read_ply_columns(path: str, want=("x", "y", "z"), optional: bool = False):
    """[N, len(want)] fp32: the properties ``want`` of a PLY file's vertex element.  With ``optional``, None
    when the element lacks one of them."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []  # elements: [name, count, [(property, dtype)]]
        while True:
            raw = f.readline()
            if not raw:
                raise ValueError(f"{path}: the header has no end_header")
            w = raw.decode("ascii", "replace").split()
            if not w or w[0] in ("comment", "obj_info"):
                continue
            if w[0] == "end_header":
                break
            if w[0] == "format" and len(w) >= 2:
                fmt = w[1]
            elif w[0] == "element" and len(w) == 3:
                elements.append([w[1], int(w[2]), []])
            elif w[0] == "property" and elements:
                if w[1] == "list":
                    if elements[-1][0] == "vertex":
                        raise ValueError(f"{path}: a list property in the vertex element")
                    elements[-1][2].append((w[-1], None))
                elif len(w) == 3 and w[1] in _PLY_TYPES:
                    elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
                else:
                    raise ValueError(f"{path}: cannot read the header line {raw!r}")
            else:
                raise ValueError(f"{path}: cannot read the header line {raw!r}")
        if fmt not in ("binary_little_endian", "ascii"):
            raise ValueError(f"{path}: format {fmt!r}; binary_little_endian and ascii are read")
        if not elements or elements[0][0] != "vertex":
            raise ValueError(f"{path}: the first element must be vertex")
        _, n, props = elements[0]
        names = [p[0] for p in props]
        if any(c not in names for c in want):
            if optional:
                return None
            raise ValueError(f"{path}: the vertex element has no {', '.join(want)} properties")
        if fmt == "binary_little_endian":
            rec = np.dtype([(name, "<" + t) for name, t in props])
            buf = f.read(n * rec.itemsize)
            if len(buf) != n * rec.itemsize:
                raise ValueError(f"{path}: {n} vertices declared, the file ends after {len(buf) // rec.itemsize}")
            v = np.frombuffer(buf, dtype=rec, count=n)
            return np.stack([v[c] for c in want], axis=1).astype(np.float32)
        cols = [names.index(c) for c in want]
        out = np.empty((n, len(want)), np.float32)
        for i in range(n):
            w = f.readline().split()
            if len(w) != len(props):
                raise ValueError(f"{path}: vertex {i} has {len(w)} values, the header declares {len(props)}")
            out[i] = [float(w[c]) for c in cols]
        return out


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", help="predicted cloud, PLY")
    ap.add_argument("gt", help="ground-truth cloud, PLY")
    ap.add_argument("--pred-poses", help="predicted poses, KITTI format (camera-to-world)")
    ap.add_argument("--gt-poses", help="ground-truth poses, KITTI format (camera-to-world)")
    ap.add_argument("--no-scale", action="store_true", help="rigid alignment (scale 1)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.01, 0.02, 0.05], help="distances")
    ap.add_argument("--bin-len", type=float, default=0.001, help="histogram bin; thresholds are multiples of it")
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--voxel", type=float, default=None, help="downsample both clouds to voxels of this edge first")
    return ap


def main(argv=None) -> dict:
    ap = parser()
    a = ap.parse_args(argv)
    if (a.pred_poses is None) != (a.gt_poses is None):
        ap.error("--pred-poses and --gt-poses go together")
    if a.voxel is not None and not (np.isfinite(a.voxel) and a.voxel > 0):
        ap.error("--voxel must be positive and finite")
    from sailrecon_amd.utils.cloud_eval import cloud_accuracy, evaluate_reconstruction
    pred, gt = read_ply_xyz(a.pred), read_ply_xyz(a.gt)
    kw = dict(thresholds=tuple(a.thresholds), bin_len=a.bin_len, n_bins=a.bins, voxel=a.voxel)
    if a.pred_poses is None:
        res = cloud_accuracy(pred, gt, **kw)
    else:
        pp, gp = load_kitti_w2c(a.pred_poses), load_kitti_w2c(a.gt_poses)
        if len(pp) != len(gp):
            raise ValueError(f"{a.pred_poses} has {len(pp)} poses, {a.gt_poses} has {len(gp)}")
        views = [{"extrinsic": e[None]} for e in pp]
        views[0]["points"] = pred
        for v in views[1:]:
            v["points"] = np.zeros((0, 3), np.float32)
        res = evaluate_reconstruction(views, gt, gt_poses=gp, key="points", with_scale=not a.no_scale, **kw)
    print(json.dumps(jsonable(res)))
    return res


if __name__ == "__main__":
    main()
