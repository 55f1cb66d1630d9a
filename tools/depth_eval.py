#!/usr/bin/env python
"""Score predicted depth maps against reference depth: AbsRel, SqRel, RMSE, RMSE-log, SILog, log10,
delta < 1.25^k and inlier fractions after an alignment of the prediction, per view or per scene.

    python tools/depth_eval.py PRED.npy GT.npy [--valid V.npy] [--conf C.npy --conf-quantile Q]
                               [--align none|median|scale|scale_shift] [--scope view|scene | --groups 0 0 1 ...]
                               [--thresholds 0.05 0.1 0.25] [--bin-len 0.005] [--bins 1024]

PRED.npy and GT.npy hold [N, H, W] (or [N, 1, H, W], [N, H, W, 1], [H, W]) maps of one size; zeros, NaN
and Inf in GT are invalid pixels.  --conf-quantile Q keeps the most confident 1 - Q of each view.  The
scores come from ``sailrecon_amd.utils.depth_eval``, which runs on the device; one JSON line of the
result (without the histogram) is printed.
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

from pose_eval import jsonable  # noqa: E402

ALIGNS = ("none", "median", "scale", "scale_shift")


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", help="predicted depth maps, .npy")
    ap.add_argument("gt", help="reference depth maps, .npy (0 / NaN / Inf = invalid)")
    ap.add_argument("--valid", help="bool or uint8 maps, .npy: pixels to score")
    ap.add_argument("--conf", help="confidence maps, .npy")
    ap.add_argument("--conf-quantile", type=float, help="drop the least confident fraction of each view")
    ap.add_argument("--align", choices=ALIGNS, default="median")
    ap.add_argument("--scope", choices=("view", "scene"), default="view")
    ap.add_argument("--groups", type=int, nargs="+", help="one group index per view (instead of --scope)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.05, 0.1, 0.25], help="relative errors")
    ap.add_argument("--bin-len", type=float, default=0.005, help="histogram bin; thresholds are multiples of it")
    ap.add_argument("--bins", type=int, default=1024)
    a = ap.parse_args(argv)
    if (a.conf is None) != (a.conf_quantile is None):
        ap.error("--conf and --conf-quantile go together")
    if a.conf_quantile is not None and not 0 <= a.conf_quantile <= 1:
        ap.error("--conf-quantile must lie in [0, 1]")
    return a


def main(argv=None) -> dict:
    a = parse_args(argv)
    from sailrecon_amd.utils.depth_eval import depth_accuracy
    load = lambda p: None if p is None else np.load(p, allow_pickle=False)  # noqa: E731
    res = depth_accuracy(load(a.pred), load(a.gt), valid=load(a.valid), conf=load(a.conf), conf_quantile=a.conf_quantile,
                         align=a.align, scope=a.groups if a.groups is not None else a.scope,
                         thresholds=tuple(a.thresholds), bin_len=a.bin_len, n_bins=a.bins)
    res.pop("hist")
    print(json.dumps(jsonable(res)))
    return res


if __name__ == "__main__":
    main()
