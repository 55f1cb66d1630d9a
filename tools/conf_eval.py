#!/usr/bin/env python
"""Score a depth map's confidence by sparsification curves: the error of what is left when the least
confident pixels are removed, against the oracle order that removes the largest error first (AUSE, AURG).

    python tools/conf_eval.py PRED.npy GT.npy CONF.npy [--valid V.npy] [--metric abs_rel|abs|rmse]
                              [--align none|median|scale|scale_shift] [--scope view|scene | --groups 0 0 1 ...]
                              [--steps 100] [--uncertainty]

PRED.npy, GT.npy and CONF.npy hold [N, H, W] (or [N, 1, H, W], [N, H, W, 1], [H, W]) maps of one size; zeros,
NaN and Inf in GT are invalid pixels.  --uncertainty reads CONF.npy as an uncertainty: the largest value is
removed first.  The curves come from ``sailrecon_amd.utils.conf_eval``, which runs on the device; one JSON
line of the result (without the bin sums) is printed.
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
METRICS = ("abs_rel", "abs", "rmse")


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", help="predicted depth maps, .npy")
    ap.add_argument("gt", help="reference depth maps, .npy (0 / NaN / Inf = invalid)")
    ap.add_argument("conf", help="confidence maps, .npy")
    ap.add_argument("--valid", help="bool or uint8 maps, .npy: pixels to score")
    ap.add_argument("--metric", choices=METRICS, default="abs_rel")
    ap.add_argument("--align", choices=ALIGNS, default="median")
    ap.add_argument("--scope", choices=("view", "scene"), default="view")
    ap.add_argument("--groups", type=int, nargs="+", help="one group index per view (instead of --scope)")
    ap.add_argument("--steps", type=int, default=100, help="points of the curve, 1 .. 1024")
    ap.add_argument("--uncertainty", action="store_true", help="CONF holds an uncertainty: largest removed first")
    a = ap.parse_args(argv)
    if not 1 <= a.steps <= 1024:
        ap.error("--steps must lie in [1, 1024]")
    return a


def main(argv=None) -> dict:
    a = parse_args(argv)
    from sailrecon_amd.utils.conf_eval import depth_sparsification
    load = lambda p: None if p is None else np.load(p, allow_pickle=False)  # noqa: E731
    res = depth_sparsification(load(a.pred), load(a.gt), load(a.conf), valid=load(a.valid), metric=a.metric,
                               align=a.align, scope=a.groups if a.groups is not None else a.scope, n_steps=a.steps,
                               order="uncertainty" if a.uncertainty else "confidence")
    res.pop("bin_sum")
    print(json.dumps(jsonable(res)))
    return res


if __name__ == "__main__":
    main()
