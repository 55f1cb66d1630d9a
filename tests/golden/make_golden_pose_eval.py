"""Golden data for the pose-scoring kernels (sr_pose_pair_errors): g14_pose_eval.npz (build container
only; the reference tree is imported read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pose_eval.py

Data only: the poses of the pair cases of tests/pose_eval_ref.py and, for one explicit pair list,
what the reference's own compute_relative_pose (train/utils/geometry.py:240-282; pad_poses,
torch.inverse and torch.bmm in fp32) returns for them, next to the same product with an fp64 inverse
of the same inputs.  The reference module imports networkx at the top, which compute_relative_pose
never touches: if it is missing, an empty stand-in module is registered before the import.

Seeds: per case the seeds are searched upward from pose_eval_ref.SEED0[case]; the first one for which
every histogram run of the case (pose_eval_ref.RUNS) meets the margin condition -- every fp64 error,
rotation, translation and their maximum, at least 10 x its bound from every positive bin edge -- is
kept.  The bound is the case's own: 4 x the fp32 restatement's largest error against the fp64 one.

Stored per case: <case>/pred [n, 3, 4] fp32, <case>/gt [n, 4, 4] fp32, <case>/seed.
Stored for the list: rel/case, rel/pair_i, rel/pair_j, rel/gt_ref and rel/pred_ref [P, 4, 4] fp32 (the
reference's outputs), rel/gt_inv64 and rel/pred_inv64 [P, 4, 4] fp64 (dst @ inv(src) in fp64).
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SFM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "train"))
sys.dont_write_bytecode = True

try:
    import networkx  # noqa: F401
except ImportError:
    sys.modules["networkx"] = types.ModuleType("networkx")

from utils.geometry import compute_relative_pose  # noqa: E402

import pose_eval_ref as R  # noqa: E402

OUT = os.path.join(HERE, "g14_pose_eval.npz")
REL_CASE = "a33"


def find_seed(name: str):
    runs = [r for r in R.RUNS if r["case"] == name]
    for seed in range(R.SEED0[name], R.SEED0[name] + 5000):
        pred, gt = R.make_pair_case(name, seed)
        bounds = R.bounds_of(pred, gt)
        margins = [R.margin_of(r, pred, gt, bounds) for r in runs]
        if min(margins) >= R.MARGIN:
            return seed, pred, gt, bounds, margins
    raise SystemExit(f"{name}: no seed meets the margin condition")


def main():
    out = {}
    for name in R.PAIR_CASES:
        seed, pred, gt, bounds, margins = find_seed(name)
        out[f"{name}/pred"], out[f"{name}/gt"], out[f"{name}/seed"] = pred, gt, np.int64(seed)
        print(f"{name}: seed {seed}, bounds rot {bounds[0]:.3e} trans {bounds[1]:.3e} deg, margins "
              + " ".join(f"{m:.1f}" for m in margins))
    pred, gt = out[f"{REL_CASE}/pred"], out[f"{REL_CASE}/gt"]
    i, j = R.explicit_pairs(len(pred))
    keep = (i < len(pred)) & (j < len(pred))  # the reference has no rule for an index out of range
    i, j = i[keep], j[keep]
    out["rel/case"], out["rel/pair_i"], out["rel/pair_j"] = np.array(REL_CASE), i, j
    for key, T in (("gt", gt), ("pred", pred)):
        src, dst = torch.from_numpy(np.ascontiguousarray(T[i])), torch.from_numpy(np.ascontiguousarray(T[j]))
        ref = compute_relative_pose(src, dst)
        assert ref.dtype == torch.float32 and tuple(ref.shape) == (len(i), 4, 4)
        out[f"rel/{key}_ref"] = ref.numpy()
        pad = lambda x: np.concatenate([x[:, :3, :].astype(np.float64),  # noqa: E731
                                        np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (len(x), 1, 1))], 1)
        out[f"rel/{key}_inv64"] = pad(T[j]) @ np.linalg.inv(pad(T[i]))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes")
    assert size < 64 * 1024


if __name__ == "__main__":
    main()
