#!/usr/bin/env python
"""Writes tests/golden/g22_cloud_render.npz: the golden cloud and cameras of tests/cloud_render_ref.py, the
images of the numpy restatement at radius 0 and 1, and -- the part that needs the reference checkout, read-only
and only when this script is run by hand -- the ``image_points`` [3, N, 2] and ``cam_points`` [3, 3, N] that the
reference's project_world_points_to_cam (sailrecon/utils/geometry.py:215-303) gives for them in fp64 on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cloud_render.py REFERENCE_ROOT

Two margins are asserted on the inputs: every u + 0.5 and v + 0.5 of a point inside the depth range is at
least 1e-6 from an integer, and every c_z at least 1e-6 (relative) from z_near and z_far.  With them the integer
pixels and the classes of the reference's projection and of the restatement must agree exactly, and the real
(u, v) to 1e-9 px: the reference multiplies with bmm, the restatement in a fixed association.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import cloud_render_ref as R  # noqa: E402


def reference_projection(points, extrinsic, intrinsic, root):
    import torch
    sys.path.insert(0, root)
    from sailrecon.utils.geometry import project_world_points_to_cam
    img, cam = project_world_points_to_cam(torch.from_numpy(points).double(), torch.from_numpy(extrinsic).double(),
                                           torch.from_numpy(intrinsic).double())
    return img.numpy(), cam.numpy()


def check_against(z, img, cam):
    """The assertions of the module docstring; tests/test_cloud_render.py repeats them on the stored arrays."""
    H, W = R.HW
    p, E, K = z["points"], z["extrinsic"], z["intrinsic"]
    assert R.margins_ok(p, E, K).all()
    pr = R.project(p, E, K, R.HW, z_near=R.GOLDEN_NEAR, z_far=R.GOLDEN_FAR)
    assert img.shape == (R.GOLDEN_V, R.GOLDEN_N, 2) and cam.shape == (R.GOLDEN_V, 3, R.GOLDEN_N)
    assert np.abs(cam - pr["c"]).max() <= 1e-12
    live = pr["state"] != R.CLIPPED
    assert ((cam[:, 2] >= R.GOLDEN_NEAR) & (cam[:, 2] <= R.GOLDEN_FAR) == live).all()
    assert np.abs(img - pr["uv"])[live].max() <= 1e-9
    ix, iy = np.floor(img[..., 0] + 0.5), np.floor(img[..., 1] + 0.5)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    drawn = pr["state"] == R.DRAWN
    assert (inside[live] == drawn[live]).all()
    assert (ix[drawn] == pr["ix"][drawn]).all() and (iy[drawn] == pr["iy"][drawn]).all()
    assert (pr["state"] == R.CLIPPED).any() and (pr["state"] == R.OUTSIDE).any() and (cam[:, 2] < 0).any()


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_cloud_render.py REFERENCE_ROOT (the checkout that holds sailrecon/utils/geometry.py)")
    root = sys.argv[1]
    z = R.build_golden()
    img, cam = reference_projection(z["points"], z["extrinsic"], z["intrinsic"], root)
    check_against(z, img, cam)
    z["ref/image_points"], z["ref/cam_points"] = img, cam
    np.savez_compressed(R.GOLDEN, **z)
    print(f"{R.GOLDEN}: {len(z)} arrays, {os.path.getsize(R.GOLDEN)} bytes")
