"""Depth unprojection and point projection — drop-in for sailrecon/utils/geometry.py:19-130 and :215-303.

``unproject_depth_points`` runs on device (sr_unproject_depth_f32).
``unproject_depth_map_to_point_map`` keeps the reference's contract: it returns a numpy array
of world points [S, H, W, 3] in float64, which the reference produces from its float64
closed-form SE(3) inverse (geometry.py:132-186).  The arithmetic here is fp32 on the GPU;
only the result is copied to the host.

``project_world_points_to_cam`` / ``img_from_cam`` keep the reference's signatures and returned shapes
(image points B x N x 2, camera points B x 3 x N).  They are plain torch on whatever device and dtype their
arguments have: the check of a convention, not a hot path.  The z-buffered renderer that draws with this
projection is sr_cloud_render (utils/cloud_render.py).
"""

from __future__ import annotations

import numpy as np
import torch

from .. import ops, runtime


def unproject_depth_points(depth_map: torch.Tensor, extrinsics_cam: torch.Tensor,
                           intrinsics_cam: torch.Tensor) -> torch.Tensor:
    """depth [S, H, W] or [S, H, W, 1], extrinsic [S, 3, 4] (cam from world, OpenCV),
    intrinsic [S, 3, 3] (zero skew) -> world points [S, H, W, 3] fp32 on device."""
    runtime.require_device(depth_map, "unproject_depth_points")
    d = depth_map.detach().float()
    if d.dim() == 4:
        d = d.squeeze(-1)
    d = d.contiguous()
    S, H, W = d.shape
    e = extrinsics_cam.detach().float().reshape(S, 3, 4).contiguous()
    k = intrinsics_cam.detach().float().reshape(S, 3, 3).contiguous()
    out = torch.empty(S, H, W, 3, device=d.device, dtype=torch.float32)
    ops.unproject_depth(d, e, k, out)
    return out


def unproject_depth_map_to_point_map(depth_map, extrinsics_cam, intrinsics_cam) -> np.ndarray:
    """Reference-compatible wrapper: same arguments, numpy float64 [S, H, W, 3] result."""
    pts = unproject_depth_points(depth_map, extrinsics_cam, intrinsics_cam)
    return pts.cpu().numpy().astype(np.float64)


def project_world_points_to_cam(world_points, cam_extrinsics, cam_intrinsics=None, distortion_params=None, default=0,
                                only_points_cam=False):
    """world points [N, 3], extrinsics [B, 3, 4] (cam from world, OpenCV), intrinsics [B, 3, 3] ->
    (image points [B, N, 2], camera points [B, 3, N]); (None, camera points) with ``only_points_cam``."""
    if distortion_params is not None:
        raise NotImplementedError("distortion models are not part of this projection")
    homogeneous = torch.cat([world_points, torch.ones_like(world_points[:, :1])], dim=1)  # [N, 4]
    cam_points = torch.matmul(cam_extrinsics, homogeneous.T.unsqueeze(0))  # [B, 3, 4] x [1, 4, N]
    if only_points_cam:
        return None, cam_points
    return img_from_cam(cam_intrinsics, cam_points, default=default), cam_points


def img_from_cam(cam_intrinsics, cam_points, distortion_params=None, default=0.0):
    """intrinsics [B, 3, 3], camera points [B, 3, N] -> pixel coordinates [B, N, 2]: K (x / z, y / z, 1), a
    NaN replaced by ``default``."""
    if distortion_params is not None:
        raise NotImplementedError("distortion models are not part of this projection")
    xy = (cam_points / cam_points[:, 2:3, :])[:, :2, :]
    pixels = torch.matmul(cam_intrinsics, torch.cat([xy, torch.ones_like(xy[:, :1, :])], dim=1))[:, :2, :]
    return torch.nan_to_num(pixels, nan=default).transpose(1, 2)
