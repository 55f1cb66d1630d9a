"""Reducing and exporting point clouds on the device (sr_cloud_voxel, sr_sort_pairs; definitions: DESIGN.md
"Downsampling point clouds").

    voxel_downsample   points in, one point per occupied voxel out (the mean of its members or its best
                       member), in ascending voxel-key order, deterministic to the bit
    scene_cloud        the views of SailRecon.forward / reloc result dicts as one coloured cloud, filtered by
                       confidence and, with ``voxel``, downsampled
    save_ply           the demo's binary little-endian PLY

There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops
from .cloud_eval import _as_points, _as_xform, _device_of

Tensor = torch.Tensor


def _as_columns(x, name: str, lead, vector: bool = False) -> Tensor:
    """[n, c] from a [..., c] tensor or array whose leading shape is that of the points, ``lead``; [n] from
    [...] for a ``vector``."""
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()  # torch wraps arrays in place and warns about read-only ones
    t = torch.as_tensor(x)
    if vector:
        if tuple(t.shape) != tuple(lead):
            raise ValueError(f"{name} must be {tuple(lead)}, got {tuple(t.shape)}")
        return t.reshape(-1)
    if t.dim() < 1 or tuple(t.shape[:-1]) != tuple(lead):
        raise ValueError(f"{name} must be {tuple(lead)} + (c,), got {tuple(t.shape)}")
    return t.reshape(-1, t.shape[-1])


def voxel_downsample(points, voxel: float, *, attrs=None, weight=None, valid=None, mode: str = "mean",
                     origin=(0.0, 0.0, 0.0), axis_bits: int = 21, xform=None, capacity: Optional[int] = None,
                     return_inverse: bool = False) -> dict:
    """One point per occupied voxel of edge ``voxel`` around ``origin``.  ``points`` [..., 3], ``attrs``
    [..., c <= 8], ``weight`` [...] (mode "best" only) and ``valid`` [...] bool are tensors or arrays (host
    inputs are uploaded); ``xform`` (scale, R, t), or an fp64 vector holding them, is applied inside the
    kernel.  A point counts when it is valid, finite (before and after the transform; under "best" its
    weight is no NaN) and its cell lies in [-2^(axis_bits - 1), 2^(axis_bits - 1)) on every axis.

    Returns device tensors sliced to the voxel count, in ascending key order (z-major, then y, then x):
    ``points`` [m, 3], ``attrs`` [m, c] (or None), ``count`` [m] members, ``index`` [m] (the lowest member
    under "mean", the chosen one under "best"), ``key`` [m] int64 and, with ``return_inverse``, ``inverse``
    [n] int32 (the row of every input point, -1 if it does not count); and the integers ``n_voxels``,
    ``n_considered``, ``n_skipped``, ``n_outside``, read in one D2H copy.  "mean": the fp64 sum of the
    members in ascending input order, divided by the count, rounded once.  "best": the member of largest
    weight, the first of equals.  Raises if ``capacity`` rows do not hold the result."""
    lead = tuple(np.shape(points))[:-1]
    p = _as_points(points, "points")
    dev = _device_of(points, attrs, weight, valid, xform)
    n = p.shape[0]
    up = lambda t, dt: t.to(device=dev, dtype=dt).contiguous()  # noqa: E731
    p = up(p, torch.float32)
    a = None if attrs is None else up(_as_columns(attrs, "attrs", lead), torch.float32)
    w = None if weight is None else up(_as_columns(weight, "weight", lead, True), torch.float32)
    m = None
    if valid is not None:
        m = _as_columns(valid, "valid", lead, True)
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid must be bool or uint8, got {m.dtype}")
        m = up(m, torch.uint8)
    cap = n if capacity is None else int(capacity)
    if not 1 <= cap <= n:
        raise ValueError(f"capacity must be in [1, {n}], got {capacity!r}")
    c = 0 if a is None else a.shape[1]
    out_p = torch.empty(cap, 3, device=dev, dtype=torch.float32)
    out_a = torch.empty(cap, c, device=dev, dtype=torch.float32) if c else None
    count = torch.empty(cap, device=dev, dtype=torch.int32)
    index = torch.empty(cap, device=dev, dtype=torch.int32)
    key = torch.empty(cap, device=dev, dtype=torch.int64)
    inverse = torch.empty(n, device=dev, dtype=torch.int32) if return_inverse else None
    counts = torch.empty(4, device=dev, dtype=torch.int32)
    ops.cloud_voxel(p, float(voxel), out_p, attr=a, mask=m, weight=w, xform=_as_xform(xform, dev, "xform"), origin=origin,
                    axis_bits=axis_bits, mode=mode, capacity=cap, out_attr=out_a, out_count=count, out_index=index,
                    out_key=key, voxel_of=inverse, counts=counts)
    nv, nc, ns, no = (int(v) for v in counts.cpu().tolist())  # the call's one D2H copy
    if nv > cap:
        raise ValueError(f"{nv} voxels are occupied, capacity holds {cap}")
    return {"points": out_p[:nv], "attrs": None if out_a is None else out_a[:nv], "count": count[:nv], "index": index[:nv],
            "key": key[:nv], "inverse": inverse, "n_voxels": nv, "n_considered": nc, "n_skipped": ns, "n_outside": no}


def scene_cloud(predictions, *, key: str = "point_map_by_unprojection", conf_key: str = "dpt_cnf",
                conf_quantile: float = 0.0, conf_thresh: Optional[float] = None, voxel: Optional[float] = None,
                mode: str = "mean", xform=None) -> dict:
    """The views of ``predictions`` (the list of per-view dicts SailRecon.forward and reloc return) as one
    cloud with the attributes r, g, b (from ``images``) and the confidence ``conf_key``.  A pixel is kept
    when its confidence is at least its view's ``conf_quantile`` element (depth_eval.select_quantiles'
    rule, as in evaluate_depth; 0 keeps every pixel whose confidence is no NaN) and, with ``conf_thresh``,
    exceeds it.  With ``voxel`` the kept pixels go through voxel_downsample (under "best" the confidence
    is the weight), whose dict is returned with ``colors`` [m, 3] and ``conf`` [m] added.  Without it the
    kept, finite points are returned as they are (``xform`` is then not applied)."""
    from .depth_eval import select_quantiles
    if not (isinstance(predictions, (list, tuple)) and predictions and isinstance(predictions[0], dict)):
        raise ValueError("predictions must be a non-empty list of per-view dicts")
    dev = _device_of(*[v.get(k) for v in predictions for k in (key, conf_key, "images")])
    pts, rgb, conf = [], [], []
    for k, v in enumerate(predictions):
        for name in (key, conf_key, "images"):
            if name not in v:
                raise ValueError(f"predictions[{k}] has no {name!r}")
        p = _as_points(v[key], f"predictions[{k}][{key!r}]").to(device=dev, dtype=torch.float32)
        c = torch.as_tensor(v[conf_key]).to(device=dev, dtype=torch.float32).reshape(-1)
        im = torch.as_tensor(v["images"]).to(device=dev, dtype=torch.float32)
        if c.numel() != p.shape[0] or im.numel() != 3 * p.shape[0]:
            raise ValueError(f"predictions[{k}]: {p.shape[0]} points, {c.numel()} confidences, {im.numel() // 3} pixels")
        pts.append(p), conf.append(c), rgb.append(im.reshape(3, -1).T)
    keep = []
    same = len({c.numel() for c in conf}) == 1
    if same:  # one select over all views
        thr = select_quantiles(torch.stack(conf), [conf_quantile])[:, 0]
    for k, c in enumerate(conf):
        t = thr[k] if same else select_quantiles(c[None], [conf_quantile])[0, 0]
        ok = c >= t  # a NaN confidence, and every pixel of a view without a finite one, fails
        if conf_thresh is not None:
            ok = ok & (c > conf_thresh)
        keep.append(ok)
    p, c, keep = torch.cat(pts), torch.cat(conf), torch.cat(keep)
    attrs = torch.cat([torch.cat(rgb), c[:, None]], dim=1).contiguous()
    if voxel is None:
        ok = keep & torch.isfinite(p).all(dim=1)
        return {"points": p[ok], "attrs": attrs[ok], "colors": attrs[ok][:, :3], "conf": c[ok], "n_points": int(ok.sum())}
    res = voxel_downsample(p, voxel, attrs=attrs, weight=c if mode == "best" else None, valid=keep, mode=mode, xform=xform)
    res["colors"], res["conf"] = res["attrs"][:, :3], res["attrs"][:, 3]
    return res


def save_ply(path: str, points, colors) -> int:
    """Binary little-endian PLY: x, y, z float32 and uchar red, green, blue = clip(c * 255 + 0.5) of the
    colours in [0, 1] (the layout and the rounding of tools/demo_imc_forward.py's pred.ply).  Returns the
    vertex count."""
    xyz = (points.detach().cpu().numpy() if isinstance(points, Tensor) else np.asarray(points)).reshape(-1, 3)
    rgb = (colors.detach().cpu().float().numpy() if isinstance(colors, Tensor) else np.asarray(colors)).reshape(-1, 3)
    if len(xyz) != len(rgb):
        raise ValueError(f"{len(xyz)} points, {len(rgb)} colours")
    rec = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c8 = np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8)
    rec["r"], rec["g"], rec["b"] = c8[:, 0], c8[:, 1], c8[:, 2]
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(rec)}\n"
                 "property float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode())
        f.write(rec.tobytes())
    return len(rec)
