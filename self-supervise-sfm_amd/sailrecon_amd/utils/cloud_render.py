"""Rendering point clouds into camera views on the device (sr_cloud_render; definitions: DESIGN.md "Rendering
point clouds").

    render_cloud             points and cameras in; per camera a z-buffered depth image, the index of the point
                             every pixel shows and the point's attributes, deterministic to the bit
    render_predictions       the views of SailRecon.forward / reloc result dicts as one cloud, drawn into each of
                             the scene's own predicted cameras, every view without its own points (``cross``)
    cross_view_consistency   that rendering scored against every view's own depth map: what the other views say
                             about this view's depth

There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .cloud_eval import _as_points, _as_xform, _device_of
from .cloud_export import _as_columns

Tensor = torch.Tensor


def _as_cameras(extrinsic, intrinsic, dev):
    e, k = torch.as_tensor(extrinsic), torch.as_tensor(intrinsic)
    if e.dim() == 2:
        e, k = e[None], k[None]
    if e.dim() != 3 or tuple(e.shape[1:]) not in ((3, 4), (4, 4)) or tuple(k.shape) != (e.shape[0], 3, 3):
        raise ValueError(f"extrinsic must be [V, 3, 4] (or [V, 4, 4]) and intrinsic [V, 3, 3], got {tuple(e.shape)} and "
                         f"{tuple(k.shape)}")
    up = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    return up(e[:, :3, :]), up(k)


def render_cloud(points, extrinsic, intrinsic, hw, *, attrs=None, valid=None, view_id=None, exclude=None, radius: int = 0,
                 z_near: float = 1e-6, z_far: float = float("inf"), xform=None, attr_fill: float = float("nan")) -> dict:
    """Draws ``points`` [..., 3] into the V cameras ``extrinsic`` [V, 3, 4] (camera from world, OpenCV) /
    ``intrinsic`` [V, 3, 3] (zero skew) at ``hw`` = (H, W), pixel centres at integers.  Inputs are tensors or
    arrays (host inputs are uploaded).  ``attrs`` [..., c <= 8] ride along; ``valid`` [...] bool; ``view_id`` [...]
    and ``exclude`` [V] integers: view v does not draw the points whose view_id is exclude[v]; ``radius`` 0 .. 3 is
    the half width of the square footprint; ``xform`` (scale, R, t), or an fp64 vector holding them, is applied
    to the points inside the kernel.  A pixel shows the nearest point that covers it, the lowest index among
    equal fp32 depths.

    Returns device tensors ``depth`` [V, H, W] fp32 (NaN where nothing was drawn, the invalid pixel of
    depth_accuracy), ``index`` [V, H, W] int32 (-1 there), ``attrs`` [V, H, W, c] (``attr_fill`` there; None
    without attrs) and ``counts`` [V, 4] int32 (covered pixels, drawn, clipped, outside points), and ``coverage``,
    a host list of one dict per view (covered, drawn, clipped, outside, skipped, fraction = covered / (H W)) from
    one D2H copy of the counts."""
    lead = tuple(np.shape(points))[:-1]
    p = _as_points(points, "points")
    dev = _device_of(points, extrinsic, intrinsic, attrs, valid, view_id, xform)
    n = p.shape[0]
    H, W = (int(v) for v in hw)
    if not (isinstance(radius, (int, np.integer)) and 0 <= radius <= 3):
        raise ValueError(f"radius must be an integer in [0, 3], got {radius!r}")
    if (view_id is None) != (exclude is None):
        raise ValueError("view_id and exclude go together")
    up = lambda t, dt: t.to(device=dev, dtype=dt).contiguous()  # noqa: E731
    p = up(p, torch.float32)
    e, k = _as_cameras(extrinsic, intrinsic, dev)
    V = e.shape[0]
    a = None if attrs is None else up(_as_columns(attrs, "attrs", lead), torch.float32)
    m = vid = exc = None
    if valid is not None:
        m = _as_columns(valid, "valid", lead, True)
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid must be bool or uint8, got {m.dtype}")
        m = up(m, torch.uint8)
    if view_id is not None:
        vid = up(_as_columns(view_id, "view_id", lead, True), torch.int32)
        exc = up(torch.as_tensor(exclude).reshape(-1), torch.int32)
        if exc.numel() != V:
            raise ValueError(f"exclude must have one entry per view ({V}), got {exc.numel()}")
    c = 0 if a is None else a.shape[1]
    depth = torch.empty(V, H, W, device=dev, dtype=torch.float32)
    index = torch.empty(V, H, W, device=dev, dtype=torch.int32)
    out_a = torch.empty(V, H, W, c, device=dev, dtype=torch.float32) if c else None
    counts = torch.empty(V, 4, device=dev, dtype=torch.int32)
    ops.cloud_render(p, e, k, (H, W), attr=a, mask=m, view_id=vid, exclude=exc, xform=_as_xform(xform, dev, "xform"),
                     radius=int(radius), z_near=z_near, z_far=z_far, attr_fill=attr_fill, depth=depth, index=index,
                     out_attr=out_a, counts=counts)
    host = counts.cpu().numpy().astype(np.int64) & 0xFFFFFFFF  # the call's one D2H copy
    coverage = [{"covered": int(r[0]), "drawn": int(r[1]), "clipped": int(r[2]), "outside": int(r[3]),
                 "skipped": int(n - r[1] - r[2] - r[3]), "fraction": float(r[0]) / (H * W)} for r in host]
    return {"depth": depth, "index": index, "attrs": out_a, "counts": counts, "coverage": coverage}


def _scene(predictions, key: str, conf_key: str, extra=()):
    """Per-view tensors of the result dicts: points [S, H W, 3], confidences [S, H W], colours [S, H W, 3],
    cameras, (H, W), and the maps of ``extra`` as [S, H, W]."""
    if not (isinstance(predictions, (list, tuple)) and predictions and isinstance(predictions[0], dict)):
        raise ValueError("predictions must be a non-empty list of per-view dicts")
    need = (key, conf_key, "images", "extrinsic", "intrinsic") + tuple(extra)
    dev = _device_of(*[v.get(k) for v in predictions for k in need])
    cols = {k: [] for k in need}
    hw = None
    for i, v in enumerate(predictions):
        for name in need:
            if name not in v:
                raise ValueError(f"predictions[{i}] has no {name!r}")
        im = torch.as_tensor(v["images"]).to(device=dev, dtype=torch.float32)
        if im.dim() < 3 or im.numel() != 3 * im.shape[-2] * im.shape[-1]:
            raise ValueError(f"predictions[{i}]['images'] must be one [3, H, W] image, got {tuple(im.shape)}")
        if hw is None:
            hw = (int(im.shape[-2]), int(im.shape[-1]))
        if tuple(im.shape[-2:]) != hw:
            raise ValueError("the views differ in size")
        n = hw[0] * hw[1]
        p = _as_points(v[key], f"predictions[{i}][{key!r}]").to(device=dev, dtype=torch.float32)
        if p.shape[0] != n:
            raise ValueError(f"predictions[{i}]: {p.shape[0]} points for {n} pixels")
        cols[key].append(p), cols["images"].append(im.reshape(3, n).T)
        for name in (conf_key,) + tuple(extra):
            t = torch.as_tensor(v[name]).to(device=dev, dtype=torch.float32)
            if t.numel() != n:
                raise ValueError(f"predictions[{i}][{name!r}] has {t.numel()} entries for {n} pixels")
            cols[name].append(t.reshape(n))
        cols["extrinsic"].append(torch.as_tensor(v["extrinsic"]).to(device=dev, dtype=torch.float32).reshape(-1, 4)[:3])
        cols["intrinsic"].append(torch.as_tensor(v["intrinsic"]).to(device=dev, dtype=torch.float32).reshape(3, 3))
    return {k: torch.stack(v) for k, v in cols.items()}, hw, dev


def render_predictions(predictions, *, key: str = "point_map_by_unprojection", conf_key: str = "dpt_cnf",
                       conf_quantile: float = 0.0, cross: bool = True, radius: int = 0) -> dict:
    """The views of ``predictions`` (the list of per-view dicts SailRecon.forward and reloc return) as one cloud
    -- the points ``key``, the colours of ``images`` and the confidence ``conf_key`` as a fourth attribute, a
    pixel kept by scene_cloud's rule (its confidence at least its view's ``conf_quantile`` element) -- drawn
    into each of the scene's own predicted cameras.  With ``cross`` view v does not draw the points that came
    from view v: the image is what the other views say about it.  Returns render_cloud's dict with ``colors``
    [S, H, W, 3] and ``conf`` [S, H, W] added."""
    from .depth_eval import select_quantiles
    s, hw, dev = _scene(predictions, key, conf_key)
    S, n = s[conf_key].shape
    thr = select_quantiles(s[conf_key], [conf_quantile])[:, :1]
    keep = s[conf_key] >= thr  # a NaN confidence, and every pixel of a view without a finite one, fails
    attrs = torch.cat([s["images"], s[conf_key][..., None]], dim=-1)
    vid = torch.arange(S, device=dev, dtype=torch.int32)
    res = render_cloud(s[key].reshape(S * n, 3), s["extrinsic"], s["intrinsic"], hw, attrs=attrs.reshape(S * n, 4),
                       valid=keep.reshape(S * n), view_id=vid[:, None].expand(S, n).reshape(S * n) if cross else None,
                       exclude=vid if cross else None, radius=radius)
    res["colors"], res["conf"] = res["attrs"][..., :3], res["attrs"][..., 3]
    return res


def cross_view_consistency(predictions, *, key: str = "point_map_by_unprojection", depth_key: str = "depth_map",
                           conf_key: str = "dpt_cnf", radius: int = 0, **depth_kw) -> dict:
    """What the other views say about every view's depth: render_predictions(cross=True), then
    depth_eval.depth_accuracy(rendered, own depth, valid = isfinite(rendered) & own depth valid, align="none"),
    per view and pooled; further keyword arguments are depth_accuracy's.  Returns its dict with, added,
    ``coverage`` [S] (the share of a view's valid pixels -- own depth finite and positive -- that some other view
    reaches) and, on the device, ``rendered`` [S, H, W] (NaN where no other view reaches), ``rel_err`` [S, H, W]
    (|rendered - own| / own, NaN where either is invalid) and ``conf`` [S, H, W], the views' own ``conf_key``.
    These three go into conf_eval.sparsification_curves unchanged:

        r = cross_view_consistency(predictions)
        curves = sparsification_curves(r["rel_err"], r["conf"])
    """
    from .depth_eval import depth_accuracy
    if "align" in depth_kw or "valid" in depth_kw:
        raise ValueError("align and valid are fixed here: align='none', valid = rendered finite and own depth valid")
    s, hw, dev = _scene(predictions, key, conf_key, extra=(depth_key,))
    res = render_predictions(predictions, key=key, conf_key=conf_key, cross=True, radius=radius)
    S = s[depth_key].shape[0]
    own = s[depth_key].reshape(S, *hw)
    rendered = res["depth"]
    own_valid = torch.isfinite(own) & (own > 0)
    valid = torch.isfinite(rendered) & own_valid
    out = depth_accuracy(rendered, own, valid=valid, align="none", **depth_kw)
    both = torch.stack([valid.reshape(S, -1).sum(dim=1), own_valid.reshape(S, -1).sum(dim=1)]).cpu().numpy()
    with np.errstate(all="ignore"):
        out["coverage"] = both[0] / both[1].astype(np.float64)
    nan = torch.full_like(own, float("nan"))
    out["rendered"] = rendered
    out["rel_err"] = torch.where(valid, (rendered - own).abs() / own, nan)
    out["conf"] = s[conf_key].reshape(S, *hw)
    out["render"] = res
    return out
