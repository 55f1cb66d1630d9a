"""Scoring confidence maps by sparsification curves on the device (sr_sparsify; definitions: DESIGN.md
"Scoring confidence maps").

Elements are removed in order of least confidence and the mean error of the remainder is tracked; the same is
done in the oracle order, largest error first.  AUSE is the area between the two curves, AURG the area gained
over random removal:

    curves_from_bins           curves, AUSE, AURG from the device's bin sums.  Host only.
    sparsification_curves      any per-element error with any confidence, [rows, ...], by group of rows
    depth_sparsification       a depth map's error after sr_depth_eval's alignment against its confidence
    evaluate_depth_confidence  the same for the per-view dicts SailRecon.forward / reloc return

There is no confidence gate here: the curve is the sweep over that gate, and ``cut`` holds the confidence
threshold of every step.  There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .cloud_eval import _device_of
from .depth_eval import _as_maps, _as_tensor, _groups_of

Tensor = torch.Tensor

METRICS = ("abs_rel", "abs", "rmse")


def bin_bounds(n: int, n_steps: int) -> np.ndarray:
    """b_k = floor(k n / K), k = 0 .. K, in integers."""
    return np.array([k * int(n) // int(n_steps) for k in range(int(n_steps) + 1)], dtype=np.int64)


def curves_from_bins(bin_sum, n_considered: int, n_steps: int, root: bool = False) -> dict:
    """The sparsification curves of one group from sr_sparsify's ``bin_sum`` [2, K] (row 0 the confidence
    order, row 1 the oracle order) and its considered count n.  Host only.

    curve[c][k] = (sum_{j >= k} bin_sum[c][j]) / (n - b_k), the mean error of what is left after the first b_k
    elements of order c are removed; the suffix sums run from k = K - 1 downwards in fp64.  With ``root`` the
    square root of every mean is taken before anything else (the RMSE curve of squared errors).
    random = curve[0][0] (nothing removed: what random removal keeps on average); ause = mean_k (curve[0][k] -
    curve[1][k]); ause_norm = ause / random (NaN when random is 0); aurg = mean_k (random - curve[0][k]);
    fractions[k] = b_k / n.  Everything is NaN for n = 0."""
    K, n = int(n_steps), int(n_considered)
    s = np.asarray(bin_sum, dtype=np.float64)
    if K < 1 or s.shape != (2, K):
        raise ValueError(f"bin_sum must be [2, {K}], got {s.shape}")
    nan = float("nan")
    if n <= 0:
        return {"curve": np.full((2, K), nan), "fractions": np.full(K, nan), "random": nan, "ause": nan,
                "ause_norm": nan, "aurg": nan}
    b = bin_bounds(n, K)
    # cumsum adds one element after the other: the suffix sums from k = K - 1 downwards
    curve = np.cumsum(s[:, ::-1], axis=1)[:, ::-1] / (n - b[:K]).astype(np.float64)
    if root:
        curve = np.sqrt(curve)
    random = float(curve[0, 0])
    ause = float(np.mean(curve[0] - curve[1]))
    return {"curve": curve, "fractions": b[:K] / np.float64(n), "random": random, "ause": ause,
            "ause_norm": ause / random if random != 0 else nan, "aurg": float(np.mean(random - curve[0]))}


def _check_steps(n_steps) -> int:
    if not (isinstance(n_steps, (int, np.integer)) and 1 <= n_steps <= 1024):
        raise ValueError(f"n_steps must be an integer in [1, 1024], got {n_steps!r}")
    return int(n_steps)


def _run(err: Tensor, conf: Tensor, mask, grp, ng: int, K: int, order: str, root: bool, extra=()) -> dict:
    """ops.sparsify on device rows, one D2H copy (with the fp64 vectors of ``extra`` appended), the curves of
    every group stacked."""
    dev = err.device
    bin_sum = torch.empty(ng, 2, K, device=dev, dtype=torch.float64)
    cut = torch.empty(ng, K, device=dev, dtype=torch.float32)
    count = torch.empty(ng, 2, device=dev, dtype=torch.int32)
    ops.sparsify(err, conf, K, bin_sum, mask=mask, group=grp, n_groups=ng, order=order, cut=cut, count=count)
    # the call's one D2H copy: counts are exact in fp64, cut travels as its bits
    parts = [bin_sum.reshape(-1), cut.reshape(-1).view(torch.int32).to(torch.float64),
             (count.to(torch.int64) & 0xFFFFFFFF).reshape(-1).to(torch.float64)] + [e.reshape(-1) for e in extra]
    host = torch.cat(parts).cpu().numpy()
    pieces = np.split(host, np.cumsum([p.numel() for p in parts])[:-1])
    s = pieces[0].reshape(ng, 2, K)
    cut_h = pieces[1].astype(np.int64).astype(np.int32).view(np.float32).reshape(ng, K)
    cnt = pieces[2].astype(np.int64).reshape(ng, 2)
    rows = [curves_from_bins(s[g], cnt[g, 0], K, root=root) for g in range(ng)]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    out.update(bin_sum=s, cut=cut_h, n_considered=cnt[:, 0].copy(), n_skipped=cnt[:, 1].copy(), n_groups=ng)
    out["_extra"] = pieces[3:]
    return out


def sparsification_curves(err, conf, n_steps: int = 100, mask=None, group=None, order: str = "confidence",
                          root: bool = False) -> dict:
    """Sparsification curves of a per-element error ``err`` under the confidence ``conf`` (tensors or arrays
    [rows, ...] of one shape; host inputs are uploaded), per group of rows (``group``: "view", "scene" or one
    group index per row; default every row its own group).  An element counts where ``mask`` (bool or uint8,
    optional) holds and both values are finite.  ``order`` "confidence" removes the smallest ``conf`` first,
    "uncertainty" the largest.  sr_cloud_nn's ``dist`` with the ``xyz_cnf`` of the same points goes in as it is.

    Returns curves_from_bins' entries, each stacked to [n_groups, ...], with ``cut`` [n_groups, K] (the
    confidence threshold that removes fractions[k]), ``bin_sum``, ``n_considered`` and ``n_skipped``, after one
    D2H copy."""
    K = _check_steps(n_steps)
    if order not in ops.SPARSIFY_ORDER:
        raise ValueError(f"order must be one of {sorted(ops.SPARSIFY_ORDER)}, got {order!r}")
    e, c = _as_tensor(err, "err"), _as_tensor(conf, "conf")
    if e.dim() < 1 or e.numel() == 0 or e.shape != c.shape:
        raise ValueError(f"err and conf must be non-empty [rows, ...] of one shape, got {tuple(e.shape)} and {tuple(c.shape)}")
    m = None
    if mask is not None:
        m = _as_tensor(mask, "mask")
        if m.shape != e.shape or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool or uint8 {tuple(e.shape)}, got {m.dtype} {tuple(m.shape)}")
    n_rows = e.shape[0]
    grp, ng = (None, n_rows) if group is None else _groups_of(group, n_rows)
    dev = _device_of(err, conf, mask)
    flat = lambda t, dt: t.to(device=dev, dtype=dt).reshape(n_rows, -1).contiguous()  # noqa: E731
    out = _run(flat(e, torch.float32), flat(c, torch.float32), None if m is None else flat(m, torch.uint8),
               None if grp is None else grp.to(dev), ng, K, order, bool(root))
    out.pop("_extra")
    return out


def depth_sparsification(pred, gt, conf, valid=None, metric: str = "abs_rel", align: str = "median", scope="view",
                         n_steps: int = 100, xform=None, gt_min: float = 0.0, gt_max: float = float("inf"),
                         order: str = "confidence") -> dict:
    """Sparsification curves of a depth map's error against its confidence.  ``pred``, ``gt``, ``conf`` (and
    the bool ``valid``) are [N, H, W] maps as depth_accuracy takes them; validity, ``align``, ``xform`` and
    ``scope`` are depth_accuracy's, and the curves are per group of the same scope.  The per-pixel error comes
    from one sr_depth_eval call: ``metric`` "abs_rel" is its fl32(|a - g| / g), "abs" is |a - g| and "rmse" is
    (a - g)^2 with the root taken of every mean, both in fp32 from the aligned a.  Invalid pixels are NaN
    there and count as skipped.  ``order`` "uncertainty" reads ``conf`` as an uncertainty.  Returns
    sparsification_curves' entries plus ``scale``, ``shift`` and ``status`` per group."""
    K = _check_steps(n_steps)
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if order not in ops.SPARSIFY_ORDER:
        raise ValueError(f"order must be one of {sorted(ops.SPARSIFY_ORDER)}, got {order!r}")
    if align not in ops.DEPTH_ALIGN:
        raise ValueError(f"align must be one of {sorted(ops.DEPTH_ALIGN)}, got {align!r}")
    if (align == "given") != (xform is not None):
        raise ValueError("xform goes with align='given'")
    p, g, c = _as_maps(pred, "pred"), _as_maps(gt, "gt"), _as_maps(conf, "conf")
    if p.shape != g.shape or p.shape != c.shape:
        raise ValueError(f"pred is {tuple(p.shape)}, gt {tuple(g.shape)}, conf {tuple(c.shape)}: resize before scoring")
    nv, n_pix = p.shape[0], p.shape[1] * p.shape[2]
    m = None
    if valid is not None:
        m = _as_maps(valid, "valid")
        if m.shape != p.shape or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid must be bool {tuple(p.shape)}, got {m.dtype} {tuple(m.shape)}")
    grp, ng = _groups_of(scope, nv)
    dev = _device_of(pred, gt, conf, valid, xform)
    flat = lambda t, dt: t.to(device=dev, dtype=dt).reshape(nv, n_pix).contiguous()  # noqa: E731
    p, g, c = flat(p, torch.float32), flat(g, torch.float32), flat(c, torch.float32)
    m = None if m is None else flat(m, torch.uint8)
    grp = None if grp is None else grp.to(dev)
    if xform is not None:
        xf = _as_tensor(xform, "xform")
        if xf.numel() != 2 * ng:
            raise ValueError(f"xform must be [{ng}, 2] (s, t per group), got {tuple(xf.shape)}")
        xf = xf.to(device=dev, dtype=torch.float64).reshape(ng, 2).contiguous()
    else:
        xf = torch.empty(ng, 2, device=dev, dtype=torch.float64)
    status = torch.empty(ng, device=dev, dtype=torch.int32)
    stats = torch.empty(ng + 1, 16, device=dev, dtype=torch.float64)
    hist = torch.empty(ng + 1, 3, device=dev, dtype=torch.int32)
    rel = torch.empty(nv, n_pix, device=dev, dtype=torch.float32) if metric == "abs_rel" else None
    ali = torch.empty(nv, n_pix, device=dev, dtype=torch.float32) if metric != "abs_rel" else None
    ops.depth_eval(p, g, align=align, xform=xf, status=status, stats=stats, hist=hist, bin_len=1.0, mask=m, group=grp,
                   n_groups=ng, gt_min=gt_min, gt_max=gt_max, aligned=ali, rel_err=rel)
    if metric == "abs_rel":
        err = rel
    else:
        diff = ali - g  # fp32; NaN on invalid pixels
        err = diff.abs() if metric == "abs" else diff * diff
    out = _run(err, c, None, grp, ng, K, order, metric == "rmse", extra=(xf, status.to(torch.float64)))
    x, st = out.pop("_extra")
    x = x.reshape(ng, 2)
    out.update(scale=x[:, 0].copy(), shift=x[:, 1].copy(), status=st.astype(np.int64), metric=metric)
    return out


def evaluate_depth_confidence(predictions, gt_depth, key: str = "depth_map", conf_key: str = "dpt_cnf", **kw) -> dict:
    """depth_sparsification of the depth maps ``key`` and confidences ``conf_key`` of ``predictions`` -- one
    dict or the list of result dicts SailRecon.forward / reloc(save_depth=True) return, as evaluate_depth takes
    them -- against ``gt_depth`` [N, 1, H, W] / [N, H, W].  Further keyword arguments are
    depth_sparsification's."""
    if isinstance(predictions, dict):
        predictions = [predictions]
    if not (isinstance(predictions, (list, tuple)) and predictions and isinstance(predictions[0], dict)):
        raise ValueError("predictions must be a result dict or a non-empty list of them")

    def gather(k):
        maps = []
        for i, v in enumerate(predictions):
            if k not in v:
                raise ValueError(f"predictions[{i}] has no {k!r}")
            t = _as_tensor(v[k], f"predictions[{i}][{k!r}]")
            if t.dim() == 3 and t.shape[-1] == 1:  # one view as [H, W, 1]
                t = t[None]
            maps.append(_as_maps(t, f"predictions[{i}][{k!r}]"))
        if any(mp.shape[1:] != maps[0].shape[1:] for mp in maps):
            raise ValueError(f"the {k!r} maps differ in size")
        return torch.cat([mp.to(maps[0].device) for mp in maps]) if len(maps) > 1 else maps[0]

    return depth_sparsification(gather(key), gt_depth, gather(conf_key), **kw)
