"""Scoring a predicted point cloud against a ground-truth one on the device (sr_cloud_nn; definitions:
DESIGN.md "Scoring point clouds").

What the reference hands to its ``eval`` package after ``save_pointcloud_with_plyfile``
(train/train_imc.py:301-317; the package is absent from the reference tree): the metrics
reconstruction papers report after a similarity alignment.

    nn_distances             distance of every query point to its nearest target (and its index)
    distance_quantiles       exact order statistics (median, p90, ...) of those distances, on the device
    scores_from_hists        accuracy / completeness / Chamfer / precision / recall / F-score, derived on
                             the host from the two device histograms and moment vectors alone
    cloud_accuracy           both directions of one (pred, gt) and the scores, one D2H copy
    evaluate_reconstruction  the same for the per-view dicts SailRecon.forward / reloc return, aligned
                             to ground-truth poses by sr_pose_align without leaving the device

With ``voxel`` both clouds are first reduced to one point per voxel (cloud_export.voxel_downsample), the
usual protocol of accuracy / completeness, which also makes whole scenes affordable for the brute-force
search.

accuracy is the distance pred -> gt, completeness gt -> pred; precision@t / recall@t are the fractions
of all predicted / ground-truth points closer than t.  The nearest neighbour is found by brute force
from direct coordinate differences in fp32, so a cloud far from the origin keeps its digits.  There is
no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from .pose_eval import MAX_BINS, _as_poses, _fmt, _threshold_bins

Tensor = torch.Tensor

MAX_POINTS = 2 ** 31 - 1


def _check_bins(bin_len: float, n_bins: int) -> None:
    if not (isinstance(n_bins, int) and 0 < n_bins <= MAX_BINS):
        raise ValueError(f"n_bins must be an integer in [1, {MAX_BINS}], got {n_bins!r}")
    if not (np.isfinite(bin_len) and bin_len > 0):
        raise ValueError(f"bin_len must be positive and finite, got {bin_len!r}")


def _as_points(x, name: str, valid=None, allow_empty: bool = False) -> Tensor:
    """[N, 3] from a [..., 3] tensor or array, wherever it lives; ``valid`` [...] bool selects points."""
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()  # torch wraps arrays in place and warns about read-only ones
    try:
        t = torch.as_tensor(x)
    except Exception as e:
        raise ValueError(f"{name} is not a tensor or an array: {e}") from None
    if t.dim() < 1 or t.shape[-1] != 3:
        raise ValueError(f"{name} must be [..., 3], got {tuple(t.shape)}")
    if valid is not None:
        m = torch.as_tensor(valid)
        if m.dtype != torch.bool or tuple(m.shape) != tuple(t.shape[:-1]):
            raise ValueError(f"{name}'s mask must be bool {tuple(t.shape[:-1])}, got {m.dtype} {tuple(m.shape)}")
        t = t[m.to(t.device)]
    t = t.reshape(-1, 3)
    if not (0 if allow_empty else 1) <= t.shape[0] <= MAX_POINTS:
        raise ValueError(f"{name} has {t.shape[0]} points, 1 to {MAX_POINTS} are scored")
    return t


def _device_of(*xs):
    for x in xs:
        if isinstance(x, Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda")


def _upload(t: Tensor, dev) -> Tensor:
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _as_xform(x, dev, name: str) -> Optional[Tensor]:
    """fp64 device vector whose first 13 entries are scale, R row-major, t; a device tensor stays where
    it lies (sr_pose_align's ``out``), a host (scale, R, t) triple or 13-vector is uploaded."""
    if x is None:
        return None
    if isinstance(x, (tuple, list)) and len(x) == 3:
        x = np.concatenate([np.asarray(x[0], np.float64).reshape(1), np.asarray(x[1], np.float64).reshape(9),
                            np.asarray(x[2], np.float64).reshape(3)])
    t = torch.as_tensor(x)
    if t.dim() != 1 or t.numel() < 13:
        raise ValueError(f"{name} must be (scale, R, t) or a vector of at least 13 entries, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float64).contiguous()


def nn_distances(query, target, *, query_xform=None, target_xform=None, return_index: bool = False):
    """``dist`` [Nq] fp32 on the device: the distance of every query point to its nearest target; with
    ``return_index`` also ``index`` [Nq] int32, the lowest index among equally near targets.  A
    non-finite query, or one without a finite target, gets NaN / -1."""
    q, t = _as_points(query, "query"), _as_points(target, "target")
    dev = _device_of(query, target)
    q, t = _upload(q, dev), _upload(t, dev)
    dist = torch.empty(q.shape[0], device=dev, dtype=torch.float32)
    index = torch.empty(q.shape[0], device=dev, dtype=torch.int32) if return_index else None
    ops.cloud_nn(q, t, query_xform=_as_xform(query_xform, dev, "query_xform"),
                 target_xform=_as_xform(target_xform, dev, "target_xform"), dist=dist, index=index)
    return (dist, index) if return_index else dist


def distance_quantiles(dist, fractions: Sequence = (0.5, 0.9)) -> Tensor:
    """[len(fractions)] fp32 on the device: the exact order statistics of the finite entries of
    ``nn_distances``' output (sr_select_ranks: the ascending element max(ceil(q n) - 1, 0), so 0.5 is the
    lower median), which the histogram only brackets to a bin.  NaN if no distance is finite."""
    from .depth_eval import select_quantiles
    d = torch.as_tensor(dist)
    if d.dim() != 1 or d.numel() == 0:
        raise ValueError(f"dist must be a non-empty vector, got {tuple(d.shape)}")
    return select_quantiles(d[None], fractions)[0]


def _side(hist, stats, name: str):
    h = np.asarray(hist).astype(np.int64) & 0xFFFFFFFF  # uint32 counts, whatever the storage
    s = np.asarray(stats, dtype=np.float64)
    if h.ndim != 1 or h.shape[0] < 3:
        raise ValueError(f"hist_{name} must be [n_bins + 2], got {h.shape}")
    if s.shape != (6,):
        raise ValueError(f"stats_{name} must be [6], got {s.shape}")
    n_fin, n_bad = int(s[0]), int(s[4])
    if n_fin + n_bad != int(h.sum()) or n_bad != int(h[-1]):
        raise ValueError(f"hist_{name} and stats_{name} count different numbers of points")
    mean = s[1] / n_fin if n_fin else float("nan")
    rms = float(np.sqrt(s[2] / n_fin)) if n_fin else float("nan")
    return h, n_fin + n_bad, n_bad, float(mean), rms, float(s[3]) if n_fin else float("nan")


def scores_from_hists(hist_acc, hist_comp, stats_acc, stats_comp, thresholds: Sequence[float], bin_len: float) -> dict:
    """The scores of one (pred, gt) from the pred -> gt histogram and moments (``hist_acc`` [n_bins + 2],
    ``stats_acc`` [6] = n_finite, sum d, sum d^2, max d, n_nonfinite, 0) and the gt -> pred ones.  Host
    only.  Means, rms and maxima run over the finite distances; precision@t / recall@t are fractions of
    ALL predicted / ground-truth points (overflow and non-finite points count in the denominator only);
    fscore@t = 2 P R / (P + R), 0 when P + R = 0.  A threshold must be a positive multiple of ``bin_len``
    inside the histogram (ValueError otherwise)."""
    ha, n_pred, bad_pred, acc_mean, acc_rms, acc_max = _side(hist_acc, stats_acc, "acc")
    hc, n_gt, bad_gt, comp_mean, comp_rms, comp_max = _side(hist_comp, stats_comp, "comp")
    if ha.shape != hc.shape:
        raise ValueError(f"the histograms have {ha.shape[0]} and {hc.shape[0]} slots")
    n_bins = ha.shape[0] - 2
    _check_bins(bin_len, n_bins)
    ks = _threshold_bins(thresholds, bin_len, n_bins)
    out = {"acc_mean": acc_mean, "acc_rms": acc_rms, "acc_max": acc_max, "comp_mean": comp_mean, "comp_rms": comp_rms,
           "comp_max": comp_max, "chamfer": (acc_mean + comp_mean) / 2}
    ca, cc = np.cumsum(ha[:n_bins]), np.cumsum(hc[:n_bins])  # c[k - 1] = points below k * bin_len
    for tau, k in zip(thresholds, ks):
        p, r = float(ca[k - 1]) / n_pred, float(cc[k - 1]) / n_gt
        out[f"precision@{_fmt(tau)}"], out[f"recall@{_fmt(tau)}"] = p, r
        out[f"fscore@{_fmt(tau)}"] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    out.update(n_pred=n_pred, n_gt=n_gt, n_nonfinite_pred=bad_pred, n_nonfinite_gt=bad_gt, hist_acc=ha, hist_comp=hc)
    return out


def _accuracy_device(p: Tensor, g: Tensor, xform: Optional[Tensor], n_bins: int, bin_len: float):
    """Both directions into one int32 [2, n_bins + 2] and one fp64 [2, 6] device tensor."""
    hist = torch.empty(2, n_bins + 2, device=p.device, dtype=torch.int32)
    stats = torch.empty(2, 6, device=p.device, dtype=torch.float64)
    ops.cloud_nn(p, g, query_xform=xform, hist=hist[0], bin_len=bin_len, stats=stats[0])
    ops.cloud_nn(g, p, target_xform=xform, hist=hist[1], bin_len=bin_len, stats=stats[1])
    return hist, stats


def _one_copy(hist: Tensor, stats: Tensor, extra: Optional[Tensor] = None):
    """The call's one D2H copy: the counts are exact in fp64."""
    parts = [hist.reshape(-1).to(torch.float64), stats.reshape(-1)] + ([] if extra is None else [extra.reshape(-1)])
    host = torch.cat(parts).cpu().numpy()
    nh = hist.numel()
    return host[:nh].astype(np.int64).reshape(hist.shape), host[nh:nh + 12].reshape(2, 6), host[nh + 12:]


def _voxel_pair(p: Tensor, g: Tensor, xform: Optional[Tensor], voxel: float):
    """Both clouds reduced to the mean point of every occupied voxel of edge ``voxel``: the ground truth in its
    frame, the prediction after ``xform`` (applied inside the kernel, so a device fit stays where it is)."""
    from .cloud_export import voxel_downsample
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError(f"voxel must be positive and finite, got {voxel!r}")
    pv, gv = voxel_downsample(p, voxel, xform=xform), voxel_downsample(g, voxel)
    if pv["n_voxels"] == 0 or gv["n_voxels"] == 0:
        raise ValueError(f"no point left after downsampling at {voxel}: {pv['n_voxels']} predicted, "
                         f"{gv['n_voxels']} ground-truth voxels")
    return pv["points"], gv["points"]


def cloud_accuracy(pred_points, gt_points, thresholds: Sequence[float] = (0.01, 0.02, 0.05), bin_len: float = 0.001,
                   n_bins: int = 1024, xform=None, pred_valid=None, gt_valid=None, voxel: Optional[float] = None) -> dict:
    """scores_from_hists of pred -> gt (accuracy) and gt -> pred (completeness).  Points are [..., 3]
    tensors or arrays (host inputs are uploaded), ``pred_valid`` / ``gt_valid`` optional bool masks of
    their leading shape.  ``xform`` (scale, R, t), or an fp64 vector holding them in that order, maps
    the predicted cloud into the ground-truth frame inside the kernel.  With ``voxel`` the ground-truth cloud
    is downsampled at that edge in its frame and the predicted one after ``xform``, the two reduced clouds
    are scored with no further transform, and the result gains ``n_pred_voxels`` and ``n_gt_voxels``."""
    _check_bins(bin_len, n_bins)
    _threshold_bins(thresholds, bin_len, n_bins)
    p, g = _as_points(pred_points, "pred_points", pred_valid), _as_points(gt_points, "gt_points", gt_valid)
    dev = _device_of(pred_points, gt_points, xform)
    p, g, xf = _upload(p, dev), _upload(g, dev), _as_xform(xform, dev, "xform")
    if voxel is not None:
        p, g = _voxel_pair(p, g, xf, voxel)
        xf = None
    hist, stats = _accuracy_device(p, g, xf, n_bins, float(bin_len))
    h, s, _ = _one_copy(hist, stats)
    res = scores_from_hists(h[0], h[1], s[0], s[1], tuple(thresholds), float(bin_len))
    if voxel is not None:
        res.update(n_pred_voxels=p.shape[0], n_gt_voxels=g.shape[0])
    return res


def evaluate_reconstruction(predictions, gt_points, gt_poses=None, key: str = "point_map_by_unprojection",
                            conf_key: Optional[str] = None, conf_thresh: Optional[float] = None,
                            with_scale: bool = True, thresholds: Sequence[float] = (0.01, 0.02, 0.05),
                            bin_len: float = 0.001, n_bins: int = 1024, gt_valid=None,
                            voxel: Optional[float] = None) -> dict:
    """cloud_accuracy of the points of ``predictions`` (the list of per-view dicts SailRecon.forward and
    reloc return) against ``gt_points``.  The points come from ``key`` ("point_map_by_unprojection", or
    "point_map" with ``conf_key="xyz_cnf"``), kept where ``conf_key`` exceeds ``conf_thresh`` when both
    are given.  With ``gt_poses`` (world-to-camera, as ``pose_eval`` takes them) the predicted frame is
    first aligned to the ground-truth one: sr_pose_align fits gt ~ s R pred + t on the camera centres of
    the predictions' extrinsics, and the fit goes to the kernel as it lies on the device.  The result
    then also carries ``scale``, ``R``, ``t``, ``ate`` and ``status``.  A ``status`` with bit 1 (value 2)
    set means the centres are collinear or coincident and the rotation is NOT unique (two views always
    are): the scores then describe one of many equally good alignments; it is returned, not hidden.
    With ``voxel`` both clouds are downsampled as in cloud_accuracy, the predicted one after the fit, which
    goes to the downsampling kernel as it lies on the device; the result gains ``n_pred_voxels`` and
    ``n_gt_voxels``."""
    _check_bins(bin_len, n_bins)
    _threshold_bins(thresholds, bin_len, n_bins)
    if not (isinstance(predictions, (list, tuple)) and predictions and isinstance(predictions[0], dict)):
        raise ValueError("predictions must be a non-empty list of per-view dicts")
    if (conf_key is None) != (conf_thresh is None):
        raise ValueError("conf_key and conf_thresh go together")
    dev = _device_of(gt_points, *[v.get(key) for v in predictions], *[v.get("extrinsic") for v in predictions])
    views = []
    for k, v in enumerate(predictions):
        if key not in v:
            raise ValueError(f"predictions[{k}] has no {key!r}")
        valid = None
        if conf_key is not None:
            if conf_key not in v:
                raise ValueError(f"predictions[{k}] has no {conf_key!r}")
            valid = torch.as_tensor(v[conf_key]) > conf_thresh
        pts = _as_points(v[key], f"predictions[{k}][{key!r}]", valid, allow_empty=True)
        if pts.shape[0]:
            views.append(_upload(pts, dev))
    if not views:
        raise ValueError("the predictions hold no point" + (f" with {conf_key} above {conf_thresh}" if conf_key else ""))
    p = torch.cat(views) if len(views) > 1 else views[0]
    g = _upload(_as_points(gt_points, "gt_points", gt_valid), dev)
    fit = status = None
    if gt_poses is not None:
        pp, gp = _as_poses(predictions, "predictions"), _as_poses(gt_poses, "gt_poses")
        if pp.shape[0] != gp.shape[0]:
            raise ValueError(f"gt_poses has {gp.shape[0]} views, predictions have {pp.shape[0]}")
        fit = torch.empty(14, device=dev, dtype=torch.float64)
        status = torch.empty(1, device=dev, dtype=torch.int32)
        ops.pose_align(_upload(pp, dev), _upload(gp, dev), fit, status, with_scale=with_scale)
    if voxel is None:
        hist, stats = _accuracy_device(p, g, fit, n_bins, float(bin_len))
    else:
        p, g = _voxel_pair(p, g, fit, voxel)
        hist, stats = _accuracy_device(p, g, None, n_bins, float(bin_len))
    extra = None if fit is None else torch.cat([fit, status.to(torch.float64)])
    h, s, e = _one_copy(hist, stats, extra)
    res = scores_from_hists(h[0], h[1], s[0], s[1], tuple(thresholds), float(bin_len))
    if voxel is not None:
        res.update(n_pred_voxels=p.shape[0], n_gt_voxels=g.shape[0])
    if fit is not None:
        res.update(scale=float(e[0]), R=e[1:10].reshape(3, 3).copy(), t=e[10:13].copy(), ate=float(e[13]),
                   status=int(e[14]))
    return res
