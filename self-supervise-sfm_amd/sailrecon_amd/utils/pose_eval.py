"""Scoring predicted camera poses against ground truth on the device (sr_pose_pair_errors,
sr_pose_align; definitions: DESIGN.md "Scoring poses").

What the reference's demos hand to their ``eval`` package (train/demo_imc_forward.py:109-128; the
package is absent from the reference tree), on the relative pose of compute_relative_pose
(train/utils/geometry.py:240-282):

    pose_pair_errors   per-pair relative rotation / translation errors in degrees
    pose_accuracy      RRA@t, RTA@t and AUC@t, derived on the host from the device histogram alone
    align_poses        Umeyama fit of the camera centres and the absolute trajectory error (ATE)
    evaluate_poses     both, merged

Poses are world-to-camera [R|t] (OpenCV), as ``predictions[i]["extrinsic"]`` and
``batch["poses_w2c"]``: [N, 3, 4], [N, 4, 4] or [1, N, ...] tensors or arrays, or the list of per-view
dicts SailRecon.forward / reloc return.  Host inputs are uploaded; 3x4 predictions against 4x4 ground
truth is the normal case.  There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .. import ops

Tensor = torch.Tensor

MAX_VIEWS = 65535
MAX_BINS = 1024


def _as_poses(x, name: str) -> Tensor:
    """[N, 3, 4] or [N, 4, 4] from any accepted form of ``name``, checked, wherever it lives."""
    if isinstance(x, (list, tuple)) and len(x) > 0 and isinstance(x[0], dict):
        views = []
        for k, v in enumerate(x):
            if "extrinsic" not in v:
                raise ValueError(f"{name}[{k}] has no 'extrinsic'")
            e = torch.as_tensor(v["extrinsic"])
            if e.dim() < 2 or tuple(e.shape[-2:]) not in ((3, 4), (4, 4)):
                raise ValueError(f"{name}[{k}]['extrinsic'] must end in 3x4 or 4x4, got {tuple(e.shape)}")
            if views and e.shape[-2] != views[0].shape[-2]:
                raise ValueError(f"{name}[{k}]['extrinsic'] is {tuple(e.shape[-2:])}, {name}[0]'s is "
                                 f"{tuple(views[0].shape[-2:])}")
            views.append(e.reshape(-1, *e.shape[-2:]))
        t = torch.cat([v.to(views[0].device) for v in views])
    else:
        if isinstance(x, np.ndarray) and not x.flags.writeable:
            x = x.copy()  # torch wraps arrays in place and warns about read-only ones
        try:
            t = torch.as_tensor(x)
        except Exception as e:
            raise ValueError(f"{name} is not a tensor, an array or a list of per-view dicts: {e}") from None
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3 or tuple(t.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"{name} must be [N, 3, 4], [N, 4, 4] or [1, N, ...], got {tuple(t.shape)}")
    if t.shape[0] == 0:
        raise ValueError(f"{name} has no views")
    if t.shape[0] > MAX_VIEWS:
        raise ValueError(f"{name} has {t.shape[0]} views, at most {MAX_VIEWS}")
    return t


def _device_of(*xs):
    for x in xs:
        if isinstance(x, Tensor) and x.is_cuda:
            return x.device
        if isinstance(x, (list, tuple)) and x and isinstance(x[0], dict):
            e = x[0].get("extrinsic")
            if isinstance(e, Tensor) and e.is_cuda:
                return e.device
    return torch.device("cuda")


def _inputs(pred, gt, pairs=None):
    """(pred, gt, pair_i, pair_j) on the device, fp32 / int32 and contiguous; every check comes
    before the first upload."""
    p, g = _as_poses(pred, "pred"), _as_poses(gt, "gt")
    if p.shape[0] != g.shape[0]:
        raise ValueError(f"gt has {g.shape[0]} views, pred has {p.shape[0]}")
    pi, pj = _pair_lists(pairs)
    dev = _device_of(pred, gt)
    up = lambda t, dt: None if t is None else t.to(device=dev, dtype=dt).contiguous()  # noqa: E731
    return up(p, torch.float32), up(g, torch.float32), up(pi, torch.int32), up(pj, torch.int32)


def _pair_lists(pairs):
    if pairs is None:
        return None, None
    if isinstance(pairs, (tuple, list)) and len(pairs) == 2 and not np.isscalar(pairs[0]):
        i, j = torch.as_tensor(pairs[0]), torch.as_tensor(pairs[1])
    else:
        t = torch.as_tensor(pairs)
        if t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"pairs must be (pair_i, pair_j) or [P, 2], got {tuple(t.shape)}")
        i, j = t[:, 0], t[:, 1]
    if i.dim() != 1 or j.dim() != 1 or i.numel() != j.numel() or i.numel() == 0:
        raise ValueError(f"pairs must hold two equally long non-empty index vectors, got {tuple(i.shape)} and "
                         f"{tuple(j.shape)}")
    if i.is_floating_point() or j.is_floating_point():
        raise ValueError("pairs must hold integer indices")
    # indices beyond int32 are out of range whatever the view count: -1 keeps them so
    fit = lambda v: torch.where((v < 0) | (v > 2 ** 31 - 1), torch.full_like(v, -1), v).to(torch.int32)  # noqa: E731
    return fit(i), fit(j)


def _check_bins(bin_deg: float, n_bins: int) -> None:
    if not (isinstance(n_bins, int) and 0 < n_bins <= MAX_BINS):
        raise ValueError(f"n_bins must be an integer in [1, {MAX_BINS}], got {n_bins!r}")
    if not (np.isfinite(bin_deg) and bin_deg > 0):
        raise ValueError(f"bin_deg must be positive and finite, got {bin_deg!r}")


def _threshold_bins(thresholds: Sequence[float], bin_deg: float, n_bins: int):
    out = []
    for tau in thresholds:
        k = tau / bin_deg
        if not (np.isfinite(k) and k > 0 and abs(k - round(k)) <= 1e-9 * max(1.0, abs(k))):
            raise ValueError(f"threshold {tau} is not a positive multiple of bin_deg {bin_deg}")
        if round(k) > n_bins:
            raise ValueError(f"threshold {tau} lies beyond the histogram's {n_bins} bins of {bin_deg} degrees")
        out.append(int(round(k)))
    return out


def _fmt(tau) -> str:
    return f"{tau:g}"


def accuracy_from_hist(hist, thresholds: Sequence[float] = (5, 15, 30), bin_deg: float = 1.0) -> dict:
    """RRA / RTA / AUC from a [3, n_bins + 2] histogram (rows rot / trans / max; slot n_bins overflow,
    slot n_bins + 1 non-finite).  RRA@t, RTA@t: fractions of all pairs below t; AUC@t = (1/K) sum_{k=1..K}
    F(k bin_deg), K = t / bin_deg, F the fraction of all pairs with max error below its argument.
    Overflow and non-finite pairs count in the denominator only."""
    h = np.asarray(hist).astype(np.int64) & 0xFFFFFFFF  # uint32 counts, whatever the storage
    if h.ndim != 2 or h.shape[0] != 3 or h.shape[1] < 3:
        raise ValueError(f"hist must be [3, n_bins + 2], got {h.shape}")
    n_bins = h.shape[1] - 2
    _check_bins(bin_deg, n_bins)
    ks = _threshold_bins(thresholds, bin_deg, n_bins)
    total = int(h[0].sum())
    if not (int(h[1].sum()) == total == int(h[2].sum())):
        raise ValueError("hist rows count different numbers of pairs")
    out = {"n_pairs": total, "n_nonfinite": int(h[0, n_bins + 1])}
    cum = np.cumsum(h[:, :n_bins], axis=1)  # cum[r, k - 1] = pairs of row r below k * bin_deg
    for tau, k in zip(thresholds, ks):
        out[f"rra@{_fmt(tau)}"] = float(cum[0, k - 1]) / total if total else float("nan")
        out[f"rta@{_fmt(tau)}"] = float(cum[1, k - 1]) / total if total else float("nan")
        out[f"auc@{_fmt(tau)}"] = float(cum[2, :k].sum()) / (k * total) if total else float("nan")
    out["hist"] = h
    return out


def pose_pair_errors(pred, gt, pairs=None, trans_ambiguity: bool = True) -> Tuple[Tensor, Tensor]:
    """(rot_deg, trans_deg) [P] fp32 on the device: all i < j in lexicographic order, or the explicit
    ``pairs`` ((pair_i, pair_j) or [P, 2]; any order, i == j and repeats allowed; an index outside
    [0, N) gives NaN)."""
    p, g, pi, pj = _inputs(pred, gt, pairs)
    n = p.shape[0]
    n_pairs = pi.numel() if pi is not None else n * (n - 1) // 2
    rot = torch.empty(n_pairs, device=p.device, dtype=torch.float32)
    trans = torch.empty_like(rot)
    hist = torch.empty(3, 3, device=p.device, dtype=torch.int32)
    ops.pose_pair_errors(p, g, hist, bin_deg=180.0, trans_ambiguity=trans_ambiguity, pair_i=pi, pair_j=pj,
                         rot_err=rot, trans_err=trans)
    return rot, trans


def _accuracy(p: Tensor, g: Tensor, pi, pj, thresholds, trans_ambiguity, bin_deg, n_bins) -> dict:
    hist = torch.empty(3, n_bins + 2, device=p.device, dtype=torch.int32)
    ops.pose_pair_errors(p, g, hist, bin_deg=bin_deg, trans_ambiguity=trans_ambiguity, pair_i=pi, pair_j=pj)
    return accuracy_from_hist(hist.cpu().numpy(), thresholds, bin_deg)  # the one D2H copy


def pose_accuracy(pred, gt, thresholds: Sequence[float] = (5, 15, 30), pairs=None, trans_ambiguity: bool = True,
                  bin_deg: float = 1.0, n_bins: int = 180) -> dict:
    """{rra@t, rta@t, auc@t for every threshold, n_pairs, n_nonfinite, hist}.  Thresholds must be
    multiples of ``bin_deg`` inside the histogram's range (ValueError otherwise)."""
    _check_bins(bin_deg, n_bins)
    _threshold_bins(thresholds, bin_deg, n_bins)
    p, g, pi, pj = _inputs(pred, gt, pairs)
    return _accuracy(p, g, pi, pj, tuple(thresholds), trans_ambiguity, float(bin_deg), n_bins)


def _align(p: Tensor, g: Tensor, with_scale: bool, per_view: bool) -> dict:
    out = torch.empty(14, device=p.device, dtype=torch.float64)
    status = torch.empty(1, device=p.device, dtype=torch.int32)
    err = torch.empty(p.shape[0], device=p.device, dtype=torch.float64) if per_view else None
    ops.pose_align(p, g, out, status, with_scale=with_scale, err=err)
    o = out.cpu().numpy()
    res = {"scale": float(o[0]), "R": o[1:10].reshape(3, 3).copy(), "t": o[10:13].copy(), "ate": float(o[13]),
           "status": int(status.cpu())}
    if per_view:
        res["err"] = err
    return res


def align_poses(pred, gt, with_scale: bool = True, per_view: bool = False) -> dict:
    """Umeyama fit gt ~ scale R pred + t of the camera centres c = -R^T t over all views:
    {scale, R [3, 3], t [3], ate (ground-truth units), status[, err [N] fp64 on the device]}.
    status: 2 = the covariance has rank < 2 and the rotation is not unique (the ATE still holds),
    3 = the predicted centres coincide (scale 1, R = I, t the difference of the means)."""
    p, g, _, _ = _inputs(pred, gt)
    return _align(p, g, with_scale, per_view)


def evaluate_poses(pred, gt, thresholds: Sequence[float] = (5, 15, 30), pairs=None, trans_ambiguity: bool = True,
                   bin_deg: float = 1.0, n_bins: int = 180, with_scale: bool = True, per_view: bool = False) -> dict:
    """pose_accuracy and align_poses of one (pred, gt), merged."""
    _check_bins(bin_deg, n_bins)
    _threshold_bins(thresholds, bin_deg, n_bins)
    p, g, pi, pj = _inputs(pred, gt, pairs)
    res = _accuracy(p, g, pi, pj, tuple(thresholds), trans_ambiguity, float(bin_deg), n_bins)
    res.update(_align(p, g, with_scale, per_view))
    return res
