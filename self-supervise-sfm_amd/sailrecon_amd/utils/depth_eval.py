"""Scoring predicted depth maps against reference depth on the device (sr_depth_eval, sr_select_ranks;
definitions: DESIGN.md "Scoring depth maps").

The numbers depth papers report, after an alignment of the prediction (median ratio, least-squares
scale, or scale and shift), per group of views and pooled:

    select_quantiles   exact order statistics of a device tensor's rows, by group
    metrics_from_stats AbsRel, SqRel, RMSE, RMSE-log, SILog, log10, delta < 1.25^k and inlier fractions,
                       derived on the host from the device's sums, counts and histogram alone
    depth_accuracy     one (pred, gt) of [N, H, W] maps scored, one D2H copy
    evaluate_depth     the same for the per-view dicts SailRecon.forward / reloc return

The reference depth is what the reference's training batch carries per view at model resolution with
zeros invalid (``depth_pr_processed``, train/datasets/imc2021.py:277-296).  Shapes must match: resizing
stays with the caller.  There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

from fractions import Fraction
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from .cloud_eval import _check_bins, _device_of
from .pose_eval import MAX_VIEWS, _fmt, _threshold_bins

Tensor = torch.Tensor

MAX_DEN = 2 ** 20
N_STATS = 16


def rank_fraction(q) -> tuple:
    """(num, den) of a quantile for sr_select_ranks: the closest fraction with den <= 2^20 (0.5 -> 1 / 2,
    0.9 -> 9 / 10); a (num, den) pair passes through."""
    if isinstance(q, (tuple, list)) and len(q) == 2:
        num, den = int(q[0]), int(q[1])
    else:
        if not (isinstance(q, (int, float, Fraction, np.floating)) and 0 <= q <= 1):
            raise ValueError(f"a quantile must lie in [0, 1], got {q!r}")
        f = Fraction(float(q)).limit_denominator(MAX_DEN)
        num, den = f.numerator, f.denominator
    if not 0 <= num <= den <= MAX_DEN or den < 1:
        raise ValueError(f"a rank fraction needs 0 <= num <= den <= {MAX_DEN}, got {num} / {den}")
    return num, den


def rank_index(num: int, den: int, n: int) -> int:
    """The index sr_select_ranks picks among n ascending values: max(ceil(num n / den) - 1, 0)."""
    return max((num * n + den - 1) // den - 1, 0)


def _as_tensor(x, name: str) -> Tensor:
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()  # torch wraps arrays in place and warns about read-only ones
    try:
        return torch.as_tensor(x)
    except Exception as e:
        raise ValueError(f"{name} is not a tensor or an array: {e}") from None


def _as_maps(x, name: str) -> Tensor:
    """[N, H, W] from [H, W], [N, H, W], [N, 1, H, W], [N, H, W, 1], [1, N, H, W] or [1, N, H, W, 1],
    wherever it lives."""
    t = _as_tensor(x, name)
    if t.dim() == 5 and t.shape[0] == 1 and t.shape[-1] == 1:
        t = t[0, ..., 0]
    elif t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    elif t.dim() == 4 and t.shape[-1] == 1:
        t = t[..., 0]
    elif t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    elif t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or 0 in t.shape:
        raise ValueError(f"{name} must be [N, H, W], [N, 1, H, W], [N, H, W, 1], [1, N, H, W, 1] or [H, W], "
                         f"got {tuple(torch.as_tensor(x).shape)}")
    if t.shape[0] > MAX_VIEWS:
        raise ValueError(f"{name} has {t.shape[0]} views, at most {MAX_VIEWS}")
    return t


def _groups_of(scope, n_views: int):
    """(int32 group vector or None, n_groups) of ``scope``: "view", "scene" or one group index per view."""
    if isinstance(scope, str):
        if scope == "view":
            return None, n_views
        if scope == "scene":
            return torch.zeros(n_views, dtype=torch.int32), 1
        raise ValueError(f"scope must be 'view', 'scene' or a group index per view, got {scope!r}")
    g = _as_tensor(scope, "scope")
    if g.dim() != 1 or g.numel() != n_views or g.is_floating_point():
        raise ValueError(f"scope must hold one integer group index per view ({n_views}), got {tuple(g.shape)} {g.dtype}")
    g = g.to("cpu", torch.int64)
    ng = int(g.max()) + 1
    if int(g.min()) < 0 or ng > n_views or len(torch.unique(g)) != ng:
        raise ValueError("group indices must cover 0 .. n_groups - 1 without gaps")
    return g.to(torch.int32), ng


def select_quantiles(x, fractions: Sequence, mask=None, group=None, return_counts: bool = False):
    """``value`` [n_groups, len(fractions)] fp32 on the device: the exact order statistics of the finite
    elements of each group of rows of ``x`` [rows, ...] (``mask``: bool or uint8 of the same shape,
    false = skip; ``group``: one group index per row, default every row its own group).  A fraction is a
    quantile in [0, 1] or a (num, den) pair and selects the ascending element max(ceil(num n / den) - 1, 0):
    1 / 2 the lower median.  An empty group gives NaN.  With ``return_counts`` also ``count``
    [n_groups, 2] int32: considered, skipped."""
    ranks = [rank_fraction(q) for q in fractions]
    if not 1 <= len(ranks) <= 4:
        raise ValueError(f"1 to 4 fractions are selected at once, got {len(ranks)}")
    t = _as_tensor(x, "x")
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError(f"x must be a non-empty [rows, ...] tensor, got {tuple(t.shape)}")
    m = None
    if mask is not None:
        m = _as_tensor(mask, "mask")
        if tuple(m.shape) != tuple(t.shape) or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be bool or uint8 {tuple(t.shape)}, got {m.dtype} {tuple(m.shape)}")
    n_rows = t.shape[0]
    g, ng = (None, n_rows) if group is None else _groups_of(group, n_rows)
    dev = _device_of(x, mask)
    t = t.to(device=dev, dtype=torch.float32).reshape(n_rows, -1).contiguous()
    if m is not None:
        m = m.to(device=dev, dtype=torch.uint8).reshape(n_rows, -1).contiguous()
    if g is not None:
        g = g.to(dev)
    value = torch.empty(ng, len(ranks), device=dev, dtype=torch.float32)
    count = torch.empty(ng, 2, device=dev, dtype=torch.int32) if return_counts else None
    ops.select_ranks(t, ranks, value, mask=m, group=g, n_groups=ng, count=count)
    return (value, count) if return_counts else value


def metrics_from_stats(stats, hist, thresholds: Sequence[float], bin_len: float) -> dict:
    """The metrics of one row of sr_depth_eval's ``stats`` [16] and ``hist`` [n_bins + 2].  Host only.
    abs_rel = sum rel / n, sq_rel = sum (a - g)^2 / g / n, rmse = sqrt(sum (a - g)^2 / n) over the n valid
    pixels; rmse_log = sqrt(mean d^2), silog = 100 sqrt(mean d^2 - (mean d)^2), log10 = mean |d| / ln 10
    over the n - n_nonpos pixels with a > 0; delta_k and inlier@t = fraction of ALL valid pixels (a pixel
    with a <= 0 fails every delta; inlier@t counts fl32(rel) below t, read off the histogram, so t must be
    a positive multiple of ``bin_len`` inside it).  NaN where the denominator is zero."""
    s = np.asarray(stats, dtype=np.float64)
    h = np.asarray(hist).astype(np.int64) & 0xFFFFFFFF  # uint32 counts, whatever the storage
    if s.shape != (N_STATS,) or h.ndim != 1 or h.shape[0] < 3:
        raise ValueError(f"stats must be [{N_STATS}] and hist [n_bins + 2], got {s.shape} and {h.shape}")
    n_bins = h.shape[0] - 2
    _check_bins(bin_len, n_bins)
    ks = _threshold_bins(thresholds, bin_len, n_bins)
    n, n_nonpos, n_invalid = int(s[0]), int(s[1]), int(s[2])
    if int(h.sum()) != n:
        raise ValueError(f"hist counts {int(h.sum())} pixels, stats {n}")
    n_log = n - n_nonpos
    nan = float("nan")
    out = {"abs_rel": s[3] / n if n else nan, "sq_rel": s[4] / n if n else nan,
           "rmse": float(np.sqrt(s[5] / n)) if n else nan}
    if n_log:
        md, md2 = s[6] / n_log, s[7] / n_log
        out.update(rmse_log=float(np.sqrt(md2)), silog=100.0 * float(np.sqrt(max(md2 - md * md, 0.0))), log10=s[8] / n_log)
    else:
        out.update(rmse_log=nan, silog=nan, log10=nan)
    for k in range(3):
        out[f"delta{k + 1}"] = s[9 + k] / n if n else nan
    cum = np.cumsum(h[:n_bins])  # cum[k - 1] = pixels below k * bin_len
    for tau, k in zip(thresholds, ks):
        out[f"inlier@{_fmt(tau)}"] = float(cum[k - 1]) / n if n else nan
    out.update(rel_max=float(s[12]) if n else nan, n_valid=n, n_nonpos=n_nonpos, n_invalid=n_invalid)
    return {k: (float(v) if isinstance(v, np.floating) else v) for k, v in out.items()}


def depth_accuracy(pred, gt, valid=None, conf=None, conf_quantile: Optional[float] = None, align: str = "median",
                   scope="view", thresholds: Sequence[float] = (0.05, 0.1, 0.25), bin_len: float = 0.005,
                   n_bins: int = 1024, xform=None, gt_min: float = 0.0, gt_max: float = float("inf")) -> dict:
    """Scores ``pred`` against ``gt`` ([N, H, W], [N, 1, H, W], [N, H, W, 1] or [H, W] tensors or arrays;
    host inputs are uploaded).  A pixel is valid where ``valid`` (bool, optional) holds, ``gt`` is finite
    with gt_min < gt <= gt_max, ``pred`` is finite and, with ``conf`` and ``conf_quantile`` = q, ``conf`` is
    at least the view's exact q-quantile (the most confident 1 - q of each view; the quantile never
    leaves the device).  ``align``: "none", "median", "scale", "scale_shift", or "given" with ``xform``
    [n_groups, 2] = (s, t), host or device (e.g. built from sr_pose_align's scale).  ``scope``: "view" (a
    group per view), "scene" (one group) or one group index per view.

    Returns a dict of arrays [n_groups], one entry per group: abs_rel, sq_rel, rmse, rmse_log, silog,
    log10, delta1..3, inlier@t per threshold, rel_median, rel_p90, rel_max, n_valid, n_nonpos, n_invalid,
    scale, shift, status (bit 0: degenerate fit, s = 1; bit 1: no valid pixel); ``pooled``: the same over
    all groups, each under its own alignment; ``hist`` [n_groups + 1, n_bins + 2].  Everything is derived
    from the device's sums, counts, histogram and selects in one D2H copy."""
    _check_bins(bin_len, n_bins)
    _threshold_bins(thresholds, bin_len, n_bins)
    if align not in ops.DEPTH_ALIGN:
        raise ValueError(f"align must be one of {sorted(ops.DEPTH_ALIGN)}, got {align!r}")
    if (align == "given") != (xform is not None):
        raise ValueError("xform goes with align='given'")
    if (conf is None) != (conf_quantile is None):
        raise ValueError("conf and conf_quantile go together")
    p, g = _as_maps(pred, "pred"), _as_maps(gt, "gt")
    if p.shape != g.shape:
        raise ValueError(f"pred is {tuple(p.shape)}, gt is {tuple(g.shape)}: resize before scoring")
    nv, n_pix = p.shape[0], p.shape[1] * p.shape[2]
    m = c = None
    if valid is not None:
        m = _as_maps(valid, "valid")
        if m.shape != p.shape or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid must be bool {tuple(p.shape)}, got {m.dtype} {tuple(m.shape)}")
    if conf is not None:
        c = _as_maps(conf, "conf")
        if c.shape != p.shape:
            raise ValueError(f"conf is {tuple(c.shape)}, pred is {tuple(p.shape)}")
        rank = rank_fraction(conf_quantile)
    grp, ng = _groups_of(scope, nv)
    dev = _device_of(pred, gt, valid, conf, xform)
    flat = lambda t, dt: t.to(device=dev, dtype=dt).reshape(nv, n_pix).contiguous()  # noqa: E731
    p, g = flat(p, torch.float32), flat(g, torch.float32)
    m = None if m is None else flat(m, torch.uint8)
    conf_min = None
    if c is not None:
        c = flat(c, torch.float32)
        conf_min = torch.empty(nv, 1, device=dev, dtype=torch.float32)
        ops.select_ranks(c, [rank], conf_min)
    grp = None if grp is None else grp.to(dev)
    if xform is not None:
        xf = _as_tensor(xform, "xform")
        if xf.numel() != 2 * ng:
            raise ValueError(f"xform must be [{ng}, 2] (s, t per group), got {tuple(xf.shape)}")
        xf = xf.to(device=dev, dtype=torch.float64).reshape(ng, 2).contiguous()
    else:
        xf = torch.empty(ng, 2, device=dev, dtype=torch.float64)
    status = torch.empty(ng, device=dev, dtype=torch.int32)
    stats = torch.empty(ng + 1, N_STATS, device=dev, dtype=torch.float64)
    hist = torch.empty(ng + 1, n_bins + 2, device=dev, dtype=torch.int32)
    rel_q = torch.empty(ng + 1, 2, device=dev, dtype=torch.float32)
    ops.depth_eval(p, g, align=align, xform=xf, status=status, stats=stats, hist=hist, bin_len=float(bin_len), mask=m,
                   conf=c, conf_min=conf_min, group=grp, n_groups=ng, gt_min=gt_min, gt_max=gt_max, rel_q=rel_q)
    # the call's one D2H copy: counts and fp32 values are exact in fp64
    host = torch.cat([stats.reshape(-1), (hist.to(torch.int64) & 0xFFFFFFFF).reshape(-1).to(torch.float64),
                      rel_q.reshape(-1).to(torch.float64), xf.reshape(-1), status.to(torch.float64)]).cpu().numpy()
    cut = np.cumsum([stats.numel(), hist.numel(), rel_q.numel(), xf.numel()])
    s, h, rq, x, st = np.split(host, cut)
    s, h, rq, x = s.reshape(ng + 1, N_STATS), h.astype(np.int64).reshape(ng + 1, n_bins + 2), rq.reshape(ng + 1, 2), x.reshape(ng, 2)
    rows = []
    for k in range(ng + 1):
        r = metrics_from_stats(s[k], h[k], tuple(thresholds), float(bin_len))
        r.update(rel_median=float(rq[k, 0]), rel_p90=float(rq[k, 1]))
        rows.append(r)
    out = {key: np.array([r[key] for r in rows[:ng]]) for key in rows[0]}
    out.update(scale=x[:, 0].copy(), shift=x[:, 1].copy(), status=st.astype(np.int64), pooled=rows[ng], hist=h,
               n_groups=ng)
    return out


def evaluate_depth(predictions, gt_depth, valid=None, conf_quantile: Optional[float] = None, key: str = "depth_map",
                   conf_key: str = "dpt_cnf", **kw) -> dict:
    """depth_accuracy of the depth maps of ``predictions`` -- one dict or the list of result dicts
    SailRecon.forward / reloc(save_depth=True) return, each with ``key`` [1, S, H, W, 1] (or [S, H, W],
    [H, W, 1], ...) -- against ``gt_depth`` [N, 1, H, W] / [N, H, W] (``depth_pr_processed``), N the total
    number of views.  With ``conf_quantile`` the maps of ``conf_key`` gate the pixels.  Further keyword
    arguments are depth_accuracy's."""
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

    pred = gather(key)
    conf = gather(conf_key) if conf_quantile is not None else None
    return depth_accuracy(pred, gt_depth, valid=valid, conf=conf, conf_quantile=conf_quantile, **kw)
