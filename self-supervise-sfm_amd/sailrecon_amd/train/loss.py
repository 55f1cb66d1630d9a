"""Self-supervised training loss on the HIP path — mirror of compute_loss
(train/train_imc.py:141-246) and CDFLossIndexPytorch (train/losses/cdf_loss.py:19-242).

``CDFLossIndexPytorch`` keeps the reference constructor (min_val, max_val, num_bins, src_indices,
dst_indices, gradient_smooth, num_nodes) and its smoothing taps (cdf_loss.py:62-84); the
histogram / CDF / PDF / lookup run inside sr_imc_loss together with the geometry, and the
gradient the reference's CDFLossTorchWrapper supplies (pdf * weight) is chained down to the pose
encodings in the same call.  ``compute_loss`` returns the reference's {"loss": ...} plus the
gradient with respect to the query views' pose encodings ("d_pose_enc"), which TrainGraph.backward
consumes (the role of ``scaler.scale(loss).backward()``, train_imc.py:404).

``residual_stats`` / ``summarize`` report the residuals the loss bins, in pixels, per pair
(sr_imc_residual_stats): the readable number the reference gets from sanity_check_relative_poses
(train_imc.py:371), and the frame CDFs / PDFs ``compute_loss(do_record=True)`` returns as the
reference's "plot_data" (train_imc.py:257-266).
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib, ops

Tensor = torch.Tensor


class CDFLossIndexPytorch:
    def __init__(self, min_val: float, max_val: float, num_bins: int, src_indices: Tensor, dst_indices: Tensor,
                 gradient_smooth: float = 0.0001, num_nodes: Optional[int] = None):
        self.min_val, self.max_val, self.num_bins = float(min_val), float(max_val), int(num_bins)
        self.gradient_smooth = gradient_smooth
        self.src_indices = torch.as_tensor(src_indices).long()
        self.dst_indices = torch.as_tensor(dst_indices).long()
        if num_nodes is None:
            num_nodes = int(torch.cat([self.src_indices, self.dst_indices]).max()) + 1
        self.num_nodes = num_nodes
        bw = (self.max_val - self.min_val) / self.num_bins
        if gradient_smooth > 0:  # cdf_loss.py:62-84 (same fp32 ops -> same taps)
            r = max(1, int(gradient_smooth / bw))
            idx = torch.arange(2 * r + 1, dtype=torch.float32) - r
            g = torch.exp(-0.5 * (idx / (gradient_smooth / bw)) ** 2)
            self.smooth = g / torch.sum(g)
        else:
            self.smooth = torch.ones(1)
        self._dev = {}

    def to(self, device):
        return self

    def device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = dict(smooth=self.smooth.to(device).contiguous(),
                                  src=self.src_indices.int().to(device), dst=self.dst_indices.int().to(device))
        return self._dev[key]


def _fill_desc(pose_enc: Tensor, hw: Tuple[int, int], K_prime_to_K: Tensor, shared_focal: bool, src_idx: Tensor,
               dst_idx: Tensor, src_coords: Tensor, dst_coords: Tensor, src_depth: Tensor, dst_depth: Tensor,
               cdf: CDFLossIndexPytorch):
    """The geometry / CDF half of sr_imc_loss_desc shared by imc_loss and residual_stats:
    (desc, enc [N, 9], tensors the desc points into)."""
    dev = pose_enc.device
    enc = pose_enc.reshape(-1, 9).float().contiguous()
    n = enc.shape[0]
    P, K = src_coords.shape[0], src_coords.shape[1]
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    i = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    tabs = cdf.device_tables(dev)
    if tabs["src"].numel() < P or tabs["dst"].numel() < P:
        raise IndexError(f"CDFLossIndexPytorch built on {tabs['src'].numel()} / {tabs['dst'].numel()} src / dst "
                         f"indices cannot index {P} pairs (cdf_loss.py:147-148)")
    node_src, node_dst = tabs["src"], tabs["dst"]
    kp, sc, dc, sd, dd = f(K_prime_to_K), f(src_coords), f(dst_coords), f(src_depth), f(dst_depth)
    si, di = i(src_idx), i(dst_idx)
    d = _lib.ImcLossDesc()
    d.enc, d.n_views, d.H, d.W = ops._p(enc), n, int(hw[0]), int(hw[1])
    d.kp2k, d.shared_focal = ops._p(kp), int(bool(shared_focal))
    d.n_pairs, d.n_points = P, K
    d.src_idx, d.dst_idx = ops._p(si), ops._p(di)
    d.src_coords, d.dst_coords, d.src_depth, d.dst_depth = ops._p(sc), ops._p(dc), ops._p(sd), ops._p(dd)
    d.node_src, d.node_dst = ops._p(node_src), ops._p(node_dst)
    d.n_nodes = cdf.num_nodes
    d.min_val, d.max_val, d.num_bins = cdf.min_val, cdf.max_val, cdf.num_bins
    d.smooth_w, d.smooth_radius = ops._p(tabs["smooth"]), tabs["smooth"].numel() // 2
    return d, enc, (kp, sc, dc, sd, dd, si, di, node_src, node_dst, tabs["smooth"])


def imc_loss(pose_enc: Tensor, hw: Tuple[int, int], K_prime_to_K: Tensor, shared_focal: bool, src_idx: Tensor,
             dst_idx: Tensor, src_coords: Tensor, dst_coords: Tensor, src_depth: Tensor, dst_depth: Tensor,
             cdf: CDFLossIndexPytorch, grad_scale: float = 1.0, loss_out: Optional[Tensor] = None,
             d_enc_out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(loss [1], d loss / d pose_enc [N, 9] * grad_scale) for pose encodings [N, 9] (device fp32)."""
    d, enc, keep = _fill_desc(pose_enc, hw, K_prime_to_K, shared_focal, src_idx, dst_idx, src_coords, dst_coords,
                              src_depth, dst_depth, cdf)
    dev, n = enc.device, enc.shape[0]
    loss = loss_out if loss_out is not None else torch.empty(1, device=dev, dtype=torch.float32)
    d_enc = d_enc_out if d_enc_out is not None else torch.empty(n, 9, device=dev, dtype=torch.float32)
    L = _lib.load()
    ws_n = L.sr_imc_loss_workspace(n, d.n_pairs, d.n_points, cdf.num_nodes, cdf.num_bins)
    ws = ops._train_ws(dev, "imc_loss", ws_n)
    d.grad_scale = float(grad_scale)
    d.loss, d.d_enc, d.workspace = ops._p(loss), ops._p(d_enc), ops._p(ws)
    _lib.check(L.sr_imc_loss(ops._stream(enc), ctypes.byref(d)), "sr_imc_loss")
    del keep
    return loss, d_enc


RESIDUAL_VARIANTS = ("reproj", "reproj_fixed_depth", "sampson")
_THRESH_DEV = {}


def stats_words(n_pairs: int, n_thresh: int) -> int:
    """fp32 words of residual_stats' pair_stats + pair_counts block (one D2H copy for summarize)."""
    return 3 * n_pairs * (4 + 2 + n_thresh)


def residual_stats(pose_enc: Tensor, hw: Tuple[int, int], K_prime_to_K: Tensor, shared_focal: bool, src_idx: Tensor,
                   dst_idx: Tensor, src_coords: Tensor, dst_coords: Tensor, src_depth: Tensor, dst_depth: Tensor,
                   cdf: CDFLossIndexPytorch, thresholds=(1., 2., 4., 8.), residuals: bool = False,
                   pairs_out: Optional[Tensor] = None) -> dict:
    """sr_imc_residual_stats on imc_loss's arguments: the residuals the loss bins, in pixels (exact
    reprojection, fixed depth, Sampson), summarised per pair, and the per-frame arrays the loss looks
    its values up in (CDFLossIndexPytorch.get_frame_statistics, cdf_loss.py:245-259).  Device tensors:
      frame_pmf / frame_cdf / frame_pdf [2, num_nodes, num_bins]   (variants 0, 1)
      pair_stats  [3, P, 4] fp32   mean, median, p90, max over the finite points (NaN if none)
      pair_counts [3, P, 2 + len(thresholds)] int32   n_finite, n_behind, points with r < threshold
      residuals   [3, P, K] fp32   with residuals=True
    plus "thresholds" and "n_points".  pair_stats and pair_counts are views of one flat buffer
    ("_pairs"; ``pairs_out`` supplies it, >= stats_words(P, len(thresholds)) fp32), so summarize
    reads them back in one copy."""
    d, enc, keep = _fill_desc(pose_enc, hw, K_prime_to_K, shared_focal, src_idx, dst_idx, src_coords, dst_coords,
                              src_depth, dst_depth, cdf)
    dev, n, P, K = enc.device, enc.shape[0], d.n_pairs, d.n_points
    thresholds = tuple(float(t) for t in thresholds)
    nt = len(thresholds)
    nn, nb = cdf.num_nodes, cdf.num_bins
    words = stats_words(P, nt)
    if pairs_out is None:
        pairs_out = torch.empty(words, device=dev, dtype=torch.float32)
    elif pairs_out.numel() < words or pairs_out.dtype != torch.float32 or not pairs_out.is_contiguous():
        raise ValueError(f"pairs_out must be contiguous fp32 with >= {words} elements")
    pair_stats = pairs_out[:3 * P * 4].view(3, P, 4)
    pair_counts = pairs_out[3 * P * 4:words].view(torch.int32).view(3, P, 2 + nt)
    frames = torch.empty(3, 2, nn, nb, device=dev, dtype=torch.float32)
    out = {"frame_pmf": frames[0], "frame_cdf": frames[1], "frame_pdf": frames[2], "pair_stats": pair_stats,
           "pair_counts": pair_counts, "thresholds": thresholds, "n_points": K, "_pairs": pairs_out[:words]}
    # uploaded once per (device, thresholds): a host tensor's copy would block the host until the stream reaches it
    key = (str(dev), thresholds)
    if nt and key not in _THRESH_DEV:
        _THRESH_DEV[key] = torch.tensor(thresholds, dtype=torch.float32).to(dev)
    th = _THRESH_DEV[key] if nt else None
    L = _lib.load()
    ws_n = L.sr_imc_stats_workspace(n, P, K, nn, nb)
    ws = ops._train_ws(dev, "imc_residual_stats", ws_n)
    s = _lib.ImcStatsDesc()
    if residuals:
        out["residuals"] = torch.empty(3, P, K, device=dev, dtype=torch.float32)
        s.residuals = ops._p(out["residuals"])
    s.frame_pmf, s.frame_cdf, s.frame_pdf = ops._p(frames[0]), ops._p(frames[1]), ops._p(frames[2])
    s.thresh, s.n_thresh = ops._p(th), nt
    s.pair_counts, s.pair_stats = ops._p(pair_counts), ops._p(pair_stats)
    s.workspace, s.workspace_floats = ops._p(ws), ws.numel()
    _lib.check(L.sr_imc_residual_stats(ops._stream(enc), ctypes.byref(d), ctypes.byref(s)), "sr_imc_residual_stats")
    del keep
    return out


def summarize(stats: dict, host_pairs=None) -> dict:
    """Host summary of residual_stats' per-pair block (one D2H copy; ``host_pairs`` = that block
    already on the host).  Per variant of RESIDUAL_VARIANTS:
      median_px   median over the pairs of the per-pair medians, NaN pairs ignored
      inlier@t    sum of the counts below threshold t / sum of n_finite
      behind      sum of n_behind / sum of n_finite
      nonfinite   share of the points whose residual is not finite"""
    th, K = tuple(stats["thresholds"]), int(stats["n_points"])
    if host_pairs is None and "_pairs" in stats:
        host_pairs = stats["_pairs"].cpu().numpy()
    if host_pairs is not None:
        flat = np.asarray(host_pairs)
        P = flat.size // (3 * (6 + len(th)))
        ps = flat[:3 * P * 4].reshape(3, P, 4)
        pc = flat[3 * P * 4:3 * P * (6 + len(th))].view(np.int32).reshape(3, P, 2 + len(th))
    else:
        ps = np.asarray(stats["pair_stats"].cpu() if torch.is_tensor(stats["pair_stats"]) else stats["pair_stats"])
        pc = np.asarray(stats["pair_counts"].cpu() if torch.is_tensor(stats["pair_counts"]) else stats["pair_counts"])
    pc = pc.astype(np.int64)
    out = {}
    for v, name in enumerate(RESIDUAL_VARIANTS):
        med = ps[v, :, 1].astype(np.float64)
        med = med[~np.isnan(med)]
        n_fin = int(pc[v, :, 0].sum())
        r = {"median_px": float(np.median(med)) if med.size else float("nan")}
        for t, tau in enumerate(th):
            r[f"inlier@{tau:g}"] = float(pc[v, :, 2 + t].sum()) / n_fin if n_fin else float("nan")
        r["behind"] = float(pc[v, :, 1].sum()) / n_fin if n_fin else float("nan")
        r["nonfinite"] = 1.0 - n_fin / float(pc.shape[1] * K)
        out[name] = r
    return out


def plot_data(stats: dict, cdf: CDFLossIndexPytorch, summary: Optional[dict] = None) -> dict:
    """compute_loss's "plot_data" (train_imc.py:257-266; the exact-reprojection variant) from
    residual_stats' output, plus "residual_stats" (summarize)."""
    return {"frame_cdfs": stats["frame_cdf"][0].cpu().numpy(), "frame_pdfs": stats["frame_pdf"][0].cpu().numpy(),
            "max_val": cdf.max_val, "min_val": cdf.min_val, "num_bins": cdf.num_bins,
            "residual_stats": summary if summary is not None else summarize(stats)}


def compute_loss(predictions, batch, device, cdf_loss_module: CDFLossIndexPytorch, do_record: bool = False,
                 image_hw: Tuple[int, int] = (518, 518), grad_scale: float = 1.0) -> dict:
    """train_imc.py:141-246 on the HIP path.  ``predictions``: a list of per-view dicts with
    "pose_enc" ([1, 9] or [9]) like the reference's, or one dict / tensor holding the query
    views' [1, N, 9] pose encoding.  Returns {"loss": [1] tensor, "d_pose_enc": [N, 9]} and, with
    ``do_record``, the reference's "plot_data" (train_imc.py:257-266) from residual_stats."""
    if isinstance(predictions, Tensor):
        enc = predictions
    elif isinstance(predictions, dict):
        enc = predictions["pose_enc"]
    else:
        enc = torch.cat([p["pose_enc"].reshape(-1, 9) for p in predictions], 0)
    loss, d_enc = imc_loss(enc.to(device), image_hw, batch["K_prime_to_K"], bool(batch["shared_focal"]),
                           batch["src_idx"], batch["dst_idx"], batch["src_coords"], batch["dst_coords"],
                           batch["src_depth"], batch["dst_depth"], cdf_loss_module, grad_scale=grad_scale)
    result = {"loss": loss, "d_pose_enc": d_enc}
    if do_record:
        stats = residual_stats(enc.to(device), image_hw, batch["K_prime_to_K"], bool(batch["shared_focal"]),
                               batch["src_idx"], batch["dst_idx"], batch["src_coords"], batch["dst_coords"],
                               batch["src_depth"], batch["dst_depth"], cdf_loss_module)
        result["plot_data"] = plot_data(stats, cdf_loss_module)
    return result
