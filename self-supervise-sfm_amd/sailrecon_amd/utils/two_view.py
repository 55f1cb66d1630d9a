"""Two-view geometry on the device (sr_two_view; definitions: DESIGN.md "Two-view geometry").

    estimate_two_view   correspondences and intrinsics in; per pair the essential matrix the correspondences
                        imply, its inliers and the relative pose (R, t) by cheirality.  No ground truth is read.
    verify_poses        a training batch's pairs: how far the predicted relative poses are from the two-view
                        estimates, and the inlier ratio that says how much each estimate is worth

There is no torch fallback: the library does the work or the call raises.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .pose_eval import accuracy_from_hist

Tensor = torch.Tensor


def _device_of(*xs):
    for x in xs:
        if isinstance(x, Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda")


def _as(x, name: str, dev, dtype, shape_tail=None):
    if x is None:
        return None
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()
    t = torch.as_tensor(x)
    if shape_tail is not None and tuple(t.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise ValueError(f"{name} must end in {tuple(shape_tail)}, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=dtype).contiguous()


def _extrinsic(x, name: str, dev, n_views=None):
    if x is None:
        return None
    t = torch.as_tensor(x)
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or tuple(t.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"{name} must be [V, 3, 4] or [V, 4, 4], got {tuple(t.shape)}")
    if n_views is not None and t.shape[0] != n_views:
        raise ValueError(f"{name} has {t.shape[0]} views, the intrinsics {n_views}")
    return t[:, :3, :].to(device=dev, dtype=torch.float32).contiguous()


def essential_from_extrinsic(extrinsic: Tensor, src_idx: Tensor, dst_idx: Tensor) -> Tensor:
    """[P, 9] fp64 E = [t]x R of the relative poses T = E_d E_s^-1, t scaled to length 1 (zeros for a zero
    baseline or a pair of equal views)."""
    e = extrinsic.to(torch.float64)
    s, d = src_idx.long(), dst_idx.long()
    R = e[d, :, :3] @ e[s, :, :3].transpose(1, 2)
    t = e[d, :, 3] - (R @ e[s, :, 3, None])[..., 0]
    n = t.norm(dim=1, keepdim=True)
    t = torch.where(n > 0, t / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(t))
    z = torch.zeros_like(t[:, 0])
    tx = torch.stack([z, -t[:, 2], t[:, 1], t[:, 2], z, -t[:, 0], -t[:, 1], t[:, 0], z], dim=1).reshape(-1, 3, 3)
    return (tx @ R).reshape(-1, 9).contiguous()


def estimate_two_view(src_coords, dst_coords, intrinsic, src_idx, dst_idx, *, valid=None, threshold_px: float = 2.0,
                      hypotheses: int = 1024, refine_iters: int = 8, seed: int = 0, init_extrinsic=None,
                      ref_extrinsic=None, return_hypotheses: bool = False) -> dict:
    """The relative pose that the correspondences of every pair imply.  ``src_coords`` / ``dst_coords`` [P, K, 2]
    pixels of the views ``src_idx`` / ``dst_idx`` [P] with ``intrinsic`` [V, 3, 3] (zero skew); tensors or arrays
    (host inputs are uploaded).  ``valid`` [P, K] bool; ``threshold_px`` the inlier threshold on the pixel Sampson
    distance; ``hypotheses`` 8-point models are drawn per pair; ``init_extrinsic`` [V, 3, 4] adds the given poses'
    own model E = [t]x R per pair, scored ahead of the drawn ones, so the result's cost is never above that
    pose's; ``ref_extrinsic`` [V, 3, 4] adds ``pose_err``.

    Returns device tensors: ``E`` [P, 3, 3], ``R`` [P, 3, 3] and unit ``t`` [P, 3] (X_dst = R X_src + t) fp64,
    ``cost`` [P] fp64, ``n_inliers`` / ``n_front`` [P] int32, ``best`` / ``refined`` /
    ``status`` [P] int32 (status 0 a result, 1 fewer than 8 valid correspondences, 2 no finite model, 3 equal or
    unknown views), ``inlier_mask`` [P, K] bool, ``pose_err`` [P, 2] degrees (rotation, translation direction; only
    with ``ref_extrinsic``), ``init_cost`` [P] (only with ``init_extrinsic``: the given pose's cost), and with
    ``return_hypotheses`` ``hyp_idx`` [P, H, 8], ``hyp_E`` [P, G + H, 3, 3], ``hyp_cost`` and ``hyp_inliers``
    [P, G + H]."""
    dev = _device_of(src_coords, dst_coords, intrinsic, valid, init_extrinsic, ref_extrinsic)
    sc = _as(src_coords, "src_coords", dev, torch.float32, (2,))
    dc = _as(dst_coords, "dst_coords", dev, torch.float32, (2,))
    if sc.dim() == 2:
        sc, dc = sc[None], dc[None]
    if sc.dim() != 3 or sc.shape != dc.shape or sc.numel() == 0:
        raise ValueError(f"src_coords and dst_coords must both be [P, K, 2], got {tuple(sc.shape)} and {tuple(dc.shape)}")
    P, K = sc.shape[:2]
    k = _as(intrinsic, "intrinsic", dev, torch.float32, (3, 3))
    if k.dim() != 3:
        raise ValueError(f"intrinsic must be [V, 3, 3], got {tuple(k.shape)}")
    V = k.shape[0]
    si = _as(src_idx, "src_idx", dev, torch.int32).reshape(-1)
    di = _as(dst_idx, "dst_idx", dev, torch.int32).reshape(-1)
    if si.numel() != P or di.numel() != P:
        raise ValueError(f"src_idx and dst_idx must have one entry per pair ({P})")
    m = None
    if valid is not None:
        m = torch.as_tensor(valid)
        if m.dtype not in (torch.bool, torch.uint8) or m.numel() != P * K:
            raise ValueError(f"valid must be [P, K] bool or uint8, got {m.dtype} {tuple(m.shape)}")
        m = m.to(device=dev, dtype=torch.uint8).reshape(P, K).contiguous()
    init = _extrinsic(init_extrinsic, "init_extrinsic", dev, V)
    ref = _extrinsic(ref_extrinsic, "ref_extrinsic", dev, V)
    given = None
    if init is not None:
        ok = (si >= 0) & (si < V) & (di >= 0) & (di < V)
        zero = torch.zeros_like(si)
        given = essential_from_extrinsic(init, torch.where(ok, si, zero), torch.where(ok, di, zero)).reshape(P, 1, 9)
    G, H = 0 if given is None else 1, int(hypotheses)
    f64, i32 = torch.float64, torch.int32
    new = lambda *shape, dt=f64: torch.empty(*shape, device=dev, dtype=dt)  # noqa: E731
    o = dict(E=new(P, 9), R=new(P, 9), t=new(P, 3), cost=new(P), n_inliers=new(P, dt=i32), n_front=new(P, dt=i32),
             best=new(P, dt=i32), refined=new(P, dt=i32), status=new(P, dt=i32), inlier_mask=new(P, K, dt=torch.uint8))
    if ref is not None:
        o["pose_err"] = new(P, 2)
    if return_hypotheses or G:
        o["hyp_cost"] = new(P, G + H)
    if return_hypotheses:
        o["hyp_E"], o["hyp_inliers"] = new(P, G + H, 9), new(P, G + H, dt=i32)
        if H:
            o["hyp_idx"] = new(P, H, 8, dt=i32)
    ops.two_view(sc, dc, k, si, di, mask=m, given_E=given, ref_extrinsic=ref, n_hyp=H, threshold_px=float(threshold_px),
                 refine_iters=int(refine_iters), seed=int(seed), **o)
    o["E"], o["R"] = o["E"].reshape(P, 3, 3), o["R"].reshape(P, 3, 3)
    o["inlier_mask"] = o["inlier_mask"].bool()
    if G:
        o["init_cost"] = o["hyp_cost"][:, 0].clone()
        if not return_hypotheses:
            del o["hyp_cost"]
    if return_hypotheses:
        o["hyp_E"] = o["hyp_E"].reshape(P, G + H, 3, 3)
    return o


def _predicted_cameras(predictions):
    if isinstance(predictions, dict):
        return predictions["extrinsic"], predictions["intrinsic"]
    if isinstance(predictions, (list, tuple)) and len(predictions) == 2 and not isinstance(predictions[0], dict):
        return predictions
    if isinstance(predictions, (list, tuple)) and predictions and isinstance(predictions[0], dict):
        e = torch.stack([torch.as_tensor(v["extrinsic"]).reshape(-1, 4)[:3] for v in predictions])
        k = torch.stack([torch.as_tensor(v["intrinsic"]).reshape(3, 3).to(e.device) for v in predictions])
        return e, k
    raise ValueError("predictions must be (extrinsic, intrinsic), a dict with those keys or a list of per-view dicts")


def verify_poses(predictions, batch: dict, *, thresholds=(5, 15, 30), **kw) -> dict:
    """Predicted relative poses against the two-view estimates of a training batch's pairs (the keys of
    train.data.correspondence_batch / synthetic_batch: src_idx, dst_idx, src_coords, dst_coords; K_prime_to_K
    [V, 3, 3], when present, maps the predicted intrinsics K' to the pixels of the correspondences, K = K_prime_to_K
    K').  ``predictions``: (extrinsic [V, 3, 4], intrinsic [V, 3, 3]), a dict with those keys, or the list of per-view
    result dicts.  ``kw`` goes to estimate_two_view.

    Returns ``rot_err`` / ``trans_err`` [P] fp64 degrees on the device (NaN for a pair without an estimate),
    ``inlier_ratio`` [P] (inliers over correspondences), ``status`` [P], the estimate itself under ``estimate``, and
    on the host ``n_pairs``, ``n_estimated``, ``rra@t`` / ``rta@t`` / ``auc@t`` for t in ``thresholds`` (fractions
    of all pairs, pose_eval.accuracy_from_hist) and ``hist``."""
    ext, intr = _predicted_cameras(predictions)
    dev = _device_of(ext, intr, batch.get("src_coords"), batch.get("dst_coords"))
    ext = _extrinsic(ext, "extrinsic", dev)
    k = _as(intr, "intrinsic", dev, torch.float32, (3, 3)).reshape(-1, 3, 3)
    if "K_prime_to_K" in batch and batch["K_prime_to_K"] is not None:
        kp = _as(batch["K_prime_to_K"], "K_prime_to_K", dev, torch.float32, (3, 3)).reshape(-1, 3, 3)
        k = (kp.double() @ k.double()).float()
    est = estimate_two_view(batch["src_coords"], batch["dst_coords"], k, batch["src_idx"], batch["dst_idx"],
                            ref_extrinsic=ext, **kw)
    err = est["pose_err"]
    K = est["inlier_mask"].shape[1]
    n_bins = 180
    # the histogram of pose_eval: rows rot / trans / max, slot n_bins the rest, slot n_bins + 1 the non-finite pairs
    rows = torch.stack([err[:, 0], err[:, 1], torch.maximum(err[:, 0], err[:, 1])])
    finite = torch.isfinite(rows).all(dim=0)
    slot = torch.where(finite[None], rows.clamp(0, n_bins).floor(), torch.full_like(rows, n_bins + 1)).long()
    hist = torch.zeros(3, n_bins + 2, dtype=torch.int64, device=dev)
    hist.scatter_add_(1, slot, torch.ones_like(slot))
    out = accuracy_from_hist(hist.cpu().numpy(), thresholds, 1.0)
    out.update(rot_err=err[:, 0], trans_err=err[:, 1], inlier_ratio=est["n_inliers"].double() / K, status=est["status"],
               estimate=est, n_estimated=int((est["status"] == 0).sum()))
    return out
