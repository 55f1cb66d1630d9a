"""Synthetic IMC2021-shaped training batches (the dataset and its HDF5 reader are absent here:
datasets/imc2021.py:260-301 + collate_fn).  A batch holds, like the reference's:
  rgb_processed [N, 3, S, S] in [0, 1], K_prime_to_K [N, 3, 3], shared_focal,
  src_idx / dst_idx [P], src_coords / dst_coords [P, K, 2], src_depth / dst_depth [P, K]
Pairs default to the chain (0,1), (1,2), ...; correspondences are random pixels displaced by a
few pixels with positive depths, so residuals land inside the CDF's [0, 15) log range."""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch


def synthetic_batch(n_views: int, n_points: int = 1024, size: int = 518, seed: int = 0,
                    pairs: Optional[List[Tuple[int, int]]] = None, shared_focal: bool = False) -> dict:
    g = torch.Generator().manual_seed(seed)
    if pairs is None:
        pairs = [(i, i + 1) for i in range(n_views - 1)] or [(0, 0)]
    P = len(pairs)
    s = 0.8 + 0.4 * torch.rand(n_views, generator=g)
    kp = torch.zeros(n_views, 3, 3)
    kp[:, 0, 0] = s
    kp[:, 1, 1] = s
    kp[:, 0, 2] = 20 * torch.randn(n_views, generator=g)
    kp[:, 1, 2] = 20 * torch.randn(n_views, generator=g)
    kp[:, 2, 2] = 1
    src = torch.rand(P, n_points, 2, generator=g) * (size - 20) + 10
    dst = src + 6 * torch.randn(P, n_points, 2, generator=g)
    sd = 1 + 4 * torch.rand(P, n_points, generator=g)
    dd = sd * (1 + 0.05 * torch.randn(P, n_points, generator=g))
    return dict(rgb_processed=torch.rand(n_views, 3, size, size, generator=g), K_prime_to_K=kp,
                shared_focal=shared_focal, src_idx=torch.tensor([a for a, _ in pairs]),
                dst_idx=torch.tensor([b for _, b in pairs]), src_coords=src, dst_coords=dst, src_depth=sd,
                dst_depth=dd)


def correspondence_batch(pairs, depths, sample_num: int = 10000, min_corres_conf: float = 0.1, uniforms=None,
                         device="cuda") -> dict:
    """IMC2021._create_downsampled_arrays (datasets/imc2021.py:317-390) on the HIP path: every pair's
    sample_correspondence_and_depth in one launch sequence (sr_corres_sample).

    ``pairs``: [(src_view, dst_view, corr)], corr either {coords_src, coords_dst, certainty} or the
    matcher's stored uint16 maps {x_png, y_png, conf_png}; ``depths``: one [H, W] fp32 map per view
    (metres).  Arrays or tensors, on the host or the device.  ``uniforms`` ([P, K] fp64 in [0, 1))
    default to np.random.random_sample((P, K)) from numpy's global state -- the draws the reference's
    loop of np.random.choice calls makes, so the same np.random.seed gives the same samples.

    Returns, on ``device``, the reference's src_idx / dst_idx [P] int64, src_coords / dst_coords
    [P, K, 2] and src_depth / dst_depth [P, K] fp32: ``batch.update(...)`` it into a batch for
    Trainer.step / compute_loss.  Raises ValueError naming the pair when none of its correspondences
    lies above ``min_corres_conf`` (io.py:319-322)."""
    from .. import ops
    from ..utils import io

    if int(sample_num) <= 0:
        raise ValueError(f"sample_num must be positive (got {sample_num})")
    if len(pairs) == 0:
        raise ValueError("correspondence_batch: no pairs")
    views = [io.depth_entry(d, f"depths[{v}]") for v, d in enumerate(depths)]
    entries = []
    for j, (s, t, corr) in enumerate(pairs):
        for name, v in (("src_view", s), ("dst_view", t)):
            if not 0 <= int(v) < len(views):
                raise IndexError(f"pair {j}: {name} {v} outside the {len(views)} depth maps")
        entries.append(io.corres_entry(corr, f"pair {j}"))
    u = io.corres_uniforms(uniforms, len(pairs), int(sample_num))
    dev = torch.device(device)
    views = [io._to_corres_device(d, dev) for d in views]
    recs = []
    for (s, t, _), e in zip(pairs, entries):
        r = {k: io._to_corres_device(v, dev) for k, v in e.items()}
        r["depth_src"], r["depth_dst"] = views[int(s)], views[int(t)]
        recs.append(r)
    out = ops.corres_sample(recs, io._to_corres_device(u, dev), min_corres_conf, want_index=False)
    idx = torch.tensor([[int(s) for s, _, _ in pairs], [int(t) for _, t, _ in pairs]], dtype=torch.long)
    idx = idx.to(dev)
    return dict(src_idx=idx[0], dst_idx=idx[1], src_coords=out["src_coords"], dst_coords=out["dst_coords"],
                src_depth=out["src_depth"], dst_depth=out["dst_depth"])
