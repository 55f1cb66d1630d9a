"""Golden vectors for the self-supervised training loss from the REAL
reference modules (read-only import; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss.py

Imports the reference's CDFLossIndexPytorch (train/losses/cdf_loss.py:19-242), its projective
geometry (train/utils/geometry.py: backproject_and_reproject[_with_approximation],
compute_relative_pose, compute_projective_residual) and pose decode
(sailrecon/utils/pose_enc.py:68-135), and composes them in the order of compute_loss
(train/train_imc.py:141-246; that file itself imports packages absent here — eval, tensorboard —
so its 40-line body is followed step by step below).  fp32 on CPU, autograd for the gradient of
the loss with respect to the pose encodings (the camera head's output).

Cases (g8_loss.npz, prefix per case):
  dummy   train_epoch's own setup (train_imc.py:334-350): CDF module built on the dummy indices
          [0] / [0] (one histogram), 2 query views, one pair, 700 points
  shared  as dummy with batch['shared_focal'] = True (averaged recovered intrinsics)
  multi   4 views, 3 pairs x 300 points, CDF nodes = the pairs' frame indices (4 histograms)

Sweep (g8b_loss_sweep.npz): the settings g8 never leaves — non-square images, a CDF window that
puts points outside [min, max), no smoothing, 1024 bins, 64 views / 70 pairs, sparse node ids, a
single point (SWEEP below).  Inputs follow make_case's recipe with a general upper-left 2x2 in
K', coordinates scaled by W and H separately, and a redraw loop: the residuals are evaluated in
fp64 with the oracle's geometry (oracle.sfm_oracle.imc_residuals) and every point whose log1p
residual (either variant) lies within delta = min(1e-3, bin_width / 20) of a multiple of
bin_width / 2 — a histogram edge or a +0.5 lookup edge — or whose projected depth |p_z| < 0.2 is
drawn again until none is left.  An fp32 implementation and an fp64 one then bin every stored
point alike, so a comparison needs no exclusion list.  g8_loss.npz is left alone when its
arrays come out unchanged.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/train")
sys.dont_write_bytecode = True

from losses.cdf_loss import CDFLossIndexPytorch  # noqa: E402
from utils.geometry import (backproject_and_reproject, backproject_and_reproject_with_approximation,  # noqa: E402
                            compute_projective_residual, compute_relative_pose)

from sailrecon.utils.pose_enc import pose_encoding_to_extri_intri  # noqa: E402

from oracle import sfm_oracle as O  # noqa: E402  (fp64 geometry of the redraw loop only)

H = W = 518
CDF_DEFAULT = (0.0, 15.0, 250, 0.05)


def make_case(seed, n_views, pairs, npts, shared, nodes):
    g = torch.Generator().manual_seed(seed)
    T = 0.3 * torch.randn(n_views, 3, generator=g)
    q = torch.randn(n_views, 4, generator=g) * 0.2
    q[:, 3] += 1.0
    fov = 0.9 + 0.3 * torch.rand(n_views, 2, generator=g)
    enc = torch.cat([T, q, fov], -1)
    s = 0.5 + torch.rand(n_views, generator=g)
    kp2k = torch.zeros(n_views, 3, 3)
    kp2k[:, 0, 0] = s
    kp2k[:, 1, 1] = s
    kp2k[:, 0, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 1, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 2, 2] = 1
    P = len(pairs)
    src_idx = torch.tensor([a for a, _ in pairs])
    dst_idx = torch.tensor([b for _, b in pairs])
    src_coords = torch.rand(P, npts, 2, generator=g) * torch.tensor([W * 0.8, H * 0.8]) + 50
    dst_coords = src_coords + 25 * torch.randn(P, npts, 2, generator=g)
    src_depth = 1 + 4 * torch.rand(P, npts, generator=g)
    dst_depth = src_depth * (1 + 0.1 * torch.randn(P, npts, generator=g))
    return dict(enc=enc, kp2k=kp2k, src_idx=src_idx, dst_idx=dst_idx, src_coords=src_coords, dst_coords=dst_coords,
                src_depth=src_depth, dst_depth=dst_depth, shared=shared, nodes_src=torch.tensor(nodes[0]),
                nodes_dst=torch.tensor(nodes[1]))


def edge_delta(min_val, max_val, num_bins):
    bw = (max_val - min_val) / num_bins
    return min(1e-3, bw / 20)


def near_edge(res, min_val, max_val, num_bins):
    """True where res is within edge_delta of min_val + a multiple of bin_width / 2."""
    half = (max_val - min_val) / num_bins / 2
    x = (res - min_val) / half
    return (x - torch.round(x)).abs() * half < edge_delta(min_val, max_val, num_bins)


def make_sweep_case(seed, n_views, pairs, npts, hw, shared, cdf, nodes, num_nodes=None):
    """make_case's recipe with (a) a general upper-left 2x2 in K', (b) coordinates scaled by W and
    H separately, (c) the redraw loop of the module docstring.  Returns (case, redraw rounds)."""
    Hc, Wc = hw
    g = torch.Generator().manual_seed(seed)
    T = 0.3 * torch.randn(n_views, 3, generator=g)
    q = torch.randn(n_views, 4, generator=g) * 0.2
    q[:, 3] += 1.0
    fov = 0.9 + 0.3 * torch.rand(n_views, 2, generator=g)
    enc = torch.cat([T, q, fov], -1)
    kp2k = torch.zeros(n_views, 3, 3)
    kp2k[:, 0, 0] = 0.5 + torch.rand(n_views, generator=g)
    kp2k[:, 1, 1] = 0.5 + torch.rand(n_views, generator=g)
    kp2k[:, 0, 1] = 0.02 * torch.randn(n_views, generator=g)
    kp2k[:, 1, 0] = 0.02 * torch.randn(n_views, generator=g)
    kp2k[:, 0, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 1, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 2, 2] = 1
    P = len(pairs)
    src_idx = torch.tensor([a for a, _ in pairs])
    dst_idx = torch.tensor([b for _, b in pairs])
    size = torch.tensor([float(Wc), float(Hc)])

    def draw(m):
        sc = torch.rand(m, 2, generator=g) * size * 0.8 + size * (50.0 / 518.0)
        dc = sc + 25 * torch.randn(m, 2, generator=g)
        sd = 1 + 4 * torch.rand(m, generator=g)
        dd = sd * (1 + 0.1 * torch.randn(m, generator=g))
        return sc, dc, sd, dd

    sc, dc, sd, dd = (t.reshape(P, npts, *t.shape[1:]) for t in draw(P * npts))
    rounds = 0
    while True:
        r1, r2, pz = O.imc_residuals(enc.double(), hw, kp2k, shared, src_idx, dst_idx, sc, dc, sd, dd)
        bad = near_edge(r1, *cdf[:3]) | near_edge(r2, *cdf[:3]) | (pz.abs() < 0.2)
        if not bool(bad.any()):
            break
        rounds += 1
        for t, n in zip((sc, dc, sd, dd), draw(int(bad.sum()))):
            t[bad] = n
    case = dict(enc=enc, kp2k=kp2k, src_idx=src_idx, dst_idx=dst_idx, src_coords=sc, dst_coords=dc, src_depth=sd,
                dst_depth=dd, shared=shared, nodes_src=torch.tensor(nodes[0]), nodes_dst=torch.tensor(nodes[1]),
                H=Hc, W=Wc, min_val=cdf[0], max_val=cdf[1], num_bins=cdf[2], gradient_smooth=cdf[3],
                num_nodes=num_nodes if num_nodes is not None else max(max(nodes[0]), max(nodes[1])) + 1)
    res = torch.stack([r1, r2])
    return case, rounds, float((res >= cdf[1]).double().mean()), float((res < cdf[0]).double().mean())


def reference_loss(c, hw=(H, W), cdf_args=CDF_DEFAULT, num_nodes=None):
    """compute_loss, train_imc.py:141-246, with predictions from pose_encoding_to_extri_intri."""
    enc = c["enc"].clone().requires_grad_(True)
    extrinsic, intrinsic = pose_encoding_to_extri_intri(enc[None], hw)            # sail_recon.py:122-126
    predicted_intrinsics_batched = intrinsic[0]                                     # :157
    recovered = torch.bmm(c["kp2k"], predicted_intrinsics_batched)                 # :166
    if c["shared"]:                                                                 # :169-174
        recovered = recovered.mean(0, keepdim=True).repeat(recovered.shape[0], 1, 1)
    poses = extrinsic[0]                                                            # :177
    src_K, dst_K = recovered[c["src_idx"]], recovered[c["dst_idx"]]                 # :188-191
    rel = compute_relative_pose(poses[c["src_idx"]], poses[c["dst_idx"]])          # :194
    P = c["src_coords"].shape[0]
    ones = torch.ones(P, 1)
    pred, valid = backproject_and_reproject(c["src_coords"], c["src_depth"], src_K, dst_K, rel, ones)   # :202-209
    res = compute_projective_residual(pred, c["dst_coords"]) * valid.float()       # :212-215
    pred2, valid2 = backproject_and_reproject_with_approximation(                   # :219-228
        c["src_coords"], c["src_depth"], c["dst_depth"], src_K, dst_K, rel, ones, ones)
    res2 = compute_projective_residual(pred2, c["dst_coords"]) * valid2.float()    # :231-234
    rl, rl2 = torch.log1p(res), torch.log1p(res2)                                   # :237-238
    w, w2 = valid.float(), valid2.float()
    cdf = CDFLossIndexPytorch(cdf_args[0], cdf_args[1], cdf_args[2], c["nodes_src"], c["nodes_dst"],       # :334-350
                              gradient_smooth=cdf_args[3], num_nodes=num_nodes)
    a, b = cdf(rl, w)
    reg = (a.mean() + b.mean()) / 2.0                                               # :246-247
    a2, b2 = cdf(rl2, w2)
    approx = (a2.mean() + b2.mean()) / 2.0
    loss = (reg + approx) / 2.0                                                     # :254
    loss.backward()
    return dict(loss=loss.detach(), grad=enc.grad, rl=rl.detach(), rl2=rl2.detach(), cdf_src=a.detach(),
                cdf_dst=b.detach())


def _ring(n):
    return [(i, (i + 1) % n) for i in range(n)]


_V64 = [(i, (7 * i + 3) % 64) for i in range(64)] + [((5 * i + 1) % 64, i) for i in range(6)]

# name: (seed, views, pairs, points, (H, W), shared, (min, max, bins, smooth), (nodes_src, nodes_dst), num_nodes)
SWEEP = {
    "nonsquare": (11, 3, [(0, 1), (1, 2), (2, 0)], 300, (392, 518), False, CDF_DEFAULT, None, None),
    "window": (12, 4, [(0, 1), (1, 2), (3, 0), (2, 3)], 257, (518, 518), False, (4.5, 6.0, 64, 0.05), None, None),
    "nosmooth": (13, 2, [(0, 1)], 700, (518, 336), True, (0.0, 15.0, 250, 0.0), ([0], [0]), None),
    "bins1024": (14, 5, _ring(5), 513, (518, 518), True, (0.0, 15.0, 1024, 0.2), None, None),
    "v64": (15, 64, _V64, 130, (294, 518), False, CDF_DEFAULT, None, None),
    "sparse_nodes": (16, 4, [(0, 1), (2, 2), (3, 1)], 256, (518, 392), False, CDF_DEFAULT, ([5, 0, 2], [2, 6, 6]), 7),
    "one_point": (17, 2, [(1, 0)], 1, (518, 518), False, CDF_DEFAULT, ([0], [0]), None),
}


def _arrays(case, result, keys):
    out = {k: np.asarray(v.numpy() if torch.is_tensor(v) else v) for k, v in case.items()}
    out.update({f"out_{k}": result[k].numpy() for k in keys})
    return out


def main():
    torch.manual_seed(0)
    cases = {
        "dummy": make_case(1, 2, [(0, 1)], 700, False, ([0], [0])),
        "shared": make_case(2, 2, [(1, 0)], 700, True, ([0], [0])),
        "multi": make_case(3, 4, [(0, 1), (1, 2), (3, 0)], 300, False, ([0, 1, 3], [1, 2, 0])),
    }
    out = {}
    for name, c in cases.items():
        r = reference_loss(c)
        for k, v in _arrays(c, r, list(r)).items():
            out[f"{name}/{k}"] = v
        print(name, "loss", float(r["loss"]), "|grad|", float(r["grad"].norm()))
    path = os.path.join(HERE, "g8_loss.npz")
    old = dict(np.load(path)) if os.path.exists(path) else {}
    if old.keys() == out.keys() and all(old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k]) for k in out):
        print("g8_loss.npz unchanged, not rewritten")
    else:
        np.savez_compressed(path, **out)

    out = {}
    for name, (seed, nv, pairs, npts, hw, shared, cdf, nodes, num_nodes) in SWEEP.items():
        if nodes is None:  # CDF nodes = the pairs' view indices
            nodes = ([a for a, _ in pairs], [b for _, b in pairs])
        c, rounds, above, below = make_sweep_case(seed, nv, pairs, npts, hw, shared, cdf, nodes, num_nodes)
        r = reference_loss(c, hw, cdf, c["num_nodes"])
        for k, v in _arrays(c, r, ["loss", "grad"]).items():
            out[f"{name}/{k}"] = v
        print(f"{name}: loss {float(r['loss']):.7f} |grad| {float(r['grad'].norm()):.5f} redraw rounds {rounds} "
              f"above {100 * above:.1f}% below {100 * below:.1f}%")
        if name == "window":
            assert 0.10 <= above + below <= 0.60 and above > 0 and below > 0, "move the window"
    np.savez_compressed(os.path.join(HERE, "g8b_loss_sweep.npz"), **out)


if __name__ == "__main__":
    main()
