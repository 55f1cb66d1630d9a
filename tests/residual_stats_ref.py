"""Restatement of sr_imc_residual_stats' contract (include/sfm_amd.h, DESIGN.md "Residual
diagnostics") in torch / numpy, following the dtype of its inputs: fp64 is the checker, fp32 sets
the bounds (4 x its own error against fp64, per case).

Variants 0 / 1 and the frame arrays come from the oracle (oracle.sfm_oracle.imc_residuals, cdf_bins,
cdf_smooth_kernel and its pose decode); the Sampson residual and the rank rules are written out here.
Results are computed once per (case, dtype) and shared: callers do not modify them.
"""

import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from goldens import LOSS_G8, LOSS_G8B, load_npz, loss_case, loss_geometry_args
from oracle import sfm_oracle as O

CASES = LOSS_G8 + LOSS_G8B
GOLDEN_FILE = os.path.join(GOLDEN, "g17_frame_stats.npz")
GOLDEN_CASES = ("dummy", "multi", "window", "nosmooth", "bins1024", "sparse_nodes")
VARIANTS = ("reproj", "reproj_fixed_depth", "sampson")
# 4 x the largest |fp32 restatement - golden| measured over GOLDEN_CASES and the three arrays
# (tests/test_residual_stats.py::test_fp32_restatement_reproduces_golden prints every figure):
# 1.7285e-6, the cdf of bins1024, where 1024 fp32 partial sums meet the reference's CPU cumsum (a
# double accumulator); pmf differs by 0, pdf by at most 1.24e-6 (nosmooth, values up to 1.7)
GOLDEN_BOUND = 4 * 1.7285346984863281e-06


def skew(t):
    z = torch.zeros_like(t[..., 0])
    return torch.stack([torch.stack([z, -t[..., 2], t[..., 1]], -1), torch.stack([t[..., 2], z, -t[..., 0]], -1),
                        torch.stack([-t[..., 1], t[..., 0], z], -1)], -2)


def fundamental(enc, hw, kp2k, shared, src_idx, dst_idx):
    """[P, 3, 3] F = K_d^-T [t]x R K_s^-1 of (R | t) = top 3x4 of E_d E_s^-1, unit Frobenius norm, in enc.dtype."""
    dt = enc.dtype
    ext, intr = O.pose_encoding_to_extri_intri(enc[None], hw)
    K = torch.bmm(kp2k.to(dt), intr[0])
    if shared:
        K = K.mean(0, keepdim=True).repeat(K.shape[0], 1, 1)
    pad = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dt).expand(ext.shape[1], 1, 4)
    E = torch.cat([ext[0], pad], 1)
    s, d = src_idx.long(), dst_idx.long()
    T = torch.bmm(E[d], torch.inverse(E[s]))
    F = torch.inverse(K[d]).transpose(1, 2) @ skew(T[:, :3, 3]) @ T[:, :3, :3] @ torch.inverse(K[s])
    return F / F.flatten(1).norm(dim=1)[:, None, None]


def sampson(F, src_coords, dst_coords, src_idx, dst_idx):
    """[P, K] |x'^T F x| / sqrt((Fx)_0^2 + (Fx)_1^2 + (F^T x')_0^2 + (F^T x')_1^2); NaN where src == dst."""
    dt = F.dtype
    x = torch.cat([src_coords.to(dt), torch.ones_like(src_coords[..., :1], dtype=dt)], -1)
    xp = torch.cat([dst_coords.to(dt), torch.ones_like(dst_coords[..., :1], dtype=dt)], -1)
    Fx = torch.einsum("pij,pkj->pki", F, x)
    Ftx = torch.einsum("pji,pkj->pki", F, xp)
    num = (xp * Fx).sum(-1).abs()
    r = num / torch.sqrt(Fx[..., 0] ** 2 + Fx[..., 1] ** 2 + Ftx[..., 0] ** 2 + Ftx[..., 1] ** 2)
    r[src_idx.long() == dst_idx.long()] = float("nan")
    return r


def residuals_of(c, dtype):
    """(r [3, P, K] pixels, rl [2, P, K] log1p residuals, p_z [P, K]) of a case dict, in ``dtype``."""
    args = loss_geometry_args(c, dtype)
    r1, r2, pz = O.imc_residuals(*args)
    F = fundamental(args[0], args[1], args[2], args[3], c["src_idx"], c["dst_idx"])
    r = torch.stack([torch.expm1(r1), torch.expm1(r2), sampson(F, c["src_coords"], c["dst_coords"], c["src_idx"],
                                                               c["dst_idx"])])
    return r, torch.stack([r1, r2]), pz


def frames_of(c, rl):
    """hist [2, nn, nb] (int64), tot [2, nn] (int64), pmf / cdf / pdf [2, nn, nb] in rl.dtype: the
    arrays of compute_weighted_pdf_cdf_vectorized (cdf_loss.py:123-189) with all-ones weights."""
    dt, nn, nb = rl.dtype, c["num_nodes"], c["num_bins"]
    bw = (c["max_val"] - c["min_val"]) / nb
    ns = c["nodes_src"].long()[:, None].expand(rl.shape[1:]).reshape(-1)
    nd = c["nodes_dst"].long()[:, None].expand(rl.shape[1:]).reshape(-1)
    hist = torch.zeros(2, nn * nb, dtype=torch.int64)
    tot = torch.zeros(2, nn, dtype=torch.int64)
    for v in range(2):
        b, _ = O.cdf_bins(rl[v], c["min_val"], c["max_val"], nb)
        ok = ((b >= 0) & (b < nb)).reshape(-1).long()
        b = b.clamp(0, nb - 1).reshape(-1)
        hist[v].index_add_(0, ns * nb + b, ok)
        hist[v].index_add_(0, nd * nb + b, ok)
        tot[v].index_add_(0, ns, torch.ones_like(ok))
        tot[v].index_add_(0, nd, torch.ones_like(ok))
    hist = hist.view(2, nn, nb)
    pmf = hist.to(dt) / (tot.to(dt)[..., None] + 1e-10)
    # cumsum in bin order with every partial sum rounded to dt: torch.cumsum on the CPU keeps a double
    # accumulator for fp32 input, which would make the "fp32" run of this step an fp64 one
    cdf = torch.empty_like(pmf)
    acc = torch.zeros_like(pmf[..., 0])
    for i in range(nb):
        acc = acc + pmf[..., i]
        cdf[..., i] = acc
    sobel = torch.tensor([-1.0, 0.0, 1.0], dtype=dt) / (2.0 * bw)
    taps = O.cdf_smooth_kernel(bw, c["gradient_smooth"]).to(dt)
    pdf = O._reflect_conv(O._reflect_conv(cdf.view(2 * nn, nb), sobel), taps).view(2, nn, nb)
    return hist, tot, pmf, cdf, pdf


@functools.lru_cache(maxsize=None)
def restate(name, dtype=torch.float64):
    """Everything above for golden case ``name``: dict of r, rl, pz, hist, tot, pmf, cdf, pdf."""
    c = loss_case(name)
    r, rl, pz = residuals_of(c, dtype)
    hist, tot, pmf, cdf, pdf = frames_of(c, rl)
    return dict(r=r, rl=rl, pz=pz, hist=hist, tot=tot, pmf=pmf, cdf=cdf, pdf=pdf)


def residual_error(r, r64):
    """|r - r64| / max(r64, 1 px) per variant ([3] maxima), NaN == NaN counted as no error."""
    r, r64 = np.asarray(r, dtype=np.float64), np.asarray(r64, dtype=np.float64)
    both_nan = np.isnan(r) & np.isnan(r64)
    e = np.where(both_nan, 0.0, np.abs(r - r64) / np.maximum(np.where(both_nan, 1.0, r64), 1.0))
    return e.reshape(3, -1).max(1)


@functools.lru_cache(maxsize=None)
def bounds(name):
    """GPU bounds of case ``name``: 4 x the fp32 restatement's error against the fp64 one.
    {"r": [3] relative to max(r64, 1 px), "cdf": abs, "pdf": abs}."""
    a, b = restate(name, torch.float32), restate(name, torch.float64)
    return {"r": 4.0 * residual_error(a["r"].numpy(), b["r"].numpy()),
            "cdf": 4.0 * float((a["cdf"].double() - b["cdf"]).abs().max()),
            "pdf": 4.0 * float((a["pdf"].double() - b["pdf"]).abs().max())}


def behind_of(r0, pz):
    """Points counted in n_behind: exact residual finite and projected depth <= 0."""
    r0, pz = np.asarray(r0), np.asarray(pz)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r0) & (pz <= 0)


def ranks(n):
    """(median, p90) indices into the n finite values sorted ascending: torch's lower median and
    the smallest element with at least 90 % of the values at or below it."""
    return (n - 1) // 2, (9 * n + 9) // 10 - 1


def pair_summary(r32, behind, thresholds):
    """The rank rules on an fp32 array r32 [3, P, K] (the kernel's own residuals in the GPU tests):
    counts [3, P, 2 + T] int64 (n_finite, n_behind, r < threshold), stats [3, P, 4] fp32 (mean rounded
    once from fp64, median, p90, max: exact elements found with np.partition; NaN if n = 0)."""
    r32 = np.asarray(r32, dtype=np.float32)
    V, P, _ = r32.shape
    th = np.asarray(thresholds, dtype=np.float32)
    counts = np.zeros((V, P, 2 + th.size), dtype=np.int64)
    stats = np.full((V, P, 4), np.nan, dtype=np.float32)
    for v in range(V):
        for p in range(P):
            x = r32[v, p][np.isfinite(r32[v, p])]
            n = x.size
            counts[v, p, 0] = n
            counts[v, p, 1] = int(np.asarray(behind[p]).sum())
            counts[v, p, 2:] = [(x < t).sum() for t in th]
            if n:
                k50, k90 = ranks(n)
                part = np.partition(x, sorted({k50, k90}))
                stats[v, p] = (np.float32(x.astype(np.float64).sum() / n), part[k50], part[k90], x.max())
    return counts, stats


def mean_bound(r32):
    """[3, P] 2 ulp (fp32) of the fp64 mean of the finite values."""
    r = np.asarray(r32, dtype=np.float64)
    fin = np.isfinite(r)
    m = np.where(fin, r, 0.0).sum(-1) / np.maximum(fin.sum(-1), 1)  # 0 where nothing is finite (not compared)
    return 2.0 * np.spacing(np.abs(m).astype(np.float32)).astype(np.float64), m


def golden(name):
    z = load_npz(os.path.basename(GOLDEN_FILE))
    return {k: z[f"{name}/{k}"] for k in ("pmf", "cdf", "pdf")}


def synth_case(seed, n_views, pairs, npts):
    """make_case's recipe (tests/golden/make_golden_loss.py) for the selection shapes: a seeded
    synthetic scene, one CDF node per view, the default CDF settings."""
    g = torch.Generator().manual_seed(seed)
    T = 0.3 * torch.randn(n_views, 3, generator=g)
    q = torch.randn(n_views, 4, generator=g) * 0.2
    q[:, 3] += 1.0
    fov = 0.9 + 0.3 * torch.rand(n_views, 2, generator=g)
    s = 0.5 + torch.rand(n_views, generator=g)
    kp2k = torch.zeros(n_views, 3, 3)
    kp2k[:, 0, 0] = s
    kp2k[:, 1, 1] = s
    kp2k[:, 0, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 1, 2] = 40 * torch.randn(n_views, generator=g)
    kp2k[:, 2, 2] = 1
    P = len(pairs)
    src_coords = torch.rand(P, npts, 2, generator=g) * torch.tensor([518 * 0.8, 518 * 0.8]) + 50
    dst_coords = src_coords + 25 * torch.randn(P, npts, 2, generator=g)
    src_depth = 1 + 4 * torch.rand(P, npts, generator=g)
    dst_depth = src_depth * (1 + 0.1 * torch.randn(P, npts, generator=g))
    return dict(enc=torch.cat([T, q, fov], -1), kp2k=kp2k, src_idx=torch.tensor([a for a, _ in pairs]),
                dst_idx=torch.tensor([b for _, b in pairs]), src_coords=src_coords, dst_coords=dst_coords,
                src_depth=src_depth, dst_depth=dst_depth, shared=False,
                nodes_src=torch.tensor([a for a, _ in pairs]), nodes_dst=torch.tensor([b for _, b in pairs]),
                H=518, W=518, min_val=0.0, max_val=15.0, num_bins=250, gradient_smooth=0.05, num_nodes=n_views)
