"""fp64 numpy restatement of the correspondence sampler's contract (csrc/sr_corres.hip,
include/sfm_amd.h "Training correspondences and depths") -- the oracle of tests/test_corres_sample.py
and tests/test_corres_gpu.py, and the margin rule of tests/golden/make_golden_corres.py.

    weights            w_i = c_i if c_i > float32(min_conf) else 0           (fp32 compare)
    sample_indices     first i with cumsum64(w)[i] > u * T, clamped to the last positive weight
    to_pixels          (c + 1) * (size - 1) / 2 in fp32 (numpy's own rounding: bit-equal)
    bilinear64         grid_sample(bilinear, zeros, align_corners=False) evaluated in fp64
    reference_cdf      the CDF np.random.choice builds from the reference's p = c / sum(c)
    edge_margin        min distance of the uniforms from every edge of reference_cdf
    decode_png / grid  IMC2021._png2coords / _png2certainty and the linspace grid (imc2021.py:68-75,126-131)
"""

from __future__ import annotations

import functools
import os

import numpy as np

MARGIN = 2.0 ** -22  # see DESIGN.md: the reference's CDF edges lie within 2^-22 of the exact-weight ones


def weights(certainty, min_conf) -> np.ndarray:
    c = np.asarray(certainty, dtype=np.float32).reshape(-1)
    return np.where(c > np.float32(min_conf), c, np.float32(0)).astype(np.float64)


def sample_indices(certainty, uniforms, min_conf) -> np.ndarray:
    w = weights(certainty, min_conf)
    cdf = np.cumsum(w)
    total = cdf[-1]
    if not total > 0:
        raise ValueError("no eligible correspondence")
    idx = np.searchsorted(cdf, np.asarray(uniforms, dtype=np.float64) * total, side="right")
    return np.minimum(idx, np.flatnonzero(w > 0)[-1]).astype(np.int64)


def to_pixels(coords, h: int, w: int) -> np.ndarray:
    c = np.asarray(coords, dtype=np.float32)
    out = c.copy()
    out[..., 0] = (c[..., 0] + np.float32(1)) * np.float32(w - 1) / np.float32(2)
    out[..., 1] = (c[..., 1] + np.float32(1)) * np.float32(h - 1) / np.float32(2)
    return out


def bilinear64(depth, coords) -> np.ndarray:
    d = np.asarray(depth, dtype=np.float64)
    h, w = d.shape
    g = np.asarray(coords, dtype=np.float32).astype(np.float64)
    x = ((g[..., 0] + 1) * w - 1) / 2
    y = ((g[..., 1] + 1) * h - 1) / 2
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    out = np.zeros(x.shape, dtype=np.float64)
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            xi, yi = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            out += np.where(ok, d[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)] * wx * wy, 0.0)
    return out


def reference_cdf(certainty, min_conf):
    """(selector, cdf): the reference's filter (io.py:314) and the normalised CDF np.random.choice
    forms from its fp32 probabilities (io.py:325; mtrand: p -> float64, cumsum, / cdf[-1])."""
    c = np.asarray(certainty).reshape(-1)
    sel = c > min_conf
    cf = c[sel]
    p = cf / np.sum(cf)
    cdf = np.asarray(p, dtype=np.float64).cumsum()
    cdf /= cdf[-1]
    return sel, cdf


def edge_margin(certainty, uniforms, min_conf) -> float:
    """min |u - edge| over the uniforms and the interior edges of the reference's CDF (the last edge
    is 1 and no uniform reaches it)."""
    _, cdf = reference_cdf(certainty, min_conf)
    u = np.asarray(uniforms, dtype=np.float64).reshape(-1)
    edges = cdf[:-1]
    if edges.size == 0:
        return 1.0
    j = np.searchsorted(edges, u)
    lo = np.abs(u - edges[np.clip(j - 1, 0, edges.size - 1)])
    hi = np.abs(edges[np.clip(j, 0, edges.size - 1)] - u)
    return float(np.minimum(lo, hi).min())


def decode_png(x_png, y_png, conf_png):
    """(coords_dst [hs*ws, 2] fp32, certainty [hs*ws] fp32)."""
    dec = lambda a: np.asarray(a).astype(np.float32) / 65535.0 * 2 - 1  # noqa: E731
    coords_dst = np.stack([dec(x_png), dec(y_png)], axis=-1).reshape(-1, 2)
    return coords_dst, (np.asarray(conf_png).astype(np.float32) / 1000).reshape(-1)


def grid(hs: int, ws: int) -> np.ndarray:
    """coords_src [hs*ws, 2] fp32: the fp64 linspace grid rounded like imc2021.py:307."""
    xx, yy = np.meshgrid(np.linspace(-1 + 1 / ws, 1 - 1 / ws, ws), np.linspace(-1 + 1 / hs, 1 - 1 / hs, hs),
                         indexing="xy")
    return np.stack([xx, yy], axis=-1).astype(np.float32).reshape(-1, 2)


def sample(coords_src, coords_dst, certainty, depth_src, depth_dst, uniforms, min_conf):
    """The whole contract for one pair: (index, src_coords, dst_coords, src_depth64, dst_depth64)."""
    idx = sample_indices(certainty, uniforms, min_conf)
    cs = np.asarray(coords_src, dtype=np.float32).reshape(-1, 2)[idx]
    cd = np.asarray(coords_dst, dtype=np.float32).reshape(-1, 2)[idx]
    return (idx, to_pixels(cs, *depth_src.shape), to_pixels(cd, *depth_dst.shape), bilinear64(depth_src, cs),
            bilinear64(depth_dst, cd))


# ---------------------------------------------------------------- g13_corres.npz access
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_corres.npz")
SINGLE = ("grid", "chunks", "sparse", "one", "png")
CASES = SINGLE + ("multi",)


@functools.lru_cache(maxsize=None)
def _npz():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """One golden case as {K, min_conf, seed, uniforms [P, K], views, depths, pairs: [{coords_src, coords_dst,
    certainty, depth_src, depth_dst, (x_png, y_png, conf_png)}], index [P, K], out_* [P, K(, 2)]}."""
    z = _npz()
    depths = [z[f"depth_{v}"] for v in range(3)]
    if name == "multi":
        sources = [str(s) for s in z["multi/corr_from"]]
        views = list(zip(z["multi/src_view"].tolist(), z["multi/dst_view"].tolist()))
        outs = {k: z[f"multi/{k}"] for k in ("index", "out_src_coords", "out_dst_coords", "out_src_depth",
                                              "out_dst_depth", "uniforms")}
    else:
        sources = [name]
        views = [(int(z[f"{name}/src_view"]), int(z[f"{name}/dst_view"]))]
        outs = {k: z[f"{name}/{k}"][None] for k in ("index", "out_src_coords", "out_dst_coords", "out_src_depth",
                                                    "out_dst_depth", "uniforms")}
    pairs = []
    for src, (s, t) in zip(sources, views):
        p = {k: z[f"{src}/{k}"] for k in ("coords_src", "coords_dst", "certainty")}
        if src == "png":
            p.update({k: z[f"png/{k}"] for k in ("x_png", "y_png", "conf_png")})
        p["depth_src"], p["depth_dst"] = depths[s], depths[t]
        pairs.append(p)
    return dict(K=int(z[f"{name}/K"]), min_conf=float(z[f"{name}/min_conf"]), seed=int(z[f"{name}/seed"]),
                views=views, depths=depths, pairs=pairs, **outs)


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """The fp64 restatement on a golden case, computed once: per pair (index, src_coords, dst_coords,
    src_depth64, dst_depth64)."""
    c = case(name)
    return [sample(p["coords_src"], p["coords_dst"], p["certainty"], p["depth_src"], p["depth_dst"], c["uniforms"][j],
                   c["min_conf"]) for j, p in enumerate(c["pairs"])]


def depth_bound(name: str) -> float:
    """The depth rule: max(4 * the reference's own fp32 error against the fp64 bilinear, 2 fp32 ulps
    of the case's largest depth), from the golden itself."""
    c, o = case(name), oracle(name)
    ref_err, largest = 0.0, 0.0
    for j, (_, _, _, sd, dd) in enumerate(o):
        ref_err = max(ref_err, np.abs(c["out_src_depth"][j] - sd).max(), np.abs(c["out_dst_depth"][j] - dd).max())
        largest = max(largest, np.abs(sd).max(), np.abs(dd).max())
    return max(4.0 * ref_err, 2.0 * float(np.spacing(np.float32(largest))))
