"""Rendering point clouds into camera views (sr_cloud_render, sailrecon_amd/utils/cloud_render.py): the numpy
restatement of the contract (DESIGN.md "Rendering point clouds"), line by line, the case generators and the
generator of tests/golden/g22_cloud_render.npz.  numpy only.

There are no bounds here: every decision is a test on the bits, an integer, or an IEEE fp64 operation in a
stated association, and the z-buffer is a minimum of integers, so everything is compared bit for bit.
"""

import os

import numpy as np

from cloud_eval_ref import sim3, xform_points

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_cloud_render.npz")

QNAN = np.uint32(0x7fc00000)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
DRAWN, SKIPPED, CLIPPED, OUTSIDE = 0, 1, 2, 3
HW = (37, 53)  # odd, and no multiple of any tile
GRID_N = (1, 63, 64, 65, 255, 257, 1025, 2049, 70001)  # 1025: one point beyond a draw tile of 4 x 256
GOLDEN_N, GOLDEN_V = 3000, 3
GOLDEN_NEAR, GOLDEN_FAR = 0.5, 7.0


def finite_bits(x):
    """Exponent bits not all ones, fp32 or fp64."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        return (x.view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
    return (x.view(np.uint64) & np.uint64(0x7ff0000000000000)) != np.uint64(0x7ff0000000000000)


def project(points, extrinsic, intrinsic, hw, *, mask=None, view_id=None, exclude=None, xform=None, z_near=1e-6,
            z_far=np.inf):
    """Per view and point: ``state`` [V, n] (DRAWN, SKIPPED, CLIPPED, OUTSIDE), the camera point ``c`` [V, 3, n]
    fp64, the real pixel ``uv`` [V, n, 2] fp64 and the integer pixel ``ix``, ``iy`` [V, n] int64 (where drawn)."""
    H, W = hw
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    E = np.asarray(extrinsic, np.float32).reshape(-1, 3, 4).astype(np.float64)  # widened exactly
    K = np.asarray(intrinsic, np.float32).reshape(-1, 3, 3).astype(np.float64)
    V, n = len(E), len(p)
    q = xform_points(p, xform) if xform is not None else p
    skip = ~finite_bits(p).all(axis=1) | ~finite_bits(q).all(axis=1)
    if mask is not None:
        skip |= np.asarray(mask).reshape(-1) == 0
    state = np.empty((V, n), np.int8)
    c = np.empty((V, 3, n), np.float64)
    uv = np.full((V, n, 2), np.nan)
    ix, iy = np.zeros((V, n), np.int64), np.zeros((V, n), np.int64)
    qx, qy, qz = (q[:, k].astype(np.float64) for k in range(3))
    z_near, z_far = np.float64(z_near), np.float64(z_far)
    with np.errstate(all="ignore"):
        for v in range(V):
            sk = skip.copy()
            if view_id is not None and exclude is not None:
                sk |= np.asarray(view_id).reshape(-1) == np.asarray(exclude).reshape(-1)[v]
            for r in range(3):
                c[v, r] = ((E[v, r, 0] * qx + E[v, r, 1] * qy) + E[v, r, 2] * qz) + E[v, r, 3]
            clip = ~finite_bits(c[v]).all(axis=0) | (c[v, 2] < z_near) | (c[v, 2] > z_far)
            z = np.where(clip | sk, 1.0, c[v, 2])
            u = K[v, 0, 0] * (c[v, 0] / z) + K[v, 0, 2]
            w = K[v, 1, 1] * (c[v, 1] / z) + K[v, 1, 2]
            fx, fy = np.floor(u + 0.5), np.floor(w + 0.5)
            inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)  # a NaN is outside
            state[v] = np.where(sk, SKIPPED, np.where(clip, CLIPPED, np.where(inside, DRAWN, OUTSIDE)))
            d = state[v] == DRAWN
            ix[v, d], iy[v, d] = fx[d].astype(np.int64), fy[d].astype(np.int64)
            live = ~(sk | clip)
            uv[v, live, 0], uv[v, live, 1] = u[live], w[live]
    return {"state": state, "c": c, "uv": uv, "ix": ix, "iy": iy}


def render(points, extrinsic, intrinsic, hw, *, attr=None, n_attr=None, radius=0, attr_fill=np.nan, **kw):
    """The contract's outputs as integers: ``keys`` [V, H, W] uint64, ``depth`` [V, H, W] uint32 (the bits),
    ``index`` [V, H, W] int32, ``attr`` [V, H, W, c] uint32 (the bits; None without attributes), ``counts`` [V, 4]
    uint32 (covered, drawn, clipped, outside) and ``skipped`` [V]."""
    H, W = hw
    pr = project(points, extrinsic, intrinsic, hw, **kw)
    V, n = pr["state"].shape
    keys = np.full((V, H * W), EMPTY, np.uint64)
    counts = np.zeros((V, 4), np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for v in range(V):
            st = pr["state"][v]
            d = st == DRAWN
            z32 = pr["c"][v, 2].astype(np.float32)  # fl32(c_z)
            key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    x, y = pr["ix"][v] + dx, pr["iy"][v] + dy
                    ok = d & (x >= 0) & (x < W) & (y >= 0) & (y < H)  # footprint pixels outside the frame are dropped
                    np.minimum.at(keys[v], (y * W + x)[ok], key[ok])
            counts[v, 1:] = [(st == DRAWN).sum(), (st == CLIPPED).sum(), (st == OUTSIDE).sum()]
    covered = keys != EMPTY
    counts[:, 0] = covered.sum(axis=1)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.uint32), QNAN)
    index = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    out_attr = None
    if attr is not None:
        a = np.ascontiguousarray(np.asarray(attr, np.float32))
        c = a.shape[1] if n_attr is None else n_attr
        bits = np.ascontiguousarray(a[:, :c]).view(np.uint32)
        fill = np.float32(attr_fill).view(np.uint32) if not isinstance(attr_fill, np.uint32) else attr_fill
        out_attr = np.where(covered[..., None], bits[np.where(covered, index, 0)], fill).reshape(V, H, W, c)
    return {"keys": keys.reshape(V, H, W), "depth": depth.reshape(V, H, W), "index": index.reshape(V, H, W),
            "attr": out_attr, "counts": counts, "skipped": n - counts[:, 1:].astype(np.int64).sum(axis=1),
            "state": pr["state"], "uv": pr["uv"], "c": pr["c"]}


# ---------------------------------------------------------------- generators
def rotation(w):
    """Rodrigues' rotation of the axis-angle vector w, fp64."""
    t = np.linalg.norm(w)
    if t == 0:
        return np.eye(3)
    k = np.asarray(w) / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def cameras(rng, V, hw=HW, turn=0.15, spread=0.3):
    """(extrinsic [V, 3, 4], intrinsic [V, 3, 3]) fp32: cameras near the origin looking down +z, zero skew."""
    H, W = hw
    E, K = np.zeros((V, 3, 4), np.float32), np.zeros((V, 3, 3), np.float32)
    for v in range(V):
        E[v, :, :3] = rotation(rng.normal(0, turn, 3))
        E[v, :, 3] = rng.uniform(-spread, spread, 3)
        f = rng.uniform(0.7, 1.0) * W
        K[v] = [[f, 0, (W - 1) / 2 + rng.uniform(-2, 2)], [0, f * rng.uniform(0.95, 1.05), (H - 1) / 2 + rng.uniform(-2, 2)],
                [0, 0, 1]]
    return E, K


def cloud(rng, n, ldp=3):
    """[n, ldp] fp32: most points in front of cameras(), a share behind them and a share far to the side."""
    p = np.empty((n, ldp), np.float32)
    p[:, 0], p[:, 1] = rng.uniform(-3, 3, n), rng.uniform(-2.5, 2.5, n)
    p[:, 2] = np.where(rng.random(n) < 0.12, rng.uniform(-4, 0.2, n), rng.uniform(0.8, 6, n))
    if ldp > 3:
        p[:, 3:] = np.nan  # padding that is never read
    return p


def gen_case(name, n=2049, V=3, seed=0):
    """Seeded inputs of one named case: a dict of render()'s arguments."""
    rng = np.random.default_rng([2201, seed, n, V, sum(map(ord, name))])
    E, K = cameras(rng, V)
    c = {"points": cloud(rng, n), "extrinsic": E, "intrinsic": K, "hw": HW}
    if name == "grid":
        pass
    elif name == "full":  # every optional input at once
        c["points"] = cloud(rng, n, ldp=5)
        c["attr"] = rng.standard_normal((n, 6)).astype(np.float32)
        c["n_attr"] = 4
        c["mask"] = (rng.random(n) < 0.9).astype(np.uint8)
        c["view_id"] = rng.integers(0, V + 1, n).astype(np.int32)
        c["exclude"] = np.arange(V, dtype=np.int32)[::-1].copy()
        c["xform"] = sim3(rng, 1.1) * np.r_[1, np.ones(9), 0.05 * np.ones(3)]
        c["xform"][1:10] = rotation(rng.normal(0, 0.1, 3)).reshape(-1)
        c["radius"], c["z_near"], c["z_far"], c["attr_fill"] = 1, 0.9, 5.5, -7.5
    elif name == "classes":  # every class of point, planted
        c.update(classes_case(rng, n, V))
    else:
        raise KeyError(name)
    return c


def classes_case(rng, n, V):
    """Identity cameras with exact intrinsics, so that the class of every point is known by construction."""
    H, W = HW
    E = np.zeros((V, 3, 4), np.float32)
    E[:, :, :3] = np.eye(3)
    K = np.tile(np.float32([[32, 0, 26], [0, 32, 18], [0, 0, 1]]), (V, 1, 1))
    kinds = rng.integers(0, 7, n)  # masked, non-finite, near, far, behind, outside, drawn
    z = rng.integers(2, 5, n).astype(np.float32)  # powers of two and 3: x / z * 32 is exact for z in {2, 4}
    z[z == 3] = 4
    px, py = rng.integers(0, W, n).astype(np.float32), rng.integers(0, H, n).astype(np.float32)
    p = np.stack([(px - 26) * z / 32, (py - 18) * z / 32, z], axis=1).astype(np.float32)
    mask = np.ones(n, np.uint8)
    mask[kinds == 0] = 0
    bad = np.nonzero(kinds == 1)[0]
    p[bad, rng.integers(0, 3, len(bad))] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(bad))]
    p[kinds == 2, 2] = 0.25  # below z_near = 1
    p[kinds == 3, 2] = 16.0  # above z_far = 8
    p[kinds == 4, 2] = -2.0
    out = np.nonzero(kinds == 5)[0]
    # u just below -0.5 (outside) ... ; the same points just inside go to kind 6 below
    side = rng.integers(0, 4, len(out))
    zz = p[out, 2]
    p[out, 0] = np.where(side == 0, (np.float32(-0.5 - 2 ** -10) - 26) * zz / 32,
                         np.where(side == 1, (np.float32(W - 0.5) - 26) * zz / 32, p[out, 0]))
    p[out, 1] = np.where(side == 2, (np.float32(-0.5 - 2 ** -10) - 18) * zz / 32,
                         np.where(side == 3, (np.float32(H - 0.5) - 18) * zz / 32, p[out, 1]))
    inn = np.nonzero(kinds == 6)[0][:8]  # u just below W - 0.5 and at -0.5 exactly: the last and the first column
    zz = p[inn, 2]
    p[inn[:4], 0] = (np.float32(W - 0.5 - 2 ** -10) - 26) * zz[:4] / 32
    p[inn[4:], 0] = (np.float32(-0.5) - 26) * zz[4:] / 32
    return {"points": p, "extrinsic": E, "intrinsic": K, "mask": mask, "z_near": 1.0, "z_far": 8.0, "kinds": kinds}


def golden_inputs():
    """The golden's cloud and cameras, redrawn until the margins of make_golden_cloud_render.py hold."""
    rng = np.random.default_rng(2202)
    E, K = cameras(rng, GOLDEN_V)
    p = cloud(rng, GOLDEN_N)
    for _ in range(100):
        bad = ~margins_ok(p, E, K)
        if not bad.any():
            return p, E, K
        p[bad] = cloud(rng, int(bad.sum()))
    raise AssertionError("the margins never held")


def margins_ok(p, E, K, eps=1e-6):
    """Per point: in every view, u + 0.5 and v + 0.5 at least eps from an integer and c_z at least eps
    (relative) from z_near and z_far, for every point that is not behind the near plane by more than that."""
    pr = project(p, E, K, HW, z_near=1e-300)
    ok = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        for v in range(len(E)):
            z = pr["c"][v, 2]
            ok &= (np.abs(z - GOLDEN_NEAR) >= eps * GOLDEN_NEAR) & (np.abs(z - GOLDEN_FAR) >= eps * GOLDEN_FAR)
            t = pr["uv"][v] + 0.5
            live = (z >= GOLDEN_NEAR) & (z <= GOLDEN_FAR)
            ok &= ~live | (np.abs(t - np.round(t)) >= eps).all(axis=1)
    return ok


def build_golden():
    """Our own arrays of the golden file: the inputs and the restatement's images at radius 0 and 1."""
    p, E, K = golden_inputs()
    z = {"points": p, "extrinsic": E, "intrinsic": K, "hw": np.int32(HW), "z_near": np.float64(GOLDEN_NEAR),
         "z_far": np.float64(GOLDEN_FAR)}
    for r in (0, 1):
        out = render(p, E, K, HW, radius=r, z_near=GOLDEN_NEAR, z_far=GOLDEN_FAR)
        z[f"r{r}/depth"], z[f"r{r}/index"], z[f"r{r}/counts"] = out["depth"], out["index"], out["counts"]
    return z
