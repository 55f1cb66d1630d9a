"""Two-view geometry (sr_two_view, sailrecon_amd/utils/two_view.py): the numpy fp64 restatement of every stage of
include/sfm_amd.h's "Two-view geometry" -- the counter hash, the scorer in the stated operation order (bit for bit
what the kernel computes), selection, refinement, decomposition, pose error -- and the synthetic pair generator of the
tests and of tests/golden/g23_two_view.npz.  numpy only.

The solver stages (null vector, essential projection) use numpy.linalg.eigh on A^T A and E^T E where the kernel
runs cyclic Jacobi on the same matrices: the same definition, equal up to rounding, not to the bit.
"""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_two_view.npz")
CHUNK = 256          # the cost's summation order: chunks of 256 consecutive valid correspondences
MASK64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------- sampling
def mix64(z):
    """The splitmix64 finaliser on a uint64 array."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_slots(seed, p, n_hyp, n_valid):
    """[n_hyp, 8] int64: the positions among the valid correspondences that every hypothesis of pair ``p`` draws; a
    void hypothesis (8 slots not filled after 64 attempts) is a row of -1."""
    h = np.arange(n_hyp, dtype=np.uint64)
    slots = np.full((n_hyp, 8), -1, np.int64)
    filled = np.zeros(n_hyp, np.int64)
    base = ((np.uint64(p) << np.uint64(20)) + h) * np.uint64(64)
    for a in range(64):
        with np.errstate(over="ignore"):
            u = mix64(np.uint64(seed & MASK64) + np.uint64(GOLDEN_GAMMA) * (base + np.uint64(a) + np.uint64(1)))
        j = (((u >> np.uint64(32)) * np.uint64(n_valid)) >> np.uint64(32)).astype(np.int64)
        dup = (slots == j[:, None]).any(axis=1)
        take = ~dup & (filled < 8)
        rows = np.nonzero(take)[0]
        slots[rows, filled[rows]] = j[rows]
        filled[rows] += 1
    slots[filled < 8] = -1
    return slots


# ---------------------------------------------------------------- valid correspondences, normalised coordinates
def valid_flags(src, dst, mask=None):
    """[K] bool of one pair: the mask byte is non-zero and the four fp32 coordinates are finite."""
    ok = np.isfinite(src).all(axis=-1) & np.isfinite(dst).all(axis=-1)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def fxfycxcy(K):
    K = np.asarray(K, np.float32).astype(np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def normalise(src, dst, K_s, K_d):
    """[n, 4] fp64 (x, y, x', y') of fp32 pixels, and the scorer's constants a[4]."""
    fxs, fys, cxs, cys = fxfycxcy(K_s)
    fxd, fyd, cxd, cyd = fxfycxcy(K_d)
    s, d = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        xn = np.stack([(s[:, 0] - cxs) / fxs, (s[:, 1] - cys) / fys, (d[:, 0] - cxd) / fxd, (d[:, 1] - cyd) / fyd], axis=1)
        a = np.array([1.0 / (fxd * fxd), 1.0 / (fyd * fyd), 1.0 / (fxs * fxs), 1.0 / (fys * fys)])
    return xn, a


def rows9(xn):
    """[n, 9] the epipolar rows x^' (x) x^."""
    x, y, xp, yp = xn[:, 0], xn[:, 1], xn[:, 2], xn[:, 3]
    return np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones_like(x)], axis=1)


# ---------------------------------------------------------------- the solver
def smallest_eigenvector(S):
    """[B, 9] unit eigenvectors of the smallest eigenvalue of the symmetric [B, 9, 9]."""
    S = np.asarray(S, np.float64)
    out = np.full(S.shape[:-1], np.nan)
    ok = np.isfinite(S).all(axis=(-1, -2))
    if ok.any():
        out[ok] = np.linalg.eigh(S[ok])[1][..., 0]
    return out


def essential_frames(E):
    """U, V [B, 3, 3] as arrays of columns-in-rows (U[b, k] = u_{k+1}) of include/sfm_amd.h's "decompose"."""
    E = np.asarray(E, np.float64).reshape(-1, 3, 3)
    U, V = np.full(E.shape, np.nan), np.full(E.shape, np.nan)
    ok = np.isfinite(E).all(axis=(-1, -2))
    if ok.any():
        Eo = E[ok]
        q = np.linalg.eigh(np.swapaxes(Eo, 1, 2) @ Eo)[1]  # ascending
        v1, v2 = q[:, :, 2], q[:, :, 1]
        with np.errstate(all="ignore"):
            u1 = np.einsum("brc,bc->br", Eo, v1)
            u1 = u1 / np.linalg.norm(u1, axis=1, keepdims=True)
            w = np.einsum("brc,bc->br", Eo, v2)
            w = w - (u1 * w).sum(axis=1, keepdims=True) * u1
            u2 = w / np.linalg.norm(w, axis=1, keepdims=True)
        U[ok] = np.stack([u1, u2, np.cross(u1, u2)], axis=1)
        V[ok] = np.stack([v1, v2, np.cross(v1, v2)], axis=1)
    return U, V


def project_essential(e):
    """[B, 9] the nearest essential matrices (singular values 1, 1, 0) of [B, 9]; NaN rows where not finite."""
    U, V = essential_frames(e)
    E = np.einsum("br,bc->brc", U[:, 0], V[:, 0]) + np.einsum("br,bc->brc", U[:, 1], V[:, 1])
    E = E.reshape(-1, 9)
    E[~np.isfinite(E).all(axis=1)] = np.nan
    return E


def solve_hypotheses(xn, slots):
    """[H, 9] the projected 8-point models of the drawn slots ([H, 8] positions in xn, -1 rows void), and the
    condition numbers sigma_1 / sigma_8 of their 8 x 9 systems (Inf for a void row)."""
    H = slots.shape[0]
    E, kappa = np.full((H, 9), np.nan), np.full(H, np.inf)
    ok = slots[:, 0] >= 0
    if ok.any():
        A = rows9(xn[slots[ok].reshape(-1)]).reshape(-1, 8, 9)
        E[ok] = project_essential(smallest_eigenvector(np.swapaxes(A, 1, 2) @ A))
        sv = np.linalg.svd(A, compute_uv=False)
        with np.errstate(all="ignore"):
            kappa[ok] = sv[:, 0] / sv[:, 7]
    return E, kappa


# ---------------------------------------------------------------- the scorer, to the bit
def sampson2(E, xn, a):
    """r2 [M, n] and g' [M, n] of models [M, 9] and correspondences [n, 4], in the header's operation order."""
    E = np.asarray(E, np.float64).reshape(-1, 9)[:, :, None]
    x, y, xp, yp = (xn[None, :, k] for k in range(4))
    with np.errstate(all="ignore"):
        ex0 = (E[:, 0] * x + E[:, 1] * y) + E[:, 2]
        ex1 = (E[:, 3] * x + E[:, 4] * y) + E[:, 5]
        ex2 = (E[:, 6] * x + E[:, 7] * y) + E[:, 8]
        e = (xp * ex0 + yp * ex1) + ex2
        et0 = (E[:, 0] * xp + E[:, 3] * yp) + E[:, 6]
        et1 = (E[:, 1] * xp + E[:, 4] * yp) + E[:, 7]
        q0, q1, q2, q3 = ex0 * ex0, ex1 * ex1, et0 * et0, et1 * et1
        g = ((q0 * a[0] + q1 * a[1]) + q2 * a[2]) + q3 * a[3]
        gp = ((q0 + q1) + q2) + q3
        return (e * e) / g, gp


def score(E, xn, a, tau):
    """cost [M] fp64, inliers [M] uint32 and the inlier flags [M, n] of models [M, 9]: the header's "score",
    "inlier" and "cost", bit for bit."""
    E = np.asarray(E, np.float64).reshape(-1, 9)
    tau2 = np.float64(tau) * np.float64(tau)
    r2, _ = sampson2(E, xn, a)
    with np.errstate(invalid="ignore"):
        inl = r2 < tau2
    n = xn.shape[0]
    nch = (n + CHUNK - 1) // CHUNK
    terms = np.zeros((E.shape[0], nch * CHUNK))  # x + 0.0 == x: the padding does not change a sum of terms >= 0
    terms[:, :n] = np.where(inl, r2, tau2)
    terms = terms.reshape(E.shape[0], nch, CHUNK)
    part = np.zeros((E.shape[0], nch))
    for i in range(CHUNK):
        part = part + terms[:, :, i]
    cost = np.zeros(E.shape[0])
    for c in range(nch):
        cost = cost + part[:, c]
    bad = ~np.isfinite(E).all(axis=1)
    cost[bad] = np.inf
    inl[bad] = False
    return cost, inl.sum(axis=1).astype(np.uint32), inl


def select(cost):
    """The lowest model index of the minimum cost; -1 if no cost is finite."""
    m = int(np.argmin(cost))
    return m if np.isfinite(cost[m]) else -1


# ---------------------------------------------------------------- refinement
def refine(E0, xn, a, tau, iters):
    """(E, cost, round) after ``iters`` rounds of the reweighted 8-point from E0."""
    tau2 = np.float64(tau) * np.float64(tau)
    best_E = cur = np.asarray(E0, np.float64).reshape(9)
    best_cost, best_round = score(cur, xn, a, tau)[0][0], 0
    A = rows9(xn)
    for k in range(1, iters + 1):
        s2 = 4.0 * tau2 if k <= iters // 2 else tau2
        r2, gp = sampson2(cur, xn, a)
        with np.errstate(all="ignore"):
            t = 1.0 + r2[0] / s2
            w = (1.0 / (t * t)) / gp[0]
        w[~np.isfinite(w)] = 0.0
        new = project_essential(smallest_eigenvector((A * w[:, None]).T @ A)[None])[0]
        if not np.isfinite(new).all():
            continue
        cur = new
        c = score(cur, xn, a, tau)[0][0]
        if c < best_cost:
            best_E, best_cost, best_round = cur, c, k
    return best_E, best_cost, best_round


# ---------------------------------------------------------------- decomposition, pose error
def candidates(E):
    """The four (R, t) of one E in the header's order."""
    U, V = essential_frames(E)
    U, V = U[0], V[0]
    x = np.outer(U[0], V[1]) - np.outer(U[1], V[0])
    z = np.outer(U[2], V[2])
    Ra, Rb = z + x, z - x
    return [(Ra, U[2]), (Ra, -U[2]), (Rb, U[2]), (Rb, -U[2])]


def front_count(R, t, xn):
    """Correspondences with positive depth in both cameras: the header's closed form, in its operation order."""
    x, y, xp, yp = (xn[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        av = [(R[r, 0] * x + R[r, 1] * y) + R[r, 2] for r in range(3)]
        aa = (av[0] * av[0] + av[1] * av[1]) + av[2] * av[2]
        bb = (xp * xp + yp * yp) + 1.0
        ab = (av[0] * xp + av[1] * yp) + av[2]
        at = (av[0] * t[0] + av[1] * t[1]) + av[2] * t[2]
        bt = (xp * t[0] + yp * t[1]) + t[2]
        D = aa * bb - ab * ab
        lam, mu = (ab * bt - bb * at) / D, (aa * bt - ab * at) / D
        return int(((D > 0.0) & (lam > 0.0) & (mu > 0.0)).sum())


def decompose(E, xn_inliers):
    """(R [3, 3], t [3], n_front, counts [4]) by cheirality over the inliers."""
    cand = candidates(E)
    counts = [front_count(R, t, xn_inliers) for R, t in cand]
    win = int(np.argmax(counts))
    return cand[win][0], cand[win][1], counts[win], counts


def relative_pose(ext, si, di):
    """(R, t) with X_dst = R X_src + t of fp32 camera-from-world [V, 3, 4] extrinsics, in fp64."""
    e = np.asarray(ext, np.float32).astype(np.float64)
    R = e[di, :, :3] @ e[si, :, :3].T
    return R, e[di, :, 3] - R @ e[si, :, 3]


def rot_angle_deg(Ra, Rb):
    Q = Ra.T @ Rb
    v = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    return float(np.degrees(np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(Q) - 1.0))))


def dir_angle_deg(a, b):
    if not (a @ a) > 0.0:
        return float("nan")
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def essential_of(R, t):
    """[t]x R with t scaled to length 1 (zeros for a zero baseline), as [9]."""
    n = np.linalg.norm(t)
    return (skew(t / n) @ R).reshape(9) if n > 0 else np.zeros(9)


# ---------------------------------------------------------------- the whole estimator
def two_view(src, dst, intrinsic, src_idx, dst_idx, *, mask=None, given_E=None, n_hyp=1024, tau=2.0, iters=8, seed=0,
             ref_extrinsic=None):
    """Every output of sr_two_view for [P, K, 2] fp32 coordinates, as a dict of arrays."""
    src, dst = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    P, K = src.shape[:2]
    G = 0 if given_E is None else given_E.shape[1]
    M, V = G + n_hyp, len(intrinsic)
    nan = np.nan
    o = dict(E=np.full((P, 9), nan), R=np.full((P, 9), nan), t=np.full((P, 3), nan), cost=np.full(P, nan),
             n_inliers=np.zeros(P, np.uint32), n_front=np.zeros(P, np.uint32), best=np.full(P, -1, np.int32),
             refined=np.full(P, -1, np.int32), status=np.zeros(P, np.int32), inlier_mask=np.zeros((P, K), np.uint8),
             pose_err=np.full((P, 2), nan), hyp_idx=np.full((P, n_hyp, 8), -1, np.int32), hyp_E=np.full((P, M, 9), nan),
             hyp_cost=np.full((P, M), nan), hyp_inliers=np.zeros((P, M), np.uint32), kappa=np.full((P, n_hyp), np.inf))
    for p in range(P):
        si, di = int(src_idx[p]), int(dst_idx[p])
        if si == di or not (0 <= si < V and 0 <= di < V):
            o["status"][p] = 3
            continue
        ok = valid_flags(src[p], dst[p], None if mask is None else mask[p])
        vi = np.nonzero(ok)[0]
        if len(vi) < 8:
            o["status"][p] = 1
            continue
        xn, a = normalise(src[p][vi], dst[p][vi], intrinsic[si], intrinsic[di])
        if G:
            o["hyp_E"][p, :G] = given_E[p]
        if n_hyp:
            slots = draw_slots(seed, p, n_hyp, len(vi))
            o["hyp_idx"][p] = np.where(slots >= 0, vi[np.maximum(slots, 0)], -1)
            o["hyp_E"][p, G:], o["kappa"][p] = solve_hypotheses(xn, slots)
        o["hyp_cost"][p], o["hyp_inliers"][p], _ = score(o["hyp_E"][p], xn, a, tau)
        best = select(o["hyp_cost"][p])
        if best < 0:
            o["status"][p] = 2
            continue
        o["best"][p] = best
        finish_pair(o, p, o["hyp_E"][p, best], xn, a, vi, tau, iters, ref_extrinsic, si, di)
    return o


def finish_pair(o, p, E_sel, xn, a, vi, tau, iters, ref_extrinsic, si, di):
    """Refinement, mask, decomposition and pose error of pair p from its selected model."""
    E, _, rnd = refine(E_sel, xn, a, tau, iters)
    cost, inl, flags = score(E, xn, a, tau)
    R, t, nf, _ = decompose(E, xn[flags[0]])
    o["E"][p], o["cost"][p], o["n_inliers"][p], o["refined"][p] = E, cost[0], inl[0], rnd
    o["inlier_mask"][p, vi[flags[0]]] = 1
    o["R"][p], o["t"][p], o["n_front"][p] = R.reshape(9), t, nf
    if ref_extrinsic is not None:
        Rr, tr = relative_pose(ref_extrinsic, si, di)
        o["pose_err"][p] = rot_angle_deg(Rr, R), dir_angle_deg(tr, t)


# ---------------------------------------------------------------- an independent pixel-space Sampson distance
def pixel_sampson2(E, src, dst, K_s, K_d, dtype=np.longdouble):
    """Squared Sampson distance [n] in pixels through F = K_d^-T E K_s^-1, by matrix products in ``dtype``: extended
    precision by default, so that the cancellation in x'^T F x (terms of the size of the pixel coordinates against
    a residual of a pixel or less) stays out of the reference."""
    def inv(K):
        K = np.asarray(K, np.float32).astype(dtype)
        o = np.zeros((3, 3), dtype)
        o[0, 0], o[1, 1], o[2, 2] = 1 / K[0, 0], 1 / K[1, 1], 1
        o[0, 2], o[1, 2] = -K[0, 2] / K[0, 0], -K[1, 2] / K[1, 1]
        return o

    F = inv(K_d).T @ np.asarray(E, np.float64).reshape(3, 3).astype(dtype) @ inv(K_s)
    x = np.concatenate([np.asarray(src, np.float32).astype(dtype), np.ones((len(src), 1), dtype)], axis=1)
    xp = np.concatenate([np.asarray(dst, np.float32).astype(dtype), np.ones((len(dst), 1), dtype)], axis=1)
    Fx, Ftx = x @ F.T, xp @ F
    e = (xp * Fx).sum(axis=1)
    return e * e / (Fx[:, 0] ** 2 + Fx[:, 1] ** 2 + Ftx[:, 0] ** 2 + Ftx[:, 1] ** 2)


# ---------------------------------------------------------------- synthetic pairs
def rodrigues(axis, deg):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.radians(deg)
    Kx = skew(k)
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def make_pair(seed, K=1000, outliers=0.3, noise_px=0.5, hw=(480, 640), rot_deg=None, planar=False, baseline=1.0):
    """One synthetic pair: points at depth 4 .. 9 baselines in front of both cameras, two different zero-skew
    intrinsics, a rotation of 5 .. 25 degrees, Gaussian pixel noise, a planted share of uniformly random outliers,
    coordinates rounded to fp32.  Returns a dict (src, dst [K, 2] fp32; K_s, K_d [3, 3] fp32; ext [2, 3, 4] fp32 with
    view 0 the source; R, t the fp64 pose of those fp32 extrinsics; planted [K] bool inliers)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    Ks = np.float32([[rng.uniform(480, 620), 0, W / 2 + rng.uniform(-20, 20)], [0, rng.uniform(480, 620), H / 2 + rng.uniform(-20, 20)],
                     [0, 0, 1]])
    Kd = np.float32([[rng.uniform(480, 620), 0, W / 2 + rng.uniform(-20, 20)], [0, rng.uniform(480, 620), H / 2 + rng.uniform(-20, 20)],
                     [0, 0, 1]])
    deg = rng.uniform(5, 25) if rot_deg is None else rot_deg
    R = rodrigues(rng.normal(size=3), deg)
    t = rng.normal(size=3)
    t = baseline * t / np.linalg.norm(t)
    ext = np.zeros((2, 3, 4), np.float32)
    ext[0, :, :3] = np.eye(3)
    ext[1, :, :3], ext[1, :, 3] = R, t
    R, t = relative_pose(ext, 0, 1)  # what the fp32 extrinsics say
    scale = baseline if baseline > 0 else 1.0
    src, dst = np.zeros((K, 2)), np.zeros((K, 2))
    n = 0
    ksd, kdd = Ks.astype(np.float64), Kd.astype(np.float64)
    while n < K:
        uv = rng.uniform([0, 0], [W, H], size=(K, 2))
        z = np.full(K, 6.0 * scale) if planar else rng.uniform(4, 9, size=K) * scale
        X = np.stack([(uv[:, 0] - ksd[0, 2]) / ksd[0, 0] * z, (uv[:, 1] - ksd[1, 2]) / ksd[1, 1] * z, z], axis=1)
        Y = X @ R.T + t
        keep = Y[:, 2] > 0.5 * scale
        m = min(int(keep.sum()), K - n)
        Yk = Y[keep][:m]
        src[n:n + m] = uv[keep][:m]
        dst[n:n + m] = np.stack([kdd[0, 0] * Yk[:, 0] / Yk[:, 2] + kdd[0, 2], kdd[1, 1] * Yk[:, 1] / Yk[:, 2] + kdd[1, 2]], axis=1)
        n += m
    src += rng.normal(scale=noise_px, size=src.shape) if noise_px > 0 else 0.0
    dst += rng.normal(scale=noise_px, size=dst.shape) if noise_px > 0 else 0.0
    planted = np.ones(K, bool)
    n_out = int(round(outliers * K))
    out = rng.permutation(K)[:n_out]
    planted[out] = False
    src[out] = rng.uniform([0, 0], [W, H], size=(n_out, 2))
    dst[out] = rng.uniform([0, 0], [W, H], size=(n_out, 2))
    return dict(src=src.astype(np.float32), dst=dst.astype(np.float32), K_s=Ks, K_d=Kd, ext=ext, R=R, t=t, planted=planted)


def stack_pairs(pairs):
    """Several make_pair results as one problem: pair p uses views 2 p and 2 p + 1."""
    src = np.stack([q["src"] for q in pairs])
    dst = np.stack([q["dst"] for q in pairs])
    intr = np.stack([k for q in pairs for k in (q["K_s"], q["K_d"])])
    ext = np.concatenate([q["ext"] for q in pairs])
    si = np.arange(0, 2 * len(pairs), 2, dtype=np.int32)
    return src, dst, intr, si, si + 1, ext


# ---------------------------------------------------------------- the shapes and bounds of the GPU tests
KAPPA_MAX = 1e5    # hypotheses whose 8 x 9 system is worse conditioned are left out of the hyp_E bound (at most 2 %)
HYP_Q = 2          # the kernel and this file solve on A^T A: the error grows with kappa^2
C_HYP = 18.75      # hyp_E: angle to the restatement's <= C_HYP 2^-52 kappa^2: 8 x the worst ratio on an MI355X, 2.344
                   # (case p1_k1003_h512)
REFINE_TOL = 5.4e-12  # refined E: angle to the restatement's in radians: 8 x the worst on an MI355X, 6.72e-13


def angle_up_to_sign(a, b):
    """Angles [B] between the rows of [B, 9] up to sign, by the chord (accurate near 0)."""
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    d = np.minimum(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))
    return 2.0 * np.arcsin(np.minimum(0.5 * d, 1.0))


def _scene(seeds, K, **kw):
    return stack_pairs([make_pair(s, K, **kw) for s in seeds])


def gpu_cases():
    """name -> dict(src, dst, intrinsic, src_idx, dst_idx, ext, mask, given_E, n_hyp, iters, seed, tau): P in
    {1, 3, 70}, K in {8, 9, 257, 1003}, H in {0, 1, 63, 65, 512}, G in {0, 1, 5}; masks, NaN / Inf coordinates, a
    pair with 7 valid points, a pair of equal views, NaN and duplicate given models."""
    rng = np.random.default_rng(23)
    cases = {}

    def add(name, scene, n_hyp, iters, seed, mask=None, given_E=None, tau=2.0):
        src, dst, intr, si, di, ext = scene
        cases[name] = dict(src=src, dst=dst, intrinsic=intr, src_idx=si, dst_idx=di, ext=ext, mask=mask, given_E=given_E,
                           n_hyp=n_hyp, iters=iters, seed=seed, tau=tau)

    add("p1_k1003_h512", _scene([11], 1003), 512, 8, 5)
    # three pairs: masked with NaN / Inf coordinates; 7 valid points; equal views
    sc = list(_scene([21, 22, 23], 257, outliers=0.2))
    mask = (rng.random((3, 257)) < 0.8).astype(np.uint8)
    sc[0][0, 5, 0], sc[0][0, 77, 1], sc[1][0, 130, 0], sc[1][0, 256, 1] = np.nan, np.inf, -np.inf, np.nan
    mask[0, [5, 77, 130, 256]] = 1
    mask[1] = 0
    mask[1, [0, 3, 64, 65, 128, 255, 256]] = 1
    sc[4] = sc[4].copy()
    sc[4][2] = sc[3][2]
    true_E = np.stack([essential_of(*relative_pose(sc[5], 2 * p, 2 * p + 1)) for p in range(3)])
    add("p3_k257_h65_g1", tuple(sc), 65, 4, 1234567890123, mask=mask, given_E=true_E[:, None, :].copy())
    add("p70_k9_h63", _scene(range(100, 170), 9, outliers=0.0, noise_px=0.2), 63, 2, 2 ** 63 + 9)
    sc = _scene([31, 32, 33], 8, outliers=0.0, noise_px=0.2)
    add("p3_k8_h1_g5", sc, 1, 1, 3, given_E=rng.normal(size=(3, 5, 9)))
    add("p1_k8_h65_void", _scene([34], 8, outliers=0.0, noise_px=0.2), 65, 2, 11)  # seed 11: one hypothesis is void
    sc = _scene([41], 1003)
    g = rng.normal(size=(1, 5, 9))
    g[0, 1] = essential_of(*relative_pose(sc[5], 0, 1))
    g[0, 3] = g[0, 1]          # an exact tie: the lower index wins
    g[0, 0, 4] = np.nan        # a NaN model: cost +Inf
    add("p1_k1003_h0_g5", sc, 0, 0, 0, given_E=g)
    sc = _scene([51], 1003)
    g = np.full((1, 1, 9), np.nan)
    add("p1_k1003_h0_g1_nan", sc, 0, 3, 0, given_E=g)   # no finite model: status 2
    return cases
