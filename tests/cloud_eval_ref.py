"""Point-cloud scoring (sr_cloud_nn, sailrecon_amd/utils/cloud_eval.py): the fp64 numpy restatement of
the contract (DESIGN.md "Scoring point clouds"), an fp32 restatement in which every step is rounded to
fp32, and the generator of the cases of tests/golden/g18_cloud_eval.npz.  Brute force in blocks; numpy
only.

Bounds.  Per case the fp32 restatement is compared with the fp64 one; 4 x its largest error is the
bound the GPU kernel must meet on that case (the margin rule of the pose scores: the kernel contracts
FMAs and so rounds in other places than the restatement, never more often).
"""

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_cloud_eval.npz")

SWEEP_NQ = (1, 63, 64, 65, 257, 1025)
SWEEP_NT = (1, 63, 65, 1000, 4097)
HIST_BIN, HIST_BINS = 0.05, 24
CASES = ("sweep", "ties", "far", "hist", "xform")


# ---------------------------------------------------------------- the contract, restated
def xform_points(p, xf):
    """fl32(s (R p) + t): fp64, every product and sum left to right, rounded to fp32 once."""
    p = np.asarray(p, np.float32).astype(np.float64)
    xf = np.asarray(xf, np.float64)
    s, R, t = xf[0], xf[1:10].reshape(3, 3), xf[10:13]
    out = np.empty(p.shape, np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            rp = (R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]
            out[:, r] = (s * rp + t[r]).astype(np.float32)
    return out


def _finite_rows(p):
    return np.isfinite(p).all(axis=1)


def _nn(q, t, dtype, block):
    """(d2 minimum, index) per query in ``dtype`` arithmetic, every step rounded to it; non-finite
    targets are never selected; non-finite queries, overflowing minima and empty target sets give
    (inf, -1)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    ok_t = np.nonzero(_finite_rows(t))[0]
    ok_q = _finite_rows(q)
    best = np.full(len(q), np.inf, dtype)
    index = np.full(len(q), -1, np.int64)
    if len(ok_t) == 0:
        return best, index
    tt = t[ok_t].astype(dtype)
    with np.errstate(all="ignore"):
        for a in range(0, len(q), block):
            qq = np.where(ok_q[a:a + block, None], q[a:a + block], 0).astype(dtype)
            dx = qq[:, None, 0] - tt[None, :, 0]
            dy = qq[:, None, 1] - tt[None, :, 1]
            dz = qq[:, None, 2] - tt[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            k = d2.argmin(axis=1)  # the first minimum: the lowest index
            m = d2[np.arange(len(k)), k]
            good = ok_q[a:a + block] & np.isfinite(m)
            best[a:a + block] = np.where(good, m, np.inf)
            index[a:a + block] = np.where(good, ok_t[k], -1)
    return best, index


def nn64(q, t, q_xf=None, t_xf=None, block=256):
    """(dist fp64 [Nq], index [Nq]) of the contract: the transform rounds to fp32, everything after it is
    fp64.  NaN / -1 for the non-finite queries."""
    q = xform_points(q, q_xf) if q_xf is not None else np.asarray(q, np.float32)
    t = xform_points(t, t_xf) if t_xf is not None else np.asarray(t, np.float32)
    d2, i = _nn(q, t, np.float64, block)
    return np.where(i >= 0, np.sqrt(np.where(i >= 0, d2, 0)), np.nan), i


def nn32(q, t, q_xf=None, t_xf=None, block=256):
    """The same with every step after the transform rounded to fp32 (no FMA): dist fp32, index."""
    q = xform_points(q, q_xf) if q_xf is not None else np.asarray(q, np.float32)
    t = xform_points(t, t_xf) if t_xf is not None else np.asarray(t, np.float32)
    d2, i = _nn(q, t, np.float32, block)
    return np.where(i >= 0, np.sqrt(np.where(i >= 0, d2, np.float32(0))), np.float32(np.nan)).astype(np.float32), i


def hist_of(d, bin_len, n_bins):
    """[n_bins + 2] counts: slot k < n_bins holds k <= fl32(d / bin_len) < k + 1 (d and bin_len as fp32),
    slot n_bins the larger distances, slot n_bins + 1 the non-finite ones."""
    d = np.asarray(d)
    bad = ~np.isfinite(d)
    with np.errstate(all="ignore"):
        q = (np.where(bad, 0, d).astype(np.float32) / np.float32(bin_len)).astype(np.float32)
    slot = np.where(q < n_bins, np.floor(q), n_bins).astype(np.int64)
    slot[bad] = n_bins + 1
    return np.bincount(slot, minlength=n_bins + 2).astype(np.int64)


def stats_of(d):
    """[6] fp64: n_finite, sum d, sum d^2, max d, n_nonfinite, 0 of fp32 distances (fsum: exact sums)."""
    import math
    d = np.asarray(d)
    fin = d[np.isfinite(d)].astype(np.float64)
    return np.array([len(fin), math.fsum(fin), math.fsum(fin * fin), fin.max() if len(fin) else 0.0, len(d) - len(fin),
                     0.0])


def metrics(d_acc, d_comp, thresholds):
    """The scores from the two distance vectors directly (no histogram)."""
    out = {}
    for name, d in (("acc", np.asarray(d_acc, np.float64)), ("comp", np.asarray(d_comp, np.float64))):
        fin = d[np.isfinite(d)]
        out[f"{name}_mean"], out[f"{name}_rms"], out[f"{name}_max"] = fin.mean(), np.sqrt((fin * fin).mean()), fin.max()
    out["chamfer"] = (out["acc_mean"] + out["comp_mean"]) / 2
    for tau in thresholds:
        p = float((d_acc < tau).sum()) / len(d_acc)  # NaN compares false: in the denominator only
        r = float((d_comp < tau).sum()) / len(d_comp)
        out[f"precision@{tau:g}"], out[f"recall@{tau:g}"] = p, r
        out[f"fscore@{tau:g}"] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out


# ---------------------------------------------------------------- the cases
def sim3(rng, scale):
    """[13] fp64: scale, a random rotation row-major, a translation."""
    a = rng.standard_normal((3, 3))
    qm, r = np.linalg.qr(a)
    qm = qm * np.sign(np.diag(r))
    if np.linalg.det(qm) < 0:
        qm[:, 0] = -qm[:, 0]
    return np.concatenate([[scale], qm.reshape(-1), rng.uniform(-2, 2, 3)])


def sim3_inverse(xf):
    s, R, t = xf[0], xf[1:10].reshape(3, 3), xf[10:13]
    return np.concatenate([[1 / s], R.T.reshape(-1), -(R.T @ t) / s])


def _lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def hist_margin(d64, bound, bin_len, n_bins):
    """Smallest distance of a value to a positive bin edge, in units of ``bound``."""
    edges = np.arange(1, n_bins + 1) * np.float64(np.float32(bin_len))
    return np.abs(d64[:, None] - edges[None, :]).min() / bound


def gen_case(name):
    """The inputs of one case (fp32 clouds, fp64 transforms), seeded."""
    if name == "sweep":  # ragged tiles and slices: prefixes of one pair of clouds
        rng = np.random.default_rng(1801)
        return {"query": rng.uniform(-1, 1, (max(SWEEP_NQ), 3)).astype(np.float32),
                "target": rng.uniform(-1, 1, (max(SWEEP_NT), 3)).astype(np.float32)}
    if name == "ties":
        # a 6^3 integer lattice, every point again 216 places later, against queries at cell centres
        # (8 equally near corners), face centres (4), edge midpoints (2) and on lattice points (0 away):
        # every difference, square and sum is exact in fp32, so the ties are ties in the kernel too
        rng = np.random.default_rng(1802)
        lat = _lattice(6)[rng.permutation(216)]
        q = []
        for off in ((.5, .5, .5), (.5, .5, 0), (.5, 0, 0), (0, 0, 0)):
            q.append(_lattice(5) + np.asarray(off, np.float32))
        q = np.concatenate(q)[rng.permutation(500)][:321]
        return {"query": q.astype(np.float32), "target": np.concatenate([lat, lat]).astype(np.float32)}
    if name == "far":  # 1e3 away from the origin on every axis, 1e-3 between neighbours
        rng = np.random.default_rng(1803)
        t = 1e3 + 1e-3 * (_lattice(12)[:1500] + rng.uniform(-.3, .3, (1500, 3)))
        q = 1e3 + 1e-3 * rng.uniform(0, 11, (700, 3))
        return {"query": q.astype(np.float32), "target": t.astype(np.float32)}
    if name == "hist":  # seeds until every distance keeps 10 bounds from every bin edge
        for seed in range(1804, 1904):
            rng = np.random.default_rng(seed)
            c = {"query": rng.uniform(-1, 1, (5000, 3)).astype(np.float32) * np.float32([1, 1, .2]),
                 "target": rng.uniform(-1, 1, (3000, 3)).astype(np.float32) * np.float32([.8, .8, .1])}
            d64, _ = nn64(c["query"], c["target"])
            d32, _ = nn32(c["query"], c["target"])
            if hist_margin(d64, 4 * np.abs(d32 - d64).max(), HIST_BIN, HIST_BINS) >= 10:
                c["seed"] = np.int64(seed)
                return c
        raise RuntimeError("no seed meets the margin condition")
    if name == "xform":  # pred = S^-1(a subset of gt), rounded to fp32
        rng = np.random.default_rng(1805)
        gt = (rng.uniform(-1, 1, (2000, 3)) * [3, 2, 1] + [4, -1, 7]).astype(np.float32)
        S = sim3(rng, 1.7)
        sub = np.sort(rng.permutation(2000)[:1200])
        return {"gt": gt, "pred": xform_points(gt[sub], sim3_inverse(S)), "S": S, "subset": sub.astype(np.int64)}
    raise KeyError(name)


def answers(name, c):
    """The fp64 answers of a case."""
    if name == "sweep":
        out = {}
        for nt in SWEEP_NT:
            out[f"dist_{nt}"], out[f"index_{nt}"] = nn64(c["query"], c["target"][:nt])
        return out
    if name == "xform":
        a, ai = nn64(c["pred"], c["gt"], q_xf=c["S"])
        b, bi = nn64(c["gt"], c["pred"], t_xf=c["S"])
        return {"acc": a, "acc_index": ai, "comp": b, "comp_index": bi}
    d, i = nn64(c["query"], c["target"])
    return {"dist": d, "index": i}


def build_golden():
    z = {}
    for name in CASES:
        c = gen_case(name)
        for k, v in {**c, **answers(name, c)}.items():
            z[f"{name}/{k}"] = v
    return z


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case(name):
    """Inputs and fp64 answers of a golden case."""
    pre = name + "/"
    return {k[len(pre):]: v for k, v in _npz().items() if k.startswith(pre)}


@functools.lru_cache(maxsize=None)
def case_bound(name):
    """(largest error of the fp32 restatement against the golden fp64 answers, the GPU bound = 4 x it,
    the case's largest distance)."""
    c = case(name)
    if name == "sweep":
        err = big = 0.0
        for nt in SWEEP_NT:
            d32, _ = nn32(c["query"], c["target"][:nt])
            err, big = max(err, np.abs(d32 - c[f"dist_{nt}"]).max()), max(big, c[f"dist_{nt}"].max())
    elif name == "xform":
        a, _ = nn32(c["pred"], c["gt"], q_xf=c["S"])
        b, _ = nn32(c["gt"], c["pred"], t_xf=c["S"])
        err = max(np.abs(a - c["acc"]).max(), np.abs(b - c["comp"]).max())
        big = max(c["acc"].max(), c["comp"].max())
    else:
        d32, _ = nn32(c["query"], c["target"])
        err, big = np.abs(d32 - c["dist"]).max(), c["dist"].max()
    return float(err), 4.0 * float(err), float(big)
