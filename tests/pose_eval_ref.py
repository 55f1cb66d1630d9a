"""fp64 numpy restatement of the pose-scoring contract (csrc/sr_pose_eval.hip, include/sfm_amd.h
"Scoring poses", DESIGN.md "Scoring poses") -- the oracle of tests/test_pose_eval.py and
tests/test_pose_eval_gpu.py, and the margin rule of tests/golden/make_golden_pose_eval.py.

    errors             per-pair (rot, trans) in degrees; dtype=np.float32 rounds after every step
    slots / histogram  the [3, n_bins + 2] histogram of a set of errors
    accuracy           RRA / RTA / AUC from a histogram
    centres / umeyama  camera centres and the similarity fit (np.linalg.svd), ATE, status bits
    make_pair_case     the seeded generator of the pair cases (stored in golden/g14_pose_eval.npz)
    align_case         the seeded generator of the alignment cases (made when asked for)
    RUNS               every histogram run of the tests: (case, views, bin_deg, n_bins, ambiguity)

Cases and bounds.  A case is a set of views (pred and gt poses).  Its bound is 4 x the largest error
of the fp32 restatement against the fp64 one over all of its pairs, rotation and translation apart
(case_bounds).  The runs with fewer views (N = 2, 3, 65) take the first N views of a case: their pairs
are among the case's, so the case's bound holds for them.  A run's bin width is chosen so that a seed
search can meet the margin condition (every fp64 error >= 10 x its bound from every positive bin
edge): with V error values spread over many bins and a margin m, a seed passes with probability about
exp(-2 m V / bin_deg), so bin_deg grows with the pair count (1 degree up to 3 views, 5 at 33, 15 at
65, 45 at 130).
"""

from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_pose_eval.npz")
RANK_TOL = 1e-12  # sigma_2 <= RANK_TOL * sigma_1: the covariance has rank < 2


# ---------------------------------------------------------------- pair errors
def as34(T) -> np.ndarray:
    T = np.asarray(T)
    if T.ndim == 4 and T.shape[0] == 1:
        T = T[0]
    assert T.ndim == 3 and T.shape[1:] in ((3, 4), (4, 4)), T.shape
    return T[:, :3, :]


def all_pairs(n: int):
    """(i, j) of all i < j in lexicographic order: pair p = i (2n - i - 1) / 2 + (j - i - 1)."""
    i, j = np.triu_indices(n, 1)
    assert np.array_equal(i * (2 * n - i - 1) // 2 + (j - i - 1), np.arange(i.size))
    return i.astype(np.int64), j.astype(np.int64)


def _mm(A, B, ta: bool, tb: bool):
    """[P, 3, 3] product op(A) op(B), every product and every sum rounded to the arrays' dtype."""
    ga = (lambda a, k: A[:, k, a]) if ta else (lambda a, k: A[:, a, k])
    gb = (lambda k, c: B[:, c, k]) if tb else (lambda k, c: B[:, k, c])
    out = np.empty_like(A)
    for a in range(3):
        for c in range(3):
            out[:, a, c] = (ga(a, 0) * gb(0, c) + ga(a, 1) * gb(1, c)) + ga(a, 2) * gb(2, c)
    return out


def relative(T, i, j):
    """R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i in T's dtype ([N, 3, 4])."""
    R, t = T[:, :, :3], T[:, :, 3]
    Rr = _mm(R[j], R[i], False, True)
    ti = t[i]
    Rt = np.stack([(Rr[:, a, 0] * ti[:, 0] + Rr[:, a, 1] * ti[:, 1]) + Rr[:, a, 2] * ti[:, 2] for a in range(3)], 1)
    return Rr, t[j] - Rt


def errors(pred, gt, pairs=None, trans_ambiguity: bool = True, dtype=np.float64):
    """(rot, trans) in degrees per pair, as float64 arrays holding ``dtype`` values.  NaN for a pair
    with a non-finite pose or an index outside [0, N); 0 / 0 for i == j (T_i T_i^-1 is the identity)."""
    P, G = as34(pred).astype(dtype), as34(gt).astype(dtype)
    n = len(P)
    assert len(G) == n
    if pairs is None:
        i, j = all_pairs(n)
    else:
        i, j = np.asarray(pairs[0], dtype=np.int64), np.asarray(pairs[1], dtype=np.int64)
    fin = np.isfinite(P).all((1, 2)) & np.isfinite(G).all((1, 2))
    inside = (i >= 0) & (i < n) & (j >= 0) & (j < n)
    ii, jj = np.where(inside, i, 0), np.where(inside, j, 0)
    ok = inside & fin[ii] & fin[jj]
    safe = np.flatnonzero(fin)[0] if fin.any() else 0  # a stand-in for the pairs that are not evaluated
    ii, jj = np.where(ok, ii, safe), np.where(ok, jj, safe)
    with np.errstate(all="ignore"):
        Rg, a = relative(G, ii, jj)
        Rp, b = relative(P, ii, jj)
        E = _mm(Rg, Rp, True, False)
        half, one = dtype(0.5), dtype(1)
        v = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
        s = half * np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        c = half * (((E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]) - one)
        deg = dtype(180.0 / np.pi)
        rot = np.arctan2(s, c) * deg
        dot = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]  # noqa: E731
        aa, bb, d = dot(a, a), dot(b, b), dot(a, b)
        x = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        trans = np.arctan2(np.sqrt(dot(x, x)), np.abs(d) if trans_ambiguity else d) * deg
        worst = dtype(90.0 if trans_ambiguity else 180.0)
        trans = np.where((aa == 0) & (bb == 0), dtype(0), np.where((aa == 0) | (bb == 0), worst, trans))
    rot, trans = rot.astype(np.float64), trans.astype(np.float64)
    same = ok & (i == j)
    rot[same], trans[same] = 0.0, 0.0
    rot[~ok], trans[~ok] = np.nan, np.nan
    return rot, trans


def slots(err, bin_deg: float, n_bins: int) -> np.ndarray:
    err = np.asarray(err, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = np.floor(err / bin_deg)
    k = np.where(np.isfinite(err), np.minimum(k, n_bins), n_bins + 1)
    return k.astype(np.int64)


def histogram(rot, trans, bin_deg: float, n_bins: int) -> np.ndarray:
    """[3, n_bins + 2] int64, rows rot / trans / max; a pair with a non-finite error is non-finite in
    all three rows."""
    bad = ~(np.isfinite(rot) & np.isfinite(trans))
    rows = [np.where(bad, np.nan, e) for e in (rot, trans, np.maximum(rot, trans))]
    return np.stack([np.bincount(slots(e, bin_deg, n_bins), minlength=n_bins + 2) for e in rows]).astype(np.int64)


def accuracy(hist, thresholds, bin_deg: float) -> dict:
    hist = np.asarray(hist, dtype=np.int64)
    n_bins, total = hist.shape[1] - 2, int(hist[0].sum())
    out = {"n_pairs": total, "n_nonfinite": int(hist[0, -1])}
    for tau in thresholds:
        K = tau / bin_deg
        if abs(K - round(K)) > 1e-9 or not 0 < round(K) <= n_bins:
            raise ValueError(f"threshold {tau} is not a multiple of bin_deg {bin_deg} inside the histogram")
        K = int(round(K))
        below = lambda row, k: int(hist[row, :k].sum())  # noqa: E731  pairs of the row with error < k * bin_deg
        out[f"rra@{tau:g}"] = below(0, K) / total
        out[f"rta@{tau:g}"] = below(1, K) / total
        out[f"auc@{tau:g}"] = sum(below(2, k) / total for k in range(1, K + 1)) / K
    return out


# ---------------------------------------------------------------- alignment
def centres(T) -> np.ndarray:
    T = as34(T).astype(np.float64)
    return -np.einsum("nba,nb->na", T[:, :, :3], T[:, :, 3])


def umeyama(pred, gt, with_scale: bool = True, sign_fix: bool = True) -> dict:
    """gt ~ scale R pred + t over the camera centres; means and deviations taken from view 0's centre
    (coincident centres give a variance of exactly 0).  ``sign_fix=False`` is the naive fit."""
    p, g = centres(pred), centres(gt)
    n = len(p)
    mp, mg = p[0] + (p - p[0]).sum(0) / n, g[0] + (g - g[0]).sum(0) / n
    pc, gc = p - mp, g - mg
    var, S = (pc * pc).sum() / n, gc.T @ pc / n
    status, R, scale, D = 0, np.eye(3), 1.0, np.zeros(3)
    if not var > 0:
        status = 3
    else:
        U, D, Vt = np.linalg.svd(S)
        d = np.ones(3)
        if sign_fix and np.linalg.det(U) * np.linalg.det(Vt) < 0:
            d[2] = -1.0
        R = U @ np.diag(d) @ Vt
        if with_scale:
            scale = float((D * d).sum() / var)
        if not D[1] > RANK_TOL * D[0]:
            status = 2
    t = mg - scale * R @ mp
    err = np.linalg.norm(g - (scale * p @ R.T + t), axis=1)
    return dict(scale=scale, R=R, t=t, ate=float(np.sqrt((err * err).mean())), status=status, err=err, sigma=D,
                extent=float(np.sqrt((gc * gc).sum() / n)))


# ---------------------------------------------------------------- generators
def rotations(rng, n: int, angle=None) -> np.ndarray:
    """[n, 3, 3] fp64: uniformly random rotations, or rotations by ``angle`` (radians, scalar or [n])
    about random axes."""
    if angle is None:
        q = rng.standard_normal((n, 4))
    else:
        ax = rng.standard_normal((n, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        a = np.broadcast_to(np.asarray(angle, dtype=np.float64), (n,))[:, None]
        q = np.concatenate([np.cos(a / 2), np.sin(a / 2) * ax], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def spread_centres(rng, n: int, lo: float = 1.0, hi: float = 10.0) -> np.ndarray:
    """[n, 3] centres of magnitude <= hi per axis, every two at least lo apart (relative translations
    do not cancel)."""
    out = np.empty((n, 3))
    k = 0
    while k < n:
        c = rng.uniform(-hi, hi, 3)
        if k == 0 or np.linalg.norm(out[:k] - c, axis=1).min() >= lo:
            out[k] = c
            k += 1
    return out


def poses(R, c, four: bool) -> np.ndarray:
    """fp32 [n, 3, 4] (or [n, 4, 4]) world-to-camera poses with rotations R and centres c."""
    n = len(R)
    T = np.zeros((n, 4 if four else 3, 4))
    T[:, :3, :3] = R
    T[:, :3, 3] = -np.einsum("nab,nb->na", R, c)
    if four:
        T[:, 3, 3] = 1.0
    return T.astype(np.float32)


# name -> (views, generator settings); pred is 3x4 and gt 4x4, the normal mix
PAIR_CASES = {
    "a33": dict(n=33, rot=0.35, centre_scale=1.7, centre_noise=0.3),     # errors over tens of degrees
    "b130": dict(n=130, rot=0.35, centre_scale=0.6, centre_noise=0.3),   # three 64-wide tiles per side
    "amb12": dict(n=12, rot=0.35, centre_scale=None, centre_noise=0.0),  # unrelated centres: angles up to 180
    "small3": dict(n=33, rot=1e-3, centre_scale=1.7, centre_noise=1e-3),
    "small5": dict(n=33, rot=1e-5, centre_scale=1.7, centre_noise=1e-5),
}
SEED0 = {"a33": 100, "b130": 200, "amb12": 300, "small3": 400, "small5": 500}

# every histogram run: bin widths as the module docstring derives them
RUNS = (
    dict(case="a33", n=2, bin_deg=1.0, n_bins=180, ambiguity=True),
    dict(case="a33", n=3, bin_deg=1.0, n_bins=180, ambiguity=True),
    dict(case="a33", n=33, bin_deg=5.0, n_bins=36, ambiguity=True),
    dict(case="a33", n=33, bin_deg=1.0, n_bins=5, ambiguity=True),  # most pairs overflow
    dict(case="b130", n=65, bin_deg=15.0, n_bins=12, ambiguity=True),
    dict(case="b130", n=130, bin_deg=45.0, n_bins=4, ambiguity=True),
    dict(case="amb12", n=12, bin_deg=5.0, n_bins=36, ambiguity=True),
    dict(case="amb12", n=12, bin_deg=5.0, n_bins=36, ambiguity=False),
    dict(case="small3", n=33, bin_deg=1.0, n_bins=180, ambiguity=True),
    dict(case="small5", n=33, bin_deg=1.0, n_bins=180, ambiguity=True),
    dict(case="a33", n=33, bin_deg=5.0, n_bins=36, ambiguity=True, pairs="list"),  # explicit_pairs(33)
)
MARGIN = 10.0  # x the bound, from every positive bin edge


def make_pair_case(name: str, seed: int):
    """(pred [n, 3, 4] fp32, gt [n, 4, 4] fp32) of a pair case."""
    cfg = PAIR_CASES[name]
    rng = np.random.default_rng(seed)
    n = cfg["n"]
    Rg, cg = rotations(rng, n), spread_centres(rng, n)
    Rp = np.einsum("nab,nbc->nac", rotations(rng, n, angle=cfg["rot"] * rng.uniform(0.2, 1.0, n)), Rg)
    if cfg["centre_scale"] is None:
        cp = spread_centres(rng, n)
    else:
        cp = cfg["centre_scale"] * cg + cfg["centre_noise"] * rng.standard_normal((n, 3))
    return poses(Rp, cp, False), poses(Rg, cg, True)


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(pred, gt) of a stored pair case; shared, do not modify."""
    z = _npz()
    pred, gt = z[f"{name}/pred"], z[f"{name}/gt"]
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


def ordered_pairs(n: int):
    """Every (i, j) with i != j: all i < j first, then the same pairs reversed."""
    i, j = all_pairs(n)
    return np.concatenate([i, j]), np.concatenate([j, i])


def bounds_of(pred, gt):
    """(rot bound, trans bound) in degrees of a set of views: 4 x max |fp32 restatement - fp64
    restatement| over all of its ordered pairs (an explicit list may hold either order), with and
    without the translation ambiguity."""
    pairs = ordered_pairs(len(pred))
    rb = np.abs(errors(pred, gt, pairs, True, np.float32)[0] - errors(pred, gt, pairs)[0]).max()
    tb = max(np.abs(errors(pred, gt, pairs, amb, np.float32)[1] - errors(pred, gt, pairs, amb)[1]).max()
             for amb in (True, False))
    return 4.0 * float(rb), 4.0 * float(tb)


def prefix_pairs(n_case: int, n: int) -> np.ndarray:
    """Positions, in a case's all-pairs order, of the pairs among its first n views (in that prefix's
    own all-pairs order)."""
    _, j = all_pairs(n_case)
    return np.flatnonzero(j < n)


def edge_margin(err, bound: float, bin_deg: float, n_bins: int) -> float:
    """min over the errors of the distance to the nearest positive bin edge (k bin_deg, 1 <= k <=
    n_bins), in units of ``bound``."""
    err = np.asarray(err, dtype=np.float64)
    edges = bin_deg * np.arange(1, n_bins + 1)
    return float(np.abs(err[:, None] - edges[None, :]).min() / bound)


def run_pairs(run: dict):
    """(pair_i, pair_j) of a run over the first run['n'] views: None (all i < j) or the explicit list."""
    return explicit_pairs(run["n"]) if run.get("pairs") == "list" else None


def margin_of(run: dict, pred, gt, bounds) -> float:
    """The margin of one histogram run on the given views of its case, in units of the bounds."""
    n = run["n"]
    rot, trans = errors(pred[:n], gt[:n], run_pairs(run), run["ambiguity"])
    ok = np.isfinite(rot)
    rot, trans, (rb, tb) = rot[ok], trans[ok], bounds
    return min(edge_margin(rot, rb, run["bin_deg"], run["n_bins"]), edge_margin(trans, tb, run["bin_deg"], run["n_bins"]),
               edge_margin(np.maximum(rot, trans), max(rb, tb), run["bin_deg"], run["n_bins"]))


@functools.lru_cache(maxsize=None)
def case_errors(name: str, ambiguity: bool = True):
    """fp64 (rot, trans) of all pairs i < j of a stored case; computed once, shared, do not modify."""
    return errors(*case(name), None, ambiguity)


@functools.lru_cache(maxsize=None)
def case_bounds(name: str):
    return bounds_of(*case(name))


def run_errors(run: dict):
    """fp64 (rot, trans) of a histogram run, in the order the kernel writes them."""
    if run.get("pairs") == "list":
        pred, gt = case(run["case"])
        return errors(pred[:run["n"]], gt[:run["n"]], run_pairs(run), run["ambiguity"])
    rot, trans = case_errors(run["case"], run["ambiguity"])
    sel = prefix_pairs(PAIR_CASES[run["case"]]["n"], run["n"])
    return rot[sel], trans[sel]


def run_margin(run: dict) -> float:
    return margin_of(run, *case(run["case"]), case_bounds(run["case"]))


def explicit_pairs(n: int):
    """A list over n >= 4 views with i > j, i == j, repeats and one index out of range."""
    i = np.array([3, 0, 2, 2, 1, n - 1, 0, 3, 1, n, 2], dtype=np.int32)
    j = np.array([1, 3, 2, 0, 1, 0, 3, 1, 2, 0, 3], dtype=np.int32)
    return i, j


# ---------------------------------------------------------------- alignment cases
ALIGN_CASES = ("n1", "n2", "n3", "n4", "n4_mirror", "n257", "n1000")


@functools.lru_cache(maxsize=None)
def align_case(name: str, noise: float = 0.02):
    """(pred [n, 4, 4], gt [n, 3, 4], truth) with gt centres = s0 R0 pred centres + t0 (+ noise; the
    mirrored case flips z first: no proper rotation maps one onto the other).  For n >= 3 the singular
    values of the covariance are asserted to be separated by >= 10 %."""
    n = {"n1": 1, "n2": 2, "n3": 3, "n4": 4, "n4_mirror": 4, "n257": 257, "n1000": 1000}[name]
    for seed in range(7000 + n, 7100 + n):
        rng = np.random.default_rng(seed)
        cp = spread_centres(rng, n) * np.array([1.0, 0.7, 0.45])  # an anisotropic cloud
        s0, R0, t0 = 2.5, rotations(rng, 1)[0], np.array([1.0, -2.0, 3.0])
        src = cp * np.array([1.0, 1.0, -1.0]) if name == "n4_mirror" else cp
        cg = s0 * src @ R0.T + t0 + noise * rng.standard_normal((n, 3))
        pred, gt = poses(rotations(rng, n), cp, True), poses(rotations(rng, n), cg, False)
        sig = umeyama(pred, gt)["sigma"]
        if n < 3 or (sig[0] >= 1.1 * sig[1] and (n == 3 or sig[1] >= 1.1 * sig[2])):
            return pred, gt, dict(scale=s0, R=R0, t=t0, seed=seed)
    raise AssertionError(f"no seed separates the singular values of {name}")
