"""Depth-map scoring (sr_depth_eval, sr_select_ranks, sailrecon_amd/utils/depth_eval.py): the fp64 numpy
restatement of the contract (DESIGN.md "Scoring depth maps") and the generator of the cases of
tests/golden/g19_depth_eval.npz.  Ranks by np.partition, sums by math.fsum; numpy only.

The restatement is cut where the GPU test cuts it: ``valid_mask`` / ``fit`` / ``apply`` / ``score``.  The
kernel's (s, t) are compared with ``fit``; its ``aligned`` with ``apply`` of ITS (s, t), bit for bit; its
sums, histogram and quantiles with ``score`` of ITS ``aligned``.
"""

import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_depth_eval.npz")

ALIGNS = ("none", "median", "scale", "scale_shift")
N_BINS, BIN_LEN = 100, 0.005  # the golden's histogram: larger errors count in the overflow slot
MARGIN_ULPS = 4
QNAN = np.uint32(0x7fc00000)
DELTAS = (1.25, 1.5625, 1.953125)


# ---------------------------------------------------------------- order statistics
def rank_index(num, den, n):
    """The rule of sr_select_ranks (DESIGN §17's: 1/2 -> (n - 1) // 2, 9/10 -> (9 n + 9) // 10 - 1)."""
    return max((num * n + den - 1) // den - 1, 0)


def select(x, ranks, mask=None, group=None, n_groups=None):
    """(value bits uint32 [n_groups, n_ranks], count [n_groups, 2]) of rows x [n_rows, row_len] fp32."""
    x = np.asarray(x, np.float32)
    n_rows = x.shape[0]
    group = np.arange(n_rows) if group is None else np.asarray(group)
    n_groups = n_rows if n_groups is None else n_groups
    ok = np.isfinite(x) if mask is None else np.isfinite(x) & (np.asarray(mask) != 0)
    value = np.full((n_groups, len(ranks)), QNAN, np.uint32)
    count = np.zeros((n_groups, 2), np.int64)
    for g in range(n_groups):
        rows = group == g
        v = x[rows][ok[rows]]
        count[g] = len(v), int(rows.sum()) * x.shape[1] - len(v)
        for r, (num, den) in enumerate(ranks):
            if len(v):
                k = rank_index(num, den, len(v))
                value[g, r] = np.partition(v, k)[k].view(np.uint32)
    return value, count


# ---------------------------------------------------------------- the scorer, restated
def valid_mask(pred, gt, mask=None, conf=None, conf_min=None, gt_min=0.0, gt_max=np.inf):
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(pred) & np.isfinite(gt) & (gt > np.float32(gt_min)) & (gt <= np.float32(gt_max))
        if mask is not None:
            ok &= np.asarray(mask) != 0
        if conf is not None:
            ok &= np.asarray(conf, np.float32) >= np.asarray(conf_min, np.float32)[:, None]
    return ok


def _fsum(x):
    return math.fsum(np.asarray(x, np.float64).ravel().tolist())


def fit(pred, gt, ok, align, group, n_groups):
    """(xform [n_groups, 2] fp64, status [n_groups]) of the contract's alignments."""
    xf = np.tile(np.array([1.0, 0.0]), (n_groups, 1))
    status = np.zeros(n_groups, np.int64)
    for g in range(n_groups):
        sel = ok & (group == g)[:, None]
        p, q = pred[sel].astype(np.float64), gt[sel].astype(np.float64)
        n = len(p)
        if n == 0:
            status[g] = 2
        elif align == "median":
            k = rank_index(1, 2, n)
            mp, mg = np.partition(p, k)[k], np.partition(q, k)[k]
            if mp > 0:
                xf[g, 0] = mg / mp
            else:
                status[g] = 1
        elif align == "scale":
            spp = _fsum(p * p)
            if spp > 0:
                xf[g, 0] = _fsum(q * p) / spp
            else:
                status[g] = 1
        elif align == "scale_shift":
            pm, gm = _fsum(p) / n, _fsum(q) / n
            sxx = _fsum((p - pm) * (p - pm))
            if sxx > 0:
                xf[g, 0] = _fsum((p - pm) * (q - gm)) / sxx
                xf[g, 1] = gm - xf[g, 0] * pm
            else:
                status[g], xf[g, 1] = 1, gm - pm
    return xf, status


def apply(pred, xf, group):
    """fl32(s p + t): product and sum in fp64, rounded once."""
    with np.errstate(all="ignore"):
        s, t = xf[group, 0][:, None], xf[group, 1][:, None]
        return (s * np.asarray(pred, np.float32).astype(np.float64) + t).astype(np.float32)


def rel_of(aligned, gt):
    """fp64 rel = |a - g| / g from the fp32 a and g."""
    with np.errstate(all="ignore"):
        a, g = aligned.astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
        return np.abs(a - g) / g


def slots(r32, n_bins, bin_len):
    """Histogram slot of every fl32(rel): k <= fl32(r32 / bin_len) < k + 1, n_bins beyond, n_bins + 1 non-finite."""
    with np.errstate(all="ignore"):
        q = r32 / np.float32(bin_len)
        k = np.where(q < np.float32(n_bins), q, n_bins).astype(np.int64)
    return np.where(np.isfinite(r32), k, n_bins + 1)


def score(aligned, gt, ok, group, n_groups, n_bins=N_BINS, bin_len=BIN_LEN):
    """stats [n_groups + 1, 16], hist [n_groups + 1, n_bins + 2], rel_err bits [views, pixels], rel_q bits
    [n_groups + 1, 2] from the fp32 aligned maps."""
    gt = np.asarray(gt, np.float32)
    rel = rel_of(aligned, gt)
    with np.errstate(all="ignore"):
        r32 = rel.astype(np.float32)
    rel_bits = np.where(ok, r32.view(np.uint32), QNAN)
    slot = slots(r32, n_bins, bin_len)
    stats = np.zeros((n_groups + 1, 16))
    hist = np.zeros((n_groups + 1, n_bins + 2), np.int64)
    for g in range(n_groups):
        rows = (group == g)[:, None] & np.ones_like(ok)
        sel = ok & rows
        a, q = aligned[sel].astype(np.float64), gt[sel].astype(np.float64)
        r = rel[sel]
        e = a - q
        pos = np.isfinite(aligned[sel]) & (aligned[sel] > 0)
        with np.errstate(all="ignore"):
            d = np.log(a[pos]) - np.log(q[pos])
        fin = np.isfinite(r32[sel])
        st = stats[g]
        st[0], st[1], st[2] = len(a), int((~pos).sum()), int(rows.sum() - sel.sum())
        st[3], st[4], st[5] = _fsum(r), _fsum(e * e / q), _fsum(e * e)
        st[6], st[7], st[8] = _fsum(d), _fsum(d * d), _fsum(np.abs(d) * 0.43429448190325182765)
        ap, qp = a[pos], q[pos]
        for k, c in enumerate(DELTAS):
            st[9 + k] = int(((ap < c * qp) & (qp < c * ap)).sum())
        st[12] = r[fin].max() if fin.any() else 0.0
        hist[g] = np.bincount(slot[sel], minlength=n_bins + 2)
    for e in range(16):
        stats[n_groups, e] = stats[:n_groups, e].max() if e == 12 else _fsum(stats[:n_groups, e])
    hist[n_groups] = hist[:n_groups].sum(0)
    rel_f = rel_bits.view(np.float32)
    in_group = (group >= 0) & (group < n_groups)
    q_g, _ = select(rel_f, [(1, 2), (9, 10)], group=group, n_groups=n_groups)
    q_all, _ = select(rel_f[in_group], [(1, 2), (9, 10)], group=np.zeros(int(in_group.sum()), np.int64), n_groups=1)
    return dict(stats=stats, hist=hist, rel_err=rel_bits, rel_q=np.concatenate([q_g, q_all]))


def depth_eval(pred, gt, align, group=None, n_groups=None, mask=None, conf=None, conf_min=None, xform=None,
               n_bins=N_BINS, bin_len=BIN_LEN, gt_min=0.0, gt_max=np.inf):
    """The whole call: dict of valid, xform, status, aligned (bits), stats, hist, rel_err (bits), rel_q (bits)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    nv = pred.shape[0]
    if group is None:
        group, n_groups = np.arange(nv), nv
    group = np.asarray(group)
    ok = valid_mask(pred, gt, mask, conf, conf_min, gt_min, gt_max)
    if align == "given":
        _, status = fit(pred, gt, ok, "none", group, n_groups)
        xf = np.asarray(xform, np.float64).reshape(n_groups, 2)
    else:
        xf, status = fit(pred, gt, ok, align, group, n_groups)
    a = apply(pred, xf, group)
    out = score(a, gt, ok, group, n_groups, n_bins, bin_len)
    out.update(valid=ok, xform=xf, status=status, aligned=np.where(ok, a.view(np.uint32), QNAN))
    return out


def metrics(stats, hist, thresholds, bin_len=BIN_LEN):
    """The host-side derivation, restated from the definitions (for one row)."""
    n, n_log = stats[0], stats[0] - stats[1]
    md, md2 = stats[6] / n_log, stats[7] / n_log
    out = dict(abs_rel=stats[3] / n, sq_rel=stats[4] / n, rmse=math.sqrt(stats[5] / n), rmse_log=math.sqrt(md2),
               silog=100 * math.sqrt(md2 - md * md), log10=stats[8] / n_log, delta1=stats[9] / n, delta2=stats[10] / n,
               delta3=stats[11] / n)
    for t in thresholds:
        out[f"inlier@{t:g}"] = hist[:int(round(t / bin_len))].sum() / n
    return out


# ---------------------------------------------------------------- cases
SHAPES = {"a": (3, 70, 70), "b": (5, 37, 53)}
SCOPES = {"a": {"view": None, "scene": [0, 0, 0], "mixed": [0, 1, 0]},
          "b": {"view": None, "scene": [0, 0, 0, 0, 0], "mixed": [0, 1, 0, 1, 2]}}


def make_inputs(seed):
    """Seeded maps: gt in [1, 6), pred = (gt (1 + 0.05 N(0, 1)) - t0) / s0 per view, with planted zeros, NaN
    and Inf, outliers that align to a negative depth, a view without a valid pixel, a view whose median
    prediction is negative and a constant prediction."""
    rng = np.random.default_rng(seed)
    z = {}
    for name, (nv, h, w) in SHAPES.items():
        n = h * w
        gt = rng.uniform(1.0, 6.0, (nv, n))
        s0, t0 = rng.uniform(0.9, 1.1, (nv, 1)), rng.uniform(0.0, 0.1, (nv, 1))
        pred = (gt * (1 + 0.05 * rng.standard_normal((nv, n))) - t0) / s0
        assert (pred.std(1) / pred.mean(1) >= 0.1).all()
        gt, pred = gt.astype(np.float32), pred.astype(np.float32)
        mask = (rng.uniform(size=(nv, n)) > 0.03).astype(np.uint8)
        gt[:, ::17] = 0                                  # the dataset's invalid pixels
        gt[0, 5], gt[0, 6], gt[0, 7] = np.nan, np.inf, -1.0
        pred[0, 40], pred[0, 41], pred[0, 42] = np.nan, np.inf, -np.inf
        pred[0, 100:105] = -20.0                         # aligned depth below zero: n_nonpos
        if name == "b":
            gt[1] = 0                                    # no valid pixel: status bit 1
            pred[2] = -pred[2]                           # med(pred) < 0: status bit 0 under MEDIAN
            pred[3] = 1.5                                # constant: status bit 0 under SCALE_SHIFT
            z["b/conf"] = rng.uniform(1.0, 3.0, (nv, n)).astype(np.float32)
        z[f"{name}/pred"], z[f"{name}/gt"], z[f"{name}/mask"] = pred, gt, mask
    return z


def configs():
    for name in SHAPES:
        for scope, grp in SCOPES[name].items():
            for align in ALIGNS:
                yield name, scope, align


def groups_of(name, scope):
    nv = SHAPES[name][0]
    grp = SCOPES[name][scope]
    return (np.arange(nv), nv) if grp is None else (np.asarray(grp), max(grp) + 1)


def run_config(z, name, scope, align, n_views=None):
    group, ng = groups_of(name, scope)
    nv = SHAPES[name][0] if n_views is None else n_views
    if n_views is not None:
        group = group[:nv]
        ng = int(group.max()) + 1
    return depth_eval(z[f"{name}/pred"][:nv], z[f"{name}/gt"][:nv], align, group, ng, mask=z[f"{name}/mask"][:nv])


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def edge_margin(aligned_bits, gt, ok):
    """Smallest distance of a valid pixel's fp64 rel to a positive bin edge of the histogram, in fp32
    ulps of that rel (nothing lies below edge 0; beyond the last edge everything is overflow)."""
    rel = rel_of(aligned_bits.view(np.float32), gt)[ok]
    rel = rel[np.isfinite(rel)]
    edge = np.clip(np.round(rel / BIN_LEN), 1, N_BINS) * BIN_LEN
    return float((np.abs(rel - edge) / ulp32(rel)).min())


def margins(z):
    """The smallest edge_margin over every configuration of the golden."""
    worst = np.inf
    for name, scope, align in configs():
        group, ng = groups_of(name, scope)
        pred, gt = z[f"{name}/pred"], z[f"{name}/gt"]
        ok = valid_mask(pred, gt, z[f"{name}/mask"])
        xf, _ = fit(pred, gt, ok, align, group, ng)
        worst = min(worst, edge_margin(apply(pred, xf, group).view(np.uint32), gt, ok))
        if worst < MARGIN_ULPS:
            break
    return worst


def build_golden(max_seed=200):
    """The inputs of the first seed whose every fp64 rel lies >= MARGIN_ULPS fp32 ulps from every bin
    edge in every configuration, and the restatement's answers."""
    for seed in range(max_seed):
        z = make_inputs(seed)
        if margins(z) >= MARGIN_ULPS:
            break
    else:
        raise RuntimeError("no seed meets the margin")
    out = dict(z)
    out["seed"] = np.int64(seed)
    for name, scope, align in configs():
        r = run_config(z, name, scope, align)
        for k in ("xform", "status", "stats", "hist", "rel_q"):
            out[f"{name}/{scope}/{align}/{k}"] = r[k]
    return out


_CACHE = {}


def golden():
    if "z" not in _CACHE:
        with np.load(GOLDEN, allow_pickle=False) as f:
            _CACHE["z"] = {k: f[k] for k in f.files}
    return _CACHE["z"]
