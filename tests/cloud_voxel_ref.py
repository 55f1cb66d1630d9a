"""Voxel downsampling (sr_sort_pairs, sr_cloud_voxel, sailrecon_amd/utils/cloud_export.py): the numpy
restatement of the contract (DESIGN.md "Downsampling point clouds"), the numpy model of the sort's tile
plan, and the generator of the cases of tests/golden/g20_cloud_voxel.npz.  numpy only.

There are no bounds here: keys are integers, the order is fixed and the sums are IEEE fp64 in a stated
order, so everything is compared bit for bit.
"""

import functools
import os

import numpy as np

from cloud_eval_ref import sim3, xform_points

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_cloud_voxel.npz")

MEAN, BEST = "mean", "best"

# the sort's tile plan (csrc/sr_sort.hip)
TILE, WAVES, ROUNDS, LANES = 2048, 4, 8, 64
SORT_N = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 3 * TILE + 5, 70001)
SORT_BITS = (1, 7, 8, 9, 16, 33, 64)
SORT_KINDS = ("constant", "two", "random", "top_byte", "low_byte", "ascending", "descending", "three", "junk")


# ---------------------------------------------------------------- the sort's contract and its tile plan
def key_mask(key_bits):
    return np.uint64(0xFFFFFFFFFFFFFFFF) if key_bits >= 64 else np.uint64((1 << key_bits) - 1)


def sort_ref(keys, key_bits=64):
    """The contract: np.argsort(keys & mask, kind="stable")."""
    return np.argsort(np.asarray(keys, np.uint64) & key_mask(key_bits), kind="stable")


def sort_keys(kind, n, key_bits, seed=0):
    """[n] uint64 keys of one kind of the test list."""
    rng = np.random.default_rng([2001, seed, n, key_bits, SORT_KINDS.index(kind)])
    rnd = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    m = key_mask(key_bits)
    if kind == "constant":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if kind == "two":
        return np.where(rng.integers(0, 2, n) == 1, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
    if kind == "random":
        return rnd
    if kind == "top_byte":
        return (rnd & np.uint64(0xFF00000000000000)) | np.uint64(0x00123456789ABCDE)
    if kind == "low_byte":
        return (rnd & np.uint64(0xFF)) | np.uint64(0x123456789ABCDE00)
    if kind == "ascending":
        return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    if kind == "descending":
        return (np.uint64(n) - np.arange(n, dtype=np.uint64)) * np.uint64(0x10001)
    if kind == "three":
        return np.array([5, 0x0101010101010101, 0xF0F0F0F0F0F0F0F0], np.uint64)[rng.integers(0, 3, n)]
    if kind == "junk":  # few distinct values under the mask, random bits above it
        return (rnd & ~m) | (rng.integers(0, 7, n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) & m)
    raise KeyError(kind)


def sort_plan_model(keys, key_bits=64, values=None):
    """What the three kernels of every pass compute, restated: tiles of 2048, four waves of eight rounds of
    64 lanes; the digit-major [256][tiles] table and its exclusive scan; an element's rank among its
    tile's equal digits = the waves before it + its wave's earlier rounds + the lanes below it in its
    ballot group.  Asserts that every position is inside [0, n) and taken once.  Returns (keys, values)
    after the last pass."""
    keys = np.asarray(keys, np.uint64).copy()
    n = len(keys)
    vals = np.arange(n, dtype=np.int64) if values is None else np.asarray(values).astype(np.int64).copy()
    tiles = -(-n // TILE)
    m = key_mask(key_bits)
    lower = np.tril(np.ones((LANES, LANES), bool), -1)  # [lane, earlier lane]
    for p in range(-(-key_bits // 8)):
        digit = np.full(tiles * TILE, -1, np.int64)
        digit[:n] = (((keys & m) >> np.uint64(8 * p)) & np.uint64(255)).astype(np.int64)
        d4 = digit.reshape(tiles, WAVES, ROUNDS, LANES)  # ascending (tile, wave, round, lane) = ascending position
        live = d4 >= 0
        # sort_hist_kernel: the count of every digit per (tile, wave, round), and the table
        group = np.arange(tiles * WAVES * ROUNDS).reshape(tiles, WAVES, ROUNDS, 1)
        flat = (group * 256 + np.where(live, d4, 0))[live]
        cnt = np.bincount(flat, minlength=tiles * WAVES * ROUNDS * 256).reshape(tiles, WAVES, ROUNDS, 256)
        table = cnt.sum(axis=(1, 2)).T  # [256][tiles]
        totals = table.sum(axis=1)
        # sort_scan_kernel: workgroup d starts from the totals of the digits below d and scans its row
        base = np.cumsum(totals) - totals
        scan = base[:, None] + np.cumsum(table, axis=1) - table
        assert (scan.reshape(-1) == np.cumsum(table.reshape(-1)) - table.reshape(-1)).all()  # the whole table's scan
        # sort_scatter_kernel
        per_wave = cnt.sum(axis=2)  # [tiles][WAVES][256]
        wave_base = np.cumsum(per_wave, axis=1) - per_wave
        seen = np.cumsum(cnt, axis=2) - cnt  # the wave's earlier rounds
        same = (d4[..., :, None] == d4[..., None, :]) & live[..., None, :] & lower
        below = same.sum(axis=-1)  # lanes below in the ballot group
        t_i, w_i, r_i, _ = np.nonzero(live)
        dd = d4[live]
        pos = scan[dd, t_i] + wave_base[t_i, w_i, dd] + seen[t_i, w_i, r_i, dd] + below[live]
        assert pos.min() >= 0 and pos.max() < n, "a scattered store would leave the buffer"
        assert len(np.unique(pos)) == n, "two elements share a position"
        nk, nv = np.empty_like(keys), np.empty_like(vals)
        nk[pos], nv[pos] = keys, vals  # live elements in ascending position are the elements in order
        keys, vals = nk, nv
    return keys, vals


# ---------------------------------------------------------------- the downsampling contract
def transformed(points, xform=None):
    """q fp32 [n, 3]: the first three columns, through fl32(s (R p) + t) when a transform is given."""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    return xform_points(p, xform) if xform is not None else p


def voxel_keys(points, voxel, origin=(0, 0, 0), axis_bits=21, mask=None, weight=None, mode=MEAN, xform=None):
    """(q [n, 3] fp32, key [n] uint64 with 2^(3b) where not considered, state [n]: 0 considered, 1 skipped,
    2 outside)."""
    p = np.asarray(points, np.float32)[:, :3]
    n, b = len(p), int(axis_bits)
    q = transformed(p, xform)
    skipped = ~np.isfinite(p).all(axis=1) | ~np.isfinite(q).all(axis=1)
    if mask is not None:
        skipped |= np.asarray(mask) == 0
    if mode == BEST and weight is not None:
        skipped |= np.isnan(np.asarray(weight, np.float32))
    o, v = np.asarray(origin, np.float64), np.float64(voxel)
    with np.errstate(all="ignore"):
        f = np.floor((np.where(skipped[:, None], 0, q).astype(np.float64) - o[None, :]) / v)
    half = np.float64(2 ** (b - 1))
    inside = ((f >= -half) & (f < half)).all(axis=1)  # in fp64, before any conversion to an integer
    considered = inside & ~skipped
    u = np.where(considered[:, None], f + half, 0).astype(np.int64).astype(np.uint64)
    key = (u[:, 2] << np.uint64(2 * b)) | (u[:, 1] << np.uint64(b)) | u[:, 0]
    key = np.where(considered, key, np.uint64(1) << np.uint64(3 * b))
    state = np.where(considered, 0, np.where(skipped, 1, 2))
    return q, key, state


def _segment_sums(values, start, count):
    """fp64 sums of the fp32 ``values`` [m, c] (already in member order) over the segments, left to right:
    step k adds every segment's k-th member to its running sum."""
    acc = np.zeros((len(start), values.shape[1]), np.float64)
    for k in range(int(count.max()) if len(count) else 0):
        rows = np.nonzero(count > k)[0]
        acc[rows] = acc[rows] + values[start[rows] + k].astype(np.float64)
    return acc


def downsample(points, voxel, *, attr=None, n_attr=None, mask=None, weight=None, xform=None, origin=(0, 0, 0),
               axis_bits=21, mode=MEAN):
    """The contract, restated.  Returns points [m, 3] fp32, attr [m, n_attr] fp32, count, index, key [m],
    voxel_of [n] and counts [4] = voxels, considered, skipped, outside."""
    q, key, state = voxel_keys(points, voxel, origin, axis_bits, mask, weight, mode, xform)
    n = len(q)
    a = np.zeros((n, 0), np.float32) if attr is None else np.asarray(attr, np.float32)
    a = a[:, :a.shape[1] if n_attr is None else n_attr]
    order = np.argsort(key, kind="stable")
    order = order[:int((state == 0).sum())]  # the sentinel is the largest key
    sk = key[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    start = np.nonzero(head)[0]
    count = np.diff(np.append(start, len(sk)))
    row = np.cumsum(head) - 1
    voxel_of = np.full(n, -1, np.int64)
    voxel_of[order] = row
    if mode == MEAN:
        with np.errstate(all="ignore"):
            sums = _segment_sums(np.concatenate([q, a], axis=1)[order], start, count)
            out = (sums / count[:, None].astype(np.float64)).astype(np.float32)
        out_p, out_a, index = out[:, :3], out[:, 3:], order[start]
    else:
        w = np.zeros(n, np.float32) if weight is None else np.asarray(weight, np.float32)
        ws = w[order]
        best, pick = ws[start].copy(), start.copy()
        for k in range(1, int(count.max()) if len(count) else 0):
            rows = np.nonzero(count > k)[0]
            better = ws[start[rows] + k] > best[rows]  # strict: equal weights (-0 = +0) keep the lowest index
            best[rows[better]], pick[rows[better]] = ws[start[rows[better]] + k], start[rows[better]] + k
        index = order[pick]
        out_p, out_a = q[index], a[index]
    counts = np.array([len(start), (state == 0).sum(), (state == 1).sum(), (state == 2).sum()], np.int64)
    return {"points": np.ascontiguousarray(out_p), "attr": np.ascontiguousarray(out_a), "count": count.astype(np.int64),
            "index": index.astype(np.int64), "key": sk[start], "voxel_of": voxel_of, "counts": counts}


# ---------------------------------------------------------------- the cases
BOX_LO, BOX_HI = np.float64([3.0, -7.0, 10.0]), np.float64([5.0, -5.5, 11.0])  # the origin is outside
BOX_N = 5000
BOX_VOXELS = {"v1": 0.0843, "v8": 0.1687, "all": 64.0}  # (3 / 5000)^(1/3): about 1; twice that: about 8; one cell


def _box(seed, planted):
    rng = np.random.default_rng(seed)
    p = (BOX_LO + rng.uniform(0, 1, (BOX_N, 3)) * (BOX_HI - BOX_LO)).astype(np.float32)
    rgb = rng.integers(0, 256, (BOX_N, 3)).astype(np.float32) / np.float32(255)
    conf = (1 + rng.integers(0, 64, BOX_N)).astype(np.float32) / np.float32(8)  # coarse: many equal weights
    mask = np.ones(BOX_N, np.uint8)
    weight = conf.copy()
    if planted:
        bad = rng.permutation(BOX_N)[:60]
        p[bad[0:8], 0] = np.nan
        p[bad[8:14], 1] = np.inf
        p[bad[14:20], 2] = -np.inf
        mask[bad[20:40]] = 0
        mask[bad[0]] = 0  # masked and NaN at once: skipped once
        weight[bad[40:52]] = np.nan
        weight[bad[52:56]] = np.float32(-0.0)
        weight[bad[56:60]] = np.float32(0.0)
    return {"points": p, "attr": np.concatenate([rgb, conf[:, None]], axis=1), "mask": mask, "weight": weight}


def _grid(lo, hi):
    g = np.arange(lo, hi, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def gen_case(name):
    """Inputs of one case and the list of its configurations."""
    if name == "box_a":
        c = _box(2011, planted=True)
        c["cfg"] = [dict(voxel=v, tag=t) for t, v in BOX_VOXELS.items()]
        return c
    if name == "box_b":
        c = _box(2012, planted=False)
        c["cfg"] = [dict(voxel=v, tag=t) for t, v in BOX_VOXELS.items()]
        return c
    if name == "faces":
        # every coordinate is origin + k / 4 exactly: the point lies on the face between cells k - 1 and k and
        # belongs to k; its neighbour one ulp below belongs to k - 1
        rng = np.random.default_rng(2013)
        o = np.float64([1.0, 2.0, 3.0])
        on = (o + _grid(-3, 4) * 0.25).astype(np.float32)
        under = np.nextafter(on, np.float32(-np.inf))
        p = np.concatenate([on, under, on])[rng.permutation(3 * len(on))]
        return {"points": p, "attr": rng.uniform(0, 1, (len(p), 4)).astype(np.float32),
                "weight": rng.integers(0, 3, len(p)).astype(np.float32), "cfg": [dict(voxel=0.25, origin=o, tag="q")]}
    if name == "range":
        # both ends of the representable range and one ulp outside it, for axis_bits 4 (cells -8 .. 7 of
        # edge 1/2) and 21 (cells -2^20 .. 2^20 - 1)
        rng = np.random.default_rng(2014)
        pts = []
        for edge in (4.0, 524288.0):
            e = np.float32(edge)
            ends = np.float32([-e, np.nextafter(-e, np.float32(-np.inf)), np.nextafter(e, np.float32(0)), e, 0.25])
            for ax in range(3):
                for v in ends:
                    q = np.float32([0.25, -0.25, 0.75])
                    q[ax] = v
                    pts += [q, q]
        p = np.stack(pts)[rng.permutation(len(pts))]
        return {"points": p, "attr": rng.uniform(0, 1, (len(p), 4)).astype(np.float32),
                "weight": rng.integers(0, 2, len(p)).astype(np.float32),
                "cfg": [dict(voxel=0.5, axis_bits=4, tag="b4"), dict(voxel=0.5, axis_bits=21, tag="b21")]}
    if name == "origin":  # neither the origin nor the edge is an fp32 number
        rng = np.random.default_rng(2015)
        p = rng.uniform(-1, 1, (1500, 3)).astype(np.float32)
        return {"points": p, "attr": rng.uniform(0, 1, (1500, 4)).astype(np.float32),
                "weight": rng.uniform(0, 1, 1500).astype(np.float32),
                "cfg": [dict(voxel=0.05, origin=np.float64([0.1, -0.2, 1 / 3]), axis_bits=7, tag="o")]}
    if name == "xform":  # a similarity with scale 1.7 applied inside the call
        rng = np.random.default_rng(2016)
        p = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
        p[rng.permutation(2000)[:5]] = np.float32(3e38)  # finite, and not after the transform: skipped
        return {"points": p, "attr": rng.uniform(0, 1, (2000, 4)).astype(np.float32),
                "weight": rng.integers(0, 5, 2000).astype(np.float32), "S": sim3(rng, 1.7),
                "cfg": [dict(voxel=0.3, origin=np.float64([0.5, 0.5, 0.5]), axis_bits=10, tag="s")]}
    raise KeyError(name)


CASES = ("box_a", "box_b", "faces", "range", "origin", "xform")
STORED = ("points", "attr", "count", "index", "key", "voxel_of", "counts")


def run_cfg(c, cfg, mode, n_attr=4):
    """The restatement on one configuration of a case."""
    return downsample(c["points"], cfg["voxel"], attr=c["attr"], n_attr=n_attr, mask=c.get("mask"),
                      weight=c.get("weight") if mode == BEST else None, xform=c.get("S"),
                      origin=cfg.get("origin", (0, 0, 0)), axis_bits=cfg.get("axis_bits", 21), mode=mode)


def build_golden():
    """Inputs of every case; the answers of every configuration: the MEAN outputs in full, of BEST what a
    copy of input rows does not already say (index, counts)."""
    z = {}
    for name in CASES:
        c = gen_case(name)
        for k, v in c.items():
            if k != "cfg":
                z[f"{name}/{k}"] = v
        for cfg in c["cfg"]:
            r = run_cfg(c, cfg, MEAN)
            for k in STORED:
                z[f"{name}/{cfg['tag']}/mean/{k}"] = r[k]
            r = run_cfg(c, cfg, BEST)
            z[f"{name}/{cfg['tag']}/best/index"], z[f"{name}/{cfg['tag']}/best/counts"] = r["index"], r["counts"]
    return z


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case(name):
    """Inputs of a golden case as stored, with its configurations, and its stored answers under "answers"."""
    pre = name + "/"
    c = {"cfg": gen_case(name)["cfg"], "answers": {}}
    for k, v in _npz().items():
        if k.startswith(pre):
            rest = k[len(pre):]
            (c["answers"] if "/" in rest else c)[rest] = v
    return c
