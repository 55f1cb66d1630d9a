"""The stable radix sort and the voxel downsampling on the GPU (sr_sort_pairs, sr_cloud_voxel,
sailrecon_amd/utils/cloud_export.py) against the numpy restatement (tests/cloud_voxel_ref.py,
tests/golden/g20_cloud_voxel.npz).

There are no tolerances: keys are integers, the order is fixed and the sums are IEEE fp64 in a stated
order.  Every comparison is bit for bit, and a second run gives the same bits.
"""

import os
import sys

import numpy as np
import pytest
import torch

import cloud_voxel_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT32, SENT64, SENTF = -7, -7, -7.0


def bits(x):
    """The bit patterns of a float array (NaN-safe equality)."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint64) if x.dtype == np.float64 else x


def dev_keys(k):
    return torch.from_numpy(np.asarray(k, np.uint64).view(np.int64).copy()).to(DEV)


# ---------------------------------------------------------------- the sort
def gpu_sort(keys, key_bits, values=None, want_keys=True):
    from sailrecon_amd import ops
    k = dev_keys(keys)
    v = None if values is None else torch.from_numpy(values.astype(np.int32)).to(DEV)
    before = k.clone()
    sk, sv = ops.sort_pairs(k, v, key_bits, want_keys=want_keys)
    assert torch.equal(k, before), "the input keys were written"
    return (None if sk is None else sk.cpu().numpy().view(np.uint64)), sv.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("key_bits", R.SORT_BITS)
def test_sort_is_the_stable_argsort(key_bits):
    """Every size x every kind of key, with the values absent (the permutation) and given, with and
    without the sorted keys; the large sizes twice."""
    for n in R.SORT_N:
        for kind in R.SORT_KINDS:
            keys = R.sort_keys(kind, n, key_bits)
            ref = R.sort_ref(keys, key_bits)
            sk, perm = gpu_sort(keys, key_bits)
            assert np.array_equal(perm, ref), (n, kind, "permutation")
            assert np.array_equal(sk, keys[ref]), (n, kind, "keys: bits above key_bits ride along")
            vals = (np.arange(n, dtype=np.int64) * 7919 + 13) % 2 ** 31
            sk2, sv = gpu_sort(keys, key_bits, values=vals, want_keys=False)
            assert sk2 is None and np.array_equal(sv, vals[ref]), (n, kind, "values, no keys")
            if n >= 2049:
                sk3, sv3 = gpu_sort(keys, key_bits, values=vals)
                assert np.array_equal(sv3, sv) and np.array_equal(sk3, sk), (n, kind, "second run")


# 1025 tiles: the rows that sort_scan_kernel and voxel_head_scan_kernel scan in chunks of 4 x 256 values enter a
# second chunk, whose results depend on the carry out of the first
CARRY_N = 1024 * R.TILE + 1


def test_sort_carries_into_the_second_chunk_of_the_table_scan():
    keys = R.sort_keys("random", CARRY_N, 40)
    ref = R.sort_ref(keys, 40)
    sk, perm = gpu_sort(keys, 40)
    assert np.array_equal(perm, ref), "permutation"
    assert np.array_equal(sk, keys[ref]), "keys: bits above key_bits ride along"


def test_sort_rejections_surface_as_errors():
    from sailrecon_amd import ops
    from sailrecon_amd._lib import SfmAmdError
    k = dev_keys(np.arange(10))
    v = torch.arange(10, device=DEV, dtype=torch.int32)
    with pytest.raises(SfmAmdError, match="key_bits"):
        ops.sort_pairs(k, key_bits=65)
    with pytest.raises(SfmAmdError, match="own input"):
        ops.sort_pairs(k, out_keys=k)
    with pytest.raises(SfmAmdError, match="own input"):
        ops.sort_pairs(k, v, out_values=v)


# ---------------------------------------------------------------- the downsampling
OUTS = ("points", "attr", "count", "index", "key", "voxel_of", "counts")


def gpu_voxel(points, voxel, *, attr=None, n_attr=0, mask=None, weight=None, xform=None, origin=(0, 0, 0), axis_bits=21,
              mode="mean", capacity=None, extra=0, skip=()):
    """One sr_cloud_voxel call with every output (but those in ``skip``) allocated ``capacity + extra`` rows
    and prefilled with a sentinel; the raw arrays, on the host."""
    from sailrecon_amd import ops
    up = lambda x, dt=None: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype=dt)  # noqa: E731
    p = up(points)
    n = len(points)
    cap = n if capacity is None else capacity
    rows = cap + extra
    o = {"points": torch.full((rows, 3), SENTF, device=DEV),
         "attr": torch.full((rows, n_attr), SENTF, device=DEV) if n_attr else None,
         "count": torch.full((rows,), SENT32, device=DEV, dtype=torch.int32),
         "index": torch.full((rows,), SENT32, device=DEV, dtype=torch.int32),
         "key": torch.full((rows,), SENT64, device=DEV, dtype=torch.int64),
         "voxel_of": torch.full((n,), SENT32, device=DEV, dtype=torch.int32),
         "counts": torch.full((4,), SENT32, device=DEV, dtype=torch.int32)}
    for k in skip:
        o[k] = None
    ops.cloud_voxel(p, voxel, o["points"], attr=up(attr), n_attr=n_attr if attr is not None else None, mask=up(mask),
                    weight=up(weight), xform=up(xform, torch.float64), origin=origin, axis_bits=axis_bits, mode=mode,
                    capacity=cap, out_attr=o["attr"], out_count=o["count"], out_index=o["index"], out_key=o["key"],
                    voxel_of=o["voxel_of"], counts=o["counts"])
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def compare(got, want, n_attr, what, rows=None):
    """Bit for bit, the first ``rows`` rows (default: all voxels); every row after them keeps the sentinel."""
    m = int(want["counts"][0])
    rows = m if rows is None else rows
    assert np.array_equal(got["counts"].astype(np.int64), want["counts"]), (what, got["counts"], want["counts"])
    assert np.array_equal(got["voxel_of"].astype(np.int64), want["voxel_of"]), what
    assert np.array_equal(bits(got["points"][:rows]), bits(want["points"][:rows])), what
    assert (got["points"][rows:] == SENTF).all(), (what, "rows beyond the result were written")
    if n_attr:
        assert np.array_equal(bits(got["attr"][:rows]), bits(want["attr"][:rows, :n_attr])), what
        assert (got["attr"][rows:] == SENTF).all(), what
    for k, w in (("count", want["count"]), ("index", want["index"]), ("key", want["key"].view(np.int64))):
        assert np.array_equal(got[k][:rows].astype(np.int64), w[:rows]), (what, k)
        assert (got[k][rows:] == SENT32).all(), (what, k)


@pytest.mark.parametrize("name", R.CASES)
def test_golden_cases(name):
    """Every golden case x both modes x n_attr 0, 1, 4 x ldp 3 and 4 (the fourth column NaN), against the
    restatement and, where they are stored, the golden answers; the first configuration twice."""
    c = R.case(name)
    again = None
    for cfg in c["cfg"]:
        for mode in (R.MEAN, R.BEST):
            for n_attr in (0, 1, 4):
                want = R.run_cfg(c, cfg, mode, n_attr)
                if n_attr == 4:
                    pre = f"{cfg['tag']}/{mode}/"
                    for k, v in c["answers"].items():
                        if k.startswith(pre):
                            assert np.array_equal(bits(want[k[len(pre):]]), bits(v)), (name, k)
                for ldp in (3, 4):
                    p = c["points"]
                    if ldp == 4:
                        p = np.concatenate([p, np.full((len(p), 1), np.nan, np.float32)], axis=1)
                    kw = dict(attr=c["attr"] if n_attr else None, n_attr=n_attr, mask=c.get("mask"),
                              weight=c.get("weight") if mode == R.BEST else None, xform=c.get("S"),
                              origin=cfg.get("origin", (0, 0, 0)), axis_bits=cfg.get("axis_bits", 21), mode=mode)
                    got = gpu_voxel(p, cfg["voxel"], extra=8, **kw)
                    what = (name, cfg["tag"], mode, n_attr, ldp)
                    compare(got, want, n_attr, what)
                    assert int(got["counts"][1:].sum()) == len(p), what
                    if again is None:
                        again = gpu_voxel(p, cfg["voxel"], extra=8, **kw)
                        for k in OUTS:
                            if got[k] is not None:
                                assert np.array_equal(bits(got[k]), bits(again[k])), (what, k, "second run")


@pytest.mark.parametrize("n", (1, 5, 257, 70001))
def test_sizes(n):
    rng = np.random.default_rng(2020 + n)
    p = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    a = rng.uniform(0, 1, (n, 4)).astype(np.float32)
    w = rng.integers(0, 4, n).astype(np.float32)
    m = (rng.uniform(0, 1, n) > 0.1).astype(np.uint8)
    voxel = 0.11 if n > 1000 else 0.9
    for mode in (R.MEAN, R.BEST):
        kw = dict(attr=a, n_attr=4, mask=m, weight=w if mode == R.BEST else None, origin=(0.05, 0.0, -0.05), axis_bits=8,
                  mode=mode)
        want = R.downsample(p, voxel, **kw)
        compare(gpu_voxel(p, voxel, extra=8, **kw), want, 4, (n, mode))


def test_head_scan_carries_into_the_second_chunk():
    """CARRY_N points in about 1.6 million voxels: the last tile's base and the voxel count come through the carry."""
    p = np.random.default_rng(2023).uniform(-4, 4, (CARRY_N, 3)).astype(np.float32)
    want = R.downsample(p, 0.05)
    assert want["counts"][0] > 2 ** 20 and want["counts"][1] == CARRY_N
    compare(gpu_voxel(p, 0.05, extra=8), want, 0, "second chunk")


def test_every_optional_output_may_be_absent():
    c = R.case("origin")
    cfg = c["cfg"][0]
    kw = dict(attr=c["attr"], n_attr=4, weight=c["weight"], origin=cfg["origin"], axis_bits=cfg["axis_bits"], mode=R.BEST)
    full = gpu_voxel(c["points"], cfg["voxel"], **kw)
    for k in OUTS[1:]:
        got = gpu_voxel(c["points"], cfg["voxel"], skip=(k,), **kw)
        for j in OUTS:
            if j != k:
                assert np.array_equal(bits(got[j]), bits(full[j])), (k, j)


def test_truncation_leaves_the_rows_beyond_capacity_alone():
    c = R.case("box_a")
    cfg = c["cfg"][1]
    for mode in (R.MEAN, R.BEST):
        want = R.run_cfg(c, cfg, mode)
        m = int(want["counts"][0])
        kw = dict(attr=c["attr"], n_attr=4, mask=c["mask"], weight=c["weight"] if mode == R.BEST else None, mode=mode)
        for cap in (1, m // 2, m - 1):
            # capacity + 8 rows, prefilled: rows at or beyond capacity keep the sentinel; counts[0] and
            # voxel_of are the true ones (compare checks both against the untruncated answer)
            compare(gpu_voxel(c["points"], cfg["voxel"], capacity=cap, extra=8, **kw), want, 4, (mode, cap), rows=cap)
        # an ample buffer: rows at or beyond n_voxels keep it
        compare(gpu_voxel(c["points"], cfg["voxel"], capacity=m + 100, extra=8, **kw), want, 4, (mode, "ample"))


def test_xform_from_the_uploaded_golden_fit():
    """The golden similarity, uploaded as the fp64 vector sr_pose_align writes (13 entries and its ate)."""
    c = R.case("xform")
    cfg = c["cfg"][0]
    fit = np.concatenate([c["S"], [0.25]])
    for mode in (R.MEAN, R.BEST):
        want = R.run_cfg(c, cfg, mode)
        assert want["counts"][2] == 5  # the points that overflow under the transform are skipped
        got = gpu_voxel(c["points"], cfg["voxel"], attr=c["attr"], n_attr=4, weight=c["weight"] if mode == R.BEST else None,
                        xform=fit, origin=cfg["origin"], axis_bits=cfg["axis_bits"], mode=mode, extra=8)
        compare(got, want, 4, ("xform", mode))


# ---------------------------------------------------------------- the Python layer
def quantile_element(c, q):
    """depth_eval.select_quantiles' rule: the ascending finite element max(ceil(q n) - 1, 0)."""
    s = np.sort(c[np.isfinite(c)])
    return s[max(int(np.ceil(q * len(s))) - 1, 0)]


@pytest.fixture(scope="module")
def dpt_views():
    """Result dicts as SailRecon.forward returns them, from the depth head at the g6_dpt_small configuration
    and three made-up cameras; and the same arrays on the host."""
    from goldens import DPT_SMALL, dpt_small_model_sd, load_npz
    from sailrecon_amd.utils.geometry import unproject_depth_map_to_point_map
    g = load_npz("g6_dpt_small.npz")
    m, sd = dpt_small_model_sd("depth")
    m.load_state_dict(sd)
    m = m.to(DEV)
    toks = {l: torch.from_numpy(g[f"tok_{l}"]).to(DEV) for l in DPT_SMALL["intermediate_layer_idx"]}
    images = torch.from_numpy(g["images"]).to(DEV)
    with torch.no_grad():
        depth, conf = m(toks, images=images, patch_start_idx=5, frames_chunk_size=2)
    s, h, w = depth.shape[1:4]
    rng = np.random.default_rng(7)
    ext = np.zeros((s, 3, 4), np.float32)
    for k in range(s):
        q, r = np.linalg.qr(np.eye(3) + 0.2 * rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        ext[k, :, :3], ext[k, :, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-0.3, 0.3, 3)
    intr = np.tile(np.float32([[w, 0, w / 2], [0, w, h / 2], [0, 0, 1]]), (s, 1, 1))
    pts = unproject_depth_map_to_point_map(depth.squeeze(0), torch.from_numpy(ext).to(DEV), torch.from_numpy(intr).to(DEV))
    views = [{"point_map_by_unprojection": pts[None][:, k], "dpt_cnf": conf[:, k], "images": images[:, k],
              "extrinsic": torch.from_numpy(ext[None][:, k]).to(DEV)} for k in range(s)]
    host = {"points": np.asarray(pts).reshape(s, -1, 3).astype(np.float32), "conf": conf[0].reshape(s, -1).cpu().numpy(),
            "rgb": images[0].reshape(s, 3, -1).permute(0, 2, 1).cpu().numpy(), "ext": ext}
    return views, host


@pytest.mark.parametrize("mode", (R.MEAN, R.BEST))
@pytest.mark.parametrize("q", (0.0, 0.5))
def test_scene_cloud_equals_the_restatement(dpt_views, q, mode):
    from sailrecon_amd.utils.cloud_export import scene_cloud
    views, host = dpt_views
    extent = host["points"].reshape(-1, 3).max(0) - host["points"].reshape(-1, 3).min(0)
    voxel = float(extent.max()) / 24
    got = scene_cloud(views, conf_quantile=q, voxel=voxel, mode=mode)
    keep = np.concatenate([c >= quantile_element(c, q) for c in host["conf"]])
    p, c = host["points"].reshape(-1, 3), host["conf"].reshape(-1)
    attr = np.concatenate([host["rgb"].reshape(-1, 3), c[:, None]], axis=1)
    want = R.downsample(p, voxel, attr=attr, mask=keep.astype(np.uint8), weight=c if mode == R.BEST else None, mode=mode)
    assert got["n_voxels"] == want["counts"][0] > 1 and got["n_considered"] == want["counts"][1] == keep.sum()
    assert q == 0.0 or 0.45 * len(keep) < keep.sum() < 0.6 * len(keep)
    for k, w in (("points", want["points"]), ("attrs", want["attr"]), ("colors", want["attr"][:, :3]), ("conf", want["attr"][:, 3])):
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(w)), (k, q, mode)
    for k in ("count", "index"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k]), k
    assert np.array_equal(got["key"].cpu().numpy().view(np.uint64), want["key"])
    only = scene_cloud(views, conf_quantile=q, conf_thresh=float(np.median(c)))
    ok = keep & (c > float(np.median(c))) & np.isfinite(p).all(1)
    assert only["n_points"] == ok.sum() and np.array_equal(bits(only["points"].cpu().numpy()), bits(p[ok]))


def test_voxel_downsample_reports_truncation_and_the_inverse():
    from sailrecon_amd.utils.cloud_export import voxel_downsample
    c = R.case("origin")
    cfg = c["cfg"][0]
    kw = dict(attrs=c["attr"], origin=cfg["origin"], axis_bits=cfg["axis_bits"])
    want = R.run_cfg(c, cfg, R.MEAN)
    got = voxel_downsample(c["points"].reshape(30, 50, 3), cfg["voxel"], attrs=c["attr"].reshape(30, 50, 4),
                           origin=cfg["origin"], axis_bits=cfg["axis_bits"], return_inverse=True)
    assert got["points"].is_cuda and np.array_equal(bits(got["points"].cpu().numpy()), bits(want["points"]))
    assert np.array_equal(got["inverse"].cpu().numpy().astype(np.int64), want["voxel_of"])
    assert [got[k] for k in ("n_voxels", "n_considered", "n_skipped", "n_outside")] == want["counts"].tolist()
    with pytest.raises(ValueError, match="capacity"):
        voxel_downsample(c["points"], cfg["voxel"], capacity=int(want["counts"][0]) - 1, **kw)
    from sailrecon_amd._lib import SfmAmdError
    with pytest.raises(SfmAmdError, match="SR_VOXEL_BEST only"):
        voxel_downsample(c["points"], cfg["voxel"], weight=c["weight"], **kw)


def test_evaluate_reconstruction_with_voxel_scores_the_downsampled_clouds(dpt_views):
    """evaluate_reconstruction(voxel=v) = cloud_accuracy of the restatement's two downsampled clouds: the
    ground truth in its frame, the prediction under the fit the call reports."""
    import cloud_eval_ref as CE
    from sailrecon_amd.utils.cloud_eval import cloud_accuracy, evaluate_reconstruction
    views, host = dpt_views
    S = CE.sim3(np.random.default_rng(9), 1.3)
    pred = host["points"].reshape(-1, 3)
    gt = CE.xform_points(pred, S)[::2]
    # ground-truth poses: the predicted cameras moved by S (centres s R c + t, rotations R_pred R^T)
    s, Rm, t = S[0], S[1:10].reshape(3, 3), S[10:13]
    gt_ext = []
    for e in host["ext"].astype(np.float64):
        centre = -e[:, :3].T @ e[:, 3]
        rg = e[:, :3] @ Rm.T
        gt_ext.append(np.concatenate([rg, (-rg @ (s * Rm @ centre + t))[:, None]], axis=1))
    gt_ext = np.stack(gt_ext).astype(np.float32)
    extent = float((gt.max(0) - gt.min(0)).max())
    voxel = extent / 20
    kw = dict(thresholds=(voxel,), bin_len=voxel / 8, n_bins=256)
    res = evaluate_reconstruction(views, gt, gt_poses=gt_ext, voxel=voxel, **kw)
    plain = evaluate_reconstruction(views, gt, gt_poses=gt_ext, **kw)
    assert "n_pred_voxels" not in plain and plain["n_pred"] == len(pred) and plain["scale"] == res["scale"]
    fit = np.concatenate([[res["scale"]], res["R"].reshape(-1), res["t"]])
    assert abs(res["scale"] - 1.3) < 1e-3 and res["status"] == 0
    p_ds, g_ds = R.downsample(pred, voxel, xform=fit), R.downsample(gt, voxel)
    assert res["n_pred_voxels"] == p_ds["counts"][0] == res["n_pred"] and res["n_gt_voxels"] == g_ds["counts"][0] == res["n_gt"]
    assert 1 < res["n_pred_voxels"] < len(pred) / 4
    want = cloud_accuracy(p_ds["points"], g_ds["points"], **kw)
    for k, v in want.items():
        assert np.array_equal(res[k], v), k
    same = cloud_accuracy(pred, gt, xform=fit, voxel=voxel, **kw)
    for k, v in want.items():
        assert np.array_equal(same[k], v), k


def test_demo_writes_the_filtered_cloud(tmp_path):
    """The demo at a small image size with --voxel: pred_filtered.ply holds scene_cloud's vertices and
    colours, scene_info.txt gains its line, and the three usual outputs are byte for byte those of a run
    without the flag."""
    import cloud_eval as tool
    import demo_imc_forward as D
    from sailrecon_amd.utils.cloud_export import scene_cloud
    model = D.load_model(None, "cuda", img_size=224)
    outs = {}
    for name, kw in (("plain", {}), ("voxel", dict(voxel=0.05, conf_quantile=0.25, voxel_mode="best"))):
        model.aggregator.generator.manual_seed(0)
        res = D.demo(model=model, num_images=2, max_scenes=1, out_dir=str(tmp_path / name), img_size=224, verbose=False, **kw)
        outs[name] = tmp_path / name / "scene_000_scene000_"
    assert sorted(p.name for p in outs["plain"].iterdir()) == ["pred.ply", "pred.txt", "scene_info.txt"]
    assert sorted(p.name for p in outs["voxel"].iterdir()) == ["pred.ply", "pred.txt", "pred_filtered.ply", "scene_info.txt"]
    for f in ("pred.ply", "pred.txt"):
        assert (outs["plain"] / f).read_bytes() == (outs["voxel"] / f).read_bytes(), f
    info, info_v = (outs["plain"] / "scene_info.txt").read_text(), (outs["voxel"] / "scene_info.txt").read_text()
    cloud = scene_cloud(res[0], conf_quantile=0.25, voxel=0.05, mode="best")
    assert info_v == info + f"Filtered Points: {cloud['n_voxels']} (voxel 0.05, conf quantile 0.25, best)\n"
    assert 0 < cloud["n_voxels"] <= cloud["n_considered"] <= 0.8 * 2 * 224 * 224
    raw = (outs["voxel"] / "pred_filtered.ply").read_bytes()
    assert np.array_equal(bits(tool.read_ply_xyz(str(outs["voxel"] / "pred_filtered.ply"))), bits(cloud["points"].cpu().numpy()))
    rec = np.frombuffer(raw.split(b"end_header\n", 1)[1],
                        dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    want = np.clip(cloud["colors"].cpu().numpy() * 255.0 + 0.5, 0, 255).astype(np.uint8)
    assert np.array_equal(np.stack([rec["r"], rec["g"], rec["b"]], 1), want)
