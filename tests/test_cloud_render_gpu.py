"""GPU checks of the point-cloud renderer (sr_cloud_render, sailrecon_amd/utils/cloud_render.py, ABI 1.15).
Every comparison with the numpy restatement (tests/cloud_render_ref.py) is bit for bit, depth by its bits.  The
sizes are the smallest at which the kernels can still go wrong: tails of the 256-point tiles and of the 64-lane
waves, an odd frame that is no multiple of any tile, more than one workgroup per view, several views."""

import os
import sys

import numpy as np
import pytest
import torch

import cloud_render_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W = R.HW
EXTRA = 5  # rows of every output beyond what the call may write
SENT32, SENTF = -7, -7.0


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _up(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def run(c, want=("depth", "index", "attr", "counts"), check=True):
    """One ops.cloud_render of the case dict ``c`` (render()'s arguments as numpy arrays; ``xform_dev`` a device
    vector instead of ``xform``) into outputs with EXTRA sentinel rows; compared with the restatement bit for
    bit; the inputs must come back unchanged.  Returns (device outputs, restatement)."""
    from sailrecon_amd import ops
    c = dict(c)
    hw = c.pop("hw", R.HW)
    c.pop("kinds", None)
    pts, E, K = c.pop("points"), c.pop("extrinsic"), c.pop("intrinsic")
    xf_dev = c.pop("xform_dev", None)
    if xf_dev is not None:
        c["xform"] = xf_dev.cpu().numpy()[:13]
    V, n = len(E), len(pts)
    pix = V * hw[0] * hw[1]
    attr = c.get("attr")
    ca = 0 if attr is None else (c.get("n_attr") or attr.shape[1])
    ins = {"points": _up(pts), "extrinsic": _up(E), "intrinsic": _up(K), "attr": _up(attr), "mask": _up(c.get("mask")),
           "view_id": _up(c.get("view_id")), "exclude": _up(c.get("exclude")),
           "xform": xf_dev if xf_dev is not None else _up(c.get("xform"), torch.float64)}
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    out = {"depth": torch.full((pix + EXTRA,), SENTF, device=DEV) if "depth" in want else None,
           "index": torch.full((pix + EXTRA,), SENT32, device=DEV, dtype=torch.int32) if "index" in want else None,
           "attr": torch.full((pix * ca + EXTRA,), SENTF, device=DEV) if "attr" in want and ca else None,
           "counts": torch.full((4 * V + EXTRA,), SENT32, device=DEV, dtype=torch.int32) if "counts" in want else None}
    ops.cloud_render(ins["points"], ins["extrinsic"], ins["intrinsic"], hw, attr=ins["attr"] if out["attr"] is not None else None,
                     n_attr=ca if out["attr"] is not None else None, mask=ins["mask"], view_id=ins["view_id"],
                     exclude=ins["exclude"], xform=ins["xform"], radius=c.get("radius", 0), z_near=c.get("z_near", 1e-6),
                     z_far=c.get("z_far", float("inf")), attr_fill=c.get("attr_fill", float("nan")), depth=out["depth"],
                     index=out["index"], out_attr=out["attr"], counts=out["counts"])
    torch.cuda.synchronize()
    ref = R.render(pts, E, K, hw, **c)
    if check:
        for k, v in before.items():
            assert torch.equal(ins[k].view(torch.uint8), v.view(torch.uint8)), f"input {k} was written"
        if out["depth"] is not None:
            assert np.array_equal(_bits(out["depth"][:pix]), ref["depth"].reshape(-1)), "depth"
            assert (out["depth"][pix:] == SENTF).all()
        if out["index"] is not None:
            assert np.array_equal(out["index"][:pix].cpu().numpy(), ref["index"].reshape(-1)), "index"
            assert (out["index"][pix:] == SENT32).all()
        if out["attr"] is not None:
            assert np.array_equal(_bits(out["attr"][:pix * ca]), ref["attr"].reshape(-1)), "attr"
            assert (out["attr"][pix * ca:] == SENTF).all()
        if out["counts"] is not None:
            assert np.array_equal(_bits(out["counts"][:4 * V]), ref["counts"].reshape(-1)), "counts"
            assert (out["counts"][4 * V:] == SENT32).all()
    return out, ref


# ---------------------------------------------------------------- grid and tails
@pytest.mark.parametrize("V", (1, 3))
def test_sizes_and_tails(V):
    for n in R.GRID_N:
        c = R.gen_case("grid", n, V)
        rng = np.random.default_rng(n)
        c["attr"] = rng.standard_normal((n, 3)).astype(np.float32)
        out, ref = run(c)
        assert n < 2049 or ref["counts"][:, 0].min() > 0  # something is drawn


def test_each_output_may_be_absent():
    c = R.gen_case("full", 2049, 3)
    every = ("depth", "index", "attr", "counts")
    run(c, every)
    for gone in every:
        run(c, tuple(k for k in every if k != gone))
    for only in ("depth", "index", "counts"):
        run(c, (only,))


def test_a_second_run_gives_the_same_bits():
    c = R.gen_case("full", 70001, 3)
    a, ref = run(c)
    b, _ = run(c, check=False)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert (ref["counts"][:, 1] > 5000).all() and (ref["skipped"] > 5000).all()


# ---------------------------------------------------------------- classes, borders, ties
def test_every_class_of_point():
    c = R.gen_case("classes", 2049, 3)
    out, ref = run(c)
    kinds = c["kinds"]
    want = np.array([R.SKIPPED, R.SKIPPED, R.CLIPPED, R.CLIPPED, R.CLIPPED, R.OUTSIDE, R.DRAWN])[kinds]
    got = out["counts"][:12].cpu().numpy().reshape(3, 4)
    assert (got[:, 1:] == [(want == s).sum() for s in (R.DRAWN, R.CLIPPED, R.OUTSIDE)]).all()
    assert all((kinds == k).sum() > 100 for k in range(7))
    # u just below -0.5 and at W - 0.5 are outside, u just below W - 0.5 and at -0.5 are columns W - 1 and 0
    drawn = np.nonzero(kinds == 6)[0][:8]
    pr = R.project(c["points"], c["extrinsic"], c["intrinsic"], R.HW, mask=c["mask"], z_near=1.0, z_far=8.0)
    assert (ref["state"][0, drawn] == R.DRAWN).all()
    assert (pr["ix"][0, drawn[:4]] == W - 1).all() and (pr["ix"][0, drawn[4:]] == 0).all()
    assert (pr["uv"][0, drawn[:4], 0] < W - 0.5).all() and (pr["uv"][0, drawn[4:], 0] == -0.5).all()
    out_x = pr["uv"][0, kinds == 5, 0]
    assert ((out_x < -0.5) & (out_x > -0.51)).any() and (out_x == W - 0.5).any()


@pytest.mark.parametrize("radius", (0, 1, 3))
def test_footprints_at_borders_and_corners(radius):
    E = np.zeros((2, 3, 4), np.float32)
    E[:, :, :3] = np.eye(3)
    E[1, 0, 3] = 0.25  # the second view sees everything shifted by 4 pixels at depth 2
    K = np.tile(np.float32([[32, 0, 26], [0, 32, 18], [0, 0, 1]]), (2, 1, 1))
    px = [(x, y) for x in (0, 1, 26, W - 2, W - 1) for y in (0, 1, 18, H - 2, H - 1)]
    p = np.float32([[(x - 26) * 2 / 32, (y - 18) * 2 / 32, 2] for x, y in px])
    out, ref = run({"points": p, "extrinsic": E, "intrinsic": K, "radius": radius,
                    "attr": np.arange(len(p), dtype=np.float32).reshape(-1, 1).copy(), "attr_fill": 0.0})
    assert ref["counts"][0, 1] == len(p) and ref["counts"][1, 3] == 10  # x = W - 2 and W - 1 leave the second view
    if radius == 0:
        assert ref["counts"][0, 0] == len(p)
    assert (ref["index"][0, :radius + 1, :radius + 1] == 0).all()  # the corner's clipped footprint
    # one attribute column whose stride says nothing (numpy's x[:, None]) goes through the Python layer
    from sailrecon_amd.utils.cloud_render import render_cloud
    r = render_cloud(p, E, K, (H, W), attrs=np.arange(len(p), dtype=np.float32)[:, None], radius=radius, attr_fill=0.0)
    assert np.array_equal(_bits(r["attrs"]), ref["attr"]) and np.array_equal(_bits(r["counts"]), ref["counts"])


def test_a_duplicated_cloud_gives_the_lowest_index():
    c = R.gen_case("grid", 2049, 3)
    c["points"] = np.concatenate([c["points"], c["points"]])
    c["radius"] = 1
    out, ref = run(c)
    assert (out["index"][:3 * H * W] < 2049).all() and (ref["index"] >= 0).any()


def test_one_pixel_under_contention():
    """100,000 points that all project to one pixel: the nearest wins, equal depths go to the lowest index."""
    n = 100_000
    rng = np.random.default_rng(5)
    E = np.zeros((1, 3, 4), np.float32)
    E[0, :, :3] = np.eye(3)
    K = np.float32([[[32, 0, 26], [0, 32, 18], [0, 0, 1]]])
    z = rng.uniform(2, 4, n).astype(np.float32)
    nearest = np.float32(1.5)
    where = rng.choice(n, 7, replace=False)
    z[where] = nearest
    p = np.stack([np.zeros(n, np.float32), np.zeros(n, np.float32), z], axis=1)
    out, ref = run({"points": p, "extrinsic": E, "intrinsic": K, "attr": z[:, None].copy()})
    assert ref["counts"].tolist() == [[1, n, 0, 0]]
    assert int(out["index"][18 * W + 26]) == where.min() and float(out["depth"][18 * W + 26]) == 1.5
    out, ref = run({"points": p, "extrinsic": E, "intrinsic": K, "radius": 3})
    assert ref["counts"].tolist() == [[49, n, 0, 0]] and (out["index"][:H * W] >= 0).sum() == 49


def test_view_exclusion():
    n, V = 2049, 3
    c = R.gen_case("grid", n, V)
    c["view_id"] = (np.arange(n) % 4).astype(np.int32)
    c["exclude"] = np.int32([2, 0, 9])
    out, ref = run(c)
    plain = R.render(c["points"], c["extrinsic"], c["intrinsic"], R.HW)
    idx = out["index"][:V * H * W].cpu().numpy().reshape(V, H, W)
    for v, e in enumerate(c["exclude"]):
        assert not (idx[v][idx[v] >= 0] % 4 == e).any()
        gone = ((plain["state"][v] == R.DRAWN) & (c["view_id"] == e)).sum()
        assert ref["counts"][v, 1] == plain["counts"][v, 1] - gone and (gone > 0) == (e < 4)


def test_xform_from_pose_align_as_it_lies():
    """The similarity sr_pose_align writes, handed over on the device as it lies (14 entries, the last its ate)."""
    from sailrecon_amd import ops
    rng = np.random.default_rng(9)
    pred, _ = R.cameras(rng, 6, spread=1.0)
    s, Rs, ts = 1.07, R.rotation(rng.normal(0, 0.08, 3)), rng.uniform(-0.1, 0.1, 3)
    gt = np.zeros_like(pred)
    for k in range(len(pred)):
        Rk, tk = pred[k, :, :3].astype(np.float64), pred[k, :, 3].astype(np.float64)
        centre = s * Rs @ (-Rk.T @ tk) + ts
        gt[k, :, :3] = Rk @ Rs.T
        gt[k, :, 3] = -(Rk @ Rs.T) @ centre
    fit = torch.empty(14, device=DEV, dtype=torch.float64)
    status = torch.empty(1, device=DEV, dtype=torch.int32)
    ops.pose_align(_up(pred), _up(gt), fit, status)
    assert int(status) == 0 and abs(float(fit[0]) - s) < 1e-3
    for n in (257, 2049):
        c = R.gen_case("grid", n, 3)
        c["xform_dev"] = fit
        out, ref = run(c)
        plain = R.render(c["points"], c["extrinsic"], c["intrinsic"], R.HW)
        assert ref["counts"][:, 1].min() > 0 and not np.array_equal(ref["index"], plain["index"])
    # a transform that sends points to infinity: they are skipped, not drawn
    wild = fit.clone()
    wild[0] = 1e300
    c = R.gen_case("grid", 257, 3)
    c["xform_dev"] = wild
    out, ref = run(c)
    assert ref["counts"][:, 1:].sum() == 0 and (ref["skipped"] == 257).all()


@pytest.mark.parametrize("n_attr", (0, 1, 4, 8))
def test_attribute_columns(n_attr):
    n = 2049
    c = R.gen_case("grid", n, 3)
    c["radius"] = 1
    if n_attr:
        a = np.random.default_rng(n_attr).standard_normal((n, n_attr + 3)).astype(np.float32)
        a[::7, 0] = np.uint32(0x7fc01234).view(np.float32)  # a payload that a float move may not keep
        a[::11, -1] = np.nan  # beyond n_attr: never read
        c["attr"], c["n_attr"], c["attr_fill"] = a, n_attr, np.uint32(0xffc00001).view(np.float32)
    out, ref = run(c)
    if n_attr:
        assert (ref["attr"] == 0x7fc01234).any()


# ---------------------------------------------------------------- round trip, golden, Python layers
def test_round_trip_through_unproject():
    """A view's own fp32-unprojected points at radius 0 come back as index == arange(H W) exactly, and the depth
    within 1e-5 z (a sanity bound, about 20 x what a CPU run of the same arithmetic gave; the bit-for-bit tests
    are the contract)."""
    from sailrecon_amd.utils.cloud_render import render_cloud
    from sailrecon_amd.utils.geometry import unproject_depth_points
    rng = np.random.default_rng(3)
    V = 3
    E, K = R.cameras(rng, V, spread=2.0, turn=0.4)  # |world| up to about 8
    depth = rng.uniform(2, 4, (V, H, W)).astype(np.float32)
    pts = unproject_depth_points(_up(depth), _up(E), _up(K))
    assert float(pts.abs().max()) < 8
    for v in range(V):
        r = render_cloud(pts[v], E[v], K[v], (H, W))
        assert torch.equal(r["index"][0].reshape(-1).cpu(), torch.arange(H * W, dtype=torch.int32))
        dz = (r["depth"][0].cpu().numpy().astype(np.float64) - depth[v]) / depth[v]
        print(f"view {v}: max |dz| / z = {np.abs(dz).max():.3e}")
        assert np.abs(dz).max() <= 1e-5
        assert r["coverage"][0] == {"covered": H * W, "drawn": H * W, "clipped": 0, "outside": 0, "skipped": 0, "fraction": 1.0}


def test_golden_file():
    with np.load(R.GOLDEN, allow_pickle=False) as g:
        g = {k: g[k] for k in g.files}
    for r in (0, 1):
        out, ref = run({"points": g["points"], "extrinsic": g["extrinsic"], "intrinsic": g["intrinsic"], "radius": r,
                        "z_near": float(g["z_near"]), "z_far": float(g["z_far"])})
        V = 3
        assert np.array_equal(_bits(out["depth"][:V * H * W]), g[f"r{r}/depth"].reshape(-1))
        assert np.array_equal(out["index"][:V * H * W].cpu().numpy(), g[f"r{r}/index"].reshape(-1))
        assert np.array_equal(_bits(out["counts"][:4 * V]), g[f"r{r}/counts"].reshape(-1))
    # the drawn pixels are where the reference's projection puts them
    img = g["ref/image_points"]
    idx = g["r0/index"]
    for v in range(3):
        ys, xs = np.nonzero(idx[v] >= 0)
        i = idx[v][ys, xs]
        assert (np.floor(img[v, i, 0] + 0.5) == xs).all() and (np.floor(img[v, i, 1] + 0.5) == ys).all()


def _plane_scene():
    """Three identity-rotation cameras translated in x and y that look at the world plane z = 3: every view's
    depth of every point is 3.  Result dicts as SailRecon.forward returns them, on the device."""
    from sailrecon_amd.utils.geometry import unproject_depth_points
    V = 3
    E = np.zeros((V, 3, 4), np.float32)
    E[:, :, :3] = np.eye(3)
    E[:, 0, 3], E[:, 1, 3] = [0.0, 0.375, -0.1875], [0.0, -0.09375, 0.28125]  # whole pixels at f = 32, z = 3: 4, -1, ...
    K = np.tile(np.float32([[32, 0, 26], [0, 32, 18], [0, 0, 1]]), (V, 1, 1))
    depth = np.full((V, H, W), 3.0, np.float32)
    rng = np.random.default_rng(4)
    conf = rng.uniform(1, 2, (V, H, W)).astype(np.float32)
    images = rng.uniform(0, 1, (V, 3, H, W)).astype(np.float32)
    pts = unproject_depth_points(_up(depth), _up(E), _up(K))
    views = [{"extrinsic": _up(E[v:v + 1]), "intrinsic": _up(K[v:v + 1]), "depth_map": _up(depth[v:v + 1, :, :, None]),
              "dpt_cnf": _up(conf[v:v + 1]), "images": _up(images[v:v + 1]),
              "point_map_by_unprojection": pts[v:v + 1].cpu().numpy().astype(np.float64)} for v in range(V)]
    return views, {"E": E, "K": K, "depth": depth, "conf": conf, "images": images, "points": pts.cpu().numpy()}


def test_cross_view_consistency_on_a_plane():
    from sailrecon_amd.utils.cloud_render import cross_view_consistency, render_predictions
    from sailrecon_amd.utils.conf_eval import sparsification_curves
    views, host = _plane_scene()
    V, n = 3, H * W
    r = cross_view_consistency(views)
    flat = host["points"].reshape(V * n, 3)
    vid = np.repeat(np.arange(V, dtype=np.int32), n)
    attrs = np.concatenate([host["images"].reshape(V, 3, n).transpose(0, 2, 1).reshape(V * n, 3),
                            host["conf"].reshape(V * n, 1)], axis=1)
    ref = R.render(flat, host["E"], host["K"], (H, W), attr=attrs, view_id=vid, exclude=np.arange(V, dtype=np.int32))
    assert np.array_equal(_bits(r["rendered"]), ref["depth"])
    assert np.array_equal(_bits(r["render"]["attrs"]), ref["attr"])
    assert np.array_equal(r["render"]["index"].cpu().numpy(), ref["index"])
    print("pooled abs_rel", r["pooled"]["abs_rel"], "coverage", r["coverage"])
    assert r["pooled"]["abs_rel"] <= 1e-6 and r["pooled"]["n_valid"] == int(ref["counts"][:, 0].sum())
    want = ref["counts"][:, 0] / float(n)
    assert np.array_equal(r["coverage"], want) and (want > 0.5).all() and (want < 1).all()
    assert [c["covered"] for c in r["render"]["coverage"]] == ref["counts"][:, 0].tolist()
    rel = r["rel_err"].cpu().numpy()
    assert (np.isnan(rel) == (ref["index"] < 0)).all() and np.nanmax(rel) <= 1e-6
    assert torch.equal(r["conf"].cpu(), torch.from_numpy(host["conf"]))
    curves = sparsification_curves(r["rel_err"], r["conf"])  # unchanged, as the docstring says
    assert curves["curve"].shape[0] == V
    # without exclusion the first view shows its own points: all depths are equal and its indices the lowest
    own = render_predictions(views, cross=False)
    assert torch.equal(own["index"][0].cpu().reshape(-1), torch.arange(n, dtype=torch.int32))
    plain = R.render(flat, host["E"], host["K"], (H, W), attr=attrs)
    assert np.array_equal(own["index"].cpu().numpy(), plain["index"]) and np.array_equal(_bits(own["conf"]), plain["attr"][..., 3])


def test_rejections_surface_as_errors():
    from sailrecon_amd import ops
    from sailrecon_amd._lib import SfmAmdError
    c = R.gen_case("grid", 65, 1)
    p, E, K = _up(c["points"]), _up(c["extrinsic"]), _up(c["intrinsic"])
    depth = torch.empty(H * W, device=DEV)
    with pytest.raises(SfmAmdError, match="radius 4 outside"):
        ops.cloud_render(p, E, K, R.HW, radius=4, depth=depth)
    with pytest.raises(SfmAmdError, match="z_near must be positive"):
        ops.cloud_render(p, E, K, R.HW, z_near=0.0, depth=depth)
    with pytest.raises(SfmAmdError, match="no output"):
        ops.cloud_render(p, E, K, R.HW)


def test_tool_renders_a_ply(tmp_path, capsys):
    """tools/render_cloud.py on a PLY and a pose file as the demo writes them: the arrays it saves are the
    restatement's, the colours those of the file."""
    import json

    import render_cloud as tool
    from pose_eval import load_kitti_w2c
    from sailrecon_amd.utils.cloud_export import save_ply
    rng = np.random.default_rng(6)
    c = R.gen_case("grid", 2049, 1)
    p = c["points"][np.isfinite(c["points"]).all(axis=1)]
    rgb = rng.uniform(0, 1, (len(p), 3)).astype(np.float32)
    ply, poses, out = str(tmp_path / "c.ply"), str(tmp_path / "p.txt"), str(tmp_path / "o")
    save_ply(ply, p, rgb)
    with open(poses, "w") as f:  # camera to world, KITTI: identity rotations, exact translations
        for t in ((0.0, 0.0, 0.0), (0.25, -0.125, 0.5)):
            f.write(" ".join(f"{v:.9e}" for v in (1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, t[2])) + "\n")
    res = tool.main([ply, poses, "--intrinsics", "40,41,26,18", "--size", str(H), str(W), "--radius", "1", "--out", out])
    E = load_kitti_w2c(poses)[:, :3, :]
    K = np.tile(np.float32([[40, 0, 26], [0, 41, 18], [0, 0, 1]]), (2, 1, 1))
    a8 = np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8).astype(np.float32) / np.float32(255)
    ref = R.render(p, E, K, (H, W), attr=a8, radius=1)
    assert np.array_equal(np.load(os.path.join(out, "depth.npy")).view(np.uint32), ref["depth"])
    assert np.array_equal(np.load(os.path.join(out, "index.npy")), ref["index"])
    assert np.array_equal(np.load(os.path.join(out, "color.npy")).view(np.uint32), ref["attr"])
    lines = [json.loads(l[len("counts "):]) for l in capsys.readouterr().out.splitlines() if l.startswith("counts ")]
    assert [(l["view"], l["covered"], l["drawn"], l["clipped"], l["outside"]) for l in lines] == \
        [(v, *ref["counts"][v].tolist()) for v in range(2)]
    assert ref["counts"][:, 1].min() > 100 and res["coverage"][1]["skipped"] == 0
    vox = tool.main([ply, poses, "--intrinsics", "40,41,26,18", "--size", str(H), str(W), "--voxel", "1.0", "--out", out])
    assert 0 < vox["coverage"][0]["drawn"] < ref["counts"][0, 1]
