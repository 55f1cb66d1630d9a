"""CPU checks of the point-cloud renderer (ABI 1.15): the restatement's planted answers, every rejection of
sr_cloud_render through the bindings, the workspace, the ctypes layout, the projection mirror and the restatement
against the golden file, and the tool's arguments."""

import ctypes
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import cloud_render_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_15 = (1 << 16) | 15
NEW = ("sr_cloud_render_workspace", "sr_cloud_render")


@pytest.fixture(autouse=True, scope="module")
def abi_1_15():
    """Everything here is about the library that has the renderer."""
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_15
    assert all(s in _lib.EXPORTED for s in NEW)


# ---------------------------------------------------------------- ABI
def _header_fields(struct):
    src = open(os.path.join(REPO, "include", "sfm_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    names = []
    for line in body.splitlines():
        decl = line.split("/*")[0].strip()
        for stmt in filter(None, (s.strip() for s in decl.split(";"))):
            first, *rest = stmt.split(",")
            names += [first.split()[-1]] + [r.strip() for r in rest]
    return [n.lstrip("*").split("[")[0] for n in names]


def test_version_and_exports():
    from sailrecon_amd import _lib, ops
    assert _header_fields("sr_cloud_render_desc") == [f[0] for f in _lib.CloudRenderDesc._fields_]
    src = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "sr_api.hip")).read()
    assert "1.15: sr_cloud_render" in src
    assert (_lib.SR_RENDER_MAX_ATTR, _lib.SR_RENDER_MAX_RADIUS) == (8, 3)
    assert callable(ops.cloud_render) and callable(ops.cloud_render_workspace_bytes)
    mk = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "Makefile")).read()
    assert "sr_cloud_render.hip" in mk
    for obj in ("$(BUILD)/sr_cloud_render.o", "$(BUILD)/debug/sr_cloud_render.o"):
        assert re.search(re.escape(obj) + r": \w+ \+= -ffp-contract=off -fhonor-nans", mk), obj


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "cloud_render"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    assert set(lay) == {"sr_cloud_render_desc"}
    c, cls = lay["sr_cloud_render_desc"], _lib.CloudRenderDesc
    assert ctypes.sizeof(cls) == c["size"]
    assert {f[0] for f in cls._fields_} == set(c["fields"])
    for f, off in c["fields"].items():
        assert getattr(cls, f).offset == off, f


N, VIEWS, H, W = 70001, 3, 37, 53
A = 0x7f0000000000  # fake, suitably aligned device addresses: validation never dereferences them


def _desc(**kw):
    from sailrecon_amd import _lib
    d = _lib.CloudRenderDesc()
    (d.points, d.attr, d.mask, d.view_id, d.exclude, d.xform, d.extrinsic, d.intrinsic, d.depth, d.index, d.out_attr,
     d.counts, d.workspace) = (A + (i << 24) for i in range(1, 14))
    d.n, d.ldp, d.lda, d.n_attr, d.n_views, d.height, d.width, d.radius = N, 3, 5, 4, VIEWS, H, W, 1
    d.z_near, d.z_far, d.attr_fill = 1e-6, float("inf"), 0.5
    d.workspace_bytes = _lib.load().sr_cloud_render_workspace(VIEWS, H, W)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(descs):
    """Each call through the bindings' ``check`` on a thread of its own (sr_last_error is per thread, and
    test_abi.py expects the main thread's to be empty): the SfmAmdError text, or 0 for a call that passed."""
    from sailrecon_amd import _lib
    lib, got = _lib.load(), []

    def work():
        for d in descs:
            try:
                _lib.check(lib.sr_cloud_render(None, ctypes.byref(d) if d is not None else None), "sr_cloud_render")
                got.append(0)
            except _lib.SfmAmdError as e:
                got.append(str(e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_render_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    ws = _lib.load().sr_cloud_render_workspace
    need, huge, nan, inf = ws(VIEWS, H, W), 2 ** 50, float("nan"), float("inf")
    no_out = dict(depth=None, index=None, counts=None)
    bad = {
        "null desc": None, "null points": _desc(points=None), "null extrinsic": _desc(extrinsic=None),
        "null intrinsic": _desc(intrinsic=None), "null workspace": _desc(workspace=None), "n 0": _desc(n=0), "n -1": _desc(n=-1),
        "n 2^31": _desc(n=2 ** 31), "ldp 2": _desc(ldp=2), "n_attr -1": _desc(n_attr=-1), "n_attr 9": _desc(n_attr=9, lda=9),
        "n_attr without attr": _desc(attr=None), "n_attr without out_attr": _desc(out_attr=None), "lda < n_attr": _desc(lda=3),
        "view_id alone": _desc(exclude=None), "exclude alone": _desc(view_id=None), "n_views 0": _desc(n_views=0),
        "n_views -2": _desc(n_views=-2), "n_views 65536": _desc(n_views=65536, height=1, width=1, workspace_bytes=huge),
        "height 0": _desc(height=0), "width 0": _desc(width=0), "width -4": _desc(width=-4),
        "2^31 pixels": _desc(n_views=2, height=2 ** 15, width=2 ** 15, workspace_bytes=huge),
        "a product that overflows": _desc(n_views=65535, height=2 ** 31 - 1, width=2 ** 31 - 1, workspace_bytes=huge),
        "radius -1": _desc(radius=-1), "radius 4": _desc(radius=4), "z_near 0": _desc(z_near=0.0), "z_near -1": _desc(z_near=-1.0),
        "z_near NaN": _desc(z_near=nan), "z_near Inf": _desc(z_near=inf), "z_far NaN": _desc(z_far=nan),
        "z_far < z_near": _desc(z_near=2.0, z_far=1.0), "no output": _desc(n_attr=0, attr=None, out_attr=None, **no_out),
        "no output, out_attr without columns": _desc(n_attr=0, **no_out),
        "workspace short": _desc(workspace_bytes=need - 1), "workspace % 16": _desc(workspace=A + (13 << 24) + 8),
        "xform % 8": _desc(xform=A + (6 << 24) + 4),
    }
    for what, msg in zip(bad, _call(list(bad.values()))):
        assert isinstance(msg, str) and "sr_cloud_render failed (-1): sr_cloud_render: " in msg, (what, msg)
    # what passes validation fails at the launch only (there is no device)
    ok = [_desc(), _desc(radius=0), _desc(radius=3), _desc(mask=None, view_id=None, exclude=None, xform=None),
          _desc(n_attr=0, attr=None, out_attr=None), _desc(n_attr=8, lda=8), _desc(z_far=1e-6), _desc(depth=None),
          _desc(index=None), _desc(counts=None), _desc(n_attr=0, attr=None, out_attr=None, depth=None, index=None),
          _desc(depth=None, index=None, counts=None), _desc(n=1), _desc(n=2 ** 31 - 1, ldp=7),
          _desc(n_views=65535, height=1, width=1, workspace_bytes=huge),
          _desc(n_views=1, height=1, width=2 ** 31 - 1, workspace_bytes=huge)]
    for msg in _call(ok):
        assert isinstance(msg, str) and "sr_cloud_render failed (-2)" in msg, msg


def test_workspace_never_shrinks():
    from sailrecon_amd import _lib, ops
    ws = _lib.load().sr_cloud_render_workspace
    most = 2 ** 31 - 1
    for v in (1, 2, 3, 32, 65535):
        for h in (1, 2, 37, 518, 1024):
            for w in (1, 2, 53, 518, 2047):
                b = ws(v, h, w)
                if v * h * w > most:
                    assert b == 0, (v, h, w)
                    continue
                assert b > 0 and b % 16 == 0 and b >= 8 * v * h * w + 16 * v, (v, h, w)
                for v2, h2, w2 in ((v + 1, h, w), (v, h + 1, w), (v, h, w + 1)):
                    assert v2 > 65535 or v2 * h2 * w2 > most or ws(v2, h2, w2) >= b, (v, h, w)
    for args in ((0, 5, 5), (-1, 5, 5), (65536, 1, 1), (1, 0, 5), (1, 5, 0), (1, -3, 5), (1, 2 ** 16, 2 ** 15),
                 (2, 2 ** 15, 2 ** 15), (65535, most, most)):
        assert ws(*args) == 0 and ops.cloud_render_workspace_bytes(*args) == 0, args
    assert ops.cloud_render_workspace_bytes(1, 2 ** 40, 1) == 0
    assert ws(1, most, 1) > 0 and ws(1, 1, most) > 0 and ws(65535, 1, 1) > 0
    assert ops.cloud_render_workspace_bytes(32, 518, 518) == ws(32, 518, 518) == 8 * 32 * 518 * 518 + 16 * 32 * (1 + 64)


# ---------------------------------------------------------------- planted answers in the restatement
def _plane_cameras(V=1):
    E = np.zeros((V, 3, 4), np.float32)
    E[:, :, :3] = np.eye(3)
    K = np.tile(np.float32([[32, 0, 26], [0, 32, 18], [0, 0, 1]]), (V, 1, 1))
    return E, K


def _plane(z, step=1):
    """One point per ``step``-th pixel centre of the 37 x 53 frame of _plane_cameras, at depth z (exact in fp32)."""
    ys, xs = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    zf = np.float32(z)
    return np.stack([(xs - 26) * zf / 32, (ys - 18) * zf / 32, np.full(xs.shape, zf)], -1).reshape(-1, 3).astype(np.float32)


def test_a_near_plane_occludes_a_far_one():
    E, K = _plane_cameras()
    far, near = _plane(4.0), _plane(2.0, step=2)
    for order in (0, 1):
        p = np.concatenate([far, near] if order == 0 else [near, far])
        r = R.render(p, E, K, (H, W))
        from_near = (r["index"][0] >= len(far)) if order == 0 else (r["index"][0] < len(near))
        want = np.zeros((H, W), bool)
        want[::2, ::2] = True
        assert (from_near == want).all()
        assert (r["depth"][0].view(np.float32) == np.where(want, 2.0, 4.0)).all()
        assert r["counts"].tolist() == [[H * W, len(p), 0, 0]] and r["skipped"].tolist() == [0]
    # radius 1: the near plane's footprints close its gaps, apart from nothing at all (step 2 leaves none)
    r = R.render(np.concatenate([far, near]), E, K, (H, W), radius=1)
    assert (r["depth"][0].view(np.float32) == 2.0).all() and (r["index"][0] >= len(far)).all()


def test_a_duplicated_cloud_gives_the_lowest_index():
    c = R.gen_case("grid", 2049, 3)
    p = np.concatenate([c["points"], c["points"]])
    for radius in (0, 2):
        one = R.render(c["points"], c["extrinsic"], c["intrinsic"], R.HW, radius=radius)
        two = R.render(p, c["extrinsic"], c["intrinsic"], R.HW, radius=radius)
        assert (two["index"] < len(c["points"])).all() and np.array_equal(two["index"], one["index"])
        assert np.array_equal(two["depth"], one["depth"]) and (two["counts"][:, 1:] == 2 * one["counts"][:, 1:]).all()
        assert (two["counts"][:, 0] == one["counts"][:, 0]).all()


def test_footprints_at_the_frame_corners():
    E, K = _plane_cameras()
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    p = np.float32([[(x - 26) * 2 / 32, (y - 18) * 2 / 32, 2] for x, y in corners])
    for radius in range(4):
        r = R.render(p, E, K, (H, W), radius=radius, attr=np.float32([[1], [2], [3], [4]]), attr_fill=-1.0)
        assert r["counts"].tolist() == [[4 * (radius + 1) ** 2, 4, 0, 0]]
        a = r["attr"][0, :, :, 0].view(np.float32)
        for k, (x, y) in enumerate(corners):
            ys = slice(0, radius + 1) if y == 0 else slice(H - 1 - radius, H)
            xs = slice(0, radius + 1) if x == 0 else slice(W - 1 - radius, W)
            assert (r["index"][0, ys, xs] == k).all() and (a[ys, xs] == k + 1).all()
        assert ((r["index"][0] == -1) == (a == -1.0)).all() and (r["depth"][0][r["index"][0] == -1] == R.QNAN).all()


def test_every_class_of_point_is_counted():
    c = R.gen_case("classes", 2049, 3)
    r = R.render(c["points"], c["extrinsic"], c["intrinsic"], R.HW, mask=c["mask"], z_near=1.0, z_far=8.0)
    want = np.array([R.SKIPPED, R.SKIPPED, R.CLIPPED, R.CLIPPED, R.CLIPPED, R.OUTSIDE, R.DRAWN])[c["kinds"]]
    assert (r["state"] == want[None]).all() and all((c["kinds"] == k).any() for k in range(7))
    assert (r["counts"][:, 1:] == [(want == s).sum() for s in (R.DRAWN, R.CLIPPED, R.OUTSIDE)]).all()
    assert (r["skipped"] == (want == R.SKIPPED).sum()).all()
    # exclusion: view v loses exactly the drawn points of its own id
    vid = (np.arange(len(want)) % 4).astype(np.int32)
    x = R.render(c["points"], c["extrinsic"], c["intrinsic"], R.HW, mask=c["mask"], z_near=1.0, z_far=8.0, view_id=vid,
                 exclude=np.int32([0, 1, 7]))
    for v, e in enumerate((0, 1, 7)):
        assert x["counts"][v, 1] == ((want == R.DRAWN) & (vid != e)).sum()
        assert not np.isin(x["index"][v][x["index"][v] >= 0] % 4, [e]).any()


# ---------------------------------------------------------------- golden, mirror, tool
def _golden():
    with np.load(R.GOLDEN, allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def test_generator_reproduces_the_golden():
    z, g = R.build_golden(), _golden()
    assert sorted(g) == sorted(list(z) + ["ref/image_points", "ref/cam_points"])
    for k in z:
        assert g[k].dtype == z[k].dtype and g[k].shape == z[k].shape, k
        assert g[k].tobytes() == z[k].tobytes(), k
    assert os.path.getsize(R.GOLDEN) < 1 << 19
    assert len(g["points"]) == R.GOLDEN_N >= 2000 and g["extrinsic"].shape == (3, 3, 4) and tuple(g["hw"]) == (37, 53)


def test_restatement_agrees_with_the_reference_projection():
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_golden_cloud_render as M
    g = _golden()
    M.check_against(g, g["ref/image_points"], g["ref/cam_points"])


def test_projection_mirror_against_the_golden():
    import torch
    from sailrecon_amd.utils.geometry import img_from_cam, project_world_points_to_cam
    g = _golden()
    p, E, K = (torch.from_numpy(g[k]).double() for k in ("points", "extrinsic", "intrinsic"))
    img, cam = project_world_points_to_cam(p, E, K)
    assert tuple(img.shape) == (3, R.GOLDEN_N, 2) and tuple(cam.shape) == (3, 3, R.GOLDEN_N)
    assert np.abs(cam.numpy() - g["ref/cam_points"]).max() <= 1e-12
    live = (g["ref/cam_points"][:, 2] >= R.GOLDEN_NEAR) & (g["ref/cam_points"][:, 2] <= R.GOLDEN_FAR)
    assert np.abs(img.numpy() - g["ref/image_points"])[live].max() <= 1e-9
    ours, ref = np.floor(img.numpy()[live] + 0.5), np.floor(g["ref/image_points"][live] + 0.5)
    assert (ours == ref).all()
    none, cam2 = project_world_points_to_cam(p, E, only_points_cam=True)
    assert none is None and torch.equal(cam2, cam) and torch.equal(img_from_cam(K, cam), img)
    # a NaN becomes ``default``; fp32 in, fp32 out
    z = project_world_points_to_cam(torch.zeros(1, 3), E.float(), K.float(), default=-3)[0]
    assert z.dtype == torch.float32 and tuple(z.shape) == (3, 1, 2) and not torch.isnan(z).any()
    with pytest.raises(NotImplementedError):
        project_world_points_to_cam(p, E, K, distortion_params=torch.zeros(3, 1))
    with pytest.raises(NotImplementedError):
        img_from_cam(K, cam, torch.zeros(3, 2))


def test_python_layer_checks_its_arguments_before_the_device():
    import inspect
    from sailrecon_amd.utils import cloud_render
    sig = inspect.signature(cloud_render.render_cloud).parameters
    assert [sig[k].default for k in ("attrs", "valid", "view_id", "exclude", "radius", "z_near", "z_far", "xform")] == \
        [None, None, None, None, 0, 1e-6, float("inf"), None]
    assert np.isnan(sig["attr_fill"].default)
    sig = inspect.signature(cloud_render.render_predictions).parameters
    assert [sig[k].default for k in ("key", "conf_key", "conf_quantile", "cross", "radius")] == \
        ["point_map_by_unprojection", "dpt_cnf", 0.0, True, 0]
    sig = inspect.signature(cloud_render.cross_view_consistency).parameters
    assert (sig["key"].default, sig["depth_key"].default, sig["radius"].default) == ("point_map_by_unprojection", "depth_map", 0)
    assert "sparsification_curves(r[\"rel_err\"], r[\"conf\"])" in cloud_render.cross_view_consistency.__doc__
    p, E, K = np.zeros((5, 3), np.float32), np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 3), np.float32)
    for kw in (dict(radius=4), dict(radius=-1), dict(radius=1.5), dict(view_id=np.zeros(5, np.int32)),
               dict(exclude=np.zeros(2, np.int32))):
        with pytest.raises(ValueError):
            cloud_render.render_cloud(p, E, K, (4, 4), **kw)
    with pytest.raises(ValueError):
        cloud_render.render_predictions([])
    with pytest.raises(ValueError):
        cloud_render.cross_view_consistency([{"depth_map": p}], align="median")


def test_tool_argument_parsing(tmp_path):
    import render_cloud as tool
    a = tool.parse_args(["c.ply", "p.txt", "--intrinsics", "400,410,258.5,258.5", "--size", "518", "518"])
    assert (a.cloud, a.poses, a.size, a.radius, a.voxel, a.out) == ("c.ply", "p.txt", [518, 518], 0, None, "render_out")
    k = tool.load_intrinsics(a.intrinsics, 3)
    assert k.shape == (3, 3, 3) and k.dtype == np.float32 and k[2].tolist() == [[400, 0, 258.5], [0, 410, 258.5], [0, 0, 1]]
    kf = tmp_path / "K.txt"
    np.savetxt(kf, np.arange(18, dtype=np.float64).reshape(2, 9))
    a = tool.parse_args(["c.ply", "p.txt", "--intrinsics", str(kf), "--size", "37", "53", "--radius", "3", "--voxel", "0.02",
                         "--out", "o"])
    assert (a.size, a.radius, a.voxel, a.out) == ([37, 53], 3, 0.02, "o")
    assert tool.load_intrinsics(str(kf), 2)[1].reshape(-1).tolist() == list(range(9, 18))
    with pytest.raises(ValueError):
        tool.load_intrinsics(str(kf), 3)
    base = ["c.ply", "p.txt", "--intrinsics", "1,1,0,0", "--size", "4", "4"]
    for bad in (["c.ply", "p.txt", "--size", "4", "4"], ["c.ply", "p.txt", "--intrinsics", "1,1,0,0"], base + ["--radius", "4"],
                base + ["--radius", "-1"], base + ["--voxel", "0"], ["c.ply", "p.txt", "--intrinsics", "1,2,3", "--size", "4", "4"],
                ["c.ply", "p.txt", "--intrinsics", "1,1,0,0", "--size", "0", "4"], ["c.ply"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    # the reader the tool shares with tools/cloud_eval.py: colours when the file has them
    from cloud_eval import read_ply_columns, read_ply_xyz
    from sailrecon_amd.utils.cloud_export import save_ply
    ply = str(tmp_path / "c.ply")
    save_ply(ply, np.float32([[1, 2, 3], [4, 5, 6]]), np.float32([[0, 0.5, 1], [1, 0, 0]]))
    assert read_ply_xyz(ply).tolist() == [[1, 2, 3], [4, 5, 6]]
    assert read_ply_columns(ply, ("red", "green", "blue")).tolist() == [[0, 128, 255], [255, 0, 0]]
    assert read_ply_columns(ply, ("nx",), optional=True) is None
    import kbench
    assert callable(kbench.render) and callable(kbench.render_once) and "sr_cloud_render" in kbench.render.__doc__
