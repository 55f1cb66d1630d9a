"""CPU checks of the stable sort and the voxel downsampling (ABI 1.13): the restatement's planted
answers, the numpy model of the sort's tile plan, every rejection of both entry points through the
bindings, workspaces, ctypes layouts, the PLY writer, the tools' arguments and the golden file."""

import ctypes
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import cloud_voxel_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_13 = (1 << 16) | 13
NEW = ("sr_sort_workspace", "sr_sort_pairs", "sr_cloud_voxel_workspace", "sr_cloud_voxel")


@pytest.fixture(autouse=True, scope="module")
def abi_1_13():
    """Everything here is about the library that has the sort and the downsampling."""
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_13
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
    assert _header_fields("sr_sort_desc") == [f[0] for f in _lib.SortDesc._fields_]
    assert _header_fields("sr_cloud_voxel_desc") == [f[0] for f in _lib.CloudVoxelDesc._fields_]
    src = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "sr_api.hip")).read()
    assert "1.13: sr_sort_pairs" in src
    assert ops.VOXEL_MODE == {"mean": 0, "best": 1} and _lib.SR_VOXEL_MAX_ATTR == 8
    assert _lib.ABI_MIN == 1 << 16


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "cloud_voxel"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    mirror = {"sr_sort_desc": _lib.SortDesc, "sr_cloud_voxel_desc": _lib.CloudVoxelDesc}
    assert set(lay) == set(mirror)
    for name, cls in mirror.items():
        c = lay[name]
        assert ctypes.sizeof(cls) == c["size"], name
        assert {f[0] for f in cls._fields_} == set(c["fields"]), name
        for f, off in c["fields"].items():
            assert getattr(cls, f).offset == off, (name, f)


N = 70001
A = 0x7f0000000000  # fake, suitably aligned device addresses: validation never dereferences them


def _sort(**kw):
    from sailrecon_amd import _lib
    d = _lib.SortDesc()
    d.keys_in, d.vals_in, d.keys_out, d.vals_out, d.workspace = (A + (i << 24) for i in range(1, 6))
    d.n, d.key_bits, d.workspace_bytes = N, 64, _lib.load().sr_sort_workspace(N)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _voxel(**kw):
    from sailrecon_amd import _lib
    d = _lib.CloudVoxelDesc()
    d.points, d.attr, d.mask, d.weight, d.xform = (A + (i << 24) for i in range(1, 6))
    d.n, d.ldp, d.lda, d.n_attr, d.axis_bits, d.mode = N, 3, 4, 4, 21, _lib.SR_VOXEL_BEST
    d.origin[0], d.origin[1], d.origin[2], d.voxel, d.capacity = 0.1, -0.2, 0.3, 0.05, N
    d.out_points, d.out_attr, d.out_count, d.out_index, d.out_key, d.voxel_of, d.counts, d.workspace = \
        (A + (i << 24) for i in range(6, 14))
    d.workspace_bytes = _lib.load().sr_cloud_voxel_workspace(N)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _call(fn, descs):
    """Each call through the bindings' ``check`` on a thread of its own (sr_last_error is per thread, and
    test_abi.py expects the main thread's to be empty): the SfmAmdError text, or 0 for a call that passed."""
    from sailrecon_amd import _lib
    lib, got = _lib.load(), []

    def work():
        for d in descs:
            try:
                _lib.check(getattr(lib, fn)(None, ctypes.byref(d) if d is not None else None), fn)
                got.append(0)
            except _lib.SfmAmdError as e:
                got.append(str(e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_sort_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    need = _lib.load().sr_sort_workspace(N)
    bad = {
        "null desc": None, "null keys_in": _sort(keys_in=None), "null vals_out": _sort(vals_out=None),
        "null workspace": _sort(workspace=None), "n 0": _sort(n=0), "n -1": _sort(n=-1),
        "n 2^31": _sort(n=2 ** 31, workspace_bytes=2 ** 50), "key_bits 0": _sort(key_bits=0),
        "key_bits 65": _sort(key_bits=65), "key_bits -8": _sort(key_bits=-8),
        "keys_out == keys_in": _sort(keys_out=A + (1 << 24)), "vals_out == vals_in": _sort(vals_out=A + (2 << 24)),
        "keys_in % 8": _sort(keys_in=A + (1 << 24) + 4), "keys_out % 8": _sort(keys_out=A + (3 << 24) + 4),
        "vals_in % 4": _sort(vals_in=A + (2 << 24) + 2), "vals_out % 4": _sort(vals_out=A + (4 << 24) + 1),
        "workspace short": _sort(workspace_bytes=need - 1), "workspace % 16": _sort(workspace=A + (5 << 24) + 8),
    }
    for what, msg in zip(bad, _call("sr_sort_pairs", list(bad.values()))):
        assert isinstance(msg, str) and "sr_sort_pairs failed (-1): sr_sort_pairs: " in msg, (what, msg)
    # what passes validation fails at the launch only (there is no device)
    ok = [_sort(), _sort(vals_in=None), _sort(keys_out=None), _sort(vals_in=None, keys_out=None)] + \
         [_sort(key_bits=b) for b in R.SORT_BITS] + [_sort(n=n, workspace_bytes=2 ** 40) for n in R.SORT_N + (2 ** 31 - 1,)]
    for msg in _call("sr_sort_pairs", ok):
        assert isinstance(msg, str) and "sr_sort_pairs failed (-2)" in msg, msg


def test_cloud_voxel_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    need = _lib.load().sr_cloud_voxel_workspace(N)
    nan, inf = float("nan"), float("inf")
    bad = {
        "null desc": None, "null points": _voxel(points=None), "null out_points": _voxel(out_points=None),
        "null workspace": _voxel(workspace=None), "n 0": _voxel(n=0), "n 2^31": _voxel(n=2 ** 31, workspace_bytes=2 ** 50),
        "ldp 2": _voxel(ldp=2), "n_attr -1": _voxel(n_attr=-1), "n_attr 9": _voxel(n_attr=9, lda=9),
        "n_attr without attr": _voxel(attr=None), "lda < n_attr": _voxel(lda=3),
        "weight under MEAN": _voxel(mode=_lib.SR_VOXEL_MEAN), "mode 2": _voxel(mode=2), "mode -1": _voxel(mode=-1),
        "axis_bits 0": _voxel(axis_bits=0), "axis_bits 22": _voxel(axis_bits=22), "origin nan": _voxel(origin=(0, nan)),
        "origin inf": _voxel(origin=(2, -inf)), "voxel 0": _voxel(voxel=0.0), "voxel -1": _voxel(voxel=-1.0),
        "voxel inf": _voxel(voxel=inf), "voxel nan": _voxel(voxel=nan), "capacity 0": _voxel(capacity=0),
        "capacity n + 1": _voxel(capacity=N + 1), "workspace short": _voxel(workspace_bytes=need - 1),
        "workspace % 16": _voxel(workspace=A + (13 << 24) + 8), "xform % 8": _voxel(xform=A + (5 << 24) + 4),
        "out_key % 8": _voxel(out_key=A + (10 << 24) + 4),
    }
    for what, msg in zip(bad, _call("sr_cloud_voxel", list(bad.values()))):
        assert isinstance(msg, str) and "sr_cloud_voxel failed (-1): sr_cloud_voxel: " in msg, (what, msg)
    ok = [_voxel(), _voxel(mode=_lib.SR_VOXEL_MEAN, weight=None), _voxel(weight=None),
          _voxel(attr=None, n_attr=0, mask=None, xform=None, out_attr=None, out_count=None, out_index=None, out_key=None,
                 voxel_of=None, counts=None), _voxel(ldp=4, lda=9, n_attr=8, capacity=1), _voxel(axis_bits=1),
          _voxel(n=1, capacity=1), _voxel(voxel=5e-324), _voxel(origin=(0, 1e300))]
    for msg in _call("sr_cloud_voxel", ok):
        assert isinstance(msg, str) and "sr_cloud_voxel failed (-2)" in msg, msg


def test_workspaces_never_shrink():
    from sailrecon_amd import _lib
    srt, vox = _lib.load().sr_sort_workspace, _lib.load().sr_cloud_voxel_workspace
    ns = sorted(set(R.SORT_N) | {5 * 518 * 518, 32 * 518 * 518, 2 ** 30, 2 ** 31 - 1})
    s, v = [srt(n) for n in ns], [vox(n) for n in ns]
    assert all(x > 0 and x % 16 == 0 for x in s + v) and s == sorted(s) and v == sorted(v)
    for n, a, b in zip(ns, s, v):
        tiles = -(-n // R.TILE)
        assert a >= 24 * n + 4 * 256 * tiles and b >= a + 24 * n + 4 * tiles, n
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert srt(n) == 0 and vox(n) == 0, n


# ---------------------------------------------------------------- the sort's tile plan, on the host
@pytest.mark.parametrize("key_bits", R.SORT_BITS)
def test_tile_plan_model_is_the_stable_argsort(key_bits):
    """What the three kernels of a pass compute, restated in numpy, gives a permutation of [0, n) (the model
    asserts that every scattered position is inside the buffer and taken once) equal to the stable argsort,
    at every size of the GPU list."""
    for n in R.SORT_N:
        for kind in R.SORT_KINDS if n < 5000 else ("random", "three", "junk", "constant"):
            keys = R.sort_keys(kind, n, key_bits)
            ref = R.sort_ref(keys, key_bits)
            sk, perm = R.sort_plan_model(keys, key_bits)
            assert np.array_equal(perm, ref) and np.array_equal(sk, keys[ref]), (n, kind)
    vals = np.arange(300, dtype=np.int64)[::-1].copy()
    keys = R.sort_keys("three", 300, key_bits)
    assert np.array_equal(R.sort_plan_model(keys, key_bits, vals)[1], vals[R.sort_ref(keys, key_bits)])


def test_sort_contract_ignores_the_bits_above_key_bits():
    keys = np.array([0x1F0, 0x2E1, 0x3D0, 0x4C1], np.uint64)
    assert R.sort_ref(keys, 4).tolist() == [0, 2, 1, 3]  # by the low nibble, ties in input order
    assert R.sort_ref(keys, 64).tolist() == [0, 1, 2, 3]
    assert int(R.SORT_N[-2]) > 3 * R.TILE  # one size spans more than three tiles


# ---------------------------------------------------------------- planted answers in the restatement
def test_lattice_with_k_copies_gives_count_k_and_the_cell_s_own_point():
    g = np.arange(-2, 3, dtype=np.float32)
    cell = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(0.5)  # cell centres, edge 1
    k = 3
    rng = np.random.default_rng(5)
    order = rng.permutation(k * len(cell))
    p = np.tile(cell, (k, 1))[order]
    a = np.tile(np.arange(len(cell), dtype=np.float32)[:, None], (k, 1))[order]
    for mode in (R.MEAN, R.BEST):
        r = R.downsample(p, 1.0, attr=a, axis_bits=3, mode=mode)
        assert r["counts"].tolist() == [125, 375, 0, 0] and (r["count"] == k).all()
        # ascending key is z-major, then y, then x: the lattice sorted by (z, y, x)
        want = cell[np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))]
        assert np.array_equal(r["points"], want)  # the mean of k equal points is the point
        assert np.array_equal(r["attr"][:, 0], np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2])).astype(np.float32))
        firsts = np.array([np.nonzero((p == c).all(1))[0][0] for c in want])
        assert np.array_equal(r["index"], firsts)  # the lowest member index, in both modes without weights
        assert np.array_equal(r["voxel_of"], np.searchsorted(r["key"], R.voxel_keys(p, 1.0, axis_bits=3)[1]))


def test_face_points_fall_in_the_upper_cell():
    o = np.float64([1.0, 2.0, 3.0])
    on = (o + np.float64([[0.25, -0.5, 0.75]])).astype(np.float32)
    under = np.nextafter(on, np.float32(-np.inf))
    _, key, state = R.voxel_keys(np.concatenate([on, under]), 0.25, origin=o, axis_bits=4)
    assert state.tolist() == [0, 0]
    u = lambda k: [(int(k) >> s) & 15 for s in (0, 4, 8)]  # noqa: E731
    assert u(key[0]) == [1 + 8, -2 + 8, 3 + 8] and u(key[1]) == [0 + 8, -3 + 8, 2 + 8]
    c = R.case("faces")
    r = R.run_cfg(c, c["cfg"][0], R.MEAN)
    assert r["counts"][2] == 0 and r["counts"][3] == 0 and r["counts"][1] == len(c["points"])


def test_range_ends_and_the_sentinel():
    p = np.float32([[-4, 0, 0], [np.nextafter(np.float32(-4), np.float32(-9)), 0, 0], [np.nextafter(np.float32(4), np.float32(0)), 0, 0],
                    [4, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    _, key, state = R.voxel_keys(p, 0.5, axis_bits=4)
    assert state.tolist() == [0, 2, 0, 2, 1, 1]
    assert (key[state != 0] == np.uint64(1 << 12)).all() and key[0] & np.uint64(15) == 0 and key[2] & np.uint64(15) == 15
    r = R.downsample(p, 0.5, axis_bits=4, mask=np.uint8([1, 1, 0, 1, 0, 1]))
    assert r["counts"].tolist() == [1, 1, 3, 2] and r["voxel_of"].tolist() == [0, -1, -1, -1, -1, -1]


def test_best_ties_go_to_the_lowest_index_and_nan_weights_are_skipped():
    p = np.float32([[0.1, 0.1, 0.1]] * 6 + [[1.1, 0.1, 0.1]] * 3)
    p[:, 1] += np.arange(9, dtype=np.float32) * np.float32(0.01)
    w = np.float32([1, 3, np.nan, 3, 2, 3, -0.0, 0.0, -0.0])
    a = np.arange(9, dtype=np.float32)[:, None]
    r = R.downsample(p, 1.0, attr=a, weight=w, mode=R.BEST, axis_bits=2)
    assert r["counts"].tolist() == [2, 8, 1, 0] and r["count"].tolist() == [5, 3]
    assert r["index"].tolist() == [1, 6] and r["attr"][:, 0].tolist() == [1.0, 6.0]
    assert np.array_equal(r["points"], p[[1, 6]])  # copied bit for bit
    assert R.downsample(p, 1.0, mode=R.BEST, axis_bits=2)["index"].tolist() == [0, 6]  # no weight: the lowest index
    m = R.downsample(p, 1.0, attr=a, mode=R.MEAN, axis_bits=2)
    assert m["count"].tolist() == [6, 3] and m["index"].tolist() == [0, 6]
    s = np.float64(0)
    for v in p[:6, 1]:
        s = s + np.float64(v)  # left to right
    assert m["points"][0, 1] == np.float32(s / np.float64(6)) and m["attr"][0, 0] == np.float32(2.5)


def test_mean_is_the_left_to_right_sum():
    """Values whose pairwise and left-to-right fp64 sums differ: the restatement follows the latter."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 8, 4000)).astype(np.float32)
    p = np.zeros((4000, 3), np.float32)
    p[:, 0] = np.float32(0.5)
    r = R.downsample(p, 1.0, attr=x[:, None], axis_bits=2)
    s = np.float64(0)
    for v in x:
        s = s + np.float64(v)
    assert r["attr"][0, 0] == np.float32(s / np.float64(4000)) and r["count"].tolist() == [4000]


# ---------------------------------------------------------------- Python layer, tools, golden
def test_save_ply_round_trip(tmp_path):
    import cloud_eval as tool
    from sailrecon_amd.utils.cloud_export import save_ply
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((257, 3)).astype(np.float32)
    rgb = rng.uniform(-0.1, 1.1, (257, 3)).astype(np.float32)
    path = str(tmp_path / "c.ply")
    assert save_ply(path, xyz, rgb) == 257
    assert np.array_equal(tool.read_ply_xyz(path), xyz)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 257\n") and len(body) == 257 * 15
    rec = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    want = np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8)  # the demo's colour rounding
    assert np.array_equal(np.stack([rec["r"], rec["g"], rec["b"]], 1), want)
    import torch
    assert save_ply(path, torch.from_numpy(xyz), torch.from_numpy(rgb)) == 257 and open(path, "rb").read() == raw
    with pytest.raises(ValueError):
        save_ply(path, xyz, rgb[:5])


def test_the_demo_s_own_ply_writer_has_the_same_layout(tmp_path):
    import demo_imc_forward as demo
    import torch
    from sailrecon_amd.utils.cloud_export import save_ply
    rng = np.random.default_rng(4)
    xyz = rng.standard_normal((1, 6, 7, 3))
    img = torch.from_numpy(rng.uniform(0, 1, (1, 3, 6, 7)).astype(np.float32))
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    demo.save_pointcloud_ply([{"point_map_by_unprojection": xyz, "images": img}], a)
    save_ply(b, xyz.reshape(-1, 3).astype(np.float32), img.reshape(3, -1).T)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_tool_argument_parsing():
    import cloud_eval as tool
    import demo_imc_forward as demo
    a = tool.parser().parse_args(["p.ply", "g.ply", "--voxel", "0.02"])
    assert a.voxel == 0.02 and tool.parser().parse_args(["p.ply", "g.ply"]).voxel is None
    for bad in (["p.ply", "g.ply", "--voxel", "0"], ["p.ply", "g.ply", "--voxel", "nan"], ["p.ply", "g.ply", "--voxel"]):
        with pytest.raises(SystemExit):
            tool.main(bad)
    d = demo.parser().parse_args([])
    assert d.voxel is None and d.conf_quantile == 0.0 and d.voxel_mode == "mean"
    d = demo.parser().parse_args(["--voxel", "0.05", "--conf-quantile", "0.3", "--voxel-mode", "best"])
    assert (d.voxel, d.conf_quantile, d.voxel_mode) == (0.05, 0.3, "best")
    for bad in (["--voxel-mode", "median", "--voxel", "1"], ["--conf-quantile", "0.5"], ["--voxel-mode", "best"],
                ["--voxel", "-1"], ["--voxel", "1", "--conf-quantile", "1.5"]):
        with pytest.raises(SystemExit):
            demo.main(bad)
    import kbench
    assert callable(kbench.voxel) and "sr_sort_pairs" in kbench.voxel.__doc__


def test_python_layer_checks_its_arguments_before_the_device():
    from sailrecon_amd.utils import cloud_eval, cloud_export
    import inspect
    for fn in (cloud_eval.cloud_accuracy, cloud_eval.evaluate_reconstruction):
        assert inspect.signature(fn).parameters["voxel"].default is None
    sig = inspect.signature(cloud_export.voxel_downsample).parameters
    assert [sig[k].default for k in ("mode", "axis_bits", "capacity", "return_inverse")] == ["mean", 21, None, False]
    sig = inspect.signature(cloud_export.scene_cloud).parameters
    assert (sig["key"].default, sig["conf_key"].default, sig["conf_quantile"].default, sig["voxel"].default) == \
        ("point_map_by_unprojection", "dpt_cnf", 0.0, None)
    with pytest.raises(ValueError):
        cloud_export.scene_cloud([])
    with pytest.raises(ValueError):
        cloud_export.voxel_downsample(np.zeros((4, 2), np.float32), 1.0)


def test_generator_reproduces_the_golden():
    z = R.build_golden()
    with np.load(R.GOLDEN, allow_pickle=False) as g:
        assert sorted(g.files) == sorted(z)
        for k in g.files:
            assert g[k].dtype == z[k].dtype and g[k].shape == z[k].shape, k
            assert g[k].tobytes() == z[k].tobytes(), k
    assert os.path.getsize(R.GOLDEN) < 1 << 20
    c = R.case("box_a")
    assert len(c["points"]) == R.BOX_N and not ((c["points"].min(0) <= 0) & (c["points"].max(0) >= 0)).all()
    per = {cfg["tag"]: R.run_cfg(c, cfg, R.MEAN)["count"].mean() for cfg in c["cfg"]}
    assert 1 <= per["v1"] < 2 and 4 < per["v8"] < 10 and per["all"] > 4000
