"""Point-cloud scoring (sr_cloud_nn, sailrecon_amd/utils/cloud_eval.py), CPU side: the restatement of the
contract (tests/cloud_eval_ref.py) against its golden answers (tests/golden/g18_cloud_eval.npz) and a
k-d tree, the bounds the GPU test uses and the margin condition that makes histogram equality hold with
no exclusions, the host-side scores, the PLY reader, the ctypes mirror of the new ABI struct and every
argument check (no GPU is touched).

Bounds.  Per case the fp32 restatement (every step rounded to fp32) is compared with the fp64 one;
4 x its largest error is the bound the GPU kernel must meet on that case (printed here, copied into
DESIGN.md).  Each must stay below 2e-6 x the case's largest distance: on the `far` case a kernel using
|q|^2 + |t|^2 - 2 q.t is off by as much as the distances themselves (shown below), so it cannot pass.
"""

import ctypes
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import cloud_eval_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_11 = (1 << 16) | 11


# ---------------------------------------------------------------- ABI
def test_version_and_exports():
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_11
    assert "sr_cloud_nn" in _lib.EXPORTED and "sr_cloud_nn_workspace" in _lib.EXPORTED
    src = open(os.path.join(REPO, "include", "sfm_amd.h")).read()
    body = re.search(r"typedef struct sr_cloud_nn_desc \{(.*?)\} sr_cloud_nn_desc;", src, flags=re.S).group(1)
    names = []
    for line in body.splitlines():
        decl = line.split("/*")[0].strip()
        for stmt in filter(None, (s.strip() for s in decl.split(";"))):
            first, *rest = stmt.split(",")
            names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert names == [f[0] for f in _lib.CloudNnDesc._fields_]
    doc = src.split("typedef struct sr_cloud_nn_desc")[0][-4000:]
    assert "train_imc.py:301-317" in doc and "direct" in doc and "ABI 1.11" in doc


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "cloud_eval"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    assert set(lay) == {"sr_cloud_nn_desc"}
    cls, c = _lib.CloudNnDesc, lay["sr_cloud_nn_desc"]
    assert ctypes.sizeof(cls) == c["size"]
    assert {f[0] for f in cls._fields_} == set(c["fields"])
    for f, off in c["fields"].items():
        assert getattr(cls, f).offset == off, f


def _desc(**kw):
    """A descriptor that passes every check (fake, suitably aligned device addresses: validation never
    dereferences them)."""
    from sailrecon_amd import _lib
    d = _lib.CloudNnDesc()
    d.query, d.target, d.n_query, d.n_target = 0x7f0000001000, 0x7f0000002000, 5000, 3000
    d.query_xform, d.dist, d.index, d.n_bins, d.bin_len = 0x7f0000003000, 0x7f0000004000, 0x7f0000005000, 100, 0.01
    d.hist, d.stats, d.workspace = 0x7f0000006000, 0x7f0000007000, 0x7f0000008000
    d.workspace_bytes = _lib.load().sr_cloud_nn_workspace(5000, 3000, 0, 1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(descs):
    """Run the calls on a thread of their own: sr_last_error is per thread, and test_abi.py expects the
    main thread's to be empty."""
    from sailrecon_amd import _lib
    lib, got = _lib.load(), []

    def work():
        for d in descs:
            rc = lib.sr_cloud_nn(None, ctypes.byref(d) if d is not None else None)
            got.append((rc, lib.sr_last_error()))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_every_rejection_without_gpu():
    from sailrecon_amd import _lib
    ws = _lib.load().sr_cloud_nn_workspace
    need = ws(5000, 3000, 0, 1)
    assert need > 0
    bad = {
        "null desc": None,
        "null query": _desc(query=None), "null target": _desc(target=None), "null workspace": _desc(workspace=None),
        "0 queries": _desc(n_query=0), "2^31 queries": _desc(n_query=2 ** 31),
        "0 targets": _desc(n_target=0), "2^31 targets": _desc(n_target=2 ** 31), "-1 targets": _desc(n_target=-1),
        "every output NULL": _desc(dist=None, index=None, hist=None, stats=None),
        "0 bins": _desc(n_bins=0), "1025 bins": _desc(n_bins=1025), "-1 bins": _desc(n_bins=-1),
        "bin_len 0": _desc(bin_len=0.0), "bin_len -1": _desc(bin_len=-1.0), "bin_len inf": _desc(bin_len=float("inf")),
        "bin_len nan": _desc(bin_len=float("nan")),
        "chunk -64": _desc(target_chunk=-64), "chunk 100": _desc(target_chunk=100), "chunk 32": _desc(target_chunk=32),
        "65536 slices": _desc(n_target=64 * 65535 + 1, target_chunk=64, workspace_bytes=2 ** 62),
        "workspace short": _desc(workspace_bytes=need - 1),
        "workspace short for the chunk": _desc(target_chunk=64, workspace_bytes=ws(5000, 3000, 64, 1) - 1),
        "workspace % 16": _desc(workspace=0x7f0000008008),
        "query_xform % 8": _desc(query_xform=0x7f0000003004), "target_xform % 8": _desc(target_xform=0x7f0000003004),
        "stats % 8": _desc(stats=0x7f0000007004),
    }
    for (what, _), (rc, msg) in zip(bad.items(), _call(list(bad.values()))):
        assert rc == -1 and msg.startswith(b"sr_cloud_nn: "), (what, rc, msg)
    # what passes validation fails at the launch only (there is no device): the histogram's fields are
    # ignored without a histogram, 1024 bins and both ends of the counts are accepted
    ok = [_desc(), _desc(hist=None, n_bins=0, bin_len=0.0), _desc(n_bins=1024), _desc(n_bins=1, index=None, dist=None),
          _desc(n_query=1, n_target=1, target_chunk=64), _desc(query_xform=None, target_xform=0x7f0000003000),
          _desc(n_query=2 ** 31 - 1, n_target=2 ** 31 - 1, target_chunk=1 << 20,
                workspace_bytes=ws(2 ** 31 - 1, 2 ** 31 - 1, 1 << 20, 0))]
    for rc, msg in _call(ok):
        assert rc == -2, (rc, msg)


def test_workspace_is_monotone():
    from sailrecon_amd import _lib
    ws = _lib.load().sr_cloud_nn_workspace
    ns = [1, 63, 64, 1024, 1025, 2048, 4096, 4097, 10 ** 5, 2 ** 20, 2 ** 20 + 1, 8_600_000, 2 ** 31 - 1]
    for chunk in (0, 1 << 16, 1 << 20):
        for fixed in ns:
            sizes_q = [ws(n, fixed, chunk, 0) for n in ns]
            sizes_t = [ws(fixed, n, chunk, 0) for n in ns]
            assert all(s > 0 for s in sizes_q + sizes_t), (chunk, fixed)
            assert sizes_q == sorted(sizes_q) and sizes_t == sorted(sizes_t), (chunk, fixed)
    for nq, nt in ((1, 1), (4096, 8_600_000), (2 ** 20, 2 ** 20)):
        assert ws(nq, nt, 0, 0) <= ws(nq, nt, 0, 1)
        by_chunk = [ws(nq, nt, c, 0) for c in (256, 1024, 4096, 1 << 16) if (nt + c - 1) // c <= 65535]
        assert by_chunk == sorted(by_chunk, reverse=True)  # fewer slices, fewer partials
        assert ws(nq, nt, 0, 0) >= 16 * nt + 8 * nq
    for args in ((0, 5, 0, 0), (5, 0, 0, 0), (2 ** 31, 5, 0, 0), (5, 2 ** 31, 0, 0), (5, 5, -64, 0), (5, 5, 100, 0),
                 (5, 64 * 65535 + 1, 64, 0)):
        assert ws(*args) == 0, args


def test_ops_argument_checks():
    import torch
    from sailrecon_amd import ops
    q, t = torch.zeros(5, 3), torch.zeros(7, 3)
    with pytest.raises(ValueError, match="device tensor"):
        ops.cloud_nn(q, t, dist=torch.zeros(5))
    from sailrecon_amd.utils import cloud_eval as C
    for bad in (np.zeros((4, 2)), np.zeros((0, 3)), 3.0):
        with pytest.raises(ValueError):
            C._as_points(bad, "x")
    with pytest.raises(ValueError, match="mask"):
        C._as_points(np.zeros((4, 3)), "x", np.zeros(3, bool))
    assert C._as_points(np.arange(24.).reshape(2, 4, 3), "x", np.array([[1, 0, 0, 1], [0, 0, 0, 1]], bool)).shape == (3, 3)
    for kw in (dict(n_bins=0), dict(n_bins=1025), dict(bin_len=0.0), dict(bin_len=float("nan")), dict(thresholds=(0.0015,)),
               dict(thresholds=(2.0,)), dict(thresholds=(-0.01,))):
        with pytest.raises(ValueError):  # every check comes before the first upload
            C.cloud_accuracy(np.zeros((4, 3)), np.zeros((4, 3)), **kw)
    with pytest.raises(ValueError, match="go together"):
        C.evaluate_reconstruction([{"point_map": np.zeros((4, 3))}], np.zeros((4, 3)), key="point_map", conf_key="xyz_cnf")


# ---------------------------------------------------------------- host-side scores
def _stats(d):
    return R.stats_of(np.asarray(d, np.float32))


def test_scores_from_hand_made_histograms():
    from sailrecon_amd.utils.cloud_eval import scores_from_hists
    # bins of 0.1: pred -> gt distances 0.05 0.05 0.15 0.25 0.95 (overflow) and one non-finite point
    da = np.array([0.05, 0.05, 0.15, 0.25, 0.95, np.nan], np.float32)
    dc = np.array([0.05, 0.35, 0.35, 0.15], np.float32)
    ha, hc = R.hist_of(da, 0.1, 4), R.hist_of(dc, 0.1, 4)
    assert ha.tolist() == [2, 1, 1, 0, 1, 1] and hc.tolist() == [1, 1, 0, 2, 0, 0]
    s = scores_from_hists(ha, hc, _stats(da), _stats(dc), (0.1, 0.2, 0.4), 0.1)
    fin = da[:5].astype(np.float64)
    assert s["acc_mean"] == pytest.approx(fin.mean(), rel=1e-15) and s["acc_max"] == fin.max()
    assert s["acc_rms"] == pytest.approx(np.sqrt((fin * fin).mean()), rel=1e-15)
    assert s["comp_mean"] == pytest.approx(dc.astype(np.float64).mean(), rel=1e-15)
    assert s["chamfer"] == pytest.approx((s["acc_mean"] + s["comp_mean"]) / 2, rel=1e-15)
    # the non-finite and the overflow point stay in the denominator: 2/6, 3/6, 4/6
    assert [s[f"precision@{t}"] for t in ("0.1", "0.2", "0.4")] == [2 / 6, 3 / 6, 4 / 6]
    assert [s[f"recall@{t}"] for t in ("0.1", "0.2", "0.4")] == [1 / 4, 2 / 4, 4 / 4]
    assert s["fscore@0.4"] == pytest.approx(2 * (4 / 6) * 1 / (4 / 6 + 1))
    assert (s["n_pred"], s["n_gt"], s["n_nonfinite_pred"], s["n_nonfinite_gt"]) == (6, 4, 1, 0)
    assert s["hist_acc"].tolist() == ha.tolist() and s["hist_comp"].tolist() == hc.tolist()
    ref = R.metrics(da, dc, (0.1, 0.2, 0.4))
    for k, v in ref.items():
        assert s[k] == pytest.approx(v, rel=1e-12), k
    # P + R = 0: nothing below the first edge on either side
    far = np.array([0.35, 0.25], np.float32)
    z = scores_from_hists(R.hist_of(far, 0.1, 4), R.hist_of(far, 0.1, 4), _stats(far), _stats(far), (0.1,), 0.1)
    assert z["precision@0.1"] == 0 and z["recall@0.1"] == 0 and z["fscore@0.1"] == 0.0
    # int32 storage of uint32 counts
    big = np.array([-(2 ** 31), 0, 0], np.int32)  # 2^31 points in bin 0
    st = np.array([2.0 ** 31, 1.0, 1.0, 0.5, 0, 0])
    assert scores_from_hists(big, big, st, st, (1.0,), 1.0)["precision@1"] == 1.0
    for kw in (dict(thresholds=(0.15,)), dict(thresholds=(0.5,)), dict(thresholds=(0.0,)), dict(bin_len=0.0)):
        args = dict(thresholds=(0.1,), bin_len=0.1)
        args.update(kw)
        with pytest.raises(ValueError):  # not a multiple of the bin / beyond the histogram / not positive
            scores_from_hists(ha, hc, _stats(da), _stats(dc), args["thresholds"], args["bin_len"])
    with pytest.raises(ValueError, match="count different"):
        scores_from_hists(ha, hc, _stats(dc), _stats(dc), (0.1,), 0.1)


# ---------------------------------------------------------------- PLY reader
def test_ply_reader_round_trips(tmp_path):
    import torch
    from cloud_eval import read_ply_xyz
    from demo_imc_forward import save_pointcloud_ply
    rng = np.random.default_rng(5)
    views = []
    for _ in range(2):
        pts = rng.standard_normal((1, 6, 7, 3))
        pts[0, 2, 3, 1] = np.nan  # the writer drops non-finite points
        views.append({"point_map_by_unprojection": pts, "images": torch.rand(1, 3, 6, 7)})
    path = str(tmp_path / "pred.ply")
    n = save_pointcloud_ply(views, path)
    want = np.concatenate([v["point_map_by_unprojection"].reshape(-1, 3) for v in views]).astype(np.float32)
    want = want[np.isfinite(want).all(1)]
    got = read_ply_xyz(path)
    assert n == len(want) == 82 and got.dtype == np.float32 and np.array_equal(got, want)
    # ascii, colours in front, doubles, a comment and a face element the reader skips
    a = str(tmp_path / "a.ply")
    with open(a, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty uchar red\nproperty uchar green\n"
                "property uchar blue\nproperty double x\nproperty float y\nproperty float z\nproperty float nx\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                "255 0 0 1.5 2 -3 0\n0 255 0 0.25 1e3 7 0\n1 2 3 -1 -2 -3.5 1\n3 0 1 2\n")
    assert read_ply_xyz(a).tolist() == [[1.5, 2, -3], [0.25, 1000, 7], [-1, -2, -3.5]]
    for text in ("plx\n", "ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n", "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n1\n",
                 "ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n"):
        bad = str(tmp_path / "bad.ply")
        open(bad, "w").write(text)
        with pytest.raises(ValueError):
            read_ply_xyz(bad)
    open(path, "r+b").truncate(os.path.getsize(path) - 1)
    with pytest.raises(ValueError, match="ends after"):
        read_ply_xyz(path)


# ---------------------------------------------------------------- the restatement
def test_generator_and_answers_reproduce_the_golden():
    z = R._npz()
    assert os.path.getsize(R.GOLDEN) < 512 * 1024
    fresh = R.build_golden()
    assert set(fresh) == set(z)
    for k, v in fresh.items():
        assert z[k].dtype == v.dtype and np.array_equal(z[k], v, equal_nan=True), k


def test_restatement_agrees_with_a_kd_tree():
    tree = pytest.importorskip("scipy.spatial").cKDTree
    for name in ("sweep", "far", "hist"):
        c = R.case(name)
        q, t = c["query"].astype(np.float64), c["target"].astype(np.float64)
        d, i = tree(t).query(q)
        want = c["dist_4097"] if name == "sweep" else c["dist"]
        wi = c["index_4097"] if name == "sweep" else c["index"]
        assert np.abs(d - want).max() <= 1e-15 * np.abs(t).max() and np.array_equal(i, wi), name


def test_known_answers():
    c = R.case("ties")
    assert np.array_equal(np.unique(c["dist"]), np.sqrt([0, .25, .5, .75])) and (c["index"] < 216).all()
    d32, i32 = R.nn32(c["query"], c["target"])
    assert np.array_equal(i32, c["index"])  # the ties are ties in fp32 too: every step is exact
    # every target appears again 216 places later, and every query but the ones on a lattice point has
    # further equally near targets
    d2 = ((c["query"][:, None, :].astype(np.float64) - c["target"][None].astype(np.float64)) ** 2).sum(-1)
    n_min = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert sorted(np.unique(n_min).tolist()) == [2, 4, 8, 16]
    assert np.array_equal(c["index"], np.argmax(d2 == d2.min(1, keepdims=True), axis=1))
    # non-finite points
    q = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0]], np.float32)
    t = np.array([[np.inf, 0, 0], [1, 1, 0], [0, 0, np.nan], [0, 0, 2]], np.float32)
    d, i = R.nn64(q, t)
    assert i.tolist() == [1, -1, 1, -1] and np.isnan(d[[1, 3]]).all() and d[0] == np.sqrt(2) and d[2] == 1
    d, i = R.nn64(q, t[[0, 2]])
    assert (i == -1).all() and np.isnan(d).all()
    big = np.array([[3e38, 3e38, 0]], np.float32)  # d2 overflows fp32 but not fp64
    assert R.nn32(-big, big)[1].tolist() == [-1] and R.nn64(-big, big)[1].tolist() == [0]
    # the transform rounds once
    xf = np.concatenate([[2.0], np.eye(3).reshape(-1), [1, 2, 3]])
    assert R.xform_points(np.float32([[1, 1, 1]]), xf).tolist() == [[3, 4, 5]]
    S = R.case("xform")["S"]
    assert np.abs(R.xform_points(R.xform_points(q[[0, 2]], S), R.sim3_inverse(S)) - q[[0, 2]]).max() < 1e-6


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_restatement_error_gives_the_gpu_bound(name):
    err, bound, big = R.case_bound(name)
    print(f"{name}: fp32 restatement max error {err:.3e} -> GPU bound {bound:.3e}; largest distance {big:.3e}, "
          f"bound / largest {bound / big:.3e}")
    assert 0 < bound < 2e-6 * big


def test_expansion_formula_misses_the_far_bound():
    """|q|^2 + |t|^2 - 2 q.t in fp32 on the `far` case: off by orders of magnitude more than the bound."""
    c = R.case("far")
    q, t = c["query"], c["target"]
    d2 = (q * q).sum(1, dtype=np.float32)[:, None] + (t * t).sum(1, dtype=np.float32)[None] - np.float32(2) * (q @ t.T)
    d = np.sqrt(np.maximum(d2.min(1), 0))
    err = np.abs(d - c["dist"]).max()
    _, bound, big = R.case_bound("far")
    print(f"far: expansion formula error {err:.3e} against a bound of {bound:.3e} and distances up to {big:.3e}")
    assert err > 1e4 * bound and err >= 0.5 * big  # every digit is lost: the minimum of d2 is <= 0


def test_histogram_margin_condition():
    """Every fp64 distance of the histogram case lies >= 10 bounds from every positive bin edge, so a
    kernel within the bound puts every point into the slot the fp64 answer names."""
    c = R.case("hist")
    _, bound, _ = R.case_bound("hist")
    m = R.hist_margin(c["dist"], bound, R.HIST_BIN, R.HIST_BINS)
    print(f"hist: seed {int(c['seed'])}, {len(c['dist'])} distances, nearest bin edge {m:.1f} bounds away")
    assert m >= 10
    h = R.hist_of(c["dist"], R.HIST_BIN, R.HIST_BINS)
    assert h.sum() == 5000 and (h[:7] > 0).all() and h[-2:].tolist() == [0, 0]
    d32, _ = R.nn32(c["query"], c["target"])
    assert np.array_equal(R.hist_of(d32, R.HIST_BIN, R.HIST_BINS), h)
