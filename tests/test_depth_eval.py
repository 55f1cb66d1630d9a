"""Depth-map scoring and order statistics (sr_depth_eval, sr_select_ranks,
sailrecon_amd/utils/depth_eval.py), CPU side: planted answers in the restatement of the contract
(tests/depth_eval_ref.py), the rank rule, the host-side metrics, the golden's generator and its margin
condition, the ctypes mirrors of the new ABI structs, every argument check and the tool's argument
parsing (no GPU is touched).
"""

import ctypes
import json
import math
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import depth_eval_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_12 = (1 << 16) | 12
NEW = ("sr_select_workspace", "sr_select_ranks", "sr_depth_eval_workspace", "sr_depth_eval")


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
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_12
    assert all(s in _lib.EXPORTED for s in NEW)
    assert _header_fields("sr_select_desc") == [f[0] for f in _lib.SelectDesc._fields_]
    assert _header_fields("sr_depth_eval_desc") == [f[0] for f in _lib.DepthEvalDesc._fields_]
    src = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "sr_api.hip")).read()
    assert "1.12: sr_select_ranks" in src
    from sailrecon_amd import ops
    assert ops.DEPTH_ALIGN == {"none": 0, "median": 1, "scale": 2, "scale_shift": 3, "given": 4}


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "depth_eval"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    mirror = {"sr_select_desc": _lib.SelectDesc, "sr_depth_eval_desc": _lib.DepthEvalDesc}
    assert set(lay) == set(mirror)
    for name, cls in mirror.items():
        c = lay[name]
        assert ctypes.sizeof(cls) == c["size"], name
        assert {f[0] for f in cls._fields_} == set(c["fields"]), name
        for f, off in c["fields"].items():
            assert getattr(cls, f).offset == off, (name, f)


PIX = 70 * 70


def _select(**kw):
    """A descriptor that passes every check (fake, suitably aligned device addresses: validation never
    dereferences them)."""
    from sailrecon_amd import _lib
    d = _lib.SelectDesc()
    d.x, d.mask, d.group = 0x7f0000001000, 0x7f0000002000, 0x7f0000003000
    d.n_rows, d.row_len, d.row_stride, d.n_groups, d.n_ranks = 5, PIX, PIX, 3, 2
    d.rank_num[0], d.rank_den[0], d.rank_num[1], d.rank_den[1] = 1, 2, 9, 10
    d.value, d.count, d.workspace = 0x7f0000004000, 0x7f0000005000, 0x7f0000006000
    d.workspace_bytes = _lib.load().sr_select_workspace(3, 2)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _depth(**kw):
    from sailrecon_amd import _lib
    d = _lib.DepthEvalDesc()
    d.pred, d.gt, d.mask, d.conf, d.conf_min, d.group = (0x7f0000001000 + (i << 12) for i in range(6))
    d.n_pix, d.stride, d.n_views, d.n_groups, d.gt_min, d.gt_max = PIX, PIX, 5, 3, 0.0, float("inf")
    d.align, d.n_bins, d.bin_len = 1, 1024, 0.005
    d.xform, d.status, d.stats, d.hist, d.aligned, d.rel_err, d.rel_q, d.workspace = \
        (0x7f0000010000 + (i << 12) for i in range(8))
    d.workspace_bytes = _lib.load().sr_depth_eval_workspace(5, PIX, PIX, 3, 1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(fn, descs):
    """Each call through the bindings' ``check`` on a thread of its own (sr_last_error is per thread, and
    test_abi.py expects the main thread's to be empty): the SfmAmdError text, or the return code of a
    call that passed ``check``."""
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


def test_select_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    need = _lib.load().sr_select_workspace(3, 2)
    bad = {
        "null desc": None, "null x": _select(x=None), "null value": _select(value=None),
        "null workspace": _select(workspace=None), "0 ranks": _select(n_ranks=0), "5 ranks": _select(n_ranks=5),
        "num -1": _select(rank_num=(0, -1)), "den 0": _select(rank_den=(1, 0)), "num > den": _select(rank_num=(0, 3)),
        "den 2^20 + 1": _select(rank_den=(0, 2 ** 20 + 1)), "0 rows": _select(n_rows=0), "-1 rows": _select(n_rows=-1),
        "row_len 0": _select(row_len=0), "stride < row_len": _select(row_stride=PIX - 1),
        "2^31 + 1 elements": _select(n_rows=1, n_groups=1, row_len=2 ** 31 + 1, row_stride=2 ** 31 + 1),
        "0 groups": _select(n_groups=0), "6 groups of 5 rows": _select(n_groups=6, workspace_bytes=2 ** 40),
        "no group, 3 groups": _select(group=None), "blocks_per_row -1": _select(blocks_per_row=-1),
        "blocks_per_row 65536": _select(blocks_per_row=65536), "workspace short": _select(workspace_bytes=need - 1),
        "workspace % 16": _select(workspace=0x7f0000006008),
    }
    for what, msg in zip(bad, _call("sr_select_ranks", list(bad.values()))):
        assert isinstance(msg, str) and "sr_select_ranks failed (-1): sr_select_ranks: " in msg, (what, msg)
    # what passes validation fails at the launch only (there is no device)
    four = _select(n_ranks=4, rank_num=(3, 2 ** 20), rank_den=(3, 2 ** 20), workspace_bytes=2 ** 30)
    four.rank_num[2], four.rank_den[2] = 0, 1
    ok = [_select(), _select(mask=None, count=None), _select(group=None, n_groups=5, workspace_bytes=2 ** 30), four,
          _select(n_rows=1, n_groups=1, row_len=2 ** 31, row_stride=2 ** 31), _select(blocks_per_row=65535),
          _select(row_stride=PIX + 1, rank_num=(0, 0))]
    for msg in _call("sr_select_ranks", ok):
        assert isinstance(msg, str) and "sr_select_ranks failed (-2)" in msg, msg


def test_depth_eval_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    ws = _lib.load().sr_depth_eval_workspace
    nan, inf = float("nan"), float("inf")
    bad = {
        "null desc": None,
        **{f"null {k}": _depth(**{k: None}) for k in ("pred", "gt", "xform", "status", "stats", "hist", "workspace")},
        "0 views": _depth(n_views=0), "65536 views": _depth(n_views=65536, n_pix=1, stride=1, workspace_bytes=2 ** 40),
        "0 pixels": _depth(n_pix=0), "stride < n_pix": _depth(stride=PIX - 1),
        "2^31 + 5 floats": _depth(stride=(2 ** 31) // 5 + 1, workspace_bytes=2 ** 50),
        "0 groups": _depth(n_groups=0), "6 groups of 5 views": _depth(n_groups=6, workspace_bytes=2 ** 40),
        "no group, 3 groups": _depth(group=None), "conf without conf_min": _depth(conf_min=None),
        "conf_min without conf": _depth(conf=None), "gt_min nan": _depth(gt_min=nan), "gt_max nan": _depth(gt_max=nan),
        "gt_min >= gt_max": _depth(gt_min=1.0, gt_max=1.0), "align -1": _depth(align=-1), "align 5": _depth(align=5),
        "0 bins": _depth(n_bins=0), "1025 bins": _depth(n_bins=1025), "bin_len 0": _depth(bin_len=0.0),
        "bin_len -1": _depth(bin_len=-1.0), "bin_len inf": _depth(bin_len=inf), "bin_len nan": _depth(bin_len=nan),
        "workspace short": _depth(workspace_bytes=ws(5, PIX, PIX, 3, 0) - 1),
        "workspace short for the scratch": _depth(rel_err=None, workspace_bytes=ws(5, PIX, PIX, 3, 1) - 1),
        "workspace % 16": _depth(workspace=0x7f0000017008), "xform % 8": _depth(xform=0x7f0000010004),
        "stats % 8": _depth(stats=0x7f0000012004),
    }
    for what, msg in zip(bad, _call("sr_depth_eval", list(bad.values()))):
        assert isinstance(msg, str) and "sr_depth_eval failed (-1): sr_depth_eval: " in msg, (what, msg)
    ok = [_depth(), _depth(mask=None, conf=None, conf_min=None, aligned=None, rel_err=None),
          _depth(rel_q=None, rel_err=None, workspace_bytes=ws(5, PIX, PIX, 3, 0)), _depth(group=None, n_groups=5,
                                                                                         workspace_bytes=2 ** 30),
          _depth(gt_min=-inf, gt_max=0.5), _depth(n_bins=1), _depth(stride=PIX + 3, workspace_bytes=2 ** 30)] + \
         [_depth(align=a) for a in range(5)]
    for msg in _call("sr_depth_eval", ok):
        assert isinstance(msg, str) and "sr_depth_eval failed (-2)" in msg, msg


def test_workspaces_never_shrink():
    from sailrecon_amd import _lib
    sel, dep = _lib.load().sr_select_workspace, _lib.load().sr_depth_eval_workspace
    for r in (1, 2, 3, 4):
        sizes = [sel(g, r) for g in (1, 2, 63, 64, 65, 4096, 65535, 2 ** 20)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert [sel(64, r) for r in (1, 2, 3, 4)] == sorted(sel(64, r) for r in (1, 2, 3, 4))
    assert sel(64, 2) >= 64 * 2 * 256 * 4
    for args in ((0, 1), (1, 0), (1, 5), (-1, 1)):
        assert sel(*args) == 0, args
    pix = [1, 2047, 2048, 2049, 4900, 518 * 518, 518 * 518 + 1, 2 ** 20]
    views = [1, 2, 5, 64, 65, 2000]
    for scratch in (0, 1):
        for n in pix:
            by_views = [dep(v, n, n, 1, scratch) for v in views]
            assert all(s > 0 for s in by_views) and by_views == sorted(by_views), (n, scratch)
            for v in views:
                assert dep(v, n, n, v, scratch) >= dep(v, n, n, 1, scratch) and dep(v, n, n + 5, 1, scratch) >= dep(v, n, n, 1, scratch)
        for v in views:
            by_pix = [dep(v, n, 2 ** 20, 1, scratch) for n in pix]
            assert by_pix == sorted(by_pix), (v, scratch)
    assert dep(64, 518 * 518, 518 * 518, 64, 1) >= dep(64, 518 * 518, 518 * 518, 64, 0) + 64 * 518 * 518 * 4
    for args in ((0, 5, 5, 1, 0), (65536, 1, 1, 1, 0), (5, 0, 5, 1, 0), (5, 6, 5, 1, 0), (5, 5, 5, 0, 0), (5, 5, 5, 6, 0),
                 (8192, 518 * 518, 518 * 518, 1, 0)):
        assert dep(*args) == 0, args


# ---------------------------------------------------------------- the rank rule
def test_rank_rule_is_the_residual_statistics_rule():
    """the median is s[(n - 1) / 2], p90 is s[(9 n + 9) / 10 - 1]."""
    from sailrecon_amd.utils import depth_eval as D
    for n in list(range(1, 2100)) + [268324, 17172736, 2 ** 31]:
        assert R.rank_index(1, 2, n) == (n - 1) // 2 == D.rank_index(1, 2, n)
        assert R.rank_index(9, 10, n) == (9 * n + 9) // 10 - 1 == D.rank_index(9, 10, n)
        assert R.rank_index(0, 1, n) == 0 and R.rank_index(1, 1, n) == n - 1
        assert R.rank_index(2 ** 19, 2 ** 20, n) == (n - 1) // 2  # an equal fraction, an equal rank
    assert D.rank_fraction(0.5) == (1, 2) and D.rank_fraction(0.9) == (9, 10) and D.rank_fraction(0.25) == (1, 4)
    assert D.rank_fraction(0) == (0, 1) and D.rank_fraction(1.0) == (1, 1) and D.rank_fraction((3, 7)) == (3, 7)
    num, den = D.rank_fraction(1 / 3 + 1e-9)
    assert den <= 2 ** 20 and abs(num / den - 1 / 3) < 1e-6
    for bad in (-0.1, 1.5, float("nan"), "half", (3, 2), (1, 2 ** 20 + 1), (-1, 2)):
        with pytest.raises(ValueError):
            D.rank_fraction(bad)
    x = np.array([[5, 1, 4, np.nan, 2, 3, np.inf, -np.inf]], np.float32)
    v, c = R.select(x, [(1, 2), (9, 10), (0, 1), (1, 1)])
    assert v.view(np.float32).tolist() == [[3.0, 5.0, 1.0, 5.0]] and c.tolist() == [[5, 3]]
    v, c = R.select(x, [(1, 2)], mask=np.zeros_like(x, np.uint8))
    assert v[0, 0] == R.QNAN and c.tolist() == [[0, 8]]


# ---------------------------------------------------------------- planted answers
def _gt(seed=0, nv=3, n=500):
    return np.random.default_rng(seed).uniform(1.0, 6.0, (nv, n)).astype(np.float32)


@pytest.mark.parametrize("align", ["median", "scale"])
def test_half_depth_aligns_with_scale_two_exactly(align):
    gt = _gt()
    out = R.depth_eval(gt / 2, gt, align)
    assert (out["xform"] == [2.0, 0.0]).all() and (out["status"] == 0).all()
    assert np.array_equal(out["aligned"].view(np.float32), gt)
    st = out["stats"]
    assert (st[:, 0] == [500, 500, 500, 1500]).all() and (st[:, [1, 2, 3, 4, 5, 6, 7, 8, 12]] == 0).all()
    assert (st[:, 9:12] == st[:, :1]).all()
    assert (out["hist"][:, 0] == st[:, 0]).all() and out["hist"][:, 1:].sum() == 0
    assert (out["rel_q"].view(np.float32) == 0).all()


def test_planted_scale_and_shift_are_recovered():
    gt = _gt(1)
    s0, t0 = 2.5, 0.75
    pred = ((gt.astype(np.float64) - t0) / s0).astype(np.float32)
    for group, ng in ((None, None), (np.zeros(3, np.int64), 1)):
        out = R.depth_eval(pred, gt, "scale_shift", group, ng)
        assert np.abs(out["xform"] - [s0, t0]).max() < 1e-6  # the fp32 rounding of pred
        assert out["stats"][-1, 3] / out["stats"][-1, 0] < 1e-7 and (out["stats"][:, 9] == out["stats"][:, 0]).all()
    # exactly representable data: the fit is exact
    p = np.arange(1, 65, dtype=np.float32)[None]
    out = R.depth_eval(p, 2 * p + 3, "scale_shift")
    assert out["xform"].tolist() == [[2.0, 3.0]] and out["stats"][0, 5] == 0


def test_status_bits_and_nonpositive_depth():
    gt = _gt(2)
    pred = (gt / 2).copy()
    gt2 = gt.copy()
    gt2[1] = 0
    out = R.depth_eval(pred, gt2, "median")
    assert out["status"].tolist() == [0, 2, 0] and out["xform"][1].tolist() == [1.0, 0.0]
    assert out["stats"][1, 0] == 0 and out["stats"][1, 2] == 500 and (out["rel_q"][1] == R.QNAN).all()
    assert np.array_equal(out["rel_q"][3], R.select(out["rel_err"].view(np.float32).reshape(1, -1), [(1, 2), (9, 10)])[0][0])
    neg = pred.copy()
    neg[0] = -neg[0]
    out = R.depth_eval(neg, gt, "median")
    assert out["status"].tolist() == [1, 0, 0] and out["xform"][0].tolist() == [1.0, 0.0]
    assert out["stats"][0, 1] == 500 and (out["stats"][0, 6:12] == 0).all() and out["stats"][0, 3] > 500
    const = pred.copy()
    const[2] = 1.5
    out = R.depth_eval(const, gt, "scale_shift")
    assert out["status"].tolist() == [0, 0, 1] and out["xform"][2, 0] == 1.0
    assert out["xform"][2, 1] == math.fsum(gt[2].astype(np.float64).tolist()) / 500 - 1.5
    out = R.depth_eval(pred, gt, "given", xform=[[2, 0], [-2, 0], [2, -100]])
    assert out["status"].tolist() == [0, 0, 0] and out["stats"][:3, 1].tolist() == [0, 500, 500]
    assert (out["stats"][1:3, 9:12] == 0).all() and (out["stats"][0, 9:12] == 500).all()


def test_invalid_pixels_count_nowhere_else():
    gt = _gt(3, 1, 100)
    pred = (gt * 1.1).astype(np.float32)
    gt[0, :4] = [0, np.nan, np.inf, -2]
    pred[0, 4:6] = [np.nan, -np.inf]
    mask = np.ones_like(gt, np.uint8)
    mask[0, 6:9] = 0
    conf = np.full_like(gt, 2.0)
    conf[0, 9:12] = [1.0, np.nan, 1.99]
    out = R.depth_eval(pred, gt, "none", mask=mask, conf=conf, conf_min=np.array([2.0], np.float32))
    assert out["stats"][0, 0] == 88 and out["stats"][0, 2] == 12 and out["hist"][0].sum() == 88
    assert (out["rel_err"][0, :12] == R.QNAN).all() and (out["aligned"][0, :12] == R.QNAN).all()
    out = R.depth_eval(pred, gt, "none", mask=mask, gt_min=1.5, gt_max=4.0)
    assert out["stats"][0, 0] == ((gt[0] > 1.5) & (gt[0] <= 4.0) & np.isfinite(pred[0]) & (mask[0] != 0)).sum()


# ---------------------------------------------------------------- host-side metrics
def test_metrics_from_stats_and_histogram():
    from sailrecon_amd.utils.depth_eval import metrics_from_stats
    z = R.golden()
    taus = (0.05, 0.1, 0.25)
    for name, scope, align in (("a", "view", "median"), ("b", "mixed", "scale_shift"), ("a", "scene", "none")):
        stats, hist = z[f"{name}/{scope}/{align}/stats"], z[f"{name}/{scope}/{align}/hist"]
        for row in range(len(stats)):
            if stats[row, 0] == 0:
                got = metrics_from_stats(stats[row], hist[row], taus, R.BIN_LEN)
                assert all(math.isnan(got[k]) for k in ("abs_rel", "rmse", "silog", "delta1", "inlier@0.05"))
                continue
            got, want = metrics_from_stats(stats[row], hist[row], taus, R.BIN_LEN), R.metrics(stats[row], hist[row], taus)
            for k, v in want.items():
                assert got[k] == pytest.approx(v, rel=1e-14, abs=1e-300), (name, scope, align, row, k)
            assert got["n_valid"] == stats[row, 0] and got["n_nonpos"] == stats[row, 1] and got["n_invalid"] == stats[row, 2]
    # by hand: four pixels, rel 0.01 0.04 0.06 0.3, bins of 0.05
    st = np.zeros(16)
    st[[0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]] = [4, 0.41, 0.2, 0.8, 0.4, 0.1, 0.2, 3, 4, 4, 0.3]
    got = metrics_from_stats(st, np.array([2, 1, 0, 0, 0, 0, 1, 0, 0, 0], np.int64), (0.05, 0.1, 0.3), 0.05)
    assert got["abs_rel"] == 0.41 / 4 and got["sq_rel"] == 0.05 and got["rmse"] == math.sqrt(0.2)
    assert got["rmse_log"] == math.sqrt(0.025) and got["silog"] == pytest.approx(100 * math.sqrt(0.025 - 0.01), rel=1e-14)
    assert got["log10"] == 0.05 and (got["delta1"], got["delta2"], got["delta3"]) == (0.75, 1.0, 1.0)
    assert (got["inlier@0.05"], got["inlier@0.1"], got["inlier@0.3"]) == (0.5, 0.75, 0.75)
    with pytest.raises(ValueError, match="counts"):
        metrics_from_stats(st, np.array([2, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.int64), (0.05,), 0.05)


def test_threshold_and_argument_validation():
    import torch
    from sailrecon_amd import ops
    from sailrecon_amd.utils import depth_eval as D
    st, h = np.zeros(16), np.zeros(12, np.int64)
    for taus, bin_len in (((0.0075,), 0.005), ((1.0,), 0.005), ((-0.05,), 0.005), ((0.0,), 0.005), ((0.05,), 0.0),
                          ((0.05,), float("nan"))):
        with pytest.raises(ValueError):
            D.metrics_from_stats(st, h, taus, bin_len)
    p = np.ones((2, 4, 5), np.float32)
    for kw in (dict(n_bins=0), dict(n_bins=1025), dict(bin_len=0.0), dict(bin_len=float("inf")), dict(thresholds=(0.007,)),
               dict(thresholds=(6.0,)), dict(align="log"), dict(align="given"), dict(xform=[[1, 0], [1, 0]]),
               dict(conf=p), dict(conf_quantile=0.5), dict(conf=p, conf_quantile=1.5), dict(scope="pair"),
               dict(scope=[0, 2]), dict(scope=[0, 1, 1]), dict(scope=[0.0, 1.0]), dict(valid=np.ones((2, 4, 5))),
               dict(valid=np.ones((2, 4, 4), bool)), dict(conf=np.ones((2, 4, 4), np.float32), conf_quantile=0.5)):
        with pytest.raises(ValueError):  # every check comes before the first upload
            D.depth_accuracy(p, p, **kw)
    with pytest.raises(ValueError, match="resize"):
        D.depth_accuracy(p, np.ones((2, 4, 6), np.float32))
    for bad in (np.ones(5), np.ones((2, 3, 4, 5)), np.ones((0, 4, 5)), "x"):
        with pytest.raises(ValueError):
            D._as_maps(bad, "pred")
    for good, shape in ((np.ones((4, 5)), (1, 4, 5)), (np.ones((3, 1, 4, 5)), (3, 4, 5)), (np.ones((3, 4, 5, 1)), (3, 4, 5)),
                        (np.ones((1, 3, 4, 5, 1)), (3, 4, 5)), (np.ones((1, 3, 4, 5)), (3, 4, 5))):
        assert tuple(D._as_maps(good, "pred").shape) == shape
    with pytest.raises(ValueError, match="no 'depth_map'"):
        D.evaluate_depth([{"depth": p}], p)
    with pytest.raises(ValueError, match="non-empty list"):
        D.evaluate_depth([], p)
    with pytest.raises(ValueError):
        D.select_quantiles(np.ones((2, 5)), ())
    with pytest.raises(ValueError):
        D.select_quantiles(np.ones((2, 5)), (0.5,), mask=np.ones((2, 4), bool))
    with pytest.raises(ValueError):
        D.select_quantiles(np.ones((2, 5)), (0.5,), group=[0, 2])
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="device tensor"):
        ops.select_ranks(x, [(1, 2)], torch.zeros(3, 1))
    with pytest.raises(ValueError, match="device tensor"):
        ops.depth_eval(x, x, align="none", xform=torch.zeros(3, 2, dtype=torch.float64), status=torch.zeros(3, dtype=torch.int32),
                       stats=torch.zeros(4, 16, dtype=torch.float64), hist=torch.zeros(4, 12, dtype=torch.int32), bin_len=0.1)
    with pytest.raises(ValueError, match="align"):
        ops.depth_eval(x, x, align="best", xform=None, status=None, stats=None, hist=None, bin_len=0.1)
    from sailrecon_amd.utils.cloud_eval import distance_quantiles
    with pytest.raises(ValueError):
        distance_quantiles(np.zeros((3, 3)))


def test_tool_argument_parsing():
    import depth_eval as tool
    a = tool.parse_args(["p.npy", "g.npy"])
    assert (a.align, a.scope, a.groups, a.conf, a.thresholds, a.bin_len, a.bins) == \
        ("median", "view", None, None, [0.05, 0.1, 0.25], 0.005, 1024)
    a = tool.parse_args(["p.npy", "g.npy", "--conf", "c.npy", "--conf-quantile", "0.2", "--align", "scale_shift", "--scope",
                         "scene", "--valid", "v.npy", "--thresholds", "0.1", "--bin-len", "0.01", "--bins", "64"])
    assert (a.conf, a.conf_quantile, a.align, a.scope, a.valid, a.thresholds, a.bin_len, a.bins) == \
        ("c.npy", 0.2, "scale_shift", "scene", "v.npy", [0.1], 0.01, 64)
    assert tool.parse_args(["p.npy", "g.npy", "--groups", "0", "0", "1"]).groups == [0, 0, 1]
    for bad in (["p.npy"], ["p.npy", "g.npy", "--conf", "c.npy"], ["p.npy", "g.npy", "--conf-quantile", "0.5"],
                ["p.npy", "g.npy", "--align", "given"], ["p.npy", "g.npy", "--conf", "c.npy", "--conf-quantile", "2"],
                ["p.npy", "g.npy", "--scope", "pair"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


# ---------------------------------------------------------------- the golden
def test_generator_reproduces_the_golden():
    z = R.golden()
    assert os.path.getsize(R.GOLDEN) < 315542  # g18's size
    fresh = R.build_golden()
    assert set(fresh) == set(z)
    for k, v in fresh.items():
        assert np.asarray(v).tobytes() == z[k].tobytes() and np.asarray(v).dtype == z[k].dtype, k


def test_every_rel_keeps_its_distance_from_the_bin_edges():
    """Every fp64 rel of every configuration lies >= 4 fp32 ulps from every positive bin edge, so a
    kernel whose fl32(rel) is the correctly rounded one bins every pixel as the restatement does; the
    generator takes the first seed for which this holds."""
    z = R.golden()
    worst = R.margins(z)
    print(f"seed {int(z['seed'])}: smallest distance to a bin edge {worst:.2f} fp32 ulps")
    assert worst >= R.MARGIN_ULPS
    for seed in range(int(z["seed"])):
        assert R.margins(R.make_inputs(seed)) < R.MARGIN_ULPS, seed
    for name, (nv, h, w) in R.SHAPES.items():
        p = z[f"{name}/pred"].astype(np.float64)
        keep = [v for v in range(nv) if not (name == "b" and v in (2, 3))]  # the negated and the constant view
        assert (p[keep, 200:].std(1) / p[keep, 200:].mean(1) >= 0.1).all()
