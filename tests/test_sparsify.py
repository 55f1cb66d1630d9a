"""CPU checks of the sparsification curves (ABI 1.14): the restatement's planted answers, curves_from_bins on
hand numbers, every rejection of sr_sparsify through the bindings, the workspace, the ctypes layout, the tool's
arguments and the golden file."""

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

import sparsify_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_14 = (1 << 16) | 14
NEW = ("sr_sparsify_workspace", "sr_sparsify")


@pytest.fixture(autouse=True, scope="module")
def abi_1_14():
    """Everything here is about the library that has the sparsification."""
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_14
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
    assert _header_fields("sr_sparsify_desc") == [f[0] for f in _lib.SparsifyDesc._fields_]
    src = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "sr_api.hip")).read()
    assert "1.14: sr_sparsify" in src
    assert ops.SPARSIFY_ORDER == {"confidence": 0, "uncertainty": 1}
    mk = open(os.path.join(REPO, "self-supervise-sfm_amd", "csrc", "Makefile")).read()
    for obj in ("$(BUILD)/sr_sparsify.o", "$(BUILD)/debug/sr_sparsify.o"):
        assert re.search(re.escape(obj) + r": \w+ \+= -ffp-contract=off -fhonor-nans", mk), obj


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "sparsify"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    assert set(lay) == {"sr_sparsify_desc"}
    c, cls = lay["sr_sparsify_desc"], _lib.SparsifyDesc
    assert ctypes.sizeof(cls) == c["size"]
    assert {f[0] for f in cls._fields_} == set(c["fields"])
    for f, off in c["fields"].items():
        assert getattr(cls, f).offset == off, f


ROWS, LEN = 3, 70001
A = 0x7f0000000000  # fake, suitably aligned device addresses: validation never dereferences them


def _desc(**kw):
    from sailrecon_amd import _lib
    d = _lib.SparsifyDesc()
    d.err, d.conf, d.mask, d.group, d.bin_sum, d.cut, d.count, d.workspace = (A + (i << 24) for i in range(1, 9))
    d.n_rows, d.row_len, d.row_stride, d.n_groups, d.n_steps, d.order = ROWS, LEN, LEN + 3, 2, 100, 0
    d.workspace_bytes = _lib.load().sr_sparsify_workspace(ROWS, LEN, 2, 100)
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
                _lib.check(lib.sr_sparsify(None, ctypes.byref(d) if d is not None else None), "sr_sparsify")
                got.append(0)
            except _lib.SfmAmdError as e:
                got.append(str(e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_sparsify_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    ws = _lib.load().sr_sparsify_workspace
    need, huge = ws(ROWS, LEN, 2, 100), 2 ** 50
    bad = {
        "null desc": None, "null err": _desc(err=None), "null conf": _desc(conf=None), "null bin_sum": _desc(bin_sum=None),
        "null workspace": _desc(workspace=None), "n_rows 0": _desc(n_rows=0), "n_rows -1": _desc(n_rows=-1),
        "row_len 0": _desc(row_len=0), "row_len -5": _desc(row_len=-5), "row_stride < row_len": _desc(row_stride=LEN - 1),
        "2^31 elements": _desc(n_rows=2 ** 16, row_len=2 ** 15, row_stride=2 ** 15, workspace_bytes=huge),
        "a product that overflows": _desc(n_rows=2 ** 62, row_len=4, row_stride=4, workspace_bytes=huge),
        "n_groups 0": _desc(n_groups=0), "n_groups -1": _desc(n_groups=-1), "n_groups > n_rows": _desc(n_groups=ROWS + 1),
        "n_groups 65536": _desc(n_rows=70000, row_len=3, row_stride=3, n_groups=65536, workspace_bytes=huge),
        "no group, n_groups != n_rows": _desc(group=None), "n_steps 0": _desc(n_steps=0), "n_steps -3": _desc(n_steps=-3),
        "n_steps 1025": _desc(n_steps=1025, workspace_bytes=huge), "order 2": _desc(order=2), "order -1": _desc(order=-1),
        "workspace short": _desc(workspace_bytes=need - 1), "workspace % 16": _desc(workspace=A + (8 << 24) + 8),
        "bin_sum % 8": _desc(bin_sum=A + (5 << 24) + 4),
    }
    for what, msg in zip(bad, _call(list(bad.values()))):
        assert isinstance(msg, str) and "sr_sparsify failed (-1): sr_sparsify: " in msg, (what, msg)
    # what passes validation fails at the launch only (there is no device)
    ok = [_desc(), _desc(order=1), _desc(mask=None, cut=None, count=None), _desc(row_stride=LEN),
          _desc(group=None, n_groups=ROWS, workspace_bytes=ws(ROWS, LEN, ROWS, 100)),
          _desc(n_groups=1), _desc(n_steps=1), _desc(n_steps=1024, workspace_bytes=ws(ROWS, LEN, 2, 1024)),
          _desc(n_rows=1, row_len=2 ** 31 - 1, row_stride=2 ** 31 - 1, n_groups=1, workspace_bytes=huge),
          _desc(n_rows=70000, row_len=3, row_stride=3, n_groups=65535, n_steps=1024, workspace_bytes=huge)]
    for msg in _call(ok):
        assert isinstance(msg, str) and "sr_sparsify failed (-2)" in msg, msg


def test_workspace_never_shrinks():
    from sailrecon_amd import _lib, ops
    ws = _lib.load().sr_sparsify_workspace
    srt = _lib.load().sr_sort_workspace
    rows, lens = (1, 2, 3, 5, 32, 65535, 70001), (1, 2, 63, 64, 65, 2047, 2048, 2049, 6149, 30000)
    groups, steps = (1, 2, 3, 5, 32, 65535), (1, 2, 3, 7, 100, 1024)
    for r in rows:
        for l in lens:
            for g in groups:
                if g > r:
                    continue
                for k in steps:
                    w = ws(r, l, g, k)
                    assert w > 0 and w % 16 == 0 and w >= 32 * r * l + srt(r * l) + 16 * g * k, (r, l, g, k)
                    assert ws(r + 1, l, g, k) >= w and ws(r, l + 1, g, k) >= w, (r, l, g, k)
                    assert g + 1 > min(r, 65535) or ws(r, l, g + 1, k) >= w, (r, l, g, k)
                    assert k == 1024 or ws(r, l, g, k + 1) >= w, (r, l, g, k)
    for args in ((0, 5, 1, 1), (5, 0, 1, 1), (-1, 5, 1, 1), (5, 5, 0, 1), (5, 5, 6, 1), (70000, 5, 65536, 1), (5, 5, 1, 0),
                 (5, 5, 1, 1025), (2, 2 ** 30, 1, 1), (2 ** 31, 1, 1, 1), (2 ** 62, 4, 1, 1)):
        assert ws(*args) == 0 and ops.sparsify_workspace_bytes(*args) == 0, args
    assert ws(2 ** 31 - 1, 1, 1, 1) > 0 and ws(1, 2 ** 31 - 1, 1, 1) > 0
    assert ops.sparsify_workspace_bytes(32, 518 * 518, 32, 100) == ws(32, 518 * 518, 32, 100)


# ---------------------------------------------------------------- planted answers in the restatement
def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def test_key_order_and_finiteness_on_the_bits():
    x = np.float32([np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf])
    k = R.key32(x[1:])
    assert (np.diff(k.astype(np.int64)) > 0).all()  # the reals' order, -0 strictly before +0
    assert R.finite_bits(x).tolist() == [False, False, True, True, True, True, True, True, False]
    nan_neg = np.uint32([0xffc00000, 0x7f800001]).view(np.float32)
    assert not R.finite_bits(nan_neg).any()


def test_conf_minus_err_is_the_oracle():
    rng = np.random.default_rng(0)
    err = np.abs(rng.standard_normal((3, 501))).astype(np.float32)
    err[0, :40] = err[0, 40:80]  # ties, which both orders break by flat index
    for K in (1, 7, 100):
        r = R.sparsify(err, -err, K)
        assert np.array_equal(_bits(r["bin_sum"][:, 0]), _bits(r["bin_sum"][:, 1]))
        for g in range(3):
            assert R.curves(r, g, K)["ause"] == 0.0
        r = R.sparsify(err, err, K, order=R.UNCERTAINTY)
        assert np.array_equal(_bits(r["bin_sum"][:, 0]), _bits(r["bin_sum"][:, 1]))


def test_constant_confidence_gives_flat_index_ranges():
    rng = np.random.default_rng(1)
    err = rng.integers(1, 4097, (2, 300)).astype(np.float32)
    conf = np.full_like(err, 0.25)
    for order in R.ORDERS:
        for group, G in ((None, 2), ([0, 0], 1)):
            r = R.sparsify(err, conf, 7, group=group, n_groups=G, order=order)
            flat = err.reshape(G, -1).astype(np.float64)
            for g in range(G):
                b = R.bounds(flat.shape[1], 7)
                want = [flat[g, b[k]:b[k + 1]].sum() for k in range(7)]
                assert r["bin_sum"][g, 0].tolist() == want
                assert (r["cut"][g] == np.float32(0.25).view(np.uint32)).all()


def test_bin_boundaries_and_the_empty_group():
    assert R.bounds(3, 7) == [0, 0, 0, 1, 1, 2, 2, 3]
    err, conf = np.float32([[4, 1, 2]]), np.float32([[0.3, 0.1, 0.2]])
    r = R.sparsify(err, conf, 7)
    assert r["bin_sum"][0, 0].tolist() == [0, 0, 1, 0, 2, 0, 4] and r["bin_sum"][0, 1].tolist() == [0, 0, 4, 0, 2, 0, 1]
    assert r["cut"][0].view(np.float32).tolist() == [np.float32(v) for v in (0.1, 0.1, 0.1, 0.2, 0.2, 0.3, 0.3)]
    assert not np.signbit(r["bin_sum"]).any()
    r = R.sparsify(np.float32([[np.nan, 1, 2]]), np.float32([[1, np.inf, 3]]), 4, mask=np.uint8([[1, 1, 0]]))
    assert r["count"].tolist() == [[0, 3]] and (r["bin_sum"] == 0).all() and not np.signbit(r["bin_sum"]).any()
    assert (r["cut"] == R.QNAN).all()
    assert all(math.isnan(v) for v in (R.curves(r, 0, 4)["ause"], R.curves(r, 0, 4)["random"]))


def test_groups_out_of_range_are_ignored_and_padding_is_not_read():
    err = np.float32([[1, 2, np.nan], [3, 4, np.nan], [5, 6, np.nan], [7, 8, np.nan]])
    conf = np.float32([[1, 2, np.nan], [1, 2, np.nan], [0, 3, np.nan], [9, 9, np.nan]])
    r = R.sparsify(err, conf, 2, group=[1, 5, 1, -1], n_groups=2, row_len=2)
    assert r["count"].tolist() == [[0, 0], [4, 0]]
    assert r["bin_sum"][1].tolist() == [[5 + 1, 2 + 6], [6 + 5, 2 + 1]]  # C: conf 0, 1 | 2, 3; O: err 6, 5 | 2, 1
    assert r["cut"][1].view(np.float32).tolist() == [0.0, 2.0]
    z = R.sparsify(np.float32([[1, 2]]), np.float32([[0.0, -0.0]]), 2)
    assert z["bin_sum"][0, 0].tolist() == [2, 1] and z["cut"][0].tolist() == [0x80000000, 0]  # -0 before +0
    z = R.sparsify(np.float32([[1, 2]]), np.float32([[0.0, -0.0]]), 2, order=R.UNCERTAINTY)
    assert z["bin_sum"][0, 0].tolist() == [1, 2] and z["cut"][0].tolist() == [0, 0x80000000]


# ---------------------------------------------------------------- curves_from_bins
def test_curves_from_bins_on_hand_numbers():
    from sailrecon_amd.utils.conf_eval import bin_bounds, curves_from_bins
    assert bin_bounds(3, 7).tolist() == [0, 0, 0, 1, 1, 2, 2, 3]
    # n = 8, K = 4, bins of two: order C removes errors 1, 1 | 2, 2 | 3, 3 | 9, 9; order O the reverse
    s = np.float64([[2, 4, 6, 18], [18, 6, 4, 2]])
    r = curves_from_bins(s, 8, 4)
    assert r["curve"][0].tolist() == [30 / 8, 28 / 6, 24 / 4, 18 / 2] and r["curve"][1].tolist() == [30 / 8, 12 / 6, 6 / 4, 2 / 2]
    assert r["fractions"].tolist() == [0, 0.25, 0.5, 0.75] and r["random"] == 3.75
    ause = ((28 / 6 - 2) + (6 - 1.5) + (9 - 1)) / 4
    assert r["ause"] == pytest.approx(ause, rel=1e-15) and r["ause_norm"] == pytest.approx(ause / 3.75, rel=1e-15)
    assert r["aurg"] == pytest.approx((0 + (3.75 - 28 / 6) + (3.75 - 6) + (3.75 - 9)) / 4, rel=1e-15)
    q = curves_from_bins(s, 8, 4, root=True)  # the root of every mean before anything else
    assert q["curve"].tolist() == np.sqrt(r["curve"]).tolist() and q["random"] == math.sqrt(3.75)
    assert q["ause"] == pytest.approx(float(np.mean(np.sqrt(r["curve"][0]) - np.sqrt(r["curve"][1]))), rel=1e-15)
    # a perfect confidence: both rows equal, ause exactly 0, aurg positive
    p = curves_from_bins(np.float64([[18, 6, 4, 2], [18, 6, 4, 2]]), 8, 4)
    assert p["ause"] == 0.0 and p["ause_norm"] == 0.0 and p["aurg"] > 0
    # K > n: empty bins repeat the curve's value
    e = curves_from_bins(np.float64([[0, 0, 1, 0, 2, 0, 4], [0, 0, 4, 0, 2, 0, 1]]), 3, 7)
    assert e["curve"][0].tolist() == [7 / 3, 7 / 3, 7 / 3, 3, 3, 4, 4] and e["curve"][1].tolist() == [7 / 3, 7 / 3, 7 / 3, 1.5, 1.5, 1, 1]
    z = curves_from_bins(np.zeros((2, 3)), 5, 3)
    assert z["random"] == 0.0 and z["ause"] == 0.0 and math.isnan(z["ause_norm"])
    n0 = curves_from_bins(np.zeros((2, 3)), 0, 3)
    assert np.isnan(n0["curve"]).all() and np.isnan(n0["fractions"]).all()
    assert all(math.isnan(n0[k]) for k in ("random", "ause", "ause_norm", "aurg"))
    with pytest.raises(ValueError):
        curves_from_bins(np.zeros((2, 4)), 5, 3)


def test_curves_from_bins_agrees_with_the_definition():
    from sailrecon_amd.utils.conf_eval import curves_from_bins
    c = R.gen_case("hetero")
    for tag, root in (("inv_sigma", False), ("random", True), ("anti", False)):
        r = R.sparsify(c["err"], c["conf/" + tag], 100)
        for g in range(3):
            got, want = curves_from_bins(r["bin_sum"][g], r["count"][g, 0], 100, root=root), R.curves(r, g, 100, root=root)
            for k in ("curve", "fractions", "random", "ause", "ause_norm", "aurg"):
                assert np.allclose(got[k], want[k], rtol=1e-12, atol=0), (tag, g, k)
    good, rand, anti = (R.curves(R.sparsify(c["err"], c["conf/" + t], 100), 0, 100) for t in ("inv_sigma", "random", "anti"))
    assert 0 < good["ause"] < rand["ause"] < anti["ause"] and good["aurg"] > 0 > anti["aurg"]
    assert abs(rand["aurg"]) < 0.2 * good["aurg"]


# ---------------------------------------------------------------- Python layer, tool, golden
def test_python_layer_checks_its_arguments_before_the_device():
    import inspect
    from sailrecon_amd.utils import conf_eval
    sig = inspect.signature(conf_eval.depth_sparsification).parameters
    assert [sig[k].default for k in ("valid", "metric", "align", "scope", "n_steps", "xform", "gt_min")] == \
        [None, "abs_rel", "median", "view", 100, None, 0.0]
    sig = inspect.signature(conf_eval.sparsification_curves).parameters
    assert [sig[k].default for k in ("n_steps", "mask", "group", "order", "root")] == [100, None, None, "confidence", False]
    sig = inspect.signature(conf_eval.evaluate_depth_confidence).parameters
    assert (sig["key"].default, sig["conf_key"].default) == ("depth_map", "dpt_cnf")
    m = np.ones((2, 4, 5), np.float32)
    for kw in (dict(metric="mse"), dict(align="affine"), dict(n_steps=0), dict(n_steps=1025), dict(n_steps=2.5),
               dict(order="random"), dict(align="given"), dict(xform=[[1, 0], [1, 0]])):
        with pytest.raises(ValueError):
            conf_eval.depth_sparsification(m, m, m, **kw)
    with pytest.raises(ValueError):
        conf_eval.depth_sparsification(m, m, m[:1])
    with pytest.raises(ValueError):
        conf_eval.sparsification_curves(m, m[:, :2])
    with pytest.raises(ValueError):
        conf_eval.sparsification_curves(m, m, order="best")
    with pytest.raises(ValueError):
        conf_eval.evaluate_depth_confidence([], m)
    with pytest.raises(ValueError):
        conf_eval.evaluate_depth_confidence({"depth_map": m}, m)


def test_tool_argument_parsing():
    import conf_eval as tool
    a = tool.parse_args(["p.npy", "g.npy", "c.npy"])
    assert (a.metric, a.align, a.scope, a.groups, a.steps, a.uncertainty, a.valid) == \
        ("abs_rel", "median", "view", None, 100, False, None)
    a = tool.parse_args(["p.npy", "g.npy", "c.npy", "--valid", "v.npy", "--metric", "rmse", "--align", "scale_shift",
                         "--groups", "0", "1", "0", "--steps", "7", "--uncertainty"])
    assert (a.valid, a.metric, a.align, a.groups, a.steps, a.uncertainty) == ("v.npy", "rmse", "scale_shift", [0, 1, 0], 7, True)
    assert tool.parse_args(["p.npy", "g.npy", "c.npy", "--scope", "scene"]).scope == "scene"
    for bad in (["p.npy", "g.npy"], ["p.npy", "g.npy", "c.npy", "--steps", "0"], ["p.npy", "g.npy", "c.npy", "--steps", "1025"],
                ["p.npy", "g.npy", "c.npy", "--metric", "mse"], ["p.npy", "g.npy", "c.npy", "--align", "given"],
                ["p.npy", "g.npy", "c.npy", "--scope", "pair"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    import kbench
    assert callable(kbench.sparsify) and "sr_sparsify" in kbench.sparsify.__doc__


def test_generator_reproduces_the_golden():
    z = R.build_golden()
    with np.load(R.GOLDEN, allow_pickle=False) as g:
        assert sorted(g.files) == sorted(z)
        for k in g.files:
            assert g[k].dtype == z[k].dtype and g[k].shape == z[k].shape, k
            assert g[k].tobytes() == z[k].tobytes(), k
    voxel = os.path.join(os.path.dirname(R.GOLDEN), "g20_cloud_voxel.npz")
    assert os.path.getsize(R.GOLDEN) <= os.path.getsize(voxel) < 1 << 20
    # what the cases are there for
    p = R.case("planted")
    bad_e, bad_c = ~np.isfinite(p["err"]), ~np.isfinite(p["conf/c"])
    assert (bad_e & ~bad_c).any() and (bad_c & ~bad_e).any() and (bad_e & bad_c).any() and ((p["mask"] == 0) & bad_e).any()
    assert {0x7fc00000, 0x7f800000, 0xff800000} <= set(p["err"].view(np.uint32)[bad_e].tolist())
    zc = R.case("zeros")["conf/c"].view(np.uint32)
    assert (zc == 0).any() and (zc == 0x80000000).any()
    assert len(np.unique(R.case("two")["conf/c"])) == 2
    assert R.case("empty")["answers"]["c/K5/confidence"]["count"][1].tolist() == [0, 200]
    s = R.case("stride")
    assert s["err"].shape[1] > int(s["row_len"]) and np.isnan(s["err"][:, int(s["row_len"]):]).all()
    assert R.case("inter")["group"].tolist() == [0, 1, 0, 2, 1] and R.case("oor")["group"].tolist() == [0, 3, 1, -1, 1]
    assert R.case("oor")["answers"]["c/K7/confidence"]["count"].sum() == 3 * 130
