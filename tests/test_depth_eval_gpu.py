"""Order statistics and depth-map scoring on the GPU (sr_select_ranks, sr_depth_eval,
sailrecon_amd/utils/depth_eval.py) against the fp64 restatement (tests/depth_eval_ref.py,
tests/golden/g19_depth_eval.npz).

What is exact and what has a bound.  Selected values, counts, the MEDIAN alignment, ``aligned`` (against
fl32(s p + t) in numpy fp64 from the kernel's own (s, t)), ``rel_err``, the histogram, delta counts, the
maximum and the quantiles are compared bit for bit.  The SCALE / SCALE_SHIFT fits and the fp64 sums are
held to 1e-12 relative of math.fsum (the figure DESIGN §18 holds its fp64 sums to): a fixed tree over
n <= 14,700 terms of one sign errs by at most log2(n) eps = 1.6e-15 relative.
"""

import json
import os
import sys

import numpy as np
import pytest
import torch

import depth_eval_ref as R
from conftest import REPO
from goldens import DPT_SMALL, dpt_small_model_sd, load_npz

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANKS = [(1, 2), (9, 10), (0, 1), (1, 1)]
ROW_LENS = (1, 63, 64, 65, 255, 257, 1025, 4900)
SUM_TOL = 1e-12


# ---------------------------------------------------------------- select
def run_select(x, ranks=RANKS, mask=None, group=None, n_groups=None, bpr=0, row_len=None):
    """One sr_select_ranks call: (value bits [n_groups, n_ranks], count [n_groups, 2]) on the host.
    ``row_len``: only the first row_len columns of x are the rows (the rest is padding between rows)."""
    from sailrecon_amd import ops
    xt = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    mt = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV)
    if row_len is not None:
        xt = xt[:, :row_len]
        mt = None if mt is None else mt[:, :row_len]
    n_rows = xt.shape[0]
    gt = None if group is None else torch.as_tensor(np.asarray(group, np.int32)).to(DEV)
    ng = n_rows if group is None else n_groups
    value = torch.full((ng, len(ranks)), -7.0, device=DEV)
    count = torch.full((ng, 2), -7, device=DEV, dtype=torch.int32)
    ops.select_ranks(xt, ranks, value, mask=mt, group=gt, n_groups=ng, count=count, blocks_per_row=bpr)
    return value.cpu().numpy().view(np.uint32), count.cpu().numpy().astype(np.int64)


def groupings(n_rows):
    yield None, n_rows
    yield np.zeros(n_rows, np.int32), 1
    g = np.array([0, 1, 0, 1, 2][:n_rows], np.int32)
    yield g, int(g.max()) + 1


def patterns(rng, n_rows, n):
    """name -> (x fp32 [n_rows, n], mask or None); no +-0 anywhere."""
    lowbyte = (np.uint32(0x40490f00) + rng.integers(0, 256, (n_rows, n)).astype(np.uint32)).view(np.float32)
    den = rng.integers(1, 1 << 22, (n_rows, n)).astype(np.uint32)
    den = (den | (rng.integers(0, 2, (n_rows, n)).astype(np.uint32) << 31)).view(np.float32)
    planted = rng.standard_normal((n_rows, n)).astype(np.float32)
    planted.ravel()[::5] = np.nan
    planted.ravel()[1::7] = np.inf
    planted.ravel()[2::11] = -np.inf
    masked = rng.uniform(1, 2, (n_rows, n)).astype(np.float32)
    mask = rng.integers(0, 2, (n_rows, n)).astype(np.uint8) * 255
    mask[0] = 0  # with identity groups, group 0 is empty
    return {"constant": (np.full((n_rows, n), 3.25, np.float32), None),
            "two values": (rng.choice(np.array([-1.5, 2.5], np.float32), (n_rows, n)), None),
            "lowest byte": (lowbyte, None),
            "both signs": (rng.standard_normal((n_rows, n)).astype(np.float32), None),
            "denormals": (den, None),
            "nan and inf": (planted, None),
            "masked": (masked, mask)}


@pytest.mark.parametrize("n_rows", [1, 2, 5])
def test_select_sizes_and_patterns(n_rows):
    rng = np.random.default_rng(100 + n_rows)
    for n in ROW_LENS:
        for name, (x, mask) in patterns(rng, n_rows, n).items():
            assert not (x == 0).any()
            for group, ng in groupings(n_rows):
                want_v, want_c = R.select(x, RANKS, mask, group, ng)
                got_v, got_c = run_select(x, mask=mask, group=group, n_groups=ng)
                what = (name, n, n_rows, None if group is None else group.tolist())
                assert np.array_equal(got_c, want_c), what
                assert np.array_equal(got_v, want_v), what
            if name == "masked":
                v, c = run_select(x, mask=mask)
                assert (v[0] == R.QNAN).all() and c[0, 0] == 0 and c[0, 1] == n


@pytest.mark.parametrize("n_rows", [1, 5])
def test_select_never_reads_the_padding(n_rows):
    """row_stride > row_len, the padding holds NaN and huge values (and, for the mask, ones)."""
    rng = np.random.default_rng(7)
    for n in ROW_LENS:
        for pad in (1, 3, 4, 130):
            buf = np.empty((n_rows, n + pad), np.float32)
            buf[:, :n] = rng.standard_normal((n_rows, n))
            buf[:, n:] = np.where(np.arange(pad) % 2 == 0, np.float32(np.nan), np.float32(3e38))
            mask = np.ones((n_rows, n + pad), np.uint8)
            mask[:, :n] = rng.integers(0, 4, (n_rows, n)) > 0
            for m in (None, mask):
                want_v, want_c = R.select(buf[:, :n], RANKS, None if m is None else m[:, :n])
                got_v, got_c = run_select(buf, mask=m, row_len=n)
                assert np.array_equal(got_c, want_c) and np.array_equal(got_v, want_v), (n, pad, m is not None)


def test_select_is_bit_identical_across_runs_and_grid_shapes():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((5, 4900)).astype(np.float32) * 1e-3
    x[:, ::13] = np.nan
    group = np.array([0, 1, 0, 1, 2], np.int32)
    want = R.select(x, RANKS, None, group, 3)
    for bpr in (0, 0, 1, 2, 3, 7, 64, 5000):
        got = run_select(x, group=group, n_groups=3, bpr=bpr)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), bpr


def test_select_large_rows_take_the_split_path():
    """Rows long enough for the automatic split into several workgroups per row, vector and scalar loads."""
    rng = np.random.default_rng(12)
    full = np.exp(rng.standard_normal((3, 70004))).astype(np.float32)
    full_mask = (rng.uniform(size=full.shape) > 0.2).astype(np.uint8)
    for cols, row_len in ((70004, 70004), (70004, 70001), (70003, 70003)):  # 16-byte loads, with a tail, scalar loads
        x, mask = full[:, :cols], full_mask[:, :cols]
        want = R.select(x[:, :row_len], RANKS, mask[:, :row_len])
        got = run_select(x, mask=mask, row_len=row_len)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (cols, row_len)


def test_select_quantiles_and_distance_quantiles():
    from sailrecon_amd.utils.cloud_eval import distance_quantiles
    from sailrecon_amd.utils.depth_eval import select_quantiles
    rng = np.random.default_rng(13)
    x = rng.uniform(0, 1, (4, 9, 11)).astype(np.float32)
    v, c = select_quantiles(x, (0.5, 0.9, (1, 3)), mask=x > 0.1, group=[0, 1, 1, 0], return_counts=True)
    want_v, want_c = R.select(x.reshape(4, -1), [(1, 2), (9, 10), (1, 3)], (x > 0.1).reshape(4, -1), np.array([0, 1, 1, 0]), 2)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want_v) and np.array_equal(c.cpu().numpy(), want_c)
    d = x.reshape(-1).copy()
    d[::9] = np.nan
    q = distance_quantiles(torch.as_tensor(d).to(DEV), (0.5, 0.9)).cpu().numpy()
    assert np.array_equal(q.view(np.uint32), R.select(d[None], [(1, 2), (9, 10)])[0][0])


# ---------------------------------------------------------------- depth scorer
def run_depth(pred, gt, align, group=None, n_groups=None, mask=None, conf=None, conf_min=None, xform=None,
              n_bins=R.N_BINS, bin_len=R.BIN_LEN, outputs=True):
    """One sr_depth_eval call with every output, on the host (fp32 outputs as their bits)."""
    from sailrecon_amd import ops
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)  # noqa: E731
    p, g = up(pred, torch.float32), up(gt, torch.float32)
    nv, n = p.shape
    ng = nv if group is None else n_groups
    xf = torch.full((ng, 2), -7.0, device=DEV, dtype=torch.float64) if xform is None else up(xform, torch.float64)
    status = torch.full((ng,), -7, device=DEV, dtype=torch.int32)
    stats = torch.full((ng + 1, 16), -7.0, device=DEV, dtype=torch.float64)
    hist = torch.full((ng + 1, n_bins + 2), -7, device=DEV, dtype=torch.int32)  # the call clears it
    aligned = torch.full((nv, n), -7.0, device=DEV) if outputs else None
    rel_err = torch.full((nv, n), -7.0, device=DEV) if outputs else None
    rel_q = torch.full((ng + 1, 2), -7.0, device=DEV)
    ops.depth_eval(p, g, align=align, xform=xf, status=status, stats=stats, hist=hist, bin_len=bin_len,
                   mask=up(mask, torch.uint8), conf=up(conf, torch.float32), conf_min=up(conf_min, torch.float32),
                   group=up(group, torch.int32), n_groups=ng, aligned=aligned, rel_err=rel_err, rel_q=rel_q)
    bits = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)  # noqa: E731
    return dict(xform=xf.cpu().numpy(), status=status.cpu().numpy().astype(np.int64), stats=stats.cpu().numpy(),
                hist=hist.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, aligned=bits(aligned), rel_err=bits(rel_err),
                rel_q=bits(rel_q))


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


def check_config(z, name, scope, align, n_views=None, worst=None):
    group, ng = R.groups_of(name, scope)
    nv = R.SHAPES[name][0] if n_views is None else n_views
    group = group[:nv]
    ng = int(group.max()) + 1
    pred, gt, mask = z[f"{name}/pred"][:nv], z[f"{name}/gt"][:nv], z[f"{name}/mask"][:nv]
    what = (name, nv, scope, align)
    ident = scope == "view"
    got = run_depth(pred, gt, align, None if ident else group, ng, mask=mask)
    ok = R.valid_mask(pred, gt, mask)
    want_xf, want_status = R.fit(pred, gt, ok, align, group, ng)
    assert np.array_equal(got["status"], want_status), what
    if align in ("none", "median"):
        assert got["xform"].tobytes() == want_xf.tobytes(), what
    else:
        err = np.abs(got["xform"] - want_xf) / np.abs(want_xf).clip(1e-300)
        err = err[want_xf != 0].max() if (want_xf != 0).any() else 0.0
        print(f"{what}: (s, t) relative error {err:.2e}")
        worst["fit"] = max(worst["fit"], err)
        assert err <= SUM_TOL and np.array_equal(got["xform"] == 0, want_xf == 0), what
    # aligned, from the kernel's own (s, t); everything after it from the kernel's own aligned
    a = R.apply(pred, got["xform"], group)
    assert np.array_equal(got["aligned"], np.where(ok, a.view(np.uint32), R.QNAN)), what
    want = R.score(got["aligned"].view(np.float32), gt, ok, group, ng)
    ulp = np.abs(got["rel_err"].astype(np.int64) - want["rel_err"].astype(np.int64)).max()
    assert ulp == 0, (what, f"rel_err differs by {ulp} fp32 ulps")
    assert np.array_equal(got["hist"], want["hist"]), what
    assert np.array_equal(got["rel_q"], want["rel_q"]), what
    exact = [0, 1, 2, 9, 10, 11, 12, 13, 14, 15]
    assert np.array_equal(got["stats"][:, exact], want["stats"][:, exact]), what
    sums = [3, 4, 5, 6, 7, 8]
    with np.errstate(all="ignore"):
        rel = np.abs(got["stats"][:, sums] - want["stats"][:, sums]) / np.abs(want["stats"][:, sums])
    rel = np.where(want["stats"][:, sums] == got["stats"][:, sums], 0.0, rel)
    print(f"{what}: sums relative error {rel.max():.2e}")
    worst["sum"] = max(worst["sum"], rel.max())
    assert rel.max() <= SUM_TOL, (what, rel)
    if n_views is None:  # the golden's answers: the whole restatement, no exclusions
        for k in ("status", "hist", "rel_q"):
            gk = z[f"{name}/{scope}/{align}/{k}"]
            assert np.array_equal(got[k], gk.astype(got[k].dtype)), (what, k)
        if (got["status"] & 2).any():
            g_empty = np.nonzero(got["status"] & 2)[0]
            assert (got["stats"][g_empty][:, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]] == 0).all(), what
            assert (got["rel_q"][g_empty] == R.QNAN).all(), what
    # GIVEN with the (s, t) the mode produced; and a second run
    given = run_depth(pred, gt, "given", None if ident else group, ng, mask=mask, xform=got["xform"])
    assert np.array_equal(given["status"], got["status"] & 2), what
    given["status"] = got["status"]
    assert same_bits(given, got), what
    assert same_bits(run_depth(pred, gt, align, None if ident else group, ng, mask=mask), got), what
    return got


@pytest.mark.parametrize("align", R.ALIGNS)
@pytest.mark.parametrize("name,n_views", [("a", 1), ("a", None), ("b", None)])
def test_depth_eval_against_the_restatement(name, n_views, align):
    z = R.golden()
    worst = {"fit": 0.0, "sum": 0.0}
    seen = {}
    for scope in R.SCOPES[name]:
        seen[scope] = check_config(z, name, scope, align, n_views, worst)
    print(f"{name} {n_views} {align}: worst fit error {worst['fit']:.2e}, worst sum error {worst['sum']:.2e} (bound {SUM_TOL})")
    if name == "b" and n_views is None:
        st = seen["view"]["status"]
        assert st[1] == 2                                     # no valid pixel
        assert (st[2] == 1) == (align == "median")            # med(pred) < 0
        assert (st[3] == 1) == (align == "scale_shift")       # constant prediction
    if name == "a" and align == "scale_shift":
        assert seen["view"]["stats"][0, 1] >= 4               # the planted outliers align below zero
        assert seen["view"]["stats"][0, 9] < seen["view"]["stats"][0, 0]


def test_depth_eval_full_histogram_strided_rows_and_missing_outputs():
    """1024 bins; rows with padding between them that is never read; rel_q without rel_err (the scratch)."""
    from sailrecon_amd import ops
    z = R.golden()
    pred, gt, mask = z["b/pred"], z["b/gt"], z["b/mask"]
    group = np.array([0, 1, 0, 1, 2], np.int32)
    want = R.depth_eval(pred, gt, "median", group, 3, mask=mask, n_bins=1024, bin_len=0.0005)
    got = run_depth(pred, gt, "median", group, 3, mask=mask, n_bins=1024, bin_len=0.0005)
    for k in ("status", "hist", "rel_q", "aligned", "rel_err"):
        assert np.array_equal(got[k], want[k].astype(got[k].dtype)), k
    assert got["xform"].tobytes() == want["xform"].tobytes()
    lean = run_depth(pred, gt, "median", group, 3, mask=mask, n_bins=1024, bin_len=0.0005, outputs=False)
    for k in ("xform", "status", "stats", "hist", "rel_q"):
        assert lean[k].tobytes() == got[k].tobytes(), k
    nv, n = pred.shape
    pad = 7
    buf = {k: torch.full((nv, n + pad), float("nan"), device=DEV) for k in ("pred", "gt")}
    mbuf = torch.ones((nv, n + pad), device=DEV, dtype=torch.uint8)
    buf["pred"][:, :n], buf["gt"][:, :n], mbuf[:, :n] = (torch.as_tensor(a).to(DEV) for a in (pred, gt, mask))
    buf["gt"][:, n:] = 2.0  # valid-looking padding: scoring it would change every count
    buf["pred"][:, n:] = 1.0
    xf = torch.empty(3, 2, device=DEV, dtype=torch.float64)
    status = torch.empty(3, device=DEV, dtype=torch.int32)
    stats = torch.empty(4, 16, device=DEV, dtype=torch.float64)
    hist = torch.empty(4, 1026, device=DEV, dtype=torch.int32)
    rel_q = torch.empty(4, 2, device=DEV)
    ops.depth_eval(buf["pred"][:, :n], buf["gt"][:, :n], align="median", xform=xf, status=status, stats=stats, hist=hist,
                   bin_len=0.0005, mask=mbuf[:, :n], group=torch.as_tensor(group).to(DEV), n_groups=3, rel_q=rel_q)
    assert stats.cpu().numpy().tobytes() == got["stats"].tobytes()
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), got["hist"])
    assert np.array_equal(rel_q.cpu().numpy().view(np.uint32), got["rel_q"])


# ---------------------------------------------------------------- Python layer
def test_conf_quantile_keeps_the_most_confident_pixels():
    from sailrecon_amd.utils.depth_eval import depth_accuracy
    z = R.golden()
    pred, gt, mask, conf = z["b/pred"], z["b/gt"], z["b/mask"], z["b/conf"].copy()
    conf[0, ::50] = np.nan  # never valid, never selected
    nv, (h, w) = pred.shape[0], R.SHAPES["b"][1:]
    shape = (nv, h, w)
    res = depth_accuracy(pred.reshape(shape), gt.reshape(shape), valid=mask.reshape(shape).astype(bool),
                         conf=conf.reshape(shape), conf_quantile=0.3, align="median", scope="view",
                         n_bins=R.N_BINS, bin_len=R.BIN_LEN)
    thr = R.select(conf, [(3, 10)])[0].view(np.float32)[:, 0]
    ok = R.valid_mask(pred, gt, mask, conf, thr)
    assert np.array_equal(ok, R.valid_mask(pred, gt, mask) & (conf >= thr[:, None]))
    assert np.array_equal(res["n_valid"], ok.sum(1))
    want = R.depth_eval(pred, gt, "median", mask=mask, conf=conf, conf_min=thr)
    assert np.array_equal(res["hist"], want["hist"])
    assert res["scale"].tobytes() == want["xform"][:, 0].tobytes()
    keep = want["stats"][:nv, 0] > 0
    assert np.allclose(res["abs_rel"][keep], want["stats"][:nv, 3][keep] / want["stats"][:nv, 0][keep], rtol=1e-12)
    assert np.isnan(res["abs_rel"][~keep]).all() and res["pooled"]["n_valid"] == ok.sum()


def test_depth_head_scored_end_to_end():
    """The depth head at the g6_dpt_small configuration against the golden reference depth."""
    from sailrecon_amd.utils.depth_eval import evaluate_depth
    g = load_npz("g6_dpt_small.npz")
    m, sd = dpt_small_model_sd("depth")
    m.load_state_dict(sd)
    m = m.to(DEV)
    toks = {l: torch.from_numpy(g[f"tok_{l}"]).to(DEV) for l in DPT_SMALL["intermediate_layer_idx"]}
    with torch.no_grad():
        preds, conf = m(toks, images=torch.from_numpy(g["images"]).to(DEV), patch_start_idx=5, frames_chunk_size=2)
    ref = g["depth_preds"]
    assert preds.shape == ref.shape
    res = evaluate_depth({"depth_map": preds, "dpt_cnf": conf}, ref[0, ..., 0], align="none", scope="scene")
    print(f"depth head: abs_rel {res['pooled']['abs_rel']:.3e}, delta1 {res['pooled']['delta1']}")
    assert res["pooled"]["delta1"] == 1.0 and res["pooled"]["abs_rel"] < 1e-4
    assert res["pooled"]["n_valid"] == ref.size and res["status"].tolist() == [0]
    res3 = evaluate_depth({"depth_map": 3 * preds, "dpt_cnf": conf}, ref[0, ..., 0], align="median", scope="scene")
    print(f"3 x depth, median aligned: abs_rel {res3['pooled']['abs_rel']:.3e}, scale {res3['scale'][0]:.9f}")
    assert abs(res3["pooled"]["abs_rel"] - res["pooled"]["abs_rel"]) <= 1e-6
    assert abs(res3["scale"][0] - 1 / 3) <= 1e-6


def test_tool_equals_the_function(tmp_path, capsys):
    import depth_eval as tool
    from sailrecon_amd.utils.depth_eval import depth_accuracy
    z = R.golden()
    shape = R.SHAPES["a"]
    pred, gt, mask = (z[f"a/{k}"].reshape(shape) for k in ("pred", "gt", "mask"))
    conf = np.random.default_rng(3).uniform(1, 2, shape).astype(np.float32)
    for k, a in (("pred", pred), ("gt", gt), ("valid", mask), ("conf", conf)):
        np.save(tmp_path / f"{k}.npy", a)
    argv = [str(tmp_path / "pred.npy"), str(tmp_path / "gt.npy"), "--valid", str(tmp_path / "valid.npy"), "--conf",
            str(tmp_path / "conf.npy"), "--conf-quantile", "0.25", "--align", "scale_shift", "--groups", "0", "1", "0",
            "--thresholds", "0.05", "0.1", "--bins", "200"]
    tool.main(argv)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = depth_accuracy(pred, gt, valid=mask, conf=conf, conf_quantile=0.25, align="scale_shift", scope=[0, 1, 0],
                          thresholds=(0.05, 0.1), n_bins=200)
    assert "hist" not in printed and printed["n_groups"] == 2
    for k in ("abs_rel", "rmse", "silog", "delta1", "inlier@0.05", "inlier@0.1", "rel_median", "rel_p90", "scale", "shift",
              "n_valid", "status"):
        assert np.array_equal(np.asarray(printed[k], np.float64), np.asarray(want[k], np.float64)), k
    assert printed["pooled"]["abs_rel"] == want["pooled"]["abs_rel"]
