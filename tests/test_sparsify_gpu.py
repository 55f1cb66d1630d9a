"""The sparsification sums on the GPU (sr_sparsify, sailrecon_amd/utils/conf_eval.py, tools/conf_eval.py) against
the numpy restatement (tests/sparsify_ref.py, tests/golden/g21_sparsify.npz).

Counts and cuts are compared on the bits.  With an integer-valued error every bin sum is exact in fp64 and is
compared on the bits too, which pins the membership of every bin.  With a real-valued error a bin sum is held
to |got - fsum| <= SUM_TOL fsum(|v|), the project's figure for fp64 sums (tests/test_depth_eval_gpu.py, DESIGN
section 18); every figure is printed before it is asserted.
"""

import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

import depth_eval_ref as D
import sparsify_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
SUM_TOL = 1e-12
ROW_LENS = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6149)
STEPS = (1, 2, 3, 7, 100, 1024)
SENT = -7


def bits(x):
    """The bit patterns of a float array (NaN-safe equality)."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint64) if x.dtype == np.float64 else x


def gpu(err, conf, K, mask=None, group=None, n_groups=None, order=R.CONFIDENCE, row_len=None, outputs=True):
    """ops.sparsify on [rows, stride] arrays whose first ``row_len`` columns count: bin_sum fp64, cut as bits,
    count, all numpy; checks that the inputs were not written."""
    from sailrecon_amd import ops
    e, c = torch.from_numpy(np.asarray(err, np.float32)).to(DEV), torch.from_numpy(np.asarray(conf, np.float32)).to(DEV)
    m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(DEV)
    g = None if group is None else torch.tensor(np.asarray(group).tolist(), device=DEV, dtype=torch.int32)
    L = e.shape[1] if row_len is None else row_len
    G = e.shape[0] if group is None else int(n_groups)
    keep = [t.clone() for t in (e, c)] + ([] if m is None else [m.clone()])
    bin_sum = torch.full((G, 2, K), float(SENT), device=DEV, dtype=torch.float64)
    cut = torch.full((G, K), float(SENT), device=DEV, dtype=torch.float32) if outputs else None
    count = torch.full((G, 2), SENT, device=DEV, dtype=torch.int32) if outputs else None
    ops.sparsify(e[:, :L], c[:, :L], K, bin_sum, mask=None if m is None else m[:, :L], group=g, n_groups=G, order=order,
                 cut=cut, count=count)
    out = dict(bin_sum=bin_sum.cpu().numpy())
    if outputs:
        out.update(cut=cut.cpu().numpy().view(np.uint32), count=count.cpu().numpy().astype(np.int64))
    for a, b in zip(keep, [e, c] + ([] if m is None else [m])):
        assert torch.equal(a.view(torch.uint8 if a.dtype == torch.uint8 else torch.int32),
                           b.view(torch.uint8 if b.dtype == torch.uint8 else torch.int32)), "an input was written"
    return out


def compare(got, want, what, exact):
    """cut and count on the bits; bin_sum on the bits (``exact``) or within SUM_TOL of fsum.  Returns the
    largest error of a bin sum in units of fsum(|v|)."""
    if "count" in got:
        assert np.array_equal(got["count"], want["count"]), (what, "count")
        assert np.array_equal(got["cut"], want["cut"]), (what, "cut")
    assert not np.signbit(got["bin_sum"][want["fsum_abs"] == 0]).any(), (what, "an empty bin is +0")
    if exact:
        assert np.array_equal(bits(got["bin_sum"]), bits(want["bin_sum"])), (what, "bin_sum bits")
        return 0.0
    err = np.abs(got["bin_sum"] - want["bin_sum"])
    assert (err <= SUM_TOL * want["fsum_abs"]).all(), (what, "bin_sum", float(err.max()))
    nz = want["fsum_abs"] > 0
    return float((err[nz] / want["fsum_abs"][nz]).max()) if nz.any() else 0.0


def make(rows, L, kind, seed, with_mask):
    """err, conf, mask of a case.  "int": err = (i mod 4096) + 1 at flat index i, every sum exact in fp64.
    "real": a heteroscedastic error with planted NaN and Inf.  The confidence has ties (eighths) and, from eight
    elements on, a NaN and an Inf of its own."""
    rng = np.random.default_rng(seed)
    n = rows * L
    if kind == "int":
        err = ((np.arange(n) % 4096) + 1).astype(np.float32).reshape(rows, L)
    else:
        err = np.abs(rng.standard_normal((rows, L)) * np.exp(rng.standard_normal((rows, L)))).astype(np.float32)
    conf = (np.round(rng.standard_normal((rows, L)) * 8) / 8).astype(np.float32)
    if n >= 8:
        p = rng.permutation(n)
        conf.flat[p[0]], conf.flat[p[1]] = np.nan, -np.inf
        if kind == "real":
            err.flat[p[2]], err.flat[p[3]], err.flat[p[0]] = np.nan, np.inf, np.nan
    mask = (rng.random((rows, L)) > 0.25).astype(np.uint8) if with_mask else None
    return err, conf, mask


COMBOS = list(itertools.product(R.ORDERS, (False, True), (False, True), ("view", "scene", "vector")))


def scope_of(scope, rows):
    if scope == "view":
        return None, rows
    if scope == "scene":
        return [0] * rows, 1
    return ([0, 1, 0], 2) if rows == 3 else ([0], 1)


@pytest.mark.parametrize("row_len", ROW_LENS)
def test_kernel_against_the_restatement(row_len):
    """Every row length x 1 and 3 rows x three of the six K (all six over two neighbouring lengths), both kinds
    of error; the order, the mask, the optional outputs and the scope rotate through all their combinations."""
    idx = ROW_LENS.index(row_len)
    worst, seen = 0.0, 0
    for rows in (1, 3):
        for K in STEPS[idx % 2::2]:
            order, with_mask, outputs, scope = COMBOS[(7 * seen + 5 * idx) % len(COMBOS)]
            seen += 1
            group, G = scope_of(scope, rows)
            for kind in ("int", "real"):
                err, conf, mask = make(rows, row_len, kind, 1000 * idx + seen, with_mask)
                want = R.sparsify(err, conf, K, mask=mask, group=group, n_groups=G, order=order)
                got = gpu(err, conf, K, mask=mask, group=group, n_groups=G, order=order, outputs=outputs)
                worst = max(worst, compare(got, want, (rows, row_len, K, order, with_mask, outputs, scope, kind), kind == "int"))
    print(f"row_len {row_len}: worst bin-sum error {worst:.2e} of fsum(|v|) (bound {SUM_TOL})")


def test_every_option_meets_every_other():
    """All 24 combinations of order, mask, optional outputs and scope at one size with more than one workgroup."""
    for i, (order, with_mask, outputs, scope) in enumerate(COMBOS):
        group, G = scope_of(scope, 3)
        err, conf, mask = make(3, 300, "int", 50 + i, with_mask)
        want = R.sparsify(err, conf, 7, mask=mask, group=group, n_groups=G, order=order)
        compare(gpu(err, conf, 7, mask=mask, group=group, n_groups=G, order=order, outputs=outputs), want, COMBOS[i], True)


@pytest.mark.parametrize("K", (1, 100))
def test_multi_tile_sorts_and_split_bins(K):
    """1 x 70,001: 35 sort tiles, and at K = 1 a bin of 18 chunks."""
    for order in R.ORDERS:
        for kind in ("int", "real"):
            err, conf, mask = make(1, 70001, kind, 7 + K, kind == "real")
            want = R.sparsify(err, conf, K, mask=mask, order=order)
            worst = compare(gpu(err, conf, K, mask=mask, order=order), want, (K, order, kind), kind == "int")
            print(f"70001, K {K}, {order}, {kind}: worst bin-sum error {worst:.2e} of fsum(|v|) (bound {SUM_TOL})")


def test_group_scan_carries_into_the_second_chunk():
    """1025 rows of 8 as 1025 groups: sparsify_scan_kernel scans the group counts in chunks of 4 x 256, and the
    last group's start and first workgroup come through the carry out of the first chunk."""
    for kind in ("int", "real"):
        err, conf, mask = make(1025, 8, kind, 77, kind == "real")
        want = R.sparsify(err, conf, 4, mask=mask)
        assert want["count"][1024, 0] > 0
        compare(gpu(err, conf, 4, mask=mask), want, ("second chunk", kind), kind == "int")


@pytest.mark.parametrize("name", R.CASES)
def test_golden_cases(name):
    """Every golden case and configuration, against the restatement and against the stored answers."""
    c = R.case(name)
    kw = dict(mask=c.get("mask"), group=c.get("group"), n_groups=None if "n_groups" not in c else int(c["n_groups"]),
              row_len=None if "row_len" not in c else int(c["row_len"]))
    for cfg in c["cfg"]:
        tag, K, order = cfg
        want = R.run_cfg(c, cfg)
        got = gpu(c["err"], c["conf/" + tag], K, order=order, **kw)
        worst = compare(got, want, (name, cfg), False)
        stored = c["answers"][R.cfg_tag(cfg)]
        assert np.array_equal(got["cut"], stored["cut"]) and np.array_equal(got["count"], stored["count"]), (name, cfg)
        assert (np.abs(got["bin_sum"] - stored["bin_sum"]) <= SUM_TOL * want["fsum_abs"]).all(), (name, cfg)
        print(f"{name} {R.cfg_tag(cfg)}: worst bin-sum error {worst:.2e} of fsum(|v|) (bound {SUM_TOL})")
    if name == "hetero":  # a calibrated confidence beats a random one beats the error itself
        from sailrecon_amd.utils.conf_eval import sparsification_curves
        a = {t: sparsification_curves(c["err"], c["conf/" + t], 100)["ause"] for t in ("inv_sigma", "random", "anti")}
        assert (0 < a["inv_sigma"]).all() and (a["inv_sigma"] < a["random"]).all() and (a["random"] < a["anti"]).all()


def test_planted_on_the_device():
    rng = np.random.default_rng(3)
    err = np.abs(rng.standard_normal((3, 6149)) * np.exp(rng.standard_normal((3, 6149)))).astype(np.float32)
    err[1, :500] = err[1, 500:1000]  # ties
    for K, group, G in ((1, None, 3), (7, [0, 0, 0], 1), (100, [0, 1, 0], 2)):
        a = gpu(err, -err, K, group=group, n_groups=G)
        assert np.array_equal(bits(a["bin_sum"][:, 0]), bits(a["bin_sum"][:, 1])), (K, "conf = -err is the oracle")
        b = gpu(err, err, K, group=group, n_groups=G, order=R.UNCERTAINTY)
        assert np.array_equal(bits(b["bin_sum"]), bits(a["bin_sum"])), K
        again = gpu(err, -err, K, group=group, n_groups=G)
        for k in a:
            assert np.array_equal(bits(again[k]), bits(a[k])), (K, k, "a second run gives the same bits")
    ie = ((np.arange(3 * 6149) % 4096) + 1).astype(np.float32).reshape(3, 6149)
    const = np.full_like(ie, 0.25)
    for order in R.ORDERS:
        for K, group, G in ((3, None, 3), (100, [0, 0, 0], 1)):
            got = gpu(ie, const, K, group=group, n_groups=G, order=order)
            flat = ie.reshape(G, -1).astype(np.float64)
            b = R.bounds(flat.shape[1], K)
            want = np.array([[flat[g, b[k]:b[k + 1]].sum() for k in range(K)] for g in range(G)])
            assert np.array_equal(got["bin_sum"][:, 0], want), (order, K, "a constant confidence keeps the flat index")
            assert (got["cut"] == np.float32(0.25).view(np.uint32)).all()


def test_the_binding_checks_shapes_before_the_call():
    from sailrecon_amd import ops
    e = torch.ones(3, 10, device=DEV)
    out = torch.empty(3, 2, 1025, device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.sparsify(e, e, 1025, out)
    with pytest.raises(ValueError):
        ops.sparsify(e, e[:, :5], 4, out[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        ops.sparsify(e, e, 4, out[:, :, :4].contiguous(), order="random")
    with pytest.raises(ValueError):
        ops.sparsify(e, e, 4, out[:, :, :4].contiguous(), cut=torch.empty(3, 5, device=DEV))
    with pytest.raises(ValueError):
        ops.sparsify(e, e, 4, out[:2, :, :4].contiguous(), group=torch.zeros(3, device=DEV, dtype=torch.int32))


# ---------------------------------------------------------------- the Python layer
S, H, W = 3, 37, 41


@pytest.fixture(scope="module")
def maps():
    rng = np.random.default_rng(21)
    gt = rng.uniform(1.0, 10.0, (S, H, W)).astype(np.float32)
    sigma = np.exp(0.6 * rng.standard_normal((S, H, W)))
    pred = (0.4 * gt * (1 + 0.1 * sigma * rng.standard_normal((S, H, W))) + 0.05).astype(np.float32)
    conf = (1 / sigma + 0.3 * rng.random((S, H, W))).astype(np.float32)
    gt.flat[rng.permutation(gt.size)[:90]] = 0.0      # invalid pixels
    pred.flat[rng.permutation(gt.size)[:20]] = np.nan
    conf.flat[rng.permutation(gt.size)[:15]] = np.nan  # valid pixels without a confidence are skipped
    valid = rng.random((S, H, W)) > 0.1
    return pred, gt, conf, valid


def expected(pred, gt, conf, valid, metric, align, group, G, K, got):
    """The restatement fed the error tests/depth_eval_ref.py states, from the call's own (s, t) as
    tests/test_depth_eval_gpu.py does; that (s, t) is held to the reference fit first."""
    p, g = pred.reshape(S, -1), gt.reshape(S, -1)
    grp = np.arange(S) if group is None else np.asarray(group)
    ok = D.valid_mask(p, g, valid.reshape(S, -1).astype(np.uint8))
    xf, status = D.fit(p, g, ok, align, grp, G)
    got_xf = np.stack([got["scale"], got["shift"]], 1)
    assert np.array_equal(got["status"], status)
    if align == "median":
        assert got_xf.tobytes() == xf.tobytes()
    else:
        assert (np.abs(got_xf - xf) <= SUM_TOL * np.abs(xf)).all()
    a = D.apply(p, got_xf, grp)
    with np.errstate(all="ignore"):
        if metric == "abs_rel":
            err = D.rel_of(a, g).astype(np.float32)
        elif metric == "abs":
            err = np.abs(a - g)
        else:
            err = (a - g) * (a - g)
    err = np.where(ok, err, np.float32(np.nan)).astype(np.float32)
    return R.sparsify(err, conf.reshape(S, -1), K, group=group, n_groups=G)


@pytest.mark.parametrize("metric", ("abs_rel", "abs", "rmse"))
@pytest.mark.parametrize("align", ("median", "scale_shift"))
def test_depth_sparsification(maps, metric, align):
    from sailrecon_amd.utils.conf_eval import depth_sparsification
    pred, gt, conf, valid = maps
    K = 20
    for scope, (group, G) in {"view": (None, S), "scene": ([0] * S, 1), "vector": ([0, 1, 0], 2)}.items():
        got = depth_sparsification(pred, gt, conf, valid=valid, metric=metric, align=align, n_steps=K,
                                   scope=scope if group is None or scope == "scene" else group)
        want = expected(pred, gt, conf, valid, metric, align, group, G, K, got)
        assert got["n_groups"] == G and got["metric"] == metric
        assert np.array_equal(got["n_considered"], want["count"][:, 0]) and np.array_equal(got["n_skipped"], want["count"][:, 1])
        assert np.array_equal(bits(got["cut"]), want["cut"]), (scope, "cut")
        assert (want["count"][:, 0] > 0).all() and (want["count"][:, 1] > 100).all()
        for g in range(G):
            w = R.curves(want, g, K, root=metric == "rmse")
            for k in ("curve", "fractions", "random", "ause", "ause_norm", "aurg"):
                rel = np.max(np.abs(np.asarray(got[k][g]) - np.asarray(w[k])) / np.abs(np.asarray(w[k]) + (np.asarray(w[k]) == 0)))
                print(f"{metric} {align} {scope} group {g} {k}: relative error {rel:.2e} (bound {SUM_TOL})")
                assert rel <= SUM_TOL, (scope, g, k)
            assert 0 < got["ause"][g] < got["random"][g] and got["aurg"][g] > 0  # an informative confidence


def test_evaluate_depth_confidence_gathers_the_result_dicts(maps):
    from sailrecon_amd.utils.conf_eval import depth_sparsification, evaluate_depth_confidence
    pred, gt, conf, valid = maps
    preds = [{"depth_map": torch.from_numpy(pred[None, :2, :, :, None]), "dpt_cnf": torch.from_numpy(conf[None, :2])},
             {"depth_map": torch.from_numpy(pred[None, 2:, :, :, None]).to(DEV), "dpt_cnf": torch.from_numpy(conf[None, 2:]).to(DEV)}]
    for kw in (dict(), dict(metric="rmse", align="scale_shift", scope="scene", n_steps=7, valid=valid)):
        got = evaluate_depth_confidence(preds, gt[:, None], **kw)
        want = depth_sparsification(pred, gt, conf, **kw)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(bits(np.asarray(got[k])), bits(np.asarray(want[k]))) if isinstance(want[k], np.ndarray) \
                else got[k] == want[k], k
    one = evaluate_depth_confidence({"depth_map": pred[:1, :, :, None], "dpt_cnf": conf[:1]}, gt[:1])
    assert one["n_groups"] == 1 and np.array_equal(one["n_considered"], want_first(pred, gt, conf))


def want_first(pred, gt, conf):
    from sailrecon_amd.utils.conf_eval import depth_sparsification
    return depth_sparsification(pred[:1], gt[:1], conf[:1])["n_considered"]


def test_cloud_distances_go_in_as_they_are():
    """sparsification_curves on [rows, ...] device tensors, an uncertainty, a mask and the RMSE root."""
    from sailrecon_amd.utils.conf_eval import sparsification_curves
    rng = np.random.default_rng(8)
    dist = np.abs(rng.standard_normal((2, 30, 31))).astype(np.float32)
    unc = (dist * rng.uniform(0.5, 1.5, dist.shape)).astype(np.float32)
    mask = rng.random(dist.shape) > 0.3
    got = sparsification_curves(torch.from_numpy(dist * dist).to(DEV), torch.from_numpy(unc).to(DEV), n_steps=10,
                                mask=torch.from_numpy(mask), group="scene", order="uncertainty", root=True)
    want = R.sparsify((dist * dist).reshape(2, -1), unc.reshape(2, -1), 10, mask=mask.reshape(2, -1), group=[0, 0], n_groups=1,
                      order=R.UNCERTAINTY)
    assert np.array_equal(bits(got["cut"]), want["cut"]) and np.array_equal(got["n_considered"], want["count"][:, 0])
    w = R.curves(want, 0, 10, root=True)
    for k in ("curve", "random", "ause", "aurg"):
        assert np.allclose(got[k][0], w[k], rtol=SUM_TOL, atol=0), k
    assert got["curve"].shape == (1, 2, 10) and got["bin_sum"].shape == (1, 2, 10)


def test_tool_prints_what_the_function_returns(maps, tmp_path, capsys):
    import conf_eval as tool
    from pose_eval import jsonable
    from sailrecon_amd.utils.conf_eval import depth_sparsification
    pred, gt, conf, valid = maps
    for k, a in (("pred", pred), ("gt", gt), ("conf", conf), ("valid", valid)):
        np.save(tmp_path / f"{k}.npy", a)
    argv = [str(tmp_path / "pred.npy"), str(tmp_path / "gt.npy"), str(tmp_path / "conf.npy"), "--valid",
            str(tmp_path / "valid.npy"), "--metric", "abs", "--align", "scale_shift", "--groups", "0", "1", "0", "--steps", "9"]
    tool.main(argv)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    want = depth_sparsification(pred, gt, conf, valid=valid, metric="abs", align="scale_shift", scope=[0, 1, 0], n_steps=9)
    want.pop("bin_sum")
    assert line == json.dumps(jsonable(want))
    printed = json.loads(line)
    assert "bin_sum" not in printed and printed["n_groups"] == 2 and len(printed["curve"][0][0]) == 9
    tool.main(argv[:3] + ["--scope", "scene", "--uncertainty", "--steps", "5"])
    unc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    flipped = depth_sparsification(pred, gt, conf, scope="scene", n_steps=5, order="uncertainty")
    straight = depth_sparsification(pred, gt, conf, scope="scene", n_steps=5)
    assert unc["ause"] == flipped["ause"].tolist() and unc["ause"][0] > straight["ause"][0]  # read the wrong way round
