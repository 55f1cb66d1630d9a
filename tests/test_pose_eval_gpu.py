"""sr_pose_pair_errors / sr_pose_align on the device against the fp64 restatement
(tests/pose_eval_ref.py), through sailrecon_amd.utils.pose_eval.

Pair errors must lie within their case's bound (4 x the fp32 restatement's own error against fp64,
tests/test_pose_eval.py prints and checks them: all below 1e-3 degrees, so a kernel that takes
acos((tr E - 1) / 2) fails the small-angle cases by two orders of magnitude) and the histograms must
be equal, which the margin condition asserted there makes hold for every pair.

Alignment: the kernel and the restatement accumulate the same fp32 inputs in fp64, so scale, t, the
ATE and (where the singular values are separated) R must agree to 1e-9 relative.  t and the ATE are
measured against the scene: where the fit is exact (N <= 2 with scale) their own size is rounding
noise, so the reference size is max(|value|, the rms extent of the ground-truth centres).
"""

import os
import sys

import numpy as np
import pytest
import torch

import pose_eval_ref as R
from conftest import REPO
from goldens import load_npz, rule_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
sys.path.insert(0, os.path.join(REPO, "tools"))


def E():
    from sailrecon_amd.utils import pose_eval
    return pose_eval


def run_views(run, four_pred=False, three_gt=False):
    pred, gt = R.case(run["case"])
    pred, gt = pred[:run["n"]].copy(), gt[:run["n"]].copy()  # the shared cases are read-only
    if four_pred:  # 3x4 -> 4x4
        pred = np.concatenate([pred, np.tile(np.array([[[0, 0, 0, 1]]], np.float32), (len(pred), 1, 1))], 1)
    if three_gt:
        gt = np.ascontiguousarray(gt[:, :3])
    return pred, gt


def check_run(run, pred, gt):
    rb, tb = R.case_bounds(run["case"])
    rot64, trans64 = R.run_errors(run)
    pairs = R.run_pairs(run)
    rot, trans = E().pose_pair_errors(pred, gt, pairs=pairs, trans_ambiguity=run["ambiguity"])
    rot, trans = rot.cpu().numpy().astype(np.float64), trans.cpu().numpy().astype(np.float64)
    assert rot.shape == rot64.shape and trans.shape == trans64.shape
    nan = np.isnan(rot64)
    assert np.array_equal(np.isnan(rot), nan) and np.array_equal(np.isnan(trans), nan)
    er, et = np.abs(rot - rot64)[~nan].max(), np.abs(trans - trans64)[~nan].max()
    print(f"{run}: max error rot {er:.3e} (bound {rb:.3e}) trans {et:.3e} (bound {tb:.3e}) deg")
    assert er <= rb and et <= tb
    acc = E().pose_accuracy(pred, gt, thresholds=(run["bin_deg"],), pairs=pairs, trans_ambiguity=run["ambiguity"],
                            bin_deg=run["bin_deg"], n_bins=run["n_bins"])
    want = R.histogram(rot64, trans64, run["bin_deg"], run["n_bins"])
    assert np.array_equal(acc["hist"], want), (acc["hist"], want)
    ref = R.accuracy(want, (run["bin_deg"],), run["bin_deg"])
    for k, v in ref.items():
        assert acc[k] == pytest.approx(v, abs=1e-15), k
    return acc


@pytest.mark.parametrize("k", range(len(R.RUNS)))
def test_pair_errors_and_histograms(k):
    """Every run of pose_eval_ref.RUNS with 3x4 predictions against 4x4 ground truth (strides 12 / 16):
    N = 2, 3, 33, 65 and 130 (one past the 32- and 64-wide tile edges, a three-tile triangle), five bins
    (most pairs overflow), translation angles above 90 degrees with and without the ambiguity, the
    small-angle cases, and the explicit list with i > j, i == j, repeats and an index out of range."""
    run = R.RUNS[k]
    acc = check_run(run, *run_views(run))
    if run.get("pairs") == "list":
        assert acc["n_nonfinite"] == 1 and acc["n_pairs"] == len(R.explicit_pairs(run["n"])[0])
    else:
        assert acc["n_nonfinite"] == 0 and acc["n_pairs"] == run["n"] * (run["n"] - 1) // 2


@pytest.mark.parametrize("four_pred,three_gt", [(True, False), (False, True), (True, True)])
def test_strides(four_pred, three_gt):
    """16 / 16, 12 / 12 and 16 / 12 floats per view (12 / 16 is the cases' own mix), all pairs and the list."""
    for k in (2, len(R.RUNS) - 1):
        run = R.RUNS[k]
        assert run["case"] == "a33" and run["n"] == 33
        check_run(run, *run_views(run, four_pred, three_gt))


def test_device_tensors_and_view_dicts_are_accepted():
    run = R.RUNS[2]
    pred, gt = run_views(run)
    dicts = [{"extrinsic": torch.from_numpy(pred[k:k + 1]).to(DEV)} for k in range(len(pred))]
    a = E().pose_accuracy(dicts, torch.from_numpy(gt)[None].to(DEV), bin_deg=5.0, n_bins=36)
    b = E().pose_accuracy(pred, gt, bin_deg=5.0, n_bins=36)
    assert np.array_equal(a["hist"], b["hist"]) and a["rra@15"] == b["rra@15"] and 0 < b["auc@30"] < 1


def test_nonfinite_views():
    """A NaN and an Inf planted in one predicted view: exactly N - 1 pairs in the non-finite slot of
    all three rows, NaN in their per-pair outputs, every other pair and count as without them."""
    run = R.RUNS[2]
    pred, gt = run_views(run)
    pred[5, 1, 2], pred[5, 0, 3] = np.nan, np.inf
    n = len(pred)
    i, j = R.all_pairs(n)
    hit = (i == 5) | (j == 5)
    rot64, trans64 = R.run_errors(run)
    clean = R.histogram(rot64, trans64, run["bin_deg"], run["n_bins"])
    want = R.histogram(np.where(hit, np.nan, rot64), np.where(hit, np.nan, trans64), run["bin_deg"], run["n_bins"])
    acc = E().pose_accuracy(pred, gt, bin_deg=run["bin_deg"], n_bins=run["n_bins"])
    assert np.array_equal(acc["hist"], want)
    assert (acc["hist"][:, -1] == n - 1).all() and acc["n_nonfinite"] == n - 1
    lost = clean[:, :-1] - acc["hist"][:, :-1]
    assert (lost >= 0).all() and (lost.sum(1) == n - 1).all()
    rot, trans = (t.cpu().numpy() for t in E().pose_pair_errors(pred, gt))
    assert np.isnan(rot[hit]).all() and np.isnan(trans[hit]).all()
    rb, tb = R.case_bounds(run["case"])
    assert np.abs(rot[~hit] - rot64[~hit]).max() <= rb and np.abs(trans[~hit] - trans64[~hit]).max() <= tb
    gt_bad = gt.copy()
    gt_bad[0, 2, 3] = -np.inf  # ground truth counts too: views 0 and 5 now
    acc = E().pose_accuracy(pred, gt_bad, bin_deg=run["bin_deg"], n_bins=run["n_bins"])
    assert (acc["hist"][:, -1] == 2 * (n - 1) - 1).all()


def test_two_runs_are_identical():
    run = R.RUNS[5]
    pred, gt = (torch.from_numpy(x).to(DEV) for x in run_views(run))
    outs = []
    for _ in range(2):
        rot, trans = E().pose_pair_errors(pred, gt)
        acc = E().pose_accuracy(pred, gt, bin_deg=1.0, n_bins=180)
        outs.append((rot.view(torch.int32).cpu(), trans.view(torch.int32).cpu(), acc["hist"]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])


def test_fine_histogram_counts_the_kernels_own_errors():
    """130 views at the default 180 one-degree bins: too many errors for a margin to hold against fp64,
    so the histogram is checked against the kernel's own per-pair errors (themselves within the bound,
    above) binned by its rule, floor(fl32(err / bin_deg))."""
    run = R.RUNS[5]
    pred, gt = run_views(run)
    for bin_deg, n_bins in ((1.0, 180), (0.7, 64)):
        rot, trans = (t.cpu().numpy() for t in E().pose_pair_errors(pred, gt))
        acc = E().pose_accuracy(pred, gt, thresholds=(bin_deg,), bin_deg=bin_deg, n_bins=n_bins)
        q = lambda e: np.minimum(np.floor(e / np.float32(bin_deg)), n_bins).astype(np.int64)  # noqa: E731  fp32 division
        want = np.stack([np.bincount(q(e), minlength=n_bins + 2) for e in (rot, trans, np.maximum(rot, trans))])
        assert np.array_equal(acc["hist"], want)
        assert acc["n_pairs"] == 130 * 129 // 2


def test_many_identical_views():
    """4,096 copies of three views: 8.4 M pairs over a 64 x 64 grid of tiles, nearly all in slot 0 of
    every row (the contended path of the LDS histogram); the counts must add up exactly."""
    _, gt = R.case("a33")
    n = 4096
    views = torch.from_numpy(np.ascontiguousarray(gt[np.arange(n) % 3])).to(DEV)
    acc = E().pose_accuracy(views, views, bin_deg=1.0, n_bins=180)
    assert acc["n_pairs"] == n * (n - 1) // 2 and acc["n_nonfinite"] == 0
    assert (acc["hist"][:, 0] == n * (n - 1) // 2).all() and acc["auc@5"] == 1.0


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("name", R.ALIGN_CASES)
def test_align(name, with_scale):
    pred, gt, _ = R.align_case(name)
    ref = R.umeyama(pred, gt, with_scale)
    got = E().align_poses(pred, gt, with_scale=with_scale, per_view=True)
    n = len(pred)
    scene = max(ref["extent"], 1e-300)
    rel = lambda a, b, size: float(np.abs(np.asarray(a) - np.asarray(b)).max() / size)  # noqa: E731
    err = got["err"].cpu().numpy()
    d = {"scale": rel(got["scale"], ref["scale"], abs(ref["scale"])),
         "ate": rel(got["ate"], ref["ate"], max(ref["ate"], scene)),
         "err": rel(err, ref["err"], max(ref["err"].max(), scene))}
    unique = ref["status"] == 0  # rank >= 2: the rotation, and with it t, is unique
    if unique:
        d["R"] = rel(got["R"], ref["R"], 1.0)
        d["t"] = rel(got["t"], ref["t"], max(np.abs(ref["t"]).max(), scene))
    print(f"{name} with_scale={with_scale}: status {got['status']} scale {got['scale']:.6f} ate {got['ate']:.6e} "
          f"relative differences {({k: float(f'{v:.2e}') for k, v in d.items()})}")
    assert got["status"] == ref["status"] == {"n1": 3, "n2": 2}.get(name, 0)
    assert all(v <= 1e-9 for v in d.values()), d
    Rg = got["R"]
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rg) - 1) < 1e-12  # always a rotation
    assert err.shape == (n,) and got["ate"] == pytest.approx(np.sqrt((err * err).mean()), rel=1e-12, abs=1e-300)
    if not with_scale:
        assert got["scale"] == 1.0
    if name == "n1":
        assert np.array_equal(Rg, np.eye(3)) and got["scale"] == 1.0
        assert np.abs(got["t"] - (R.centres(gt)[0] - R.centres(pred)[0])).max() < 1e-12
    if name == "n4_mirror":
        assert got["ate"] > 0.1  # no proper rotation maps a cloud onto its mirror image
    # the fit is the same whichever of 3x4 / 4x4 holds the poses
    again = E().align_poses(pred[:, :3], np.concatenate([gt, np.tile(np.array([[[0, 0, 0, 1]]], np.float32), (n, 1, 1))], 1),
                            with_scale=with_scale)
    assert again["ate"] == got["ate"] and np.array_equal(again["R"], got["R"]) and "err" not in again


def test_align_is_bit_stable():
    pred, gt, _ = R.align_case("n1000")
    a, b = E().align_poses(pred, gt, per_view=True), E().align_poses(pred, gt, per_view=True)
    assert a["ate"] == b["ate"] and a["scale"] == b["scale"] and np.array_equal(a["R"], b["R"])
    assert np.array_equal(a["t"], b["t"]) and torch.equal(a["err"], b["err"])


def test_coincident_predicted_centres():
    _, gt, _ = R.align_case("n257")
    pred = np.repeat(R.align_case("n3")[0][:1], 257, axis=0)
    ref, got = R.umeyama(pred, gt), E().align_poses(pred, gt)
    assert got["status"] == ref["status"] == 3 and got["scale"] == 1.0 and np.array_equal(got["R"], np.eye(3))
    assert abs(got["ate"] - ref["ate"]) <= 1e-9 * ref["ate"] and np.abs(got["t"] - ref["t"]).max() <= 1e-9 * ref["extent"]


# ---------------------------------------------------------------- end to end
def test_small_model_scores_in_bin_zero():
    """The g1_small_56 model in fp32 mode: evaluate_poses(predictions, golden extrinsic) puts every
    pair in bin 0 of the rotation row (the fp32 parity bound of 1e-4 rel-L2 is about 0.006 degrees).
    The translation row is not asserted: synthetic weights give nearly coincident cameras."""
    import torch.nn as nn
    from sailrecon_amd.heads.camera_head import CameraHead
    from sailrecon_amd.models.aggregator import Aggregator
    from sailrecon_amd.utils.pose_enc import pose_encoding_to_extri_intri

    class Hot(nn.Module):
        def __init__(self):
            super().__init__()
            self.aggregator = Aggregator(img_size=56, patch_size=14, embed_dim=384, depth=2, num_heads=6,
                                         patch_embed="dinov2_vits14_reg", intermediate_layer_idx=[0, 1])
            self.camera_head = CameraHead(dim_in=768, trunk_depth=2, num_heads=6)

    torch.manual_seed(0)
    m = Hot().eval()
    m.load_state_dict(rule_state_dict("small_state_dict_keys.json"))
    m = m.to(DEV)
    g = load_npz("g1_small_56.npz")
    images = torch.from_numpy(g["images"]).to(DEV)
    n = int(g["n_views"])
    m.aggregator.generator.manual_seed(0)
    with torch.no_grad():
        feats, _, cam_last = m.aggregator(images, list(range(n)), list(range(n, images.shape[1])),
                                          fix_rank=int(g["fix_rank"]))
        ext, _ = pose_encoding_to_extri_intri(m.camera_head(feats, cam_last)[-1], tuple(images.shape[-2:]))
    predictions = [{"extrinsic": ext[:, k]} for k in range(ext.shape[1])]  # per-view dicts, as forward returns
    res = E().evaluate_poses(predictions, g["extrinsic"])
    n_pairs = ext.shape[1] * (ext.shape[1] - 1) // 2
    print("small model:", {k: v for k, v in res.items() if k not in ("hist", "R", "t")})
    assert res["n_pairs"] == n_pairs >= 1 and res["n_nonfinite"] == 0
    assert res["hist"][0, 0] == n_pairs and res["rra@5"] == 1.0
    assert np.isfinite(res["ate"]) and res["status"] in (0, 2, 3)


def test_tool_matches_evaluate_poses(tmp_path, capsys):
    import json

    import pose_eval as tool
    from demo_imc_forward import save_kitti_poses
    pred, gt = R.case("a33")
    pad = lambda T: np.concatenate([T[:, :3].astype(np.float64), np.tile(np.array([[[0, 0, 0, 1.0]]]), (len(T), 1, 1))], 1)  # noqa: E731
    for name, T in (("pred", pred), ("gt", gt)):
        save_kitti_poses(list(np.linalg.inv(pad(T))), str(tmp_path / f"{name}.txt"))
    files = [str(tmp_path / "pred.txt"), str(tmp_path / "gt.txt")]
    loaded = [tool.load_kitti_w2c(f) for f in files]
    for extra, kw in (([], {}), (["--no-scale", "--thresholds", "10", "20"], dict(with_scale=False, thresholds=(10.0, 20.0)))):
        res = tool.main(files + extra)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        want = E().evaluate_poses(*loaded, **kw)
        assert set(res) == set(want) == set(line)
        for k, v in want.items():
            assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k
            assert np.array_equal(np.asarray(line[k]), np.asarray(v)), k
    # the files hold the stored poses to 9 decimals: the scores are those of the poses themselves
    direct, filed = E().evaluate_poses(pred, gt), E().evaluate_poses(*loaded)
    assert abs(direct["ate"] - filed["ate"]) < 1e-4 and abs(direct["auc@30"] - filed["auc@30"]) < 0.01
