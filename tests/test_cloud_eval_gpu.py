"""Point-cloud scoring on the GPU (sr_cloud_nn, sailrecon_amd/utils/cloud_eval.py) against the fp64
restatement (tests/cloud_eval_ref.py, tests/golden/g18_cloud_eval.npz).

Bounds.  A case's bound is 4 x the largest error of the fp32 restatement of that case against the fp64
one (tests/test_cloud_eval.py prints and checks them); nothing here is taken from what the kernel gives.
Measured kernel errors, as a fraction of the bound (MI355X): DESIGN.md "Scoring point clouds".
"""

import json
import os
import sys

import numpy as np
import pytest
import torch

import cloud_eval_ref as R
from conftest import REPO
from goldens import load_npz

sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNKS = (0, 64, 256)


def run(q, t, *, chunk=0, q_xf=None, t_xf=None, n_bins=None, bin_len=0.0, stats=False):
    """One sr_cloud_nn call: (dist fp32, index) and, if asked, the histogram and the stats, on the host."""
    from sailrecon_amd import ops
    q, t = torch.as_tensor(q).to(DEV).contiguous(), torch.as_tensor(t).to(DEV).contiguous()
    dist = torch.empty(len(q), device=DEV, dtype=torch.float32)
    index = torch.empty(len(q), device=DEV, dtype=torch.int32)
    hist = torch.full((n_bins + 2,), -7, device=DEV, dtype=torch.int32) if n_bins else None  # the call clears it
    st = torch.full((6,), -7.0, device=DEV, dtype=torch.float64) if stats else None
    up = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.float64).to(DEV)  # noqa: E731
    ops.cloud_nn(q, t, query_xform=up(q_xf), target_xform=up(t_xf), dist=dist, index=index, hist=hist, bin_len=bin_len,
                 stats=st, target_chunk=chunk)
    out = [dist.cpu().numpy(), index.cpu().numpy().astype(np.int64)]
    if n_bins:
        out.append(hist.cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
    if stats:
        out.append(st.cpu().numpy())
    return out


def check_against(q, t, d, i, want, bound, what):
    """dist within the bound of the fp64 answer; index in range and as near, in fp64, as the fp64 nearest."""
    err = np.abs(d.astype(np.float64) - want).max()
    print(f"{what}: dist error {err:.3e}, bound {bound:.3e} ({err / bound:.2f})")
    assert err <= bound, what
    assert i.min() >= 0 and i.max() < len(t), what
    own = np.sqrt(((q.astype(np.float64) - t[i].astype(np.float64)) ** 2).sum(1))
    assert np.abs(own - want).max() <= bound, what


@pytest.mark.parametrize("chunk", CHUNKS)
def test_sizes(chunk):
    """Ragged query tiles, ragged last slices, one slice and many."""
    c = R.case("sweep")
    _, bound, _ = R.case_bound("sweep")
    for nt in R.SWEEP_NT:
        t = c["target"][:nt]
        for nq in R.SWEEP_NQ:
            q = c["query"][:nq]
            d, i = run(q, t, chunk=chunk)
            check_against(q, t, d, i, c[f"dist_{nt}"][:nq], bound, f"{nq} x {nt} chunk {chunk}")


def test_ties_take_the_lowest_index_for_every_chunk():
    c = R.case("ties")
    _, bound, _ = R.case_bound("ties")
    first = None
    for chunk in CHUNKS + (128, 448):
        for rep in range(2):
            d, i = run(c["query"], c["target"], chunk=chunk)
            assert np.array_equal(i, c["index"]), chunk  # never the copy 216 places later, never a later corner
            assert np.abs(d - c["dist"]).max() <= bound
            if first is None:
                print(f"ties: dist error {np.abs(d - c['dist']).max():.3e}, bound {bound:.3e}")
            first = (d, i) if first is None else first
            assert d.tobytes() == first[0].tobytes() and np.array_equal(i, first[1]), (chunk, rep)


def test_chunks_and_runs_are_bit_identical():
    c = R.case("hist")
    first = None
    for chunk in CHUNKS + (0,):
        got = run(c["query"], c["target"], chunk=chunk, n_bins=R.HIST_BINS, bin_len=R.HIST_BIN, stats=True)
        first = got if first is None else first
        for a, b in zip(got, first):
            assert a.tobytes() == b.tobytes(), chunk


def test_far_cloud():
    """1e3 from the origin with 1e-3 between neighbours: the direct differences keep every digit."""
    c = R.case("far")
    _, bound, big = R.case_bound("far")
    for chunk in CHUNKS:
        d, i = run(c["query"], c["target"], chunk=chunk)
        check_against(c["query"], c["target"], d, i, c["dist"], bound, f"far chunk {chunk}")
    assert bound < 2e-6 * big


def test_nonfinite_points():
    c = R.case("sweep")
    q, t = c["query"][:700].copy(), c["target"][:1000].copy()
    qi, ti = (5, 333), (17, 640)
    t[list(ti)] = 1e6  # never the nearest: the run the planted one is compared with
    for chunk in CHUNKS:
        d0, i0, h0, s0 = run(q, t, chunk=chunk, n_bins=40, bin_len=0.05, stats=True)
        assert not np.isin(i0, ti).any() and h0[-1] == 0 and s0[4] == 0
        qn, tn = q.copy(), t.copy()
        qn[qi[0], 1], qn[qi[1], 2] = np.nan, np.inf
        tn[ti[0], 0], tn[ti[1], 1] = -np.inf, np.nan
        d1, i1, h1, s1 = run(qn, tn, chunk=chunk, n_bins=40, bin_len=0.05, stats=True)
        assert np.isnan(d1[list(qi)]).all() and (i1[list(qi)] == -1).all()
        assert not np.isin(i1, ti).any()
        keep = np.ones(len(q), bool)
        keep[list(qi)] = False
        assert d1[keep].tobytes() == d0[keep].tobytes() and np.array_equal(i1[keep], i0[keep])
        moved = h0.copy()
        for k in qi:  # the two queries leave their slots for the last one
            moved[min(int(np.float32(d0[k]) / np.float32(0.05)), 40)] -= 1
        moved[-1] += 2
        assert np.array_equal(h1, moved)
        assert s1[0] == 698 and s1[4] == 2 and s1[5] == 0
        want = R.stats_of(d1)
        assert s1[3] == want[3] and abs(s1[1] - want[1]) <= 1e-12 * want[1] and abs(s1[2] - want[2]) <= 1e-12 * want[2]
        # no finite target at all
        tn[:] = np.nan
        d2, i2, h2, s2 = run(qn, tn, chunk=chunk, n_bins=40, bin_len=0.05, stats=True)
        assert np.isnan(d2).all() and (i2 == -1).all() and h2[-1] == 700 and h2[:-1].sum() == 0
        assert s2.tolist() == [0, 0, 0, 0, 700, 0]
    # a minimum that overflows fp32
    big = np.array([[3e38, 3e38, 0]], np.float32)
    d, i = run(-big, big)
    assert np.isnan(d).all() and i.tolist() == [-1]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_histogram_and_stats_against_fp64(chunk):
    c = R.case("hist")
    _, bound, _ = R.case_bound("hist")
    d, i, h, s = run(c["query"], c["target"], chunk=chunk, n_bins=R.HIST_BINS, bin_len=R.HIST_BIN, stats=True)
    check_against(c["query"], c["target"], d, i, c["dist"], bound, f"hist chunk {chunk}")
    assert np.array_equal(h, R.hist_of(c["dist"], R.HIST_BIN, R.HIST_BINS))  # no exclusions: the margin condition
    want = R.stats_of(d)
    assert s[0] == 5000 and s[4] == 0 and s[5] == 0 and s[3] == want[3]
    assert abs(s[1] - want[1]) <= 1e-12 * want[1] and abs(s[2] - want[2]) <= 1e-12 * want[2]
    assert abs(s[3] - c["dist"].max()) <= bound


def test_counts_are_exact_at_scale():
    """2^20 copies of one query against 4,097 targets (4.3e9 pairs): one slot holds every count."""
    c = R.case("sweep")
    q = np.repeat(c["query"][7:8], 1 << 20, axis=0)
    d, i, h, s = run(q, c["target"], n_bins=64, bin_len=0.01, stats=True)
    want = c["dist_4097"][7]
    _, bound, _ = R.case_bound("sweep")
    assert (d == d[0]).all() and (i == c["index_4097"][7]).all() and abs(float(d[0]) - want) <= bound
    slot = int(np.float32(d[0]) / np.float32(0.01))
    assert slot < 64 and h[slot] == 1 << 20 and h.sum() == 1 << 20
    assert s[0] == 2.0 ** 20 and s[4] == 0 and s[3] == float(d[0])
    assert abs(s[1] - 2.0 ** 20 * float(d[0])) <= 1e-12 * s[1]


def test_transform():
    """pred = S^-1(a subset of gt): with S on the predicted side the accuracy is the round trip's rounding,
    the completeness is the restatement's, whichever side of the call the transform is on."""
    c = R.case("xform")
    _, bound, _ = R.case_bound("xform")
    S, pred, gt = c["S"], c["pred"], c["gt"]
    moved = R.xform_points(pred, S)
    # the round trip: pred's rounding to fp32 (half an ulp per axis, scaled by S) and the transform's own
    ulp = lambda x: float(np.spacing(np.float32(np.abs(x).max())))  # noqa: E731
    round_trip = np.sqrt(3) * 0.5 * (S[0] * ulp(pred) + ulp(gt)) * 1.01
    for chunk in CHUNKS:
        d, i = run(pred, gt, chunk=chunk, q_xf=S)
        print(f"transform chunk {chunk}: accuracy max {d.max():.3e}, round trip bound {round_trip:.3e}")
        assert d.max() <= round_trip + bound
        assert np.abs(d - c["acc"]).max() <= bound and np.array_equal(i, c["acc_index"])
        db, ib = run(pred, gt, chunk=chunk, q_xf=np.concatenate([S, [123.0]]))  # sr_pose_align's out: 14 entries
        assert db.tobytes() == d.tobytes()
        # the kernel's transform is the restatement's, bit for bit: the same cloud uploaded moved
        dm, im = run(moved, gt, chunk=chunk)
        assert dm.tobytes() == d.tobytes() and np.array_equal(im, i)
        e, j = run(gt, pred, chunk=chunk, t_xf=S)
        check_against(gt, moved, e, j, c["comp"], bound, f"completeness chunk {chunk}")
        em, jm = run(gt, moved, chunk=chunk)
        assert em.tobytes() == e.tobytes() and np.array_equal(jm, j)
        # mirrored: the targets moved by S against the queries moved by S^-1 ... both moved is the identity of
        # the call without transforms on the moved clouds
        f, k = run(pred, gt, chunk=chunk, q_xf=S, t_xf=np.concatenate([[1.0], np.eye(3).reshape(-1), [0, 0, 0]]))
        assert f.tobytes() == d.tobytes() and np.array_equal(k, i)


def test_cloud_accuracy_matches_the_restatement():
    from sailrecon_amd.utils.cloud_eval import cloud_accuracy, nn_distances
    c = R.case("xform")
    _, bound, _ = R.case_bound("xform")
    taus = (0.05, 0.1, 0.25)
    S = c["S"]
    assert R.hist_margin(c["comp"], bound, 0.05, 16) >= 10 and R.hist_margin(c["acc"], bound, 0.05, 16) >= 10
    for xform in (S, (S[0], S[1:10].reshape(3, 3), S[10:13]), torch.as_tensor(S).to(DEV)):
        res = cloud_accuracy(c["pred"], torch.from_numpy(c["gt"]).to(DEV), thresholds=taus, bin_len=0.05, n_bins=16,
                             xform=xform)
        ref = R.metrics(c["acc"], c["comp"], taus)
        for k, v in ref.items():
            tol = bound if k.split("_")[-1] in ("mean", "rms", "max") or k == "chamfer" else 0.0
            assert abs(res[k] - v) <= tol, (k, res[k], v)
        assert np.array_equal(res["hist_comp"], R.hist_of(c["comp"], 0.05, 16))
        assert (res["n_pred"], res["n_gt"], res["n_nonfinite_pred"], res["n_nonfinite_gt"]) == (1200, 2000, 0, 0)
    # masks and leading shapes
    keep = np.zeros(2000, bool)
    keep[::2] = True
    a = cloud_accuracy(c["pred"].reshape(30, 40, 3), c["gt"].reshape(4, 500, 3), thresholds=taus, bin_len=0.05, n_bins=16,
                       xform=S, gt_valid=keep.reshape(4, 500))
    b = cloud_accuracy(c["pred"], c["gt"][keep], thresholds=taus, bin_len=0.05, n_bins=16, xform=S)
    assert a["n_gt"] == 1000 and all(np.array_equal(a[k], b[k]) for k in a)
    d, i = nn_distances(c["pred"], c["gt"], query_xform=S, return_index=True)
    assert d.is_cuda and d.dtype == torch.float32 and i.dtype == torch.int32
    assert np.array_equal(i.cpu().numpy(), c["subset"])
    assert nn_distances(c["gt"], c["pred"], target_xform=S).shape == (2000,)


def test_evaluate_reconstruction_end_to_end():
    """The unprojection of the golden depth maps (fp32, on the device) scored against the golden point
    maps as the scan, aligned by the golden extrinsics.  The fixture has two views, whose camera centres
    are collinear: the fit's rotation about their line is not unique and status says so (bit 1).  A third
    view (view 0's depth under a third pose, its scan from the fp64 oracle) makes the fit unique; the
    scores are asserted there."""
    from oracle import sfm_oracle as O
    from sailrecon_amd.utils.cloud_eval import evaluate_reconstruction
    from sailrecon_amd.utils.geometry import unproject_depth_map_to_point_map
    g = load_npz("g6_unproject.npz")
    r0 = g["extrinsic"][0, :, :3].astype(np.float64) @ g["extrinsic"][1, :, :3].astype(np.float64).T
    u, _, vt = np.linalg.svd(r0 @ g["extrinsic"][0, :, :3].astype(np.float64))
    e2 = np.concatenate([u @ vt, [[0.3], [-0.7], [1.1]]], axis=1).astype(np.float32)  # a rotation, off the line
    depth = np.concatenate([g["depth"], g["depth"][:1]])
    ext = np.concatenate([g["extrinsic"], e2[None]])
    intr = np.concatenate([g["intrinsic"], g["intrinsic"][:1]])
    scan = np.concatenate([g["points"].astype(np.float64),
                           O.unproject_depth(torch.from_numpy(depth[2:]), torch.from_numpy(ext[2:]),
                                             torch.from_numpy(intr[2:])).numpy()])
    pts = unproject_depth_map_to_point_map(torch.from_numpy(depth).to(DEV), torch.from_numpy(ext).to(DEV),
                                           torch.from_numpy(intr).to(DEV))
    views = [{"point_map_by_unprojection": pts[k:k + 1], "extrinsic": torch.from_numpy(ext[k:k + 1]).to(DEV),
              "dpt_cnf": torch.full((1, 224, 224), 2.0)} for k in range(3)]
    extent = float(np.linalg.norm(scan.reshape(-1, 3).max(0) - scan.reshape(-1, 3).min(0)))
    point_tol = 1e-5  # tests/test_dpt_gpu.py::test_unproject_matches_reference
    kw = dict(thresholds=(0.001, 0.01), bin_len=0.001, n_bins=64)
    res = evaluate_reconstruction(views, scan, gt_poses=ext, **kw)
    print(f"end to end: acc_max {res['acc_max']:.3e} comp_max {res['comp_max']:.3e} chamfer {res['chamfer']:.3e}, "
          f"tolerance {point_tol * extent:.3e} (extent {extent:.2f}); scale - 1 {res['scale'] - 1:.1e} ate {res['ate']:.1e}")
    assert res["status"] == 0 and res["n_pred"] == res["n_gt"] == 3 * 224 * 224
    assert res["precision@0.001"] == 1.0 and res["recall@0.001"] == 1.0 and res["fscore@0.001"] == 1.0
    assert res["acc_max"] < point_tol * extent and res["comp_max"] < point_tol * extent
    assert abs(res["scale"] - 1) < 1e-6 and np.abs(res["R"] - np.eye(3)).max() < 1e-6 and res["ate"] < 1e-6
    # the same without poses, and with a confidence threshold that keeps everything / one view
    plain = evaluate_reconstruction(views, scan, **kw)
    assert "status" not in plain and plain["precision@0.001"] == 1.0 and plain["acc_max"] < point_tol * extent
    conf = evaluate_reconstruction(views, scan, conf_key="dpt_cnf", conf_thresh=1.0, **kw)
    assert conf["n_pred"] == 3 * 224 * 224 and conf["acc_max"] == plain["acc_max"]
    views[1]["dpt_cnf"] = torch.zeros(1, 224, 224)
    conf = evaluate_reconstruction(views, scan, conf_key="dpt_cnf", conf_thresh=1.0, **kw)
    assert conf["n_pred"] == 2 * 224 * 224 and conf["precision@0.001"] == 1.0 and conf["recall@0.001"] < 1.0
    # the fixture as it is: two views
    two = evaluate_reconstruction(views[:2], g["points"], gt_poses=g["extrinsic"], **kw)
    assert two["status"] & 2 and two["ate"] < 1e-6


def test_tool_matches_cloud_accuracy(tmp_path, capsys):
    import cloud_eval as tool
    from demo_imc_forward import save_pointcloud_ply
    from pose_eval import load_kitti_w2c
    from demo_imc_forward import save_kitti_poses
    from sailrecon_amd.utils.cloud_eval import cloud_accuracy, evaluate_reconstruction
    c = R.case("xform")
    files = []
    for name, pts in (("pred", c["pred"]), ("gt", c["gt"])):
        views = [{"point_map_by_unprojection": pts.reshape(1, -1, 40, 3), "images": torch.rand(1, 3, len(pts) // 40, 40)}]
        files.append(str(tmp_path / f"{name}.ply"))
        assert save_pointcloud_ply(views, files[-1]) == len(pts)
    kw = dict(thresholds=(0.5, 1.0), bin_len=0.25, n_bins=64)
    got = tool.main(files + ["--thresholds", "0.5", "1.0", "--bin-len", "0.25", "--bins", "64"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = cloud_accuracy(c["pred"], c["gt"], **kw)
    assert set(got) == set(want) == set(printed)
    for k, v in want.items():
        assert np.array_equal(got[k], v) and np.array_equal(np.asarray(printed[k]), np.asarray(v)), k
    # with poses: the centres of five cameras in both frames, pred = S^-1 gt
    rng = np.random.default_rng(3)
    S = c["S"]
    s, Rm, t = S[0], S[1:10].reshape(3, 3), S[10:13]
    c2w_pred, c2w_gt = [], []
    for _ in range(5):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(-1, 1, 3)
        G = np.eye(4)
        G[:3, :3], G[:3, 3] = Rm @ T[:3, :3], s * Rm @ T[:3, 3] + t
        c2w_pred.append(T), c2w_gt.append(G)
    pp, gp = str(tmp_path / "pred.txt"), str(tmp_path / "gt.txt")
    save_kitti_poses(c2w_pred, pp), save_kitti_poses(c2w_gt, gp)
    got = tool.main(files + ["--pred-poses", pp, "--gt-poses", gp, "--thresholds", "0.5", "--bin-len", "0.25", "--bins", "64"])
    capsys.readouterr()
    views = [{"extrinsic": e[None], "points": c["pred"] if k == 0 else np.zeros((0, 3), np.float32)}
             for k, e in enumerate(load_kitti_w2c(pp))]
    want = evaluate_reconstruction(views, c["gt"], gt_poses=load_kitti_w2c(gp), key="points", thresholds=(0.5,),
                                   bin_len=0.25, n_bins=64)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    assert got["status"] == 0 and abs(got["scale"] - s) < 1e-5 and got["acc_max"] < 1e-4 and got["precision@0.5"] == 1.0
