"""Pose scoring (sr_pose_pair_errors / sr_pose_align, sailrecon_amd/utils/pose_eval.py), CPU side: the
fp64 restatement of the contract (tests/pose_eval_ref.py) against the reference's own relative poses
(tests/golden/make_golden_pose_eval.py -> g14_pose_eval.npz), the bounds the GPU test uses and the
margin condition that makes histogram equality hold with no exclusions, known answers, the Umeyama
fit's edge cases, the ctypes mirror of the new ABI structs and the argument checks (no GPU is touched).

Bounds.  Per case the fp32 restatement (every step rounded to fp32) is compared with the fp64 one;
4 x its largest error is the bound the GPU kernel must meet on that case (printed here, copied into
DESIGN.md).  Each must stay below 1e-3 degrees: the acos form of the rotation error is off by 2.7e-2
degrees at errors <= 0.1 degrees, so a kernel using it cannot pass.
"""

import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import pose_eval_ref as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))


# ---------------------------------------------------------------- the restatement against the reference
def test_closed_form_relative_pose_matches_reference():
    z = R._npz()
    pred, gt = R.case(str(z["rel/case"]))
    i, j = z["rel/pair_i"].astype(np.int64), z["rel/pair_j"].astype(np.int64)
    assert (i > j).any() and (i == j).any() and len(set(zip(i.tolist(), j.tolist()))) < len(i)
    for key, T in (("gt", gt), ("pred", pred)):
        ref, inv64 = z[f"rel/{key}_ref"], z[f"rel/{key}_inv64"]
        assert ref.dtype == np.float32 and inv64.dtype == np.float64
        bound = 4.0 * np.abs(ref - inv64).max()
        Rr, t = R.relative(R.as34(T).astype(np.float64), i, j)
        err = max(np.abs(Rr - ref[:, :3, :3]).max(), np.abs(t - ref[:, :3, 3]).max())
        print(f"relative pose ({key}): reference fp32 vs fp64 inverse {bound / 4:.3e}, bound {bound:.3e}, "
              f"closed form vs reference {err:.3e}")
        assert err <= bound
        assert np.abs(ref[:, 3] - np.array([0, 0, 0, 1.0])).max() <= bound  # the inverse's own noise


@pytest.mark.parametrize("name", list(R.PAIR_CASES))
def test_fp32_restatement_error_gives_the_gpu_bound(name):
    rb, tb = R.case_bounds(name)
    rot, trans = R.case_errors(name)
    print(f"{name}: fp32 restatement max error rot {rb / 4:.3e} trans {tb / 4:.3e} deg -> GPU bounds rot {rb:.3e} "
          f"trans {tb:.3e} deg; median rot {np.median(rot):.3e} trans {np.median(trans):.3e} deg")
    assert 0 < rb < 1e-3 and 0 < tb < 1e-3
    pred, gt = R.case(name)
    assert pred.shape == (R.PAIR_CASES[name]["n"], 3, 4) and gt.shape == (R.PAIR_CASES[name]["n"], 4, 4)
    assert pred.dtype == np.float32 and gt.dtype == np.float32


@pytest.mark.parametrize("k", range(len(R.RUNS)))
def test_runs_keep_the_margin(k):
    run = R.RUNS[k]
    m = R.run_margin(run)
    print(f"{run}: margin {m:.1f} x bound")
    assert m >= R.MARGIN  # no exclusions


def test_cases_exercise_their_risks():
    assert os.path.getsize(R.GOLDEN) < 64 * 1024
    assert {r["n"] for r in R.RUNS} >= {2, 3, 33, 65, 130}
    rot, trans = R.run_errors(R.RUNS[3])  # n_bins = 5: most pairs overflow
    assert R.RUNS[3]["n_bins"] == 5 and (np.maximum(rot, trans) >= 5).mean() > 0.5 and (rot < 5).any()
    _, t_off = R.case_errors("amb12", False)
    _, t_on = R.case_errors("amb12", True)
    assert (t_off > 90).sum() >= 10 and t_on.max() <= 90 and np.allclose(t_on[t_off > 90], 180 - t_off[t_off > 90])
    for name, rad in (("small3", 1e-3), ("small5", 1e-5)):
        rot, _ = R.case_errors(name)
        assert 0.1 * np.degrees(rad) < np.median(rot) and rot.max() < 2.1 * np.degrees(rad)
    # the acos form would miss these cases' bounds: its fp32 error at such angles is the rounding of
    # cos(x) near 1, 2^-24 / sin(x) radians
    assert np.degrees(2.0 ** -24 / np.radians(R.case_errors("small3")[0].max())) > 10 * R.case_bounds("small3")[0]
    pred, gt = R.case("a33")
    c = R.centres(gt)
    d = np.linalg.norm(c[:, None] - c[None], axis=-1) + 10 * np.eye(len(c))
    assert d.min() >= 1 - 1e-5 and np.abs(c).max() <= 10 + 1e-5


# ---------------------------------------------------------------- known answers
def _rz(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def test_pred_equals_gt_and_world_similarity():
    pred, gt = R.case("a33")
    rot, trans = R.errors(gt, gt)
    assert rot.max() < 1e-9 and trans.max() < 1e-5  # fp64 on identical inputs
    rb, tb = R.case_bounds("a33")
    r32, t32 = R.errors(gt, gt, dtype=np.float32)
    print(f"pred = gt in fp32: rot {r32.max():.3e} trans {t32.max():.3e} deg")
    assert r32.max() <= rb and t32.max() <= tb
    # the same cameras in a world moved by x' = s Q x + u: R' = R Q^T, c' = s Q c + u.  The moved poses
    # are rounded to fp32: 2^-24 relative on |t| <= 60 over baselines >= 1.7 is <= 2e-4 degrees
    rng = np.random.default_rng(5)
    Q, s, u = R.rotations(rng, 1)[0], 1.7, np.array([3.0, -1.0, 2.0])
    T = R.as34(gt).astype(np.float64)
    moved = R.poses(T[:, :, :3] @ Q.T, s * R.centres(gt) @ Q.T + u, False)
    rot, trans = R.errors(moved, gt)
    print(f"world similarity: rot {rot.max():.3e} trans {trans.max():.3e} deg")
    assert rot.max() < 1e-4 and trans.max() < 1e-3


@pytest.mark.parametrize("angle", [10.0, 100.0])
def test_single_axis_rotation(angle):
    c = np.array([[0.0, 0, 0], [2.0, 1, 0], [0, 3.0, 1]])
    gt = R.poses(np.tile(np.eye(3), (3, 1, 1)), c, True)
    Rp = np.tile(np.eye(3), (3, 1, 1))
    Rp[1] = _rz(angle)
    pred = R.poses(Rp, c, False)
    for dt in (np.float64, np.float32):
        rot, _ = R.errors(pred, gt, dtype=dt)
        assert np.allclose(rot, [angle, 0.0, angle], atol=2e-5), (dt, rot)  # pairs (0,1) (0,2) (1,2)


def test_translation_angles_and_degenerate_rules():
    eye = np.tile(np.eye(3), (2, 1, 1))
    gt = R.poses(eye, np.array([[0.0, 0, 0], [1.0, 0, 0]]), True)
    at = lambda deg: R.poses(eye, np.array([[0.0, 0, 0], [np.cos(np.radians(deg)), np.sin(np.radians(deg)), 0]]), True)  # noqa: E731
    for deg, on, off in ((30, 30, 30), (150, 30, 150), (180, 0, 180)):
        assert abs(R.errors(at(deg), gt, trans_ambiguity=True)[1][0] - on) < 1e-5
        assert abs(R.errors(at(deg), gt, trans_ambiguity=False)[1][0] - off) < 1e-5
    collapsed = R.poses(eye, np.zeros((2, 3)), True)  # every predicted camera in one point
    for dt in (np.float64, np.float32):
        assert R.errors(collapsed, gt, trans_ambiguity=True, dtype=dt)[1][0] == 90.0
        assert R.errors(collapsed, gt, trans_ambiguity=False, dtype=dt)[1][0] == 180.0
        assert R.errors(gt, collapsed, trans_ambiguity=False, dtype=dt)[1][0] == 180.0
        assert R.errors(collapsed, collapsed, dtype=dt)[1][0] == 0.0


def test_nonfinite_and_out_of_range_pairs():
    pred, gt = R.case("a33")
    pred = pred.copy()
    pred[5, 1, 2], pred[5, 0, 3] = np.nan, np.inf
    rot, trans = R.errors(pred, gt)
    i, j = R.all_pairs(len(pred))
    hit = (i == 5) | (j == 5)
    assert hit.sum() == len(pred) - 1 and np.isnan(rot[hit]).all() and np.isnan(trans[hit]).all()
    clean = R.case_errors("a33")
    assert np.array_equal(rot[~hit], clean[0][~hit]) and np.array_equal(trans[~hit], clean[1][~hit])
    h, h0 = R.histogram(rot, trans, 5.0, 36), R.histogram(*clean, 5.0, 36)
    assert (h[:, -1] == len(pred) - 1).all() and (h.sum(1) == h0.sum(1)).all() and (h[:, :-1] <= h0[:, :-1]).all()
    pi, pj = R.explicit_pairs(len(pred))
    rot, trans = R.errors(*R.case("a33"), (pi, pj))
    assert np.isnan(rot[pi == len(pred)]).all() and np.isfinite(rot[pi < len(pred)]).all()
    assert (rot[pi == pj] == 0).all() and (trans[pi == pj] == 0).all()
    k = np.flatnonzero((pi == 3) & (pj == 1))
    assert len(k) == 2 and rot[k[0]] == rot[k[1]]  # a repeat
    fwd, back = np.flatnonzero((pi == 0) & (pj == 3))[0], np.flatnonzero((pi == 3) & (pj == 0))
    assert len(back) == 0 or abs(rot[fwd] - rot[back[0]]) < 1e-9


def test_auc_of_a_hand_built_histogram():
    from sailrecon_amd.utils.pose_eval import accuracy_from_hist
    # 10 pairs, bin_deg 2, n_bins 4: max errors in bins 0 0 0 1 1 3 | 2 overflow | 2 non-finite
    h = np.zeros((3, 6), np.int64)
    h[2] = [3, 2, 0, 1, 2, 2]
    h[0] = [5, 1, 0, 0, 2, 2]
    h[1] = [3, 2, 1, 0, 2, 2]
    want = {"n_pairs": 10, "n_nonfinite": 2, "rra@2": 0.5, "rta@2": 0.3, "auc@2": 0.3,
            "rra@4": 0.6, "rta@4": 0.5, "auc@4": (0.3 + 0.5) / 2,
            "rra@8": 0.6, "rta@8": 0.6, "auc@8": (0.3 + 0.5 + 0.5 + 0.6) / 4}
    for f in (R.accuracy, accuracy_from_hist):
        got = f(h, (2, 4, 8), 2.0)
        for k, v in want.items():
            assert got[k] == pytest.approx(v, abs=1e-15), (f.__name__, k)
        with pytest.raises(ValueError, match="multiple"):
            f(h, (3,), 2.0)
        with pytest.raises(ValueError):
            f(h, (10,), 2.0)  # beyond the histogram
    # uint32 counts stored as int32 read back as the counts
    big = np.zeros((3, 3), np.int64)
    big[:, 0] = 3_000_000_000
    assert accuracy_from_hist(big.astype(np.uint32).view(np.int32), (1,), 1.0)["n_pairs"] == 3_000_000_000
    assert R.histogram(np.array([0.5, 3.0, 9.0, np.nan]), np.array([1.5, 0.1, 0.2, 0.3]), 2.0, 4).tolist() == \
        [[1, 1, 0, 0, 1, 1], [3, 0, 0, 0, 0, 1], [1, 1, 0, 0, 1, 1]]


# ---------------------------------------------------------------- Umeyama
@pytest.mark.parametrize("name", ["n3", "n4", "n257"])
def test_umeyama_recovers_a_known_similarity(name):
    pred, gt, truth = R.align_case(name, 0.0)
    for with_scale in (True, False):
        u = R.umeyama(pred, gt, with_scale)
        if with_scale:  # centres come from fp32 poses: 2^-24 relative on magnitudes <= 30
            assert abs(u["scale"] - truth["scale"]) < 1e-5 and np.abs(u["R"] - truth["R"]).max() < 1e-5
            assert np.abs(u["t"] - truth["t"]).max() < 1e-4 and u["ate"] < 1e-4 and u["status"] == 0
        else:
            assert u["scale"] == 1.0 and np.abs(u["R"] - truth["R"]).max() < 1e-5 and u["ate"] > 0.1
        assert abs(np.linalg.det(u["R"]) - 1) < 1e-12 and u["err"].shape == (len(pred),)


def test_umeyama_mirrored_needs_the_sign_fix():
    pred, gt, _ = R.align_case("n4_mirror", 0.0)
    fixed, naive = R.umeyama(pred, gt), R.umeyama(pred, gt, sign_fix=False)
    print(f"mirrored: det R {np.linalg.det(fixed['R']):+.6f} ate {fixed['ate']:.4f}; without the fix det R "
          f"{np.linalg.det(naive['R']):+.6f} ate {naive['ate']:.3e}")
    assert abs(np.linalg.det(fixed["R"]) - 1) < 1e-12 and fixed["ate"] > 0.1
    assert abs(np.linalg.det(naive["R"]) + 1) < 1e-12 and naive["ate"] < 1e-4


def test_umeyama_status_bits():
    pred, gt, _ = R.align_case("n1")
    u = R.umeyama(pred, gt)
    assert u["status"] == 3 and u["scale"] == 1.0 and np.array_equal(u["R"], np.eye(3)) and u["ate"] < 1e-12
    assert np.allclose(u["t"], R.centres(gt)[0] - R.centres(pred)[0], atol=1e-12)
    pred, gt, _ = R.align_case("n2")
    u = R.umeyama(pred, gt)
    assert u["status"] == 2 and u["ate"] < 1e-9 and abs(np.linalg.det(u["R"]) - 1) < 1e-12
    pred, gt, _ = R.align_case("n3")  # planar: one zero singular value, the rotation is still unique
    u = R.umeyama(pred, gt)
    assert u["status"] == 0 and u["sigma"][2] < 1e-12 * u["sigma"][0]
    same = np.repeat(pred[:1], 5, axis=0)  # coincident predicted centres
    assert R.umeyama(same, R.align_case("n257")[1][:5])["status"] == 3
    for name in R.ALIGN_CASES[2:]:
        sig = R.umeyama(*R.align_case(name)[:2])["sigma"]
        assert sig[0] >= 1.1 * sig[1] and (name == "n3" or sig[1] >= 1.1 * sig[2]), (name, sig)


# ---------------------------------------------------------------- ABI
def test_ctypes_mirror_of_the_pose_eval_structs():
    from sailrecon_amd import _lib
    src = open(os.path.join(REPO, "include", "sfm_amd.h")).read()
    for cname, cls in (("sr_pose_pairs_desc", _lib.PosePairsDesc), ("sr_pose_align_desc", _lib.PoseAlignDesc)):
        body = src.split(f"typedef struct {cname} {{")[1].split(f"}} {cname};")[0]
        body = "\n".join(line.split("/*")[0] for line in body.splitlines())
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
        assert names == [f[0] for f in cls._fields_], cname
    assert "sr_pose_pair_errors" in _lib.EXPORTED and "sr_pose_align" in _lib.EXPORTED
    assert _lib.load().sr_version() >= (1 << 16) | 9
    for entry in ("sr_pose_pair_errors", "sr_pose_align"):  # each entry cites its sources
        doc = src.split(f"int {entry}(")[0][-6000:]
        assert "geometry.py:240-282" in doc and "demo_imc_forward.py:109-128" in doc, entry


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "self-supervise-sfm_amd", "csrc"), "-j",
                        str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "pose_eval"], capture_output=True, text=True, env=env,
                                    check=True).stdout)
    mirror = {"sr_pose_pairs_desc": _lib.PosePairsDesc, "sr_pose_align_desc": _lib.PoseAlignDesc}
    assert set(lay) == set(mirror)
    for name, cls in mirror.items():
        assert ctypes.sizeof(cls) == lay[name]["size"], name
        assert {f[0] for f in cls._fields_} == set(lay[name]["fields"])
        for f, off in lay[name]["fields"].items():
            assert getattr(cls, f).offset == off, (name, f)


def _rejected(calls):
    """Run the calls on a thread of their own: sr_last_error is per thread, and test_abi.py expects
    the main thread's to be empty."""
    from sailrecon_amd import _lib
    lib, got = _lib.load(), []

    def work():
        for entry, desc in calls:
            rc = getattr(lib, entry)(None, ctypes.byref(desc) if desc is not None else None)
            got.append((rc, lib.sr_last_error()))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_einval_paths():
    from sailrecon_amd import _lib

    def pairs(**kw):
        d = _lib.PosePairsDesc()
        d.pred, d.gt, d.hist, d.pred_stride, d.gt_stride = 4096, 8192, 12288, 12, 16
        d.n_views, d.n_bins, d.bin_deg, d.trans_ambiguity = 33, 180, 1.0, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def align(**kw):
        d = _lib.PoseAlignDesc()
        d.pred, d.gt, d.out, d.status, d.pred_stride, d.gt_stride, d.n_views = 4096, 8192, 12288, 16384, 12, 16, 33
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad_pairs = [pairs(pred=None), pairs(gt=None), pairs(hist=None), pairs(n_views=0), pairs(n_views=-4),
                 pairs(n_views=65536), pairs(pred_stride=9), pairs(gt_stride=24), pairs(n_bins=0), pairs(n_bins=1025),
                 pairs(bin_deg=0.0), pairs(bin_deg=-1.0), pairs(bin_deg=float("nan")), pairs(bin_deg=float("inf")),
                 pairs(pair_i=4096, n_pairs=3), pairs(pair_j=4096, n_pairs=3), pairs(pair_i=4096, pair_j=8192, n_pairs=0)]
    bad_align = [align(pred=None), align(gt=None), align(out=None), align(status=None), align(n_views=0),
                 align(n_views=65536), align(pred_stride=0), align(gt_stride=15), align(out=12292)]
    calls = ([("sr_pose_pair_errors", None), ("sr_pose_align", None)] + [("sr_pose_pair_errors", d) for d in bad_pairs]
             + [("sr_pose_align", d) for d in bad_align])
    got = _rejected(calls)
    assert len(got) == len(calls)
    for (entry, _), (rc, msg) in zip(calls, got):
        assert rc == -1 and msg.startswith(entry.encode() + b":"), (entry, rc, msg)


# ---------------------------------------------------------------- Python argument checks (no upload, no launch)
def test_python_argument_checks():
    from sailrecon_amd.utils import pose_eval as E
    ok3, ok4 = np.zeros((5, 3, 4), np.float32), torch.zeros(5, 4, 4)
    for f in (E.pose_pair_errors, E.pose_accuracy, E.align_poses, E.evaluate_poses):
        with pytest.raises(ValueError, match="pred must be"):
            f(np.zeros((5, 3, 3)), ok4)
        with pytest.raises(ValueError, match="gt must be"):
            f(ok3, torch.zeros(5, 4))
        with pytest.raises(ValueError, match="gt must be"):
            f(ok3, torch.zeros(2, 5, 4, 4))  # only a leading 1 is dropped
        with pytest.raises(ValueError, match="gt has 4 views, pred has 5"):
            f(ok3, torch.zeros(1, 4, 3, 4))
        with pytest.raises(ValueError, match="pred has no views"):
            f(np.zeros((0, 3, 4)), ok4)
        with pytest.raises(ValueError, match=r"pred\[1\] has no 'extrinsic'"):
            f([{"extrinsic": torch.zeros(1, 3, 4)}, {"intrinsic": 0}], ok4[:2])
        with pytest.raises(ValueError, match=r"gt\[0\]\['extrinsic'\] must end in"):
            f(ok3[:1], [{"extrinsic": torch.zeros(3, 3)}])
        with pytest.raises(ValueError, match="at most 65535"):
            f(torch.zeros(65536, 3, 4), torch.zeros(65536, 3, 4))
    for f in (E.pose_pair_errors, E.pose_accuracy, E.evaluate_poses):
        with pytest.raises(ValueError, match="pairs"):
            f(ok3, ok4, pairs=np.zeros((4, 3), np.int64))
        with pytest.raises(ValueError, match="pairs"):
            f(ok3, ok4, pairs=(np.zeros(4, np.int64), np.zeros(3, np.int64)))
        with pytest.raises(ValueError, match="integer"):
            f(ok3, ok4, pairs=(np.zeros(4), np.zeros(4)))
    for f in (E.pose_accuracy, E.evaluate_poses):
        with pytest.raises(ValueError, match="multiple of bin_deg"):
            f(ok3, ok4, thresholds=(5, 7.5))
        with pytest.raises(ValueError, match="beyond the histogram"):
            f(ok3, ok4, thresholds=(5, 15), n_bins=10)
        with pytest.raises(ValueError, match="n_bins"):
            f(ok3, ok4, n_bins=1025)
        with pytest.raises(ValueError, match="n_bins"):
            f(ok3, ok4, n_bins=0)
        with pytest.raises(ValueError, match="bin_deg"):
            f(ok3, ok4, bin_deg=0.0)
    # the accepted forms agree on what they hold
    dicts = [{"extrinsic": torch.from_numpy(ok3[k:k + 1])} for k in range(5)]
    assert tuple(E._as_poses(dicts, "pred").shape) == (5, 3, 4)
    assert tuple(E._as_poses(ok4[None], "gt").shape) == (5, 4, 4)


def test_kitti_files_round_trip(tmp_path):
    from demo_imc_forward import save_kitti_poses
    import pose_eval as tool
    _, gt = R.case("a33")
    c2w = [np.linalg.inv(T.astype(np.float64)) for T in gt]
    save_kitti_poses(c2w, str(tmp_path / "gt.txt"))
    back = tool.load_kitti_w2c(str(tmp_path / "gt.txt"))
    assert back.shape == gt.shape and back.dtype == np.float32
    assert np.abs(back - gt).max() < 1e-5  # 9 decimals of a camera-to-world pose, inverted in fp64
    (tmp_path / "bad.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError, match="12"):
        tool.load_kitti_w2c(str(tmp_path / "bad.txt"))
