"""CPU checks of the two-view estimator (ABI 1.16): exports and layouts, every rejection of sr_two_view through the
bindings, the workspace, the restatement (tests/two_view_ref.py) against independent numpy and against the golden
file, its planted answers -- the condition the GPU tests rest on -- and the known limits, asserted as such."""

import ctypes
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import two_view_ref as T
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

V_1_16 = (1 << 16) | 16
NEW = ("sr_two_view_workspace", "sr_two_view")
CSRC = os.path.join(REPO, "self-supervise-sfm_amd", "csrc")


@pytest.fixture(autouse=True, scope="module")
def abi_1_16():
    from sailrecon_amd import _lib
    assert _lib.load().sr_version() >= V_1_16
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
    from sailrecon_amd.utils import two_view
    assert _header_fields("sr_two_view_desc") == [f[0] for f in _lib.TwoViewDesc._fields_]
    assert "1.16: sr_two_view" in open(os.path.join(CSRC, "sr_api.hip")).read()
    assert callable(ops.two_view) and callable(ops.two_view_workspace_bytes)
    assert callable(two_view.estimate_two_view) and callable(two_view.verify_poses)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sr_two_view.hip" in mk
    for obj in ("$(BUILD)/sr_two_view.o", "$(BUILD)/debug/sr_two_view.o"):
        assert re.search(re.escape(obj) + r": \w+ \+= -ffp-contract=off -fhonor-nans", mk), obj
    assert '#include "sr_eval.h"' in open(os.path.join(CSRC, "sr_two_view.hip")).read()


def test_ctypes_layout_matches_c():
    exe = os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")
    r = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 8)), "debug-build"], capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    lay = json.loads(subprocess.run([exe, "layout", "two_view"], capture_output=True, text=True, env=env, check=True).stdout)
    assert set(lay) == {"sr_two_view_desc"}
    c, cls = lay["sr_two_view_desc"], _lib.TwoViewDesc
    assert ctypes.sizeof(cls) == c["size"]
    assert {f[0] for f in cls._fields_} == set(c["fields"])
    for f, off in c["fields"].items():
        assert getattr(cls, f).offset == off, f


P, K, G, H, VIEWS = 70, 1003, 1, 65, 16
A = 0x7f0000000000  # fake, suitably aligned device addresses: validation never dereferences them
PTRS = ("src_coords", "dst_coords", "mask", "intrinsic", "src_idx", "dst_idx", "given_E", "ref_extrinsic", "E", "R", "t", "cost",
        "n_inliers", "n_front", "best", "refined", "status", "inlier_mask", "pose_err", "hyp_idx", "hyp_E", "hyp_cost",
        "hyp_inliers", "workspace")
OUTS = PTRS[8:-1]


def _desc(**kw):
    from sailrecon_amd import _lib
    d = _lib.TwoViewDesc()
    for i, name in enumerate(PTRS):
        setattr(d, name, A + ((i + 1) << 24))
    d.n_views, d.n_pairs, d.n_points, d.n_given, d.n_hyp, d.refine_iters = VIEWS, P, K, G, H, 8
    d.threshold_px, d.seed = 2.0, 2 ** 64 - 1
    d.workspace_bytes = _lib.load().sr_two_view_workspace(P, K, G, H)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(descs):
    """Each call through the bindings' ``check`` on a thread of its own (sr_last_error is per thread): the
    SfmAmdError text, or 0 for a call that passed."""
    from sailrecon_amd import _lib
    lib, got = _lib.load(), []

    def work():
        for d in descs:
            try:
                _lib.check(lib.sr_two_view(None, ctypes.byref(d) if d is not None else None), "sr_two_view")
                got.append(0)
            except _lib.SfmAmdError as e:
                got.append(str(e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    return got


def test_two_view_refuses_every_bad_argument():
    from sailrecon_amd import _lib
    need, huge, nan, inf = _lib.load().sr_two_view_workspace(P, K, G, H), 2 ** 62, float("nan"), float("inf")
    none = {k: None for k in OUTS}
    bad = {
        "null desc": None, "null src_coords": _desc(src_coords=None), "null dst_coords": _desc(dst_coords=None),
        "null intrinsic": _desc(intrinsic=None), "null src_idx": _desc(src_idx=None), "null dst_idx": _desc(dst_idx=None),
        "null workspace": _desc(workspace=None), "n_views 0": _desc(n_views=0), "n_pairs 0": _desc(n_pairs=0),
        "n_pairs -1": _desc(n_pairs=-1), "n_pairs 65536": _desc(n_pairs=65536, n_points=8, workspace_bytes=huge),
        "n_points 0": _desc(n_points=0), "n_points 2^24 + 1": _desc(n_pairs=1, n_points=2 ** 24 + 1, workspace_bytes=huge),
        "P K 2^31": _desc(n_pairs=65535, n_points=2 ** 16, workspace_bytes=huge), "n_given -1": _desc(n_given=-1),
        "n_given 2^20 + 1": _desc(n_given=2 ** 20 + 1, workspace_bytes=huge), "n_hyp -1": _desc(n_hyp=-1),
        "n_hyp 2^20 + 1": _desc(n_hyp=2 ** 20 + 1, workspace_bytes=huge), "no model": _desc(n_given=0, n_hyp=0),
        "G without given_E": _desc(given_E=None), "refine_iters -1": _desc(refine_iters=-1), "refine_iters 33": _desc(refine_iters=33),
        "tau 0": _desc(threshold_px=0.0), "tau -1": _desc(threshold_px=-1.0), "tau NaN": _desc(threshold_px=nan),
        "tau Inf": _desc(threshold_px=inf),
        "partial sums": _desc(n_pairs=65535, n_points=32767, n_given=2 ** 20, n_hyp=2 ** 20, workspace_bytes=huge),
        "pose_err without ref": _desc(ref_extrinsic=None), "no output": _desc(**none),
        "no output, hyp_idx without H": _desc(**dict(none, hyp_idx=A + (99 << 24), n_hyp=0)),
        "workspace short": _desc(workspace_bytes=need - 1), "workspace % 16": _desc(workspace=A + (24 << 24) + 8),
        "given_E % 8": _desc(given_E=A + (7 << 24) + 4), "E % 8": _desc(E=A + (9 << 24) + 4),
        "hyp_E % 8": _desc(hyp_E=A + (21 << 24) + 4),
    }
    for what, msg in zip(bad, _call(list(bad.values()))):
        assert isinstance(msg, str) and "sr_two_view failed (-1): sr_two_view: " in msg, (what, msg)
    # what passes validation fails at the launch only (there is no device)
    ok = [_desc(), _desc(mask=None), _desc(given_E=None, n_given=0), _desc(n_hyp=0), _desc(refine_iters=0), _desc(refine_iters=32),
          _desc(ref_extrinsic=None, pose_err=None), _desc(**dict(none, status=A + (17 << 24))),
          _desc(**dict(none, hyp_cost=A + (22 << 24))), _desc(n_pairs=1, n_points=1), _desc(n_pairs=1, n_points=2 ** 24, workspace_bytes=huge),
          _desc(n_pairs=65535, n_points=8, workspace_bytes=huge), _desc(n_hyp=2 ** 20, workspace_bytes=huge)]
    for msg in _call(ok):
        assert isinstance(msg, str) and "sr_two_view failed (-2)" in msg, msg


def test_workspace_never_shrinks():
    from sailrecon_amd import _lib, ops
    ws = _lib.load().sr_two_view_workspace
    for p in (1, 3, 70, 240, 65535):
        for k in (1, 8, 256, 257, 10000):
            for g in (0, 1, 5):
                for h in (0, 1, 65, 1024):
                    b = ws(p, k, g, h)
                    if g + h == 0:
                        assert b == 0
                        continue
                    nch = (k + 255) // 256
                    assert b > 0 and b % 16 == 0 and b >= 44 * p * k + (84 + 12 * nch) * p * (g + h), (p, k, g, h)
                    for a2 in ((p + 1, k, g, h), (p, k + 1, g, h), (p, k, g + 1, h), (p, k, g, h + 1)):
                        assert a2[0] > 65535 or ws(*a2) >= b, a2
    for args in ((0, 8, 0, 1), (65536, 8, 0, 1), (1, 0, 0, 1), (1, 2 ** 24 + 1, 0, 1), (65535, 2 ** 16, 0, 1), (1, 8, -1, 1),
                 (1, 8, 0, -1), (1, 8, 0, 2 ** 20 + 1), (1, 8, 0, 0), (65535, 32767, 2 ** 20, 2 ** 20)):
        assert ws(*args) == 0 and ops.two_view_workspace_bytes(*args) == 0, args
    assert ops.two_view_workspace_bytes(1, 2 ** 40, 0, 1) == 0
    assert ops.two_view_workspace_bytes(240, 10000, 0, 1024) == ws(240, 10000, 0, 1024) > 0


# ---------------------------------------------------------------- the restatement against independent numpy
def _solved(seed, K=1003, H=512):
    q = T.make_pair(seed, K, 0.3, 0.5)
    xn, a = T.normalise(q["src"], q["dst"], q["K_s"], q["K_d"])
    slots = T.draw_slots(seed, 0, H, K)
    E, kappa = T.solve_hypotheses(xn, slots)
    return q, xn, a, slots, E, kappa


def test_sampling_rule():
    assert int(T.mix64(np.uint64(0))) == 0 and int(T.mix64(np.uint64(1))) == 0x5692161D100B05E5  # splitmix64's finaliser
    s = T.draw_slots(5, 3, 200, 1003)
    assert s.shape == (200, 8) and (s >= 0).all() and (s < 1003).all()
    assert all(len(set(r)) == 8 for r in s.tolist())
    # the rule, spelt out with Python integers for one hypothesis
    p, h, seed, n = 3, 77, 5, 1003
    want, a = [], 0
    while len(want) < 8:
        z = (seed + 0x9E3779B97F4A7C15 * (((p * 2 ** 20 + h) * 64 + a) + 1)) & T.MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & T.MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & T.MASK64
        z ^= z >> 31
        j = ((z >> 32) * n) >> 32
        if j not in want:
            want.append(j)
        a += 1
    assert s[h].tolist() == want
    assert (T.draw_slots(1, 0, 50, 8) >= -1).all() and (T.draw_slots(11, 0, 65, 8)[:, 0] < 0).sum() == 1  # a void one
    assert not np.array_equal(T.draw_slots(5, 3, 20, 1003), T.draw_slots(6, 3, 20, 1003))
    assert not np.array_equal(T.draw_slots(5, 3, 20, 1003), T.draw_slots(5, 4, 20, 1003))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_null_vectors_and_projections_against_svd(seed):
    """The restatement's models meet the bound the GPU's are held to, against numpy.linalg.svd; the generator keeps
    the share of ill-conditioned hypotheses below 2 %."""
    q, xn, a, slots, E, kappa = _solved(seed)
    A = T.rows9(xn[slots.reshape(-1)]).reshape(-1, 8, 9)
    e = np.linalg.svd(A)[2][:, 8, :]
    U, _, Vt = np.linalg.svd(e.reshape(-1, 3, 3))
    Es = (U[:, :, :2] @ Vt[:, :2, :]).reshape(-1, 9)
    keep = kappa <= T.KAPPA_MAX
    assert (~keep).mean() <= 0.02
    ratio = T.angle_up_to_sign(E[keep], Es[keep]) / (2.0 ** -52 * kappa[keep] ** T.HYP_Q)
    print(f"seed {seed}: worst angle / (2^-52 kappa^2) = {ratio.max():.4g}, kappa up to {kappa.max():.4g}")
    assert ratio.max() <= T.C_HYP
    sv = np.linalg.svd(E.reshape(-1, 3, 3), compute_uv=False)
    assert np.abs(sv - [1.0, 1.0, 0.0]).max() < 1e-13
    assert np.abs(np.linalg.norm(E, axis=1) - np.sqrt(2.0)).max() < 1e-13


def test_every_gpu_case_keeps_its_conditioning():
    for name, c in T.gpu_cases().items():
        if c["n_hyp"] == 0:
            continue
        r = T.two_view(c["src"], c["dst"], c["intrinsic"], c["src_idx"], c["dst_idx"], mask=c["mask"], given_E=c["given_E"],
                       n_hyp=c["n_hyp"], tau=c["tau"], iters=0, seed=c["seed"])
        drawn = r["hyp_idx"][..., 0] >= 0
        assert drawn.any() and (r["kappa"][drawn] > T.KAPPA_MAX).mean() <= 0.02, name


def test_scorer_against_pixel_space_sampson():
    """The scorer against F = K_d^-T E K_s^-1 in pixel space at 1e-12 relative.  Relative as the project measures it
    (the error's norm over the reference's, here the maximum norm), and more: element by element 1e-12 of the
    reference wherever it is at least one pixel^2, and 1e-12 pixel^2 below that.  No bound relative to each element
    can hold at a residual near zero: x'^T E x cancels there, for any operation order in fp64.  Measured against the
    extended-precision reference: 3.3e-11 of the value at the smallest residuals for the scorer, 6.3e-10 for the
    same pixel-space formula evaluated in fp64 -- which is why the reference is computed in long double."""
    q, xn, a, slots, E, kappa = _solved(3, H=64)
    models = np.concatenate([E, np.random.default_rng(0).normal(size=(8, 9))])
    r2, _ = T.sampson2(models, xn, a)
    extended = np.finfo(np.longdouble).eps < 1e-18
    for m in range(len(models)):
        want = T.pixel_sampson2(models[m], q["src"], q["dst"], q["K_s"], q["K_d"])
        diff = np.abs(r2[m] - want).astype(np.float64)
        want = want.astype(np.float64)
        if extended:
            assert diff.max() <= 1e-12 * want.max(), m
            assert (diff <= 1e-12 * np.maximum(want, 1.0)).all(), (m, float((diff / np.maximum(want, 1.0)).max()))
        else:  # a platform whose long double is fp64: the reference's own cancellation error is of the order 1e-9
            assert diff.max() <= 1e-9 * want.max(), m
    cost, inl, flags = T.score(models, xn, a, 2.0)
    assert np.allclose(cost, np.minimum(r2, 4.0).sum(axis=1), rtol=1e-12) and np.array_equal(inl, (r2 < 4.0).sum(axis=1))
    # a non-finite model: +Inf and no inliers; a tie goes to the lowest index; nothing finite gives -1
    bad = models.copy()
    bad[0, 3] = np.nan
    bad[5] = bad[2]
    c2, i2, _ = T.score(bad, xn, a, 2.0)
    assert np.isposinf(c2[0]) and i2[0] == 0 and c2[5] == c2[2]
    assert T.select(np.array([np.inf, 3.0, 1.0, 1.0])) == 2 and T.select(np.array([np.inf, np.inf])) == -1


def test_decomposition_against_the_planted_pose():
    for seed in range(4):
        q = T.make_pair(seed, 200, 0.0, 0.0)
        xn, _ = T.normalise(q["src"], q["dst"], q["K_s"], q["K_d"])
        E = T.essential_of(q["R"], q["t"])
        for sign in (1.0, -1.0):
            R, t, nf, counts = T.decompose(sign * E, xn)
            assert nf == 200 and sorted(counts)[2] == 0, counts
            # the planted R is the product of fp32 extrinsics, orthogonal to 2^-24 per entry only: E = [t]x R is
            # that far from essential, some 1e-7 rad = 6e-6 degrees; the bound leaves a decade
            assert T.rot_angle_deg(q["R"], R) < 1e-4 and T.dir_angle_deg(q["t"], t) < 1e-4
            assert abs(np.linalg.det(R) - 1.0) < 1e-12


def test_restatement_against_the_golden_file():
    g = np.load(T.GOLDEN)
    o = T.two_view(g["src"], g["dst"], g["intrinsic"], g["src_idx"], g["dst_idx"], mask=g["mask"], n_hyp=int(g["n_hyp"]),
                   tau=float(g["tau"]), iters=int(g["iters"]), seed=int(g["seed"]), ref_extrinsic=g["ext"])
    for k in ("status", "hyp_idx", "best", "n_inliers", "n_front", "inlier_mask", "refined"):
        assert np.array_equal(o[k], g["out_" + k]), k
    # the scorer on the stored models: bit for bit, on any machine
    for p in range(len(g["src_idx"])):
        vi = np.nonzero(T.valid_flags(g["src"][p], g["dst"][p], g["mask"][p]))[0]
        xn, a = T.normalise(g["src"][p][vi], g["dst"][p][vi], g["intrinsic"][2 * p], g["intrinsic"][2 * p + 1])
        cost, inl, _ = T.score(g["out_hyp_E"][p], xn, a, float(g["tau"]))
        assert np.array_equal(cost.view(np.uint64), g["out_hyp_cost"][p].view(np.uint64))
        assert np.array_equal(inl, g["out_hyp_inliers"][p])
    assert T.angle_up_to_sign(o["hyp_E"].reshape(-1, 9), g["out_hyp_E"].reshape(-1, 9)).max() < 1e-9
    assert T.angle_up_to_sign(o["E"], g["out_E"]).max() < 1e-9
    assert np.allclose(o["cost"], g["out_cost"], rtol=1e-9) and np.allclose(o["pose_err"], g["out_pose_err"], atol=1e-6)


# ---------------------------------------------------------------- planted answers: what the GPU tests rest on
@pytest.mark.parametrize("seed", range(5))
def test_planted_pose_is_recovered(seed):
    q = T.make_pair(seed, 1000, 0.3, 0.5)
    src, dst, intr, si, di, ext = T.stack_pairs([q])
    o = T.two_view(src, dst, intr, si, di, n_hyp=512, tau=2.0, iters=8, seed=seed, ref_extrinsic=ext)
    print(f"seed {seed}: pose error {o['pose_err'][0]}, inliers {o['n_inliers'][0]} of {q['planted'].sum()} planted")
    assert o["status"][0] == 0 and o["pose_err"][0, 0] < 1.0
    assert abs(int(o["n_inliers"][0]) - int(q["planted"].sum())) <= 0.03 * q["planted"].sum()
    assert o["n_front"][0] >= 0.97 * o["n_inliers"][0]


@pytest.mark.parametrize("seed", range(3))
def test_noise_free_pose_is_exact(seed):
    q = T.make_pair(seed, 1000, 0.1, 0.0)
    src, dst, intr, si, di, ext = T.stack_pairs([q])
    o = T.two_view(src, dst, intr, si, di, n_hyp=512, tau=2.0, iters=8, seed=seed, ref_extrinsic=ext)
    assert o["status"][0] == 0 and o["pose_err"][0, 0] < 0.05 and o["pose_err"][0, 1] < 0.05


def test_statuses_of_pairs_without_a_result():
    q = T.make_pair(0, 40, 0.0, 0.2)
    src, dst, intr, si, di, ext = T.stack_pairs([q, q, q])
    mask = np.ones((3, 40), np.uint8)
    mask[1, 7:] = 0
    di = di.copy()
    di[2] = si[2]
    o = T.two_view(src, dst, intr, si, di, mask=mask, n_hyp=16, iters=2, ref_extrinsic=ext)
    assert o["status"].tolist() == [0, 1, 3]
    for p in (1, 2):
        assert np.isnan(o["E"][p]).all() and np.isnan(o["cost"][p]) and o["best"][p] == -1 and o["n_inliers"][p] == 0
        assert (o["hyp_idx"][p] == -1).all() and np.isnan(o["hyp_cost"][p]).all() and not o["inlier_mask"][p].any()
    o = T.two_view(src[:1], dst[:1], intr, si[:1], di[:1], given_E=np.full((1, 2, 9), np.nan), n_hyp=0)
    assert o["status"].tolist() == [2] and np.isposinf(o["hyp_cost"]).all()


# ---------------------------------------------------------------- known limits, asserted as such
@pytest.mark.parametrize("seed", range(3))
def test_planar_scene_is_ambiguous(seed):
    """All points on one plane: every planted inlier is found, but the 8-point system has a three-dimensional null
    space and the pose is one of the plane's family, degrees off.  The inlier ratio does not certify the pose."""
    q = T.make_pair(seed, 1000, 0.1, 0.5, planar=True)
    src, dst, intr, si, di, ext = T.stack_pairs([q])
    o = T.two_view(src, dst, intr, si, di, n_hyp=512, tau=2.0, iters=8, seed=seed, ref_extrinsic=ext)
    assert o["status"][0] == 0 and np.isfinite(o["E"]).all() and np.isfinite(o["R"]).all()
    assert o["n_inliers"][0] >= 0.97 * q["planted"].sum()
    assert o["pose_err"][0, 0] > 1.0  # measured 8.4 .. 9.1 degrees: wrong, and documented as such


@pytest.mark.parametrize("seed", range(3))
def test_pure_rotation_has_no_translation(seed):
    """A zero baseline: every [t]x R explains the correspondences.  The rotation is right, t is arbitrary, and
    the rays are parallel, so about half of the inliers triangulate in front: n_front / n_inliers flags the case."""
    q = T.make_pair(seed, 1000, 0.1, 0.5, baseline=0.0)
    src, dst, intr, si, di, ext = T.stack_pairs([q])
    o = T.two_view(src, dst, intr, si, di, n_hyp=512, tau=2.0, iters=8, seed=seed, ref_extrinsic=ext)
    assert o["status"][0] == 0 and o["pose_err"][0, 0] < 0.1 and np.isnan(o["pose_err"][0, 1])
    assert o["n_inliers"][0] >= 0.97 * q["planted"].sum() and o["n_front"][0] < 0.75 * o["n_inliers"][0]


def test_tool_arguments(tmp_path):
    import two_view as tool
    q = T.make_pair(1, 50, 0.0, 0.2)
    path = os.path.join(tmp_path, "c.npz")
    np.savez(path, src_coords=q["src"][None], dst_coords=q["dst"][None], src_idx=[0], dst_idx=[1])
    a = tool.parse_args([path, "--intrinsics", "500,510,320,240", "--threshold", "1.5", "--hypotheses", "32"])
    assert a.corres == path and a.threshold == 1.5 and a.hypotheses == 32 and a.poses is None
    k = tool.load_intrinsics(a.intrinsics, 2)
    assert k.shape == (2, 3, 3) and k[1, 0, 0] == 500 and k[0, 1, 2] == 240
    kt = os.path.join(tmp_path, "k.txt")
    np.savetxt(kt, np.stack([q["K_s"], q["K_d"]]).reshape(2, 9))
    assert np.array_equal(tool.load_intrinsics(kt, 2), np.stack([q["K_s"], q["K_d"]]))
    pt = os.path.join(tmp_path, "p.txt")
    np.savetxt(pt, q["ext"].reshape(2, 12))
    assert np.array_equal(tool.load_poses(pt), q["ext"])
    with pytest.raises(SystemExit):
        tool.parse_args([])
