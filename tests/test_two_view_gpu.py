"""GPU checks of the two-view estimator (sr_two_view, sailrecon_amd/utils/two_view.py, ABI 1.16) against the numpy
restatement (tests/two_view_ref.py).  The drawn indices are compared exactly; the solved models within
C_HYP 2^-52 kappa^2; everything the scorer produces -- costs, inlier counts, the selection, the mask -- bit for bit,
by feeding the kernel's own models to the restatement's scorer.  The shapes are the smallest that reach every edge:
one and several chunks of 256 correspondences with tails, one and several tiles of 64 and 256 models with tails, 8
and 9 points, given models only, a pair with 7 valid points, a pair of equal views, NaN / Inf coordinates."""

import numpy as np
import pytest
import torch

import two_view_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 16  # entries before and after every output that the call may not write


def _up(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


OUT = (("E", torch.float64, lambda P, K, G, H: 9 * P), ("R", torch.float64, lambda P, K, G, H: 9 * P),
       ("t", torch.float64, lambda P, K, G, H: 3 * P), ("cost", torch.float64, lambda P, K, G, H: P),
       ("n_inliers", torch.int32, lambda P, K, G, H: P), ("n_front", torch.int32, lambda P, K, G, H: P),
       ("best", torch.int32, lambda P, K, G, H: P), ("refined", torch.int32, lambda P, K, G, H: P),
       ("status", torch.int32, lambda P, K, G, H: P), ("inlier_mask", torch.uint8, lambda P, K, G, H: P * K),
       ("pose_err", torch.float64, lambda P, K, G, H: 2 * P), ("hyp_idx", torch.int32, lambda P, K, G, H: 8 * P * H),
       ("hyp_E", torch.float64, lambda P, K, G, H: 9 * P * (G + H)), ("hyp_cost", torch.float64, lambda P, K, G, H: P * (G + H)),
       ("hyp_inliers", torch.int32, lambda P, K, G, H: P * (G + H)))


def run(c, iters=None):
    """One ops.two_view of a case of T.gpu_cases() with every output between guards: dict of numpy arrays.  The
    inputs must come back unchanged and the guards untouched."""
    from sailrecon_amd import ops
    P, K = c["src"].shape[:2]
    G = 0 if c["given_E"] is None else c["given_E"].shape[1]
    H = c["n_hyp"]
    ins = dict(src=_up(c["src"]), dst=_up(c["dst"]), intrinsic=_up(c["intrinsic"]), si=_up(c["src_idx"], torch.int32),
               di=_up(c["dst_idx"], torch.int32), mask=_up(c["mask"]), given=_up(c["given_E"], torch.float64),
               ext=_up(c["ext"]))
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    bufs, outs = {}, {}
    for name, dt, size in OUT:
        n = size(P, K, G, H)
        if n == 0:
            continue
        sentinel = float("nan") if dt == torch.float64 else (201 if dt == torch.uint8 else -77)
        bufs[name] = torch.full((n + 2 * GUARD,), sentinel, device=DEV, dtype=dt)
        outs[name] = bufs[name][GUARD:GUARD + n]
    ops.two_view(ins["src"], ins["dst"], ins["intrinsic"], ins["si"], ins["di"], mask=ins["mask"], given_E=ins["given"],
                 ref_extrinsic=ins["ext"], n_hyp=H, threshold_px=c["tau"], refine_iters=c["iters"] if iters is None else iters,
                 seed=c["seed"], **outs)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(ins[k].view(torch.uint8), v.view(torch.uint8)), f"input {k} was written"
    got = {}
    for name, dt, size in OUT:
        if name not in bufs:
            got[name] = np.zeros(0)
            continue
        b = bufs[name].cpu().numpy()
        g = np.concatenate([b[:GUARD], b[-GUARD:]])
        assert np.isnan(g).all() if dt == torch.float64 else (g == (201 if dt == torch.uint8 else -77)).all(), f"{name}: guard written"
        got[name] = b[GUARD:-GUARD]
    got["hyp_idx"] = got["hyp_idx"].reshape(P, H, 8)
    got["hyp_E"] = got["hyp_E"].reshape(P, G + H, 9)
    for k in ("hyp_cost", "hyp_inliers"):
        got[k] = got[k].reshape(P, G + H)
    for k, w in (("E", 9), ("R", 9), ("t", 3), ("pose_err", 2)):
        got[k] = got[k].reshape(P, w)
    got["inlier_mask"] = got["inlier_mask"].reshape(P, K)
    return got


CASES = T.gpu_cases()
_cache = {}


def gpu(name, iters=None):
    if (name, iters) not in _cache:
        _cache[name, iters] = run(CASES[name], iters)
    return _cache[name, iters]


def ref(name):
    if ("ref", name) not in _cache:
        c = CASES[name]
        _cache["ref", name] = T.two_view(c["src"], c["dst"], c["intrinsic"], c["src_idx"], c["dst_idx"], mask=c["mask"],
                                         given_E=c["given_E"], n_hyp=c["n_hyp"], tau=c["tau"], iters=c["iters"], seed=c["seed"],
                                         ref_extrinsic=c["ext"])
    return _cache["ref", name]


def pair_data(c, p):
    """(vi, xn, a) of pair p of a case, or None for a pair without a result by its indices or its valid count."""
    si, di = int(c["src_idx"][p]), int(c["dst_idx"][p])
    if si == di:
        return None
    vi = np.nonzero(T.valid_flags(c["src"][p], c["dst"][p], None if c["mask"] is None else c["mask"][p]))[0]
    if len(vi) < 8:
        return None
    xn, a = T.normalise(c["src"][p][vi], c["dst"][p][vi], c["intrinsic"][si], c["intrinsic"][di])
    return vi, xn, a


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_status_and_drawn_indices_equal_the_restatement(name):
    g, r = gpu(name), ref(name)
    assert np.array_equal(g["status"], r["status"])
    assert np.array_equal(g["hyp_idx"], r["hyp_idx"])
    bad = np.nonzero((r["status"] == 1) | (r["status"] == 3))[0]
    for p in bad:  # NaN / 0 / -1 in every output of a pair without a result
        assert np.isnan(g["hyp_E"][p]).all() and np.isnan(g["hyp_cost"][p]).all() and (g["hyp_inliers"][p] == 0).all()
    for p in np.nonzero(r["status"] != 0)[0]:
        for k in ("E", "R", "t", "pose_err"):
            assert np.isnan(g[k][p]).all(), (k, p)
        assert np.isnan(g["cost"][p]) and g["n_inliers"][p] == 0 and g["n_front"][p] == 0 and g["best"][p] == -1
        assert g["refined"][p] == -1 and (g["inlier_mask"][p] == 0).all()


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["n_hyp"] > 0])
def test_drawn_models_within_the_conditioning_bound(name):
    """angle(hyp_E, restatement) <= C_HYP 2^-52 kappa^2 for every drawn hypothesis with kappa <= KAPPA_MAX."""
    c, g, r = CASES[name], gpu(name), ref(name)
    G = 0 if c["given_E"] is None else c["given_E"].shape[1]
    worst, left_out, total = 0.0, 0, 0
    for p in np.nonzero(r["status"] != 1)[0]:
        if r["status"][p] == 3:
            continue
        ge, re, kap = g["hyp_E"][p, G:], r["hyp_E"][p, G:], r["kappa"][p]
        void = r["hyp_idx"][p, :, 0] < 0
        assert np.isnan(ge[void]).all()
        keep = ~void & (kap <= T.KAPPA_MAX)
        total += int((~void).sum())
        left_out += int((~void & ~keep).sum())
        assert np.isfinite(ge[keep]).all()
        # singular values (1, 1, 0)
        sv = np.linalg.svd(ge[keep].reshape(-1, 3, 3), compute_uv=False)
        assert np.abs(sv - [1.0, 1.0, 0.0]).max() < 1e-12 if keep.any() else True
        ratio = T.angle_up_to_sign(ge[keep], re[keep]) / (2.0 ** -52 * kap[keep] ** T.HYP_Q)
        worst = max(worst, float(ratio.max()) if keep.any() else 0.0)
    print(f"{name}: worst angle / (2^-52 kappa^2) = {worst:.4g}; {left_out} of {total} hypotheses above kappa {T.KAPPA_MAX:g}")
    assert left_out <= 0.02 * total
    assert worst <= T.C_HYP


@pytest.mark.parametrize("name", list(CASES))
def test_scoring_and_selection_to_the_bit(name):
    """The restatement's scorer on the kernel's own models reproduces hyp_cost, hyp_inliers and best bit for bit."""
    c, g = CASES[name], gpu(name)
    for p in range(c["src"].shape[0]):
        d = pair_data(c, p)
        if d is None:
            continue
        vi, xn, a = d
        cost, inl, _ = T.score(g["hyp_E"][p], xn, a, c["tau"])
        assert same_bits(cost, g["hyp_cost"][p]), (name, p)
        assert np.array_equal(inl, g["hyp_inliers"][p].view(np.uint32)), (name, p)
        assert T.select(cost) == g["best"][p], (name, p)
        assert (g["status"][p] == 2) == (T.select(cost) < 0)
        bad = ~np.isfinite(g["hyp_E"][p]).all(axis=1)
        assert np.isposinf(g["hyp_cost"][p][bad]).all() and (g["hyp_inliers"][p][bad] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_closure_to_the_bit(name):
    """cost, n_inliers and inlier_mask are the restatement's scorer applied to the output E; without refinement E is
    hyp_E[best]; two runs give the same bytes."""
    c, g, g0 = CASES[name], gpu(name), gpu(name, 0)
    again = run(c)
    for k, v in g.items():
        assert np.array_equal(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)), k
    for p in np.nonzero(g["status"] == 0)[0]:
        vi, xn, a = pair_data(c, p)
        for out in (g, g0):
            cost, inl, flags = T.score(out["E"][p], xn, a, c["tau"])
            assert same_bits(cost[0], out["cost"][p]) and inl[0] == out["n_inliers"][p]
            mask = np.zeros(c["src"].shape[1], np.uint8)
            mask[vi[flags[0]]] = 1
            assert np.array_equal(mask, out["inlier_mask"][p])
        assert same_bits(g0["E"][p], g0["hyp_E"][p, g0["best"][p]]) and g0["refined"][p] == 0
        assert same_bits(g0["cost"][p], g0["hyp_cost"][p, g0["best"][p]])
        assert g["best"][p] == g0["best"][p] and g["cost"][p] <= g0["cost"][p]
        assert 0 <= g["refined"][p] <= c["iters"] and (g["refined"][p] > 0) == (g["cost"][p] < g0["cost"][p])
        # R, t: a proper rotation, a unit vector, E = [t]x R up to sign when E is essential; n_front by the restatement
        R, t = g["R"][p].reshape(3, 3), g["t"][p]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12 and abs(t @ t - 1) < 1e-12
        inl_xn = xn[g["inlier_mask"][p][vi] != 0]
        assert T.front_count(R, t, inl_xn) == g["n_front"][p]
        sv = np.linalg.svd(g["E"][p].reshape(3, 3), compute_uv=False)
        if np.abs(sv - [1, 1, 0]).max() < 1e-12:
            Et = (T.skew(t) @ R).reshape(9)
            assert min(np.abs(Et - g["E"][p]).max(), np.abs(Et + g["E"][p]).max()) <= 1e-12
            assert g["n_front"][p] == max(T.decompose(g["E"][p], inl_xn)[3])
        Rr, tr = T.relative_pose(c["ext"], int(c["src_idx"][p]), int(c["dst_idx"][p]))
        e = torch.tensor([T.rot_angle_deg(Rr, R), T.dir_angle_deg(tr, t)], dtype=torch.float64)
        assert np.allclose(g["pose_err"][p], e.numpy(), rtol=0, atol=1e-9, equal_nan=True)


def _torch_pose_err(ext, si, di, R, t):
    e = torch.as_tensor(ext).double()
    Rr = e[di, :, :3] @ e[si, :, :3].T
    tr = e[di, :, 3] - Rr @ e[si, :, 3]
    Q = Rr.T @ torch.as_tensor(R)
    v = torch.stack([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    rot = torch.rad2deg(torch.atan2(0.5 * v.norm(), 0.5 * (Q.trace() - 1.0)))
    tt = torch.as_tensor(t)
    tra = torch.rad2deg(torch.atan2(torch.linalg.cross(tr, tt).norm(), tr @ tt))
    return float(rot), float(tra)


def test_refinement_from_a_perturbed_pose():
    """G = 1, H = 0: the refined E within REFINE_TOL of the restatement's, the cost never above the start model's."""
    P, K = 3, 1003
    src, dst, intr, si, di, ext = T._scene([61, 62, 63], K)
    given = np.zeros((P, 1, 9))
    for p in range(P):
        R, t = T.relative_pose(ext, 2 * p, 2 * p + 1)
        given[p, 0] = T.essential_of(T.rodrigues([1, 2, 3], 1.0) @ R, t + 0.05 * np.array([1.0, -1.0, 0.5]))
    c = dict(src=src, dst=dst, intrinsic=intr, src_idx=si, dst_idx=di, ext=ext, mask=None, given_E=given, n_hyp=0, iters=8,
             seed=0, tau=2.0)
    g = run(c)
    r = T.two_view(src, dst, intr, si, di, given_E=given, n_hyp=0, tau=2.0, iters=8, ref_extrinsic=ext)
    ang = T.angle_up_to_sign(g["E"], r["E"])
    print(f"refinement: angles to the restatement {ang}, rounds {g['refined']} / {r['refined']}, "
          f"costs {g['cost']} from {g['hyp_cost'][:, 0]}, pose errors {g['pose_err'].tolist()}")
    assert (g["status"] == 0).all() and (g["cost"] <= g["hyp_cost"][:, 0]).all()
    assert (g["cost"] < g["hyp_cost"][:, 0]).all() and (g["refined"] > 0).all()
    assert np.array_equal(g["refined"], r["refined"])
    assert ang.max() <= T.REFINE_TOL
    assert (g["pose_err"][:, 0] < 1.0).all()


def test_planted_scenes_end_to_end():
    """K = 1000, 30 % outliers, 0.5 px noise, tau 2, H 512, 8 rounds, five pairs: rotation within 1 degree."""
    from sailrecon_amd.utils.two_view import estimate_two_view
    pairs = [T.make_pair(s, 1000, 0.3, 0.5) for s in range(5)]
    src, dst, intr, si, di, ext = T.stack_pairs(pairs)
    o = estimate_two_view(src, dst, intr, si, di, threshold_px=2.0, hypotheses=512, refine_iters=8, seed=0, ref_extrinsic=ext)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in o.items()}
    print("planted scenes: pose errors", o["pose_err"].tolist(), "inliers", o["n_inliers"].tolist())
    assert (o["status"] == 0).all()
    assert (o["pose_err"][:, 0] < 1.0).all()
    for p, q in enumerate(pairs):
        assert abs(int(o["n_inliers"][p]) - int(q["planted"].sum())) <= 0.03 * q["planted"].sum()
        R, t = o["R"][p], o["t"][p]
        Et = (T.skew(t) @ R).reshape(9)
        assert min(np.abs(Et - o["E"][p].reshape(9)).max(), np.abs(Et + o["E"][p].reshape(9)).max()) <= 1e-12
        xn, _ = T.normalise(q["src"], q["dst"], q["K_s"], q["K_d"])
        inl = xn[o["inlier_mask"][p]]
        assert o["n_front"][p] == T.decompose(o["E"][p].reshape(9), inl)[2] == T.front_count(R, t, inl)
        assert np.allclose(o["pose_err"][p], _torch_pose_err(ext, 2 * p, 2 * p + 1, R, t), rtol=0, atol=1e-9)


def test_init_extrinsic_bounds_the_cost():
    from sailrecon_amd.utils.two_view import estimate_two_view
    pairs = [T.make_pair(s, 257, 0.3, 0.5) for s in range(70, 73)]
    src, dst, intr, si, di, ext = T.stack_pairs(pairs)
    noisy = ext.copy()
    noisy[:, :, 3] += np.float32(0.02)
    for hyp in (0, 64):
        o = estimate_two_view(src, dst, intr, si, di, hypotheses=hyp, refine_iters=4, init_extrinsic=noisy, ref_extrinsic=ext,
                              return_hypotheses=True)
        assert (o["status"] == 0).all() and (o["cost"] <= o["init_cost"]).all()
        assert torch.equal(o["init_cost"], o["hyp_cost"][:, 0])
        assert o["hyp_E"].shape == (3, 1 + hyp, 3, 3) and o["inlier_mask"].dtype == torch.bool


def test_verify_poses_on_a_synthetic_batch():
    from sailrecon_amd.train.data import synthetic_batch
    from sailrecon_amd.utils.two_view import verify_poses
    b = synthetic_batch(4, n_points=300, size=518, seed=3)
    ext = torch.eye(4)[None, :3].repeat(4, 1, 1).clone()
    ext[:, :, 3] = torch.randn(4, 3, generator=torch.Generator().manual_seed(1))
    intr = torch.tensor([[400.0, 0, 259], [0, 400.0, 259], [0, 0, 1]]).repeat(4, 1, 1)
    out = verify_poses((ext, intr), b, hypotheses=64, refine_iters=2)
    for k in ("rot_err", "trans_err", "inlier_ratio", "status", "estimate", "n_pairs", "n_estimated", "rra@5", "rta@15",
              "auc@30", "hist"):
        assert k in out, k
    assert out["n_pairs"] == 3 and out["rot_err"].shape == (3,) and out["inlier_ratio"].shape == (3,)
    assert 0 <= out["rra@5"] <= out["rra@15"] <= out["rra@30"] <= 1
    assert out["n_estimated"] == int((out["status"] == 0).sum())
