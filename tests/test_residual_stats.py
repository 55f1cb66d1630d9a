"""Residual diagnostics of the training loss (sr_imc_residual_stats, train.loss.residual_stats /
summarize), CPU side: the restatement of the contract (tests/residual_stats_ref.py) against the
reference's own get_frame_statistics (tests/golden/make_golden_residual_stats.py ->
g17_frame_stats.npz), the per-case bounds the GPU test uses, the properties of the stored cases those
checks lean on, summarize on hand-made arrays, and the ABI (no GPU is touched).

Bounds.  Per case the fp32 run of the restatement (every step rounded to fp32, the cumulative sum
included: torch.cumsum on the CPU keeps a double accumulator, so it is written as a loop) is compared
with the fp64 run; 4 x its largest error is what the GPU kernel must meet on that case.  Measured on
the build host (the figures move by tens of percent with the torch build; the bounds are computed where the
test runs) (fp32 restatement vs fp64; residuals as |r - r64| / max(r64, 1 px), cdf / pdf absolute):
  case          reproj    fixed     sampson   cdf       pdf
  dummy         5.19e-07  4.09e-07  2.10e-05  1.19e-07  5.20e-07
  shared        3.87e-06  6.04e-06  2.06e-05  1.19e-07  7.64e-07
  multi         4.43e-06  3.45e-05  4.62e-04  3.58e-07  7.99e-07
  nonsquare     2.37e-06  3.21e-06  3.70e-05  2.38e-07  6.15e-07
  window        8.30e-07  2.34e-06  1.17e-05  1.66e-07  6.79e-07
  nosmooth      1.57e-06  7.64e-07  3.77e-07  1.19e-07  1.05e-06
  bins1024      1.65e-06  2.41e-06  7.27e-05  1.73e-06  1.11e-06
  v64           1.27e-05  1.20e-05  8.15e-05  7.46e-07  7.96e-07
  sparse_nodes  3.99e-06  7.17e-06  7.69e-05  3.91e-13  4.95e-07
  one_point     2.20e-08  1.70e-07  2.60e-07  5.00e-11  4.62e-07
The fp32 restatement against the golden (reference module, torch fp32 on the CPU): pmf equal, cdf
within 1.73e-6 (bins1024), pdf within 1.24e-6; the bound on all three is 4 x 1.73e-6 = 6.91e-6.
"""

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import residual_stats_ref as R
from conftest import REPO
from goldens import loss_case


# ---------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_fp32_restatement_reproduces_golden(name):
    a, g = R.restate(name, torch.float32), R.golden(name)
    c = loss_case(name)
    for k in ("pmf", "cdf", "pdf"):
        assert g[k].dtype == np.float32 and g[k].shape == (2, c["num_nodes"], c["num_bins"])
        err = float(np.abs(a[k].numpy().astype(np.float64) - g[k]).max())
        print(f"{name}: fp32 restatement vs golden {k} {err:.3e} (bound {R.GOLDEN_BOUND:.3e})")
        assert err <= R.GOLDEN_BOUND
    assert float(np.abs(g["pdf"]).max()) > 1.0  # the bound is small against the values it guards


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_golden_pmf_holds_the_integer_histograms(name):
    """round(pmf (total + 1e-10)) of the reference's pmf == the fp64 and fp32 restatements' counts."""
    g = R.golden(name)
    for dtype in (torch.float64, torch.float32):
        a = R.restate(name, dtype)
        tot = a["tot"].numpy().astype(np.float64)[..., None]
        h = np.round(g["pmf"].astype(np.float64) * (tot + 1e-10)).astype(np.int64)
        assert np.array_equal(h, a["hist"].numpy())
    a = R.restate(name)
    P, K = loss_case(name)["src_coords"].shape[:2]
    assert int(a["tot"].sum()) == 2 * 2 * P * K  # every point counts once on each side, in each variant


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(R.GOLDEN_FILE) < 256 * 1024
    z = np.load(R.GOLDEN_FILE)
    assert set(z.files) == {f"{n}/{k}" for n in R.GOLDEN_CASES for k in ("pmf", "cdf", "pdf")}


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_restatement_error_gives_the_gpu_bound(name):
    b = R.bounds(name)
    print(f"{name}: fp32 restatement error reproj {b['r'][0] / 4:.2e} fixed {b['r'][1] / 4:.2e} sampson "
          f"{b['r'][2] / 4:.2e} cdf {b['cdf'] / 4:.2e} pdf {b['pdf'] / 4:.2e}")
    # sanity ceilings, about 5 x the largest figure seen on any host: a bound is a fraction of a pixel, never loose
    assert (b["r"] > 0).all() and b["r"][0] < 4 * 1e-4 and b["r"][1] < 4 * 2.5e-4 and b["r"][2] < 4 * 2.5e-3
    assert 0 < b["cdf"] < 4 * 1e-5 and 0 < b["pdf"] < 4 * 1e-5


def test_cases_exercise_their_risks():
    """What the GPU checks lean on, re-asserted so that a changed golden cannot empty a check."""
    behind, nan_pairs = {}, {}
    for name in R.CASES:
        a, c = R.restate(name), loss_case(name)
        assert bool(torch.isfinite(a["r"][:2]).all()) and float(a["pz"].abs().min()) >= 0.2
        same = (c["src_idx"] == c["dst_idx"])
        assert bool(torch.isnan(a["r"][2][same]).all()) and bool(torch.isfinite(a["r"][2][~same]).all())
        nan_pairs[name] = int(same.sum())
        behind[name] = int(R.behind_of(a["r"][0].numpy(), a["pz"].numpy()).sum())
    assert {k: v for k, v in behind.items() if v} == {"bins1024": 34, "v64": 487, "sparse_nodes": 26}
    assert {k: v for k, v in nan_pairs.items() if v} == {"sparse_nodes": 1}
    assert loss_case("v64")["src_coords"].shape[0] == 70


def test_sampson_is_zero_on_exact_correspondences_and_scale_free():
    """x' = the exact reprojection of x lies on its epipolar line for any depth: r2 ~ 0 while a wrong
    depth moves r0; scaling F leaves r2 alone."""
    c = dict(loss_case("multi"))
    args = (c["enc"].double(), (c["H"], c["W"]), c["kp2k"].double(), c["shared"], c["src_idx"], c["dst_idx"])
    F = R.fundamental(*args)
    assert np.allclose(F.flatten(1).norm(dim=1).numpy(), 1.0, atol=1e-12)
    # reproject with the oracle's geometry: residual 0 <=> dst_coords == pred
    ext, intr = R.O.pose_encoding_to_extri_intri(args[0][None], args[1])
    K = torch.bmm(args[2], intr[0])
    pad = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(ext.shape[1], 1, 4)
    E = torch.cat([ext[0], pad], 1)
    s, d = c["src_idx"].long(), c["dst_idx"].long()
    T = torch.bmm(E[d], torch.inverse(E[s]))
    h = torch.cat([c["src_coords"].double(), torch.ones_like(c["src_coords"][..., :1]).double()], -1)
    for depth_scale in (1.0, 1.7):
        X = torch.einsum("pij,pkj->pki", torch.inverse(K[s]), h) * (c["src_depth"].double() * depth_scale)[..., None]
        Y = torch.einsum("pij,pkj->pki", T[:, :3, :3], X) + T[:, None, :3, 3]
        pr = torch.einsum("pij,pkj->pki", K[d], Y)
        pred = pr[..., :2] / pr[..., 2:]
        r2 = R.sampson(F, c["src_coords"], pred, c["src_idx"], c["dst_idx"])
        assert float(r2.max()) < 1e-8
        assert float(R.sampson(-3.5 * F, c["src_coords"], pred + 1.0, c["src_idx"], c["dst_idx"]).sub(
            R.sampson(F, c["src_coords"], pred + 1.0, c["src_idx"], c["dst_idx"])).abs().max()) < 1e-10


def test_rank_rules():
    assert [R.ranks(n) for n in (1, 2, 3, 10, 11, 300)] == [(0, 0), (0, 1), (1, 2), (4, 8), (5, 9), (149, 269)]
    x = np.array([[[5, 1, np.nan, 3, 3, np.inf, 2, 4, 3, 0]]], dtype=np.float32)
    counts, stats = R.pair_summary(x, np.zeros((1, 10), bool), [3.0, 100.0])
    assert counts.tolist() == [[[8, 0, 3, 8]]]            # strict <: the three 3s are not below 3
    assert stats[0, 0].tolist() == [21 / 8, 3.0, 5.0, 5.0]  # sorted 0 1 2 3 3 3 4 5: s[3], s[7]
    t = torch.tensor(x[0, 0][np.isfinite(x[0, 0])])
    assert float(t.median()) == stats[0, 0, 1]             # torch's lower median
    counts, stats = R.pair_summary(np.full((1, 1, 4), np.nan, np.float32), np.zeros((1, 4), bool), [])
    assert counts.tolist() == [[[0, 0]]] and np.isnan(stats).all()


# ---------------------------------------------------------------- summarize on hand-made arrays
def test_summarize_hand_made():
    from sailrecon_amd.train.loss import RESIDUAL_VARIANTS, summarize
    nan = float("nan")
    ps = np.zeros((3, 3, 4), np.float32)
    ps[:, :, 1] = [[1.0, 3.0, 2.0], [4.0, nan, 8.0], [nan, nan, nan]]
    pc = np.zeros((3, 3, 4), np.int32)
    pc[0] = [[10, 1, 5, 10], [10, 0, 0, 4], [10, 2, 10, 10]]
    pc[1] = [[10, 1, 2, 3], [0, 0, 0, 0], [6, 2, 1, 6]]
    out = summarize({"pair_stats": ps, "pair_counts": pc, "thresholds": (1.0, 2.5), "n_points": 10})
    assert tuple(out) == RESIDUAL_VARIANTS == R.VARIANTS
    a, b, c = (out[k] for k in RESIDUAL_VARIANTS)
    assert a == {"median_px": 2.0, "inlier@1": 0.5, "inlier@2.5": 0.8, "behind": 0.1, "nonfinite": 0.0}
    assert b["median_px"] == 6.0 and b["inlier@1"] == 3 / 16 and b["inlier@2.5"] == 9 / 16
    assert b["behind"] == 3 / 16 and abs(b["nonfinite"] - 14 / 30) < 1e-12
    assert np.isnan(c["median_px"]) and np.isnan(c["inlier@1"]) and np.isnan(c["behind"]) and c["nonfinite"] == 1.0
    # the packed form residual_stats returns: [pair_stats | pair_counts] in one fp32 buffer
    flat = np.concatenate([ps.ravel(), pc.ravel().view(np.float32)])
    again = summarize({"thresholds": (1.0, 2.5), "n_points": 10}, host_pairs=flat)
    assert again[RESIDUAL_VARIANTS[0]] == a and again[RESIDUAL_VARIANTS[1]] == b
    assert summarize({"_pairs": torch.from_numpy(flat), "thresholds": (1.0, 2.5), "n_points": 10})["reproj"] == a


# ---------------------------------------------------------------- ABI
def test_abi_version_and_symbols():
    from sailrecon_amd import _lib
    L = _lib.load()
    assert L.sr_version() >= (1 << 16) | 10
    for name in ("sr_imc_stats_workspace", "sr_imc_residual_stats"):
        assert name in _lib.EXPORTED and getattr(L, name).argtypes is not None
    assert L.sr_imc_residual_stats.argtypes[2]._type_ is _lib.ImcStatsDesc
    base = L.sr_imc_stats_workspace(4, 3, 300, 4, 250)
    assert L.sr_imc_stats_workspace(4, 3, 301, 4, 250) - base == 4 * 3  # three residual planes + the behind flags
    assert L.sr_imc_stats_workspace(4, 3, 0, 4, 250) == 0


def test_argument_errors_without_a_gpu():
    """Validation comes before any launch: SR_EINVAL (-1) with a message, on a machine with or without a GPU."""
    from sailrecon_amd import _lib
    L = _lib.load()
    g, s = _lib.ImcLossDesc(), _lib.ImcStatsDesc()
    assert L.sr_imc_residual_stats(None, None, ctypes.byref(s)) == -1
    assert L.sr_imc_residual_stats(None, ctypes.byref(g), ctypes.byref(s)) == -1
    assert b"null pointer" in L.sr_last_error()


@pytest.fixture(scope="module")
def host_check():
    csrc = os.path.join(REPO, "self-supervise-sfm_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 8)), "debug-build"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(REPO, "self-supervise-sfm_amd", "build", "debug", "abi_host_check")


def test_ctypes_struct_layout_matches_c(host_check):
    from sailrecon_amd import _lib
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([host_check, "layout", "imc_stats"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    lay = json.loads(r.stdout)
    assert set(lay) == {"sr_imc_stats_desc"}
    c = lay["sr_imc_stats_desc"]
    assert ctypes.sizeof(_lib.ImcStatsDesc) == c["size"]
    assert {f[0] for f in _lib.ImcStatsDesc._fields_} == set(c["fields"])
    for f, off in c["fields"].items():
        assert getattr(_lib.ImcStatsDesc, f).offset == off, f
