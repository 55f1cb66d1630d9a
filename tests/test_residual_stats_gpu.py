"""sr_imc_residual_stats on the GPU (train.loss.residual_stats / summarize, compute_loss(do_record=True),
Trainer.step(monitor=True)) against the fp64 restatement of tests/residual_stats_ref.py.

Residuals, cdf and pdf are held to 4 x the fp32 restatement's error against fp64, per case (and per
variant for the residuals; tests/test_residual_stats.py lists the figures).  The integer histograms
are exactly equal: the stored inputs are clear of the bin edges (tests/golden/make_golden_loss.py).
Counts, median, p90 and max are exact against the kernel's own residuals; the mean within 2 fp32 ulps
of their fp64 mean.  The selection keeps a pair's residuals in LDS up to 12,288 points and re-reads
global memory above: both sides of that size are run.

Measured on MI355X (kernel vs fp64 restatement; residuals as |r - r64| / max(r64, 1 px), cdf / pdf absolute):
  case          reproj    fixed     sampson   cdf       pdf
  dummy         2.15e-07  1.90e-07  5.06e-06  1.19e-07  4.09e-07
  shared        3.06e-06  3.27e-06  2.01e-05  1.19e-07  2.88e-07
  multi         9.07e-07  2.05e-05  4.75e-05  3.58e-07  5.30e-07
  nonsquare     2.05e-06  6.84e-06  3.40e-05  2.38e-07  4.04e-07
  window        7.70e-07  1.26e-06  1.36e-05  1.66e-07  7.73e-07
  nosmooth      5.93e-07  7.36e-07  4.22e-07  1.19e-07  4.94e-07
  bins1024      1.56e-06  1.87e-06  2.47e-05  1.73e-06  1.13e-06
  v64           1.46e-05  6.66e-06  5.17e-05  7.46e-07  5.37e-07
  sparse_nodes  3.66e-06  5.51e-06  1.87e-05  3.91e-13  1.12e-07
  one_point     4.99e-08  4.93e-08  7.36e-08  5.00e-11  4.62e-07
Each is at most 0.57 of its bound (one_point, exact reprojection); the cdf sits at exactly a
quarter: the kernel and the fp32 restatement add the same fp32 pmf values in the same order.
compute_loss(do_record=True) on multi against the golden: frame_cdfs 3.58e-7, frame_pdfs 6.56e-7 (bound 6.91e-6).
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import residual_stats_ref as R
from goldens import loss_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TH = (1.0, 2.0, 4.0, 8.0)


def _cdf(c):
    from sailrecon_amd.train.loss import CDFLossIndexPytorch
    return CDFLossIndexPytorch(c["min_val"], c["max_val"], c["num_bins"], c["nodes_src"], c["nodes_dst"],
                               gradient_smooth=c["gradient_smooth"], num_nodes=c["num_nodes"])


def _args(c):
    return (c["enc"].to(DEV), (c["H"], c["W"]), c["kp2k"], c["shared"], c["src_idx"], c["dst_idx"], c["src_coords"],
            c["dst_coords"], c["src_depth"], c["dst_depth"], _cdf(c))


def _host(out):
    return {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in out.items()}


def _stats(c, thresholds=TH, residuals=True):
    from sailrecon_amd.train.loss import residual_stats
    return _host(residual_stats(*_args(c), thresholds=thresholds, residuals=residuals))


@functools.lru_cache(maxsize=None)
def _case_stats(name):
    """One run per golden case, shared by the tests below (they do not modify it)."""
    return _stats(loss_case(name))


def _check_selection(out, thresholds, behind):
    """pair_counts / pair_stats against the rank rules applied to the kernel's own residuals."""
    lo, hi = behind if isinstance(behind, tuple) else (np.asarray(behind).sum(-1),) * 2
    counts, stats = R.pair_summary(out["residuals"], np.zeros_like(out["residuals"][0], dtype=bool), thresholds)
    got_counts = out["pair_counts"].astype(np.int64)
    assert np.array_equal(np.delete(got_counts, 1, axis=-1), np.delete(counts, 1, axis=-1))
    assert (got_counts[..., 1] >= lo).all() and (got_counts[..., 1] <= hi).all()  # [3, P] against [P]: every v alike
    assert np.array_equal(got_counts[0, :, 1], got_counts[1, :, 1]) and np.array_equal(got_counts[0, :, 1], got_counts[2, :, 1])
    got = out["pair_stats"]
    filled = ~np.isnan(stats[..., 1:])
    assert np.array_equal(np.isnan(got[..., 1:]), ~filled)
    assert np.array_equal(got[..., 1:][filled].view(np.uint32), stats[..., 1:][filled].view(np.uint32))
    two_ulp, mean64 = R.mean_bound(out["residuals"])
    empty = counts[..., 0] == 0
    assert np.array_equal(np.isnan(got[..., 0]), empty) and np.isnan(got[empty]).all()
    assert (np.abs(got[..., 0][~empty].astype(np.float64) - mean64[~empty]) <= two_ulp[~empty]).all()


PZ_EPS = 1e-4  # fp32 p_z (three dot products of terms up to ~10) is within 1e-5 of the fp64 one


def _behind64(c):
    """n_behind per pair as an interval [lo, hi]: a synthetic scene with points behind the camera also
    has points with p_z within fp32 error of 0, whose side the fp64 restatement cannot decide."""
    r, _, pz = R.residuals_of(c, torch.float64)
    assert bool(torch.isfinite(r[0]).all())
    pz = pz.numpy()
    return (pz < -PZ_EPS).sum(-1), (pz <= PZ_EPS).sum(-1)


# ---------------------------------------------------------------- compute_loss(do_record=True)
def test_compute_loss_do_record():
    from sailrecon_amd.train.loss import RESIDUAL_VARIANTS, compute_loss
    c = loss_case("multi")
    batch = {"K_prime_to_K": c["kp2k"], "shared_focal": c["shared"], "src_idx": c["src_idx"], "dst_idx": c["dst_idx"],
             "src_coords": c["src_coords"], "dst_coords": c["dst_coords"], "src_depth": c["src_depth"],
             "dst_depth": c["dst_depth"]}
    plain = compute_loss(c["enc"][None].to(DEV), batch, DEV, _cdf(c), image_hw=(c["H"], c["W"]))
    rec = compute_loss(c["enc"][None].to(DEV), batch, DEV, _cdf(c), do_record=True, image_hw=(c["H"], c["W"]))
    assert set(plain) == {"loss", "d_pose_enc"} and set(rec) == {"loss", "d_pose_enc", "plot_data"}
    assert torch.equal(plain["loss"], rec["loss"]) and torch.equal(plain["d_pose_enc"], rec["d_pose_enc"])
    pd = rec["plot_data"]
    assert set(pd) == {"frame_cdfs", "frame_pdfs", "max_val", "min_val", "num_bins", "residual_stats"}
    assert (pd["min_val"], pd["max_val"], pd["num_bins"]) == (0.0, 15.0, 250)
    g = R.golden("multi")
    for key, ref in (("frame_cdfs", g["cdf"][0]), ("frame_pdfs", g["pdf"][0])):
        assert isinstance(pd[key], np.ndarray) and pd[key].dtype == np.float32 and pd[key].shape == (4, 250)
        err = float(np.abs(pd[key].astype(np.float64) - ref).max())
        print(f"RESID_STATS do_record {key} vs golden {err:.3e} (bound {R.GOLDEN_BOUND:.3e})")
        assert err <= R.GOLDEN_BOUND
    s = pd["residual_stats"]
    assert tuple(s) == RESIDUAL_VARIANTS
    assert set(s["reproj"]) == {"median_px", "inlier@1", "inlier@2", "inlier@4", "inlier@8", "behind", "nonfinite"}
    assert 1.0 < s["reproj"]["median_px"] < 500.0 and s["reproj"]["nonfinite"] == 0.0


# ---------------------------------------------------------------- frame arrays
@pytest.mark.parametrize("case", R.CASES)
def test_frame_arrays(case):
    from sailrecon_amd.train.loss import imc_loss
    c, out, ref, b = loss_case(case), _case_stats(case), R.restate(case), R.bounds(case)
    tot = ref["tot"].numpy().astype(np.float64)[..., None]
    hist = np.round(out["frame_pmf"].astype(np.float64) * (tot + 1e-10)).astype(np.int64)
    assert np.array_equal(hist, ref["hist"].numpy())
    e_cdf = float(np.abs(out["frame_cdf"].astype(np.float64) - ref["cdf"].numpy()).max())
    e_pdf = float(np.abs(out["frame_pdf"].astype(np.float64) - ref["pdf"].numpy()).max())
    print(f"RESID_STATS {case} cdf {e_cdf:.2e}/{b['cdf']:.2e} pdf {e_pdf:.2e}/{b['pdf']:.2e}")
    assert e_cdf <= b["cdf"] and e_pdf <= b["pdf"]
    # the arrays returned are the ones the loss looked its values up in
    loss = float(imc_loss(*_args(c))[0].cpu())
    nb, bw = c["num_bins"], (c["max_val"] - c["min_val"]) / c["num_bins"]
    rl = np.log1p(out["residuals"][:2].astype(np.float64))
    bl = np.trunc((rl - c["min_val"]) / bw + 0.5).astype(np.int64)
    ok = (bl >= 0) & (bl < nb)
    bl = np.clip(bl, 0, nb - 1)
    ns, nd = c["nodes_src"].numpy()[:, None], c["nodes_dst"].numpy()[:, None]
    total = 0.0
    for v in range(2):
        cdf = out["frame_cdf"][v].astype(np.float64)
        total += np.where(ok[v], cdf[ns, bl[v]] + cdf[nd, bl[v]], 4.0).sum()
    host = total / (4.0 * rl[0].size)
    print(f"RESID_STATS {case} loss {loss:.8f} host lookup {host:.8f}")
    assert abs(host - loss) <= 1e-6 * abs(loss)


# ---------------------------------------------------------------- residuals
@pytest.mark.parametrize("case", R.CASES)
def test_residuals_match_fp64(case):
    c, out, ref, b = loss_case(case), _case_stats(case), R.restate(case), R.bounds(case)
    r64 = ref["r"].numpy()
    same = (c["src_idx"] == c["dst_idx"]).numpy()
    assert np.isnan(out["residuals"][2][same]).all() and (out["pair_counts"][2][same][:, [0, 2, 3, 4, 5]] == 0).all()
    assert np.isfinite(out["residuals"][2][~same]).all() and np.isfinite(out["residuals"][:2]).all()
    err = R.residual_error(out["residuals"], r64)
    print(f"RESID_STATS {case} residuals " + " ".join(f"{e:.2e}/{x:.2e}" for e, x in zip(err, b["r"])))
    assert (err <= b["r"]).all()
    _check_selection(out, TH, R.behind_of(r64[0], ref["pz"].numpy()))
    K = c["src_coords"].shape[1]
    assert (out["pair_counts"][:2, :, 0] == K).all() and (out["pair_counts"][2][~same][:, 0] == K).all()
    if case in ("bins1024", "v64", "sparse_nodes"):
        assert out["pair_counts"][0, :, 1].sum() == {"bins1024": 34, "v64": 487, "sparse_nodes": 26}[case]


# ---------------------------------------------------------------- selection shapes
_PAIRS3 = [(0, 1), (1, 2), (3, 0)]


@pytest.mark.parametrize("n_points", [1, 2, 3, 255, 256, 257, 700, 10000, 12288, 12289, 50000])
def test_selection_shapes(n_points):
    c = R.synth_case(100 + n_points % 97, 4, _PAIRS3, n_points)
    out = _stats(c)
    assert np.isfinite(out["residuals"]).all()
    _check_selection(out, TH, _behind64(c))


def test_selection_ties():
    """300 points = 3 correspondences repeated 100 times: both ranks fall inside tie groups."""
    c = R.synth_case(7, 4, _PAIRS3, 3)
    for k in ("src_coords", "dst_coords", "src_depth", "dst_depth"):
        c[k] = c[k].repeat_interleave(100, dim=1)[:, torch.randperm(300, generator=torch.Generator().manual_seed(1))]
    out = _stats(c)
    assert all(len(np.unique(out["residuals"][v, p])) == 3 for v in range(3) for p in range(3))
    _check_selection(out, TH, _behind64(c))
    assert np.array_equal(out["pair_stats"][..., 1], np.sort(out["residuals"], -1)[..., 149])


@pytest.mark.parametrize("n_thresh", [0, 8])
def test_thresholds_on_residual_values(n_thresh):
    """Thresholds equal to residuals that occur: r < t is strict.  0 and 8 thresholds."""
    c = R.synth_case(9, 4, _PAIRS3, 700)
    first = _stats(c)
    th = tuple(float(x) for x in np.sort(first["residuals"][0, 0])[[0, 10, 349, 350, 500, 698, 699, 699]][:n_thresh])
    out = _stats(c, thresholds=th)
    assert out["pair_counts"].shape == (3, 3, 2 + n_thresh)
    _check_selection(out, th, _behind64(c))
    if n_thresh:
        assert out["pair_counts"][0, 0, 2:].tolist() == [0, 10, 349, 350, 500, 698, 699, 699]
    assert np.array_equal(out["residuals"], first["residuals"]) and np.array_equal(out["pair_stats"], first["pair_stats"])


# ---------------------------------------------------------------- non-finite inputs
def test_nonfinite_inputs():
    c = R.synth_case(11, 4, _PAIRS3 + [(2, 3)], 700)
    clean = _stats(c)
    k_idx, m_idx = [3, 77, 300, 699], [0, 5, 650]
    c["src_depth"] = c["src_depth"].clone()
    c["dst_coords"] = c["dst_coords"].clone()
    c["src_coords"] = c["src_coords"].clone()
    c["src_depth"][0, k_idx] = float("nan")        # pair 0: variants 0 / 1 lose k, Sampson none
    c["dst_coords"][1, m_idx, 0] = float("inf")    # pair 1: every variant loses m
    c["src_depth"][2] = float("nan")               # pair 2: nothing finite in any variant
    c["src_coords"][2] = float("nan")
    out = _stats(c)
    n = out["pair_counts"][..., 0]
    assert n[:, 0].tolist() == [700 - 4, 700 - 4, 700] and n[:, 1].tolist() == [700 - 3] * 3
    assert n[:, 2].tolist() == [0, 0, 0] and n[:, 3].tolist() == [700] * 3
    assert np.isnan(out["pair_stats"][:, 2]).all() and (out["pair_counts"][:, 2] == 0).all()
    for k in ("pair_stats", "pair_counts"):  # the untouched pair is unchanged
        assert np.array_equal(out[k][:, 3], clean[k][:, 3])
    assert np.array_equal(out["residuals"][:, 3], clean["residuals"][:, 3])
    pz = R.residuals_of(R.synth_case(11, 4, _PAIRS3 + [(2, 3)], 700), torch.float64)[2].numpy()  # the clean scene's
    assert np.abs(pz).min() > 0.1
    behind = R.behind_of(out["residuals"][0], pz)  # a point whose exact residual is not finite is not counted
    _check_selection(out, TH, behind)


# ---------------------------------------------------------------- stability and arguments
def test_bit_stable_and_workspace_reuse():
    from sailrecon_amd import ops
    keys = ("residuals", "frame_pmf", "frame_cdf", "frame_pdf", "pair_stats", "pair_counts")
    a, b = _stats(loss_case("v64")), _stats(loss_case("v64"))
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)
    for key in [k for k in ops._TRAIN_WS if k[1] == "imc_residual_stats"]:
        del ops._TRAIN_WS[key]
    fresh = _stats(loss_case("one_point"))
    _stats(R.synth_case(3, 4, _PAIRS3, 50000))
    again = _stats(loss_case("one_point"))
    assert all(np.array_equal(fresh[k].view(np.uint32), again[k].view(np.uint32)) for k in keys)
    assert any(k[1] == "imc_residual_stats" for k in ops._TRAIN_WS)


def test_einval_returns_without_launching():
    from sailrecon_amd import _lib, ops
    from sailrecon_amd.train.loss import _fill_desc
    c = loss_case("multi")
    d, enc, keep = _fill_desc(*_args(c))
    L = _lib.load()
    P, K, nn, nb = 3, 300, 4, 250
    need = L.sr_imc_stats_workspace(4, P, K, nn, nb)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    bufs = dict(residuals=nan(3, P, K), frame_pmf=nan(2, nn, nb), frame_cdf=nan(2, nn, nb), frame_pdf=nan(2, nn, nb),
                pair_counts=nan(3, P, 6), pair_stats=nan(3, P, 4), workspace=nan(need))
    th = torch.tensor(TH, device=DEV)

    def desc(**kw):
        s = _lib.ImcStatsDesc()
        for k, t in bufs.items():
            setattr(s, k, ops._p(t))
        s.thresh, s.n_thresh, s.workspace_floats = ops._p(th), 4, need
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def only_workspace():
        s = _lib.ImcStatsDesc()
        s.workspace, s.workspace_floats = ops._p(bufs["workspace"]), need
        return s
    bad = [desc(n_thresh=9), desc(n_thresh=-1), desc(thresh=None), desc(pair_counts=None), desc(workspace=None),
           desc(workspace_floats=need - 1), only_workspace()]
    for s in bad:
        assert L.sr_imc_residual_stats(ops._stream(enc), ctypes.byref(d), ctypes.byref(s)) == -1
        assert L.sr_last_error()
    for field, value in (("n_views", 65), ("num_bins", 1025), ("n_points", 0), ("src_depth", None)):
        g = _lib.ImcLossDesc.from_buffer_copy(d)
        setattr(g, field, value)
        s = desc()
        assert L.sr_imc_residual_stats(ops._stream(enc), ctypes.byref(g), ctypes.byref(s)) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in bufs.values())
    s = desc()  # and the same descriptor, unchanged, runs
    assert L.sr_imc_residual_stats(ops._stream(enc), ctypes.byref(d), ctypes.byref(s)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bufs["pair_stats"].cpu().numpy().view(np.uint32),
                          _case_stats("multi")["pair_stats"].view(np.uint32))
    del keep
    from sailrecon_amd._lib import SfmAmdError
    from sailrecon_amd.train.loss import residual_stats
    with pytest.raises(SfmAmdError):
        residual_stats(*_args(c), thresholds=tuple(range(1, 10)))


# ---------------------------------------------------------------- Trainer
def test_trainer_monitor_changes_nothing():
    from sailrecon_amd.train.step import Trainer, prepare_model_input
    from test_train_step_gpu import _batch, _small
    outs, params = [], []
    for kw in ({}, {"monitor": True, "do_record": True}):
        m = _small().to(DEV)
        tr = Trainer(m, max_lr=2e-4, warmup_steps=10, max_steps=100)
        b = _batch(3)
        imgs, na, nq = prepare_model_input(b["rgb_processed"].to(DEV))
        m.aggregator.generator.manual_seed(0)
        outs.append(tr.step(imgs, na, nq, b, fix_rank=10, **kw))
        params.append(tr.flat.data.clone())
    plain, mon = outs
    assert set(plain) == {"loss", "lr", "skipped"}
    assert plain["loss"] == mon["loss"] and plain["lr"] == mon["lr"] and plain["skipped"] == mon["skipped"]
    assert torch.equal(params[0], params[1])
    for name in R.VARIANTS:
        for k in ("median_px", "inlier@1", "inlier@2", "inlier@4", "inlier@8", "behind", "nonfinite"):
            assert isinstance(mon[f"{name}/{k}"], float)
    assert mon["reproj/nonfinite"] == 0.0 and np.isfinite(mon["reproj/median_px"])
    pd = mon["plot_data"]
    assert pd["frame_cdfs"].shape == (1, 250) and pd["frame_pdfs"].shape == (1, 250) and pd["num_bins"] == 250
    assert pd["residual_stats"]["reproj"]["median_px"] == mon["reproj/median_px"]
