"""The DPT head's kernels (csrc/sr_dpt.hip, sr_conv3x3_f32) against the fp64 references and
per-element bounds of tests/dpt_ref.py (whose bounds and mutants tests/test_dpt_ref.py checks on the
CPU), at the smallest shapes that reach each branch, then DPTHead against the fp64 oracle on the
paths the golden tests do not run, the reference's own goldens of those paths, and the chunk loop.

Bit-exact: im2col3x3, convt_scatter, add_, relu_, an equal-size resize.  Bounded per element:
resize_bilinear, conv3x3 (wide and narrow kernels, stride 2, one-pixel-wide maps, residual with
gamma, no bias), gemm + convt_scatter as ConvTranspose, dpt_pos_embed_, dpt_head_out (all 4 x 3
activation pairs), unproject.  Every bounded test prints "BOUND <op> <case> <worst ratio>".
"""

import pytest
import torch

import dpt_ref as R
from goldens import DPT_SMALL, DPT_VARIANTS, dpt_variant_model_sd, load_npz, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEAD_MARGIN = 4.0  # x the fp32 CPU oracle's own error: another summation order, FMA contraction


def _ops():
    from sailrecon_amd import ops
    return ops


# ---------------------------------------------------------------- bit-exact data movement
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", R.IM2COL_CASES)
def test_im2col3x3_bit_exact(shape, stride, relu):
    n, h, w, c = shape
    x = R.rand(shape, 9 + c)
    ref, _ = R.im2col3x3(x, stride, relu)
    out = torch.full(ref.shape, float("nan"), device=DEV)
    _ops().im2col3x3(x.to(DEV), stride, relu, out)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", R.SCATTER_CASES)
def test_convt_scatter_bit_exact(case, with_bias):
    n, h, w, co, k = case
    g = R.rand((n * h * w, k * k * co), 5 + co)
    b = R.rand((co,), 6) if with_bias else None
    ref, _ = R.convt_scatter(g, n, h, w, k, co, b)
    out = torch.full(ref.shape, float("nan"), device=DEV)
    _ops().convt_scatter(g.to(DEV), n, h, w, k, co, None if b is None else b.to(DEV), out)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("numel", [4, 1028])
def test_add_relu_bit_exact(numel):
    a, b = R.rand((numel,), 1), R.rand((numel,), 2)
    a[0], a[-1], b[-1] = -0.0, 0.0, -0.0
    d = a.to(DEV)
    _ops().add_(d, b.to(DEV))
    assert torch.equal(d.cpu(), a + b)
    r = a.to(DEV)
    _ops().relu_(r)
    # fmaxf(-0.0, 0.0) may return either zero: compare values, then that nothing negative is left
    assert torch.equal(r.cpu(), a.clamp_min(0)) and not bool((r.cpu() < 0).any())


def test_resize_equal_sizes_is_a_copy():
    x = R.rand((1, 5, 7, 4), 3)
    out = torch.full(x.shape, float("nan"), device=DEV)
    _ops().resize_bilinear(x.to(DEV), out)
    assert torch.equal(out.cpu(), x)


# ---------------------------------------------------------------- bilinear resize
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("case", R.RESIZE_CASES)
def test_resize_bilinear_per_element(case, with_add):
    n, h, w, c, ho, wo = case
    x, add = R.resize_inputs(case)
    add = add if with_add else None
    ref, mag = R.resize_bilinear(x, ho, wo, add)
    out = torch.full((n, ho, wo, c), float("nan"), device=DEV)
    _ops().resize_bilinear(x.to(DEV), out, add=None if add is None else add.to(DEV))
    r = R.ratio(out.cpu(), ref, R.resize_bound(mag, add))
    print(f"BOUND resize_bilinear {case} add={with_add} {r:.3f}")
    assert r <= 1


# ---------------------------------------------------------------- conv3x3
def _run_conv(case):
    n, h, w, c, cout, stride, relu, mode = case
    z = R.conv_case(case)
    ho, wo = z["ref"].shape[1:3]
    out = z["base"].to(DEV) if z["base"] is not None else torch.full((n, ho, wo, cout), float("nan"), device=DEV)
    _ops().conv3x3(z["x"].to(DEV), z["w"].to(DEV), out, stride=stride, relu_in=relu,
                   bias=None if z["b"] is None else z["b"].to(DEV),
                   resid_gamma=None if z["gamma"] is None else z["gamma"].to(DEV))
    torch.cuda.synchronize()
    r = R.ratio(out.cpu(), z["ref"], R.conv3x3_bound(c, z["mag"]))
    return r, rel_l2(out.cpu().numpy(), z["ref"].numpy())


@pytest.mark.parametrize("case", R.CONV_CASES)
def test_conv3x3_per_element(case):
    r, l2 = _run_conv(case)
    print(f"BOUND conv3x3 {case} {r:.3f} rel-L2 {l2:.2e}")
    assert r <= 1 and l2 < 1e-5


@pytest.mark.parametrize("case", [c for c in R.CONV_CASES if c[4] <= 32])
def test_conv3x3_wide_kernel_at_narrow_widths(case):
    """cout <= 32 through the 128-wide implicit GEMM (SR_CONV_NO_NARROW=1) instead of the narrow kernel."""
    with _ops().tuning(SR_CONV_NO_NARROW=1):
        r, l2 = _run_conv(case)
    print(f"BOUND conv3x3-wide {case} {r:.3f} rel-L2 {l2:.2e}")
    assert r <= 1 and l2 < 1e-5


# ---------------------------------------------------------------- ConvTranspose as the head runs it
@pytest.mark.parametrize("case", R.CONVT_CASES)
def test_convt_gemm_scatter_per_element(case):
    from sailrecon_amd import _lib
    n, h, w, cin, co, k = case
    y, _, b, wk = R.convt_inputs(case)
    ref, mag = R.convt(y, wk, b, k)
    g = torch.full((n * h * w, k * k * co), float("nan"), device=DEV)
    _ops().gemm(y.reshape(-1, cin).to(DEV), wk.to(DEV), g, _lib.SR_EPI_BIAS, bias=None, splits=1)
    out = torch.full((n, h * k, w * k, co), float("nan"), device=DEV)
    _ops().convt_scatter(g, n, h, w, k, co, b.to(DEV), out)
    r = R.ratio(out.cpu(), ref, R.gamma(cin + 1) * mag)
    print(f"BOUND convt {case} {r:.3f}")
    assert r <= 1


# ---------------------------------------------------------------- positional embedding
@pytest.mark.parametrize("shape", R.POS_SHAPES)
def test_pos_embed_per_element(shape):
    n, h, w, c = shape
    x = R.rand(shape, h * w + c)
    worst = 0.0
    for aspect in R.POS_ASPECTS:
        for ratio in R.POS_RATIOS:
            table, _ = R.pos_embed(h, w, c, aspect, ratio)
            got = x.to(DEV)
            _ops().dpt_pos_embed_(got, aspect, ratio)
            r = R.ratio(got.cpu(), x.double() + table, R.pos_embed_bound(x, ratio))  # one table for every frame
            assert r <= 1, (aspect, ratio, r)
            worst = max(worst, r)
    print(f"BOUND pos_embed {shape} {worst:.3f}")


# ---------------------------------------------------------------- output head
def _head_out(hidden_dev, w, b, act, conf_act, cout):
    npix = hidden_dev.shape[0]
    preds = torch.full((npix, cout - 1), float("nan"), device=DEV)
    conf = torch.full((npix,), float("nan"), device=DEV)
    _ops().dpt_head_out(hidden_dev, w.to(DEV), None if b is None else b.to(DEV), act, conf_act, preds, conf)
    return preds.cpu(), conf.cpu()


@pytest.mark.parametrize("conf_act", sorted(R.CONF_ACTS))
@pytest.mark.parametrize("act", sorted(R.ACTS))
def test_head_out_all_activation_pairs(act, conf_act):
    worst = 0.0
    runs = [(c, "plain") for c in R.HEAD_OUT_CASES] + [((32, 4, 257), "ldh"), ((32, 4, 257), "nobias")]
    for (cin, cout, npix), kind in runs:
        hidden, w, b = R.head_out_inputs(cin, cout, npix, seed=kind != "plain")
        if kind == "nobias":
            b = None
        hd = hidden.to(DEV)
        if kind == "ldh":  # hidden: a column slice of a wider buffer (ldh = cin + 8 > cin)
            wide = torch.full((npix, cin + 8), float("nan"), device=DEV)
            wide[:, 4:4 + cin] = hd
            hd = wide[:, 4:4 + cin]
        s, delta, f, fc = R.head_out(hidden, w, b, act, conf_act)
        preds, conf = _head_out(hd, w, b, act, conf_act, cout)
        ok_p, r_p = R.head_out_check(preds, s[:, :-1], delta[:, :-1], f, act in R.MAY_BE_ZERO)
        ok_c, r_c = R.head_out_check(conf, s[:, -1], delta[:, -1], fc, False)
        assert ok_p and ok_c, (cin, cout, npix, kind, r_p, r_c)
        worst = max(worst, r_p, r_c)
    print(f"BOUND head_out {act}/{conf_act} {worst:.3f}")


# ---------------------------------------------------------------- unprojection
def test_unproject_per_element():
    depth, extr, intr = R.unproject_inputs()
    ref, mag = R.unproject(depth, extr, intr)
    out = torch.full((*depth.shape, 3), float("nan"), device=DEV)
    _ops().unproject_depth(depth.to(DEV), extr.to(DEV), intr.to(DEV), out)
    r = R.ratio(out.cpu(), ref, 16 * R.U * mag)
    print(f"BOUND unproject {r:.3f}")
    assert r <= 1


# ---------------------------------------------------------------- the whole head
def _run_head(c, cfg):
    m = c["model"]
    m.load_state_dict(c["sd"])
    m = m.to(DEV)
    out = m({l: t.to(DEV) for l, t in c["toks"].items()}, images=c["images"].to(DEV), patch_start_idx=5)
    torch.cuda.synchronize()
    return (out,) if cfg.get("feature_only") else tuple(out)


@pytest.mark.parametrize("name", list(R.HEAD_CONFIGS))
def test_head_against_fp64_oracle(name):
    """DPTHead against oracle.sfm_oracle.dpt_forward on .double() weights and tokens: the output has
    the oracle's shape [B,S,oh,ow,...] and max |got - ref| / (|ref| + rms(ref)) is at most
    HEAD_MARGIN x the same metric of the fp32 CPU oracle on the same input.

    Measured (the "HEAD" lines this test prints):
                          fp32 CPU oracle        this path on MI355X
                          preds     conf         preds     conf
        56x70             3.04e-06  4.72e-07     3.24e-06  4.59e-07
        84x56-B2          5.30e-06  4.57e-07     4.66e-06  4.40e-07
        60x75             3.34e-06  4.16e-07     2.66e-06  4.78e-07
        down2             3.61e-06  5.81e-07     3.59e-06  5.92e-07
        down2-feat        2.23e-06  -            2.16e-06  -
        nopos             3.90e-06  3.90e-07     4.01e-06  3.50e-07
        linear-sigmoid    3.81e-06  4.16e-07     3.32e-06  4.74e-07
        relu-expp0        4.16e-06  7.91e-07     3.74e-06  8.09e-07
    so the kernels sit at 0.80 .. 1.15 x the CPU figure, against the 4 x allowed."""
    cfg, B, S, H, W = R.HEAD_CONFIGS[name]
    c = R.head_case(name)
    got = _run_head(c, cfg)
    metrics = []
    for g, ref in zip(got, c["ref"]):
        assert g.shape == ref.shape, (name, tuple(g.shape), tuple(ref.shape))
        assert bool(torch.isfinite(g).all())
        metrics.append(R.head_metric(g.cpu(), ref))
    print("HEAD", name, "cpu", " ".join(f"{m:.2e}" for m in c["cpu_metric"]), "gpu",
          " ".join(f"{m:.2e}" for m in metrics))
    for m, cpu in zip(metrics, c["cpu_metric"]):
        assert m <= HEAD_MARGIN * cpu, (name, m, cpu)


@pytest.mark.parametrize("name", list(DPT_VARIANTS))
def test_head_variants_match_reference(name):
    """The reference's own DPTHead on 60x75 images (g6_dpt_variants.npz): its output shape
    [B,S,56,70,...] (28x35 at down_ratio=2) and values, at the suite's rel-L2 < 1e-4."""
    g = load_npz("g6_dpt_variants.npz")
    m, sd = dpt_variant_model_sd(name)
    m.load_state_dict(sd)
    m = m.to(DEV)
    toks = {l: torch.from_numpy(g[f"tok_{l}"]).to(DEV) for l in DPT_SMALL["intermediate_layer_idx"]}
    preds, conf = m(toks, images=torch.from_numpy(g["images"]).to(DEV), patch_start_idx=5)
    assert preds.shape == g[f"{name}_preds"].shape and conf.shape == g[f"{name}_conf"].shape
    assert rel_l2(preds.cpu().numpy(), g[f"{name}_preds"]) < 1e-4
    assert rel_l2(conf.cpu().numpy(), g[f"{name}_conf"]) < 1e-4


@pytest.mark.parametrize("name", ["56x70", "down2-feat"])
def test_head_chunking_is_bit_exact(name, monkeypatch):
    """The chunk loop (f0 > 0: the row offsets and the output slices) with one and with two frames
    per chunk against the one-chunk result: every op is per frame, splits=1 and the tiles are fixed,
    so the results are identical bit for bit."""
    from sailrecon_amd.heads import dpt_head
    cfg, B, S, H, W = R.HEAD_CONFIGS[name]
    c = R.head_case(name)
    m = c["model"]
    frames, ph, pw = B * S, H // 14, W // 14
    oh, ow = (int(p * 14 / cfg.get("down_ratio", 1)) for p in (ph, pw))
    per_frame = m.frame_bytes(DPT_SMALL["features"], ph, pw, oh, ow)
    seen = []
    inner = dpt_head.DPTHead._forward_chunk

    def spy(self, toks, P, psi, f0, f1, *rest):
        seen.append((f0, f1))
        return inner(self, toks, P, psi, f0, f1, *rest)

    monkeypatch.setattr(dpt_head.DPTHead, "_forward_chunk", spy)
    whole = [t.clone() for t in _run_head(c, cfg)]
    assert seen == [(0, frames)]
    for chunk in (1, 2):
        if chunk >= frames:
            continue
        seen.clear()
        monkeypatch.setattr(dpt_head, "ACT_BUDGET", per_frame * chunk + per_frame // 2)
        got = _run_head(c, cfg)
        assert seen == [(f0, min(frames, f0 + chunk)) for f0 in range(0, frames, chunk)]
        for a, b in zip(got, whole):
            assert torch.equal(a, b), (name, chunk)
