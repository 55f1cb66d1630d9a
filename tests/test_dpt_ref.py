"""tests/dpt_ref.py checks itself on the CPU: (1) every reference equals torch's own fp64 op to
1e-12 on the GPU file's shapes; (2) bound conditions: torch's fp32 CPU op (for pos_embed the
oracle's fp32-linspace table) stays inside each per-element bound that tests/test_dpt_oracle_gpu.py
applies to the kernels, so a correct fp32 kernel can meet it -- every test prints the worst ratio
"BOUND <op> <ratio>"; (3) mutants of the references break the same per-element checks."""

import pytest
import torch
import torch.nn.functional as F

import dpt_ref as R
from oracle import sfm_oracle as O

F64 = torch.float64


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


# ---------------------------------------------------------------- conv3x3
def _torch_conv(c, dt):
    n, h, w, ch, cout, stride, relu, mode = c["case"]
    x = c["x"].to(dt)
    if relu:
        x = x.clamp_min(0)
    y = _nhwc(F.conv2d(_nchw(x), R._w_oihw(c["w"].to(dt), ch), None if c["b"] is None else c["b"].to(dt),
                       stride=stride, padding=1))
    if c["base"] is not None:
        y = c["base"].to(dt) + c["gamma"].to(dt) * y
    return y


def test_conv3x3_reference_and_fp32_bound():
    worst = 0.0
    for case in R.CONV_CASES:
        c = dict(R.conv_case(case), case=case)
        assert c["ref"].dtype == F64 and (c["mag"] >= c["ref"].abs() * (1 - 1e-12)).all()
        assert (c["ref"] - _torch_conv(c, F64)).abs().max() < 1e-12 * c["mag"].max(), case
        r = R.ratio(_torch_conv(c, torch.float32), c["ref"], R.conv3x3_bound(case[3], c["mag"]))
        assert r < 1, (case, r)
        worst = max(worst, r)
    print(f"BOUND conv3x3 {worst:.3f}")


@pytest.mark.parametrize("mutant,case", [("neighbour", (1, 8, 6, 32, 8, 2, False, "plain")),
                                         ("neighbour", (1, 5, 1, 32, 36, 1, False, "plain")),
                                         ("gamma", (1, 8, 6, 32, 8, 2, False, "gamma")),
                                         ("gamma", (2, 15, 11, 32, 36, 1, True, "gamma_nobias"))])
def test_conv3x3_mutants_break_the_bound(mutant, case):
    c = R.conv_case(case)
    bad, _ = R.conv3x3(c["x"], c["w"], c["b"], case[5], case[6], c["base"], c["gamma"], mutant=mutant)
    assert R.ratio(bad, c["ref"], R.conv3x3_bound(case[3], c["mag"])) > 1e3


# ---------------------------------------------------------------- ConvTranspose
def test_convt_reference_and_fp32_bound():
    worst = 0.0
    for case in R.CONVT_CASES:
        n, h, w, cin, co, k = case
        y, wt, b, wk = R.convt_inputs(case)
        ref, mag = R.convt(y, wk, b, k)
        t64 = _nhwc(F.conv_transpose2d(_nchw(y).double(), wt.double(), b.double(), stride=k))
        assert (ref - t64).abs().max() < 1e-12 * mag.max()
        # the kernels' own route in fp32 on the CPU: GEMM to (ky, kx, co) columns, then the scatter
        got, _ = R.convt_scatter(y.reshape(-1, cin) @ wk.T, n, h, w, k, co, b)
        r = R.ratio(got, ref, R.gamma(cin + 1) * mag)
        assert r < 1, (case, r)
        worst = max(worst, r)
    print(f"BOUND convt {worst:.3f}")


def test_scatter_and_im2col_are_the_torch_ops():
    for n, h, w, co, k in R.SCATTER_CASES:
        g = R.rand((n * h * w, k * k * co), 5 + co)
        # a ConvTranspose whose GEMM is the identity: cin = k k co one-hot columns
        wt = torch.eye(k * k * co).reshape(k * k * co, k, k, co).permute(0, 3, 1, 2)
        t = _nhwc(F.conv_transpose2d(_nchw(g.reshape(n, h, w, -1)), wt, None, stride=k))
        out, _ = R.convt_scatter(g, n, h, w, k, co, None)
        assert torch.equal(out, t)
        b = R.rand((co,), 6)
        assert torch.equal(R.convt_scatter(g, n, h, w, k, co, b)[0], t + b)
    for n, h, w, c in R.IM2COL_CASES:
        for stride in (1, 2):
            for relu in (False, True):
                x = R.rand((n, h, w, c), 9 + c)
                cols, _ = R.im2col3x3(x, stride, relu)
                xin = x.clamp_min(0) if relu else x
                u = F.unfold(_nchw(xin), 3, padding=1, stride=stride)  # [n, (ci, ky, kx), L]
                u = u.reshape(n, c, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * c)
                assert torch.equal(cols, u), (n, h, w, c, stride, relu)


# ---------------------------------------------------------------- bilinear resize
def test_resize_reference_and_fp32_bound():
    worst = 0.0
    for case in R.RESIZE_CASES:
        n, h, w, c, ho, wo = case
        x, add = R.resize_inputs(case)
        for a in (None, add):
            ref, mag = R.resize_bilinear(x, ho, wo, a)
            t32 = _nhwc(F.interpolate(_nchw(x), size=(ho, wo), mode="bilinear", align_corners=True))
            t64 = _nhwc(F.interpolate(_nchw(x).double(), size=(ho, wo), mode="bilinear", align_corners=True))
            if a is not None:
                t32, t64 = t32 + a, t64 + a.double()
            # against torch's fp64 op: equal up to the fp32 rounding of the coordinates, and to 1e-12
            # where the coordinates are exact in fp32 (ratios 1/2, 1, 0 and the copy)
            assert (ref - t64).abs().max() <= 64 * R.U * mag.max(), case
            if (h - 1) * 2 == ho - 1 or ho == 1 or h == 1:
                if (w - 1) * 2 == wo - 1 or wo == 1 or w == 1:
                    assert (ref - t64).abs().max() < 1e-12 * max(1.0, float(mag.max())), case
            r = R.ratio(t32, ref, R.resize_bound(mag, a))
            assert r < 1, (case, a is not None, r)
            worst = max(worst, r)
    x = R.rand((1, 5, 7, 4), 3)
    assert torch.equal(R.resize_bilinear(x, 5, 7)[0], x.double())  # equal sizes: a copy
    print(f"BOUND resize_bilinear {worst:.3f}")


def test_resize_fp64_coordinates_are_another_operation():
    """Why the reference rounds its coordinates to fp32: torch's fp32 op against the fp64 op misses
    the bound it meets against R.resize_bilinear."""
    n, h, w, c, ho, wo = 1, 19, 19, 4, 37, 37
    x = R.rand((n, h, w, c), 41) + 3.0
    big = R.rand((1, 23, 29, 4), 42) + 3.0
    worst = 0.0
    for xx, (oh_, ow_) in ((x, (ho, wo)), (big, (61, 83))):
        t32 = _nhwc(F.interpolate(_nchw(xx), size=(oh_, ow_), mode="bilinear", align_corners=True))
        t64 = _nhwc(F.interpolate(_nchw(xx).double(), size=(oh_, ow_), mode="bilinear", align_corners=True))
        ref, mag = R.resize_bilinear(xx, oh_, ow_)
        assert R.ratio(t32, ref, R.resize_bound(mag)) < 1
        worst = max(worst, R.ratio(t32, t64, R.resize_bound(mag)))
    print(f"fp32 torch vs fp64-coordinate resize: {worst:.2f} x the bound")


def test_resize_mutants_break_the_bound():
    for case in R.RESIZE_CASES[:2]:
        n, h, w, c, ho, wo = case
        x, add = R.resize_inputs(case)
        ref, mag = R.resize_bilinear(x, ho, wo)
        bad, _ = R.resize_bilinear(x, ho, wo, mutant="last_cell")
        assert R.ratio(bad, ref, R.resize_bound(mag)) > 1e3, case
    # the shared add table: a one-frame case cannot see a per-frame index, the two-frame case does
    for case, seen in ((R.RESIZE_CASES[1], False), (R.RESIZE_CASES[0], True)):
        n, h, w, c, ho, wo = case
        x, add = R.resize_inputs(case)
        ref, mag = R.resize_bilinear(x, ho, wo, add)
        bad, _ = R.resize_bilinear(x, ho, wo, add, mutant="add_per_frame")
        assert (R.ratio(bad, ref, R.resize_bound(mag, add)) > 1e3) == seen, case


# ---------------------------------------------------------------- positional embedding
def test_pos_embed_reference_and_fp32_bound():
    worst = 0.0
    for n, h, w, c in R.POS_SHAPES:
        for aspect in R.POS_ASPECTS:
            for ratio in R.POS_RATIOS:
                table, mag = R.pos_embed(h, w, c, aspect, ratio)
                assert table.shape == (h, w, c) and table.dtype == F64
                x = R.rand((n, h, w, c), h * w + c)
                # the oracle's fp32 path: fp32 linspace, then x + table * ratio in fp32
                got = x + O._uv_pos_embed(h, w, c, aspect) * ratio
                r = R.ratio(got, x.double() + table, R.pos_embed_bound(x, ratio))
                assert r < 1, (h, w, c, aspect, ratio, r)
                worst = max(worst, r)
    t, _ = R.pos_embed(1, 1, 4, 1.0, 1.0)  # steps == 1: the grid is its start, 0
    assert torch.equal(t.reshape(-1), torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=F64))
    print(f"BOUND pos_embed {worst:.3f}")


# ---------------------------------------------------------------- output head
def _head_act_reference(out, activation, conf_activation):
    """head_act.py:82-114 restated for the four activations the kernel has."""
    xyz, conf = out[:, :-1], out[:, -1]
    if activation == "exp":
        pts = torch.exp(xyz)
    elif activation == "relu":
        pts = F.relu(xyz)
    elif activation == "inv_log":
        pts = torch.sign(xyz) * torch.expm1(torch.abs(xyz))
    else:
        assert activation == "linear"
        pts = xyz
    if conf_activation == "expp1":
        c = 1 + conf.exp()
    elif conf_activation == "expp0":
        c = conf.exp()
    else:
        assert conf_activation == "sigmoid"
        c = torch.sigmoid(conf)
    return pts, c


@pytest.mark.parametrize("conf_act", sorted(R.CONF_ACTS))
@pytest.mark.parametrize("act", sorted(R.ACTS))
def test_head_out_reference_and_fp32_bound(act, conf_act):
    worst = 0.0
    for cin, cout, npix in R.HEAD_OUT_CASES:
        hidden, w, b = R.head_out_inputs(cin, cout, npix)
        s, delta, f, fc = R.head_out(hidden, w, b, act, conf_act)
        s64 = F.conv2d(hidden.double().clamp_min(0).T[None, :, :, None], w.double()[:, :, None, None],
                       b.double())[0, :, :, 0].T
        assert (s - s64).abs().max() < 1e-12 * max(1.0, float(s.abs().max()))
        p64, c64 = _head_act_reference(s, act, conf_act)
        assert torch.equal(f(s[:, :-1]), p64) and torch.equal(fc(s[:, -1]), c64)
        if npix >= 255:
            assert s.min() < -8 and s.max() > 8 and s.abs().min() < 0.05  # both signs, near 0
        # the fp32 CPU op
        s32 = hidden.clamp_min(0) @ w.T + b
        p32, c32 = _head_act_reference(s32, act, conf_act)
        ok_p, r_p = R.head_out_check(p32, s[:, :-1], delta[:, :-1], f, act in R.MAY_BE_ZERO)
        ok_c, r_c = R.head_out_check(c32, s[:, -1], delta[:, -1], fc, False)
        assert ok_p and ok_c and max(r_p, r_c) < 1, (cin, cout, npix, r_p, r_c)
        worst = max(worst, r_p, r_c)
    print(f"BOUND head_out {act}/{conf_act} {worst:.3f}")


def test_head_out_interval_rejects_a_wrong_activation():
    hidden, w, b = R.head_out_inputs(32, 4, 255)
    s, delta, f, fc = R.head_out(hidden, w, b, "inv_log", "expp1")
    ok, _ = R.head_out_check(torch.expm1(s[:, :-1]).float(), s[:, :-1], delta[:, :-1], f, True)  # sign lost
    assert not ok
    ok, _ = R.head_out_check(torch.exp(s[:, -1]).float(), s[:, -1], delta[:, -1], fc, False)  # the + 1 lost
    assert not ok
    ok, _ = R.head_out_check((hidden.double() @ w.double().T + b.double())[:, :-1].float(), s[:, :-1], delta[:, :-1],
                             R.ACTS["linear"], True)  # the hidden ReLU lost
    assert not ok


# ---------------------------------------------------------------- unprojection
def test_unproject_reference_and_fp32_bound():
    depth, extr, intr = R.unproject_inputs()
    ref, mag = R.unproject(depth, extr, intr)
    assert (mag >= ref.abs() * (1 - 1e-12)).all() and depth.min() == 0 and depth.max() == 1e3
    S, H, W = depth.shape
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    got = []
    for s in range(S):  # the same formula in fp32
        K, E, d = intr[s], extr[s], depth[s]
        cam = torch.stack([(u - K[0, 2]) * d / K[0, 0], (v - K[1, 2]) * d / K[1, 1], d], -1)
        got.append(cam @ E[:, :3] + (-(E[:, :3].T @ E[:, 3])))
    r = R.ratio(torch.stack(got), ref, 16 * R.U * mag)
    assert r < 1
    print(f"BOUND unproject {r:.3f}")


# ---------------------------------------------------------------- the whole head
def test_head_oracle_shapes_and_fp32_metric():
    """The fp64 oracle returns the reference's [B,S,oh,ow,...] and the fp32 oracle sits a rounding
    error away: the GPU file allows the kernels 4 x these figures."""
    for name, (cfg, B, S, H, W) in R.HEAD_CONFIGS.items():
        c = R.head_case(name)
        oh, ow = (H // 14) * 14 // cfg.get("down_ratio", 1), (W // 14) * 14 // cfg.get("down_ratio", 1)
        if cfg.get("feature_only"):
            assert c["ref"][0].shape == (B, S, 64, oh, ow)
        else:
            assert c["ref"][0].shape == (B, S, oh, ow, 3) and c["ref"][1].shape == (B, S, oh, ow)
        assert all(0 < m < 1e-4 for m in c["cpu_metric"]), (name, c["cpu_metric"])
        print("HEAD", name, " ".join(f"{m:.2e}" for m in c["cpu_metric"]))
