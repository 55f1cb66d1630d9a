"""The attention-backward oracle checks itself (tests/attn_bwd_ref.py), on the CPU:

  * exact() is torch's fp64 autograd of softmax attention to 1e-12, on a two-segment case with a
    shared anchor segment (the layout conventions: column heads, batch strides, stride-0 sums);
  * modelled() with no rounding is exact();
  * every case tests/test_attn_bwd_oracle_gpu.py asserts has room under the caps it asserts: the
    kernel is allowed 1.5 x the DESIGN model's whole-tensor error and, paired with the forward kernel,
    the suite's 2e-2, so 1.5 x DESIGN < 2e-2 for the logit gains <= 4 that leg asserts; and the FLASH
    model (no operand prescale rounding) is never worse than DESIGN, which is what makes the
    DESIGN / FLASH ratio the cost of that rounding;
  * an fp32 run of exact() is within the fp32 kernel's 2e-5 of the fp64 run on every case of the
    fp32 leg, so that bound measures the kernel and not the reference.
"""

import pytest
import torch

import attn_bwd_ref as R

TOL = 2e-2  # the suite's bf16 attention-backward bound (tests/test_attn_bwd_gpu.py)
TOL_F32 = 2e-5
BF16_CASES = list(R.CASES)
F32_CASES = ["frame-small", "reloc-small", "anchor"]


def test_exact_matches_autograd64():
    """B = 3 items, 2 heads, a shared anchor segment (stride 0) plus each item's own rows."""
    torch.manual_seed(3)
    B, P, A, H, D = 3, 37, 29, 2, 16
    C = H * D
    scale = 0.31
    q, k, v, g = (torch.randn(B * P, C, dtype=torch.float64) for _ in range(4))
    k0, v0 = torch.randn(A, C, dtype=torch.float64), torch.randn(A, C, dtype=torch.float64)
    r = R.exact(q, k0, v0, g, heads=H, batch=B, lq=P, q_bstride=P, l0=A, k0_bstride=0, k1=k, v1=v, l1=P,
                k1_bstride=P, scale=scale)
    hd = lambda t, r0, n: t[r0:r0 + n].reshape(n, H, D).transpose(0, 1)  # noqa: E731
    un = lambda x: x.transpose(0, 1).reshape(x.shape[1], C)  # noqa: E731
    dk0, dv0 = torch.zeros(A, C, dtype=torch.float64), torch.zeros(A, C, dtype=torch.float64)
    for b in range(B):
        kk, vv = torch.cat([hd(k0, 0, A), hd(k, b * P, P)], 1), torch.cat([hd(v0, 0, A), hd(v, b * P, P)], 1)
        o, dq, dk, dv = R.autograd64(hd(q, b * P, P), kk, vv, hd(g, b * P, P), scale)
        rs = slice(b * P, (b + 1) * P)
        for name, got, want in (("o", r.o[rs], un(o)), ("dq", r.dq[rs], un(dq)), ("dk1", r.dk1[rs], un(dk[:, A:])),
                                ("dv1", r.dv1[rs], un(dv[:, A:]))):
            assert R.errors(got, want, D)[0] < 1e-12, (b, name)
        assert float((r.lse[b] - R.lse2(hd(q, b * P, P), kk, scale)).abs().max()) < 1e-12
        dk0 += un(dk[:, :A])
        dv0 += un(dv[:, :A])
    assert R.errors(r.dk0, dk0, D)[0] < 1e-12 and R.errors(r.dv0, dv0, D)[0] < 1e-12


@pytest.mark.parametrize("case", ["reloc-small", "frame-small"])
def test_modelled_without_rounding_is_exact(case):
    t, kw = R.make(case, "gain4"), R.geometry(case)
    args = (t["q"], t["k0"], t["v0"], t["g"])
    a = R.exact(*args, k1=t["k1"], v1=t["v1"], **kw)
    b = R.modelled(*args, k1=t["k1"], v1=t["v1"], **kw, rounding=())
    for name in R.Grads._fields:
        x, y = getattr(a, name), getattr(b, name)
        if x is not None:
            assert float((x - y).abs().max()) <= 1e-13 * float(x.abs().max()), name


def test_exact_over_live_rows_is_exact_where_do_is_zero():
    """A query row with dO = 0 contributes nothing: exact() over the other rows alone gives the same
    dK / dV, and the dropped rows' dQ is zero (what the GPU file's sparse_do check leans on)."""
    r = R.reference("reloc-small", "sparse_do")
    live = r["inputs"]["live"]
    assert 0 < int(live.sum()) < live.numel() // 8
    for name in R.OUTPUTS:
        assert R.errors(getattr(r["exact_live"], name), getattr(r["exact"], name))[0] < 1e-12, name
    assert float(r["exact"].dq[~live.reshape(-1)].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["flat", "gain4", "gain8", "lossscale"])
@pytest.mark.parametrize("case", BF16_CASES)
def test_model_leaves_room_under_the_caps(case, kind):
    r = R.reference(case, kind)
    for name in R.OUTPUTS:
        ref = getattr(r["exact"], name)
        if ref is None:
            continue
        dw, dr = R.errors(getattr(r["design"], name), ref)
        fw, fr = R.errors(getattr(r["flash"], name), ref)
        print(f"{case:12s} {kind:9s} {name:3s} DESIGN {dw:.2e} row {dr:.2e}  FLASH {fw:.2e} row {fr:.2e}  "
              f"ratio {dw / fw:.2f}")
        assert fw <= dw, (name, fw, dw)
        if R.GAIN[kind] <= 4:
            assert 1.5 * dw < TOL, (name, dw)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["flat", "gain4"])
@pytest.mark.parametrize("case", F32_CASES)
def test_fp32_reference_noise_is_below_the_fp32_bound(case, kind, D):
    t, kw = R.make(case, kind, head_dim=D, round_bf16=False), R.geometry(case)
    args = (t["q"], t["k0"], t["v0"], t["g"])
    a = R.exact(*args, k1=t["k1"], v1=t["v1"], **kw)
    b = R.exact(*args, k1=t["k1"], v1=t["v1"], **kw, dtype=torch.float32)
    for name in R.OUTPUTS:
        if getattr(a, name) is not None:
            w, row = R.errors(getattr(b, name), getattr(a, name), D)
            print(f"{case:12s} {kind:5s} D={D:3d} {name:3s} fp32 exact vs fp64: {w:.2e} row {row:.2e}")
            assert w < TOL_F32, (name, w)
