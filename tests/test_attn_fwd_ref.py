"""The attention-forward oracle checks itself (tests/attn_fwd_ref.py), on the CPU.

Why this file exists: the suite's older forward tests pool 128-258 sampled rows into one rel-L2 below
1e-2.  The mutants below -- a tail key leaking into one 32-row q-block, a q-block that drops its
segment's last key, one wave whose P.V operand is biased by 2^-6 -- each leave the whole-tensor error
of the launch BELOW that 1e-2 (and inside 1.5 x the rounding model, for the 4133-row case), while the
per-row metric of errors() rises to 2.9 - 34 x the clean model's.  tests/test_attn_fwd_oracle_gpu.py
asserts both metrics over every row for that reason.  (A P.V bias of one bf16 ulp, 2^-8, is below
what either metric resolves: test_mutant_one_wave_biases_p has the figures.)

  * exact() is torch's fp64 scaled_dot_product_attention with the equivalent dense mask to 1e-12 on
    frame, reloc and merge-in (the layout conventions, two segments, the union merge), agrees with
    attn_bwd_ref.exact()'s O and lse, and handles the fp32 kernels' three masks with a fully masked
    row (zeros, lse -inf);
  * modelled() with no rounding is exact();
  * caps: the KERNEL_MODEL error against exact() is below the suite's 1e-2 for flat, gain2.5, spike,
    vtiny, vbig and below 1.5e-2 for the gain-4 kinds, so no kind needs a bound of its own;
  * constructions: paths() -- sr_attn.hip's published per-wave decision -- puts every kind's rows
    where attn_fwd_ref.make() says, with the clearances the GPU file's exact sweep_stats lean on;
  * the mutants.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import attn_bwd_ref as B
import attn_fwd_ref as R

TOL = 1e-2  # the suite's bf16 attention-forward bound (tests/test_kernels_gpu.py, test_baseline_shapes_gpu.py)
TOL_GAIN4 = 1.5e-2
GAIN4_KINDS = ("gain4", "clustered4", "mixed")
CAP_CASES = ["frame", "global-ragged"]


def _sdpa64(q, k, v, scale, mask=None):
    """[H, n, D] operands: torch's own fp64 attention and log2-domain lse"""
    o = F.scaled_dot_product_attention(q.double()[None], k.double()[None], v.double()[None], attn_mask=mask,
                                       scale=scale)[0]
    s = q.double() @ k.double().transpose(-1, -2) * scale
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf) if mask.dtype == torch.bool else s + mask
    return o, torch.logsumexp(s, -1) / math.log(2.0)


@pytest.mark.parametrize("case", ["frame", "reloc", "merge-in"])
def test_exact_matches_sdpa64(case):
    t, geo = R.make(case, "gain2.5"), R.geometry(case)
    H, lq = geo["heads"], geo["lq"]
    got = R.run_exact(case, t)
    for b in range(geo["batch"]):
        kk, vv = R._keys(t["k0"], t["v0"], t["k1"], t["v1"], b, H, geo["l0"], geo["k0_bstride"], geo.get("l1", 0),
                         geo.get("k1_bstride", 0))
        o, lse = _sdpa64(B._heads(t["q"], b * geo["q_bstride"], lq, H), kk, vv, 0.125)
        rs = slice(b * geo["q_bstride"], b * geo["q_bstride"] + lq)
        assert R.errors(got.o[rs], B._rows(o))[0] < 1e-12, b
        assert R.lse_error(got.lse[b], lse) < 1e-12 * float(lse.abs().max()), b


def test_exact_agrees_with_the_backward_oracle():
    t, geo = R.make("reloc", "gain4"), R.geometry("reloc")
    a = R.run_exact("reloc", t)
    b = B.exact(t["q"], t["k0"], t["v0"], torch.zeros_like(t["q"]), k1=t["k1"], v1=t["v1"], **geo)
    assert R.errors(a.o, b.o)[0] < 1e-13 and R.lse_error(a.lse, b.lse) < 1e-11


@pytest.mark.parametrize("mode", ["camera", "dense", "add"])
def test_exact_masks_match_sdpa64(mode):
    """two segments for dense / add, one for camera (the kernel's rule); one row sees no key"""
    torch.manual_seed(5)
    H, D, lq, l0, l1, batch = 2, 16, 23, 19, 0 if mode == "camera" else 11, 2
    C, L = H * D, l0 + (0 if mode == "camera" else 11)
    q, k0, v0 = torch.randn(batch * lq, C), torch.randn(batch * l0, C), torch.randn(batch * l0, C)
    k1, v1 = (None, None) if not l1 else (torch.randn(l1, C), torch.randn(l1, C))
    if mode == "camera":
        n_anchor, mask = 0, None  # rows i >= l0 see nothing
        see = (torch.arange(L)[None] == torch.arange(lq)[:, None]).expand(batch, H, lq, L)
    else:
        n_anchor = 0
        see = torch.rand(batch, H, lq, L) < 0.6
        see[:, :, 7] = False
        mask = see if mode == "dense" else torch.where(see, torch.randn(batch, H, lq, L), -math.inf)
    got = R.exact(q, k0, v0, heads=H, batch=batch, lq=lq, q_bstride=lq, l0=l0, k0_bstride=l0, k1=k1, v1=v1, l1=l1,
                  k1_bstride=0, scale=0.3, mask_mode=mode, mask=mask, n_anchor=n_anchor)
    dead = ~see.any(-1)
    assert int(dead.sum()) > 0
    for b in range(batch):
        kk, vv = R._keys(k0, v0, k1, v1, b, H, l0, l0, l1, 0)
        m = see[b] if mode != "add" else mask[b].double()
        o, lse = _sdpa64(B._heads(q, b * lq, lq, H), kk, vv, 0.3, m)
        live = ~dead[b]
        go = B._heads(got.o, b * lq, lq, H)
        assert float((go[live] - o[live]).abs().max()) < 1e-12
        assert float(go[~live].abs().max()) == 0.0 and bool((got.lse[b][~live] == -math.inf).all())
        assert float((got.lse[b][live] - lse[live]).abs().max()) < 1e-12


@pytest.mark.parametrize("case", ["reloc", "frame-tiles", "merge-in", "keysplit"])
def test_modelled_without_rounding_is_exact(case):
    t = R.make(case, "gain4")
    kw = dict(parts=5) if case == "keysplit" else {}
    a, b = R.run_exact(case, t, **kw), R.run_exact(case, t, rounding=(), **kw)
    assert R.errors(b.o, a.o)[0] <= 1e-13 and R.lse_error(b.lse, a.lse) <= 1e-11
    if case in ("merge-in", "keysplit"):  # the split routes are the unsplit softmax
        geo = R.geometry(case)
        c = R.exact(t["q"], t["k0"], t["v0"], **geo)
        assert R.errors(a.o, c.o)[0] <= 1e-13 and R.lse_error(a.lse, c.lse) <= 1e-11


def test_q_scaled_is_the_same_function():
    t, geo = R.make("frame-tiles", "gain2.5"), R.geometry("frame-tiles")
    cq = (t["q"].float() * R._c32(0.125)).to(torch.bfloat16).float()
    a = R.modelled(t["q"], t["k0"], t["v0"], **geo)
    b = R.modelled(cq, t["k0"], t["v0"], q_scaled=True, **geo)
    assert torch.equal(a.o, b.o) and torch.equal(a.lse, b.lse)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", CAP_CASES)
def test_model_stays_below_the_suite_bounds(case, kind):
    whole, row, lse = R.model_errors(case, kind)
    print(f"{case:14s} {kind:10s} KERNEL_MODEL whole {whole:.2e} row {row:.2e} lse {lse:.2e}")
    assert whole < (TOL_GAIN4 if kind in GAIN4_KINDS else TOL)


@pytest.mark.parametrize("parts", R.KEYSPLIT_PARTS)
def test_key_split_model_stays_below_the_suite_bound(parts):
    whole, row, lse = R.model_errors("keysplit", "flat", parts)
    print(f"keysplit parts {parts:2d} KERNEL_MODEL whole {whole:.2e} row {row:.2e} lse {lse:.2e}")
    assert whole < TOL


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["frame", "frame-tiles", "reloc", "global-tiles", "global-ragged", "subsample"])
def test_constructions_reach_their_paths(case):
    geo = R.geometry(case)
    rows = geo["batch"] * geo["heads"] * geo["lq"]
    waves = geo["batch"] * geo["heads"] * -(-geo["lq"] // 64)
    P = {kind: R.paths(R.make(case, kind), geo) for kind in R.KINDS}
    for kind, p in P.items():
        print(f"{case:14s} {kind:10s} asm {p.asm} compiled {p.compiled} m=0 {p.m_zero} m>0 {p.m_fixed} outside "
              f"{p.outside} clearance {p.clearance:.1f} bound {float(p.qb.min()):.1f}..{float(p.qb.max()):.1f}")
        assert p.asm + p.compiled == waves
    for kind in ("flat", "vtiny", "vbig"):  # bound ~ 12: m = 0 everywhere
        assert P[kind].m_zero == rows and float(P[kind].qb.max()) < 30 and P[kind].clearance > 20
    p = P["gain2.5"]  # 64 < bound < 110: m = bound - 64 > 0, and m + bound <= 110 needs no pre-pass
    assert p.m_fixed == rows and 64 < float(p.qb.min()) and 2 * float(p.qb.max()) - 64 < R.FIX_LO
    p = P["gain4"]  # bound ~ 185: m ~ 121, inside the window only by what the pre-pass finds
    assert p.m_fixed == rows and float(p.qb.min()) - 64 > R.FIX_LO and p.compiled == 0 and p.clearance > 20
    # clustered4: the 2-norm bound alone loses rows, the boxes keep every wave on the sweep
    t = R.make(case, "clustered4")
    assert t["query_norm_max"] > 0 and P["clustered4"].compiled == 0 and P["clustered4"].clearance > 20
    assert R.paths(dict(t, query_norm_max=0.0), geo).outside > rows // 4
    # mixed: even waves inside, odd waves outside, each by >= 20 (log2)
    p, t = P["mixed"], R.make(case, "mixed")
    assert p.clearance >= 20
    m_fix = (p.qb - 64).clamp_min(0.0)
    inside = (m_fix - p.mx3 <= R.FIX_LO)
    odd = (torch.arange(geo["lq"]) // 64 % 2).bool()
    assert bool(inside[..., ~odd].all()) and not bool(inside[..., odd].any())
    n_odd = geo["lq"] // 64 // 2 + (1 if geo["lq"] % 128 > 64 else 0)
    assert p.compiled == geo["batch"] * geo["heads"] * n_odd and p.asm == waves - p.compiled
    # spike: both keys score ~ SPIKE_LOG2 above every other key, in every row; the first lies behind
    # tile 2, the second in the last tile of its segment
    t = R.make(case, "spike")
    j0, j1 = R.spike_keys(case)
    assert j0 == 3 * R.KT and j1 // R.KT == (geo["l0"] - 1) // R.KT
    ex = R.paths(t, geo)
    assert ex.compiled == 0
    c = 0.125 * R.LOG2E
    for b in range(geo["batch"]):
        kk, _ = R._keys(t["k0"], t["v0"], t["k1"], t["v1"], b, geo["heads"], geo["l0"], geo["k0_bstride"],
                        geo.get("l1", 0), geo.get("k1_bstride", 0))
        s = (B._heads(t["q"], b * geo["q_bstride"], geo["lq"], geo["heads"]).double() @ kk.double().transpose(1, 2)) * c
        sp = s[..., [j0, j1]].min(-1).values
        s[..., [j0, j1]] = -math.inf
        gap = sp - s.max(-1).values
        assert 20 < float(gap.min()) and abs(float(gap.median()) - R.SPIKE_LOG2) < 8, (float(gap.min()), float(gap.median()))
        assert float((sp - ex.mx3[b]).min()) > 20  # the pre-pass did not see them


# ------------------------------------------------------------------------------------------------
def _mutant(case, kind, mutant):
    r = R.reference(case, kind)
    t = r["inputs"]
    bad = R.modelled(t["q"], t["k0"], t["v0"], k1=t["k1"], v1=t["v1"], mutant=mutant, **r["kw"])
    clean = R.errors(r["model"].o, r["exact"].o)
    got = R.errors(bad.o, r["exact"].o)
    print(f"{case:14s} {kind:6s} clean whole {clean[0]:.2e} row {clean[1]:.2e} | mutant whole {got[0]:.2e} "
          f"row {got[1]:.2e} ({got[1] / clean[1]:.1f} x)")
    return clean, got


def test_mutant_tail_key_leaks_into_one_q_block():
    """(a) rows 4096-4127 of global-ragged also attend to the first row behind the keys -- a readable
    tail as production has it (the next rows' data: a key and value like the others)."""
    C = R.heads_of("global-ragged") * 64
    g = torch.Generator().manual_seed(99)
    leak = (R.bf16(torch.randn(1, C, generator=g)), R.bf16(torch.randn(1, C, generator=g)))
    clean, got = _mutant("global-ragged", "flat", R.Mutant(0, slice(4096, 4128), leak))
    assert got[1] > 2 * clean[1] and got[0] < TOL and got[0] < 1.5 * clean[0]


def test_mutant_last_q_block_drops_the_final_key():
    """(b) the last 32-row q-block of frame (rows 320-336 of the last item) loses key 336"""
    clean, got = _mutant("frame", "flat", R.Mutant(2, slice(320, 337), None, True))
    assert got[1] > 2 * clean[1] and got[0] < TOL


def test_mutant_one_wave_biases_p():
    """(c) wave 2 (rows 128-191) forms P.V from bf16(P (1 + bias)) while the row sum keeps bf16(P):
    numerator and denominator no longer see the same P (a bias on the P both MFMAs share cancels in
    O altogether).  What the metrics resolve, measured:
      * 2^-8 on global-ragged / mixed, as first proposed: NOT visible to either metric.  O moves by
        3.9e-3 of itself on 64 rows, while bf16(O) alone is 2^-9 per element and mixed's own outside
        rows (gain 4, peaked softmax) put the clean row metric at 1.3e-1: row 1.00 x, whole 1.00 x.  On
        flat it is 1.06 x (6.5e-3 against 6.2e-3).  A one-ulp bias of P is below what a max-over-rows
        metric at 2 x can see; the GPU test's whole-tensor margin (1.5 x) does not see it either.
      * 2^-6 on global-ragged / flat: row 2.9 x the clean model (1.8e-2 against 6.2e-3), whole 3.5e-3
        (1.2 x): flagged by the row metric, missed by the pooled one.
    Both are asserted as measured, so a change of the metric that moves either shows here."""
    clean, got = _mutant("global-ragged", "mixed", R.Mutant(0, slice(128, 192), None, False, 2.0 ** -8))
    assert got[0] < TOL_GAIN4 and got[0] < 1.5 * clean[0]  # the pooled metric misses it ...
    assert got[1] < 2 * clean[1]  # ... and so does the row metric (see above)
    clean, got = _mutant("global-ragged", "flat", R.Mutant(0, slice(128, 192), None, False, 2.0 ** -8))
    assert got[1] < 2 * clean[1] and got[0] < 1.5 * clean[0]
    clean, got = _mutant("global-ragged", "flat", R.Mutant(0, slice(128, 192), None, False, 2.0 ** -6))
    assert got[1] > 2 * clean[1] and got[0] < TOL and got[0] < 1.5 * clean[0]
