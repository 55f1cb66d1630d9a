"""tests/gemm_ref.py on the CPU: its fp64 references agree with torch's own fp64 ops, a correct
fp32-accumulate / round-once implementation (torch's CPU ops) meets every bound at every case, every
mutant fails its bound at the case built for it -- and the mutants a Frobenius norm cannot see pass the
GPU suite's ``rel() < tol`` -- and the restated index functions are bijective.

Every bounded test prints "BOUND <epilogue> <tensor> <dtype> <worst ratio> <share of two-valued
intervals>"; DESIGN.md records them.
"""

import math

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R
from gemm_ref import BF16, F32, F64, C


def rel(a, b):  # tests/test_kernels_gpu.py's measure
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _got(c, mutant):
    """What a kernel with the defect would store: the mutated fp64 value rounded once."""
    return {k: R.store(v, R.out_dtype(c) if k == "out" else c["dtype"])
            for k, (v, _) in R.evaluate(c, R.inputs(c), mutant).items()}


def _ok(c, got, name="out"):
    ref, delta = R.reference(c)[name]
    return R.check(got, ref, delta)[0]


# ---------------------------------------------------------------- the references against torch's fp64 ops
def test_case_names_are_unique():
    names = [c["name"] for c in R.ALL_SMALL + [c for cs in R.GROUP4.values() for c in cs] + R.k256_cases(R.K256_M)]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_references_match_torch_fp64(dtype):
    M, N, kt = 37, 128, 2
    for epi, kw in (("bias", dict(q_scale=0.125, q_cols=64)), ("f32", {}), ("gelu", dict(aux=True)), ("resid", {}),
                    ("patch", {}), ("gelu_bwd", {}), ("qkv", dict(embed_dim=64, aux=True, q_scale=0.125, q_cols=64))):
        c = C("k128", epi, dtype, M, N, kt, tag="torch", **kw)
        inp = R.inputs(c)
        ref = {k: v for k, (v, _) in R.evaluate(c, inp).items()}
        a, w = inp["a"].double(), inp["w"].double()
        S = F.linear(a, w, inp["bias"].double() if "bias" in inp else None)
        if epi == "bias":
            want = torch.cat([S[:, :64] * 0.125, S[:, 64:]], 1)
        elif epi == "f32":
            want = S
        elif epi == "gelu":
            want = F.gelu(S)
            assert (ref["aux"] - S).abs().max() < 1e-12
        elif epi == "resid":
            want = inp["x0"].double() + inp["gamma"].double() * S
        elif epi == "patch":
            want = inp["x0"].double().clone()
            for r in range(M):
                f, p = divmod(r, c["seg_rows"])
                want[f * c["seg_stride"] + c["seg_offset"] + p] = S[r] + inp["row_add"][p].double()
        elif epi == "gelu_bwd":
            u = inp["aux_in"].double().requires_grad_(True)
            (gp,) = torch.autograd.grad(F.gelu(u).sum(), u)
            want = F.linear(a, w) * gp
        else:
            from oracle import sfm_oracle as O
            assert (ref["aux"] - S).abs().max() < 1e-12
            pos = R.rope_pos(c, inp)
            cos, sin = O.rope_tables(32, c["rope_npos"])
            assert torch.equal(cos[:, :16], inp["rope_cos"]) and torch.equal(sin[:, :16], inp["rope_sin"])
            # the oracle in fp64, with the stored fp32 tables (rope2d builds them in fp32 itself)
            q = F.layer_norm(S[:, :64], (64,), inp["qn_w"].double(), inp["qn_b"].double(), 1e-5)
            k = F.layer_norm(S[:, 64:], (64,), inp["kn_w"].double(), inp["kn_b"].double(), 1e-5)
            q, k = _rope2d64(O, q, pos), _rope2d64(O, k, pos)
            want = torch.cat([q * 0.125, k], 1)
        assert (ref["out"] - want).abs().max() < 1e-12, epi


def _rope2d64(O, t, pos):
    """oracle.sfm_oracle.rope2d on fp64 values: its fp32 tables widen exactly, as the kernel's do."""
    out = O.rope2d(t[None, None], pos[None])
    assert out.dtype == F64
    return out[0, 0]


def test_rope_pos_modes():
    c = C("k128", "qkv", F32, 50, 64, 1, embed_dim=64, pos="grid", pos_row_base=7, tag="pos")
    pos = R.rope_pos(c, R.inputs(c))
    for r in range(50):
        t = (r + 7) % 21
        want = (0, 0) if t < 5 else ((t - 5) // 4 + 1, (t - 5) % 4 + 1)
        assert tuple(pos[r].tolist()) == want
    c = C("k128", "qkv", F32, 50, 64, 1, embed_dim=64, pos="rowmap", tag="posmap")
    inp = R.inputs(c)
    pos = R.rope_pos(c, inp)
    t = int(inp["pos_rowmap"][49]) % 21
    assert tuple(pos[49].tolist()) == ((0, 0) if t < 5 else ((t - 5) // 4 + 1, (t - 5) % 4 + 1))
    assert int(pos.max()) <= 4 and int(pos.max()) == 4  # inside, and reaching, the 5-row table


def test_bf16_rounding_from_fp64():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.0,
                      3.0e-5, -123.456], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.0, 0.0], dtype=F64)
    assert torch.equal(R.bf16_rne(x)[:6], want)  # ties to even; just past a tie rounds up (fp32 would lose the 2^-40)
    assert torch.equal(R.bf16_rne(x)[6:], x[6:].float().to(BF16).double())
    g = torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=F64)
    # against torch's fp64 -> fp32 -> bf16: equal except where the detour through fp32 rounds twice
    assert float((R.bf16_rne(g) != g.float().to(BF16).double()).double().mean()) < 1e-3
    assert float((R.bf16_rne(g) - g).abs().div(g.abs()).max()) <= 2.0 ** -8


def test_abramowitz_stegun_erf():
    """A&S 7.1.26 in fp64 against torch.erf on a dense grid: the published 1.5e-7, which EPS_H halves."""
    x = torch.linspace(-12, 12, 2_400_001, dtype=F64)
    erf_as = torch.sign(x) * (1 - 2 * R.phi_tail_as(x * math.sqrt(2.0)))
    e = float((erf_as - torch.erf(x)).abs().max())
    print(f"A&S 7.1.26 max |erf error| {e:.3e}")
    assert e <= 1.5e-7
    eg = float((R.gelu_as(x) - R.gelu_erf(x)).abs().div(x.abs().clamp_min(1e-30)).max())
    assert eg <= 0.75e-7 + 1e-12                      # |gelu_as - gelu| <= |x| 0.75e-7
    ed = float((R.gelu_grad_as(x) - R.gelu_grad(x)).abs().max())
    assert ed <= 0.75e-7 + 1e-12
    u = x.clone().requires_grad_(True)
    (gp,) = torch.autograd.grad(F.gelu(u).sum(), u)
    assert float((R.gelu_grad(x) - gp).abs().max()) < 1e-12
    assert float(R.gelu_grad(x).abs().max()) <= R.GELU_SLOPE


# ---------------------------------------------------------------- a correct implementation meets every bound
def _model_worst(cases):
    worst = {}
    for c in cases:
        inp = R.inputs(c)
        got = R.model(c, inp)
        for name, (ref, delta) in R.reference(c).items():
            ok, ratio, share = R.check(got[name], ref, delta)
            assert ok, (c["name"], name, ratio)
            key = (c["epi"], name, "bf16" if got[name].dtype == BF16 else "f32")
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], ratio), max(w[1], share))
        if c.get("colsum"):
            ref, bound = R.colsum_ref(got["out"])
            ok, ratio, _ = R.check(got["colsum"], ref, bound)
            assert ok, (c["name"], "colsum", ratio)
            key = ("gelu_bwd", "colsum", "f32")
            worst[key] = (max(worst.get(key, (0.0, 0.0))[0], ratio), 0.0)
    return worst


@pytest.mark.parametrize("group", ["k128", "k64", "splitk", "group", "group_switch", "group4"])
def test_correct_model_meets_every_bound(group):
    cases = {"k128": R.CASES_K128, "k64": R.CASES_K64 + R.CASES_K64_OFF, "splitk": R.CASES_SPLITK,
             "group": R.CASES_GROUP, "group_switch": R.CASES_GROUP_SWITCH,
             "group4": [c for cs in R.GROUP4.values() for c in cs]}[group]
    for (epi, name, dt), (ratio, share) in sorted(_model_worst(cases).items()):
        print(f"BOUND {epi} {name} {dt} {ratio:.4f} {share:.4f}")


def test_constant_head_row_stays_bounded():
    """QKV with a head row of variance 0 (A row 0 is zero, the head's bias constant): rstd = eps^-1/2,
    and the bound stays finite and is met by the fp32 model."""
    c = C("k128", "qkv", F32, 16, 128, 1, embed_dim=64, tag="const")
    inp = dict(R.inputs(c))
    inp["a"] = inp["a"].clone()
    inp["a"][0] = 0
    inp["bias"] = inp["bias"].clone()
    inp["bias"][:64] = 0.7
    ref, delta = R.evaluate(c, inp)["out"]
    assert bool(torch.isfinite(delta).all()) and float(delta[0, :64].max()) < 1e-2
    ok, ratio, _ = R.check(R.model(c, inp)["out"], ref, delta)
    print(f"BOUND qkv constant-row {ratio:.4f}")
    assert ok


# ---------------------------------------------------------------- every mutant fails its bound
_RAGGED = dict(M=127, N=124, kt=2)
MUTANTS = [
    ("acc_bf16", C("k128", "bias", BF16, 127, 124, 2)),
    ("acc_bf16", C("k128", "resid", BF16, 127, 124, 2)),
    ("bias_shift", C("k128", "bias", BF16, 127, 124, 2)),
    ("bias_shift", C("k128", "bias", F32, 127, 124, 2)),
    ("gamma_shift", C("k128", "resid", BF16, 127, 124, 2)),
    ("row_m2", C("k128", "bias", BF16, 129, 132, 2)),
    ("row_m2", C("group", "bias", BF16, 257, 256, 3)),
    ("drop_kt", C("k128", "bias", BF16, 129, 132, 2)),
    ("drop_kt", C("group", "f32", BF16, 257, 256, 3)),
    ("drop_kt", C("splitk", "bias", F32, 130, 132, 2, splits=2, tag="s2")),
    ("qscale_post", C("k128", "bias", BF16, 128, 128, 1, q_scale=0.125 * 1.1, q_cols=64, tag="qpost")),
    ("qscale_wide", C("k128", "bias", BF16, 128, 128, 1, q_scale=0.125, q_cols=64, tag="qcols64")),
    ("qscale_wide", C("group", "qkv", BF16, 257, 512, 1, aux=True, **R._QKV512)),
    ("pos_prev", C("k128", "qkv", BF16, 65, 128, 1, embed_dim=64, aux=True)),
    ("pos_prev", C("group", "qkv", BF16, 257, 256, 3, aux=True, **R._QKV256)),
    ("ln_on_aux", C("k128", "qkv", BF16, 65, 128, 1, embed_dim=64, aux=True)),
    ("gelu_tanh", C("k128", "gelu", BF16, 127, 124, 2, aux=True)),
    ("gelu_tanh", C("k128", "gelu", F32, 127, 124, 2, aux=True)),
    ("patch_special", C("k128", "patch", BF16, 127, 124, 2)),
]


@pytest.mark.parametrize("mutant,case", MUTANTS, ids=[f"{m}-{c['name']}" for m, c in MUTANTS])
def test_mutant_fails_its_bound(mutant, case):
    if mutant == "pos_prev":
        pos = R.rope_pos(case, R.inputs(case))
        assert not torch.equal(pos[-1], pos[-2])
    assert _ok(case, _got(case, None)["out"])          # the unmutated value, rounded once, is inside
    assert not _ok(case, _got(case, mutant)["out"])


def test_qscale_post_needs_a_scale_that_is_no_power_of_two():
    """c * bf16(S) rounded again equals bf16(c * S) for c = 2^-3 (scaling by a power of two commutes with
    rounding): the defect is visible only with another scale, which is why the (e) case uses 0.1375."""
    c = C("k128", "bias", BF16, 128, 128, 1, q_scale=0.125, q_cols=64, tag="qcols64")
    assert _ok(c, _got(c, "qscale_post")["out"])


@pytest.mark.parametrize("mutant", ["colsum_unrounded", "colsum_shift"])
def test_colsum_mutants_fail(mutant):
    c = C("k128", "gelu_bwd", BF16, 129, 132, 2, colsum=True)
    v = R.reference(c)["out"][0]
    stored = R.store(v, BF16)
    ref, bound = R.colsum_ref(stored)
    assert R.check(ref.float(), ref, bound)[0]
    bad, _ = R.colsum_ref(stored, mutant, unrounded=v)
    assert not R.check(bad.float(), ref, bound)[0]


# ---------------------------------------------------------------- ... and the norm does not see them
def _rel_of(c, mutant):
    """rel() of the mutated result against the GPU suite's reference, a.float() @ w.float().t() + b."""
    inp = R.inputs(c)
    base = inp["a"].float() @ inp["w"].float().t() + inp["bias"]
    if c["epi"] == "gelu":
        base = F.gelu(base)
    elif c.get("q_scale"):
        base[:, :c["q_cols"]] *= c["q_scale"]
    return rel(_got(c, mutant)["out"].float(), base)


NORM_BLIND = [
    ("acc_bf16", C("k128", "bias", BF16, 300, 256, 16, tag="norm")),
    ("qscale_post", C("k128", "bias", BF16, 300, 256, 16, q_scale=0.1375, q_cols=128, tag="norm")),
    # K = 128 (the suite's (1374, 384, 128)): at K = 1024 gamma(K) mag(S) = 1.4e-3 exceeds |tanh form - erf form|
    ("gelu_tanh", C("k128", "gelu", BF16, 300, 256, 2, tag="norm")),
    # one wrong row, or one short row, of 43,777: test_gemm256_tiles' kind of shape (the last 256-row tile holds one row)
    ("row_m2", C("k256", "bias", BF16, 171 * 256 + 1, 256, 2, tag="norm")),
    ("drop_kt", C("k256", "bias", BF16, 171 * 256 + 1, 256, 2, tag="norm")),
]


@pytest.mark.parametrize("mutant,case", NORM_BLIND, ids=[m for m, _ in NORM_BLIND])
def test_mutant_passes_the_norm_and_fails_the_bound(mutant, case):
    r = _rel_of(case, mutant)
    clean = _rel_of(case, None)
    print(f"NORM {mutant} rel {r:.3e} (correct: {clean:.3e}) tol 8e-3")
    assert r < 8e-3
    assert not _ok(case, _got(case, mutant)["out"])


def test_shifted_bias_vector_and_the_norm():
    """(b): with O(1) bias the last 4 columns of N carry rel = sqrt(4 / N) of the norm, so at the suite's
    ragged widths (388, 2052) the norm does see it (0.1, 0.044); it passes 8e-3 only past N = 1e5
    (S and the bias have variance 1 each), where the bound still fails."""
    small = C("k64", "bias", BF16, 64, 388, 4, tag="norm")
    assert _rel_of(small, "bias_shift") > 8e-3 and not _ok(small, _got(small, "bias_shift")["out"])
    wide = C("k64", "bias", BF16, 4, 131076, 1, tag="norm")
    r = _rel_of(wide, "bias_shift")
    print(f"NORM bias_shift N=131076 rel {r:.3e}")
    assert r < 8e-3 and not _ok(wide, _got(wide, "bias_shift")["out"])


# ---------------------------------------------------------------- the pure index functions
@pytest.mark.parametrize("group_m", [0, 3, 4])
@pytest.mark.parametrize("M,N", [(1025, 512), (513, 768), (257, 256), (1, 256), (2049, 1024)])
def test_tile_origin_is_a_bijection(M, N, group_m):
    ntn, ntm = N // 256, -(-M // 256)
    seen = {R.tile_origin(t, M, N, group_m) for t in range(ntn * ntm)}
    assert seen == {(i, j) for i in range(ntm) for j in range(ntn)}


def test_group_starts_pad_to_eight():
    for cs in R.GROUP4.values():
        tiles = [(c["N"] // 256) * -(-c["M"] // 256) for c in cs]
        s = R.group_starts(tiles)
        assert all(x % 8 == 0 for x in s)
        # every workgroup belongs to exactly one problem; those past its tiles are padding
        owner = [sum(1 for i in range(1, len(tiles)) if b >= s[i]) for b in range(s[-1])]
        for p, t in enumerate(tiles):
            lin = [b - s[p] for b in range(s[-1]) if owner[b] == p]
            assert lin == list(range(s[p + 1] - s[p])) and t <= len(lin) < t + 8
    assert R.group_starts([9, 1, 4, 1]) == [0, 16, 24, 32, 40]


def test_splitk_slices_tile_the_k_range():
    for M, N, kt, s in R.SPLITK_SHAPES:
        r = R.splitk_ranges(kt, s)
        assert r[0][0] == 0 and r[-1][1] == kt and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(hi > lo for lo, hi in r)
    assert R.splitk_ranges(4, 4) == [(0, 1), (1, 2), (2, 3), (3, 4)]  # kt_per_split == 1


@pytest.mark.parametrize("cus", [256, 304])
def test_tail_split_arithmetic(cus):
    M = R.tail_m(cus)
    main_rows, rest = R.tail_split(M, 256, cus)
    assert rest == 129 and main_rows % 256 == 0 and main_rows + rest == M
    assert (main_rows // 256) % cus == 0 and main_rows // 256 >= 512  # whole rounds, and still the 256x256 path
    assert R.tail_split(main_rows, 256, cus) is None                 # whole rounds: one kernel
    assert R.tail_split(R.K256_M, 256, 256) is None or cus != 256    # 512 tiles on 256 CUs: no tail
    # a production shape: 4,128 tiles at N = 3072 -> 16 rounds of 256 + 32 tiles (sr_gemm.hip's comment)
    if cus == 256:
        assert R.tail_split(344 * 256 - 128, 3072, 256) == (341 * 256, 344 * 256 - 128 - 341 * 256)
