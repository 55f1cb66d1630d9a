"""The GEMM family (csrc/sr_gemm.hip) against the fp64 references and per-element bounds of
tests/gemm_ref.py (whose bounds and mutants tests/test_gemm_ref.py checks on the CPU), at the
smallest shapes that reach each edge, through sailrecon_amd.ops (gemm, gemm_group, tuning).

Every case: the kernel it was written for is the one that ran (ops.last_kernel()); every element
below M x N of out / aux / colsum is overwritten (the buffers start as NaN) and inside its bound --
bf16 outputs inside the one-or-two-value interval; everything around them (rows before and after, the
columns between N and ldo, colsum rows past colsum_blocks(M)) is bit-unchanged; A, W, the saved
pre-activation, bias, gamma and the RoPE tables live inside larger NaN buffers, so a read outside
them turns an output non-finite.  Then row isolation, and torch.equal wherever the code claims
bit-equality between two launch strategies.  Every case prints "BOUND <case> <tensor> <worst ratio>
<share of two-valued intervals>".
"""

import pytest
import torch

import gemm_ref as R
from gemm_ref import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPI = {"bias": "SR_EPI_BIAS", "gelu": "SR_EPI_BIAS_GELU", "resid": "SR_EPI_BIAS_RESID", "qkv": "SR_EPI_QKV",
       "patch": "SR_EPI_PATCH", "f32": "SR_EPI_F32", "gelu_bwd": "SR_EPI_GELU_BWD"}


def _ops():
    from sailrecon_amd import ops
    return ops


def _epi(c):
    from sailrecon_amd import _lib as L
    return getattr(L, EPI[c["epi"]])


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _inside(t, pad=True):
    """A device copy of a 2-D tensor cut out of a larger NaN buffer (one row before and after, 8 columns
    to the right; the view's first element stays 16-B aligned), or a plain copy."""
    if not pad:
        return t.to(DEV)
    big = _nan((t.shape[0] + 2, t.shape[1] + 8), t.dtype)
    v = big[1:1 + t.shape[0], :t.shape[1]]
    v.copy_(t)
    return v


def _inside_rows(t):
    """A contiguous [rows, cols] table with a NaN row before and after it."""
    rows, cols = t.shape
    big = _nan(((rows + 2) * cols,), t.dtype)
    v = big[cols:(rows + 1) * cols].view(rows, cols)
    v.copy_(t)
    return v


def _inside1d(t, lead=4):
    big = _nan((t.numel() + 2 * lead,), t.dtype)
    v = big[lead:lead + t.numel()]
    v.copy_(t)
    return v


class Out:
    """An [rows, cols] output view inside a NaN buffer: a row before, a row after, ``extra`` columns
    between cols and the row stride, the first element at ``align`` bytes past a 16-B boundary."""

    def __init__(self, rows, cols, dtype, extra, align=0, init=None, rows_after=1):
        esz = 2 if dtype == BF16 else 4
        self.ld = cols + extra
        off = (self.ld + 7) // 8 * 8 + align // esz
        self.off = off
        self.base = _nan((off + (rows + rows_after) * self.ld + 8,), dtype)
        self.view = self.base.as_strided((rows, cols), (self.ld, 1), off)
        assert self.view.data_ptr() % 16 == align
        if init is not None:
            self.view.copy_(init)
        self.before = self.base.clone()
        self.mask = torch.zeros_like(self.base, dtype=torch.bool)
        self.mask.as_strided((rows, cols), (self.ld, 1), off).fill_(True)

    def outside_unchanged(self):
        it = torch.int16 if self.base.dtype == BF16 else torch.int32
        return bool(torch.equal(self.base.view(it)[~self.mask], self.before.view(it)[~self.mask]))


def _problem(c):
    """Device buffers and the ops keywords of one case."""
    inp = R.inputs(c)
    M, N, dt, epi, pad = c["M"], c["N"], c["dtype"], c["epi"], c["pad"]
    init = inp["x0"] if epi in ("resid", "patch") else None
    rows = init.shape[0] if epi == "patch" else M
    out = Out(rows, N, R.out_dtype(c), c["ldo_extra"], c["out_align"], init)
    p = dict(a=_inside(inp["a"], pad), w=_inside(inp["w"], pad), out=out.view)
    bufs = dict(out=out)
    if "bias" in inp:
        p["bias"] = _inside1d(inp["bias"])
    if epi == "resid":
        p["gamma"] = _inside1d(inp["gamma"])
    if epi == "gelu_bwd":
        p["aux"] = _inside(inp["aux_in"], True)
    elif c["aux"]:
        bufs["aux"] = Out(M, N, dt, 8)
        p["aux"] = bufs["aux"].view
    if c["colsum"]:
        cs = bufs["colsum"] = Out(R.colsum_blocks(M), N, F32, 0, rows_after=2)
        p["colsum"] = cs.base[cs.off:cs.off + (R.colsum_blocks(M) + 2) * N]  # two rows longer than colsum_blocks(M)
    if c.get("q_scale"):
        p["q_scale"], p["q_cols"] = c["q_scale"], c["q_cols"]
    if epi == "qkv":
        q = dict(embed_dim=c["embed_dim"], head_dim=64, qk_eps=c["qk_eps"], col_offset=c["col_offset"],
                 rope_cos=_inside_rows(inp["rope_cos"]), rope_sin=_inside_rows(inp["rope_sin"]),
                 tokens_per_frame=c["tokens_per_frame"], patch_start=c["patch_start"], grid_w=c["grid_w"],
                 pos_row_base=c["pos_row_base"])
        for k in ("qn_w", "qn_b", "kn_w", "kn_b"):
            q[k] = _inside1d(inp[k])
        for k in ("pos_yx", "pos_rowmap"):
            if k in inp:
                q[k] = inp[k].to(DEV).contiguous()
        p["qkv"] = q
    if epi == "patch":
        p["patch"] = dict(seg_rows=c["seg_rows"], seg_stride=c["seg_stride"], seg_offset=c["seg_offset"],
                          row_add=inp["row_add"].to(DEV))
    return p, bufs


def _expected_kernel(c, ops):
    tn = "__bf16" if c["dtype"] == BF16 else "float"
    e = _epi(c)
    rlds = "true" if (c["epi"] == "resid" and c["out_align"] == 0 and ops.get_tuning("SR_GEMM_RESID_LDS")) else "false"
    if c["kernel"] == "group":
        return f"gemm256_group_kernel<{e}, {rlds}>"
    if c["kernel"] == "k256":
        return f"gemm256_kernel<{e}, {rlds}>"
    if c["tile_m"] == 64:
        return f"gemm_kernel<{tn}, {e}, false, 64, 256>"
    return f"gemm_kernel<{tn}, {e}, false>"


def _launch(c, p, ops):
    if c["kernel"] == "group":
        ops.gemm_group([p], _epi(c))
    else:
        kw = {k: p[k] for k in ("bias", "gamma", "qkv", "patch", "aux", "colsum") if k in p}
        if c["epi"] == "patch":
            kw["rows"] = c["M"]
        ops.gemm(p["a"], p["w"], p["out"], _epi(c), splits=c["splits"], q_scale=p.get("q_scale", 0.0),
                 q_cols=p.get("q_cols", 0), **kw)


_WORST = {}  # (kernel, epilogue, operand dtype, tensor) -> [worst ratio, largest two-valued share, cases]


def _note(c, name, ratio, share):
    w = _WORST.setdefault((c["kernel"], c["epi"], "bf16" if c["dtype"] == BF16 else "f32", name), [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], ratio), max(w[1], share), w[2] + 1


def _verify(c, bufs, label=None):
    """Holds every written tensor of a finished case to its bound and its surroundings to bit-equality;
    returns the outputs on the CPU."""
    label = label or c["name"]
    got = {}
    for name, (ref, delta) in R.reference(c).items():
        g = bufs[name].view.cpu()
        ok, ratio, share = R.check(g, ref, delta)
        print(f"BOUND {label} {name} {ratio:.4f} {share:.4f}")
        assert ok, (label, name, ratio)
        _note(c, name, ratio, share)
        assert bufs[name].outside_unchanged(), (label, name, "wrote outside M x N")
        got[name] = g
    if c["colsum"]:
        g = bufs["colsum"].view.cpu()
        ref, bound = R.colsum_ref(got["out"])
        ok, ratio, _ = R.check(g, ref, bound)
        print(f"BOUND {label} colsum {ratio:.4f} 0.0000")
        assert ok, (label, "colsum", ratio)
        _note(c, "colsum", ratio, 0.0)
        assert bufs["colsum"].outside_unchanged(), (label, "colsum rows past colsum_blocks(M) written")
        got["colsum"] = g
    return got


_RESULT = {}


def _run(c):
    """One case through its kernel, verified; the outputs are kept for the bit-equality tests."""
    if c["name"] in _RESULT:
        return _RESULT[c["name"]]
    ops = _ops()
    p, bufs = _problem(c)
    with ops.tuning(**c["tune"]):
        want = _expected_kernel(c, ops)
        _launch(c, p, ops)
        ran = ops.last_kernel()
    torch.cuda.synchronize()
    assert ran == want, (c["name"], ran, want)
    _RESULT[c["name"]] = _verify(c, bufs)
    return _RESULT[c["name"]]


def _ids(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------- every case to its bound
@pytest.mark.parametrize("case", R.CASES_K128, ids=_ids(R.CASES_K128))
def test_gemm128(case):
    _run(case)


@pytest.mark.parametrize("case", R.CASES_K64 + R.CASES_K64_OFF, ids=_ids(R.CASES_K64 + R.CASES_K64_OFF))
def test_gemm_few_rows(case):
    _run(case)


@pytest.mark.parametrize("case", R.CASES_SPLITK, ids=_ids(R.CASES_SPLITK))
def test_gemm_splitk(case):
    assert len(R.splitk_ranges(case["K"] // case["kt"], case["splits"])) == case["splits"]
    _run(case)


@pytest.mark.parametrize("case", R.CASES_GROUP, ids=_ids(R.CASES_GROUP))
def test_gemm256_tile_body(case):
    _run(case)


@pytest.mark.parametrize("case", R.CASES_GROUP_SWITCH, ids=_ids(R.CASES_GROUP_SWITCH))
def test_gemm256_tile_body_switches(case):
    _run(case)


@pytest.mark.parametrize("epi", list(R.GROUP4))
def test_gemm_group_four_problems(epi):
    """Four problems of different M, N, K in one launch (one with 9 tiles and 7 padding workgroups, one
    with M = 1), each to its bound, and bit-equal to the same problem launched as a group of one."""
    ops = _ops()
    cases = R.GROUP4[epi]
    tiles = [(c["N"] // 256) * -(-c["M"] // 256) for c in cases]
    assert tiles[0] == 9 and R.group_starts(tiles)[1] == 16 and cases[1]["M"] == 1
    built = [_problem(c) for c in cases]
    ops.gemm_group([p for p, _ in built], _epi(cases[0]))
    ran = ops.last_kernel()
    torch.cuda.synchronize()
    assert ran == _expected_kernel(cases[0], ops)
    for c, (_, bufs) in zip(cases, built):
        got = _verify(c, bufs, c["name"] + "-of4")
        alone = _run(c)
        for k in got:
            assert torch.equal(got[k], alone[k]), (c["name"], k)


# ---------------------------------------------------------------- gemm256_kernel itself, through sr_gemm
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("epi", [e for e, _ in R.K256_EPIS])
def test_gemm256_kernel(epi):
    """N = 256, K = one k-tile, M = 511 * 256 + 1: 512 tiles, the dispatch threshold; the last row tile
    holds one row."""
    (c,) = R.k256_cases(R.K256_M, epis=[epi])
    assert (c["N"] // 256) * -(-c["M"] // 256) == 512
    _run(c)
    _RESULT.pop(c["name"])  # large: not needed again


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("epi", [e for e, _ in R.K256_EPIS if e != "patch"])
def test_gemm256_tail_split(epi, tail):
    """The tail split (whole rounds of 256x256 tiles, the remaining 129 rows as 128x128 tiles) and the one
    kernel, each held to the oracle on its own: the two are close, not equal."""
    M = R.tail_m(_cus())
    split = R.tail_split(M, 256, _cus())
    assert split is not None and split[1] == 129
    (c,) = R.k256_cases(M, tag="tail", tune=dict(SR_GEMM_TAIL=tail), epis=[epi])
    _run(c)
    _RESULT.pop(c["name"])  # large: not needed again


# ---------------------------------------------------------------- row isolation
@pytest.mark.parametrize("kernel,dtype,M,N,kt,r", [("k128", BF16, 129, 132, 2, 127), ("k128", F32, 129, 132, 2, 128),
                                                    ("k64", BF16, 33, 260, 3, 32), ("k64", F32, 64, 256, 2, 0),
                                                    ("group", BF16, 257, 256, 2, 255), ("group", BF16, 257, 512, 1, 256)])
def test_nan_in_a_row_stays_in_that_row(kernel, dtype, M, N, kt, r):
    """A NaN at A[r, k] makes exactly row r of the output non-finite, and exactly row r's 64-row colsum
    block; nothing else."""
    ops = _ops()
    c = R.C(kernel, "gelu_bwd", dtype, M, N, kt, colsum=True, tag="iso")
    p, bufs = _problem(c)
    p["a"][r, c["K"] - 3] = float("nan")
    _launch(c, p, ops)
    torch.cuda.synchronize()
    assert ops.last_kernel() == _expected_kernel(c, ops)
    fin = torch.isfinite(bufs["out"].view.cpu())
    want = torch.ones(M, N, dtype=torch.bool)
    want[r] = False
    assert torch.equal(fin, want)
    finc = torch.isfinite(bufs["colsum"].view.cpu())
    wantc = torch.ones(R.colsum_blocks(M), N, dtype=torch.bool)
    wantc[r // 64] = False
    assert torch.equal(finc, wantc)
    assert bufs["out"].outside_unchanged() and bufs["colsum"].outside_unchanged()


# ---------------------------------------------------------------- claimed bit-equalities, at the small shapes
def _same(cases):
    outs = [_run(c) for c in cases]
    for c, o in zip(cases[1:], outs[1:]):
        assert o.keys() == outs[0].keys()
        for k in o:
            assert torch.equal(o[k], outs[0][k]), (cases[0]["name"], c["name"], k)


def _switch(name):
    groups = {}
    for c in R.CASES_GROUP_SWITCH:
        if name in c["tune"]:
            groups.setdefault(c["data"], []).append(c)
    return [g for g in groups.values() if len(g) > 1]


@pytest.mark.parametrize("switch", ["SR_GEMM_RESID_LDS", "SR_GEMM_ROPE_LDS", "SR_GEMM_REG_EPI", "SR_GEMM_GROUP_M"])
def test_switches_are_bit_exact(switch):
    """RESID_LDS against the register epilogue, ROPE_LDS on against off (rope_npos 65, the global
    fallback, included), REG_EPI on against off, every GROUP_M: the same bits."""
    sets = _switch(switch)
    assert len(sets) >= 2
    for cases in sets:
        _same(cases)


def test_worst_ratios_report():
    """The worst ratio per (kernel, epilogue, operand type, tensor) over the cases this session ran."""
    for (kernel, epi, dt, name), (ratio, share, n) in sorted(_WORST.items()):
        print(f"WORST {kernel} {epi} {dt} {name} ratio {ratio:.4f} two-valued {share:.4f} cases {n}")
        assert ratio <= 1.0
