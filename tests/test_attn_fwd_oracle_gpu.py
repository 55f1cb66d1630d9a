"""sr_attention / sr_attention_pair / the key-split and merge routes against the fp64 oracle and the
bf16 rounding model of tests/attn_fwd_ref.py (whose caps, constructions and sensitivity
tests/test_attn_fwd_ref.py checks on the CPU) -- over EVERY query row of O and lse, with a per-row
metric beside the pooled one, at shapes small enough for that.

Cases (attn_fwd_ref.CASES; key tiles hold 64 keys, a wave 64 query rows, the 4 x 2 workgroup 256):
    frame          B=3, lq=l0=337             ragged q-tile (256 + 64 + 17) and ragged key tile (5 x 64 + 17)
    frame-tiles    B=2, lq=l0=320             whole key tiles: the "simple" asm sweep at kind 0
    reloc          B=3, lq=l1=300, 301 shared kind 1: two segments, both ragged
    global-tiles   batch 1, lq=l0=4160        kind 2, whole tiles
    global-ragged  batch 1, lq=l0=4133        kind 2, readable tail: the _SEG sweep by default
    subsample      batch 1, lq=4133, l0=320   kind 3
    keysplit       lq=4133, l0=4160           attention_partials with 2 / 5 / 16 parts + attn_merge_n
    merge-in       lq=337, keys 200 | 137     merge_o / merge_lse: union softmax and union lse
    pair           global-tiles + pair-sub (lq=4160 against 320 keys) in one attention_pair, with and
                   without V^T tiles: bit-identical to the two solo launches
Layouts: "slab" (H = 4, q|k|v -- and the shared k|v -- column slices of one matrix, 8 guard columns) and
"plain" (H = 2, every tensor its own matrix).  Every matrix has 64 guard rows below: NaN under q;
under K and V NaN, or +-3e4 where the launch is told the tails are readable (one leaked key wrecks
a row); a sentinel under o, whose region -- like lse -- starts as NaN.
Input kinds: attn_fwd_ref.make().

Routes (ROUTES) are the library's switches, which its header documents as choosing between kernels
that compute the same function; RUNS lists, per (case, route), the kernel ops.last_kernel() must
name, the sweep_stats the launch must report and the kinds it runs.  Left out: (case, route) pairs
that run the kernel of a listed pair of the same case (cfg0-mzero-off and the *-scan / *-notail
variants beyond one kind-0 and one kind-2 case; cfg1 beyond frame, reloc and global-ragged; kinds
whose rows take the same branch as a listed kind under that route -- a compiled kernel without the
asm sweep does not tell clustered4 or mixed from gain4, nor vtiny from flat).  gain4 (LayerNorm'd
q, k x 4: bound 185) stays INSIDE the window on every wave -- its pre-pass finds scores >= 38 in
tiles 0-2 -- so the waves that leave the window and run the compiled loop beside asm waves of the
same workgroup are mixed's odd ones.
Every unsplit route passes sweep_stats, which also keeps ops.attention from key-splitting by itself.

Checks on every run, every row: (1) kernel name and sweep counts; (2) O and lse finite, every input
and guard bit-identical to what it held, two runs bit-identical; (3) error against exact() at most
1.5 x (whole tensor) and 2 x (row metric) the KERNEL_MODEL error on the same inputs -- kernel and
model round at the same points and differ in the direction of individual roundings; the row metric
is an extreme value, hence the wider margin; (4) lse: max |kernel - exact| <= 2 x max |model - exact|
+ 4 fp32 ulps of the largest |lse|; (5) flat: the suite's absolute 1e-2 as well; (6) pair / pair_vt
bit-identical to the solo launches (sfm_amd.h).  sr_attn.hip does not promise SR_ATTN_PIPE on / off
bit-identical, so those routes are held to the oracle only.
fp32 leg: attn_f32_short_kernel / attn_f32_kernel (head_dim 64, 128) with the camera, dense and
additive masks and a row that sees no key, every row within 4 x the row error of the oracle itself
evaluated in fp32 (the per-key online order differs from torch's; the metric is an extreme value).

Every comparison prints  case route kind output kernel model  (DESIGN.md quotes them).
"""

import math

import pytest
import torch

import attn_fwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-2  # the suite's bf16 attention-forward bound
WHOLE_MARGIN, ROW_MARGIN, LSE_MARGIN, LSE_ULPS = 1.5, 2.0, 2.0, 4
F32_MARGIN = 4.0
GUARD_ROWS, GUARD_COLS = 64, 8
SENTINEL = -30000.0

ROUTES = {
    "default": dict(),
    "online": dict(bound="none"),  # no bound at all: the per-tile running max
    "cfg0-compiled": dict(sw=dict(SR_ATTN_CFG=0, SR_ATTN_PIPE=0)),
    "cfg0-asm": dict(sw=dict(SR_ATTN_CFG=0, SR_ATTN_PIPE_SEG=1)),  # (PIPE_SEG matters where the tails are readable)
    "cfg0-asm-scan": dict(sw=dict(SR_ATTN_CFG=0, SR_ATTN_PIPE_SEG=1), bound="scan"),  # the launch scans max |k|
    "cfg0-notail": dict(sw=dict(SR_ATTN_CFG=0, SR_ATTN_PIPE_SEG=1), tail=False),  # NaN behind the keys
    "cfg0-mzero-off": dict(sw=dict(SR_ATTN_CFG=0, SR_ATTN_MZERO=0)),
    "cfg1": dict(sw=dict(SR_ATTN_CFG=1)),
}
KIND_ID = {"frame": 0, "frame-tiles": 0, "reloc": 1, "global-tiles": 2, "global-ragged": 2, "subsample": 3,
           "pair-sub": 3, "keysplit": 0, "merge-in": 0}
ALL = R.KINDS
FEW = ("flat", "gain4")
LOOP = ("flat", "gain2.5", "gain4", "spike", "vbig")  # the compiled loop's branches: m = 0, fixed m > 0, m from tile 0
# route -> the kernel's template arguments (waves, q-blocks per wave, asm sweep compiled in); with the case's
# kind id that is the name ops.last_kernel() must give (kernel_name), and expected_stats() the sweep counts:
# without the asm sweep (or with SR_ATTN_MZERO=0) every wave on the compiled loop, with it every wave on the
# sweep -- but mixed's odd waves.  RUNS: (case, route) -> the kinds it runs (what is left out: the docstring)
SHAPE = {"default": (2, 2, False), "online": (2, 2, False), "cfg0-compiled": (4, 2, False), "cfg0-asm": (4, 2, True),
         "cfg0-asm-scan": (4, 2, True), "cfg0-notail": (4, 2, False), "cfg0-mzero-off": (4, 2, True),
         "cfg1": (8, 1, False)}
RUNS = {
    ("frame", "default"): FEW, ("frame", "online"): FEW + ("spike",), ("frame", "cfg0-compiled"): LOOP,
    ("frame", "cfg0-asm"): ALL, ("frame", "cfg0-asm-scan"): ("flat", "gain4", "mixed", "vbig"),
    ("frame", "cfg0-notail"): ("flat", "spike"), ("frame", "cfg1"): FEW,
    ("frame-tiles", "default"): FEW, ("frame-tiles", "cfg0-compiled"): LOOP, ("frame-tiles", "cfg0-asm"): ALL,
    ("frame-tiles", "cfg0-mzero-off"): ("flat", "gain2.5"),
    ("reloc", "default"): FEW, ("reloc", "online"): FEW, ("reloc", "cfg0-compiled"): LOOP, ("reloc", "cfg0-asm"): ALL,
    ("reloc", "cfg1"): FEW,
    ("global-tiles", "default"): FEW, ("global-tiles", "cfg0-compiled"): LOOP, ("global-tiles", "cfg0-asm"): ALL,
    ("global-tiles", "cfg0-mzero-off"): ("flat", "gain2.5"),
    ("global-ragged", "default"): FEW, ("global-ragged", "online"): FEW + ("spike",),
    ("global-ragged", "cfg0-compiled"): LOOP, ("global-ragged", "cfg0-asm"): ALL,
    ("global-ragged", "cfg0-asm-scan"): ("flat", "gain4", "mixed", "vbig"),
    ("global-ragged", "cfg0-notail"): ("flat", "spike"), ("global-ragged", "cfg1"): FEW,
    ("subsample", "default"): FEW, ("subsample", "cfg0-compiled"): ("flat", "gain4", "spike"),
    ("subsample", "cfg0-asm"): ALL,
}
PARAMS = [pytest.param(c, r, k, id=f"{c}-{r}-{k}") for (c, r), kinds in RUNS.items() for k in kinds]


def kernel_name(case, route):
    nw, qb, st = SHAPE[route]
    return f"attn_bf16_kernel<{nw}, {qb}, {KIND_ID[case]}, {'true' if st else 'false'}>"


def expected_stats(case, route, kind, geo=None):
    """[waves on the asm sweep, waves on the compiled loop] the launch must add to sweep_stats"""
    geo = geo or R.geometry(case)
    nw, qb, st = SHAPE[route]
    per = -(-geo["lq"] // (32 * qb))  # waves with query rows per (item, head)
    waves = geo["batch"] * geo["heads"] * per
    if not st or route == "cfg0-mzero-off":
        return [0, waves]
    if kind != "mixed":
        return [waves, 0]
    odd = geo["batch"] * geo["heads"] * (per // 2)  # waves 1, 3, ...: outside the window
    return [waves - odd, odd]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Problem:
    """a case's operands on the device in its layout, every matrix with its guards, and what to
    compare afterwards"""

    def __init__(self, case, t, dtype=torch.bfloat16, head_dim=64, tail=None, n_keys=None):
        cs, geo = R.CASES[case], R.geometry(case)
        self.case, self.geo, self.dtype = case, geo, dtype
        H = geo["heads"]
        C = H * head_dim
        slab = cs.layout == "slab"
        self.tail = cs.tail if tail is None else tail
        n = cs.B * cs.lq
        self.full = {}

        def mat(name, rows, cols, blocks):
            """[rows + 64, cols (+ 8)]: ``blocks`` = (first column, width, what its 64 tail rows hold)"""
            m = torch.full((rows + GUARD_ROWS, cols + (GUARD_COLS if slab else 0)), SENTINEL, dtype=dtype, device=DEV)
            for c0, w, tail_kind in blocks:
                m[rows:, c0:c0 + w] = math.nan if tail_kind == "nan" else R.tail_rows(w, self.tail).to(DEV)
            self.full[name] = m
            return m[:rows]

        if slab:
            qkv = mat("qkv", n, 3 * C, [(0, C, "nan"), (C, 2 * C, "kv")])
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C]
            if cs.A:
                ka = mat("kv_shared", cs.A, 2 * C, [(0, 2 * C, "kv")])
                k_sh, v_sh = ka[:, :C], ka[:, C:2 * C]
        else:
            q = mat("q", n, C, [(0, C, "nan")])
            if cs.own:
                k, v = mat("k", n, C, [(0, C, "kv")]), mat("v", n, C, [(0, C, "kv")])
            if cs.A:
                k_sh, v_sh = mat("k_shared", cs.A, C, [(0, C, "kv")]), mat("v_shared", cs.A, C, [(0, C, "kv")])
        q.copy_(t["q"])
        if cs.A:
            k_sh.copy_(t["k0"])
            v_sh.copy_(t["v0"])
            self.k0, self.v0 = k_sh, v_sh
            self.k1, self.v1 = (k, v) if cs.own else (None, None)
            if cs.own:
                k.copy_(t["k1"])
                v.copy_(t["v1"])
        else:
            k.copy_(t["k0"])
            v.copy_(t["v0"])
            self.k0, self.v0, self.k1, self.v1 = k, v, None, None
        self.q = q
        self.o_full = torch.full((n + GUARD_ROWS, C + (GUARD_COLS if slab else 0)), SENTINEL, dtype=dtype, device=DEV)
        self.o = self.o_full[:n, :C]
        self.lse_full = torch.full((cs.B * H * cs.lq + GUARD_ROWS,), SENTINEL, device=DEV)
        self.lse = self.lse_full[:cs.B * H * cs.lq].view(cs.B, H, cs.lq)
        self.saved = {name: m.clone() for name, m in self.full.items()}

    def clear(self):
        self.o.fill_(math.nan)
        self.lse.fill_(math.nan)

    def check_untouched(self, what):
        for name, m in self.full.items():
            assert torch.equal(_bits(m), _bits(self.saved[name])), \
                f"{what}: {name} (an input or its guards) was written"
        n, C = self.o.shape
        assert bool((self.o_full[n:] == SENTINEL).all()) and bool((self.o_full[:, C:] == SENTINEL).all()), \
            f"{what}: the guard rows / columns of o were written"
        assert bool((self.lse_full[self.lse.numel():] == SENTINEL).all()), f"{what}: lse was written past its end"


def _launch(ops, P, t, route, stats, **extra):
    spec = ROUTES[route]
    bound = spec.get("bound", "static")
    kw = dict(P.geo)
    if P.k1 is not None:
        kw.update(k1=P.k1, v1=P.v1)
    saved = ops._ATTN_BOUND
    try:
        ops._ATTN_BOUND = bound != "none"
        with ops.tuning(**spec.get("sw", {})):
            ops.attention(P.q, P.k0, P.v0, P.o, head_dim=P.q.shape[1] // kw["heads"], lse=P.lse,
                          key_norm_max=t["key_norm_max"] if bound == "static" else 0.0,
                          query_norm_max=t["query_norm_max"] if bound == "static" else 0.0,
                          tail_readable=P.tail, sweep_stats=stats, **kw, **extra)
            return ops.last_kernel()
    finally:
        ops._ATTN_BOUND = saved


def _twice(what, P, run):
    """``run()`` twice from NaN-filled outputs: finite, inputs and guards untouched, bit-identical"""
    outs = []
    for _ in range(2):
        P.clear()
        run()
        torch.cuda.synchronize()
        outs.append((P.o.clone(), P.lse.clone()))
    assert torch.isfinite(outs[0][0]).all(), f"{what}: O has non-finite values or rows the kernel did not write"
    assert torch.isfinite(outs[0][1]).all(), f"{what}: lse has non-finite values"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{what}: two runs differ"
    P.check_untouched(what)
    return R.Out(outs[0][0].float().cpu(), outs[0][1].cpu())


def _ulp32(x):
    return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 23)


def _compare(what, kind, got, ref, model_err):
    """checks 3 - 5; prints the line DESIGN.md quotes"""
    mw, mr, ml = model_err
    kw_, kr = R.errors(got.o, ref.o)
    kl = R.lse_error(got.lse, ref.lse)
    floor = LSE_ULPS * _ulp32(float(ref.lse[torch.isfinite(ref.lse)].abs().max()))
    print(f"ATTN_FWD {what} O whole: kernel {kw_:.3e} model {mw:.3e} ({kw_ / mw:.3f}) | row: kernel {kr:.3e} model "
          f"{mr:.3e} ({kr / mr:.3f}) | lse: kernel {kl:.3e} model {ml:.3e}")
    assert kw_ <= WHOLE_MARGIN * mw, f"{what}: whole-tensor error {kw_:.3e} above {WHOLE_MARGIN} x the model's {mw:.3e}"
    assert kr <= ROW_MARGIN * mr, f"{what}: row error {kr:.3e} above {ROW_MARGIN} x the model's {mr:.3e}"
    assert kl <= LSE_MARGIN * ml + floor, \
        f"{what}: lse error {kl:.3e} above {LSE_MARGIN} x the model's {ml:.3e} + {floor:.1e}"
    if kind == "flat":
        assert kw_ < TOL


@pytest.fixture(scope="module")
def ops():
    from sailrecon_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("case,route,kind", PARAMS)
def test_forward_within_the_rounding_model(ops, case, route, kind):
    r = R.reference(case, kind)
    t = r["inputs"]
    P = Problem(case, t, tail=ROUTES[route].get("tail"))
    want = expected_stats(case, route, kind)
    if SHAPE[route][2] and route != "cfg0-mzero-off":  # the table's counts are the published formula's
        p = R.paths(t, r["kw"], bound=ROUTES[route].get("bound", "static"))
        assert [p.asm, p.compiled] == want and p.clearance > 20, (p.asm, p.compiled, p.clearance)
    what = f"{case:13s} {route:14s} {kind:10s}"
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    names = []
    got = _twice(what, P, lambda: names.append(_launch(ops, P, t, route, stats)))
    assert names == [kernel_name(case, route)] * 2, (what, names)
    assert stats.tolist() == [2 * want[0], 2 * want[1]], (what, stats.tolist(), want)
    _compare(what, kind, got, r["exact"], R.model_errors(case, kind))


def test_q_scaled_route(ops):
    """q holding bf16(c q) with q_scaled: the same bits as the plain launch (the kernel's own rounding
    of c q is the one the caller did), asm and compiled."""
    r = R.reference("frame-tiles", "gain4")
    t = r["inputs"]
    for route in ("cfg0-asm", "cfg0-compiled"):
        P = Problem("frame-tiles", t)
        st = torch.zeros(2, dtype=torch.int32, device=DEV)
        plain = _twice(f"q_scaled {route} plain", P, lambda: _launch(ops, P, t, route, st))
        P.full["q"][:P.q.shape[0]].copy_((t["q"].float() * R._c32(0.125)).to(torch.bfloat16))
        P.saved["q"] = P.full["q"].clone()
        scaled = _twice(f"q_scaled {route}", P, lambda: _launch(ops, P, t, route, st, q_scaled=True))
        assert torch.equal(plain.o, scaled.o) and torch.equal(plain.lse, scaled.lse)


# ------------------------------------------------------------------------------------------------ split routes
@pytest.mark.parametrize("kind", FEW)
@pytest.mark.parametrize("route", ["default", "cfg0-asm"])
@pytest.mark.parametrize("parts", R.KEYSPLIT_PARTS)
def test_key_split(ops, parts, route, kind):
    """attention_partials + attn_merge_n: 2080 keys per chunk puts every chunk's ragged tail on the
    next chunk's real keys, 832 are whole tiles, 260 short chunks; O and the merged lse."""
    r = R.reference("keysplit", kind, parts)
    t, geo = r["inputs"], r["kw"]
    P = Problem("keysplit", t)
    H, lq, C = geo["heads"], geo["lq"], P.q.shape[1]
    o_parts = torch.full((parts * lq + GUARD_ROWS, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse_parts = torch.full((parts * H * lq + GUARD_ROWS,), SENTINEL, device=DEV)
    # auto dispatch: 17 q-tiles x 2 heads x 16 parts = 544 >= 512 workgroups picks the 4 x 2 shape
    asm = route == "cfg0-asm" or parts == 16
    want_kernel = f"attn_bf16_kernel<{4 if asm else 2}, 2, 0, {'true' if asm else 'false'}>"
    cgeo = dict(heads=H, batch=parts, lq=lq, q_bstride=0, l0=geo["l0"] // parts, k0_bstride=geo["l0"] // parts)
    if asm:  # every chunk's waves stay on the sweep (the published formula, per chunk)
        p = R.paths(t, cgeo)
        assert p.compiled == 0 and p.clearance > 20
    names = []

    def run():
        o_parts[:parts * lq].fill_(math.nan)
        lse_parts[:parts * H * lq].fill_(math.nan)
        with ops.tuning(**ROUTES[route].get("sw", {})):
            ops.attention_partials(P.q, P.k0, P.v0, o_parts, lse_parts[:parts * H * lq].view(parts, H, lq), heads=H,
                                   head_dim=64, lq=lq, l0=geo["l0"], parts=parts, key_norm_max=t["key_norm_max"],
                                   tail_readable=True)
            names.append(ops.last_kernel())
        ops.attn_merge_n(o_parts, lse_parts[:parts * H * lq], P.o, parts=parts, rows=lq, heads=H, head_dim=64,
                         lse_out=P.lse.view(H, lq))
    what = f"keysplit-{parts:<4d} {route:14s} {kind:10s}"
    got = _twice(what, P, run)
    assert names == [want_kernel] * 2, (what, names)
    assert torch.isfinite(o_parts[:parts * lq]).all() and torch.isfinite(lse_parts[:parts * H * lq]).all()
    assert bool((o_parts[parts * lq:] == SENTINEL).all()) and bool((lse_parts[parts * H * lq:] == SENTINEL).all())
    _compare(what, kind, got, r["exact"], R.model_errors("keysplit", kind, parts))


@pytest.mark.parametrize("kind", FEW)
@pytest.mark.parametrize("route", ["default", "cfg0-compiled"])
def test_merge_in(ops, route, kind):
    """keys 0-199 in one launch, keys 200-336 in a second one that folds the first in (merge_o /
    merge_lse): the union's softmax and lse."""
    r = R.reference("merge-in", kind)
    t, geo = r["inputs"], r["kw"]
    P = Problem("merge-in", t, tail=False)
    H, lq, C, S = geo["heads"], geo["lq"], P.q.shape[1], R.MERGE_SPLIT
    o_a = torch.full((lq + GUARD_ROWS, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
    lse_a = torch.full((H * lq + GUARD_ROWS,), SENTINEL, device=DEV)
    kw = dict(heads=H, head_dim=64, batch=1, lq=lq, q_bstride=0, k0_bstride=0, key_norm_max=t["key_norm_max"])
    names = []

    def run():
        o_a[:lq].fill_(math.nan)
        lse_a[:H * lq].fill_(math.nan)
        with ops.tuning(**ROUTES[route].get("sw", {})):
            for keys, o, lse, merge in ((slice(0, S), o_a[:lq], lse_a[:H * lq].view(1, H, lq), {}),
                                        (slice(S, geo["l0"]), P.o, P.lse,
                                         dict(merge_o=o_a[:lq], merge_lse=lse_a[:H * lq].view(H, lq)))):
                st = torch.zeros(2, dtype=torch.int32, device=DEV)
                ops.attention(P.q, P.k0[keys], P.v0[keys], o, l0=keys.stop - keys.start, lse=lse, sweep_stats=st,
                              **kw, **merge)
                names.append(ops.last_kernel())
    what = f"merge-in      {route:14s} {kind:10s}"
    got = _twice(what, P, run)
    assert names == [kernel_name("merge-in", route)] * 4, (what, names)
    assert bool((o_a[lq:] == SENTINEL).all()) and bool((lse_a[H * lq:] == SENTINEL).all())
    _compare(what, kind, got, r["exact"], R.model_errors("merge-in", kind))


@pytest.mark.parametrize("kind", ["flat", "gain4", "mixed"])
def test_pair_is_the_two_solo_launches(ops, kind):
    """global-tiles and pair-sub in one attention_pair, with and without V^T tiles: the kernel names,
    the sweep counts, bit-identical to the two launches apart, and each within the oracle's bounds."""
    refs = [R.reference(c, kind) for c in ("global-tiles", "pair-sub")]
    Ps = [Problem(c, r["inputs"]) for c, r in zip(("global-tiles", "pair-sub"), refs)]
    H = refs[0]["kw"]["heads"]
    solo = []
    for c, r, P in zip(("global-tiles", "pair-sub"), refs, Ps):
        st = torch.zeros(2, dtype=torch.int32, device=DEV)
        names = []
        solo.append(_twice(f"{c} solo", P, lambda: names.append(_launch(ops, P, r["inputs"], "cfg0-asm", st))))
        assert names == [kernel_name(c, "cfg0-asm")] * 2
    want = [sum(x) for x in zip(*(expected_stats(c, "cfg0-asm", kind) for c in ("global-tiles", "pair-sub")))]
    vts = [torch.empty(ops.vt_tile_shape(r["kw"]["l0"], H), dtype=torch.bfloat16, device=DEV) for r in refs]
    for P, r, vt in zip(Ps, refs, vts):
        ops.vt_tiles(P.v0, r["kw"]["l0"], H, vt)
    for use_vt in (False, True):
        st = torch.zeros(2, dtype=torch.int32, device=DEV)
        for P in Ps:
            P.clear()
        probs = [dict(q=P.q, k0=P.k0, v0=P.v0, o=P.o, lq=r["kw"]["lq"], l0=r["kw"]["l0"], lse=P.lse.view(-1),
                      key_norm_max=r["inputs"]["key_norm_max"], sweep_stats=st, **({"vt": vt} if use_vt else {}))
                 for P, r, vt in zip(Ps, refs, vts)]
        ops.attention_pair(*probs, heads=H, head_dim=64)
        torch.cuda.synchronize()
        assert ops.last_kernel() == f"attn_bf16_pair_kernel<2, {'true' if use_vt else 'false'}>"
        assert st.tolist() == want, (st.tolist(), want)
        for c, P, r, s in zip(("global-tiles", "pair-sub"), Ps, refs, solo):
            what = f"{c:13s} {'pair_vt' if use_vt else 'pair':14s} {kind:10s}"
            P.check_untouched(what)
            got = R.Out(P.o.float().cpu(), P.lse.cpu())
            assert torch.equal(got.o, s.o) and torch.equal(got.lse, s.lse), f"{what}: differs from the solo launch"
            _compare(what, kind, got, r["exact"], R.model_errors(c, kind))


# ------------------------------------------------------------------------------------------------ fp32 leg
F32_RUNS = [  # case, head_dim, mask, SR_ATTN_NO_SHORT, kernel
    ("frame", 64, "none", 0, "attn_f32_short_kernel<64>"), ("frame", 128, "camera", 0, "attn_f32_short_kernel<128>"),
    ("frame", 64, "dense", 0, "attn_f32_short_kernel<64>"), ("frame", 128, "add", 0, "attn_f32_short_kernel<128>"),
    ("frame", 64, "camera", 1, "attn_f32_kernel<64>"), ("frame", 128, "dense", 1, "attn_f32_kernel<128>"),
    ("reloc", 64, "none", 0, "attn_f32_kernel<64>"), ("reloc", 128, "dense", 0, "attn_f32_kernel<128>"),
    ("reloc", 64, "add", 0, "attn_f32_kernel<64>"),
    ("long600", 64, "camera", 0, "attn_f32_kernel<64>"), ("long600", 128, "add", 0, "attn_f32_kernel<128>"),
    ("long600", 64, "dense", 0, "attn_f32_kernel<64>"),
    ("cam-short", 64, "camera0", 0, "attn_f32_short_kernel<64>"),
    ("cam-short", 128, "camera0", 1, "attn_f32_kernel<128>"),
]


@pytest.mark.parametrize("case,D,mask_mode,no_short,kernel", F32_RUNS,
                         ids=[f"{c}-{d}-{m}-{'long' if n else 'auto'}" for c, d, m, n, _ in F32_RUNS])
def test_f32_forward_every_row(ops, case, D, mask_mode, no_short, kernel):
    """The fp32 kernels (full fp32 mantissas in) with each mask and a row that sees no key (zeros,
    lse -inf); every row within 4 x the row error of the oracle evaluated in fp32.  camera0: camera
    mask without anchors on 80 queries against 70 keys -- rows 70-79 see nothing, every other row
    sees exactly its own key and must return that value bit for bit."""
    from sailrecon_amd import _lib
    t, geo = R.make(case, "gain2.5", head_dim=D, round_bf16=False), R.geometry(case)
    P = Problem(case, t, dtype=torch.float32, head_dim=D, tail=False)
    B_, H, lq, L = geo["batch"], geo["heads"], geo["lq"], geo["l0"] + geo.get("l1", 0)
    gen = torch.Generator().manual_seed(D + len(case))
    mask, n_anchor = None, 0
    if mask_mode in ("dense", "add"):
        see = torch.rand(B_, H, lq, L, generator=gen) < 0.7
        see[:, :, 7] = False  # a row that sees no key
        mask = see if mask_mode == "dense" else torch.where(see, torch.randn(B_, H, lq, L, generator=gen), -math.inf)
    elif mask_mode == "camera":
        n_anchor = 5
    mode = "camera" if mask_mode == "camera0" else mask_mode
    okw = dict(k1=t["k1"], v1=t["v1"], mask_mode=mode, mask=mask, n_anchor=n_anchor, **geo)
    ex = R.exact(t["q"], t["k0"], t["v0"], **okw)
    ex32 = R.exact(t["q"], t["k0"], t["v0"], dtype=torch.float32, **okw)
    code = dict(none=_lib.SR_MASK_NONE, camera=_lib.SR_MASK_CAMERA, dense=_lib.SR_MASK_DENSE, add=_lib.SR_MASK_ADD)[mode]
    kw = dict(geo)
    if P.k1 is not None:
        kw.update(k1=P.k1, v1=P.v1)
    dmask = None if mask is None else mask.to(DEV)
    names = []

    def run():
        with ops.tuning(SR_ATTN_NO_SHORT=no_short):
            ops.attention(P.q, P.k0, P.v0, P.o, head_dim=D, lse=P.lse, mask_mode=code, n_anchor=n_anchor, mask=dmask,
                          **kw)
            names.append(ops.last_kernel())
    what = f"F32 {case:10s} D={D:3d} {mask_mode:7s}"
    outs = []
    for _ in range(2):
        P.clear()
        run()
        torch.cuda.synchronize()
        outs.append((P.o.clone().cpu(), P.lse.clone().cpu()))
    assert names == [kernel] * 2, (what, names)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    P.check_untouched(what)
    o, lse = outs[0]
    dead = ex.lse == -math.inf
    assert torch.isfinite(o).all() and not torch.isnan(lse).any()
    assert bool((lse[dead] == -math.inf).all()) and bool(torch.isfinite(lse[~dead]).all())
    if mask_mode != "none" and not (mask_mode == "camera" and n_anchor):
        assert int(dead.sum()) > 0
    (kw_, kr), (mw, mr) = R.errors(o, ex.o, D), R.errors(ex32.o, ex.o, D)
    kl, ml = R.lse_error(lse, ex.lse), R.lse_error(ex32.lse, ex.lse)
    print(f"ATTN_FWD {what} O whole: kernel {kw_:.3e} fp32-oracle {mw:.3e} | row: kernel {kr:.3e} fp32-oracle "
          f"{mr:.3e} ({kr / max(mr, 1e-300):.2f}) | lse: kernel {kl:.3e} fp32-oracle {ml:.3e}")
    if mask_mode == "camera0":
        assert torch.equal(o.reshape(B_, lq, -1)[:, :geo["l0"]], t["v0"][None].expand(B_, -1, -1))
        assert kr == 0.0
    else:
        assert kr <= F32_MARGIN * mr, f"{what}: row error {kr:.3e} above {F32_MARGIN} x the fp32 oracle's {mr:.3e}"
        assert kl <= F32_MARGIN * ml + LSE_ULPS * _ulp32(float(ex.lse[~dead].abs().max()))
