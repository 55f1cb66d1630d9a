"""sr_attention_bwd / sr_attention_bwd_f32 against the fp64 oracle and the bf16 rounding model of
tests/attn_bwd_ref.py (whose caps tests/test_attn_bwd_ref.py checks on the CPU), in the layouts the
trainer uses and at logits like trained weights'.

Cases (attn_bwd_ref.CASES; tiles are 64 rows, the generated sweeps take >= 256 rows):
    frame        B=2 P=337                 5 full tiles + 17 ragged rows
    frame-small  B=2 P=200                 below 256 rows: the compiled sweeps
    global       batch=1 P=1100            17 tiles + 12 ragged; q_bstride = k0_bstride = 0 as the trainer passes
    reloc        B=3 P=300 A=301           shared segment 0 (concatenated-items sweep) + per-item segment 1
    reloc-small  B=3 P=150 A=97            the same below 256 rows per item (450 concatenated rows: segment 0
                                           still takes the concatenated-items sweep unless SR_ATTN_BWD_PIPE=0)
    anchor       B=3 P=150, 700 shared keys only
Routing (ROUTES): the library's default switches; the compiled sweeps; the generated sweeps forced
wherever the host conditions allow -- each case under the modes that change its kernels, with
ops.last_kernel() asserted (it names the segment-0 dK/dV kernel), so a routing drift fails here.
Layouts: "slab" (frame, global, reloc: H = 16, C = 1024, q|k|v column slices of one bf16 matrix,
dq|dk|dv of one fp32 matrix, the anchors and their gradients slices of [A, 2C] matrices, 8 guard
columns beside each) and "plain" (H = 2, every tensor its own contiguous matrix).  Every matrix
has 64 guard rows below; guards hold a sentinel, output regions start as NaN.

Leg A (the backward alone): the kernel is given the oracle's O (bf16) and lse (fp32).  Its error
against exact() may be at most 1.5 x (whole tensor) and 2 x (row metric) the error of the model the
sweeps are held to (attn_bwd_ref.KERNEL_MODEL, today DESIGN) on the same inputs: both round at the
same points and differ only in the direction of individual roundings (fp32 against fp64 arithmetic
before them); the row metric is a maximum, an extreme value, hence the wider margin.  flat, gain4,
gain8, lossscale.  Measured: kernel / DESIGN = 1.000 - 1.001 in every line (DESIGN.md has the table).
Leg B (as the trainer pairs them): O and lse from ops.attention; whole-tensor error against exact()
below the suite's 2e-2 for flat, gain4, lossscale.  gain8 is printed only: the DESIGN model alone
reaches 1.8e-2 there (measured with the forward's lse: dQ 0.9 - 1.1e-2, dK / dV 2.1 - 2.3e-2).
Exact checks in both legs: outputs finite, every guard bit-identical to its sentinel, two runs
bit-identical.  sparse_do: a query row with dO = 0 has dQ == 0, and dK / dV match the oracle over
the live rows alone within leg A's bound.
fp32 leg: sr_attention_bwd_f32 (plain layout, head_dim 64 and 128) at its 2e-5.

Every comparison prints  case routing input output kernel DESIGN FLASH  (DESIGN.md quotes them).
"""

import functools

import pytest
import torch

import attn_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2  # the suite's bf16 attention-backward bound (tests/test_attn_bwd_gpu.py)
TOL_F32 = 2e-5
WHOLE_MARGIN, ROW_MARGIN = 1.5, 2.0
GUARD_ROWS, GUARD_COLS = 64, 8
SENTINEL = {torch.bfloat16: -30000.0, torch.float32: -12345.0}

ROUTES = {
    "default": {},
    "compiled": dict(SR_ATTN_BWD_PIPE=0, SR_ATTN_BWD_DQ_PIPE=0),
    "asm": dict(SR_ATTN_BWD_PIPE=1, SR_ATTN_BWD_DQ_PIPE=2, SR_ATTN_BWD_CAT=1),
}
COMPILED, PIPE, CAT = "attn_bwd_dkdv_kernel<0>", "attn_bwd_dkdv_pipe_kernel<0>", "attn_bwd_dkdv_pipe_kernel<0, cat>"
# (case, route) -> the segment-0 dK/dV kernel.  Left out: routes under which a case runs the kernels
# of its default route (frame-small: every sweep compiled anyway; reloc-small, anchor: segment 0 is
# already the concatenated-items sweep and no key segment has the dQ sweep's 256 rows / the default
# already takes it).
ROUTING = {
    ("frame", "default"): PIPE, ("frame", "compiled"): COMPILED, ("frame", "asm"): PIPE,
    ("frame-small", "default"): COMPILED,
    ("global", "default"): PIPE, ("global", "compiled"): COMPILED, ("global", "asm"): PIPE,
    ("reloc", "default"): CAT, ("reloc", "compiled"): COMPILED, ("reloc", "asm"): CAT,
    ("reloc-small", "default"): CAT, ("reloc-small", "compiled"): COMPILED,
    ("anchor", "default"): CAT, ("anchor", "compiled"): COMPILED,
}
RUNS = [pytest.param(c, r, id=f"{c}-{r}") for c, r in ROUTING]


class Guarded:
    """a [rows + 64, cols (+ 8)] device matrix: the region the kernel may touch and its guards"""

    def __init__(self, rows, cols, dtype, guard_cols):
        self.rows, self.cols = rows, cols
        self.full = torch.full((rows + GUARD_ROWS, cols + (GUARD_COLS if guard_cols else 0)), SENTINEL[dtype],
                               dtype=dtype, device=DEV)
        self.region = self.full[:rows, :cols]

    def guards_intact(self):
        want = torch.full_like(self.full, SENTINEL[self.full.dtype])
        return torch.equal(self.full[self.rows:], want[self.rows:]) and \
            torch.equal(self.full[:, self.cols:], want[:, self.cols:])


class Flat:
    """a [n + 64] fp32 device vector with a sentinel tail (lse, delta)"""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((n + GUARD_ROWS,), SENTINEL[torch.float32], device=DEV)
        self.region = self.full[:n]

    def guards_intact(self):
        return bool((self.full[self.n:] == SENTINEL[torch.float32]).all())


def _device_problem(case, t, dtype, head_dim=64):
    """the case's operands on the device in its layout: (buffers to guard-check, kernel arguments)"""
    cs, kw = R.CASES[case], R.geometry(case)
    H = kw["heads"]
    C = H * head_dim
    slab = cs.layout == "slab"
    n = cs.B * cs.P
    bufs = {}

    def mat(name, rows, cols, dt=dtype):
        bufs[name] = Guarded(rows, cols, dt, slab)
        return bufs[name].region

    if slab:
        qkv, dqkv = mat("qkv", n, 3 * C), mat("dqkv", n, 3 * C, torch.float32)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        dq, dk, dv = dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:]
        if cs.A:
            ka, dka = mat("kv_anchor", cs.A, 2 * C), mat("dkv_anchor", cs.A, 2 * C, torch.float32)
            k0, v0, dk0, dv0 = ka[:, :C], ka[:, C:], dka[:, :C], dka[:, C:]
    else:
        q, k, v = mat("q", n, C), mat("k", n, C), mat("v", n, C)
        dq, dk, dv = (mat(s, n, C, torch.float32) for s in ("dq", "dk", "dv"))
        if cs.A:
            k0, v0 = mat("k_anchor", cs.A, C), mat("v_anchor", cs.A, C)
            dk0, dv0 = mat("dk_anchor", cs.A, C, torch.float32), mat("dv_anchor", cs.A, C, torch.float32)
    q.copy_(t["q"])
    if cs.A:
        k0.copy_(t["k0"])
        v0.copy_(t["v0"])
        if cs.seg1:
            k.copy_(t["k1"])
            v.copy_(t["v1"])
    else:
        k.copy_(t["k0"])
        v.copy_(t["v0"])
        k0, v0, dk0, dv0 = k, v, dk, dv
    o, g = mat("o", n, C), mat("dout", n, C)
    g.copy_(t["g"])
    bufs["lse"], bufs["delta"] = Flat(cs.B * H * cs.P), Flat(cs.B * H * cs.P)
    args = dict(q=q, k0=k0, v0=v0, o=o, lse=bufs["lse"].region.view(cs.B, H, cs.P), dout=g, dq=dq, dk0=dk0, dv0=dv0,
                delta=bufs["delta"].region)
    seg1 = dict(k1=k, v1=v, dk1=dk, dv1=dv) if cs.seg1 else {}
    outs = dict(dq=dq, dk0=dk0, dv0=dv0, **({"dk1": dk, "dv1": dv} if cs.seg1 else {}))
    return bufs, args, seg1, kw, outs


def _backward_twice(case, route, bufs, args, seg1, kw, outs, want_kernel):
    """runs the backward twice from NaN-filled outputs under the route's switches; asserts the
    routing, finite outputs, intact guards and run-to-run bit-identity; returns the outputs (CPU)"""
    from sailrecon_amd import ops
    runs = []
    for _ in range(2):
        for t in outs.values():
            t.fill_(float("nan"))
        with ops.tuning(**ROUTES[route]):
            ops.attention_bwd(args["q"], args["k0"], args["v0"], args["o"], args["lse"], args["dout"], args["dq"],
                              args["dk0"], args["dv0"], args["delta"], **seg1, **kw)
            assert ops.last_kernel() == want_kernel, (case, route, ops.last_kernel())
        torch.cuda.synchronize()
        runs.append({n: t.clone() for n, t in outs.items()})
    for n in outs:
        assert torch.isfinite(runs[0][n]).all(), f"{case} {route}: {n} has rows the kernel did not write"
        assert torch.equal(runs[0][n], runs[1][n]), f"{case} {route}: {n} differs between two runs"
    for name, b in bufs.items():
        assert b.guards_intact(), f"{case} {route}: the guard rows / columns of {name} were written"
    return {n: t.cpu() for n, t in runs[0].items()}


@functools.lru_cache(maxsize=None)
def _model_errors(case, kind, against="exact"):
    """(KERNEL_MODEL, DESIGN, FLASH) errors per output against the oracle, once per case and input"""
    r = R.reference(case, kind)
    return {n: tuple(R.errors(getattr(r[m], n), getattr(r[against], n)) for m in ("model", "design", "flash"))
            for n in R.OUTPUTS if getattr(r["exact"], n) is not None}


def _leg_a(case, route, kind, against="exact"):
    r = R.reference(case, kind)
    bufs, args, seg1, kw, outs = _device_problem(case, r["inputs"], torch.bfloat16)
    args["o"].copy_(r["exact"].o)  # rounds to bf16
    args["lse"].copy_(r["exact"].lse)  # rounds to fp32
    got = _backward_twice(case, route, bufs, args, seg1, kw, outs, ROUTING[case, route])
    model = _model_errors(case, kind, against)
    bad = []
    for n, x in got.items():
        (kw_, kr), ((mw, mr), (dw, dr), (fw, fr)) = R.errors(x, getattr(r[against], n)), model[n]
        print(f"ATTN_BWD A {case:12s} {route:8s} {kind:9s} {n:3s} whole: kernel {kw_:.3e} DESIGN {dw:.3e} FLASH {fw:.3e}"
              f" | row: kernel {kr:.3e} DESIGN {dr:.3e} FLASH {fr:.3e}")
        if not (kw_ <= WHOLE_MARGIN * mw and kr <= ROW_MARGIN * mr):
            bad.append((n, kw_, mw, kr, mr))
    return got, bad


@pytest.mark.parametrize("kind", ["flat", "gain4", "gain8", "lossscale"])
@pytest.mark.parametrize("case,route", RUNS)
def test_backward_alone_within_the_rounding_model(case, route, kind):
    """Leg A: kernel error <= 1.5 x KERNEL_MODEL's (whole tensor) and <= 2 x its row metric."""
    _, bad = _leg_a(case, route, kind)
    assert not bad, f"(output, kernel whole, model whole, kernel row, model row): {bad}"


@pytest.mark.parametrize("case,route", RUNS)
def test_rows_without_upstream_gradient(case, route):
    """sparse_do: dQ is exactly zero where dO is; dK / dV (and dQ) within leg A's bound of the oracle
    computed from the live rows alone."""
    got, bad = _leg_a(case, route, "sparse_do", against="exact_live")
    live = R.reference(case, "sparse_do")["inputs"]["live"].reshape(-1)
    assert int((~live).sum()) > 0
    assert float(got["dq"][~live].abs().max()) == 0.0
    assert not bad, f"(output, kernel whole, model whole, kernel row, model row): {bad}"


@pytest.mark.parametrize("kind", ["flat", "gain4", "gain8", "lossscale"])
@pytest.mark.parametrize("case,route", RUNS)
def test_backward_paired_with_the_forward_kernel(case, route, kind):
    """Leg B: O and lse from ops.attention, as the trainer runs them; 2e-2 against exact()."""
    from sailrecon_amd import ops
    r = R.reference(case, kind)
    bufs, args, seg1, kw, outs = _device_problem(case, r["inputs"], torch.bfloat16)
    args["o"].fill_(float("nan"))
    args["lse"].fill_(float("nan"))
    fwd_seg1 = {n: seg1[n] for n in ("k1", "v1")} if seg1 else {}
    ops.attention(args["q"], args["k0"], args["v0"], args["o"], head_dim=64, lse=args["lse"], **fwd_seg1, **kw)
    assert torch.isfinite(args["o"]).all() and torch.isfinite(args["lse"]).all()
    got = _backward_twice(case, route, bufs, args, seg1, kw, outs, ROUTING[case, route])
    model = _model_errors(case, kind)
    bad = []
    for n, x in got.items():
        (kw_, kr), (_, (dw, dr), (fw, fr)) = R.errors(x, getattr(r["exact"], n)), model[n]
        print(f"ATTN_BWD B {case:12s} {route:8s} {kind:9s} {n:3s} whole: kernel {kw_:.3e} DESIGN {dw:.3e} FLASH {fw:.3e}"
              f" | row: kernel {kr:.3e} DESIGN {dr:.3e} FLASH {fr:.3e}")
        if kind != "gain8" and not kw_ < TOL:
            bad.append((n, kw_))
    assert not bad, f"(output, whole-tensor error) above {TOL}: {bad}"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["flat", "gain4"])
@pytest.mark.parametrize("case", ["frame-small", "reloc-small", "anchor"])
def test_f32_backward_matches_the_oracle(case, kind, D):
    """sr_attention_bwd_f32 (full fp32 mantissas in, the oracle's O and lse rounded to fp32) at 2e-5."""
    from sailrecon_amd import ops
    t = R.make(case, kind, head_dim=D, round_bf16=False)
    geo = R.geometry(case)
    ex = R.exact(t["q"], t["k0"], t["v0"], t["g"], k1=t["k1"], v1=t["v1"], **geo)
    bufs, args, seg1, kw, outs = _device_problem(case, t, torch.float32, head_dim=D)
    args["o"].copy_(ex.o)
    args["lse"].copy_(ex.lse)
    got = _backward_twice(case, "default", bufs, args, seg1, kw, outs, f"attn_bwd_dq_f32_kernel<{D}>")
    bad = []
    for n, x in got.items():
        w, row = R.errors(x, getattr(ex, n), D)
        print(f"ATTN_BWD F32 {case:12s} {kind:5s} D={D:3d} {n:3s} whole {w:.3e} row {row:.3e}")
        if not w < TOL_F32:
            bad.append((n, w))
    assert not bad, f"(output, whole-tensor error) above {TOL_F32}: {bad}"
