"""fp64 restatement of the attention backward (csrc/sr_attn_bwd.hip, the formulas at its top) and a
model of where the bf16 sweeps round -- the oracle of tests/test_attn_bwd_ref.py (CPU) and
tests/test_attn_bwd_oracle_gpu.py.  Plain torch; nothing of the product is imported.

    c     = scale * log2(e)
    S2    = c q.k                 lse = log2 sum_j exp2(S2_j)       P = exp2(S2 - lse)
    O     = P v                   delta = rowsum(dO * O)            dS = P * (dO.v - delta)
    dQ    = scale dS K            dK = scale dS^T Q                 dV = P^T dO

Layout: the kernel's.  Every tensor is a row-major [rows, heads * head_dim] matrix, head h in
columns [h D, (h + 1) D); item b's queries are rows b * q_bstride .. + lq, its keys of segment s
rows b * ks_bstride .. + ls.  A batch stride of 0 shares the rows between the items: a shared key
row's dK / dV is the sum over the items.  Segment 1 (l1 > 0) follows segment 0 in every softmax
row.  lse is [batch, heads, lq] in the log2 domain.

exact()     the formulas, in the given dtype (fp64; fp32 for the reference-noise check).
modelled()  the same in fp64 with the sweeps' roundings inserted, one flag each (ROUNDINGS):
    o         delta is formed from the bf16-rounded O (what the forward stores)
    lse       the saved lse is fp32
    p         P enters the dV MFMA in bf16
    ds        dS enters the dK and dQ MFMAs in bf16
    prescale  the resident S operand is rounded after the scale: bf16(c k) in the dK/dV sweeps
              (sr_attn_bwd.hip: kf = (bf16)(-k c)), bf16(c q) in the dQ sweeps (qf = (bf16)(q c)) --
              so dK / dV and dQ see two different P.
  FLASH  = what a flash-attention backward rounds (O, lse, P, dS);  DESIGN = FLASH + prescale, what
  the sweeps do today.  A kernel that drops the prescale rounding moves the tests from DESIGN to
  FLASH by changing KERNEL_MODEL below.
errors()    whole-tensor rel-L2 and the row metric  max_row |got - ref| / rms_row |ref|  (a row is one
            head's D columns of one matrix row).  A row is not normalised by its own norm: a peaked
            softmax row has a near-zero true gradient, and bf16(P) alone then reads above 1.
make()      the seeded, bf16-rounded inputs of one CASES entry: flat, gain4 / gain8 (q x 4, x 8: the
            logits of trained weights, softmax rows peaked), lossscale (dO x 1024, the trainer's
            loss scale), sparse_do (dO zero but for about 5 % of the rows, as a correspondence
            loss produces).
"""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch

LOG2E = 1.4426950408889634
ROUNDINGS = ("o", "lse", "p", "ds", "prescale")
FLASH = frozenset({"o", "lse", "p", "ds"})
DESIGN = FLASH | {"prescale"}
KERNEL_MODEL = DESIGN  # the model the bf16 sweeps are held to

Grads = namedtuple("Grads", "o lse dq dk0 dv0 dk1 dv1")
OUTPUTS = ("dq", "dk0", "dv0", "dk1", "dv1")


def bf16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to bf16 (round to nearest even), in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _heads(t, row0, n, H):
    """rows row0 .. + n of a [rows, H D] matrix as [H, n, D]"""
    return t[row0:row0 + n].reshape(n, H, -1).transpose(0, 1)


def _rows(x):
    """[H, n, D] back to [n, H D]"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def _items(q, k0, v0, g, heads, batch, lq, q_bstride, l0, k0_bstride, k1, v1, l1, k1_bstride, rows):
    """per item: (b, its query row indices, q, dO, K, V as [H, n, D])"""
    for b in range(batch):
        qi = torch.arange(lq) if rows is None else torch.as_tensor(rows[b], dtype=torch.long)
        qb = q[b * q_bstride + qi].reshape(len(qi), heads, -1).transpose(0, 1)
        gb = g[b * q_bstride + qi].reshape(len(qi), heads, -1).transpose(0, 1)
        kk, vv = _heads(k0, b * k0_bstride, l0, heads), _heads(v0, b * k0_bstride, l0, heads)
        if l1 > 0:
            kk = torch.cat([kk, _heads(k1, b * k1_bstride, l1, heads)], 1)
            vv = torch.cat([vv, _heads(v1, b * k1_bstride, l1, heads)], 1)
        yield b, qi, qb, gb, kk, vv


def _alloc(q, k0, k1, heads, batch, lq, l1, dt):
    z = lambda t: torch.zeros(t.shape, dtype=dt)  # noqa: E731
    return Grads(z(q), torch.zeros(batch, heads, lq, dtype=dt), z(q), z(k0), z(k0),
                 z(k1) if l1 > 0 else None, z(k1) if l1 > 0 else None)


def _scatter(out, b, qi, q_bstride, l0, k0_bstride, l1, k1_bstride, o, lse, dq, dk, dv):
    out.o[b * q_bstride + qi] = _rows(o)
    out.lse[b][:, qi] = lse
    out.dq[b * q_bstride + qi] = _rows(dq)
    out.dk0[b * k0_bstride:b * k0_bstride + l0] += _rows(dk[:, :l0])  # += : stride 0 sums the items
    out.dv0[b * k0_bstride:b * k0_bstride + l0] += _rows(dv[:, :l0])
    if l1 > 0:
        out.dk1[b * k1_bstride:b * k1_bstride + l1] += _rows(dk[:, l0:])
        out.dv1[b * k1_bstride:b * k1_bstride + l1] += _rows(dv[:, l0:])


def exact(q, k0, v0, g, *, heads, batch, lq, q_bstride, l0, k0_bstride, k1=None, v1=None, l1=0, k1_bstride=0,
          scale=None, dtype=torch.float64, rows=None) -> Grads:
    """O, lse (log2 domain), dQ, dK0, dV0, dK1, dV1 by the formulas above, every operation in
    ``dtype``.  ``rows`` (a list of per-item query row indices): only those queries take part;
    the other rows of O / lse / dQ stay 0."""
    cast = lambda t: None if t is None else t.detach().cpu().to(dtype)  # noqa: E731
    q, k0, v0, g, k1, v1 = (cast(t) for t in (q, k0, v0, g, k1, v1))
    D = q.shape[1] // heads
    scale = D ** -0.5 if scale is None else scale
    c = scale * LOG2E
    out = _alloc(q, k0, k1, heads, batch, lq, l1, dtype)
    for b, qi, qb, gb, kk, vv in _items(q, k0, v0, g, heads, batch, lq, q_bstride, l0, k0_bstride, k1, v1, l1,
                                        k1_bstride, rows):
        s2 = (qb @ kk.transpose(1, 2)) * c
        m = s2.max(-1, keepdim=True).values
        lse = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
        p = torch.exp2(s2 - lse)
        o = p @ vv
        delta = (gb * o).sum(-1, keepdim=True)
        ds = p * (gb @ vv.transpose(1, 2) - delta)
        _scatter(out, b, qi, q_bstride, l0, k0_bstride, l1, k1_bstride, o, lse[..., 0], (ds @ kk) * scale,
                 (ds.transpose(1, 2) @ qb) * scale, p.transpose(1, 2) @ gb)
    return out


def modelled(q, k0, v0, g, *, heads, batch, lq, q_bstride, l0, k0_bstride, k1=None, v1=None, l1=0, k1_bstride=0,
             scale=None, rounding=DESIGN, rows=None) -> Grads:
    """exact() in fp64 with bf16 / fp32 roundings at the points named in ``rounding`` (a subset of
    ROUNDINGS).  O and lse are returned as the backward is given them (rounded or not)."""
    rounding = frozenset(rounding)
    assert rounding <= set(ROUNDINGS), rounding
    dt = torch.float64
    cast = lambda t: None if t is None else t.detach().cpu().to(dt)  # noqa: E731
    q, k0, v0, g, k1, v1 = (cast(t) for t in (q, k0, v0, g, k1, v1))
    D = q.shape[1] // heads
    scale = D ** -0.5 if scale is None else scale
    c = scale * LOG2E
    # the sweeps form c in fp32 and round the fp32 product: (bf16)((float)x * c)
    c32 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    scaled = lambda x: (x.float() * c32).to(torch.bfloat16).to(dt)  # noqa: E731
    out = _alloc(q, k0, k1, heads, batch, lq, l1, dt)
    for b, qi, qb, gb, kk, vv in _items(q, k0, v0, g, heads, batch, lq, q_bstride, l0, k0_bstride, k1, v1, l1,
                                        k1_bstride, rows):
        kt = kk.transpose(1, 2)
        # forward, exact: what the backward is handed
        s2 = (qb @ kt) * c
        m = s2.max(-1, keepdim=True).values
        lse = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
        o = torch.exp2(s2 - lse) @ vv
        if "lse" in rounding:
            lse = lse.float().to(dt)
        if "o" in rounding:
            o = bf16(o)
        delta = (gb * o).sum(-1, keepdim=True)
        dp = gb @ vv.transpose(1, 2) - delta
        if "prescale" in rounding:
            p_kv = torch.exp2(qb @ scaled(kk).transpose(1, 2) - lse)  # dK/dV sweeps: K resident
            p_q = torch.exp2(scaled(qb) @ kt - lse)  # dQ sweeps: Q resident
        else:
            p_kv = p_q = torch.exp2(s2 - lse)
        ds_kv, ds_q = p_kv * dp, p_q * dp
        if "ds" in rounding:
            ds_kv, ds_q = bf16(ds_kv), bf16(ds_q)
        if "p" in rounding:
            p_kv = bf16(p_kv)
        _scatter(out, b, qi, q_bstride, l0, k0_bstride, l1, k1_bstride, o, lse[..., 0], (ds_q @ kk) * scale,
                 (ds_kv.transpose(1, 2) @ qb) * scale, p_kv.transpose(1, 2) @ gb)
    return out


def errors(got, ref, head_dim=64):
    """(whole-tensor rel-L2, max_row |got - ref| / rms_row |ref|) of two [rows, H D] matrices; a row
    is one head's head_dim columns of one matrix row."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = (got - ref).reshape(-1, head_dim).norm(dim=1)
    r = ref.reshape(-1, head_dim).norm(dim=1)
    whole = float(d.norm() / r.norm().clamp_min(1e-300))
    row = float(d.max() / r.pow(2).mean().sqrt().clamp_min(1e-300))
    return whole, row


# ------------------------------------------------------------------------------------------------
# cases: the smallest shapes that reach each sweep and tile edge (tiles are 64 rows; the generated
# sweeps need 4 full tiles = 256 rows; 128 or 256 rows per workgroup)
#   B items, P query rows each; A shared rows of segment 0 (0: segment 0 is the item's own rows);
#   seg1: the item's own rows as segment 1; layout "slab" (H = 16, q|k|v one [rows, 3C] matrix, as the
#   trainer calls it) or "plain" (H = 2, every tensor its own matrix)
Case = namedtuple("Case", "B P A seg1 layout zero_strides")
CASES = {
    "frame": Case(2, 337, 0, False, "slab", False),  # 5 full tiles + 17 ragged rows
    "frame-small": Case(2, 200, 0, False, "plain", False),  # < 256 rows: the compiled sweeps
    "global": Case(1, 1100, 0, False, "slab", True),  # 17 tiles + 12 ragged; strides 0 as the trainer passes
    "reloc": Case(3, 300, 301, True, "slab", False),  # shared segment 0 (concatenated items) + per-item segment 1
    "reloc-small": Case(3, 150, 97, True, "plain", False),
    "anchor": Case(3, 150, 700, False, "plain", False),  # shared keys only
}
KINDS = ("flat", "gain4", "gain8", "lossscale", "sparse_do")
GAIN = {"flat": 1.0, "gain4": 4.0, "gain8": 8.0, "lossscale": 1.0, "sparse_do": 1.0}


def heads_of(case: str) -> int:
    return 16 if CASES[case].layout == "slab" else 2


def geometry(case: str) -> dict:
    """the kernel's batch / segment arguments of a case"""
    cs = CASES[case]
    st = 0 if cs.zero_strides else cs.P
    kw = dict(heads=heads_of(case), batch=cs.B, lq=cs.P, q_bstride=st)
    if cs.A:
        kw.update(l0=cs.A, k0_bstride=0)
        if cs.seg1:
            kw.update(l1=cs.P, k1_bstride=cs.P)
    else:
        kw.update(l0=cs.P, k0_bstride=st)
    return kw


def make(case: str, kind: str, seed: int = 0, head_dim: int = 64, round_bf16: bool = True) -> dict:
    """q, k0, v0, k1, v1 (None without segment 1), g = dO as fp32 CPU matrices of bf16-rounded values
    (``round_bf16=False``: full fp32 mantissas, for the fp32 kernel), and the zero-dO mask of sparse_do
    as ``live`` (bool [B, P]; all True otherwise)."""
    cs = CASES[case]
    H = heads_of(case)
    C = H * head_dim
    gen = torch.Generator().manual_seed(1000 * seed + 17 * list(CASES).index(case) + KINDS.index(kind))
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    n = cs.B * cs.P
    q, k, v, g = rnd(n, C) * GAIN[kind], rnd(n, C), rnd(n, C), rnd(n, C)
    live = torch.ones(cs.B, cs.P, dtype=torch.bool)
    if kind == "lossscale":
        g = g * 1024.0
    if kind == "sparse_do":
        live = torch.rand(cs.B, cs.P, generator=gen) < 0.05
        live[:, 0] = True  # never an item without a live row
        g = g * live.reshape(n, 1)
    if cs.A:
        k0, v0 = rnd(cs.A, C), rnd(cs.A, C)
        k1, v1 = (k, v) if cs.seg1 else (None, None)
    else:
        k0, v0, k1, v1 = k, v, None, None
    t = dict(q=q, k0=k0, v0=v0, k1=k1, v1=v1, g=g)
    if round_bf16:
        t = {n_: None if x is None else bf16(x) for n_, x in t.items()}
    t["live"] = live
    return t


@functools.lru_cache(maxsize=None)
def reference(case: str, kind: str) -> dict:
    """inputs and the fp64 results of one bf16 case, computed once per process: ``exact``, ``design``,
    ``flash`` and ``model`` (the KERNEL_MODEL one), all Grads; sparse_do adds ``exact_live``, exact()
    over the rows with a non-zero dO only."""
    t = make(case, kind)
    kw = geometry(case)
    args = (t["q"], t["k0"], t["v0"], t["g"])
    seg1 = dict(k1=t["k1"], v1=t["v1"])
    r = dict(inputs=t, kw=kw, exact=exact(*args, **seg1, **kw),
             design=modelled(*args, **seg1, **kw, rounding=DESIGN),
             flash=modelled(*args, **seg1, **kw, rounding=FLASH))
    r["model"] = r["design"] if KERNEL_MODEL == DESIGN else r["flash"] if KERNEL_MODEL == FLASH else \
        modelled(*args, **seg1, **kw, rounding=KERNEL_MODEL)
    if kind == "sparse_do":
        rows = [torch.nonzero(t["live"][b])[:, 0] for b in range(CASES[case].B)]
        r["exact_live"] = exact(*args, **seg1, **kw, rows=rows)
    return r


def autograd64(q, k, v, g, scale):
    """torch's own fp64 gradient of softmax(scale q k^T) v for [H, n, D] operands: O, dq, dk, dv"""
    q, k, v = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v
    o.backward(g.double())
    return o.detach(), q.grad, k.grad, v.grad


def lse2(q, k, scale):
    """log2-domain LSE of [H, n, D] operands, by torch.logsumexp"""
    return torch.logsumexp(q.double() @ k.double().transpose(-1, -2) * scale, -1) / math.log(2.0)
