"""fp64 restatement of the attention forward (csrc/sr_attn.hip) and a model of where the bf16 sweeps
round -- the oracle of tests/test_attn_fwd_ref.py (CPU) and tests/test_attn_fwd_oracle_gpu.py.  Plain
torch; nothing of the product is imported.  The layout helpers and bf16() are attn_bwd_ref's.

    c   = scale * log2(e)         S = c q.k (+ mask)          lse = log2 sum_j exp2(S_j)
    O   = sum_j exp2(S_j - lse) v_j          a row with no attended key: O = 0, lse = -inf

Layout: the kernel's (attn_bwd_ref's docstring): [rows, heads * head_dim] matrices, item b's queries
at rows b * q_bstride .. + lq, its keys of segment s at rows b * ks_bstride .. + ls, segment 1 after
segment 0 in every softmax row; lse [batch, heads, lq] in the log2 domain.

exact()     the formulas in the given dtype (fp64; fp32 for the fp32 kernels' reference noise), with
            q_scaled (q already holds c q) and the fp32 kernels' masks: "camera" (row i sees key j iff
            j < n_anchor or j == i), "dense" (bool, True = attend), "add" (added to scale q.k in the
            natural-log domain, -inf = masked).
modelled()  the same in fp64 with the bf16 sweep's roundings inserted, one flag each (ROUNDINGS), read
            off sr_attn.hip's attn_bf16_body:
    cq        the resident Q operand is bf16((float)q * c), c formed in fp32 (qf[b][s][j] = (bf16)(q c));
              absent when q_scaled
    p         P = bf16(exp2(S - m)) feeds the P.V MFMA AND the row-sum MFMA (lacc), so numerator and
              denominator see the same rounded P
    o         O = o / l (and the merge-in fold) is rounded to bf16 once, at the store
    lse       m + log2(l) is stored as fp32
    partials  key-split and merge_o only: the partial outputs are bf16 and their LSEs fp32 before
              the merge (merged(); sr_attn_merge_n and the epilogue's merge-in read stored tensors)
  The softmax offset m (0, bound - 64, the running tile max) is a per-row constant that cancels in
  O and lse up to WHICH bf16 neighbour each P rounds to.  The model takes floor(row max): a power of
  two scales every P exactly, so this rounds as the sweeps' m = 0 does (frame / flat: 99.98 % of the
  kernel's O elements equal the model's bit for bit).  The row max itself would make each row's
  largest P exactly 1.0 -- free of rounding error, which no fixed-offset sweep gets: that model
  reads 3 - 5 % below the kernel on diffuse softmax rows (measured).
  KERNEL_MODEL = what the sweeps do today.
errors()    whole-tensor rel-L2 and the row metric: max over (query row, head) of
            |got - ref|_2 / |ref|_2 over the head's D columns.  lse_error(): max |got - ref| in log2
            units (equal infinities agree).
paths()     the bf16 kernel's published per-wave decision (sr_attn.hip: FIX_HI = 64, FIX_LO = 110, the
            1.0001 margins, the key / value boxes, the three-tile pre-pass), evaluated in fp64: which
            waves of a 4 x 2 workgroup run the hand-scheduled sweep, each row's offset class, and how
            far every deciding row is from the edge it was compared with.
make()      seeded, bf16-rounded inputs of one CASES entry and input KIND (below); reference() caches
            inputs, exact and model per process.
"""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch

import attn_bwd_ref as B
from attn_bwd_ref import LOG2E, bf16

ROUNDINGS = ("cq", "p", "o", "lse", "partials")
KERNEL_MODEL = frozenset(ROUNDINGS)  # the model the bf16 sweeps (and the key-split merge) are held to
FIX_HI, FIX_LO, FIX_HI_MAX, KT = 64.0, 110.0, 100.0, 64

Out = namedtuple("Out", "o lse")
# a bug planted into modelled() (tests/test_attn_fwd_ref.py): rows ``rows`` of item ``item`` also see
# the key / value row ``leak`` = (k, v); or lose their last key; or form P.V from P (1 + p_bias)
Mutant = namedtuple("Mutant", "item rows leak drop_last p_bias", defaults=(0, slice(0, 0), None, False, 0.0))


def _c32(scale):
    """c as the kernel forms it: (float)scale * 1.4426950408889634f"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def _keys(k0, v0, k1, v1, b, heads, l0, k0_bstride, l1, k1_bstride):
    kk, vv = B._heads(k0, b * k0_bstride, l0, heads), B._heads(v0, b * k0_bstride, l0, heads)
    if l1 > 0:
        kk = torch.cat([kk, B._heads(k1, b * k1_bstride, l1, heads)], 1)
        vv = torch.cat([vv, B._heads(v1, b * k1_bstride, l1, heads)], 1)
    return kk, vv


def _mask_bias(mask_mode, mask, b, n_anchor, lq, L, dt):
    """[H or 1, lq, L] additive bias in the log2 domain (0 / -inf / mask * log2 e), or None"""
    if mask_mode in (None, "none"):
        return None
    if mask_mode == "camera":
        i, j = torch.arange(lq)[:, None], torch.arange(L)[None, :]
        see = (j < n_anchor) | (j == i)
        return torch.zeros(1, lq, L, dtype=dt).masked_fill(~see[None], -math.inf)
    m = mask[b]
    if mask_mode == "dense":
        return torch.zeros(m.shape, dtype=dt).masked_fill(~m.bool(), -math.inf)
    assert mask_mode == "add", mask_mode
    return m.to(dt) * LOG2E


def _softmax_pv(s2, vv, rounding=frozenset(), p_bias=None):
    """one head: s2 [n, L] (log2 domain, -inf = not attended), vv [L, D] -> o [n, D] (normalised,
    unrounded), lse [n].  ``p_bias`` [n, 1]: the mutant's factor on the P.V operand."""
    m = s2.max(-1, keepdim=True).values
    dead = m == -math.inf
    if "p" in rounding:  # an integer offset: every P rounds as under the sweeps' m = 0 (see the module docstring)
        m = m.floor()
    p = torch.exp2(s2 - m.masked_fill(dead, 0.0))
    pv = p if p_bias is None else p * p_bias
    if "p" in rounding:
        p, pv = bf16(p), bf16(pv)
    l = p.sum(-1, keepdim=True)
    o = (pv @ vv) / l.masked_fill(dead, 1.0)
    lse = (m + torch.log2(l.masked_fill(dead, 1.0))).masked_fill(dead, -math.inf)
    return o.masked_fill(dead, 0.0), lse[:, 0]


def _forward(q, k0, v0, *, heads, batch, lq, q_bstride, l0, k0_bstride, k1=None, v1=None, l1=0, k1_bstride=0,
             scale=None, q_scaled=False, mask_mode=None, mask=None, n_anchor=0, dtype=torch.float64,
             rounding=frozenset(), mutant=None) -> Out:
    cast = lambda t: None if t is None else t.detach().cpu().to(dtype)  # noqa: E731
    k0, v0, k1, v1 = (cast(t) for t in (k0, v0, k1, v1))
    D = q.shape[1] // heads
    scale = D ** -0.5 if scale is None else scale
    if q_scaled:
        cq = cast(q)
    elif "cq" in rounding:
        cq = (q.detach().cpu().float() * _c32(scale)).to(torch.bfloat16).to(dtype)
    else:
        cq = cast(q) * (scale * LOG2E)
    o = torch.zeros((batch - 1) * q_bstride + lq, q.shape[1], dtype=dtype)
    lse = torch.zeros(batch, heads, lq, dtype=dtype)
    for b in range(batch):
        qb = B._heads(cq, b * q_bstride, lq, heads)
        kk, vv = _keys(k0, v0, k1, v1, b, heads, l0, k0_bstride, l1, k1_bstride)
        bias = _mask_bias(mask_mode, mask, b, n_anchor, lq, l0 + l1, dtype)
        mut = mutant if mutant is not None and mutant.item == b else None
        ob_rows = []
        for h in range(heads):
            kh, vh = kk[h], vv[h]
            if mut is not None and mut.leak is not None:
                kh = torch.cat([kh, mut.leak[0].to(dtype).reshape(heads, 1, D)[h]], 0)
                vh = torch.cat([vh, mut.leak[1].to(dtype).reshape(heads, 1, D)[h]], 0)
            s2 = qb[h] @ kh.T
            if bias is not None:
                s2 = s2 + bias[h if bias.shape[0] > 1 else 0]
            p_bias = None
            if mut is not None:
                hit = torch.zeros(lq, dtype=torch.bool)
                hit[mut.rows] = True
                if mut.leak is not None:
                    s2[~hit, -1] = -math.inf
                if mut.drop_last:
                    s2[hit, -1] = -math.inf
                if mut.p_bias:
                    p_bias = torch.where(hit, 1.0 + mut.p_bias, 1.0).to(dtype)[:, None]
            oh, lh = _softmax_pv(s2, vh, rounding, p_bias)
            ob_rows.append(oh)
            lse[b, h] = lh
        o[b * q_bstride:b * q_bstride + lq] = B._rows(torch.stack(ob_rows))
    return Out(o, lse)


def _stored(out: Out, rounding) -> Out:
    o = bf16(out.o) if "o" in rounding else out.o
    return Out(o, out.lse.float().to(out.lse.dtype) if "lse" in rounding else out.lse)


def exact(q, k0, v0, **kw) -> Out:
    """O ([rows, heads * D], item b at rows b * q_bstride) and lse ([batch, heads, lq], log2 domain),
    every operation in ``dtype`` (default fp64)."""
    return _forward(q, k0, v0, **kw)


def modelled(q, k0, v0, *, rounding=KERNEL_MODEL, mutant=None, **kw) -> Out:
    """exact() in fp64 with the roundings named in ``rounding`` (a subset of ROUNDINGS)."""
    rounding = frozenset(rounding)
    assert rounding <= set(ROUNDINGS), rounding
    return _stored(_forward(q, k0, v0, rounding=rounding, mutant=mutant, **kw), rounding)


def merge(parts, rounding=frozenset()) -> Out:
    """softmax over the union of disjoint key sets from each set's normalised O and lse
    (sr_attn_merge's formula: out = sum_p 2^(l_p - M) o_p / sum_p 2^(l_p - M), lse = M + log2 sum):
    ``parts`` a list of Out with o [rows, C] and lse [heads, rows]; the result is rounded as stored."""
    lse = torch.stack([p.lse for p in parts])  # [P, H, rows]
    M = lse.max(0).values
    dead = M == -math.inf
    w = torch.exp2(lse - M.masked_fill(dead, 0.0))
    tot = w.sum(0)
    H, rows = M.shape
    wn = (w / tot.masked_fill(dead, 1.0)).masked_fill(dead[None], 0.0)  # [P, H, rows]
    o = sum(p.o.reshape(rows, H, -1) * wn[i].T[:, :, None] for i, p in enumerate(parts)).reshape(rows, -1)
    out = Out(o, (M + torch.log2(tot.masked_fill(dead, 1.0))).masked_fill(dead, -math.inf))
    return _stored(out, rounding)


def key_split(q, k0, v0, *, heads, lq, l0, parts, rounding=frozenset(), **kw) -> Out:
    """ops.attention_partials + attn_merge_n: ``parts`` equal key chunks, each a normalised partial
    (bf16 / fp32-lse with the "partials" flag), merged; lse [1, heads, lq]."""
    chunk = l0 // parts
    inner = frozenset(rounding) - {"o", "lse"}
    ps = []
    for s in range(parts):
        r = _forward(q, k0[s * chunk:(s + 1) * chunk], v0[s * chunk:(s + 1) * chunk], heads=heads, batch=1, lq=lq,
                     q_bstride=0, l0=chunk, k0_bstride=0, rounding=inner, **kw)
        r = Out(r.o, r.lse[0])
        ps.append(_stored(r, {"o", "lse"}) if "partials" in rounding else r)
    m = merge(ps, rounding)
    return Out(m.o, m.lse[None])


def merge_in(q, k0, v0, *, heads, lq, l0, split, rounding=frozenset(), **kw) -> Out:
    """keys [0, split) in a first launch, keys [split, l0) in a second one with merge_o / merge_lse:
    the first result is stored (bf16, fp32 lse with "partials"), the second folded in unrounded."""
    inner = frozenset(rounding) - {"o", "lse"}
    geo = dict(heads=heads, batch=1, lq=lq, q_bstride=0, k0_bstride=0, rounding=inner, **kw)
    a = _forward(q, k0[:split], v0[:split], l0=split, **geo)
    b = _forward(q, k0[split:l0], v0[split:l0], l0=l0 - split, **geo)
    a, b = Out(a.o, a.lse[0]), Out(b.o, b.lse[0])
    if "partials" in rounding:
        a = _stored(a, {"o", "lse"})
    m = merge([a, b], rounding)
    return Out(m.o, m.lse[None])


def errors(got, ref, head_dim=64):
    """(whole-tensor rel-L2, max over (row, head) of |got - ref|_2 / |ref|_2 over the head's columns).
    A (row, head) whose reference is exactly zero (no attended key) must be exactly zero: it counts
    as 0 then and as inf otherwise."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = (got - ref).reshape(-1, head_dim).norm(dim=1)
    r = ref.reshape(-1, head_dim).norm(dim=1)
    whole = float(d.norm() / r.norm().clamp_min(1e-300))
    ratio = torch.where(r > 0, d / r.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0).double())
    return whole, float(ratio.max())


def lse_error(got, ref):
    """max |got - ref| in log2 units; equal infinities agree, unequal ones give inf"""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    same = got == ref
    d = (got - ref).abs().masked_fill(same, 0.0)
    return float(torch.nan_to_num(d, nan=math.inf).max())


# ------------------------------------------------------------------------------------------------
# cases: the smallest shapes that reach each path.  Key tiles hold 64 keys, a wave 64 query rows (two
# 32-row q-blocks), the 4 x 2 workgroup 256; the hand-scheduled sweep needs >= 4 key tiles and its
# pre-pass reads tiles 0-2; kinds 2 / 3 (one long query set) need lq >= 4096.
#   B items of lq query rows; own: the item's own rows are its keys (segment 0, or segment 1 behind
#   A shared rows of segment 0); A > 0 without own: the A shared rows alone; layout "slab" (H = 4,
#   q|k|v and the shared k|v column slices of one matrix + 8 guard columns) or "plain" (H = 2)
Case = namedtuple("Case", "B lq A own layout zero_strides tail")
CASES = {
    "frame": Case(3, 337, 0, True, "slab", False, True),  # 256 + 64 + 17 query rows; 5 key tiles + 17
    "frame-tiles": Case(2, 320, 0, True, "plain", False, False),  # whole key tiles: the "simple" asm sweep
    "reloc": Case(3, 300, 301, True, "slab", False, True),  # kind 1: shared segment 0 + own segment 1, both ragged
    "global-tiles": Case(1, 4160, 0, True, "plain", True, False),  # kind 2, whole tiles
    "global-ragged": Case(1, 4133, 0, True, "slab", True, True),  # kind 2, 64 tiles + 37; _SEG by default
    "subsample": Case(1, 4133, 320, False, "plain", True, False),  # kind 3: long query set, short shared keys
    "keysplit": Case(1, 4133, 4160, False, "plain", True, True),  # attention_partials + attn_merge_n
    "merge-in": Case(1, 337, 337, False, "plain", True, False),  # keys 200 | 137 through merge_o / merge_lse
    "pair-sub": Case(1, 4160, 320, False, "plain", True, False),  # attention_pair's second problem (kind 3)
    # fp32 leg only
    "long600": Case(2, 70, 600, False, "plain", False, False),  # > 512 keys: the long fp32 kernel
    "cam-short": Case(2, 80, 70, False, "plain", False, False),  # more queries than keys: camera rows without a key
}
MERGE_SPLIT = 200
KEYSPLIT_PARTS = (2, 5, 16)  # 2080 keys per chunk (ragged tail on the next chunk's keys), 832 (whole), 260
KINDS = ("flat", "gain2.5", "gain4", "clustered4", "mixed", "spike", "vtiny", "vbig")
SPIKE_LOG2 = 40.0
MIXED_GAINS = (0.5, 4.0)  # even waves (inside the window), odd waves (outside)


def heads_of(case: str) -> int:
    return 4 if CASES[case].layout == "slab" else 2


def geometry(case: str) -> dict:
    """the kernel's batch / segment arguments of a case"""
    cs = CASES[case]
    st = 0 if cs.zero_strides else cs.lq
    kw = dict(heads=heads_of(case), batch=cs.B, lq=cs.lq, q_bstride=st)
    if cs.A:
        kw.update(l0=cs.A, k0_bstride=0)
        if cs.own:
            kw.update(l1=cs.lq, k1_bstride=cs.lq)
    else:
        kw.update(l0=cs.lq, k0_bstride=st)
    return kw


def _ln(x, H):
    """per-head LayerNorm without affine: every head's D columns to zero mean, unit variance"""
    y = x.reshape(x.shape[0], H, -1)
    return ((y - y.mean(-1, keepdim=True)) / y.std(-1, keepdim=True, unbiased=False)).reshape(x.shape)


def _max_head_norm(ts, H):
    """max 2-norm of a head's D columns over the rows of the given matrices"""
    return max(float(t.double().reshape(t.shape[0], H, -1).norm(dim=-1).max()) for t in ts if t is not None)


def _key_rows(cs, j):
    """matrix rows of key j of segment 0: the shared row, or every item's own"""
    return [j] if cs.A else [b * cs.lq + j for b in range(cs.B)]


def spike_keys(case: str):
    """indices (in the key rows the item sees first: segment 0) of spike's two keys: the first key
    after tile 2 and one in the last (ragged) tile"""
    l0 = geometry(case)["l0"]
    return 3 * KT, l0 - 3


def make(case: str, kind: str, seed: int = 0, head_dim: int = 64, round_bf16: bool = True) -> dict:
    """q, k0, v0, k1, v1 (None without segment 1) as fp32 CPU matrices of bf16-rounded values
    (``round_bf16=False``: full fp32 mantissas, for the fp32 kernels), key_norm_max (the keys' actual
    largest per-head 2-norm, a little up: the static bound) and query_norm_max (clustered4 only: the
    launch then attaches the key and value boxes).

    flat        randn q, k, v: bound ~ 12, every wave runs m = 0
    gain2.5     LayerNorm'd randn q, k times 2.5: 64 < bound < 110, m = bound - 64 > 0 without pre-pass
    gain4       LayerNorm'd randn q, k times 4: bound ~ 185, m ~ 121; the pre-pass has to find a score
                above m - 110 in tiles 0-2 (it does: the scores' sigma is ~ 23)
    clustered4  gain4 with the keys around one shared direction (0.05 spread): 2-norm bound far above
                every score; query_norm_max set, so the boxes are attached
    mixed       keys as gain4 plus ONE key of 4 x the norm behind tile 2 (it sets the bound); query
                gains alternate per 64-row wave: 0.5 (bound ~ 92: inside the window) / 4 (bound ~ 740
                against a pre-pass max ~ 64: outside, the compiled loop's running max)
    spike       flat with a shared query component u and two keys along u scoring SPIKE_LOG2 above
                the rest: spike_keys() -- one the pre-pass cannot see, one in the last ragged tile
    vtiny/vbig  flat with V x 2^-14 / x 2^40: the two sides of the value window
    """
    cs = CASES[case]
    H = heads_of(case)
    C = H * head_dim
    gen = torch.Generator().manual_seed(7919 * seed + 31 * list(CASES).index(case) + KINDS.index(kind))
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    n = cs.B * cs.lq
    q, k, v = rnd(n, C), rnd(n, C), rnd(n, C)
    ka, va = (rnd(cs.A, C), rnd(cs.A, C)) if cs.A else (None, None)
    u = rnd(1, C)
    qnm = 0.0
    if kind in ("gain2.5", "gain4", "clustered4", "mixed"):
        g = 2.5 if kind == "gain2.5" else 4.0
        if kind == "clustered4":
            k = u + 0.05 * k
            ka = None if ka is None else u + 0.05 * ka
        q, k = _ln(q, H) * g, _ln(k, H) * g
        ka = None if ka is None else _ln(ka, H) * g
        if kind == "mixed":
            wave = torch.arange(n) % cs.lq // 64
            q = q / g * torch.tensor(MIXED_GAINS)[wave % 2][:, None]
            rows = _key_rows(cs, 3 * KT + 7)  # one per item, or one shared
            (k if ka is None else ka)[rows] *= 4.0
    elif kind == "spike":
        un = _ln(u, H) / head_dim ** 0.5  # unit per head
        a = 16.0  # (large against the rows' own unit component along u, which spreads the spikes' scores)
        b = (SPIKE_LOG2 + 16.0) / (head_dim ** -0.5 * LOG2E * a)  # c a b = 56: ~ 40 above the other keys' max
        q = q + a * un
        for j in spike_keys(case):
            (k if ka is None else ka)[_key_rows(cs, j)] = b * un
    elif kind == "vtiny":
        v, va = v * 2.0 ** -14, None if va is None else va * 2.0 ** -14
    elif kind == "vbig":
        v, va = v * 2.0 ** 40, None if va is None else va * 2.0 ** 40
    if cs.A:
        k0, v0 = ka, va
        k1, v1 = (k, v) if cs.own else (None, None)
    else:
        k0, v0, k1, v1 = k, v, None, None
    t = dict(q=q, k0=k0, v0=v0, k1=k1, v1=v1)
    if round_bf16:
        t = {n_: None if x is None else bf16(x) for n_, x in t.items()}
    t["key_norm_max"] = _max_head_norm([t["k0"], t["k1"]], H) * (1.0 + 2.0 ** -10)
    if kind == "clustered4":
        qnm = _max_head_norm([t["q"]], H) * (1.0 + 2.0 ** -10)
    t["query_norm_max"] = qnm
    return t


def tail_rows(cols: int, readable: bool) -> torch.Tensor:
    """the 64 rows behind a key / value matrix: NaN, or (a caller that promises readable tails)
    large finite values of alternating sign, so that one leaked key wrecks a row visibly"""
    if not readable:
        return torch.full((KT, cols), math.nan)
    sign = 1.0 - 2.0 * ((torch.arange(KT)[:, None] + torch.arange(cols)[None, :]) % 2)
    return 3.0e4 * sign


def run_exact(case, t, **kw):
    """exact() / modelled() (``rounding=`` given) of a case's inputs through its own route:
    key_split (``parts=``), merge_in (merge-in) or one launch"""
    geo = geometry(case)
    f = modelled if "rounding" in kw or "mutant" in kw else exact
    if case == "keysplit":
        return key_split(t["q"], t["k0"], t["v0"], heads=geo["heads"], lq=geo["lq"], l0=geo["l0"], **kw)
    if case == "merge-in":
        return merge_in(t["q"], t["k0"], t["v0"], heads=geo["heads"], lq=geo["lq"], l0=geo["l0"], split=MERGE_SPLIT,
                        **kw)
    return f(t["q"], t["k0"], t["v0"], k1=t["k1"], v1=t["v1"], **geo, **kw)


@functools.lru_cache(maxsize=None)
def reference(case: str, kind: str, parts: int = 0) -> dict:
    """inputs, ``exact`` and ``model`` (KERNEL_MODEL) of one bf16 case, computed once per process and
    shared (do not write to them); ``parts``: the key split of "keysplit"."""
    t = make(case, kind)
    kw = dict(parts=parts) if case == "keysplit" else {}
    return dict(inputs=t, kw=geometry(case), exact=run_exact(case, t, **kw),
                model=run_exact(case, t, rounding=KERNEL_MODEL, **kw))


@functools.lru_cache(maxsize=None)
def model_errors(case: str, kind: str, parts: int = 0):
    """(whole, row, lse) error of KERNEL_MODEL against exact()"""
    r = reference(case, kind, parts)
    return errors(r["model"].o, r["exact"].o) + (lse_error(r["model"].lse, r["exact"].lse),)


# ------------------------------------------------------------------------------------------------
Paths = namedtuple("Paths", "asm compiled m_zero m_fixed outside clearance qb mx3")


def paths(t: dict, geo: dict, *, bound: str = "static", wave_rows: int = 64, scale=None) -> Paths:
    """sr_attn.hip's per-wave decision for the 4 x 2 workgroup's hand-scheduled sweep, in fp64.
    ``bound``: "static" (key_norm_max; with query_norm_max and c |q| |k| > 87 the key / value boxes and
    the keys' actual norm as ops._attach_key_box adds them), "scan" (the launch's own max |k|; for
    one long query set the boxes too, ops._attach_scan_boxes).
    Returns waves on the asm sweep / on the compiled loop (the sweep_stats a launch with >= 4 key
    tiles must report), rows with m = 0, rows with a fixed m > 0, rows outside the window, the
    smallest distance (log2) of a deciding row from the edge it was compared with, and per-row qb /
    mx3 [batch, heads, lq]."""
    H, batch, lq = geo["heads"], geo["batch"], geo["lq"]
    l0, l1 = geo["l0"], geo.get("l1", 0)
    D = t["q"].shape[1] // H
    scale = D ** -0.5 if scale is None else scale
    cq = (t["q"].float() * _c32(scale)).to(torch.bfloat16).double()
    long_set = (batch == 1 or geo["q_bstride"] == 0) and lq >= 4096
    knm, qnm = t["key_norm_max"], t.get("query_norm_max", 0.0)
    boxes = (bound == "static" and qnm > 0 and scale * LOG2E * qnm * knm > (FIX_HI + FIX_LO) / 2) or \
        (bound == "scan" and long_set)
    asm = compiled = m_zero = m_fixed = outside = 0
    clearance = math.inf
    qb_all, mx_all = torch.zeros(batch, H, lq, dtype=torch.float64), torch.zeros(batch, H, lq, dtype=torch.float64)
    for b in range(batch):
        qh = B._heads(cq, b * geo["q_bstride"], lq, H)
        segs = [(B._heads(t["k0"].double(), b * geo["k0_bstride"], l0, H),
                 B._heads(t["v0"].double(), b * geo["k0_bstride"], l0, H))]
        if l1:
            segs.append((B._heads(t["k1"].double(), b * geo["k1_bstride"], l1, H),
                         B._heads(t["v1"].double(), b * geo["k1_bstride"], l1, H)))
        kk, vv = torch.cat([s[0] for s in segs], 1), torch.cat([s[1] for s in segs], 1)
        # the first three key TILES: tiles never straddle the segments
        first, left = [], 3
        for ks, _ in segs:
            take = min(left, -(-ks.shape[1] // KT))
            first.append(ks[:, :take * KT])
            left -= take
        k3 = torch.cat(first, 1)
        for h in range(H):
            kact = float(kk[h].norm(dim=-1).max()) * 1.0001
            kn = kact if bound == "scan" else (min(knm, kact) if boxes else knm)
            qs = qh[h].norm(dim=-1) * kn * 1.0001
            qb = qs.clone()
            hi = FIX_HI
            if boxes:
                kmax, kmin = kk[h].max(0).values, kk[h].min(0).values
                ub = torch.maximum(qh[h] * kmax, qh[h] * kmin).sum(-1)
                ab = (qh[h].abs() * torch.maximum(kmax.abs(), kmin.abs())).sum(-1)
                qb = torch.minimum(qb, ub + 2e-4 * ab)
                vmax = float(vv[h].abs().max())
                hi = min(max(125.0 - math.ceil(math.log2(l0 + l1)) - math.ceil(math.log2(max(vmax, 1.0))), FIX_HI),
                         FIX_HI_MAX)
            mx3 = (qh[h] @ k3[h].T).max(-1).values
            m_fix = (qb - hi).clamp_min(0.0)
            need = m_fix + qs > FIX_LO
            ok = ~need | (m_fix - mx3 <= FIX_LO)
            zero = (qb <= hi) & (qs <= FIX_LO)
            # (mx3 >= -qs, so a row the pre-pass is not needed for passes its test as well: one edge)
            dist = (FIX_LO - (m_fix - mx3)).abs()
            clearance = min(clearance, float(dist.min()))
            m_zero += int(zero.sum())
            m_fixed += int((ok & ~zero).sum())
            outside += int((~ok).sum())
            w_ok = [bool(ok[r:r + wave_rows].all()) for r in range(0, lq, wave_rows)]
            asm += sum(w_ok)
            compiled += len(w_ok) - sum(w_ok)
            qb_all[b, h], mx_all[b, h] = qb, mx3
    return Paths(asm, compiled, m_zero, m_fixed, outside, clearance, qb_all, mx_all)
