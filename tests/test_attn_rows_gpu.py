"""sr_attention_rows (few query rows, key-split bf16 attention) against an fp64 softmax-attention of
the same bf16 inputs, with sr_attention (bf16) run on every case as the reference kernel.

Bounds (per case unless said otherwise; every measured figure is printed):
  * rel-L2 of o against fp64 < 1e-2 (the bound of the existing bf16 attention tests) and
    <= 1.5 x sr_attention's own error on the same case: the products and the fp32 accumulation are
    the same, only the order of the sums differs;
  * the LSE error (root mean square over the case's batch * heads * lq values, log2 domain) <= 2 x
    sr_attention's own on the same case, for every case with at least LSE_MIN_VALUES = 32 values.
    A case with fewer (down to ONE value at lq = heads = batch = 1) compares a handful of samples of
    two rounding errors, whose ratio says little, so there the bound is max(2 x sr_attention's,
    LSE_FLOOR) with LSE_FLOOR = 2^-9 log2(e) = 2.8e-3: P is rounded to bf16 before it is summed, each
    P within 2^-9 of its value, so the sum is within a factor 1 +- 2^-9 and its log2 within
    2^-9 log2(e) whatever the keys (the fp32 sums and the score's own rounding are 2^-14 of that);
  * on top, the LSE errors pooled over every value of every case of one (lq, q_scaled) sweep:
    pooled rms <= 2 x sr_attention's.
"""

import ctypes
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG2E = 1.4426950408889634
LQS = (1, 2, 31, 32, 33, 64)
L0S = (1, 63, 64, 65, 127, 1000, 4100)
L1S = (0, 21, 64)
BATCHES = (1, 3)
HEADS = (1, 6, 16)
TOKEN_ROWS = 7  # ldq = 7 token rows of the packed q|k|v buffer
LSE_MIN_VALUES = 32                  # cases with fewer LSE values get the absolute floor as well
LSE_FLOOR = 2.0 ** -9 * LOG2E        # bf16 rounding of P: the worst LSE error it allows (docstring)


def lse_bound(n_values, rms_sweep_kernel):
    return 2.0 * rms_sweep_kernel if n_values >= LSE_MIN_VALUES else max(2.0 * rms_sweep_kernel, LSE_FLOOR)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sailrecon_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_case(gen, *, lq, l0, l1, batch, heads, q_scaled, big_key=False, nan_pad=0):
    """Packed [rows, 3 * heads * 64] bf16 buffers: q rows TOKEN_ROWS token rows apart in the first
    third of theirs, K / V as the second and third column slices; segment 0 shared by the items,
    segment 1 per item.  ``nan_pad`` rows of NaN follow every key segment (instance)."""
    C = heads * 64
    qbuf = torch.randn(batch * lq * TOKEN_ROWS, 3 * C, device=DEV, generator=gen)
    if q_scaled:
        qbuf *= 0.125 * LOG2E
    qbuf = qbuf.to(torch.bfloat16)
    s0 = torch.randn(l0 + nan_pad, 3 * C, device=DEV, generator=gen)
    if big_key:
        s0[l0 - 1, C:2 * C] *= 8.0  # a key of 8x norm in the last chunk: the running max moves at the merge
    s0[l0:] = float("nan")
    s0 = s0.to(torch.bfloat16)
    stride1 = l1 + nan_pad
    s1 = None
    if l1:
        s1 = torch.randn(batch * stride1, 3 * C, device=DEV, generator=gen)
        s1.view(batch, stride1, 3 * C)[:, l1:] = float("nan")
        s1 = s1.to(torch.bfloat16)
    return dict(lq=lq, l0=l0, l1=l1, batch=batch, heads=heads, q_scaled=q_scaled, qbuf=qbuf, s0=s0, s1=s1,
                stride1=stride1, C=C)


def views(c):
    C = c["C"]
    q = c["qbuf"].view(c["batch"] * c["lq"], TOKEN_ROWS * 3 * C)[:, 0:C]
    kw = dict(heads=c["heads"], head_dim=64, batch=c["batch"], lq=c["lq"], q_bstride=c["lq"], l0=c["l0"],
              k0_bstride=0, l1=c["l1"], k1_bstride=c["stride1"] if c["l1"] else 0, q_scaled=bool(c["q_scaled"]))
    if c["l1"]:
        kw.update(k1=c["s1"][:, C:2 * C], v1=c["s1"][:, 2 * C:3 * C])
    return q, c["s0"][:, C:2 * C], c["s0"][:, 2 * C:3 * C], kw


def reference(c):
    """fp64 softmax-attention of the bf16 inputs: (o [batch * lq, C], lse [batch, heads, lq], log2 domain)."""
    q, k0, v0, kw = views(c)
    B, H, lq, l0, l1 = c["batch"], c["heads"], c["lq"], c["l0"], c["l1"]
    mul = 1.0 if c["q_scaled"] else 0.125 * LOG2E
    o = torch.empty(B * lq, c["C"], device=DEV, dtype=torch.float64)
    lse = torch.empty(B, H, lq, device=DEV, dtype=torch.float64)
    for b in range(B):
        qq = q[b * lq:(b + 1) * lq].double().view(lq, H, 64).transpose(0, 1)
        kk, vv = k0[:l0].double(), v0[:l0].double()
        if l1:
            r0 = b * c["stride1"]
            kk = torch.cat([kk, kw["k1"][r0:r0 + l1].double()])
            vv = torch.cat([vv, kw["v1"][r0:r0 + l1].double()])
        kk, vv = kk.view(-1, H, 64).transpose(0, 1), vv.view(-1, H, 64).transpose(0, 1)
        s = qq @ kk.transpose(1, 2) * mul                     # [H, lq, keys], exp2 domain
        m = s.max(dim=-1, keepdim=True).values
        p = torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        o[b * lq:(b + 1) * lq] = ((p / l) @ vv).transpose(0, 1).reshape(lq, H * 64)
        lse[b] = (m + torch.log2(l))[..., 0]
    return o, lse


def run_rows(ops, c):
    q, k0, v0, kw = views(c)
    o = torch.full((c["batch"] * c["lq"], c["C"]), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((c["batch"], c["heads"], c["lq"]), float("nan"), device=DEV)
    ops.attention_rows(q, k0, v0, o, lse=lse, **kw)
    assert ops.last_kernel() == f"attn_rows_kernel<{1 if c['lq'] <= 32 else 2}>"
    return o, lse


def run_sweep_kernel(ops, c):
    """sr_attention (bf16) on the same description, its output compact like the rows kernel's."""
    from sailrecon_amd import _lib as L
    q, k0, v0, kw = views(c)
    o = torch.empty(c["batch"] * c["lq"], c["C"], device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(c["batch"], c["heads"], c["lq"], device=DEV)
    d = ops._attn_desc(q, k0, v0, o, lse=lse, **kw)
    d.o_bstride = c["lq"]
    L.check(L.load().sr_attention(ops._stream(q), L.SR_BF16, ctypes.byref(d)), "sr_attention")
    return o, lse


def errors(ops, c, c_ref=None):
    """(o error, sweep kernel's o error, lse squared errors, sweep kernel's) of one case; ``c_ref``:
    the same values without the NaN padding, for the sweep kernel."""
    o_ref, lse_ref = reference(c)
    o, lse = run_rows(ops, c)
    o_s, lse_s = run_sweep_kernel(ops, c_ref or c)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    return rel(o, o_ref), rel(o_s, o_ref), (lse.double() - lse_ref) ** 2, (lse_s.double() - lse_ref) ** 2


@pytest.mark.parametrize("q_scaled", [0, 1])
@pytest.mark.parametrize("lq", LQS)
def test_rows_sweep(ops, lq, q_scaled):
    gen = torch.Generator(device=DEV).manual_seed(1000 * lq + q_scaled)
    sq, sq_s = [], []
    bad = []
    for l0, l1, batch, heads in itertools.product(L0S, L1S, BATCHES, HEADS):
        c = make_case(gen, lq=lq, l0=l0, l1=l1, batch=batch, heads=heads, q_scaled=q_scaled)
        e, e_s, d2, d2_s = errors(ops, c)
        sq.append(d2.flatten())
        sq_s.append(d2_s.flatten())
        r, r_s = math.sqrt(float(d2.mean())), math.sqrt(float(d2_s.mean()))
        print(f"lq {lq} l0 {l0} l1 {l1} batch {batch} heads {heads} q_scaled {q_scaled}: o {e:.3e} "
              f"(sr_attention {e_s:.3e})  lse rms {r:.3e} (sr_attention {r_s:.3e}, bound "
              f"{lse_bound(d2.numel(), r_s):.3e})")
        if not (e < 1e-2 and e <= 1.5 * e_s and r <= lse_bound(d2.numel(), r_s)):
            bad.append((l0, l1, batch, heads, e, e_s, r, r_s))
    assert not bad, f"(l0, l1, batch, heads, o error, sr_attention's, lse rms, sr_attention's): {bad}"
    rms, rms_s = math.sqrt(float(torch.cat(sq).mean())), math.sqrt(float(torch.cat(sq_s).mean()))
    print(f"lq {lq} q_scaled {q_scaled}: pooled lse rms {rms:.3e} (sr_attention {rms_s:.3e})")
    assert rms <= 2.0 * rms_s


@pytest.mark.parametrize("lq", [32, 33])
def test_rows_big_key_in_last_chunk(ops, lq):
    """l0 = 4100 runs 16 chunks (the last one empty): a key of 8x norm in the last non-empty chunk
    carries that chunk's maximum far above the others', so the fold rescales every other partial."""
    assert ops.rows_chunks(heads=16, batch=1, lq=lq, l0=4100) == 16
    gen = torch.Generator(device=DEV).manual_seed(7 + lq)
    c = make_case(gen, lq=lq, l0=4100, l1=0, batch=1, heads=16, q_scaled=1, big_key=True)
    e, e_s, d2, d2_s = errors(ops, c)
    r, r_s = math.sqrt(float(d2.mean())), math.sqrt(float(d2_s.mean()))
    print(f"big key, lq {lq}: o {e:.3e} (sr_attention {e_s:.3e})  lse rms {r:.3e} (sr_attention {r_s:.3e})")
    assert e < 1e-2 and e <= 1.5 * e_s and r <= 2.0 * r_s


def test_rows_nan_past_every_segment(ops):
    """Every row past l0 / l1 of each segment instance is NaN: nothing of them may be read."""
    gen = torch.Generator(device=DEV).manual_seed(11)
    c = make_case(gen, lq=33, l0=1000, l1=21, batch=3, heads=6, q_scaled=0, nan_pad=43)
    clean = dict(c, s0=torch.nan_to_num(c["s0"]), s1=torch.nan_to_num(c["s1"]))
    e, e_s, d2, d2_s = errors(ops, c, clean)
    r, r_s = math.sqrt(float(d2.mean())), math.sqrt(float(d2_s.mean()))
    print(f"nan padding: o {e:.3e} (sr_attention {e_s:.3e})  lse rms {r:.3e} (sr_attention {r_s:.3e})")
    assert e < 1e-2 and e <= 1.5 * e_s and r <= 2.0 * r_s


def test_rows_reloc_composition(ops):
    """What the aggregator's camera-only last layer does for the query frames: every frame's camera
    row as ONE query set against the shared subsample, each row against its own frame (batch = Nq,
    lq = 1), the two merged by their LSEs -- against the fp64 softmax over the union of the keys."""
    H, C, Nq, P, n_sub = 6, 384, 5, 37, 300
    gen = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(Nq * P, 3 * C, device=DEV, generator=gen).to(torch.bfloat16)
    kv_sub = torch.randn(n_sub, 2 * C, device=DEV, generator=gen).to(torch.bfloat16)
    q = qkv.view(Nq, P * 3 * C)[:, 0:C]  # row 0 of every frame, in place
    o_parts = torch.empty(2 * Nq, C, device=DEV, dtype=torch.bfloat16)
    lse_parts = torch.empty(2, H * Nq, device=DEV)
    out = torch.empty(Nq, C, device=DEV, dtype=torch.bfloat16)
    ops.attention_rows(q, kv_sub[:, 0:C], kv_sub[:, C:2 * C], o_parts[:Nq], heads=H, head_dim=64, batch=1, lq=Nq,
                       q_bstride=0, l0=n_sub, k0_bstride=0, lse=lse_parts[0])
    ops.attention_rows(q, qkv[:, C:2 * C], qkv[:, 2 * C:3 * C], o_parts[Nq:], heads=H, head_dim=64, batch=Nq, lq=1,
                       q_bstride=1, l0=P, k0_bstride=P, lse=lse_parts[1])
    ops.attn_merge_n(o_parts, lse_parts, out, parts=2, rows=Nq, heads=H, head_dim=64, seg_rows=[Nq, 1])
    ref = torch.empty(Nq, C, device=DEV, dtype=torch.float64)
    for f in range(Nq):
        qq = qkv[f * P, 0:C].double().view(H, 1, 64)
        kk = torch.cat([kv_sub[:, 0:C], qkv[f * P:(f + 1) * P, C:2 * C]]).double().view(-1, H, 64).transpose(0, 1)
        vv = torch.cat([kv_sub[:, C:2 * C], qkv[f * P:(f + 1) * P, 2 * C:3 * C]]).double().view(-1, H, 64).transpose(0, 1)
        ref[f] = (torch.softmax(qq @ kk.transpose(1, 2) * 0.125, -1) @ vv).reshape(C)
    e = rel(out, ref)
    print(f"subsample + own frame + merge: o {e:.3e}")
    assert e < 1e-2


def test_rows_rejections(ops):
    from sailrecon_amd import _lib as L
    lib = L.load()
    gen = torch.Generator(device=DEV).manual_seed(5)

    def call(c, ws_bytes=None, **over):
        q, k0, v0, kw = views(c)
        o = torch.empty(c["batch"] * c["lq"], c["C"], device=DEV, dtype=torch.bfloat16)
        d = ops._attn_desc(q, k0, v0, o, **kw)
        for k, v in over.items():
            setattr(d, k, v)
        need = int(lib.sr_attention_rows_workspace(ctypes.byref(d)))
        ws = torch.empty(max(need, 1 << 20) // 4, device=DEV)
        return lib.sr_attention_rows(ops._stream(q), L.SR_BF16, ctypes.byref(d), ops._p(ws),
                                     need if ws_bytes is None else ws_bytes(need)), need

    c = make_case(gen, lq=64, l0=100, l1=0, batch=1, heads=2, q_scaled=0)
    assert call(c)[0] == 0
    assert call(c, lq=65) == (-3, 0)                    # SR_EUNSUPPORTED
    assert call(c, head_dim=128) == (-3, 0)
    assert call(c, mask_mode=L.SR_MASK_CAMERA) == (-3, 0)
    rc, need = call(c, ws_bytes=lambda n: n - 4)
    assert rc == -1 and need > 0                        # SR_EINVAL: the workspace is too small
    torch.cuda.synchronize()
