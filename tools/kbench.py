#!/usr/bin/env python
"""Kernel microbenchmarks at the N=32 @ 518 hot-path shapes (random data).

    python tools/kbench.py [attn] [gemm] [ln]

Each case: warm up, then time R launches with HIP events on the launching stream;
prints TFLOP/s (MFMA-bound kernels) or GB/s (LayerNorm) and the fraction of peak.
"""

import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-supervise-sfm_amd"))

import torch  # noqa: E402

from sailrecon_amd import _lib, ops  # noqa: E402

DEV = "cuda"
PEAK = 2500.0


def timeit(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attn():
    C, H, D = 1024, 16, 64
    P, N = 1374, 32
    cases = {
        "global L=43968": dict(rows=N * P, batch=1, lq=N * P, l0=N * P, kb=0),
        "frame 64x1374": dict(rows=2 * N * P, batch=2 * N, lq=P, l0=P, kb=P),
    }
    # SR_KB_STATIC=1: pass the keys' true max norm as the static bound (runtime.key_norm_bound's
    # role for qk-norm blocks) instead of the key scan
    static = os.environ.get("SR_KB_STATIC", "0") == "1"
    # SR_KB_TAIL=1 (default): buffers with 64 readable rows after them, as the aggregator's
    # workspace (ops.attention tail_readable: ragged / two-segment launches may take the asm sweep)
    tail = os.environ.get("SR_KB_TAIL", "1") == "1"
    pad = 64 if tail else 0
    for name, c in cases.items():
        qkv = torch.randn(c["rows"] + pad, 3 * C, device=DEV, dtype=torch.bfloat16)[:c["rows"]]
        o = torch.empty(c["rows"], C, device=DEV, dtype=torch.bfloat16)
        kb = float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max()) if static else 0.0

        def f():
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D, batch=c["batch"],
                          lq=c["lq"], q_bstride=c["lq"], l0=c["l0"], k0_bstride=c["kb"], key_norm_max=kb,
                          tail_readable=tail)
        ms = timeit(f, reps=5 if c["batch"] == 1 else 10)
        fl = 4.0 * c["batch"] * H * c["lq"] * c["l0"] * D
        print(f"attn {name:18s} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")
    # reloc: 32 query frames x (32*305 subsample + own 1374)
    nsub = N * 305
    qkv = torch.randn(N * P + pad, 3 * C, device=DEV, dtype=torch.bfloat16)[:N * P]
    kv = torch.randn(nsub + pad, 2 * C, device=DEV, dtype=torch.bfloat16)[:nsub]
    o = torch.empty(N * P, C, device=DEV, dtype=torch.bfloat16)
    kb = max(float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max()),
             float(kv[:, :C].float().view(-1, H, D).norm(dim=-1).max())) if static else 0.0

    def f():
        ops.attention(qkv[:, :C], kv[:, :C], kv[:, C:], o, heads=H, head_dim=D, batch=N, lq=P, q_bstride=P, l0=nsub,
                      k0_bstride=0, k1=qkv[:, C:2 * C], v1=qkv[:, 2 * C:], l1=P, k1_bstride=P, key_norm_max=kb,
                      tail_readable=tail)
    ms = timeit(f)
    fl = 4.0 * N * H * P * (nsub + P) * D
    print(f"attn {'reloc 32x(9760+1374)':18s} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")
    # the same reloc attention split (aggregator SR_RELOC_SPLIT=1): all 43,968 query rows against the
    # subsample's 152 whole tiles (one long query set), each frame against the last 32 subsample
    # keys + itself, LSE merge
    rows, nf = N * P, nsub // 64 * 64
    o_parts, lse_parts = ops.key_split_workspace(DEV, 2, rows, C, H, name="kb_reloc_split")

    def pa():
        ops.attention(qkv[:, :C], kv[:nf, :C], kv[:nf, C:], o_parts[:rows], heads=H, head_dim=D, batch=1, lq=rows,
                      q_bstride=0, l0=nf, k0_bstride=0, key_norm_max=kb, lse=lse_parts[0].view(-1), tail_readable=tail)

    def pb():
        ops.attention(qkv[:, :C], kv[nf:, :C], kv[nf:, C:], o_parts[rows:], heads=H, head_dim=D, batch=N, lq=P,
                      q_bstride=P, l0=nsub - nf, k0_bstride=0, k1=qkv[:, C:2 * C], v1=qkv[:, 2 * C:], l1=P,
                      k1_bstride=P, key_norm_max=kb, lse=lse_parts[1].view(-1), tail_readable=tail)

    def pm():
        ops.attn_merge_n(o_parts, lse_parts, o, parts=2, rows=rows, heads=H, head_dim=D, seg_rows=[rows, P])

    def pbm():  # the aggregator's form: the second pass merges the first in its epilogue
        ops.attention(qkv[:, :C], kv[nf:, :C], kv[nf:, C:], o, heads=H, head_dim=D, batch=N, lq=P,
                      q_bstride=P, l0=nsub - nf, k0_bstride=0, k1=qkv[:, C:2 * C], v1=qkv[:, 2 * C:], l1=P,
                      k1_bstride=P, key_norm_max=kb, tail_readable=tail, merge_o=o_parts[:rows],
                      merge_lse=lse_parts[0])
    ta, tb, tm, tbm = timeit(pa), timeit(pb), timeit(pm), timeit(pbm)
    print(f"attn reloc split: subsample pass {ta:.3f} ms ({4.0 * H * rows * nf * D / ta / 1e9:.1f} TF/s), "
          f"tail+own pass {tb:.3f} ms, merge {tm:.3f} ms, total {ta + tb + tm:.3f} ms  "
          f"{fl / (ta + tb + tm) / 1e9:8.1f} TF/s; merge-in pass {tbm:.3f} ms, total {ta + tbm:.3f} ms  "
          f"{fl / (ta + tbm) / 1e9:8.1f} TF/s")


def attn_pair():
    """C3 global attention + the split reloc's subsample pass: apart vs one sr_attention_pair launch."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    L, nf = N * P, N * 305 // 64 * 64
    qkv = torch.randn(L + 64, 3 * C, device=DEV, dtype=torch.bfloat16)[:L]
    qr = torch.randn(L, C, device=DEV, dtype=torch.bfloat16)
    kv = torch.randn(nf, 2 * C, device=DEV, dtype=torch.bfloat16)
    og, oa = (torch.empty(L, C, device=DEV, dtype=torch.bfloat16) for _ in range(2))
    lse = torch.empty(H, L, device=DEV)
    kb = lambda k: 1.01 * float(k.float().view(-1, H, D).norm(dim=-1).max())  # noqa: E731
    kbg, kbr = kb(qkv[:, C:2 * C]), kb(kv[:, :C])

    def apart():
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], og, heads=H, head_dim=D, batch=1, lq=L,
                      q_bstride=0, l0=L, k0_bstride=0, key_norm_max=kbg)
        ops.attention(qr, kv[:, :C], kv[:, C:], oa, heads=H, head_dim=D, batch=1, lq=L, q_bstride=0, l0=nf,
                      k0_bstride=0, key_norm_max=kbr, lse=lse.view(-1))

    def paired():
        ops.attention_pair(dict(q=qkv[:, :C], k0=qkv[:, C:2 * C], v0=qkv[:, 2 * C:], o=og, lq=L, l0=L, key_norm_max=kbg),
                           dict(q=qr, k0=kv[:, :C], v0=kv[:, C:], o=oa, lq=L, l0=nf, key_norm_max=kbr,
                                lse=lse.view(-1)), heads=H, head_dim=D)
    vtg = torch.empty(ops.vt_tile_shape(L, H), device=DEV, dtype=torch.bfloat16)
    vtr = torch.empty(ops.vt_tile_shape(nf, H), device=DEV, dtype=torch.bfloat16)

    def tiles():
        ops.vt_tiles(qkv[:, 2 * C:], L, H, vtg)
        ops.vt_tiles(kv[:, C:], nf, H, vtr)

    def paired_vt():
        ops.attention_pair(dict(q=qkv[:, :C], k0=qkv[:, C:2 * C], v0=qkv[:, 2 * C:], o=og, lq=L, l0=L, key_norm_max=kbg,
                                vt=vtg),
                           dict(q=qr, k0=kv[:, :C], v0=kv[:, C:], o=oa, lq=L, l0=nf, key_norm_max=kbr,
                                lse=lse.view(-1), vt=vtr), heads=H, head_dim=D)
    tiles()
    fl = 4.0 * H * L * (L + nf) * D
    for i in range(2):
        ta, tp, tv, tt = (timeit(apart, reps=5), timeit(paired, reps=5), timeit(paired_vt, reps=5),
                          timeit(tiles, reps=20))
        print(f"attn pair C3 global + reloc subsample: apart {ta:.3f} ms ({fl / ta / 1e9:.1f} TF/s), "
              f"paired {tp:.3f} ms ({fl / tp / 1e9:.1f} TF/s), paired V^T {tv:.3f} ms ({fl / tv / 1e9:.1f} TF/s) "
              f"+ its two sr_vt_tiles {tt * 1e3:.1f} us", flush=True)


def qk_normed(rows, g, gen, H=16, D=64):
    """[rows, H*D] bf16 as the aggregator's qk-norm produces it (attention.py:49-50,78): per-head
    LayerNorm of a gaussian times w + b, w = g (1 + 0.02 n), b = 0.02 n (the synthetic rule's LN
    affine scaled by the qk-gain g; trained q_norm / k_norm gains sit around 2-3).  Returns the
    tensor and runtime.key_norm_bound's static bound sqrt(D) max|w| + |b| (x 1 + 2^-6)."""
    x = torch.randn(rows, H, D, device=DEV, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)
    w = g * (1.0 + 0.02 * torch.randn(D, device=DEV, generator=gen))
    b = 0.02 * torch.randn(D, device=DEV, generator=gen)
    kb = (D ** 0.5 * float(w.abs().max()) + float(b.norm())) * (1.0 + 2.0 ** -6)
    return (x * w + b).reshape(rows, H * D).bfloat16(), kb


def attn_gain():
    """the hand-scheduled global sweep at qk-norm gains g = 1, 2, 4 (the bound
    qb grows as g^2).  Global L = 43,968 alone and paired with the reloc subsample pass, with the
    waves that ran the asm sweep / the compiled loop (sr_attn_desc.sweep_stats)."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    L, nf = N * P, N * 305 // 64 * 64
    fl1 = 4.0 * H * L * L * D
    fl2 = 4.0 * H * L * (L + nf) * D
    gains = [float(x) for x in os.environ.get("SR_QK_GAINS", "1,2,3,4").split(",")]
    for g in gains:
        gen = torch.Generator(device=DEV).manual_seed(1)
        q, _ = qk_normed(L, g, gen)
        k, kb = qk_normed(L, g, gen)
        v = torch.randn(L, C, device=DEV, dtype=torch.bfloat16)
        qr, _ = qk_normed(L, g, gen)
        ks, kbs = qk_normed(nf, g, gen)
        vs = torch.randn(nf, C, device=DEV, dtype=torch.bfloat16)
        o, orr = torch.empty_like(q), torch.empty_like(q)
        lse = torch.empty(H, L, device=DEV)
        st = torch.zeros(2, dtype=torch.int32, device=DEV)

        def glob(stats=None):
            ops.attention(q, k, v, o, heads=H, head_dim=D, batch=1, lq=L, q_bstride=0, l0=L, k0_bstride=0,
                          key_norm_max=kb, sweep_stats=stats)

        def pair(stats=None):
            ops.attention_pair(dict(q=q, k0=k, v0=v, o=o, lq=L, l0=L, key_norm_max=kb, sweep_stats=stats),
                               dict(q=qr, k0=ks, v0=vs, o=orr, lq=L, l0=nf, key_norm_max=kbs, lse=lse.view(-1),
                                    sweep_stats=stats), heads=H, head_dim=D)
        glob(st)
        torch.cuda.synchronize()
        sg = st.tolist()
        st.zero_()
        pair(st)
        torch.cuda.synchronize()
        sp = st.tolist()
        tg, tp = timeit(glob, reps=5), timeit(pair, reps=5)
        qb = 1.4426950408889634 / 8 * kb * kb
        print(f"attn qk-gain {g:.1f} (bound qb ~ {qb:6.1f}): global {tg:.3f} ms ({fl1 / tg / 1e9:.1f} TF/s, asm waves "
              f"{sg[0]}/{sg[0] + sg[1]}); pair {tp:.3f} ms ({fl2 / tp / 1e9:.1f} TF/s, asm waves {sp[0]}/{sp[0] + sp[1]})",
              flush=True)
        # frame / DINO attention (64 frames x 1374, compiled two-workgroups-per-CU sweep) at the same gain
        S = 64
        qf = torch.cat([q, qr])[:S * P] if 2 * L >= S * P else None
        kf, kbf = qk_normed(S * P, g, gen)
        vf = torch.randn(S * P, C, device=DEV, dtype=torch.bfloat16)
        of = torch.empty_like(vf)
        tf = timeit(lambda: ops.attention(qf, kf, vf, of, heads=H, head_dim=D, batch=S, lq=P, q_bstride=P, l0=P,
                                          k0_bstride=P, key_norm_max=kbf), reps=10)
        ff = 4.0 * S * H * P * P * D
        print(f"attn qk-gain {g:.1f} frame 64x1374: {tf:.3f} ms ({ff / tf / 1e9:.1f} TF/s)", flush=True)


def attn_frame_cfg():
    """Frame / DINO attention (64 frames x 1374 tokens, static key bound) under each bf16 workgroup
    shape (SR_ATTN_CFG: 0 = 4 waves x 2 q-blocks, 1 = 8 x 1, 2 = 2 x 2 = 128 rows), interleaved."""
    C, H, D, P, S = 1024, 16, 64, 1374, 64
    qkv = torch.randn(S * P + 64, 3 * C, device=DEV, dtype=torch.bfloat16)[:S * P]
    o = torch.empty(S * P, C, device=DEV, dtype=torch.bfloat16)
    kb = float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max())
    fl = 4.0 * S * H * P * P * D
    for cfg in (0, 1, 2, 0, 1, 2):
        with ops.tuning(SR_ATTN_CFG=cfg):
            ms = timeit(lambda: ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D,
                                              batch=S, lq=P, q_bstride=P, l0=P, k0_bstride=P, key_norm_max=kb,
                                              tail_readable=True), reps=20)
            kern = ops.last_kernel()
        print(f"attn frame cfg {cfg} ({kern}): {ms:.3f} ms  {fl / ms / 1e9:.1f} TF/s", flush=True)


def attn_frame_diag():
    """Where the frame attention loses against the long sweep: the same launch with no ragged
    q-tile (lq = 1280 = 5 x 256), with full key tiles (l0 = 1408), and with 4x longer key sweeps
    (l0 = 5496, the neighbouring frames' keys), 16 heads, static key bound."""
    C, H, D, P = 1024, 16, 64, 1374
    B = 64
    qkv = torch.randn(B * P + 8 * P, 3 * C, device=DEV, dtype=torch.bfloat16)
    o = torch.empty(B * P, C, device=DEV, dtype=torch.bfloat16)
    kb = 1.01 * float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max())
    warm = torch.randn(8192, 8192, device=DEV, dtype=torch.bfloat16)
    for _ in range(20):  # clocks up before the first timed case
        warm @ warm
    for lq, l0, b in ((P, P, B), (1280, P, B), (P, 1408, B), (1280, 1408, B), (1280, 4 * P, B),
                      (P, 4 * P, B), (1024, P, B), (768, P, B), (512, P, B), (256, P, B)):
        def f():
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D, batch=b, lq=lq,
                          q_bstride=P, l0=l0, k0_bstride=P, key_norm_max=kb, tail_readable=True)
        ms = timeit(f)
        fl = 4.0 * b * H * lq * l0 * D
        print(f"attn frame-diag b={b} lq={lq:5d} l0={l0:5d} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s", flush=True)


def attn_rank():
    """Per-rank global attention of the frame-sharded C3 forward: 32/G anchors' queries against
    all 43,968 anchor keys (one pass), G = 2, 4, 8."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    L = N * P
    qkv = torch.randn(L, 3 * C, device=DEV, dtype=torch.bfloat16)
    kb = float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max())
    for G in (1, 2, 4, 8):
        lq = L // G
        o = torch.empty(lq, C, device=DEV, dtype=torch.bfloat16)

        def f():
            ops.attention(qkv[:lq, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D, batch=1, lq=lq,
                          q_bstride=0, l0=L, k0_bstride=0, key_norm_max=kb)
        saved = ops._KSPLIT_ENV
        for split in ("0", "auto", "2", "3", "4", "6", "8"):
            ops._KSPLIT_ENV = None if split == "auto" else split
            parts = ops.key_split_parts(dtype=torch.bfloat16, batch=1, lq=lq, heads=H, l0=L, l1=0, mask_mode=0)
            ms = timeit(f, reps=5)
            fl = 4.0 * H * lq * L * D
            print(f"attn rank G={G} lq={lq:6d} keys={L} split={split:4s}(S={parts}) {ms:8.3f} ms  "
                  f"{fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")
        ops._KSPLIT_ENV = saved


def attn_rank_seg():
    """attn_rank's key-split launches (auto S) with the chunks' tails readable: the compiled sweep
    vs the hand-scheduled _SEG sweep (SR_ATTN_PIPE_SEG=1), which masks each chunk's ragged last
    key tile (43,968 / S keys are not whole 64-key tiles for S = 2, 4, 8)."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    L = N * P
    qkv = torch.randn(L + 64, 3 * C, device=DEV, dtype=torch.bfloat16)[:L]
    kb = float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max())
    for G in (2, 4, 8):
        lq = L // G
        S = ops.key_split_parts(dtype=torch.bfloat16, batch=1, lq=lq, heads=H, l0=L, l1=0, mask_mode=0)
        o_parts, lse_parts = ops.key_split_workspace(qkv.device, S, lq, C, H)
        chunk = L // S
        d = ops._attn_desc(qkv[:lq, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o_parts, heads=H, head_dim=D, batch=S,
                           lq=lq, q_bstride=0, l0=chunk, k0_bstride=chunk, lse=lse_parts)
        d.o_bstride = lq
        d.key_norm_max = kb
        d.tail_rows_readable = 64
        fl = 4.0 * H * lq * L * D

        def f():
            ops.check(_lib.load().sr_attention(ops._stream(qkv), ops.dtype_code(qkv.dtype), ops.ctypes.byref(d)),
                      "sr_attention")
        res = {}
        for seg in ("0", "1", "0", "1"):
            ops.set_tuning("SR_ATTN_PIPE_SEG", int(seg))
            ms = timeit(f, reps=10)
            res.setdefault(seg, []).append(ms)
        outs = []
        for seg in ("0", "1"):
            ops.set_tuning("SR_ATTN_PIPE_SEG", int(seg))
            o_parts.zero_()
            f()
            torch.cuda.synchronize()
            outs.append((o_parts[:S * lq].float().clone(), lse_parts.clone()))
        ops.set_tuning("SR_ATTN_PIPE_SEG", 0)
        print(f"attn rank seg G={G} max |o| diff {float((outs[0][0] - outs[1][0]).abs().max()):.3e} "
              f"max |lse| diff {float((outs[0][1] - outs[1][1]).abs().max()):.3e}")
        for seg, v in res.items():
            print(f"attn rank seg G={G} S={S} chunk={chunk} pipe_seg={seg} "
                  + " ".join(f"{m:7.3f} ms ({fl / m / 1e9:7.1f} TF/s)" for m in v))


def attn_rank_small():
    """Per-rank reloc (32/G query frames x [9760 shared subsample + own 1374]) and frame
    (64/G frames x 1374) attention of the frame-sharded C3 forward, G = 1, 2, 4, 8."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    nsub = N * 305
    for G in (1, 2, 4, 8):
        nq = N // G
        qkv = torch.randn(2 * nq * P, 3 * C, device=DEV, dtype=torch.bfloat16)
        kv = torch.randn(nsub, 2 * C, device=DEV, dtype=torch.bfloat16)
        o = torch.empty(2 * nq * P, C, device=DEV, dtype=torch.bfloat16)
        kb = 1.01 * max(float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max()),
                        float(kv[:, :C].float().view(-1, H, D).norm(dim=-1).max()))

        def rl():
            ops.attention(qkv[:nq * P, :C], kv[:, :C], kv[:, C:], o, heads=H, head_dim=D, batch=nq, lq=P,
                          q_bstride=P, l0=nsub, k0_bstride=0, k1=qkv[:nq * P, C:2 * C], v1=qkv[:nq * P, 2 * C:],
                          l1=P, k1_bstride=P, key_norm_max=kb)

        def fr():
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D, batch=2 * nq, lq=P,
                          q_bstride=P, l0=P, k0_bstride=P, key_norm_max=kb)
        ms = timeit(rl)
        fl = 4.0 * nq * H * P * (nsub + P) * D
        print(f"attn rank G={G} reloc {nq:2d}x({nsub}+{P}) {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s")
        ms = timeit(fr)
        fl = 4.0 * 2 * nq * H * P * P * D
        print(f"attn rank G={G} frame {2 * nq:2d}x{P}        {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s")


def attn_rank_cfg():
    """attn_rank_small's per-rank reloc attention at G = 4 and 8 under each bf16 workgroup shape
    (SR_ATTN_CFG: -1 auto, 0 = 4 waves x 2 q-blocks, 1 = 8 x 1, 2 = 2 x 2 = 128 rows), interleaved."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    nsub = N * 305
    for G in (4, 8):
        nq = N // G
        qkv = torch.randn(nq * P + 64, 3 * C, device=DEV, dtype=torch.bfloat16)[:nq * P]
        kv = torch.randn(nsub + 64, 2 * C, device=DEV, dtype=torch.bfloat16)[:nsub]
        o = torch.empty(nq * P, C, device=DEV, dtype=torch.bfloat16)
        kb = 1.01 * max(float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max()),
                        float(kv[:, :C].float().view(-1, H, D).norm(dim=-1).max()))
        fl = 4.0 * nq * H * P * (nsub + P) * D
        for cfg in (-1, 0, 1, 2, -1, 0, 1, 2):
            with ops.tuning(SR_ATTN_CFG=cfg):
                ms = timeit(lambda: ops.attention(qkv[:, :C], kv[:, :C], kv[:, C:], o, heads=H, head_dim=D, batch=nq,
                                                  lq=P, q_bstride=P, l0=nsub, k0_bstride=0, k1=qkv[:, C:2 * C],
                                                  v1=qkv[:, 2 * C:], l1=P, k1_bstride=P, key_norm_max=kb,
                                                  tail_readable=True))
                kern = ops.last_kernel()
            print(f"attn rank cfg G={G} reloc {nq}x({nsub}+{P}) cfg {cfg:2d} ({kern}) {ms:8.3f} ms  "
                  f"{fl / ms / 1e9:8.1f} TF/s", flush=True)


def gemm_rank():
    """The block GEMMs at the per-rank row counts of the frame-sharded C3 forward (64/G frames)."""
    for G in (1, 2, 4, 8):
        gemm(2 * 32 * 1374 // G)


def gemm(M=2 * 32 * 1374):
    for name, (N, K, epi) in {"qkv": (3072, 1024, _lib.SR_EPI_BIAS), "proj": (1024, 1024, _lib.SR_EPI_BIAS_RESID),
                              "fc1": (4096, 1024, _lib.SR_EPI_BIAS_GELU), "fc2": (1024, 4096, _lib.SR_EPI_BIAS_RESID)}.items():
        a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / 32
        b = torch.randn(N, device=DEV)
        g = torch.randn(N, device=DEV)
        if epi == _lib.SR_EPI_BIAS_RESID:
            out = torch.zeros(M, N, device=DEV)
        else:
            out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        ms = timeit(lambda: ops.gemm(a, w, out, epi, bias=b, gamma=g))
        fl = 2.0 * M * N * K
        print(f"gemm {name:5s} M={M} N={N} K={K} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")


def gemm_epi(M=2 * 32 * 1374):
    """fc1's shape (N = 4,096, K = 1,024) under each epilogue, interleaved: what the erf-GELU costs
    beside the plain bias epilogue, and K = 2,048 / 4,096 for the k-loop's share."""
    N = 4096
    for K in (1024, 2048, 4096):
        a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / 32
        b = torch.randn(N, device=DEV)
        out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        fl = 2.0 * M * N * K
        for name, epi in (("bias", _lib.SR_EPI_BIAS), ("gelu", _lib.SR_EPI_BIAS_GELU)) * 2:
            ms = timeit(lambda: ops.gemm(a, w, out, epi, bias=b))
            print(f"gemm_epi {name:4s} M={M} N={N} K={K} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s", flush=True)
        del a, w


def gemm_qkv(M=2 * 32 * 1374):
    """The QKV projection at C3 rows: plain bias (DINO) against the fused qk-LayerNorm + 2-D RoPE +
    c*q epilogue (the aggregator blocks, runtime.qkv_params(prescale=True)), and the layer's grouped
    launch (queries' and anchors' QKV + the anchor-subsample K/V, sr_gemm_group)."""
    from sailrecon_amd.layers.rope import RotaryPositionEmbedding2D
    N, K, C = 3072, 1024, 1024
    a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / 32
    b = torch.randn(N, device=DEV)
    out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    rope = RotaryPositionEmbedding2D(100).tables(64, 38, DEV)
    nw = [torch.rand(64, device=DEV) + 0.5 for _ in range(4)]
    epi = dict(embed_dim=C, head_dim=64, qk_eps=1e-5, qn_w=nw[0], qn_b=nw[1] - 1, kn_w=nw[2], kn_b=nw[3] - 1,
               rope_cos=rope[0], rope_sin=rope[1], tokens_per_frame=1374, patch_start=5, grid_w=37, pos_row_base=0,
               q_scale=0.125 * 1.4426950408889634)
    fl = 2.0 * M * N * K
    ms = timeit(lambda: ops.gemm(a, w, out, _lib.SR_EPI_BIAS, bias=b))
    print(f"gemm_qkv bias              M={M} N={N} K={K} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")
    for lds in (0, 1, 0, 1):  # RoPE tables from global memory (0) or staged in LDS (1)
        with ops.tuning(SR_GEMM_ROPE_LDS=lds):
            ms = timeit(lambda: ops.gemm(a, w, out, _lib.SR_EPI_QKV, bias=b, qkv=epi))
        print(f"gemm_qkv qkv-norm-rope lds={lds} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")
    half = M // 2
    sub = torch.randint(0, half, (32 * 305,), device=DEV, dtype=torch.int32)
    kv = torch.empty(sub.numel(), 2 * C, device=DEV, dtype=torch.bfloat16)
    e_s = dict(epi, col_offset=C, pos_rowmap=sub)
    e_s.pop("pos_row_base")
    e_s.pop("q_scale")
    probs = [dict(a=a[:half], w=w, out=out[:half], bias=b, qkv=epi),
             dict(a=a[half:], w=w, out=out[half:], bias=b, qkv=dict(epi, pos_row_base=half)),
             dict(a=a[:sub.numel()], w=w[C:], out=kv, bias=b[C:], qkv=e_s)]
    flg = fl + 2.0 * sub.numel() * 2 * C * K
    for lds in (0, 1, 0, 1):
        with ops.tuning(SR_GEMM_ROPE_LDS=lds):
            ms = timeit(lambda: ops.gemm_group(probs, _lib.SR_EPI_QKV))
        print(f"gemm_qkv group (layer) lds={lds} {ms:8.3f} ms  {flg / ms / 1e9:8.1f} TF/s  {flg / ms / 1e9 / PEAK:6.1%}")


def gemm_resid():
    """SR_GEMM_RESID_LDS A/B, interleaved: the residual GEMMs (proj K=1024, fc2 K=4096) over the C3
    frame rows with the x tile staged through LDS (1) or the register epilogue (0)."""
    M, N = 2 * 32 * 1374, 1024
    x = torch.randn(M, N, device=DEV)
    b, gam = torch.randn(N, device=DEV), torch.randn(N, device=DEV) * 1e-3
    for name, K in (("proj", 1024), ("fc2 ", 4096)):
        a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(torch.bfloat16)
        fl = 2.0 * M * N * K
        for rl in (0, 1, 0, 1):
            with ops.tuning(SR_GEMM_RESID_LDS=rl):
                ms = timeit(lambda: ops.gemm(a, w, x, _lib.SR_EPI_BIAS_RESID, bias=b, gamma=gam), reps=10)
            print(f"gemm_resid {name} resid_lds={rl} {ms:.4f} ms  {fl / ms / 1e9:7.1f} TF/s", flush=True)


def gemm_k():
    """Per-tile fixed cost of the 256x256 GEMM: exactly 5 rounds of 256 tiles (M = 81,920, N = 1024)
    at K = 256 ... 4096; time = fixed + K * per-k, the intercept is the prologue / epilogue / tile
    start cost of one round."""
    M, N = 81920, 1024
    for epi, ename in ((_lib.SR_EPI_BIAS, "bias"), (_lib.SR_EPI_BIAS_RESID, "resid")):
        for K in (256, 512, 1024, 2048, 4096):
            a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / 32
            b = torch.randn(N, device=DEV)
            g = torch.randn(N, device=DEV)
            out = torch.zeros(M, N, device=DEV) if epi == _lib.SR_EPI_BIAS_RESID else \
                torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            ms = timeit(lambda: ops.gemm(a, w, out, epi, bias=b, gamma=g))
            fl = 2.0 * M * N * K
            print(f"gemm_k {ename:5s} M={M} N={N} K={K:5d} {ms:8.4f} ms  {ms / 5 * 1e3:7.2f} us/round  "
                  f"{fl / ms / 1e9:8.1f} TF/s")


def gemm_f32():
    """The exact-fp32 GEMM at DPT conv shapes (im2col'd 3x3 convs, 8 frames per chunk)."""
    for name, (M, N, K) in {"rn1 3x3 256->256 @148": (8 * 148 * 148, 256, 2304),
                            "out1 3x3 256->128 @296": (8 * 296 * 296, 128, 2304),
                            "out2 3x3 128->32 @518": (8 * 518 * 518, 32, 1152)}.items():
        a = torch.randn(M, K, device=DEV)
        w = torch.randn(N, K, device=DEV) / 32
        out = torch.empty(M, N, device=DEV)
        ms = timeit(lambda: ops.gemm(a, w, out, _lib.SR_EPI_BIAS, splits=1), reps=3)
        fl = 2.0 * M * N * K
        print(f"gemm_f32 {name:24s} M={M} N={N} K={K} {ms:8.3f} ms  {fl / ms / 1e9:7.1f} TF/s  {fl / ms / 1e9 / 157.3:6.1%}")


def gemm_cam():
    """The camera trunk's fp32 weight-streaming GEMMs (camera_head.py:163-168 trunk blocks at dim 2048,
    M = 64 camera tokens at C3): time per launch and the weight-stream rate for each split-K count
    (the automatic plan marked *)."""
    M = 64
    shapes = {"qkv  ": (6144, 2048, _lib.SR_EPI_BIAS), "proj ": (2048, 2048, _lib.SR_EPI_BIAS_RESID),
              "fc1  ": (8192, 2048, _lib.SR_EPI_BIAS_GELU), "fc2  ": (2048, 8192, _lib.SR_EPI_BIAS_RESID)}
    for name, (N, K, epi) in shapes.items():
        a = torch.randn(M, K, device=DEV)
        w = torch.randn(N, K, device=DEV) / 32
        b, gam = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
        out = torch.zeros(M, N, device=DEV)
        auto = ops._splitk_plan(M, N, K, epi, torch.float32)
        kt = K // 32
        for s in sorted({1, 2, 4, 8, 16, 32, 64, auto}):
            if kt % s or kt // s < 2:
                continue
            ms = timeit(lambda: ops.gemm(a, w, out, epi, bias=b, gamma=gam, splits=s), reps=20)
            print(f"gemm_cam {name} N={N} K={K} splits={s:2d}{'*' if s == auto else ' '} {ms * 1e3:8.1f} us  "
                  f"{N * K * 4 / ms / 1e9:6.2f} TB/s weights")


def torch_mm():
    """Yardstick only (not a product path): the library GEMM (torch.matmul -> hipBLASLt) at the
    block shapes, plain bf16 output, no epilogue."""
    M = 2 * 32 * 1374
    for name, (N, K) in {"qkv": (3072, 1024), "proj": (1024, 1024), "fc1": (4096, 1024), "fc2": (1024, 4096)}.items():
        a = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        wt = (torch.randn(N, K, device=DEV, dtype=torch.bfloat16) / 32).t()
        ms = timeit(lambda: torch.matmul(a, wt))
        fl = 2.0 * M * N * K
        print(f"torch.mm {name:5s} M={M} N={N} K={K} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}")


def ln():
    M, C = 2 * 32 * 1374, 1024
    x = torch.randn(M, C, device=DEV)
    w, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    out = torch.empty(M, C, device=DEV, dtype=torch.bfloat16)
    ms = timeit(lambda: ops.layernorm(x, w, b, 1e-5, out))
    gb = M * C * 6 / 1e9
    print(f"layernorm M={M} C={C} {ms:8.3f} ms  {gb / ms * 1e3:8.1f} GB/s")
    # the stream rate of the same bytes without the row reductions (ATen's cast copy, fp32 -> bf16):
    # the roofline the LayerNorm's 6 B per element is held against
    ms = timeit(lambda: out.copy_(x), reps=20)
    print(f"aten cast copy fp32->bf16 M={M} C={C} {ms:8.3f} ms  {gb / ms * 1e3:8.1f} GB/s")
    x2 = torch.empty_like(x)
    ms = timeit(lambda: x2.copy_(x), reps=20)
    print(f"aten copy fp32 M={M} C={C} {ms:8.3f} ms  {M * C * 8 / 1e9 / ms * 1e3:8.1f} GB/s", flush=True)
    del x2
    # x += g * y; out = LN(x) (runtime.proj_residual_ln2), y strided in the qkv slot
    ybuf = torch.randn(M, 3 * C, device=DEV).bfloat16()
    g = torch.randn(C, device=DEV) * 0.01
    ms = timeit(lambda: ops.residual_layernorm(x, ybuf[:, :C], g, w, b, 1e-5, out))
    gb = M * C * 12 / 1e9
    print(f"residual_layernorm M={M} C={C} {ms:8.3f} ms  {gb / ms * 1e3:8.1f} GB/s", flush=True)
    yc = torch.randn(M, C, device=DEV).bfloat16()  # the deferred fc2 residual: y in the o slot (ld = C)
    # SR_RLN_WIDE variants: bit 0 16-B lanes, bit 1 two rows in flight per wave, bit 2 nt x stores
    for var in (0, 1, 2, 3, 4, 6, 0, 1, 2, 3, 4, 6):
        with ops.tuning(SR_RLN_WIDE=var):
            ms = timeit(lambda: ops.residual_layernorm(x, yc, g, w, b, 1e-5, out), reps=20)
        print(f"residual_layernorm (y ld=C, variant {var}) M={M} C={C} {ms:8.3f} ms  {gb / ms * 1e3:8.1f} GB/s",
              flush=True)


def dpt():
    """DPT point + depth heads on 32 query frames @518, fp32."""
    from sailrecon_amd.heads.dpt_head import DPTHead
    from sailrecon_amd.utils.synth_weights import synth_state_dict_like
    S, H, W, C, P = 32, 518, 518, 2048, 1374
    g = torch.Generator(device=DEV).manual_seed(0)
    toks = {l: torch.randn(1, S, P, C, device=DEV, generator=g) for l in (4, 11, 17, 23)}
    images = torch.rand(1, S, 3, H, W, device=DEV, generator=g)
    for kind, kw in (("point", dict(output_dim=4, activation="inv_log")), ("depth", dict(output_dim=2, activation="exp"))):
        m = DPTHead(dim_in=C, **kw)
        m.load_state_dict(synth_state_dict_like(m))
        m = m.to(DEV)
        ms = timeit(lambda: m(toks, images=images, patch_start_idx=5), reps=2, warm=1)
        print(f"dpt {kind:5s} head S={S} @{H}  {ms:9.2f} ms  ({ms / S:.2f} ms/frame)")


def reloc():
    """Two-phase relocalisation at N=32 anchors @518 (bf16 aggregator, fp32 heads): tmp_forward
    once, then reloc() of single query views (train/demo_imc.py flow)."""
    from sailrecon_amd.models.sail_recon import SailRecon
    from sailrecon_amd.utils.synth_weights import synth_state_dict_like
    n = 32
    m = SailRecon(kv_cache=True)
    m.load_state_dict(synth_state_dict_like(m))
    m = m.to(DEV).eval()
    x = torch.rand(n, 3, 518, 518, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ms1 = timeit(lambda: m.tmp_forward(x, fix_rank=300), reps=2, warm=1)
        for flags, name in ((dict(fast_reloc=True), "pose only"), (dict(), "pose+depth"),
                            (dict(memory_save=False, ret_img=True), "all heads")):
            ms = timeit(lambda: m.reloc(x[:1], fix_rank=300, **flags), reps=5, warm=2)
            print(f"reloc 1 view vs {n} anchors @518 ({name:10s}) {ms:8.2f} ms")
    print(f"tmp_forward {n} anchors @518            {ms1:8.2f} ms")


def io():
    """Input formation: 32 views 768x1024 -> 518 (pad to square, Pillow
    BICUBIC, ToTensor), RGB and uint16 depth; kernel passes with pixels resident in HBM, then the
    whole ImagePreprocessor.process_views from PIL images (host decode arrays + H2D included),
    beside Pillow on one host core."""
    import numpy as np
    from PIL import Image
    from sailrecon_amd.utils import io as sio
    n, h, w, T = 32, 768, 1024, 518
    m, pl, pt = max(h, w), 0, (max(h, w) - h) // 2
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dep = rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    for mode, arr, c, esz in ((sio.MODE_8BIT, rgb, 3, 1), (sio.MODE_I16, dep, 1, 2)):
        pix = sio._upload(list(arr), DEV)
        bh, kh = sio.pil_table(m, T, mode, DEV, quads=True, pad=pl, extent=w)
        bv, kv = sio.pil_table(m, T, mode, DEV, pad=pt, extent=h)
        tmp = ops.pil_tmp(n, c, h, T, pix.dtype, DEV)
        out = torch.empty(n, c, T, T, device=DEV)
        div = 255.0 if mode == sio.MODE_8BIT else 1000.0
        th_ = timeit(lambda: ops.pil_resample_h(mode, pix, bh, kh, T, tmp), reps=20)
        tv_ = timeit(lambda: ops.pil_resample_v(mode, tmp, bv, kv, div, out), reps=20)
        name = "rgb  " if mode == sio.MODE_8BIT else "depth"
        ldt = (T + 3) // 4 * 4
        bh_ = n * (h * w * c * esz + h * ldt * c * esz)
        bv_ = n * (h * ldt * c * esz + c * T * T * 4)
        ba_ = n * (h * w * c * esz + c * T * T * 4)
        print(f"io {name} h pass {th_ * 1e3:8.1f} us  {bh_ / th_ / 1e6:7.1f} GB/s   "
              f"v pass {tv_ * 1e3:8.1f} us  {bv_ / tv_ / 1e6:7.1f} GB/s   ({(th_ + tv_) / n * 1e3:.1f} us/view; "
              f"in+out {ba_ / n / 1e6:.2f} MB/view -> {ba_ / (th_ + tv_) / 1e6:.0f} GB/s)")
    pre = sio.ImagePreprocessor(T, device=DEV)
    ims = [Image.fromarray(a) for a in rgb]
    dims = [Image.fromarray(a) for a in dep]
    ms = timeit(lambda: pre.process_views(ims), reps=3, warm=1)
    msd = timeit(lambda: pre.process_views(dims, is_depth=True), reps=3, warm=1)
    print(f"io process_views from PIL (incl. host arrays + H2D): rgb {ms / n:.3f} ms/view  depth {msd / n:.3f} ms/view")
    t0 = time.perf_counter()
    for im in ims[:8]:
        sq = Image.new("RGB", (m, m))
        sq.paste(im, (pl, pt))
        np.asarray(sq.resize((T, T), Image.Resampling.BICUBIC), dtype=np.float32) / 255
    t1 = time.perf_counter()
    for im in dims[:4]:
        sq = Image.new(im.mode, (m, m))
        sq.paste(im, (pl, pt))
        np.asarray(sq.resize((T, T), Image.Resampling.BICUBIC)).astype(np.float32) / 1000
    t2 = time.perf_counter()
    print(f"io Pillow on 1 host core: rgb {(t1 - t0) / 8 * 1e3:.2f} ms/view  depth {(t2 - t1) / 4 * 1e3:.2f} ms/view")


def corres(P=240, hs=560, ws=560, K=10000, views=16, dh=768, dw=1024):
    """Training correspondences and depths (sr_corres_sample; train/utils/io.py:280-360 per pair) at a
    16-view scene's size: P ordered pairs of hs x ws matcher maps, K samples each, views depth maps
    of dh x dw.  HIP-event time of the launch sequence for both input forms, the H2D time of each
    form's inputs from pinned memory, and the achieved GB/s against the bytes the kernels must move
    (scan: certainty in, fp64 CDF out; sample: uniforms in, six fp32 + one int32 out per point plus
    the binary search's reads, counted as ceil(log2(chunks)) + ceil(log2(2048)) doubles)."""
    import math
    M = hs * ws
    g = torch.Generator(device=DEV).manual_seed(0)
    depths = [1 + 4 * torch.rand(dh, dw, device=DEV, generator=g) for _ in range(views)]
    order = [(a, b) for a in range(views) for b in range(views) if a != b][:P]
    png, f32 = [], []
    for _ in range(P):
        t = torch.randint(0, 65536, (3, hs, ws), device=DEV, generator=g, dtype=torch.int32)
        t[2] %= 1001
        png.append((t - 65536 * (t >= 32768)).to(torch.int16))  # the uint16 bits
        v = t.float()
        f32.append((torch.rand(M, 2, device=DEV, generator=g) * 2 - 1,
                    torch.stack([v[0] / 65535.0 * 2 - 1, v[1] / 65535.0 * 2 - 1], -1).reshape(M, 2).contiguous(),
                    (v[2] / 1000).reshape(M).contiguous()))
    u = torch.rand(P, K, device=DEV, dtype=torch.float64, generator=g)
    recs_png = [dict(x_png=t[0], y_png=t[1], conf_png=t[2], depth_src=depths[a], depth_dst=depths[b])
                for t, (a, b) in zip(png, order)]
    recs_f32 = [dict(coords_src=c[0], coords_dst=c[1], certainty=c[2], depth_src=depths[a], depth_dst=depths[b])
                for c, (a, b) in zip(f32, order)]
    steps = math.ceil(math.log2(max(2, math.ceil(M / 2048)))) + 11
    out_bytes = P * K * (8 + 8 * steps + 6 * 4 + 4)
    for name, recs, esz in (("f32  ", recs_f32, 4), ("png16", recs_png, 2)):
        ms = timeit(lambda: ops.corres_sample(recs, u, 0.1, check=False), reps=200, warm=3)
        t0 = time.perf_counter()
        ops.corres_sample(recs, u, 0.1)
        wall = (time.perf_counter() - t0) * 1e3
        moved = P * M * (esz + 8) + out_bytes
        print(f"corres {name} P {P} M {M} K {K}: launch sequence {ms:8.3f} ms  ({ms / P * 1e3:.1f} us/pair)  "
              f"{moved / ms / 1e6:7.1f} GB/s of {moved / 1e6:.0f} MB   call incl. table + readback {wall:.2f} ms",
              flush=True)
    for name, tensors in (("f32  ", [t for c in f32 for t in c]), ("png16", png)):
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t) for t in tensors]
        dst = [torch.empty_like(t) for t in tensors]
        nbytes = sum(t.numel() * t.element_size() for t in tensors)
        ms = timeit(lambda: [d.copy_(h, non_blocking=True) for d, h in zip(dst, host)], reps=10, warm=1)
        print(f"corres {name} H2D of the correspondence inputs (pinned): {ms:8.2f} ms  {nbytes / 1e6:.0f} MB  "
              f"{nbytes / ms / 1e6:.1f} GB/s", flush=True)
        del host, dst
    nd = views * dh * dw * 4
    print(f"corres depth maps: {nd / 1e6:.0f} MB for {views} views (resident: ImagePreprocessor's output)")


def attn_fp8():
    """Global attention with q.k^T in block-scaled fp8 (BASELINE C5) vs the bf16 kernel, at the
    C3 (L = 43,968) and C5 (L = 175,872) global lengths; the fp8 time includes both quantisations."""
    C, H, D, P = 1024, 16, 64, 1374
    for n in (32, 128):
        L = n * P
        qkv = torch.randn(L, 3 * C, device=DEV, dtype=torch.bfloat16)
        o = torch.empty(L, C, device=DEV, dtype=torch.bfloat16)
        ws = ops.Fp8Workspace()
        fl = 4.0 * H * L * L * D
        kb = float(qkv[:, C:2 * C].float().view(-1, H, D).norm(dim=-1).max())  # the static key bound's role
        for name, f in (("bf16", lambda: ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D,
                                                        batch=1, lq=L, q_bstride=0, l0=L, k0_bstride=0,
                                                        key_norm_max=kb)),
                        ("fp8 qk", lambda: ops.attention_qk8(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H,
                                                           batch=1, lq=L, q_bstride=0, l0=L, k0_bstride=0, ws=ws,
                                                           key_norm_max=kb)),
                        ("fp8 qkv", lambda: ops.attention_qk8(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H,
                                                            batch=1, lq=L, q_bstride=0, l0=L, k0_bstride=0, ws=ws,
                                                            fp8_v=True))):
            ms = timeit(f, reps=3 if n == 128 else 5, warm=1)
            print(f"attn global L={L:6d} {name:7s} {ms:9.3f} ms  {fl / ms / 1e9:8.1f} TF/s", flush=True)


def attn_bwd():
    """Attention backward at the training shapes (C4: 16 anchors -> global L = 21984; frames; the
    reloc block: 16 query frames against SR_BWD_RELOC_ANCHORS shared anchor keys + their own frame)."""
    C, H, D, P = 1024, 16, 64, 1374
    na = int(os.environ.get("SR_BWD_RELOC_ANCHORS", "9984"))
    shapes = [("global L=21984", 16 * P, 1, 16 * P, 0), ("frame 32x1374", 32 * P, 32, P, 0)]
    if os.environ.get("SR_BWD_RELOC", "1") != "0":
        shapes.append((f"reloc 16x{P}+{na}", 16 * P, 16, P, na))
    for name, rows, batch, lq, anchors in shapes:
        qkv = torch.randn(rows, 3 * C, device=DEV, dtype=torch.bfloat16)
        o = torch.empty(rows, C, device=DEV, dtype=torch.bfloat16)
        lse = torch.empty(batch, H, lq, device=DEV)
        kb = 0 if batch == 1 else lq
        if anchors:  # segment 0: anchor keys shared by every item; segment 1: the item's own frame
            akv = torch.randn(anchors, 2 * C, device=DEV, dtype=torch.bfloat16)
            seg = dict(k0=akv[:, :C], v0=akv[:, C:], l0=anchors, k0_bstride=0, l1=lq, k1_bstride=lq)
            dka = torch.empty(anchors, 2 * C, device=DEV)
        else:
            seg = dict(k0=qkv[:, C:2 * C], v0=qkv[:, 2 * C:], l0=lq, k0_bstride=kb)
        fwd_kw = dict(seg)
        k0, v0 = fwd_kw.pop("k0"), fwd_kw.pop("v0")
        if anchors:
            fwd_kw.update(k1=qkv[:, C:2 * C], v1=qkv[:, 2 * C:])
        ops.attention(qkv[:, :C], k0, v0, o, heads=H, head_dim=D, batch=batch, lq=lq, q_bstride=lq, lse=lse,
                      **fwd_kw)
        g = torch.randn(rows, C, device=DEV, dtype=torch.bfloat16)
        d = torch.empty(rows, 3 * C, device=DEV)
        delta = torch.empty(batch * H * lq, device=DEV)

        def f():
            if anchors:
                ops.attention_bwd(qkv[:, :C], k0, v0, o, lse, g, d[:, :C], dka[:, :C], dka[:, C:], delta, heads=H,
                                  batch=batch, lq=lq, q_bstride=lq, dk1=d[:, C:2 * C], dv1=d[:, 2 * C:], **fwd_kw)
            else:
                ops.attention_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, lse, g, d[:, :C], d[:, C:2 * C],
                                  d[:, 2 * C:], delta, heads=H, batch=batch, lq=lq, q_bstride=lq, l0=lq, k0_bstride=kb)
        fl = 10.0 * batch * H * lq * (lq + anchors) * D  # S, dP, dV, dK, dQ (flash-attention backward convention)
        # compiled sweeps (kb1), the asm sweeps (pipe2), + the concatenated-items dK/dV sweep (cat)
        arms = [("kb1", dict(SR_ATTN_BWD_PIPE=0, SR_ATTN_BWD_DQ_PIPE=0, SR_ATTN_BWD_CAT=0)),
                ("pipe2", dict(SR_ATTN_BWD_PIPE=1, SR_ATTN_BWD_DQ_PIPE=1, SR_ATTN_BWD_CAT=0)),
                ("cat", dict(SR_ATTN_BWD_PIPE=1, SR_ATTN_BWD_DQ_PIPE=1, SR_ATTN_BWD_CAT=1))]
        if os.environ.get("SR_BWD_AB") == "pipe":  # the asm sweeps only (A/B of library builds)
            arms = arms[1:2]
        for arm, sw in arms * 2:
            with ops.tuning(**sw):
                ms = timeit(f, reps=3 if batch == 1 else 5, warm=1)
            print(f"attn_bwd {name:16s} {arm:5s} {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TF/s  {fl / ms / 1e9 / PEAK:6.1%}",
                  flush=True)


def qk_bwd():
    """sr_qk_bwd at the C4 frame block's shape (43,968 rows, q|k|v 3,072 columns, qk-norm + RoPE):
    plain, plain + the bf16 column sum of its output (the qkv bias grad, as before round 6), and
    with the column sum from the same pass (bias_grad)."""
    from sailrecon_amd.layers.rope import RotaryPositionEmbedding2D
    R, C, D = 32 * 1374, 1024, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    raw = torch.randn(R, 3 * C, device=DEV, generator=g).bfloat16()
    dsrc = torch.randn(R, 3 * C, device=DEV, generator=g)
    out = torch.empty(R, 3 * C, device=DEV, dtype=torch.bfloat16)
    rope = RotaryPositionEmbedding2D(100).tables(D, 37, DEV)
    epi = dict(embed_dim=C, head_dim=D, qk_eps=1e-6, qn_w=torch.randn(D, device=DEV), qn_b=torch.randn(D, device=DEV),
               kn_w=torch.randn(D, device=DEV), kn_b=torch.randn(D, device=DEV), rope_cos=rope[0], rope_sin=rope[1],
               tokens_per_frame=1374, patch_start=5, grid_w=37, pos_row_base=0)
    grads = torch.zeros(4, 64, device=DEV)
    bg = torch.zeros(3 * C, device=DEV)

    def plain():
        ops.qk_bwd(raw, dsrc, out, epi, grads=grads)

    def plain_cs():
        ops.qk_bwd(raw, dsrc, out, epi, grads=grads)
        ops.colsum(out, bg, accumulate=True)

    def fused():
        ops.qk_bwd(raw, dsrc, out, epi, grads=grads, bias_grad=bg)
    for i in range(2):
        tp, tc, tf = timeit(plain, reps=20), timeit(plain_cs, reps=20), timeit(fused, reps=20)
        print(f"qk_bwd C4 frame rows: plain {tp * 1e3:.1f} us, plain + colsum {tc * 1e3:.1f} us, "
              f"fused colsum {tf * 1e3:.1f} us", flush=True)


def train():
    """BASELINE config 4 (train_imc.py step, 16-view batches): full-size SailRecon aggregator +
    camera head (DPT heads off: no loss reaches them), seeded synthetic weights, a synthetic
    16-view IMC-shaped batch (15 chained pairs x 1024 correspondences, per-frame CDF nodes), bf16
    aggregator / fp32 heads, fwd + loss + bwd + Adam per step.  SR_TRAIN_QK_GAIN=g scales every
    q_norm / k_norm weight by g first (trained-like gains)."""
    from sailrecon_amd.models.sail_recon import SailRecon
    from sailrecon_amd.train.data import synthetic_batch
    from sailrecon_amd.train.loss import CDFLossIndexPytorch
    from sailrecon_amd.train.step import Trainer, prepare_model_input
    from sailrecon_amd.utils.synth_weights import synth_state_dict_like
    n = int(os.environ.get("SR_TRAIN_VIEWS", "16"))
    steps = int(os.environ.get("SR_TRAIN_STEPS", "3"))
    t0 = time.perf_counter()
    m = SailRecon(enable_point=False, enable_depth=False)
    m.load_state_dict(synth_state_dict_like(m), strict=False)
    gain = float(os.environ.get("SR_TRAIN_QK_GAIN", "1"))
    if gain != 1.0:  # trained-like q_norm / k_norm weights (bench.py --qk-gain)
        with torch.no_grad():
            for mod in m.modules():
                for nm in ("q_norm", "k_norm"):
                    ln = getattr(mod, nm, None)
                    if ln is not None and getattr(ln, "weight", None) is not None:
                        ln.weight.mul_(gain)
    m = m.to(DEV)
    print(f"train: model built in {time.perf_counter() - t0:.1f} s (qk-norm gain {gain:g})", flush=True)
    b = synthetic_batch(n, n_points=1024, size=518, seed=0)
    cdf = CDFLossIndexPytorch(0.0, 15.0, 250, b["src_idx"], b["dst_idx"], gradient_smooth=0.05, num_nodes=n)
    tr = Trainer(m, max_lr=2e-4, warmup_steps=2000, max_steps=100_000, cdf=cdf)
    imgs, na, nq = prepare_model_input(b["rgb_processed"].to(DEV))
    ops.TIMER = ops.KernelTimer()
    out = tr.step(imgs, na, nq, b)  # warmup (allocates tapes / packs)
    torch.cuda.synchronize()
    print(f"train: warmup step loss {out['loss']:.5f}  peak HBM {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB",
          flush=True)
    # the step time without instrumentation (the per-op HIP events of ops.KernelTimer cost host time,
    # and the backward's short launches run where the host is only just ahead), then the same steps
    # again under the kernel timer for the per-class breakdown
    ops.TIMER = None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        out = tr.step(imgs, na, nq, b)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / steps
    ops.TIMER = ops.KernelTimer()
    ev[0].record()
    for _ in range(steps):
        tr.step(imgs, na, nq, b)
    ev[1].record()
    torch.cuda.synchronize()
    ms_timed = ev[0].elapsed_time(ev[1]) / steps
    summ = ops.TIMER.summary()
    ops.TIMER = None
    tot = 0.0
    for tag, r in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"]):
        tot += r["total_ms"] / steps
        print(f"  {tag:22s} {r['total_ms'] / steps:9.2f} ms/step  {r['launches'] // steps:5d} launches  "
              f"{r['tflops']:7.1f} TF/s")
    print(f"train: {n} views ({2 * n} frames @518) {ms:.1f} ms/step = {n / ms * 1e3:.2f} views/s "
          f"({1e3 / ms:.3f} steps/s); under the kernel timer {ms_timed:.1f} ms/step, timed kernels {tot:.1f} ms; "
          f"loss {out['loss']:.5f}", flush=True)
    # the box's calibration GEMM (bench.py box_calibration), so that steps from different boxes compare
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from bench import box_calibration
    cal = box_calibration(torch.device(DEV))
    print(f"train: box calibration {cal['tflops']} TF/s ({cal['kernel']}, {cal['shape']})", flush=True)


def attn_rows():
    """The camera rows of a pose-only C3 forward's last layer (ops.attention_rows, sr_attention_rows):
    32 rows x 43,968 keys (global), and 32 rows x 9,760 subsample keys + 1,374 own-frame keys with
    the LSE merge (reloc); 16 heads, the rows read in place from the packed q|k|v buffer.  Time and
    achieved GB/s against the K + V bytes of each launch."""
    C, H, D, P, N = 1024, 16, 64, 1374, 32
    nsub = N * 305
    qkv = torch.randn(N * P, 3 * C, device=DEV, dtype=torch.bfloat16)
    kv = torch.randn(nsub, 2 * C, device=DEV, dtype=torch.bfloat16)
    q = qkv.view(N, P * 3 * C)[:, :C]
    o = torch.empty(N, C, device=DEV, dtype=torch.bfloat16)
    o_parts = torch.empty(2 * N, C, device=DEV, dtype=torch.bfloat16)
    lse_parts = torch.empty(2, H * N, device=DEV)
    kw = dict(heads=H, head_dim=D, tag=None)

    def glob():
        ops.attention_rows(q, qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=1, lq=N, q_bstride=0, l0=N * P, k0_bstride=0, **kw)

    def sub():
        ops.attention_rows(q, kv[:, :C], kv[:, C:], o_parts[:N], batch=1, lq=N, q_bstride=0, l0=nsub, k0_bstride=0,
                           lse=lse_parts[0], **kw)

    def own():
        ops.attention_rows(q, qkv[:, C:2 * C], qkv[:, 2 * C:], o_parts[N:], batch=N, lq=1, q_bstride=1, l0=P,
                           k0_bstride=P, lse=lse_parts[1], **kw)

    def merge():
        ops.attn_merge_n(o_parts, lse_parts, o, parts=2, rows=N, heads=H, head_dim=D, seg_rows=[N, 1])

    def reloc():
        sub()
        own()
        merge()
    for name, fn, keys in (("global 32 x 43968", glob, N * P), ("reloc subsample 32 x 9760", sub, nsub),
                           ("reloc own 32 x (1 x 1374)", own, N * P), ("reloc merge", merge, 0),
                           ("reloc 32 x (9760 + 1374)", reloc, nsub + N * P)):
        ms = timeit(fn, reps=20, warm=3)
        nb = 2.0 * keys * C * 2
        if fn is merge:  # no K / V stream, and sr_attn_merge_n does not report its kernel
            print(f"attn_rows {name:28s} {ms * 1e3:8.1f} us  (attn_merge_n_bf16_kernel)")
            continue
        print(f"attn_rows {name:28s} {ms * 1e3:8.1f} us  {nb / 1e6:7.1f} MB K+V  {nb / ms / 1e6:8.1f} GB/s  "
              f"({ops.last_kernel()})")


def cloud(runs=3):
    """Nearest-neighbour sweep of the point-cloud scores (sr_cloud_nn: every output) against a chunked
    ``torch.cdist(q, t).min(1)`` (its distance matrix in chunks of at most 2 GiB), in alternation in one
    process, ``runs`` timed runs each after one warm-up, HIP events.  Shapes: 2^20 x 2^20 and 2^18 x 8.6 M
    (a probe against a 32-view scene at 518 px).  Per shape: pairs/s, and the fraction of the fp32 VALU
    rate with the inner loop counted as 9 operations per pair (3 subtractions, a multiply, 2 FMAs, a
    minimum, a compare and a select, an FMA counted once): plain = 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz
    = 78.6 T op/s (MI355X_MICROARCH: a wave64 VALU instruction issues in 2 cycles), packed = twice that,
    every operation a two-wide v_pk_*.  Then the largest dist difference between the two on a cloud 1e3
    from the origin with 1e-3 between neighbours."""
    plain = 256 * 4 * 32 * 2.4e9
    g = torch.Generator(device=DEV).manual_seed(0)

    def kernel(q, t):
        dist = torch.empty(q.shape[0], device=DEV, dtype=torch.float32)
        index = torch.empty(q.shape[0], device=DEV, dtype=torch.int32)
        hist = torch.empty(1026, device=DEV, dtype=torch.int32)
        stats = torch.empty(6, device=DEV, dtype=torch.float64)
        ops.cloud_nn(q, t, dist=dist, index=index, hist=hist, bin_len=0.001, stats=stats)
        return dist

    def baseline(q, t):
        rows = max(1, (1 << 29) // t.shape[0])
        return torch.cat([torch.cdist(q[a:a + rows], t).min(1).values for a in range(0, q.shape[0], rows)])

    for nq, nt in ((1 << 20, 1 << 20), (1 << 18, 8_600_000)):
        q = torch.rand(nq, 3, device=DEV, generator=g) * 2 - 1
        t = torch.rand(nt, 3, device=DEV, generator=g) * 2 - 1
        times = {"sr_cloud_nn": [], "cdist+min": []}
        fns = {"sr_cloud_nn": kernel, "cdist+min": baseline}
        for name, fn in fns.items():
            fn(q, t)
        torch.cuda.synchronize()
        for _ in range(runs):
            for name, fn in fns.items():
                times[name].append(timeit(lambda: fn(q, t), reps=1, warm=0))
        diff = float((kernel(q, t) - baseline(q, t)).abs().max())
        for name, ms in times.items():
            best, rate = min(ms), nq * nt / (min(ms) * 1e-3)
            print(f"cloud {nq} x {nt} {name:11s}: " + " ".join(f"{m:9.2f}" for m in ms) + f" ms  best {best:9.2f} ms  "
                  f"{rate / 1e12:6.3f} T pairs/s  {9 * rate / plain:6.1%} of the plain, {9 * rate / (2 * plain):6.1%} of the "
                  f"packed fp32 VALU rate", flush=True)
        print(f"cloud {nq} x {nt}: sr_cloud_nn is {min(times['cdist+min']) / min(times['sr_cloud_nn']):.2f} x the baseline's "
              f"speed; largest dist difference {diff:.3e}  [{ops.last_kernel()}]", flush=True)
        del q, t
    q = 1e3 + 1e-3 * 11 * torch.rand(4096, 3, device=DEV, generator=g)
    t = 1e3 + 1e-3 * 11 * torch.rand(65536, 3, device=DEV, generator=g)
    ref = torch.cat([torch.cdist(q[a:a + 256].double(), t.double()).min(1).values for a in range(0, 4096, 256)])
    print(f"cloud far (1e3 + 1e-3 U(0, 11), 4096 x 65536; fp64 distances up to {float(ref.max()):.3e}): largest dist "
          f"difference sr_cloud_nn - cdist+min {float((kernel(q, t) - baseline(q, t)).abs().max()):.3e}; against fp64: "
          f"sr_cloud_nn {float((kernel(q, t).double() - ref).abs().max()):.3e}, cdist+min "
          f"{float((baseline(q, t).double() - ref).abs().max()):.3e}", flush=True)


def depth(runs=3):
    """Depth-map scoring (sr_depth_eval: MEDIAN alignment, a group per view, a validity mask) against the
    torch statement (masked ``torch.median`` per view, the metrics in fp32, one ``.item()`` per metric),
    in alternation in one process, ``runs`` timed runs each after one warm-up, HIP events.  Two pairs:
    every output (aligned, rel_err and the exact median / p90 of rel) against the statement with
    ``median`` / ``kthvalue`` of rel, and the sums, counts and histogram alone against the statement
    without them.  Shapes: 64 x 518 x 518 and 5 x 518 x 518.  Effective GB/s = the bytes read once (pred,
    gt, mask: 9 per pixel) over the time, beside the 6.3 TB/s a streaming kernel reaches on this part
    (MI355X_MICROARCH "HBM").  Then sr_select_ranks alone (median and p90 of one [64, 518 x 518] fp32
    tensor, 4 bytes per element read once) for the automatic and explicit workgroups per row."""
    g = torch.Generator(device=DEV).manual_seed(0)
    ln10 = 2.302585092994046

    def kernel(p, gt, m, full):
        nv, n = p.shape
        xf = torch.empty(nv, 2, device=DEV, dtype=torch.float64)
        status = torch.empty(nv, device=DEV, dtype=torch.int32)
        stats = torch.empty(nv + 1, 16, device=DEV, dtype=torch.float64)
        hist = torch.empty(nv + 1, 1026, device=DEV, dtype=torch.int32)
        extra = {}
        if full:
            extra = dict(aligned=torch.empty(nv, n, device=DEV), rel_err=torch.empty(nv, n, device=DEV),
                         rel_q=torch.empty(nv + 1, 2, device=DEV))
        ops.depth_eval(p, gt, align="median", xform=xf, status=status, stats=stats, hist=hist, bin_len=0.005, mask=m, **extra)
        return torch.cat([stats.reshape(-1), xf.reshape(-1)]).cpu()  # the one D2H copy

    def statement(p, gt, m, full):
        out = []
        for v in range(p.shape[0]):
            ok = m[v].bool() & torch.isfinite(gt[v]) & (gt[v] > 0) & torch.isfinite(p[v])
            pv, gv = p[v][ok], gt[v][ok]
            a = pv * (gv.median() / pv.median())
            e = a - gv
            rel, d, r = e.abs() / gv, a.log() - gv.log(), torch.maximum(a / gv, gv / a)
            vals = [rel.mean(), (e * e / gv).mean(), (e * e).mean().sqrt(), (d * d).mean().sqrt(),
                    100 * d.var(unbiased=False).sqrt(), d.abs().mean() / ln10, (r < 1.25).float().mean(),
                    (r < 1.5625).float().mean(), (r < 1.953125).float().mean()]
            if full:
                vals += [rel.median(), rel.kthvalue((9 * rel.numel() + 9) // 10).values]
            out.append([x.item() for x in vals])
        return out

    for nv in (64, 5):
        n = 518 * 518
        gt = torch.rand(nv, n, device=DEV, generator=g) * 5 + 1
        p = (gt * (1 + 0.05 * torch.randn(nv, n, device=DEV, generator=g)) - 0.05) / 1.1
        gt[:, ::17] = 0
        m = (torch.rand(nv, n, device=DEV, generator=g) > 0.03).to(torch.uint8)
        fns = {"sr_depth_eval, every output": lambda: kernel(p, gt, m, True),
               "torch statement with rel quantiles": lambda: statement(p, gt, m, True),
               "sr_depth_eval, sums and histogram": lambda: kernel(p, gt, m, False),
               "torch statement": lambda: statement(p, gt, m, False)}
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(runs):
            for name, fn in fns.items():
                times[name].append(timeit(fn, reps=1, warm=0))
        for name, ms in times.items():
            print(f"depth {nv} x 518 x 518 {name:35s}: " + " ".join(f"{t:8.3f}" for t in ms) + f" ms  best {min(ms):8.3f} ms  "
                  f"{9 * nv * n / (min(ms) * 1e-3) / 1e9:8.1f} GB/s effective (HBM streaming: 6300)", flush=True)
        k, s = kernel(p, gt, m, True), statement(p, gt, m, True)
        abs_rel = (k[:nv * 16].reshape(nv, 16)[:, 3] / k[:nv * 16].reshape(nv, 16)[:, 0]).numpy()
        print(f"depth {nv} x 518 x 518: every output {min(times['torch statement with rel quantiles']) / min(times['sr_depth_eval, every output']):.1f} x, "
              f"sums and histogram {min(times['torch statement']) / min(times['sr_depth_eval, sums and histogram']):.1f} x the "
              f"statement's speed; largest abs_rel difference {max(abs(abs_rel[v] - s[v][0]) for v in range(nv)):.2e}  "
              f"[{ops.last_kernel()}]", flush=True)
        if nv == 64:
            value = torch.empty(nv, 2, device=DEV)
            for bpr in (0, 1, 4, 16, 66, 262):
                ms = [timeit(lambda: ops.select_ranks(p, [(1, 2), (9, 10)], value, blocks_per_row=bpr), reps=1, warm=0)
                      for _ in range(runs + 1)][1:]
                print(f"select 64 x 518 x 518, 2 ranks, blocks_per_row {bpr:3d}: " + " ".join(f"{t:7.3f}" for t in ms) +
                      f" ms  best {min(ms):7.3f} ms  {4 * nv * n / (min(ms) * 1e-3) / 1e9:8.1f} GB/s effective, 4 passes", flush=True)
        del gt, p, m


def voxel(runs=3):
    """The stable radix sort and the voxel downsampling (sr_sort_pairs, sr_cloud_voxel) against their torch
    statements, in alternation in one process, ``runs`` timed runs each after one warm-up, HIP events, each
    side ending in its D2H copy.
      sort      sr_sort_pairs (keys and permutation out) against torch.sort(stable=True) on int64, n = 5 and
                32 x 518^2, key_bits 31 and 64.  GB/s per pass = 32 bytes per element (the histogram reads
                the key, the scatter reads key and value and writes both) over the time of one pass, beside
                the 6.3 TB/s a streaming kernel reaches on this part (MI355X_MICROARCH "HBM").
      voxel     cloud_export.voxel_downsample (mean, r g b conf attributes) on a synthetic 32-view scene
                (32 x 518^2 points uniform in the unit cube) at edges giving about 1, 10 and 100 members per
                voxel, against torch.unique(keys, return_inverse, return_counts) + an fp64 index_add_.
      eval      cloud_eval.evaluate_reconstruction with voxel= against the same call without it, 2^20
                predicted against 2^20 ground-truth points (the size at which brute force still finishes)."""
    from sailrecon_amd.utils.cloud_eval import evaluate_reconstruction
    from sailrecon_amd.utils.cloud_export import voxel_downsample
    g = torch.Generator(device=DEV).manual_seed(0)

    def alternate(fns, label, note=lambda name, best: ""):
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(runs):
            for name, fn in fns.items():
                times[name].append(timeit(fn, reps=1, warm=0))
        for name, ms in times.items():
            print(f"{label} {name:24s}: " + " ".join(f"{t:9.3f}" for t in ms) + f" ms  best {min(ms):9.3f} ms" +
                  note(name, min(ms)), flush=True)
        return {k: min(v) for k, v in times.items()}

    for views in (5, 32):
        n = views * 518 * 518
        for bits in (31, 64):
            # non-negative int64, so that torch's signed order is the unsigned one; under 64 bits all eight digits vary
            keys = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g, dtype=torch.int64)
            keys = keys * 2 + torch.randint(0, 2, (n,), device=DEV, generator=g, dtype=torch.int64) if bits == 64 else \
                keys & (2 ** 31 - 1)
            passes = (bits + 7) // 8

            def ours():
                sk, perm = ops.sort_pairs(keys, key_bits=bits)
                return perm[:1].cpu()

            def theirs():
                sk, perm = torch.sort(keys, stable=True)
                return perm[:1].cpu()

            best = alternate({"sr_sort_pairs": ours, "torch.sort(stable)": theirs}, f"sort {views} x 518^2, {bits} bits",
                             lambda name, ms: (f"  {passes} passes, {32 * n * passes / (ms * 1e-3) / 1e9:7.1f} GB/s moved "
                                               "(HBM streaming: 6300)") if name == "sr_sort_pairs" else "")
            same = bool(torch.equal(ops.sort_pairs(keys, key_bits=bits)[1].long(), torch.sort(keys, stable=True)[1]))
            print(f"sort {views} x 518^2, {bits} bits: sr_sort_pairs is {best['torch.sort(stable)'] / best['sr_sort_pairs']:.2f} x "
                  f"torch.sort's speed; same permutation: {same}  [{ops.last_kernel()}]", flush=True)
            del keys
    n = 32 * 518 * 518
    p = torch.rand(n, 3, device=DEV, generator=g)
    attrs = torch.rand(n, 4, device=DEV, generator=g)
    for members in (1, 10, 100):
        v = (members / n) ** (1 / 3)

        def ours():
            return voxel_downsample(p, v, attrs=attrs, axis_bits=21)["n_voxels"]

        def theirs():
            f = torch.floor(p.double() / v).long() + 2 ** 20
            keys = (f[:, 2] << 42) | (f[:, 1] << 21) | f[:, 0]
            uk, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
            acc = torch.zeros(uk.numel(), 7, device=DEV, dtype=torch.float64)
            acc.index_add_(0, inv, torch.cat([p, attrs], dim=1).double())
            out = (acc / cnt[:, None]).float()
            return int(out.shape[0]), out[:1].cpu()

        best = alternate({"voxel_downsample": ours, "unique + index_add_": theirs}, f"voxel 32 x 518^2, ~{members} per voxel")
        print(f"voxel 32 x 518^2, edge {v:.5f}: {ours()} voxels (statement {theirs()[0]}); voxel_downsample is "
              f"{best['unique + index_add_'] / best['voxel_downsample']:.2f} x the statement's speed  [{ops.last_kernel()}]",
              flush=True)
    del p, attrs
    m = 1 << 20
    gt = torch.rand(m, 3, device=DEV, generator=g)
    pred = [{"points": gt[k::4] + 0.002 * torch.randn(m // 4, 3, device=DEV, generator=g)} for k in range(4)]
    res = {}

    def scored(vx):
        res[vx] = evaluate_reconstruction(pred, gt, key="points", voxel=vx)
        return res[vx]

    best = alternate({"voxel=0.02": lambda: scored(0.02), "voxel=None": lambda: scored(None)}, "eval 2^20 x 2^20")
    print(f"eval 2^20 x 2^20: voxel=0.02 scores {res[0.02]['n_pred_voxels']} x {res[0.02]['n_gt_voxels']} voxels, chamfer "
          f"{res[0.02]['chamfer']:.5f} against {res[None]['chamfer']:.5f} unreduced, {best['voxel=None'] / best['voxel=0.02']:.1f} x "
          "the speed", flush=True)


def voxel_once():
    """One sort and one downsampling at 32 x 518^2, for a kernel trace of their own."""
    from sailrecon_amd.utils.cloud_export import voxel_downsample
    g = torch.Generator(device=DEV).manual_seed(0)
    n = 32 * 518 * 518
    p = torch.rand(n, 3, device=DEV, generator=g)
    attrs = torch.rand(n, 4, device=DEV, generator=g)
    for members in (1, 10, 100):
        print(members, voxel_downsample(p, (members / n) ** (1 / 3), attrs=attrs)["n_voxels"], flush=True)


def _sparsify_inputs(views):
    """A heteroscedastic error with a half-informative confidence, [views, 518^2] fp32."""
    g = torch.Generator(device=DEV).manual_seed(0)
    sigma = torch.exp(0.75 * torch.randn(views, 518 * 518, device=DEV, generator=g))
    err = (torch.randn(views, 518 * 518, device=DEV, generator=g) * sigma).abs()
    conf = 1.0 / sigma + torch.rand(views, 518 * 518, device=DEV, generator=g)
    return err, conf


def sparsify(runs=3):
    """The sparsification sums (sr_sparsify) against their torch statement, in alternation in one process,
    ``runs`` timed runs each after one warm-up, HIP events, each side ending in its D2H copy of the
    [n_groups, 2, K] bin sums.  5 and 32 x 518^2 elements, K = 100, one group per view and one for the scene.
    The statement: the same 64-bit keys, torch.sort(stable=True) of each order, the errors gathered through the
    permutation, an fp64 cumsum and reads at the bin boundaries."""
    K = 100

    def alternate(fns, label):
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(runs):
            for name, fn in fns.items():
                times[name].append(timeit(fn, reps=1, warm=0))
        for name, ms in times.items():
            print(f"{label} {name:24s}: " + " ".join(f"{t:9.3f}" for t in ms) + f" ms  best {min(ms):9.3f} ms", flush=True)
        return {k: min(v) for k, v in times.items()}

    def key32(x):
        b = x.view(torch.int32).long() & 0xFFFFFFFF
        return b ^ torch.where(b >> 31 != 0, 0xFFFFFFFF, 0x80000000)

    for views in (5, 32):
        err, conf = _sparsify_inputs(views)
        for scope in ("view", "scene"):
            G = views if scope == "view" else 1
            grp = None if scope == "view" else torch.zeros(views, device=DEV, dtype=torch.int32)
            gid = (torch.arange(views, device=DEV) if scope == "view" else torch.zeros(views, device=DEV, dtype=torch.int64))
            gid = gid[:, None].expand(views, 518 * 518).reshape(-1)
            bin_sum = torch.empty(G, 2, K, device=DEV, dtype=torch.float64)
            cut = torch.empty(G, K, device=DEV, dtype=torch.float32)
            count = torch.empty(G, 2, device=DEV, dtype=torch.int32)

            def ours():
                ops.sparsify(err, conf, K, bin_sum, group=grp, n_groups=G, cut=cut, count=count)
                return bin_sum.cpu()

            def theirs():
                e, c = err.reshape(-1), conf.reshape(-1)
                ok = torch.isfinite(e) & torch.isfinite(c)
                kc = torch.where(ok, (gid << 32) | key32(c), G << 32)
                ko = torch.where(ok, (gid << 32) | (key32(e) ^ 0xFFFFFFFF), G << 32)
                cnt = torch.bincount(gid[ok], minlength=G)
                start = torch.cumsum(cnt, 0) - cnt
                b = start[:, None] + (torch.arange(K + 1, device=DEV)[None] * cnt[:, None]) // K
                sums = []
                for keys in (kc, ko):
                    perm = torch.sort(keys, stable=True)[1]
                    cs = torch.cat([torch.zeros(1, device=DEV, dtype=torch.float64), torch.cumsum(e[perm].double(), 0)])
                    sums.append(cs[b[:, 1:]] - cs[b[:, :-1]])
                return torch.stack(sums, 1).cpu()

            label = f"sparsify {views} x 518^2, K {K}, scope {scope}"
            best = alternate({"sr_sparsify": ours, "sort + cumsum": theirs}, label)
            a, t = ours(), theirs()
            print(f"{label}: sr_sparsify is {best['sort + cumsum'] / best['sr_sparsify']:.2f} x the statement's speed; "
                  f"largest relative difference of a bin sum {float(((a - t).abs() / t.abs()).max()):.2e}; workspace "
                  f"{ops.sparsify_workspace_bytes(views, 518 * 518, G, K) / 2 ** 20:.0f} MiB  [{ops.last_kernel()}]", flush=True)
        del err, conf


def sparsify_once(scopes=("view", "scene")):
    """One sr_sparsify at 32 x 518^2, K = 100, per scope, for a kernel trace of its own."""
    from sailrecon_amd.utils.conf_eval import sparsification_curves
    err, conf = _sparsify_inputs(32)
    for scope in scopes:
        r = sparsification_curves(err, conf, n_steps=100, group=scope)
        print(scope, r["ause"][:2], r["aurg"][:2], flush=True)


def sparsify_once_view():
    sparsify_once(("view",))


def sparsify_once_scene():
    sparsify_once(("scene",))


def _render_scene(views=32, size=518):
    """A synthetic scene on the device: ``views`` cameras side by side in front of a wavy wall, every view's
    depth map unprojected (sr_unproject_depth_f32) into one raster-ordered cloud with r, g, b, conf attributes."""
    from sailrecon_amd.utils.geometry import unproject_depth_points
    g = torch.Generator(device=DEV).manual_seed(0)
    E = torch.zeros(views, 3, 4, device=DEV)
    E[:, :, :3] = torch.eye(3, device=DEV)
    E[:, :2, 3] = torch.rand(views, 2, device=DEV, generator=g) - 0.5
    K = torch.zeros(views, 3, 3, device=DEV)
    K[:, 0, 0] = K[:, 1, 1] = 0.9 * size
    K[:, 0, 2] = K[:, 1, 2] = (size - 1) / 2
    K[:, 2, 2] = 1
    yy, xx = torch.meshgrid(torch.arange(size, device=DEV), torch.arange(size, device=DEV), indexing="ij")
    depth = 3 + 0.3 * torch.sin(xx / 40.0)[None] * torch.cos(yy / 55.0)[None] + 0.05 * torch.rand(views, size, size, device=DEV, generator=g)
    pts = unproject_depth_points(depth, E, K).reshape(-1, 3)
    attrs = torch.rand(pts.shape[0], 4, device=DEV, generator=g)
    return pts, attrs, E, K


def _render_statement(p, E, K, H, W, radius):
    """The torch statement of one rendering: per view an fp64 projection and scatter_reduce_("amin") on int64
    keys (depth bits << 32 | index).  Returns the key images [V, H W]."""
    n = p.shape[0]
    idx = torch.arange(n, device=DEV, dtype=torch.int64)
    pd = p.double()
    out = torch.full((E.shape[0], H * W), 2 ** 63 - 1, device=DEV, dtype=torch.int64)
    for v in range(E.shape[0]):
        e, k = E[v].double(), K[v].double()
        c = [((e[r, 0] * pd[:, 0] + e[r, 1] * pd[:, 1]) + e[r, 2] * pd[:, 2]) + e[r, 3] for r in range(3)]
        ix = torch.floor(k[0, 0] * (c[0] / c[2]) + k[0, 2] + 0.5)
        iy = torch.floor(k[1, 1] * (c[1] / c[2]) + k[1, 2] + 0.5)
        ok = (c[2] >= 1e-6) & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        key = (c[2].float().view(torch.int32).long() << 32) | idx
        ixl, iyl = ix.long(), iy.long()
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                x, y = ixl + dx, iyl + dy
                m = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                out[v].scatter_reduce_(0, (y * W + x)[m], key[m], "amin")
    return out


def render(runs=3):
    """The point-cloud renderer (sr_cloud_render) against its torch statement, in alternation in one process,
    ``runs`` timed runs each after one warm-up, HIP events, each side ending in a D2H copy.  A synthetic 32-view
    scene's own cloud (32 x 518^2 points in raster order, r g b conf attributes) into its 32 cameras at 518^2,
    radius 0 and 1; then the same cloud after voxel downsampling.  The statement: per view an fp64 projection and
    scatter_reduce_("amin") on int64 keys, depth and index only.  Atomics per second: drawn points times the
    footprint over the whole call's time, a lower bound of the draw kernel's own rate (the kernel trace has it)."""
    from sailrecon_amd.utils.cloud_export import voxel_downsample
    size, views = 518, 32
    pts, attrs, E, K = _render_scene(views, size)
    vox = voxel_downsample(pts, 0.01, attrs=attrs)
    shapes = {"scene": (pts, attrs), f"voxel 0.01 ({vox['n_voxels']} points)": (vox["points"].contiguous(), vox["attrs"].contiguous())}
    depth = torch.empty(views, size, size, device=DEV)
    index = torch.empty(views, size, size, device=DEV, dtype=torch.int32)
    out_a = torch.empty(views, size, size, 4, device=DEV)
    counts = torch.empty(views, 4, device=DEV, dtype=torch.int32)
    for label, (p, a) in shapes.items():
        n = p.shape[0]
        for radius in (0, 1):
            def ours():
                ops.cloud_render(p, E, K, (size, size), attr=a, radius=radius, depth=depth, index=index, out_attr=out_a,
                                 counts=counts)
                return counts.cpu()

            def theirs():
                return _render_statement(p, E, K, size, size, radius)[:, :1].cpu()

            times = {"sr_cloud_render": [], "projection + scatter amin": []}
            fns = {"sr_cloud_render": ours, "projection + scatter amin": theirs}
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(runs):
                for name, fn in fns.items():
                    times[name].append(timeit(fn, reps=1, warm=0))
            tag = f"render {label}, n {n}, V {views}, {size}^2, radius {radius}"
            for name, ms in times.items():
                print(f"{tag} {name:26s}: " + " ".join(f"{t:9.3f}" for t in ms) + f" ms  best {min(ms):9.3f} ms", flush=True)
            c = ours().long() & 0xFFFFFFFF
            keys = _render_statement(p, E, K, size, size, radius)
            want_idx = torch.where(keys == 2 ** 63 - 1, -1, keys & 0xFFFFFFFF).int().reshape(views, size, size)
            best, ref = min(times["sr_cloud_render"]), min(times["projection + scatter amin"])
            atomics = int(c[:, 1].sum()) * (2 * radius + 1) ** 2
            print(f"{tag}: sr_cloud_render is {ref / best:.2f} x the statement's speed; same index image: "
                  f"{bool(torch.equal(index, want_idx))}; drawn {int(c[:, 1].sum())}, covered {int(c[:, 0].sum())} of "
                  f"{views * size * size} pixels; >= {atomics / (best * 1e-3) / 1e9:.1f} G atomics/s over the whole call; "
                  f"workspace {ops.cloud_render_workspace_bytes(views, size, size) / 2 ** 20:.0f} MiB, the statement's "
                  f"keys at once would take {8 * views * n / 2 ** 20:.0f} MiB  [{ops.last_kernel()}]", flush=True)


def render_once():
    """One sr_cloud_render of the 32 x 518^2 scene into its 32 cameras per radius, for a kernel trace of its own."""
    from sailrecon_amd.utils.cloud_render import render_cloud
    pts, attrs, E, K = _render_scene()
    for radius in (0, 1):
        r = render_cloud(pts, E, K, (518, 518), attrs=attrs, radius=radius)
        print(radius, r["coverage"][0], flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["attn", "gemm", "ln"]
    for w in which:
        globals()[w]()
