"""Block-level training engine: forward with saved activations ("tape") and backward, on the
HIP kernels (the backward of block.py:86-112 / attention.py:70-122 /
mlp.py:34-40 / layer_scale.py:22-23 that ``loss.backward()`` runs in train_imc.py:404).

Forward (run_block_train) is run_block's kernel sequence with the backward's inputs kept:

    LN1 -> xn1 (+ x0 = x, the same pass)   GEMM qkv -> qkv  (+ aux: pre-norm q|k|v = raw)
    attention(qkv) -> o (+ lse)   GEMM proj + gamma1 + residual (in place on x)
    LN2 -> xn2 (+ x1 = x)   GEMM fc1 + GELU -> h (+ aux: pre-activation u)
    GEMM fc2 + gamma2 + residual

Backward (block_bwd) takes dx (fp32 residual grad of the block output, updated in place to the
grad of its input) and dxb (its bf16 copy, the GEMM operand), and accumulates every parameter
grad into the parameters' ``.grad`` tensors:

    dU  = GELU'(u) * (dxb . (g2 W2))        dgrad GEMM, SR_EPI_GELU_BWD (W^T pack with g2 folded in)
    dW2 = g2 * dxb^T h;  dg2 = <W2, dxb^T h> + b2 * colsum(dx);  db2 = g2 * colsum(dx)
    dxn2 = dU . W1  (fp32);  dW1 = dU^T xn2;  db1 = colsum(dU)
    dx  += LN2'(dxn2; x1)  (+ dxb refresh)   -> the same for proj (o), attention, qk-norm+RoPE, qkv, LN1

Weights for the dgrad GEMMs are packed transposed once per optimizer step (BwdPack).  fp32
blocks (the camera trunk, autocast off) use the same sequence with fp32 GEMMs, the small-row
weight-gradient kernel and the masked fp32 attention backward.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional

import torch

from .. import _lib, ops, runtime

Tensor = torch.Tensor


@dataclass
class BlockTape:
    x0: Tensor           # fp32 [R, C]  block input
    x1: Tensor           # fp32 [R, C]  after the attention residual
    xn1: Tensor          # dtype [R, C]
    raw: Tensor          # dtype [R, 3C] pre-norm q|k|v (is qkv when there is no qk-norm / RoPE)
    qkv: Tensor          # dtype [R, 3C]
    o: Tensor            # dtype [R, C]
    lse: Optional[Tensor]  # fp32 [batch*heads*lq] (bf16 attention)
    xn2: Tensor          # dtype [R, C]
    u: Tensor            # dtype [R, H] fc1 pre-activation
    h: Tensor            # dtype [R, H]


TAIL_ROWS = 64
# SR_TRAIN_PAIR_WGRAD (default 1; 0 for the A/B): block_bwd_multi's two items share weight-grad
# launches (ops.gemm_wgrad_pair) where ops.wgrad_pair_splits says it pays
_PAIR_WGRAD = os.environ.get("SR_TRAIN_PAIR_WGRAD", "1") != "0"
# SR_TRAIN_BIAS_COLSUM (bits, default 3; 0 for the A/B): bf16 bias grads from the producing pass
# instead of a column sum that re-reads the gradient: 1 = fc1's from the GELU_BWD dgrad epilogue,
# 2 = qkv's from sr_qk_bwd
_BIAS_COLSUM = int(os.environ.get("SR_TRAIN_BIAS_COLSUM", "3"))
GELU_COLSUM = bool(_BIAS_COLSUM & 1)
QK_COLSUM = bool(_BIAS_COLSUM & 2)


def alloc_tape(rows: int, dim: int, hidden: int, dtype: torch.dtype, device, lse_numel: int,
               separate_raw: bool) -> BlockTape:
    e = lambda r, c, dt=dtype: torch.empty(r, c, device=device, dtype=dt)  # noqa: E731
    # q|k|v with TAIL_ROWS zeroed rows after it: every key segment's tail is readable, so the
    # forward attention may take the hand-scheduled sweep's ragged variant (ops.attention
    # tail_readable; the C4 global block's 21,984 keys are 343.5 tiles)
    qkv = torch.zeros(rows + TAIL_ROWS, 3 * dim, device=device, dtype=dtype)[:rows]
    return BlockTape(x0=e(rows, dim, torch.float32), x1=e(rows, dim, torch.float32), xn1=e(rows, dim),
                     raw=e(rows, 3 * dim) if separate_raw else qkv, qkv=qkv, o=e(rows, dim),
                     lse=torch.empty(lse_numel, device=device, dtype=torch.float32) if lse_numel else None,
                     xn2=e(rows, dim), u=e(rows, hidden), h=e(rows, hidden))


def _gemm_stage(probs, epi: int, tag: str) -> None:
    """One GEMM stage of every item (dicts: a, w, out and ops.gemm's keywords): ONE grouped launch
    (sr_gemm_group) for several eligible problems, else ops.gemm each.  One problem never groups:
    ops.gemm picks its kernel and the split-K of few rows (the fp32 camera trunk)."""
    if len(probs) > 1 and ops.gemm_group_eligible(probs):
        ops.gemm_group(probs, epi, tag=tag)
        return
    for q in probs:
        ops.gemm(q["a"], q["w"], q["out"], epi, tag=tag, **{k: v for k, v in q.items() if k not in ("a", "w", "out")})


def _one_by_one(items, same_epi: bool) -> bool:
    """Whether several items cannot share stages: not all bf16, (C, hidden) differ or (forward) only
    some have a qk-norm / RoPE epilogue."""
    return len(items) > 1 and (
        not all(it["tape"].xn1.dtype == torch.bfloat16 for it in items) or
        len({(it["tape"].xn1.shape[1], it["tape"].u.shape[1]) for it in items}) != 1 or
        (same_epi and len({it["qkv_epi"] is None for it in items}) != 1))


def run_block_train(pb: runtime.PackedBlock, x: Tensor, r0: int, r1: int, tape: BlockTape,
                    attend: Callable[[Tensor, Tensor, Optional[Tensor]], None], qkv_epi: Optional[dict]) -> None:
    """x[r0:r1] <- Block(x[r0:r1]) keeping the backward's inputs in ``tape``."""
    run_block_train_multi([dict(pb=pb, x=x, r0=r0, r1=r1, tape=tape, attend=attend, qkv_epi=qkv_epi)])


def run_block_train_multi(items) -> None:
    """run_block_train for several independent block applications of equal width at once (the
    layer's reloc and global blocks: different weights, disjoint rows of x, the reloc block's
    anchor K|V already projected): stage by stage, each GEMM of all items as ONE grouped launch
    (sr_gemm_group) whose last partial round the items share.  At C4 each item's N = 1,024 GEMMs
    (proj, fc2) are 344 tiles of 256^2, which sr_gemm alone runs on the 128^2 kernel; grouped they
    run on the 256^2 kernel, whose results differ from it by fp32 accumulation order only
    (gemm_resid 41.7 -> 38.9 ms per C4 step, profiles/r05_j29_*).  fc1 stays one launch per item.
    ``items``: dicts of run_block_train's arguments (pb, x, r0, r1, tape, attend, qkv_epi), not
    modified; their attentions run in list order.  Items of mixed dtype, width or qkv epilogue run
    one after another."""
    if _one_by_one(items, same_epi=True):
        for it in items:
            run_block_train_multi([it])
        return
    its = [SimpleNamespace(**it, xs=it["x"][it["r0"]:it["r1"]]) for it in items]
    for s in its:
        ops.layernorm(s.xs, s.pb.ln1_w, s.pb.ln1_b, s.pb.eps, s.tape.xn1, x_copy=s.tape.x0)  # x0 = x in the same pass
    if its[0].qkv_epi is None:
        _gemm_stage([dict(a=s.tape.xn1, w=s.pb.w_qkv, out=s.tape.qkv, bias=s.pb.b_qkv) for s in its],
                    _lib.SR_EPI_BIAS, "gemm")
    else:
        _gemm_stage([dict(a=s.tape.xn1, w=s.pb.w_qkv, out=s.tape.qkv, bias=s.pb.b_qkv, qkv=s.qkv_epi, aux=s.tape.raw)
                     for s in its], _lib.SR_EPI_QKV, "gemm")
    for s in its:
        s.attend(s.tape.qkv, s.tape.o, s.tape.lse)
    _gemm_stage([dict(a=s.tape.o, w=s.pb.w_proj, out=s.xs, bias=s.pb.b_proj, gamma=s.pb.g1) for s in its],
                _lib.SR_EPI_BIAS_RESID, "gemm")
    for s in its:
        ops.layernorm(s.xs, s.pb.ln2_w, s.pb.ln2_b, s.pb.eps, s.tape.xn2, x_copy=s.tape.x1)  # x1 = x likewise
    for s in its:  # fc1 apart: sr_gemm's tail split beats the group here (35.5 vs 34.9 ms/step, j29)
        ops.gemm(s.tape.xn2, s.pb.w_fc1, s.tape.h, _lib.SR_EPI_BIAS_GELU, bias=s.pb.b_fc1, aux=s.tape.u, tag="gemm")
    _gemm_stage([dict(a=s.tape.h, w=s.pb.w_fc2, out=s.xs, bias=s.pb.b_fc2, gamma=s.pb.g2) for s in its],
                _lib.SR_EPI_BIAS_RESID, "gemm")


# ----------------------------------------------------------------------------- parameters
@dataclass
class BlockGrads:
    """The ``.grad`` tensors of one Block's parameters (fp32, accumulated into)."""
    ln1_w: Tensor
    ln1_b: Tensor
    w_qkv: Tensor
    b_qkv: Optional[Tensor]
    qkn: Optional[Tensor]  # [4, head_dim] = q_norm.weight | q_norm.bias | k_norm.weight | k_norm.bias
    w_proj: Tensor
    b_proj: Optional[Tensor]
    g1: Optional[Tensor]
    ln2_w: Tensor
    ln2_b: Tensor
    w_fc1: Tensor
    b_fc1: Optional[Tensor]
    w_fc2: Tensor
    b_fc2: Optional[Tensor]
    g2: Optional[Tensor]


def _grad(p) -> Optional[Tensor]:
    if p is None:
        return None
    if p.grad is None:
        raise RuntimeError("training engine: parameter grads must be allocated first (train.params.GradBuffer)")
    return p.grad


def block_grads(blk) -> BlockGrads:
    a = blk.attn
    qkn = None
    if getattr(a, "qk_norm", False):
        parts = [a.q_norm.weight.grad, a.q_norm.bias.grad, a.k_norm.weight.grad, a.k_norm.bias.grad]
        if any(t is None for t in parts):
            raise RuntimeError("training engine: qk-norm grads not allocated")
        d = parts[0].numel()
        base = parts[0].data_ptr()
        if any(t.data_ptr() != base + 4 * d * i for i, t in enumerate(parts)):
            raise RuntimeError("training engine: q_norm / k_norm grads must be one contiguous [4, head_dim] block")
        qkn = parts[0].as_strided((4, d), (d, 1))
    ls = lambda m: _grad(getattr(m, "gamma", None))  # noqa: E731
    return BlockGrads(ln1_w=_grad(blk.norm1.weight), ln1_b=_grad(blk.norm1.bias), w_qkv=_grad(a.qkv.weight),
                      b_qkv=_grad(a.qkv.bias), qkn=qkn, w_proj=_grad(a.proj.weight), b_proj=_grad(a.proj.bias),
                      g1=ls(blk.ls1), ln2_w=_grad(blk.norm2.weight), ln2_b=_grad(blk.norm2.bias),
                      w_fc1=_grad(blk.mlp.fc1.weight), b_fc1=_grad(blk.mlp.fc1.bias), w_fc2=_grad(blk.mlp.fc2.weight),
                      b_fc2=_grad(blk.mlp.fc2.bias), g2=ls(blk.ls2))


@dataclass
class BwdPack:
    """Per-optimizer-step transposed weights of one Block for the dgrad GEMMs (dtype), with the
    LayerScale gammas folded into proj / fc2; fp32 masters for the gamma-grad row dots."""
    wt_qkv: Tensor   # [C, 3C]  W_qkv^T
    wt_proj: Tensor  # [C, C]   (g1 * W_proj)^T
    wt_fc1: Tensor   # [C, H]   W_fc1^T
    wt_fc2: Tensor   # [H, C]   (g2 * W_fc2)^T
    w_proj: Tensor   # fp32 masters
    w_fc2: Tensor
    b_proj: Optional[Tensor]
    b_fc2: Optional[Tensor]


def pack_bwd(blk, pb: runtime.PackedBlock, dtype: torch.dtype, into: Optional[BwdPack] = None) -> BwdPack:
    a = blk.attn
    f = lambda t: t.detach()  # noqa: E731  (fp32 contiguous parameters: no copy)
    wq, wp, w1, w2 = f(a.qkv.weight), f(a.proj.weight), f(blk.mlp.fc1.weight), f(blk.mlp.fc2.weight)
    dev = wq.device
    if into is None:
        e = lambda r, c: torch.empty(r, c, device=dev, dtype=dtype)  # noqa: E731
        into = BwdPack(wt_qkv=e(wq.shape[1], wq.shape[0]), wt_proj=e(wp.shape[1], wp.shape[0]),
                       wt_fc1=e(w1.shape[1], w1.shape[0]), wt_fc2=e(w2.shape[1], w2.shape[0]), w_proj=wp, w_fc2=w2,
                       b_proj=pb.b_proj, b_fc2=pb.b_fc2)
    ops.transpose(wq, into.wt_qkv)
    ops.transpose(wp, into.wt_proj, rowscale=pb.g1)
    ops.transpose(w1, into.wt_fc1)
    ops.transpose(w2, into.wt_fc2, rowscale=pb.g2)
    return into


def refresh_items_bf16(blk, pb: runtime.PackedBlock, into: BwdPack) -> list:
    """The block's four weight_refresh items: the bf16 forward weights of the packed block (casts in
    place) and the transposed dgrad packs of pack_bwd (LayerScale gammas folded into proj / fc2)."""
    a = blk.attn
    f = lambda t: t.detach()  # noqa: E731
    return [(f(a.qkv.weight), pb.w_qkv, into.wt_qkv, None),
            (f(a.proj.weight), pb.w_proj, into.wt_proj, pb.g1),
            (f(blk.mlp.fc1.weight), pb.w_fc1, into.wt_fc1, None),
            (f(blk.mlp.fc2.weight), pb.w_fc2, into.wt_fc2, pb.g2)]


def refresh_block_bf16(blk, pb: runtime.PackedBlock, into: BwdPack) -> None:
    """After an optimizer step, one launch per block (sr_weight_refresh_bf16), each fp32 weight read once."""
    ops.weight_refresh(refresh_items_bf16(blk, pb, into))


class BwdScratch(runtime.Workspace):
    """Grow-only backward scratch shared by every block of one stream."""


def _resid_wants_sum(bias: Optional[Tensor], g_bias: Optional[Tensor], g_gamma: Optional[Tensor]) -> bool:
    return g_bias is not None or (g_gamma is not None and bias is not None)


def _resid_param_grads(dx: Tensor, bias: Optional[Tensor], gamma: Optional[Tensor], g_bias: Optional[Tensor],
                       g_gamma: Optional[Tensor], tmp: Tensor, summed: bool = False) -> None:
    """Bias and LayerScale-gamma grads of ``x += gamma * (a W^T + b)`` from colsum(dx):
    db += gamma * s, dgamma += b * s (the <W, G> part comes from the wgrad row dots).
    ``summed``: tmp already holds colsum(dx) (layernorm_bwd's dx_sum)."""
    if not _resid_wants_sum(bias, g_bias, g_gamma):
        return
    if g_bias is not None and gamma is None:
        raise RuntimeError("bias grad without gamma")
    pairs = ([(g_bias, gamma)] if g_bias is not None else []) + \
        ([(g_gamma, bias)] if g_gamma is not None and bias is not None else [])
    if not summed:  # the column sum's final launch applies the products (no scratch row, no extra launch)
        ops.colsum_fma(dx, pairs)
    elif len(pairs) == 2:
        ops.vec_fma(pairs[0][0], pairs[0][1], tmp, out2=pairs[1][0], a2=pairs[1][1])
    else:
        ops.vec_fma(pairs[0][0], pairs[0][1], tmp)


def _wgrad_stage(args, bf: bool, tag: str) -> None:
    """One weight-gradient stage of every item: (item tag, dy, x, dw, db, rowscale, wdot, rowdot)
    each.  bf16: sr_gemm_wgrad (+ db from a column sum of dy); two items of one weight shape share
    ONE launch (sr_gemm_wgrad_pair) where ops.wgrad_pair_splits says it pays.  fp32: the small-row
    kernel with db folded in."""
    if not bf:
        for _, dy, x, dw, db, rowscale, wdot, rowdot in args:
            ops.wgrad_small(dy, x, dw, db=db, accumulate=True, rowscale=rowscale, wdot=wdot, rowdot=rowdot)
        return
    sp = None
    if _PAIR_WGRAD and len(args) == 2 and args[0][3].shape == args[1][3].shape:
        sp = ops.wgrad_pair_splits(args[0][1].shape[0], args[1][1].shape[0], *args[0][3].shape)
    if sp is not None:
        ops.gemm_wgrad_pair([dict(dy=a[1], x=a[2], dw=a[3], accumulate=True, rowscale=a[5], wdot=a[6], rowdot=a[7])
                             for a in args], sp, tag=tag + ".wgrad")
    for item_tag, dy, x, dw, db, rowscale, wdot, rowdot in args:
        if sp is None:
            ops.gemm_wgrad(dy, x, dw, accumulate=True, rowscale=rowscale, wdot=wdot, rowdot=rowdot,
                           tag=item_tag + ".wgrad")
        if db is not None:
            ops.colsum(dy, db, accumulate=True)


def block_bwd(pb: runtime.PackedBlock, bp: BwdPack, g: BlockGrads, tape: BlockTape, dx: Tensor,
              dxb: Optional[Tensor], attend_bwd: Callable[[BlockTape, Tensor, Tensor], None],
              qkv_epi: Optional[dict], sc: BwdScratch, tag: str = "bwd") -> None:
    """dx (fp32 [R, C], the grad of the block's output) <- grad of its input, in place; dxb
    (bf16 copy of dx, bf16 blocks) refreshed alongside; parameter grads accumulated.
    ``attend_bwd(tape, dO, dqkv)`` writes fp32 dq|dk|dv into dqkv [R, 3C] (and any shared-segment
    grads elsewhere)."""
    block_bwd_multi([dict(pb=pb, bp=bp, g=g, tape=tape, dx=dx, dxb=dxb, attend_bwd=attend_bwd, qkv_epi=qkv_epi,
                          sc=sc, tag=tag)])


def block_bwd_multi(items, tag: str = "pair") -> None:
    """block_bwd for several independent block applications of equal width at once (the layer's
    reloc and global blocks: different weights, disjoint rows): stage by stage, each stage's
    dgrad GEMMs of all items as ONE grouped launch (sr_gemm_group), whose last partial round of
    workgroups the items share (at C4 each item's N = 1,024 dgrads are 344 tiles of 256^2, 1.3
    rounds alone).  ``items``: dicts of block_bwd's arguments (pb, bp, g, tape, dx, dxb,
    attend_bwd, qkv_epi, sc, tag), not modified; their attention backwards run in list order.
    A grouped product runs on the 256^2 kernel with sr_gemm's per-tile order; where sr_gemm
    alone would have picked the 128^2 kernel the results differ by fp32 accumulation order.
    Timer tags: ``tag`` on what the items share (dgrads, paired weight grads), the item's own on its
    other weight grads, and on everything of an item that runs alone (mixed dtypes or widths)."""
    if _one_by_one(items, same_epi=False):
        for it in items:
            block_bwd_multi([it])
        return
    if len(items) == 1:
        tag = items[0]["tag"]
    C, Hd = items[0]["dx"].shape[1], items[0]["tape"].u.shape[1]
    dev, dt = items[0]["dx"].device, items[0]["tape"].xn1.dtype
    bf = dt == torch.bfloat16
    its = [SimpleNamespace(**it) for it in items]
    for s in its:
        s.R = s.dx.shape[0]
        s.a = s.dxb if bf else s.dx   # GEMM operand view of dx
        s.tmp = s.sc.get("colsum_tmp", 1, max(C, Hd, 3 * C), torch.float32, dev)[0]
        s.dU = s.sc.get("dU", s.R, Hd, dt, dev)
        # bf16: fc1's bias grad from the GELU_BWD epilogue's per-64-row column sums (no re-read of dU)
        s.csU = (s.sc.get("dU_colsum", ops.colsum_blocks(s.R), Hd, torch.float32, dev)
                 if bf and s.g.b_fc1 is not None and GELU_COLSUM else None)
        s.dxn = s.sc.get("dxn", s.R, C, torch.float32, dev)
        s.dO = s.sc.get("dO", s.R, C, dt, dev)
    # ---- MLP: x2 = x1 + g2 * fc2(GELU(fc1(LN2(x1))))
    _gemm_stage([dict(a=s.a, w=s.bp.wt_fc2, out=s.dU, aux=s.tape.u, colsum=s.csU) for s in its],
                _lib.SR_EPI_GELU_BWD, tag + ".dgrad")
    _wgrad_stage([(s.tag, s.a, s.tape.h, s.g.w_fc2, None, s.pb.g2, s.bp.w_fc2 if s.g.g2 is not None else None, s.g.g2)
                  for s in its], bf, tag)
    for s in its:
        _resid_param_grads(s.dx, s.bp.b_fc2, s.pb.g2, s.g.b_fc2, s.g.g2, s.tmp[:C])
    _gemm_stage([dict(a=s.dU, w=s.bp.wt_fc1, out=s.dxn) for s in its], _lib.SR_EPI_F32, tag + ".dgrad")
    _wgrad_stage([(s.tag, s.dU, s.tape.xn2, s.g.w_fc1, None if s.csU is not None else s.g.b_fc1, None, None, None)
                  for s in its], bf, tag)
    for s in its:
        if s.csU is not None:
            ops.colsum(s.csU, s.g.b_fc1, accumulate=True)
    for s in its:  # (LN2's backward also sums the updated dx over the rows: proj's bias / gamma grads below)
        s.fused_sum = s.g.ln2_w is not None and C <= 2048 and _resid_wants_sum(s.bp.b_proj, s.g.b_proj, s.g.g1)
        ops.layernorm_bwd(s.tape.x1, s.dxn, s.pb.ln2_w, s.pb.eps, s.dx, dxb=s.dxb, dw=s.g.ln2_w, db=s.g.ln2_b,
                          dx_sum=s.tmp[:C] if s.fused_sum else None)
    # ---- attention: x1 = x0 + g1 * proj(attn(qk(qkv(LN1(x0)))))
    _gemm_stage([dict(a=s.a, w=s.bp.wt_proj, out=s.dO) for s in its], _lib.SR_EPI_BIAS, tag + ".dgrad")
    _wgrad_stage([(s.tag, s.a, s.tape.o, s.g.w_proj, None, s.pb.g1, s.bp.w_proj if s.g.g1 is not None else None, s.g.g1)
                  for s in its], bf, tag)
    for s in its:
        _resid_param_grads(s.dx, s.bp.b_proj, s.pb.g1, s.g.b_proj, s.g.g1, s.tmp[:C], summed=s.fused_sum)
    for s in its:
        s.draw = dqkv = s.sc.get("dqkv", s.R, 3 * C, torch.float32, dev)
        s.attend_bwd(s.tape, s.dO, dqkv)
        if bf:  # (+ the qkv bias grad from the same pass: no bf16 column sum of draw afterwards)
            s.draw = s.sc.get("draw", s.R, 3 * C, dt, dev)
            ops.qk_bwd(s.tape.raw if s.qkv_epi is not None else None, dqkv, s.draw,
                       s.qkv_epi or dict(embed_dim=C, head_dim=64), grads=s.g.qkn,
                       bias_grad=s.g.b_qkv if QK_COLSUM else None)
        elif s.qkv_epi is not None:  # fp32 block (autocast off) with qk-norm / RoPE: in place on dqkv
            ops.qk_bwd(s.tape.raw, dqkv, dqkv, s.qkv_epi, grads=s.g.qkn)
    _gemm_stage([dict(a=s.draw, w=s.bp.wt_qkv, out=s.dxn) for s in its], _lib.SR_EPI_F32, tag + ".dgrad")
    _wgrad_stage([(s.tag, s.draw, s.tape.xn1, s.g.w_qkv, None if bf and QK_COLSUM else s.g.b_qkv, None, None, None)
                  for s in its], bf, tag)
    for s in its:
        ops.layernorm_bwd(s.tape.x0, s.dxn, s.pb.ln1_w, s.pb.eps, s.dx, dxb=s.dxb, dw=s.g.ln1_w, db=s.g.ln1_b)


def frame_attend_train(pb: runtime.PackedBlock, frames: int, tokens: int):
    """Forward / backward attention callbacks within each frame (frame and DINO blocks)."""
    C = pb.dim

    def fwd(qkv, o, lse):
        ops.attention(qkv[:, 0:C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=pb.heads, head_dim=pb.head_dim,
                      batch=frames, lq=tokens, q_bstride=tokens, l0=tokens, k0_bstride=tokens, lse=lse,
                      tag="attn_frame", tail_readable=True)

    def bwd(tape, dO, dqkv):
        q = tape.qkv
        delta = _delta(dqkv.device, frames * pb.heads * tokens)
        ops.attention_bwd(q[:, 0:C], q[:, C:2 * C], q[:, 2 * C:], tape.o, tape.lse, dO, dqkv[:, 0:C],
                          dqkv[:, C:2 * C], dqkv[:, 2 * C:], delta, heads=pb.heads, batch=frames, lq=tokens,
                          q_bstride=tokens, l0=tokens, k0_bstride=tokens, tag="attn_bwd_frame")
    return fwd, bwd


_DELTA = {}


def _delta(device, n: int) -> Tensor:
    t = _DELTA.get(device)
    if t is None or t.numel() < n:
        t = torch.empty(n, device=device, dtype=torch.float32)
        _DELTA[device] = t
    return t[:n]
