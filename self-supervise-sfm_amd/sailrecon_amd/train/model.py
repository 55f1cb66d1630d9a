"""SailRecon training graph on the HIP path: aggregator + camera-head forward with saved
activations and the matching backward (the autograd graph that
``loss.backward()`` walks in train_imc.py:404 for predictions from sail_recon.py:70-159).

Scope: one scene per replica (B = 1, as train_imc.py's DataLoader batch_size=1 under DDP), the
aggregator in bf16 (autocast, train_imc.py:385) and the heads in fp32 (sail_recon.py:118-119).
The loss reaches the parameters only through the camera head's LAST iteration (the refinement
detaches the previous prediction, camera_head.py:148-150, and compute_loss reads
predictions[-1]), so the head keeps a tape for that iteration only; the DPT heads do not feed
the loss and get no gradient (DDP find_unused_parameters, train_imc.py:474).

Residual stream layout as in inference (models/aggregator.py): rows [0, Na*P) anchors,
[Na*P, S*P) queries, P = 5 + patches.  Backward walks the layers in reverse:

    layer l:  reloc block (query rows; its shared anchor-subsample segment's dK|dV -> the
              k-norm/RoPE backward -> K|V dgrad -> LayerNorm-through-row-map backward, added to
              the anchor rows) and global block (anchor rows) -> frame block (all rows)
    then the aggregator special tokens, DINO's final norm and blocks, the patch embedding.

What the forward saves for the backward travels as typed tapes (StepTape): engine.BlockTape for
every transformer block, and for everything between the blocks the records below.  The workspace
owns their memory; each buffer is requested in ONE place, by the stage that writes it, and the
backward reads the tensor from the tape it is handed.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib, ops, runtime
from ..models.aggregator import _sl, check_frame_lists, subsample_rowmap
from . import engine
from .params import FlatParams

Tensor = torch.Tensor
BF16 = torch.bfloat16
F32 = torch.float32
# SR_TRAIN_PAIR_DGRAD (default 1; 0 for the A/B): the layer's reloc and global blocks run their
# backward stage by stage with each stage's dgrad GEMMs grouped into one launch
_PAIR_DGRAD = os.environ.get("SR_TRAIN_PAIR_DGRAD", "1") != "0"
# SR_TRAIN_PAIR_FWD (default 1; 0 for the A/B): their forward likewise, each GEMM of the two
# blocks as one grouped launch (engine.run_block_train_multi)
_PAIR_FWD = os.environ.get("SR_TRAIN_PAIR_FWD", "1") != "0"


def _i32(rows, dev) -> Tensor:
    return runtime.to_device(torch.as_tensor(np.asarray(rows, dtype=np.int32)), dev)


@dataclass
class Scene:
    """One step's plan: sizes, the internal frame order ([anchors ; queries]) and what every layer shares."""
    S: int
    Na: int
    Nq: int
    H: int
    W: int
    P: int                  # rows per frame: the special tokens, then n_patch patches
    n_patch: int
    types: List[int]        # per internal frame: 0 = ORIGINAL frame 0 as an anchor, 1 = other anchors, 2 = queries
    cam_rows: Tensor        # int32 [S]: every frame's camera-token row of x
    rope: Optional[tuple]
    posctx: dict            # the QKV epilogue's position keywords (runtime.qkv_params)

    @property
    def R(self) -> int:     # rows of x
        return self.S * self.P

    @property
    def q0(self) -> int:    # first query row of x
        return self.Na * self.P


@dataclass
class EmbedTape:
    cols: Tensor                 # [S * n_patch, kpad] normalised im2col patches (the patch GEMM's operand)
    prenorm: Optional[Tensor]    # fp32 [R, C] x before DINO's final norm (DINO only)
    pos_resampled: bool          # DINO's pos-embed went through the bicubic resampling (its grad takes the adjoint)


@dataclass
class SubsampleTape:
    """One layer's anchor subsample, the reloc block's shared key / value segment."""
    rowmap: Tensor               # int32 [n_sub] rows of x: per anchor frame its special rows, then the drawn patches
    xn_sub: Tensor               # [n_sub, C]  LN1 of those rows
    kv_sub: Tensor               # [n_sub, 2C] k|v after k-norm + RoPE
    kv_raw: Optional[Tensor]     # [n_sub, 2C] pre-norm k|v (None without qk-norm / RoPE: kv_sub is it)


@dataclass
class CameraTape:
    """The camera head's LAST refinement iteration (the trunk blocks keep engine.BlockTapes)."""
    Na: int
    cam_in: Tensor     # [S, 2C] camera tokens of the last layer (frame half | global / reloc half)
    tok: Tensor        # token_norm(cam_in)
    pred_in: Tensor    # [S, 9] embed_pose's input, the detached previous prediction
    emb: Tensor        # embed_pose output
    act_emb: Tensor    # silu(emb)
    mod: Tensor        # [S, 3 * 2C] shift | scale | gate
    xn_ada: Tensor     # adaln_norm(tok)
    xm_out: Tensor     # the trunk's output, before trunk_norm
    xn_t: Tensor       # trunk_norm(xm_out)
    pre: Tensor        # pose_branch.fc1 pre-activation
    hb: Tensor         # gelu(pre)
    act: Tensor        # [S, 9] activated pose encoding


@dataclass
class StepTape:
    scene: Scene
    embed: EmbedTape
    layers: List[SubsampleTape]
    cam: CameraTape


class TrainGraph:
    """Training forward/backward for a SailRecon-style module with ``aggregator`` and
    ``camera_head`` (the DPT heads are not run: they do not feed the loss)."""

    def __init__(self, model, flat: Optional[FlatParams] = None, compute_dtype: torch.dtype = BF16):
        """``compute_dtype``: the aggregator's operand dtype.  bf16 (default) is train_imc.py's
        autocast; fp32 runs every aggregator GEMM and attention (forward and backward) in exact
        fp32, which pins the graph's wiring against fp32 autograd far below bf16 noise
        (tests/test_train_graph_gpu.py)."""
        if compute_dtype not in (BF16, F32):
            raise ValueError(f"TrainGraph: compute_dtype bf16 or fp32 (got {compute_dtype})")
        self.cdt = compute_dtype
        self.model = model
        self.agg = model.aggregator
        self.cam = model.camera_head
        self.flat = flat if flat is not None else FlatParams(model)
        self.dev = self.flat.data.device
        self.invalidate()
        self._tapes = {}
        self._sc = engine.BwdScratch()
        self._sc2 = engine.BwdScratch()  # the global block's scratch beside the reloc block's (block_bwd_multi)
        self._step: Optional[StepTape] = None   # what the last forward() saved, until backward() has used it
        # grad_ready_hook(module): called once a module's parameter grads are final within the
        # backward (data-parallel training starts that module's all-reduce right away)
        self.grad_ready_hook = None

    def _ready(self, module) -> None:
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(module)

    # ------------------------------------------------------------------ parameter packs
    def invalidate(self) -> None:
        """Drop every derived weight pack (call after load_state_dict)."""
        self.agg.invalidate_packed()
        if self.cam is not None:
            self.cam.invalidate_packed()
        self._reset_pos_cache()
        # block -> (dtype, its backward pack), in the order the first backward asked for them
        self._bwd: Dict[torch.nn.Module, Tuple[torch.dtype, engine.BwdPack]] = {}
        self._refresh = None  # (the packs it was built from, ops.weight_refresh_table, its items) of refresh_packs

    def _reset_pos_cache(self) -> None:
        pe = self.agg.patch_embed
        if hasattr(pe, "_pos_cache"):
            pe._pos_cache = {}

    def refresh_packs(self) -> None:
        """After an optimizer step: recast the bf16 forward weights in place (fp32 biases, gammas
        and norms alias the flat parameter buffer) and rebuild the transposed backward packs."""
        # bf16 blocks with a backward pack: every block's casts and transposed packs in ONE launch
        # (sr_weight_refresh_list_bf16 over a device table built once: the packs and the flat
        # parameter buffer do not move; one launch per block left the GPU waiting on the host).
        # The table is kept with the very pack objects it was built from and reused only while the
        # blocks still hold those (``is``): a re-created pack rebuilds it instead of refreshing a stale copy
        fused = [(blk, blk._packed[BF16], bp) for blk, (dt, bp) in self._bwd.items()
                 if dt == BF16 and blk._packed.get(BF16) is not None]
        if fused:
            src = [o for f in fused for o in f]
            if self._refresh is None or len(self._refresh[0]) != len(src) or \
                    any(a is not b for a, b in zip(self._refresh[0], src)):
                items = []
                for blk, pb, bp in fused:
                    items += engine.refresh_items_bf16(blk, pb, bp)
                self._refresh = (src, ops.weight_refresh_table(items, self.dev), items)
            ops.weight_refresh_list(self._refresh[1])
        done = {blk for blk, _, _ in fused}
        for blk in self._agg_blocks():
            pb = blk._packed.get(BF16)
            if pb is not None and blk not in done:
                a = blk.attn
                for src, dst in ((a.qkv.weight, pb.w_qkv), (a.proj.weight, pb.w_proj),
                                 (blk.mlp.fc1.weight, pb.w_fc1), (blk.mlp.fc2.weight, pb.w_fc2)):
                    ops.cast_bf16(src.detach(), dst)
        self.agg._packed.clear()  # patch weights / special-token table (small; rebuilt per step)
        self._reset_pos_cache()
        for blk, (dt, bp) in self._bwd.items():
            if blk not in done:
                engine.pack_bwd(blk, blk.packed(dt), dt, into=bp)

    def _agg_blocks(self):
        a = self.agg
        out = list(a.frame_blocks) + list(a.global_blocks) + list(a.global_reloc_blocks)
        if hasattr(a.patch_embed, "blocks"):
            out += list(a.patch_embed.blocks)
        return out

    def _bwd_pack(self, blk, dt) -> engine.BwdPack:
        if blk not in self._bwd:
            self._bwd[blk] = (dt, engine.pack_bwd(blk, blk.packed(dt), dt))
        return self._bwd[blk][1]

    def _tape(self, key, rows, dim, hidden, dt, lse_numel, separate_raw) -> engine.BlockTape:
        t = self._tapes.get(key)
        if t is None or t.x0.shape[0] != rows or t.x0.shape[1] != dim or t.xn1.dtype != dt:
            t = engine.alloc_tape(rows, dim, hidden, dt, self.dev, lse_numel, separate_raw)
            self._tapes[key] = t
        return t

    def _buf(self, name, rows, cols, dt):
        return self._sc.get("g_" + name, rows, cols, dt, self.dev)

    # ------------------------------------------------------------------ forward
    def forward(self, images: Tensor, no_reloc_list: List[int], reloc_list: List[int], fix_rank=300) -> Tensor:
        """Training forward (aggregator bf16 + camera head fp32).  Returns the activated pose
        encoding of the query views of the last refinement iteration, [1, Nq, 9] (the
        ``pose_enc`` / extrinsic / intrinsic source of compute_loss), and keeps the tapes."""
        agg = self.agg
        sc, imgs = self._plan(images, no_reloc_list, reloc_list)
        x, embed = self._embed_forward(sc, imgs)
        # subsample draws (aggregator.py:580-626), the generator order of inference; after the
        # embedding's launches are queued, so that the host draws while the device runs them
        idx = agg.plan_subsample(fix_rank, 1, sc.Na, sc.n_patch)
        rowmap = runtime.to_device(torch.from_numpy(subsample_rowmap(idx, sc.S, sc.P, agg.patch_start_idx)[:, 0]),
                                   self.dev)
        # ---- alternating layers, aggregator.py:339-423
        cam_in = self._buf("cam_in", sc.S, 2 * agg.embed_dim, F32)
        layers = [self._layer_forward(sc, x, l, rowmap[l], cam_in) for l in range(agg.depth)]
        # ---- camera head, fp32 (camera_head.py:85-186)
        cam = self._camera_forward(cam_in, sc.Na)
        self._step = StepTape(sc, embed, layers, cam)
        return cam.act[sc.Na:].view(1, sc.Nq, 9)

    def _plan(self, images: Tensor, no_reloc_list: List[int], reloc_list: List[int]) -> Tuple[Scene, Tensor]:
        """The checked scene and its images in the internal frame order, fp32 [S, 3, H, W]."""
        agg = self.agg
        B, S, C_in, H, W = images.shape
        if B != 1:
            raise NotImplementedError("training runs one scene per replica (B == 1, train_imc.py:503-510)")
        if C_in != 3:
            raise ValueError(f"Expected 3 input channels, got {C_in}")
        runtime.require_device(images, "TrainGraph")
        check_frame_lists(no_reloc_list, reloc_list, S)
        Na, Nq = len(no_reloc_list), len(reloc_list)
        if Nq == 0:
            raise ValueError("training needs anchors and queries")
        ps = agg.patch_size
        assert H % ps == 0 and W % ps == 0
        gh, gw = H // ps, W // ps
        psi = agg.patch_start_idx
        P = gh * gw + psi
        imgs = images[:, list(no_reloc_list) + list(reloc_list)].reshape(S, 3, H, W).float().contiguous()
        rope = agg.rope.tables(agg.embed_dim // agg.num_heads, max(gh, gw) + 1, self.dev) if agg.rope is not None \
            else None
        return Scene(S=S, Na=Na, Nq=Nq, H=H, W=W, P=P, n_patch=gh * gw,
                     types=[0 if a == 0 else 1 for a in no_reloc_list] + [2] * Nq,
                     cam_rows=_i32([f * P for f in range(S)], self.dev), rope=rope,
                     posctx=dict(tokens_per_frame=P, patch_start=psi, grid_w=gw)), imgs

    def _embed_forward(self, sc: Scene, imgs: Tensor) -> Tuple[Tensor, EmbedTape]:
        """Patch embed (+ DINO) and the aggregator's special tokens, vision_transformer.py:242-307 /
        aggregator.py:267-299 -> the residual stream x fp32 [R, C]."""
        agg, cdt, dev = self.agg, self.cdt, self.dev
        S, P, R, C, n_patch = sc.S, sc.P, sc.R, agg.embed_dim, sc.n_patch
        ps, psi = agg.patch_size, agg.patch_start_idx
        hidden = agg.frame_blocks[0].mlp.fc1.out_features
        x = self._buf("x", R, C, F32)
        kpad = -(-3 * ps * ps // 64) * 64
        misc = agg._pack_misc(cdt, kpad)
        tape = EmbedTape(cols=self._buf("im2col", S * n_patch, kpad, cdt), prenorm=None, pos_resampled=False)
        ops.im2col_normalize(imgs, ps, tape.cols, kpad)
        is_dino = hasattr(agg.patch_embed, "blocks")
        if is_dino:
            dino = agg.patch_embed
            tape.pos_resampled = dino.pos_resampled(sc.H, sc.W)
            if tape.pos_resampled:
                # interpolate_pos_encoding (vision_transformer.py:206-240) of the live parameter, every
                # step (the optimizer updates it in place): a 5 MB table transform on the device;
                # backward() applies its adjoint to the patch rows' colsum
                pe = dino.pos_embed.detach()[0]
                pos_tab = torch.cat([pe[:1], dino.resample_patch_pos(pe[1:], sc.H, sc.W)], 0).contiguous()
            else:
                pos_tab = dino.pos_embed_for(sc.H, sc.W)
            row_add = pos_tab[1:]
        else:
            row_add = self._buf("zeros_pos", n_patch, C, F32).zero_()
        ops.gemm(tape.cols, misc["w_patch"], x, _lib.SR_EPI_PATCH, bias=misc["b_patch"], rows=S * n_patch,
                 patch=dict(seg_rows=n_patch, seg_stride=P, seg_offset=psi, row_add=row_add), tag="gemm")
        if is_dino:
            dtab = torch.cat([(dino.cls_token[0, 0] + pos_tab[0])[None], dino.register_tokens[0]], 0)
            ops.set_special_tokens(x, S, P, dtab.detach().float().contiguous()[None],
                                   torch.zeros(S, device=dev, dtype=torch.int32))
            for i, blk in enumerate(dino.blocks):
                pb = blk.packed(cdt)
                fwd, _ = engine.frame_attend_train(pb, S, P)
                engine.run_block_train(pb, x, 0, R, self._tape(("dino", i), R, C, hidden, cdt, S * pb.heads * P,
                                                                False), fwd, None)
            tape.prenorm = self._buf("dino_prenorm", R, C, F32)
            ops.copy_rows(tape.prenorm, x, R)
            ops.layernorm(x, dino.norm.weight, dino.norm.bias, dino.norm.eps, x)
        ops.set_special_tokens(x, S, P, misc["special"], _i32(sc.types, dev))
        return x, tape

    def _layer_forward(self, sc: Scene, x: Tensor, l: int, rowmap: Tensor, cam_in: Tensor) -> SubsampleTape:
        """Layer l: the frame block, then the reloc (query rows) and global (anchor rows) blocks; the last
        layer's camera-token rows go to ``cam_in`` (frame half after the frame block, then the other)."""
        agg, cdt = self.agg, self.cdt
        S, P, R, q0, C = sc.S, sc.P, sc.R, sc.q0, agg.embed_dim
        hidden = agg.frame_blocks[0].mlp.fc1.out_features
        n_sub = rowmap.shape[0]
        last = l == agg.depth - 1
        pf = agg.frame_blocks[l].packed(cdt)
        fwd, _ = engine.frame_attend_train(pf, S, P)
        engine.run_block_train(pf, x, 0, R, self._tape(("frame", l), R, C, hidden, cdt, S * pf.heads * P, True),
                               fwd, runtime.qkv_params(pf, sc.rope, pos_row_base=0, **sc.posctx))
        if last:
            ops.copy_rows(cam_in[:, :C], x, S, rowmap=sc.cam_rows)
        pr = agg.global_reloc_blocks[l].packed(cdt)
        pg = agg.global_blocks[l].packed(cdt)
        # anchor-subsample K|V of the reloc block (reads the anchors before the global block)
        epi = runtime.kv_params(pr, sc.rope, pos_rowmap=rowmap, **sc.posctx)
        sub = SubsampleTape(rowmap=rowmap, xn_sub=self._buf(f"xn_sub{l}", n_sub, C, cdt),
                            kv_sub=self._buf(f"kv_sub{l}", n_sub, 2 * C, cdt),
                            kv_raw=self._buf(f"kv_raw{l}", n_sub, 2 * C, cdt) if epi is not None else None)
        ops.layernorm(x, pr.ln1_w, pr.ln1_b, pr.eps, sub.xn_sub, rowmap=rowmap, rows=n_sub)
        runtime.kv_gemm(pr, sub.xn_sub, sub.kv_sub, epi, aux=sub.kv_raw)
        rfwd, _ = self._reloc_attn(pr, sub.kv_sub, None, sc.Nq, P, n_sub)
        rel = dict(pb=pr, x=x, r0=q0, r1=R, tape=self._tape(("reloc", l), R - q0, C, hidden, cdt,
                                                            sc.Nq * pr.heads * P, True),
                   attend=rfwd, qkv_epi=runtime.qkv_params(pr, sc.rope, pos_row_base=q0, **sc.posctx))
        gfwd, _ = self._global_attn(pg, q0)
        glo = dict(pb=pg, x=x, r0=0, r1=q0, tape=self._tape(("global", l), q0, C, hidden, cdt, pg.heads * q0, True),
                   attend=gfwd, qkv_epi=runtime.qkv_params(pg, sc.rope, pos_row_base=0, **sc.posctx))
        if _PAIR_FWD:  # disjoint rows; the reloc block's anchor K|V was projected above
            engine.run_block_train_multi([rel, glo])
        else:
            for it in (rel, glo):
                engine.run_block_train_multi([it])
        if last:
            ops.copy_rows(cam_in[:, C:], x, S, rowmap=sc.cam_rows)
        return sub

    def _global_attn(self, pg, La):
        C = pg.dim

        def fwd(qkv, o, lse):
            # the tape's q|k|v has readable tail rows (engine.alloc_tape): the hand-scheduled sweep's
            # ragged variant covers L = 21,984 (C4); the key bound comes from the per-launch key scan
            # (the weights move every step)
            ops.attention(qkv[:, 0:C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=pg.heads, head_dim=pg.head_dim,
                          batch=1, lq=La, q_bstride=0, l0=La, k0_bstride=0, lse=lse, tag="attn_global",
                          tail_readable=True)

        def bwd(tape, dO, dqkv):
            q = tape.qkv
            ops.attention_bwd(q[:, 0:C], q[:, C:2 * C], q[:, 2 * C:], tape.o, tape.lse, dO, dqkv[:, 0:C],
                              dqkv[:, C:2 * C], dqkv[:, 2 * C:], engine._delta(dqkv.device, pg.heads * La),
                              heads=pg.heads, batch=1, lq=La, q_bstride=0, l0=La, k0_bstride=0, tag="attn_bwd_global")
        return fwd, bwd

    def _reloc_attn(self, pr, kv_sub, dkv_sub, Nq, P, n_sub):
        C = pr.dim

        def fwd(qkv, o, lse):
            ops.attention(qkv[:, 0:C], kv_sub[:, 0:C], kv_sub[:, C:2 * C], o, heads=pr.heads, head_dim=pr.head_dim,
                          batch=Nq, lq=P, q_bstride=P, l0=n_sub, k0_bstride=0, k1=qkv[:, C:2 * C],
                          v1=qkv[:, 2 * C:3 * C], l1=P, k1_bstride=P, lse=lse, tag="attn_reloc")

        def bwd(tape, dO, dqkv):
            q = tape.qkv
            ops.attention_bwd(q[:, 0:C], kv_sub[:, 0:C], kv_sub[:, C:2 * C], tape.o, tape.lse, dO, dqkv[:, 0:C],
                              dkv_sub[:, 0:C], dkv_sub[:, C:2 * C], engine._delta(dqkv.device, Nq * pr.heads * P),
                              heads=pr.heads, batch=Nq, lq=P, q_bstride=P, l0=n_sub, k0_bstride=0,
                              k1=q[:, C:2 * C], v1=q[:, 2 * C:3 * C], dk1=dqkv[:, C:2 * C], dv1=dqkv[:, 2 * C:],
                              l1=P, k1_bstride=P, tag="attn_bwd_reloc")
        return fwd, bwd

    # ------------------------------------------------------------------ camera head
    def _camera_forward(self, cam_in: Tensor, Na: int) -> CameraTape:
        cam = self.cam
        M, Cc = cam_in.shape
        f = lambda t: t.detach()  # noqa: E731 (fp32 contiguous params alias the flat buffer)
        buf = lambda name, cols=Cc: self._buf(name, M, cols, F32)  # noqa: E731
        t = CameraTape(Na=Na, cam_in=cam_in, tok=buf("cam_tok"), pred_in=buf("cam_pred_in", 9), emb=buf("cam_emb"),
                       act_emb=buf("cam_act_emb"), mod=buf("cam_mod", 3 * Cc), xn_ada=buf("cam_xn_ada"),
                       xm_out=buf("cam_xm_out"), xn_t=buf("cam_xn_t"), pre=buf("cam_pre", Cc // 2),
                       hb=buf("cam_hb", Cc // 2), act=torch.empty(M, 9, device=self.dev, dtype=F32))
        ops.layernorm(cam_in, cam.token_norm.weight, cam.token_norm.bias, cam.token_norm.eps, t.tok)
        pbs = [blk.packed(F32) for blk in cam.trunk]
        hid = pbs[0].w_fc1.shape[0]
        xm, delta, pred = buf("cam_xm"), buf("cam_delta", 9), buf("cam_pred", 9)
        w_emb, b_emb = f(cam.embed_pose.weight), f(cam.embed_pose.bias)
        w_mod, b_mod = f(cam.poseLN_modulation[1].weight), f(cam.poseLN_modulation[1].bias)
        pbr = cam.pose_branch
        n_it = 4
        for it in range(n_it):
            last = it == n_it - 1
            if it == 0:
                ops.linear_small(f(cam.empty_pose_tokens).reshape(1, 9), w_emb, b_emb, t.emb, rows=M, lda=0)
            else:
                ops.linear_small(pred, w_emb, b_emb, t.emb, rows=M)
                if last:  # embed_pose's input (the detached previous prediction), for its weight grad
                    ops.copy2d(t.pred_in, pred)
            ops.silu(t.emb, t.act_emb)
            ops.gemm(t.act_emb, w_mod, t.mod, _lib.SR_EPI_BIAS, bias=b_mod)
            ops.layernorm(t.tok, None, None, cam.adaln_norm.eps, t.xn_ada)
            ops.adaln_modulate(t.xn_ada, t.tok, t.mod, xm)
            for bi, pb in enumerate(pbs):
                fwd = self._cam_attn(pb, M, Na)[0]
                if last:
                    engine.run_block_train(pb, xm, 0, M, self._tape(("cam", bi), M, Cc, hid, F32, 0, False), fwd, None)
                else:
                    sc = runtime.scratch(self._sc, M, Cc, hid, F32, self.dev, tag="_camfwd")
                    runtime.run_block(pb, xm, 0, M, sc, lambda qkv, o, fwd=fwd: fwd(qkv, o, None), None)
            if last:
                ops.copy_rows(t.xm_out, xm, M)
            ops.layernorm(xm, cam.trunk_norm.weight, cam.trunk_norm.bias, cam.trunk_norm.eps, t.xn_t)
            ops.gemm(t.xn_t, f(pbr.fc1.weight), t.hb, _lib.SR_EPI_BIAS_GELU, bias=f(pbr.fc1.bias), aux=t.pre)
            ops.linear_small(t.hb, f(pbr.fc2.weight), f(pbr.fc2.bias), delta, rows=M)
            ops.pose_update(pred, delta, t.act, first=(it == 0))
        return t

    def _cam_attn(self, pb, M, Na):
        C, H, D = pb.dim, pb.heads, pb.head_dim

        def fwd(qkv, o, lse):
            ops.attention(qkv[:, 0:C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, heads=H, head_dim=D, batch=1, lq=M,
                          q_bstride=0, l0=M, k0_bstride=0, mask_mode=_lib.SR_MASK_CAMERA, n_anchor=Na)

        def bwd(tape, dO, dqkv):
            q = tape.qkv
            ops.attention_bwd_small(q[:, 0:C], q[:, C:2 * C], q[:, 2 * C:], dO, dqkv[:, 0:C], dqkv[:, C:2 * C],
                                    dqkv[:, 2 * C:], heads=H, head_dim=D, mask_mode=_lib.SR_MASK_CAMERA, n_anchor=Na)
        return fwd, bwd

    # ------------------------------------------------------------------ backward
    def backward(self, d_pose: Tensor) -> None:
        """Accumulate into every parameter's .grad the gradient of <d_pose, pose> where pose is
        forward()'s output ([1, Nq, 9] activated pose encoding of the last iteration)."""
        step = self._step
        if step is None:
            raise RuntimeError("backward() needs a training forward() first")
        d_raw = self._camera_backward(step.cam, d_pose.reshape(-1, 9).float().contiguous())
        self._ready(self.cam)
        self._aggregator_backward(step, d_raw)
        self._step = None

    def _camera_backward(self, t: CameraTape, d_act_q: Tensor) -> Tensor:
        cam = self.cam
        M, Cc = t.cam_in.shape
        g = lambda p: p.grad  # noqa: E731
        f = lambda p: p.detach()  # noqa: E731
        buf = lambda name, cols=Cc, rows=M: self._buf(name, rows, cols, F32)  # noqa: E731
        pbr = cam.pose_branch
        # activate_pose backward (FoV ReLU; translation / quaternion linear), head_act.py:12-60;
        # pred_4 = pred_3.detach() + delta_4 -> d delta_4 = d pred_4 (anchor rows: no loss)
        dd = buf("cd_delta", 9)
        ops.pose_act_bwd(dd, d_act_q, t.act, t.Na)
        ops.wgrad_small(dd, t.hb, g(pbr.fc2.weight), db=g(pbr.fc2.bias), accumulate=True)
        w2t = buf("cw2t", 9, rows=Cc // 2)
        ops.transpose(f(pbr.fc2.weight), w2t)
        dhb = buf("cd_hb", Cc // 2)
        ops.linear_small(dd, w2t, None, dhb, rows=M)
        dpre = buf("cd_pre", Cc // 2)
        ops.act_bwd(ops.ACT_GELU, t.pre, dhb, dpre)
        ops.wgrad_small(dpre, t.xn_t, g(pbr.fc1.weight), db=g(pbr.fc1.bias), accumulate=True)
        w1t = buf("cw1t", Cc // 2, rows=Cc)
        ops.transpose(f(pbr.fc1.weight), w1t)
        dxn = buf("cd_xn")
        ops.gemm(dpre, w1t, dxn, _lib.SR_EPI_F32)
        dxm = buf("cd_xm").zero_()
        ops.layernorm_bwd(t.xm_out, dxn, cam.trunk_norm.weight, cam.trunk_norm.eps, dxm,
                          dw=g(cam.trunk_norm.weight), db=g(cam.trunk_norm.bias))
        # trunk blocks (fp32, camera mask), reverse
        for bi in reversed(range(len(cam.trunk))):
            blk = cam.trunk[bi]
            pb = blk.packed(F32)
            _, bwd = self._cam_attn(pb, M, t.Na)
            engine.block_bwd(pb, self._bwd_pack(blk, F32), engine.block_grads(blk), self._tapes[("cam", bi)], dxm,
                             None, bwd, None, self._sc, tag="cam")
        # adaLN: xm = gate * (LN(tok) * (1 + scale) + shift) + tok
        dtok = buf("cd_tok")
        ops.copy_rows(dtok, dxm, M)
        dxa = buf("cd_xn_ada")
        dmod = buf("cd_mod", 3 * Cc)
        ops.adaln_bwd(t.xn_ada, t.mod, dxm, dxa, dmod)
        ops.layernorm_bwd(t.tok, dxa, None, cam.adaln_norm.eps, dtok)
        lin = cam.poseLN_modulation[1]
        ops.wgrad_small(dmod, t.act_emb, g(lin.weight), db=g(lin.bias), accumulate=True)
        wmt = buf("cwmt", 3 * Cc, rows=Cc)
        ops.transpose(f(lin.weight), wmt)
        dact = buf("cd_act_emb")
        ops.gemm(dmod, wmt, dact, _lib.SR_EPI_F32)
        demb = buf("cd_emb")
        ops.act_bwd(ops.ACT_SILU, t.emb, dact, demb)
        ops.wgrad_small(demb, t.pred_in, g(cam.embed_pose.weight), db=g(cam.embed_pose.bias), accumulate=True)
        # token_norm
        d_raw = buf("cd_raw").zero_()
        ops.layernorm_bwd(t.cam_in, dtok, cam.token_norm.weight, cam.token_norm.eps, d_raw,
                          dw=g(cam.token_norm.weight), db=g(cam.token_norm.bias))
        return d_raw

    def _aggregator_backward(self, step: StepTape, d_raw: Tensor) -> None:
        agg, sc = self.agg, step.scene
        C = agg.embed_dim
        dx = self._buf("dx", sc.R, C, F32).zero_()
        dxb = self._buf("dxb", sc.R, C, BF16) if self.cdt == BF16 else None  # fp32 mode: dx itself is the GEMM operand
        # camera tokens of the last layer: second half = after the global / reloc blocks
        ops.scatter_rows(dx, sc.cam_rows, d_raw[:, C:], accumulate=True)
        for l in reversed(range(agg.depth)):
            self._layer_backward(sc, step.layers[l], l, dx, dxb, d_raw)
        self._embed_backward(sc, step.embed, dx, dxb)

    def _layer_backward(self, sc: Scene, sub: SubsampleTape, l: int, dx: Tensor, dxb: Optional[Tensor],
                        d_raw: Tensor) -> None:
        """Layer l's reloc and global blocks, the anchor subsample they share, then the frame block."""
        agg, cdt = self.agg, self.cdt
        S, P, q0, C = sc.S, sc.P, sc.q0, agg.embed_dim
        bf = cdt == BF16
        n_sub = sub.rowmap.shape[0]
        dkv_sub = self._buf("dkv_sub", n_sub, 2 * C, F32)
        dkv_raw = self._buf("dkv_raw", n_sub, 2 * C, BF16) if bf else dkv_sub
        dxn_sub = self._buf("dxn_sub", n_sub, C, F32)
        if bf:
            ops.cast_bf16(dx, dxb)
        br, bg = agg.global_reloc_blocks[l], agg.global_blocks[l]
        pr, pg = br.packed(cdt), bg.packed(cdt)
        # reloc block (query rows); its shared segment's dK|dV land in dkv_sub
        _, rbwd = self._reloc_attn(pr, sub.kv_sub, dkv_sub, sc.Nq, P, n_sub)
        gr = engine.block_grads(br)
        # global block (anchor rows)
        _, gbwd = self._global_attn(pg, q0)
        tg = self._tapes[("global", l)]
        bp = self._bwd_pack(br, cdt)
        rel = dict(pb=pr, bp=bp, g=gr, tape=self._tapes[("reloc", l)], dx=dx[q0:], dxb=dxb[q0:] if bf else None,
                   attend_bwd=rbwd, qkv_epi=runtime.qkv_params(pr, sc.rope, pos_row_base=q0, **sc.posctx),
                   sc=self._sc, tag="reloc")
        glo = dict(pb=pg, bp=self._bwd_pack(bg, cdt), g=engine.block_grads(bg), tape=tg, dx=dx[:q0],
                   dxb=dxb[:q0] if bf else None, attend_bwd=gbwd,
                   qkv_epi=runtime.qkv_params(pg, sc.rope, pos_row_base=0, **sc.posctx), sc=self._sc2, tag="global")
        if _PAIR_DGRAD and sc.Nq > 0:
            # the two blocks' dgrad GEMMs stage by stage as grouped launches (engine.block_bwd_multi)
            engine.block_bwd_multi([rel, glo], tag="pair")
        else:
            for it in (rel, glo):  # one after another: both on the first scratch
                engine.block_bwd_multi([dict(it, sc=self._sc)])
        # anchor subsample: k-norm + RoPE backward -> K|V dgrad / wgrad -> LN1 (row map) backward
        epi = runtime.kv_params(pr, sc.rope, pos_rowmap=sub.rowmap, **sc.posctx)
        db_kv = _sl(gr.b_qkv, C, 3 * C)
        if bf or epi is not None:  # fp32 without qk-norm / RoPE: dkv_raw is dkv_sub
            ops.qk_bwd(sub.kv_raw, dkv_sub, dkv_raw, epi or dict(embed_dim=C, head_dim=64, col_offset=C), grads=gr.qkn,
                       bias_grad=db_kv if bf and engine.QK_COLSUM else None)
        ops.gemm(dkv_raw, bp.wt_qkv[:, C:], dxn_sub, _lib.SR_EPI_F32, tag="reloc.dgrad")
        if bf:  # (the k|v bias grad came out of qk_bwd)
            ops.gemm_wgrad(dkv_raw, sub.xn_sub, gr.w_qkv[C:], accumulate=True, tag="reloc.wgrad")
            if not engine.QK_COLSUM:
                ops.colsum(dkv_raw, db_kv, accumulate=True)
        else:
            ops.wgrad_small(dkv_raw, sub.xn_sub, gr.w_qkv[C:], db=db_kv, accumulate=True)
        ops.layernorm_bwd(tg.x0, dxn_sub, pr.ln1_w, pr.eps, dx, rowmap=sub.rowmap, rows=n_sub,
                          dw=gr.ln1_w, db=gr.ln1_b)
        self._ready(br)
        self._ready(bg)
        if l == agg.depth - 1:  # first half of the camera tokens = the frame block's output
            ops.scatter_rows(dx, sc.cam_rows, d_raw[:, :C], accumulate=True)
        if bf:
            ops.cast_bf16(dx, dxb)
        bf_ = agg.frame_blocks[l]
        pf = bf_.packed(cdt)
        _, fbwd = engine.frame_attend_train(pf, S, P)
        engine.block_bwd(pf, self._bwd_pack(bf_, cdt), engine.block_grads(bf_), self._tapes[("frame", l)], dx,
                         dxb, fbwd, runtime.qkv_params(pf, sc.rope, pos_row_base=0, **sc.posctx), self._sc, tag="frame")
        self._ready(bf_)

    def _embed_backward(self, sc: Scene, embed: EmbedTape, dx: Tensor, dxb: Optional[Tensor]) -> None:
        self._special_tokens_backward(sc, dx)
        pe = self.agg.patch_embed
        if hasattr(pe, "blocks"):
            dx = self._dino_backward(sc, embed, dx, dxb)
            pe = pe.patch_embed
        self._patch_backward(sc, embed, pe.proj, dx)
        self._ready(None)  # every remaining parameter

    def _special_tokens_backward(self, sc: Scene, dx: Tensor) -> None:
        """Aggregator special tokens (aggregator.py:287-299), by the forward's frame types; their rows
        were overwritten, so nothing flows below them.  Runs of equal type are column-summed as
        strided frame views."""
        agg = self.agg
        S, P, C, psi, types = sc.S, sc.P, agg.embed_dim, agg.patch_start_idx, sc.types
        dst = {0: (agg.camera_token.grad[0, 0, 0], agg.register_token.grad[0, 0]),
               1: (agg.camera_token.grad[0, 1, 0], agg.register_token.grad[0, 1]),
               2: (agg.camera_token_reloc.grad[0, 0, 0], agg.register_token_reloc.grad[0, 0])}
        groups, f0 = [], 0
        for f in range(1, S + 1):
            if f == S or types[f] != types[f0]:
                groups.append((f0, f) + dst[types[f0]])
                f0 = f
        for f0, f1, gcam, greg in groups:
            view = dx[f0 * P:]
            ops.colsum(view.as_strided((f1 - f0, C), (P * C, 1)), gcam, accumulate=True)
            ops.colsum(view[1:].as_strided((f1 - f0, 4 * C), (P * C, 1)), greg.reshape(-1), accumulate=True)
        spec_rows = _i32([f * P + t for f in range(S) for t in range(psi)], self.dev)
        zero = self._buf("zero_row", 1, C, F32).zero_()[0]
        ops.scatter_rows(dx, spec_rows, zero, accumulate=False)

    def _dino_backward(self, sc: Scene, embed: EmbedTape, dx: Tensor, dxb: Optional[Tensor]) -> Tensor:
        """DINO's final norm, blocks and tokens -> the grad of the patch embedding's output rows."""
        dino = self.agg.patch_embed
        S, P, R, C, n_patch, psi = sc.S, sc.P, sc.R, self.agg.embed_dim, sc.n_patch, self.agg.patch_start_idx
        g = lambda p: p.grad  # noqa: E731
        dx2 = self._buf("dx2", R, C, F32).zero_()
        ops.layernorm_bwd(embed.prenorm, dx, dino.norm.weight, dino.norm.eps, dx2, dxb=dxb,
                          dw=g(dino.norm.weight), db=g(dino.norm.bias))
        dx = dx2
        for i in reversed(range(len(dino.blocks))):
            blk = dino.blocks[i]
            pb = blk.packed(self.cdt)
            _, bwd = engine.frame_attend_train(pb, S, P)
            engine.block_bwd(pb, self._bwd_pack(blk, self.cdt), engine.block_grads(blk), self._tapes[("dino", i)],
                             dx, dxb, bwd, None, self._sc, tag="dino")
            self._ready(blk)
        # cls + pos[0] (row 0), registers (rows 1..4), patches + pos[1:] (vision_transformer.py:242-259)
        ops.colsum(dx.as_strided((S, C), (P * C, 1)), dino.cls_token.grad.reshape(-1), accumulate=True)
        ops.colsum(dx.as_strided((S, C), (P * C, 1)), dino.pos_embed.grad[0, 0], accumulate=True)
        ops.colsum(dx[1:].as_strided((S, 4 * C), (P * C, 1)), dino.register_tokens.grad.reshape(-1),
                   accumulate=True)
        if embed.pos_resampled:
            # adjoint of the bicubic resampling: d(pos_embed[1:]) += R^T d(table[1:])
            dtab = self._buf("dpos_tab", n_patch, C, F32)
            ops.colsum(dx[psi:].as_strided((S, n_patch * C), (P * C, 1)), dtab.reshape(-1))
            with torch.enable_grad():
                src = dino.pos_embed.detach()[0, 1:].clone().requires_grad_(True)
                dsrc, = torch.autograd.grad(dino.resample_patch_pos(src, sc.H, sc.W), src, dtab)
            ops.copy2d(dino.pos_embed.grad[0, 1:], dsrc.contiguous(), accumulate=True)
        else:
            ops.colsum(dx[psi:].as_strided((S, n_patch * C), (P * C, 1)),
                       dino.pos_embed.grad[0, 1:].reshape(-1), accumulate=True)
        return dx

    def _patch_backward(self, sc: Scene, embed: EmbedTape, conv, dx: Tensor) -> None:
        """Patch conv as im2col GEMM: dW = dpatch^T cols, db = colsum(dpatch)."""
        agg = self.agg
        S, P, C, n_patch, psi = sc.S, sc.P, agg.embed_dim, sc.n_patch, agg.patch_start_idx
        prow = _i32([f * P + psi + p for f in range(S) for p in range(n_patch)], self.dev)
        dpatch = self._buf("dpatch", S * n_patch, C, F32)
        ops.copy_rows(dpatch, dx, S * n_patch, rowmap=prow)
        kk, kpad = 3 * agg.patch_size ** 2, embed.cols.shape[1]
        wtmp = self._buf("dw_patch", C, kpad, F32)
        if self.cdt == BF16:
            dpb = self._buf("dpatch_b", S * n_patch, C, BF16)
            ops.cast_bf16(dpatch, dpb)
            if kpad % 128:
                raise NotImplementedError("patch wgrad needs the im2col width to be a multiple of 128")
            ops.gemm_wgrad(dpb, embed.cols, wtmp, tag="patch.wgrad")
        else:
            ops.wgrad_small(dpatch, embed.cols, wtmp)
        ops.copy2d(conv.weight.grad.reshape(C, kk), wtmp[:, :kk], accumulate=True)
        if conv.bias is not None:
            ops.colsum(dpatch, conv.bias.grad, accumulate=True)
