"""Aggregator — MI355X-native re-design of sailrecon/models/aggregator.py.

Same constructor arguments, parameter names and ``forward(images, no_reloc_list,
reloc_list, fix_rank)`` contract as the reference (aggregator.py:62-85, 242-433).

Layout (SURVEY §7 design stance):
  * ONE fp32 residual buffer x [B*S*P, C] for the whole forward; frames are ordered
    internally as [anchors (no_reloc_list order) ; queries (reloc_list order)] per
    batch item, so the global stack is the contiguous anchor slice and the reloc
    stack the contiguous query slice — no torch.ones + scatter reassembly
    (aggregator.py:393-399) and no dense (S*P)^2 mask (aggregator.py:302-311);
  * every Block is the 7-launch HIP sequence of runtime.run_block;
  * the anchor subsample (aggregator.py:580-626) is a row map: its LayerNorm reads
    the selected rows directly and only their K/V are projected (their query rows
    are discarded by the reference, aggregator.py:737);
  * global_reloc attention = segment 0 (shared anchor subsample K/V) + segment 1
    (own frame), exactly the reference mask's allowed set;
  * subsample draws replay the reference generator order (layer -> batch -> anchor,
    ``randperm(n_patch, generator)[:rank]``) on the host while the GPU runs DINO.
"""

from __future__ import annotations

import logging
import os
from dataclasses import dataclass
from functools import partial
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops, runtime
from ..frame_dedup import group_frames
from ..layers import PatchEmbed
from ..layers.block import Block
from ..layers.rope import PositionGetter, RotaryPositionEmbedding2D
from ..layers.vision_transformer import vit_base, vit_giant2, vit_large, vit_small

logger = logging.getLogger(__name__)

_RESNET_MEAN = [0.485, 0.456, 0.406]
_RESNET_STD = [0.229, 0.224, 0.225]


@dataclass
class _LayerCtx:
    """What one forward's alternating layers share, then (``l`` on) what the caller sets per layer.  x orders
    each batch item's frames as [Na_l anchors ; Nq_l queries] of P rows each; ``a_counts`` = anchor frames
    per rank of the ``G`` ranks of ``group`` (this one: r); Pp = subsample rows per anchor frame."""
    x: torch.Tensor
    sc: runtime.BlockScratch
    P: int
    Pp: int
    rope: Optional[tuple]
    posctx: dict
    dtype: torch.dtype
    dev: object
    Na_l: int
    Nq_l: int
    group: object = None
    G: int = 1
    r: int = 0
    a_counts: tuple = (0,)
    rowmap_t: Optional[torch.Tensor] = None       # [depth, B, Na_l * Pp] subsample rows of x, where wanted
    fill_cache: bool = False                      # keep every layer's anchor-subsample K|V (kv_cache)
    l: int = 0
    pr: Optional[runtime.PackedBlock] = None      # global_reloc block (query rows)
    pg: Optional[runtime.PackedBlock] = None      # global block (anchor rows)
    defer: bool = False                           # leave the blocks' fc2 residuals pending

    def rows(self, b: int) -> Tuple[int, int, int]:
        """(a0, q0, q1): batch item b's anchor rows [a0, q0) and query rows [q0, q1) of x."""
        a0 = b * (self.Na_l + self.Nq_l) * self.P
        return a0, a0 + self.Na_l * self.P, a0 + (self.Na_l + self.Nq_l) * self.P


class Aggregator(nn.Module):
    def __init__(self, img_size=518, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0,
                 num_register_tokens=4, block_fn=Block, qkv_bias=True, proj_bias=True, ffn_bias=True,
                 patch_embed="dinov2_vitl14_reg", aa_order=["frame", "global"], aa_block_size=1, qk_norm=True,
                 rope_freq=100, init_values=0.01, intermediate_layer_idx=[4, 11, 17, 23], min_rank: int = 150,
                 kv_cache: bool = False):
        super().__init__()
        if list(aa_order) != ["frame", "global"] or aa_block_size != 1:
            raise NotImplementedError("the SailRecon hot path uses aa_order=['frame','global'], aa_block_size=1")
        self.__build_patch_embed__(patch_embed, img_size, patch_size, num_register_tokens, embed_dim=embed_dim)
        self.rope = RotaryPositionEmbedding2D(frequency=rope_freq) if rope_freq > 0 else None
        self.position_getter = PositionGetter() if self.rope is not None else None
        self.intermediate_layer_idx = intermediate_layer_idx
        # BASELINE C5 "fp8 QKV": the global blocks' q.k^T in block-scaled e4m3 (ops.attention_qk8);
        # opt-in (set_fp8_global or SR_FP8_GLOBAL=1), no reference output pins its precision
        self.fp8_global = os.environ.get("SR_FP8_GLOBAL", "0") in ("1", "qkv")
        self.fp8_v = os.environ.get("SR_FP8_GLOBAL", "0") == "qkv"
        self._fp8_ws = None
        # frame sharding: global attention starts on the local anchors' K/V while the remote
        # anchors' K/V are still being gathered, then merges the two passes by their LSEs
        # (SR_SHARD_OVERLAP=0: wait for the gather, one pass over every anchor)
        self.shard_overlap = os.environ.get("SR_SHARD_OVERLAP", "1") != "0"

        def blocks(cache=False):
            return nn.ModuleList([block_fn(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                           proj_bias=proj_bias, ffn_bias=ffn_bias, init_values=init_values,
                                           qk_norm=qk_norm, rope=self.rope, kv_cache=cache) for _ in range(depth)])

        self.frame_blocks = blocks()
        self.global_blocks = blocks()
        self.global_reloc_blocks = blocks(kv_cache)
        self.depth = depth
        self.aa_order = aa_order
        self.patch_size = patch_size
        self.aa_block_size = aa_block_size
        self.aa_block_num = depth // aa_block_size
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.camera_token = nn.Parameter(torch.randn(1, 2, 1, embed_dim))
        self.register_token = nn.Parameter(torch.randn(1, 2, num_register_tokens, embed_dim))
        self.camera_token_reloc = nn.Parameter(torch.randn(1, 1, 1, embed_dim))
        self.register_token_reloc = nn.Parameter(torch.randn(1, 1, num_register_tokens, embed_dim))
        self.patch_start_idx = 1 + num_register_tokens
        self.num_register_tokens = num_register_tokens
        for p in (self.camera_token, self.register_token, self.camera_token_reloc, self.register_token_reloc):
            nn.init.normal_(p, std=1e-6)
        for name, value in (("_resnet_mean", _RESNET_MEAN), ("_resnet_std", _RESNET_STD)):
            self.register_buffer(name, torch.FloatTensor(value).view(1, 1, 3, 1, 1), persistent=False)
        self.min_rank = min_rank
        self.use_reentrant = False
        self.generator = self._generate_per_rank_generator()
        # None: follow autocast (bf16 under torch.autocast, exact fp32 otherwise)
        self.compute_dtype: Optional[torch.dtype] = None
        self._ws = runtime.Workspace()
        self._packed: Dict[Tuple[str, torch.dtype], object] = {}
        self.last_subsample_indices: Optional[torch.Tensor] = None
        # two-phase relocalisation (attention.py:40-100, aggregator.py:435-578): anchor-subsample
        # K|V of every global_reloc layer, kept in HBM (the reference round-trips it via the CPU)
        self.kv_cache = kv_cache
        self._kv_cache_layers: Optional[List[torch.Tensor]] = None
        # (frames, distinct frames the DINO stack ran on) of the last _embed, and its cached tables
        self.last_frame_groups: Optional[Tuple[int, int]] = None
        self._rep_host: Optional[torch.Tensor] = None
        self._dedup_tables = None

    # ------------------------------------------------------------------ construction
    def __build_patch_embed__(self, patch_embed, img_size, patch_size, num_register_tokens,
                              interpolate_antialias=True, interpolate_offset=0.0, block_chunks=0, init_values=1.0,
                              embed_dim=1024):
        """aggregator.py:196-240."""
        if "conv" in patch_embed:
            self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=3, embed_dim=embed_dim)
        else:
            vit_models = {"dinov2_vitl14_reg": vit_large, "dinov2_vitb14_reg": vit_base,
                          "dinov2_vits14_reg": vit_small, "dinov2_vitg2_reg": vit_giant2}
            self.patch_embed = vit_models[patch_embed](img_size=img_size, patch_size=patch_size,
                                                       num_register_tokens=num_register_tokens,
                                                       interpolate_antialias=interpolate_antialias,
                                                       interpolate_offset=interpolate_offset,
                                                       block_chunks=block_chunks, init_values=init_values)
            if hasattr(self.patch_embed, "mask_token"):
                self.patch_embed.mask_token.requires_grad_(False)

    def _generate_per_rank_generator(self):
        """aggregator.py:628-641.  Multi-GPU sharding (parallel.py) uses ONE draw
        sequence on every rank instead of per-rank seeds, so results do not depend on
        the world size (SURVEY §7 hard parts)."""
        seed = torch.randint(0, 2 ** 32, (1,)).item()
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        g = torch.Generator()
        g.manual_seed(seed + rank)
        return g

    def invalidate_packed(self):
        """Call after changing parameters in place (load_state_dict does it automatically)."""
        self._packed.clear()
        for m in self.modules():
            if isinstance(m, Block):
                m.invalidate_packed()

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super()._load_from_state_dict(*args, **kwargs)

    def _pack_misc(self, dtype: torch.dtype, kpad: int):
        key = ("misc", dtype, kpad)
        if key not in self._packed:
            pe = self.patch_embed
            conv = pe.patch_embed.proj if hasattr(pe, "blocks") else pe.proj
            C = conv.weight.shape[0]
            w = conv.weight.detach().reshape(C, -1).float()
            wp = torch.zeros(C, kpad, device=w.device, dtype=torch.float32)
            wp[:, : w.shape[1]] = w
            nreg = self.num_register_tokens
            table = torch.empty(3, 1 + nreg, C, device=w.device, dtype=torch.float32)
            table[0, 0] = self.camera_token[0, 0, 0]
            table[1, 0] = self.camera_token[0, 1, 0]
            table[2, 0] = self.camera_token_reloc[0, 0, 0]
            table[0, 1:] = self.register_token[0, 0]
            table[1, 1:] = self.register_token[0, 1]
            table[2, 1:] = self.register_token_reloc[0, 0]
            self._packed[key] = dict(w_patch=wp.to(dtype).contiguous(), b_patch=conv.bias.detach().float().contiguous(),
                                     special=table.detach().contiguous())
        return self._packed[key]

    # ------------------------------------------------------------------ subsample draws
    def draw_subsample(self, depth: int, B: int, na: int, n_patch: int, rank: int) -> np.ndarray:
        """Replays random_select_features' draws (aggregator.py:339,351-357,617-621):
        order layer -> batch -> anchor, ``randperm(n_patch, generator)[:rank]``."""
        out = np.empty((depth, B, na, rank), dtype=np.int64)
        for l in range(depth):
            for b in range(B):
                for a in range(na):
                    out[l, b, a] = torch.randperm(n_patch, generator=self.generator)[:rank].numpy()
        return out

    def plan_subsample(self, fix_rank: Optional[int], B: int, na: int, n_patch: int) -> np.ndarray:
        """The forward's draws in the reference's order (aggregator.py:580-626): the rank (``fix_rank``
        clipped to the patch count, else drawn), then every layer's selection -> [depth, B, na, rank];
        sets ``rank`` and ``last_subsample_indices``.  The inference and the training forward both
        draw here, so the generator advances identically on either path."""
        if fix_rank is not None:
            self.rank = min(fix_rank, n_patch)
        else:
            lo, hi = min(self.min_rank, n_patch // 2), max(self.min_rank, n_patch // 2)
            self.rank = int(torch.randint(lo, hi, (1,), generator=self.generator).item())
        idx = self.draw_subsample(self.depth, B, na, n_patch, self.rank)
        self.last_subsample_indices = torch.from_numpy(idx)
        return idx

    # ------------------------------------------------------------------ multi-GPU
    def set_frame_sharding(self, group=None):
        """Shard frames across the ranks of ``group`` (torch.distributed, RCCL on ROCm).

        Rank r of G owns a contiguous, balanced slice of no_reloc_list and of reloc_list
        (``shard_range``: counts differ by at most one; uneven splits are exact, no padded
        frames ever enter a softmax).  DINO, frame blocks, subsampling and every per-token GEMM
        stay local; the global block all-gathers K/V of the anchors (attending to the local
        anchors while the gather is in flight, then to the remote ones, merged by LSE), the
        global_reloc block all-gathers the anchor-subsample K/V, and the camera head runs
        replicated on gathered camera tokens.  Every rank needs >= 1 anchor;
        a rank may own no query frame.  The subsample generator is re-seeded identically on every
        rank (broadcast from rank 0) so the draws do not depend on the world size.
        ``group=None`` disables sharding."""
        self._shard_group = group
        if isinstance(group, RankSim):  # one rank's workload without peers (timing rehearsal)
            return
        if group is not None:
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
            dist = torch.distributed
            if dist.get_backend(group) == "nccl":
                seed = seed.cuda()
            dist.broadcast(seed, src=dist.get_global_rank(group, 0) if hasattr(dist, "get_global_rank") else 0,
                           group=group)
            self.generator.manual_seed(int(seed.item()))

    def _world(self):
        g = getattr(self, "_shard_group", None)
        if g is None:
            return None, 1, 0
        if isinstance(g, RankSim):
            return g, g.world, g.rank
        return g, torch.distributed.get_world_size(g), torch.distributed.get_rank(g)

    # ------------------------------------------------------------------ forward
    def _embed(self, imgs: torch.Tensor, F_: int, H: int, W: int, ftype_t_fn, dtype) -> Tuple[torch.Tensor, object]:
        """Image normalise + DINO patch embed (+ its blocks and final norm) + aggregator special
        tokens (aggregator.py:267-299): fills the residual stream x [F_*P, C] of the workspace."""
        dev = imgs.device
        C = self.embed_dim
        ps = self.patch_size
        gh, gw = H // ps, W // ps
        n_patch = gh * gw
        psi = self.patch_start_idx
        P = n_patch + psi
        R = F_ * P
        ws = self._ws
        hidden = self.frame_blocks[0].mlp.fc1.out_features
        x = ws.get("x", R, C, torch.float32, dev)
        sc = runtime.scratch(ws, R, C, hidden, dtype, dev)

        # ---- patch embed (+ DINOv2 stack), vision_transformer.py:242-307
        kt = 64 if dtype == torch.bfloat16 else 32
        kpad = -(-3 * ps * ps // kt) * kt
        misc = self._pack_misc(dtype, kpad)
        cols = ws.get("im2col", F_ * n_patch, kpad, dtype, dev)
        is_dino = hasattr(self.patch_embed, "blocks")
        # ---- frame dedup: the DINO stack once per DISTINCT frame (frame_dedup.py).  U frames run on
        # the compact stream xd [U*P, C]; DINO's final norm expands them into x by a row map
        U, fmap, expand = F_, None, None
        if is_dino and _DEDUP_FRAMES and F_ >= 2 and imgs.is_cuda:
            fmap, expand = self._frame_groups(imgs, F_, P)
            U = F_ if fmap is None else fmap.numel()
        self.last_frame_groups = (F_, U)
        xd = x if U == F_ else ws.get("x_dino", U * P, C, torch.float32, dev)
        Rd = U * P
        if fmap is None:
            ops.im2col_normalize(imgs, ps, cols, kpad)
        else:
            ops.im2col_normalize(imgs, ps, cols, kpad, frame_map=fmap)  # the U distinct frames, no gather pass
        if is_dino:
            dino = self.patch_embed
            pos_tab = dino.pos_embed_for(H, W)  # [1 + n_patch, C] fp32
            row_add = pos_tab[1:]
        else:
            row_add = ws.get("zeros_pos", n_patch, C, torch.float32, dev).zero_()
        ops.gemm(cols, misc["w_patch"], xd, _lib.SR_EPI_PATCH, bias=misc["b_patch"], rows=U * n_patch,
                 patch=dict(seg_rows=n_patch, seg_stride=P, seg_offset=psi, row_add=row_add), tag="gemm")
        if is_dino:
            nreg_d = dino.num_register_tokens
            if 1 + nreg_d != psi:
                raise NotImplementedError("DINO register count must equal the aggregator's")
            # DINO's cls (+ its pos-embed row) and register rows, and an all-zero frame-type table:
            # parameter preprocessing, built once per resolution (no torch kernels per forward)
            key = ("dino_tokens", H, W, F_, str(dev), dino.cls_token._version, dino.register_tokens._version,
                   dino.pos_embed._version)
            if key not in self._packed:
                dtab = torch.cat([(dino.cls_token[0, 0] + pos_tab[0])[None], dino.register_tokens[0]], 0)
                self._packed = {k: v for k, v in self._packed.items() if not (isinstance(k, tuple) and
                                                                             k[0] == "dino_tokens")}
                self._packed[key] = (dtab.detach().float().contiguous()[None],
                                     torch.zeros(F_, 1, dtype=torch.int32, device=dev))
            dtab, zero_t = self._packed[key]
            ops.set_special_tokens(xd, U, P, dtab, zero_t)
            pending = []  # fc2 residual of block i folded into block i+1's LN1 (runtime.Pending)
            nblk = len(dino.blocks)
            for i, blk in enumerate(dino.blocks):
                pb = blk.packed(dtype)
                qs = runtime.q_prescale(pb)  # c*q rounded once by the QKV GEMM (runtime.q_prescale)
                p = runtime.run_block(pb, xd, 0, Rd, sc, runtime.frame_attend(pb, U, P, tail_readable=True,
                                                                              q_scaled=qs > 0),
                                      runtime.qkv_params(pb, None, prescale=True), pending=pending,
                                      defer=i < nblk - 1, q_scale=qs)
                if p is not None:
                    pending.append(p)
            assert not pending
            # in place (row-local); deduplicated: x row f*P + t = LN(xd row slot(f)*P + t), the expansion
            ops.layernorm(xd, dino.norm.weight, dino.norm.bias, dino.norm.eps, x, rowmap=expand)

        # ---- aggregator special tokens, aggregator.py:287-299 (type by ORIGINAL frame index)
        ops.set_special_tokens(x, F_, P, misc["special"], ftype_t_fn())
        return x, sc

    def _frame_groups(self, imgs: torch.Tensor, F_: int, P: int):
        """The bit-identical frames among ``imgs`` [F_, 3, H, W] (ops.frame_groups; ONE small pinned
        read-back and stream wait) -> (frame map int32 [U], row map int32 [F_*P]) on the device for
        im2col and the expanding LayerNorm, or (None, None) when every frame is distinct."""
        dev = imgs.device
        rep_d = ops.frame_groups(imgs.view(F_, -1))
        host = self._rep_host
        if host is None or host.numel() < F_:
            host = self._rep_host = torch.empty(max(F_, 64), dtype=torch.int32).pin_memory()
        host[:F_].copy_(rep_d, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        rep = host[:F_].numpy().copy()
        if (rep == np.arange(F_)).all():
            return None, None
        key = (rep.tobytes(), P, str(dev))
        if self._dedup_tables is None or self._dedup_tables[0] != key:  # the same grouping as last time: keep
            uniq, _, rowmap = group_frames(rep, P)
            buf = runtime.to_device(torch.from_numpy(np.concatenate([uniq, rowmap])), dev)
            self._dedup_tables = (key, buf[:len(uniq)], buf[len(uniq):])
        return self._dedup_tables[1], self._dedup_tables[2]

    def forward(self, images: torch.Tensor, no_reloc_list: list, reloc_list: list,
                fix_rank: Union[int, None] = None, *, outputs: str = "all"
                ) -> Tuple[Dict[int, torch.Tensor], int, torch.Tensor]:
        """``outputs="camera"`` (single GPU, no kv_cache, at least one query frame; SR_CAMERA_ONLY=0
        makes it behave as "all"): the caller reads only the camera-token row of every frame's last
        layer (a pose-only SailRecon.forward: aggregator.py:414-423 and camera_head.py's
        ``tokens[:, :, 0]``).  Then no intermediate map is allocated or copied, and the last layer's
        global / global_reloc blocks project K / V for every row but run attention, proj, LN2 and the
        MLP for the camera rows only (_layer_global_camera).  The returned dict is {depth - 1: t,
        -1: t} with t [B, Nq, 1, 2C] -- the shape the frame-sharded path hands the camera head;
        psi and the anchors' camera tokens are as with "all"."""
        if outputs not in ("all", "camera"):
            raise ValueError(f"outputs must be 'all' or 'camera', got {outputs!r}")
        B, S, C_in, H, W = images.shape
        num_recon, num_reloc = len(no_reloc_list), len(reloc_list)
        self.num_recon = num_recon
        if C_in != 3:
            raise ValueError(f"Expected 3 input channels, got {C_in}")
        runtime.require_device(images, "Aggregator")
        check_frame_lists(no_reloc_list, reloc_list, S)
        ps = self.patch_size
        assert H % ps == 0 and W % ps == 0, f"image size {H}x{W} is not a multiple of the patch size {ps}"
        group, G, r = self._world()
        Na, Nq = num_recon, num_reloc
        if self.kv_cache and Nq > 0:
            raise NotImplementedError("a kv_cache aggregator runs anchors only here (SailRecon.tmp_forward) and "
                                      "queries through forward_with_cache (SailRecon.reloc), like the reference")
        fill_cache = self.kv_cache  # anchors-only pass: keep every layer's anchor-subsample K|V
        if G > 1 and (B != 1 or Na < G):
            raise ValueError(f"frame sharding over {G} ranks needs B == 1 and at least one anchor frame per "
                             f"rank (got B={B}, Na={Na})")
        a_start, Na_l = shard_range(Na, G, r)
        q_start, Nq_l = shard_range(Nq, G, r)
        a_counts = [shard_range(Na, G, j)[1] for j in range(G)]
        q_counts = [shard_range(Nq, G, j)[1] for j in range(G)]
        my_anchors = list(no_reloc_list)[a_start:a_start + Na_l]
        my_queries = list(reloc_list)[q_start:q_start + Nq_l]
        S_l = Na_l + Nq_l

        dev = images.device
        dtype = runtime.compute_dtype(self.compute_dtype)
        C, nh = self.embed_dim, self.num_heads
        gh, gw = H // ps, W // ps
        n_patch = gh * gw
        psi = self.patch_start_idx
        P = n_patch + psi
        F_ = B * S_l

        # ---- internal (local) frame order: anchors then queries, per batch item
        order = my_anchors + my_queries
        imgs = images if order == list(range(S)) else images[:, order]
        imgs = imgs.reshape(F_, 3, H, W).float().contiguous()

        need_sub = Nq > 0 or fill_cache
        camera = outputs == "camera" and _CAMERA_ONLY and G == 1 and not self.kv_cache and Nq > 0
        if fill_cache and B != 1:
            raise NotImplementedError("kv_cache needs B == 1 (aggregator.py:452)")
        host = {}

        def host_tables():
            """Every per-forward host table in ONE pinned H2D copy, built once _embed has queued its GPU
            work (so the subsample draws overlap DINO): the frame types (aggregator.py:287-299, by
            ORIGINAL frame index), the anchors' camera-token rows and the per-layer subsample row maps
            (aggregator.py:277-285, 580-626).  Returns the frame-type view."""
            # the reference draws at every layer even without queries (select_scene_repe_for_reloc,
            # aggregator.py:351-357), so the generator advances identically
            idx = self.plan_subsample(fix_rank, B, Na, n_patch)  # every rank draws all anchors
            Pp = min(self.rank + psi, P)
            ftype = np.array(sum(([0 if a == 0 else 1 for a in my_anchors] + [2] * Nq_l for _ in range(B)), []),
                             dtype=np.int32)
            anchors, queries = camera_row_tables(B, Na_l, Nq_l, P)
            if not camera:
                queries = queries[:0]
            parts = [ftype, anchors, queries]
            if need_sub:  # this rank's anchors
                parts.append(subsample_rowmap(idx[:, :, a_start:a_start + Na_l], S_l, P, psi).reshape(-1))
            buf = runtime.to_device(torch.from_numpy(np.concatenate(parts)), dev)
            n0, n1 = len(ftype), len(ftype) + len(anchors)
            n2 = n1 + len(queries)
            host.update(Pp=Pp, anchor_rows0=buf[n0:n1], query_rows0=buf[n1:n2],
                        rowmap_t=buf[n2:].view(self.depth, B, Na_l * Pp) if need_sub else None)
            return buf[:n0]

        x, sc = self._embed(imgs, F_, H, W, ftype_t_fn=host_tables, dtype=dtype)
        Pp, rowmap_t, anchor_rows0 = host["Pp"], host["rowmap_t"], host["anchor_rows0"]
        query_rows0 = host["query_rows0"]
        if fill_cache:
            self._kv_cache_layers = [None] * self.depth
        rope = self.rope.tables(C // nh, max(gh, gw) + 1, dev) if self.rope is not None else None
        ctx = _LayerCtx(x=x, sc=sc, P=P, Pp=Pp, rope=rope, posctx=dict(tokens_per_frame=P, patch_start=psi, grid_w=gw),
                        dtype=dtype, dev=dev, Na_l=Na_l, Nq_l=Nq_l, group=group, G=G, r=r, a_counts=a_counts,
                        rowmap_t=rowmap_t, fill_cache=fill_cache)

        # ---- outputs (this rank's query frames)
        out_maps: Dict[int, torch.Tensor] = {}
        if Nq > 0 and not camera:
            for l in self.intermediate_layer_idx:
                out_maps[l] = torch.empty(B, Nq_l, P, 2 * C, device=dev, dtype=torch.float32)
        # camera mode: the queries' camera tokens only (frame half | reloc half), no maps
        qcam = torch.empty(B, Nq_l, 1, 2 * C, device=dev, dtype=torch.float32) if camera else None
        qcam_flat = qcam.view(B * Nq_l, 2 * C) if camera else None
        cam_loc = torch.empty(B, Na_l, 2 * C, device=dev, dtype=torch.float32)
        cam_flat = cam_loc.view(B * Na_l, 2 * C)

        # ---- alternating layers, aggregator.py:339-423
        pending = []  # the global / reloc blocks' fc2 residuals, folded into the next frame block's LN1
        for l in range(self.depth):
            self._frame_block(ctx, l, F_, pending)
            if l in out_maps and Nq_l > 0:  # frame half of the intermediate, :403-413
                self._copy_query_half(ctx, out_maps[l], 0)
            if l == self.depth - 1:  # :414-423 frame half
                ops.copy_rows(cam_flat[:, :C], x, B * Na_l, rowmap=anchor_rows0)
                if camera:
                    ops.copy_rows(qcam_flat[:, :C], x, B * Nq_l, rowmap=query_rows0)
            ctx.l, ctx.pr, ctx.pg = l, self.global_reloc_blocks[l].packed(dtype), self.global_blocks[l].packed(dtype)
            # the next reader of x after this layer's global / reloc blocks is the next frame block's LN1,
            # unless an output map or the camera tokens copy x first
            ctx.defer = l + 1 < self.depth and l not in out_maps and not fill_cache and not _concurrent_stacks()
            if camera and l == self.depth - 1:
                # x is dead after this layer: only the camera rows' tails run, on a compact stream
                for b in range(B):
                    self._layer_global_camera(ctx, b, anchor_rows0, query_rows0, cam_flat, qcam_flat)
                break
            for b in range(B):
                pending += self._layer_global(ctx, b)
            if l in out_maps and Nq_l > 0:  # reloc half
                self._copy_query_half(ctx, out_maps[l], 1)
            if l == self.depth - 1:
                ops.copy_rows(cam_flat[:, C:], x, B * Na_l, rowmap=anchor_rows0)

        output_dict: Dict[int, torch.Tensor] = dict(out_maps)
        if camera:
            output_dict[self.depth - 1] = qcam
        assert (self.depth - 1 in output_dict) or Nq == 0, \
            f"Please make sure the last layer ({self.depth - 1}) is in the output_dict: {output_dict.keys()}"
        if Nq > 0:
            output_dict[-1] = output_dict[self.depth - 1]
        if G > 1:
            # camera head inputs for every frame: anchor camera tokens and query camera tokens
            cam_last = torch.empty(B * Na, 2 * C, device=dev, dtype=torch.float32)
            works = gather_rows(cam_last, cam_loc.view(B * Na_l, 2 * C), a_counts, group, r)
            if Nq > 0:
                qcam = torch.empty(B * Nq, 2 * C, device=dev, dtype=torch.float32)
                works += gather_rows(qcam, output_dict[-1][:, :, 0].reshape(B * Nq_l, 2 * C).contiguous(), q_counts,
                                     group, r)
                self.last_query_cam_tokens = qcam.view(B, Nq, 2 * C)
            for w in works:
                w.wait()
            cam_last = cam_last.view(B, Na, 2 * C)
        else:
            cam_last = cam_loc
            self.last_query_cam_tokens = output_dict[-1][:, :, 0] if Nq > 0 else None
        return output_dict, self.patch_start_idx, cam_last

    # ------------------------------------------------------------------ two-phase relocalisation
    def clear_kv_cache(self) -> None:
        """attention.py:48-60 for every global_reloc block."""
        self._kv_cache_layers = None

    def forward_with_cache(self, images: torch.Tensor, cameras: torch.Tensor = None, camera_dropout: float = False,
                           fix_rank: Union[int, None] = None) -> Tuple[Dict[int, torch.Tensor], int]:
        """aggregator.py:435-578: relocalise query frames against the anchors cached by an
        anchors-only ``forward`` of a ``kv_cache=True`` aggregator.  Every frame of ``images``
        is a query: reloc special tokens, frame blocks, and per layer the global_reloc block
        over [cached anchor-subsample K|V ; the frame's own tokens] (the reference's cache
        concatenation + block mask, attention.py:80-100, aggregator.py:497-509).  Returns
        (output_dict {inter layers, -1: [1, S, P, 2C]}, patch_start_idx)."""
        B, S, C_in, H, W = images.shape
        assert B == 1, "Batch size must be 1 for this model"
        if C_in != 3:
            raise ValueError(f"Expected 3 input channels, got {C_in}")
        runtime.require_device(images, "Aggregator.forward_with_cache")
        if self._kv_cache_layers is None or any(t is None for t in self._kv_cache_layers):
            raise RuntimeError("forward_with_cache needs a filled cache: run the anchors-only forward first "
                               "(SailRecon.tmp_forward)")
        if self._world()[1] > 1:
            raise NotImplementedError("forward_with_cache under frame sharding")
        ps = self.patch_size
        assert H % ps == 0 and W % ps == 0, f"image size {H}x{W} is not a multiple of the patch size {ps}"
        if fix_rank is not None:
            self.rank = fix_rank
        dev = images.device
        dtype = runtime.compute_dtype(self.compute_dtype)
        if self._kv_cache_layers[0].dtype != dtype:
            raise RuntimeError(f"the cache was built in {self._kv_cache_layers[0].dtype}, this pass computes in "
                               f"{dtype}: run both phases under the same autocast setting")
        C, nh = self.embed_dim, self.num_heads
        gh, gw = H // ps, W // ps
        psi = self.patch_start_idx
        P = gh * gw + psi
        F_ = S
        imgs = images.reshape(F_, 3, H, W).float().contiguous()
        x, sc = self._embed(imgs, F_, H, W, ftype_t_fn=lambda: torch.full((F_,), 2, device=dev, dtype=torch.int32),
                            dtype=dtype)
        rope = self.rope.tables(C // nh, max(gh, gw) + 1, dev) if self.rope is not None else None
        # every frame is a query: no anchor rows, no subsample of its own
        ctx = _LayerCtx(x=x, sc=sc, P=P, Pp=0, rope=rope, posctx=dict(tokens_per_frame=P, patch_start=psi, grid_w=gw),
                        dtype=dtype, dev=dev, Na_l=0, Nq_l=F_)
        out_maps = {l: torch.empty(1, S, P, 2 * C, device=dev, dtype=torch.float32) for l in self.intermediate_layer_idx}
        for l in range(self.depth):
            self._frame_block(ctx, l, F_)
            if l in out_maps:
                self._copy_query_half(ctx, out_maps[l], 0)
            ctx.pr = pr = self.global_reloc_blocks[l].packed(dtype)
            # the cache is a clone(), not a padded Workspace buffer: its tail is not declared readable
            runtime.run_block(pr, x, 0, F_ * P, sc, partial(self._reloc_one_launch, ctx, self._kv_cache_layers[l]),
                              self._epi(ctx, pr, 0), q_scale=runtime.q_prescale(pr))
            if l in out_maps:
                self._copy_query_half(ctx, out_maps[l], 1)
        assert self.depth - 1 in out_maps, \
            f"Please make sure the last layer ({self.depth - 1}) is in the output_dict: {out_maps.keys()}"
        output_dict: Dict[int, torch.Tensor] = dict(out_maps)
        output_dict[-1] = output_dict[self.depth - 1]
        return output_dict, self.patch_start_idx

    # ------------------------------------------------------------------ stacks
    def _epi(self, ctx: _LayerCtx, pb, row_base: int) -> Optional[dict]:
        """QKV epilogue of block ``pb`` over x rows from ``row_base`` on (its Q block leaves as c*q)."""
        return runtime.qkv_params(pb, ctx.rope, prescale=True, pos_row_base=row_base, **ctx.posctx)

    def _kv_epi(self, ctx: _LayerCtx, pb, **pos) -> Optional[dict]:
        """Epilogue of a K/V-only projection (runtime.kv_gemm); ``pos``: pos_rowmap= or pos_row_base=."""
        return runtime.kv_params(pb, ctx.rope, **pos, **ctx.posctx)

    def _frame_block(self, ctx: _LayerCtx, l: int, frames: int, pending: Optional[list] = None) -> None:
        """Frame block l over every row of x (``pending``: residual updates its LN1 folds in)."""
        pb = self.frame_blocks[l].packed(ctx.dtype)
        runtime.run_block(pb, ctx.x, 0, frames * ctx.P, ctx.sc,
                          runtime.frame_attend(pb, frames, ctx.P, tail_readable=True, q_scaled=_qs(pb)),
                          self._epi(ctx, pb, 0), pending=pending, q_scale=runtime.q_prescale(pb))

    def _copy_query_half(self, ctx: _LayerCtx, out_map: torch.Tensor, half: int) -> None:
        """x's query rows -> the frame (0) or reloc (1) half of an intermediate map [B, Nq_l, P, 2C]."""
        C = self.embed_dim
        for b in range(out_map.shape[0]):
            _, q0, q1 = ctx.rows(b)
            ops.copy_rows(out_map[b].view(q1 - q0, 2 * C)[:, half * C:(half + 1) * C], ctx.x[q0:q1], q1 - q0)

    def _layer_global(self, ctx: _LayerCtx, b: int) -> list:
        """global_reloc (queries, aggregator.py:672-741) + global (anchors, :743-769) blocks of one layer
        for one batch item, by one of three executors (each returns what run_block / run_block_tail(s)
        gave it).  Returns the fc2 residuals left pending for the next LN1 (ctx.defer; else [])."""
        a0, q0, q1 = ctx.rows(b)
        paired = ctx.G == 1 and self._paired_attention(ctx.pr, ctx.pg, ctx.dtype, q1 - q0, q0 - a0, ctx.Na_l * ctx.Pp)
        run = self._layer_sharded if ctx.G > 1 else self._layer_paired if paired else self._layer_plain
        return [p for p in run(ctx, b) if p is not None]

    def _subsample_kv(self, ctx: _LayerCtx, b: int, project: bool = True):
        """Anchor-subsample K/V (reads x before the global block updates the anchors): row-mapped LN1, the
        projection unless the caller groups it, the gather, the cache's copy -> (xn_sub, kv_sub_all, works)."""
        pr, ws, C, G = ctx.pr, self._ws, ctx.pr.dim, ctx.G
        n_sub = ctx.Na_l * ctx.Pp                  # local anchor-subsample rows
        xn_sub = ws.get("xn_sub", n_sub, C, ctx.dtype, ctx.dev)
        if G > 1:  # separate send buffer: no aliasing between collective input and output
            kv_sub = ws.get("kv_sub_loc", n_sub, 2 * C, ctx.dtype, ctx.dev)
            kv_sub_all = ws.get("kv_sub", sum(ctx.a_counts) * ctx.Pp, 2 * C, ctx.dtype, ctx.dev)
        else:
            kv_sub = kv_sub_all = ws.get("kv_sub", n_sub, 2 * C, ctx.dtype, ctx.dev)
        rowmap = ctx.rowmap_t[ctx.l, b]
        ops.layernorm(ctx.x, pr.ln1_w, pr.ln1_b, pr.eps, xn_sub, rowmap=rowmap, rows=n_sub)
        if project:
            runtime.kv_gemm(pr, xn_sub, kv_sub, self._kv_epi(ctx, pr, pos_rowmap=rowmap))
        work = gather_rows(kv_sub_all, kv_sub, [c * ctx.Pp for c in ctx.a_counts], ctx.group, ctx.r) if G > 1 else []
        if ctx.fill_cache:  # two-phase reloc: every anchor's subsample K|V of this layer
            _wait(work)
            self._kv_cache_layers[ctx.l] = kv_sub_all.clone()
        return xn_sub, kv_sub_all, work

    def _project_heads(self, ctx: _LayerCtx, b: int) -> torch.Tensor:
        """LN1 + QKV projection of the reloc (query rows) and global (anchor rows) blocks and the subsample
        K/V projection: ONE grouped GEMM launch where all are eligible, else block by block -> kv_sub."""
        pr, pg, x, sc, C = ctx.pr, ctx.pg, ctx.x, ctx.sc, ctx.pg.dim
        a0, q0, q1 = ctx.rows(b)
        xn_sub, kv_sub, _ = self._subsample_kv(ctx, b, project=False)
        epi_r, epi_g = self._epi(ctx, pr, q0), self._epi(ctx, pg, a0)
        epi_s = self._kv_epi(ctx, pr, pos_rowmap=ctx.rowmap_t[ctx.l, b])
        probs = [dict(a=sc.xn[q0:q1], w=pr.w_qkv, out=sc.qkv[q0:q1], bias=pr.b_qkv, qkv=epi_r),
                 dict(a=sc.xn[a0:q0], w=pg.w_qkv, out=sc.qkv[a0:q0], bias=pg.b_qkv, qkv=epi_g),
                 dict(a=xn_sub, w=pr.w_qkv[C:], out=kv_sub, bias=_sl(pr.b_qkv, C, 3 * C), qkv=epi_s)]
        if all(p_["qkv"] is not None for p_ in probs) and ops.gemm_group_eligible(probs):
            ops.layernorm(x[q0:q1], pr.ln1_w, pr.ln1_b, pr.eps, sc.xn[q0:q1])
            ops.layernorm(x[a0:q0], pg.ln1_w, pg.ln1_b, pg.eps, sc.xn[a0:q0])
            ops.gemm_group(probs, _lib.SR_EPI_QKV, tag="gemm")
        else:
            runtime.run_block_head(pr, x, q0, q1, sc, epi_r, runtime.q_prescale(pr))
            runtime.run_block_head(pg, x, a0, q0, sc, epi_g, runtime.q_prescale(pg))
            runtime.kv_gemm(pr, xn_sub, kv_sub, epi_s)
        return kv_sub

    def _reloc_attention(self, ctx: _LayerCtx, kv_sub_all, work_sub: list, qkv, o, pair: Optional[dict] = None) -> None:
        """The reloc block's attention (run_block's ``attend``; ``work_sub``: the subsample's gather): one
        launch, or (_split_reloc) two passes merged by their LSEs (the union of the two key sets, exactly):
        every query row against the shared anchor subsample's whole 64-key tiles as ONE long query set (the
        hand-scheduled sweep, sr_attn.hip; in ops.attention_pair's launch behind ``pair``, the global
        attention), then each query frame against the subsample's last partial tile (shared segment 0) and
        itself (segment 1) on the compiled sweep, whose epilogue folds the first pass in (sr_attn_desc.merge_o)."""
        _wait(work_sub)
        pr, pg, C, rows, n_sub_all = ctx.pr, ctx.pg, ctx.pr.dim, qkv.shape[0], kv_sub_all.shape[0]
        if not self._split_reloc(ctx.dtype, rows, n_sub_all):
            self._reloc_one_launch(ctx, kv_sub_all, qkv, o, tail_readable=True)
            return
        n_full = n_sub_all // 64 * 64
        kb, qb = runtime.key_norm_bound(pr), runtime.query_norm_bound(pr)
        o_a, lse_a = ops.key_split_workspace(ctx.dev, 1, rows, C, pr.heads, name="reloc_split")
        lse_a = lse_a[0]
        sub = dict(lq=rows, l0=n_full, key_norm_max=kb, query_norm_max=qb, lse=lse_a.view(-1), q_scaled=_qs(pr))
        q, k0, v0 = qkv[:, 0:C], kv_sub_all[:n_full, 0:C], kv_sub_all[:n_full, C:2 * C]
        if pair is None:
            ops.attention(q, k0, v0, o_a, heads=pr.heads, head_dim=pr.head_dim, batch=1, q_bstride=0, k0_bstride=0,
                          tag="attn_reloc", tail_readable=True, **sub)
        else:
            sub.update(q=q, k0=k0, v0=v0, o=o_a)
            if ops.PAIR_VT:
                # both problems' V as pre-transposed tiles: one ds_read_b128 per P.V fragment in the sweep
                for p_, name, blk in ((pair, "vt_g", pg), (sub, "vt_s", pr)):
                    p_["vt"] = ops.vt_tiles(p_["v0"], p_["l0"], blk.heads, self._ws.get(
                        name, *ops.vt_tile_shape(p_["l0"], blk.heads), ctx.dtype, ctx.dev), tag="vt_tiles")
            ops.attention_pair(pair, sub, heads=pg.heads, head_dim=pg.head_dim, tag="attn_global")
        if n_full < n_sub_all:
            self._reloc_one_launch(ctx, kv_sub_all[n_full:], qkv, o, tail_readable=True, merge_o=o_a, merge_lse=lse_a)
        else:
            ops.attention(q, qkv[:, C:2 * C], qkv[:, 2 * C:3 * C], o, heads=pr.heads, head_dim=pr.head_dim,
                          batch=ctx.Nq_l, lq=ctx.P, q_bstride=ctx.P, l0=ctx.P, k0_bstride=ctx.P, tag="attn_reloc",
                          key_norm_max=kb, query_norm_max=qb, tail_readable=True, merge_o=o_a, merge_lse=lse_a,
                          q_scaled=_qs(pr))

    def _reloc_one_launch(self, ctx: _LayerCtx, kv, qkv, o, **more) -> None:
        """Each query frame against the shared subsample K|V rows ``kv`` and itself.  ``more``: tail_readable=True
        where ``kv`` is in a padded Workspace buffer (a kv-cache clone is not), merge_o= / merge_lse= to fold in."""
        pr, C, P = ctx.pr, ctx.pr.dim, ctx.P
        ops.attention(qkv[:, 0:C], kv[:, 0:C], kv[:, C:2 * C], o, heads=pr.heads, head_dim=pr.head_dim,
                      batch=ctx.Nq_l, lq=P, q_bstride=P, l0=kv.shape[0], k0_bstride=0, k1=qkv[:, C:2 * C],
                      v1=qkv[:, 2 * C:3 * C], l1=P, k1_bstride=P, tag="attn_reloc",
                      key_norm_max=runtime.key_norm_bound(pr), query_norm_max=runtime.query_norm_bound(pr),
                      q_scaled=_qs(pr), **more)

    def _layer_paired(self, ctx: _LayerCtx, b: int) -> list:
        """G == 1, bf16 (_paired_attention): the queries' and anchors' QKV projections and the
        anchor-subsample K/V one as ONE grouped GEMM launch (the subsample's LayerNorm still reads x
        first, before the global block updates it), then the global block's attention (anchors against
        themselves) and the split reloc block's subsample pass (queries against the anchor
        subsample) in ONE launch of the hand-scheduled sweep (sr_attention_pair): each time the
        second problem fills the CUs the first one's last workgroup round leaves idle; then the
        reloc own-frame pass folds the subsample pass in, and both blocks' tails follow.  (Pairing
        needs query rows: the subsample is wanted and no cache is being filled.)"""
        pr, pg, x, sc, C = ctx.pr, ctx.pg, ctx.x, ctx.sc, ctx.pg.dim
        a0, q0, q1 = ctx.rows(b)
        La = q0 - a0  # anchor tokens
        kv_sub = self._project_heads(ctx, b)
        qkv_r, qkv_g = sc.qkv[q0:q1], sc.qkv[a0:q0]
        pa = dict(q=qkv_g[:, 0:C], k0=qkv_g[:, C:2 * C], v0=qkv_g[:, 2 * C:3 * C], o=sc.o[a0:q0], lq=La, l0=La,
                  key_norm_max=runtime.key_norm_bound(pg), query_norm_max=runtime.query_norm_bound(pg),
                  q_scaled=_qs(pg))
        self._reloc_attention(ctx, kv_sub, [], qkv_r, sc.o[q0:q1], pair=pa)
        items = [(pr, q0, q1), (pg, a0, q0)]
        if runtime.group_tails_wanted(max(q1 - q0, La)):
            return runtime.run_block_tails(items, x, sc, defer=ctx.defer)
        return [runtime.run_block_tail(blk, x, r0, r1, sc, defer=ctx.defer) for blk, r0, r1 in items]

    def _layer_plain(self, ctx: _LayerCtx, b: int) -> list:
        """G == 1, unpaired: the reloc block (query rows) and the global block (anchor rows), one
        after the other through runtime.run_block; they are independent.
        SR_CONCURRENT_STACKS=1 runs the reloc block on a side stream so that each could fill the
        other's last partial wave.  Round 1: 3% SLOWER at N=32 (68.7 -> 66.7 views/s).  Round 3,
        with the one-workgroup-per-CU asm attention and the split reloc: 0.8 % faster (409.4 / 409.1
        vs 411.9 / 413.2 ms, one box, interleaved; C2 / C3 goldens pass), but the kernels of the two
        streams then overlap, so no per-kernel time (HIP events or rocprofv3) measures a kernel any
        more -- the roofline of the dominant kernel reads 0.40 instead of 0.50.  Off by default,
        so that the bench's roofline stays a measurement of the kernel."""
        pr, pg, x, sc, dev, C = ctx.pr, ctx.pg, ctx.x, ctx.sc, ctx.dev, ctx.pg.dim
        a0, q0, q1 = ctx.rows(b)
        La = q0 - a0                   # anchor tokens
        out = []
        kv_sub = self._subsample_kv(ctx, b)[1] if ctx.rowmap_t is not None else None
        side = self._aux_stream("_side", dev) if (_concurrent_stacks() and ctx.Nq_l > 0 and a0 < q0) else None
        if ctx.Nq_l > 0:
            attend_reloc = partial(self._reloc_attention, ctx, kv_sub, [])
            if side is not None:
                side.wait_stream(torch.cuda.current_stream(dev))  # frame block + subsample K/V are done
                with torch.cuda.stream(side):
                    runtime.run_block(pr, x, q0, q1, sc, attend_reloc, self._epi(ctx, pr, q0),
                                      q_scale=runtime.q_prescale(pr))
            else:
                out.append(runtime.run_block(pr, x, q0, q1, sc, attend_reloc, self._epi(ctx, pr, q0),
                                             defer=ctx.defer, q_scale=runtime.q_prescale(pr)))

        def attend_global(qkv, o):
            self._global_attention(qkv[:, 0:C], qkv[:, C:2 * C], qkv[:, 2 * C:3 * C], o, pg, La, La)
        out.append(runtime.run_block(pg, x, a0, q0, sc, attend_global, self._epi(ctx, pg, a0), defer=ctx.defer,
                                     q_scale=runtime.q_prescale(pg)))
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)  # join before the next frame block
        return out

    def _layer_sharded(self, ctx: _LayerCtx, b: int) -> list:
        """G > 1: the anchor K/V and the anchor-subsample K/V are gathered asynchronously
        (``gather_rows``; ``ctx.a_counts`` = anchor frames per rank): the subsample K/V behind the
        query-side QKV GEMM, the anchor K/V behind the whole reloc block and the local-anchor
        attention pass."""
        pr, pg, x, sc, dev, C = ctx.pr, ctx.pg, ctx.x, ctx.sc, ctx.dev, ctx.pg.dim
        a0, q0, q1 = ctx.rows(b)
        La_l = q0 - a0                     # local anchor tokens
        La = sum(ctx.a_counts) * ctx.P     # all anchor tokens
        out = []
        kv_sub_all, work_sub = self._subsample_kv(ctx, b)[1:] if ctx.rowmap_t is not None else (None, [])
        # global block, first half: LN1 + Q GEMM locally, K/V straight into this rank's slot
        xn, qkv = sc.xn[a0:q0], sc.qkv[a0:q0]
        kv_all = self._ws.get("kv_all", La, 2 * C, ctx.dtype, dev)
        kv_loc = self._ws.get("kv_loc", La_l, 2 * C, ctx.dtype, dev)
        ops.layernorm(x[a0:q0], pg.ln1_w, pg.ln1_b, pg.eps, xn)
        epi, epi_kv = self._epi(ctx, pg, a0), self._kv_epi(ctx, pg, pos_row_base=a0)
        probs = []
        if epi is not None and epi_kv is not None:
            probs = [dict(a=xn, w=pg.w_qkv[:C], out=qkv[:, :C], bias=_sl(pg.b_qkv, 0, C), qkv=epi),
                     dict(a=xn, w=pg.w_qkv[C:], out=kv_loc, bias=_sl(pg.b_qkv, C, 3 * C), qkv=epi_kv)]
        if probs and ops.gemm_group_eligible(probs):
            # Q and K/V as ONE grouped launch: at G = 8 a rank's 5,496 anchor rows are 88 + 176
            # tiles of 256^2, each under one workgroup round on its own
            ops.gemm_group(probs, _lib.SR_EPI_QKV, tag="gemm")
        else:
            runtime.qkv_gemm(pg, xn, pg.w_qkv[:C], qkv[:, :C], _sl(pg.b_qkv, 0, C), epi, runtime.q_prescale(pg))
            runtime.kv_gemm(pg, xn, kv_loc, epi_kv)
        work_kv = gather_rows(kv_all, kv_loc, [c * ctx.P for c in ctx.a_counts], ctx.group, ctx.r)
        # the reloc block's tail waits for the global attention and runs grouped with the global
        # block's (runtime.run_block_tails: one launch per GEMM stage over both row ranges)
        group_tails = ctx.Nq_l > 0 and runtime.group_tails_wanted(max(q1 - q0, q0 - a0))
        # ... and with SR_SHARD_CONCURRENT=1 its attention runs on a second stream beside the global
        # attention's key-split passes: at G = 8 both under-fill the chip on their own
        shard_side = (self._aux_stream("_shard_side", dev)
                      if group_tails and _SHARD_CONCURRENT and torch.device(dev).type == "cuda" else None)
        if ctx.Nq_l > 0:
            attend_reloc = partial(self._reloc_attention, ctx, kv_sub_all, work_sub)
            if group_tails:  # the tail joins the global block's in run_block_tails below
                runtime.run_block_head(pr, x, q0, q1, sc, self._epi(ctx, pr, q0), runtime.q_prescale(pr))
                if shard_side is not None:
                    shard_side.wait_stream(torch.cuda.current_stream(dev))  # the reloc QKV is done
                    with torch.cuda.stream(shard_side):  # (its wait on the subsample gather too)
                        attend_reloc(sc.qkv[q0:q1], sc.o[q0:q1])
                else:
                    attend_reloc(sc.qkv[q0:q1], sc.o[q0:q1])
            else:
                out.append(runtime.run_block(pr, x, q0, q1, sc, attend_reloc, self._epi(ctx, pr, q0),
                                             defer=ctx.defer, q_scale=runtime.q_prescale(pr)))
        _wait(work_sub)  # a rank without query frames still fed the others (send buffer reuse)
        o, q = sc.o[a0:q0], sc.qkv[a0:q0, 0:C]
        fp8 = self.fp8_global and pg.head_dim == 64 and q.dtype == torch.bfloat16
        if self.shard_overlap and not fp8:
            self._global_attention_sharded(q, kv_loc, kv_all, o, pg, La_l, La, sum(ctx.a_counts[:ctx.r]) * ctx.P,
                                           work_kv)
        else:
            _wait(work_kv)
            self._global_attention(q, kv_all[:, 0:C], kv_all[:, C:2 * C], o, pg, La_l, La)
        if shard_side is not None:
            torch.cuda.current_stream(dev).wait_stream(shard_side)  # join before the grouped tails
        if group_tails:
            return out + runtime.run_block_tails([(pr, q0, q1), (pg, a0, q0)], x, sc, defer=ctx.defer)
        return out + [runtime.run_block_tail(pg, x, a0, q0, sc, defer=ctx.defer)]

    def _layer_global_camera(self, ctx: _LayerCtx, b: int, anchor_rows, query_rows, cam_a, cam_q) -> None:
        """The LAST layer's global_reloc + global blocks of one batch item when only the camera rows
        are read (forward(outputs="camera"), G == 1): LN1 and the QKV projection run for every row as
        in _layer_paired (every row is a key), then only row 0 of each frame goes on --
          * attention: the anchors' camera rows as one query set against every anchor token
            (global); the queries' camera rows as one query set against the shared anchor subsample
            and each against its own frame (batch = Nq, lq = 1), merged by their LSEs (reloc):
            ops.attention_rows, sets of at most 64 rows;
          * proj + LayerScale residual, LN2, fc1 + GELU, fc2 + LayerScale residual on a compact
            [Na + Nq, C] fp32 stream gathered from x (runtime.run_block_tails: one grouped launch
            per stage for the two blocks where eligible).
        The results land in item b's rows of ``cam_a`` / ``cam_q`` ([B * Na, 2C] / [B * Nq, 2C]; reloc
        half), ``anchor_rows`` / ``query_rows`` being the camera rows of x; x is not updated.
        fp32 compute runs the same plumbing on the exact sr_attention kernel."""
        pr, pg, x, sc, ws, dtype, dev = ctx.pr, ctx.pg, ctx.x, ctx.sc, self._ws, ctx.dtype, ctx.dev
        C, H, D, P, Na, Nq = pg.dim, pg.heads, pg.head_dim, ctx.P, ctx.Na_l, ctx.Nq_l
        a0, q0, q1 = ctx.rows(b)
        kv_sub = self._project_heads(ctx, b)
        qkv_r, qkv_g = sc.qkv[q0:q1], sc.qkv[a0:q0]
        n, n_sub, hid = Na + Nq, kv_sub.shape[0], pg.w_fc1.shape[0]
        # compact scratch: rows [0, Na) the anchors' camera rows, [Na, n) the queries'
        cs = runtime.BlockScratch(xn=ws.get("cam_xn", n, C, dtype, dev), qkv=ws.get("cam_y", n, C, dtype, dev),
                                  o=ws.get("cam_o", n, C, dtype, dev), h=ws.get("cam_h", n, hid, dtype, dev))
        xc = ws.get("cam_x", n, C, torch.float32, dev)
        ops.copy_rows(xc[:Na], x, Na, rowmap=anchor_rows[b * Na:(b + 1) * Na])
        ops.copy_rows(xc[Na:], x, Nq, rowmap=query_rows[b * Nq:(b + 1) * Nq])
        # row 0 of every frame, read in place from the packed q|k|v rows (row stride P * 3C)
        q_g = qkv_g.view(Na, P * 3 * C)[:, 0:C]
        q_r = qkv_r.view(Nq, P * 3 * C)[:, 0:C]
        for s0 in range(0, Na, ops.ROWS_MAX_LQ):
            m = min(ops.ROWS_MAX_LQ, Na - s0)
            ops.attention_rows(q_g[s0:s0 + m], qkv_g[:, C:2 * C], qkv_g[:, 2 * C:3 * C], cs.o[s0:s0 + m], heads=H,
                               head_dim=D, batch=1, lq=m, q_bstride=0, l0=q0 - a0, k0_bstride=0, q_scaled=_qs(pg))
        for s0 in range(0, Nq, ops.ROWS_MAX_LQ):
            m = min(ops.ROWS_MAX_LQ, Nq - s0)
            o_parts = ws.get("cam_parts", 2 * m, C, dtype, dev)
            lse_parts = ws.get("cam_lse", 2, H * m, torch.float32, dev)
            ops.attention_rows(q_r[s0:s0 + m], kv_sub[:, 0:C], kv_sub[:, C:2 * C], o_parts[:m], heads=H, head_dim=D,
                               batch=1, lq=m, q_bstride=0, l0=n_sub, k0_bstride=0, lse=lse_parts[0],
                               q_scaled=_qs(pr))
            own = qkv_r[s0 * P:(s0 + m) * P]
            ops.attention_rows(q_r[s0:s0 + m], own[:, C:2 * C], own[:, 2 * C:3 * C], o_parts[m:], heads=H, head_dim=D,
                               batch=m, lq=1, q_bstride=1, l0=P, k0_bstride=P, lse=lse_parts[1], q_scaled=_qs(pr))
            ops.attn_merge_n(o_parts, lse_parts, cs.o[Na + s0:Na + s0 + m], parts=2, rows=m, heads=H, head_dim=D,
                             seg_rows=[m, 1])
        runtime.run_block_tails([(pr, Na, n), (pg, 0, Na)], xc, cs, defer=False)
        ops.copy_rows(cam_a[b * Na:(b + 1) * Na, C:], xc[:Na], Na)
        ops.copy_rows(cam_q[b * Nq:(b + 1) * Nq, C:], xc[Na:], Nq)

    def set_fp8_global(self, enabled: bool = True, fp8_v: bool = False):
        """Global blocks' q.k^T in block-scaled fp8 (BASELINE C5); with ``fp8_v`` also V and P.V.
        Everything else stays bf16 -- including the last layer of a camera-only forward
        (forward(outputs="camera")), whose camera rows run the bf16 rows kernel: there is no fp8
        rows kernel."""
        self.fp8_global = bool(enabled)
        self.fp8_v = bool(enabled and fp8_v)
        return self

    def _global_attention_sharded(self, q, kv_loc, kv_all, o, pg, lq, lk, off, work_kv):
        """softmax over every anchor's keys in two passes: the local anchors (kv_loc, ready now)
        while the gather of the others is in flight, then the remote anchors (kv_all rows outside
        [off, off + lq): up to two key segments), merged exactly by the passes' LSEs."""
        C, H, D = pg.dim, pg.heads, pg.head_dim
        kb, qb = runtime.key_norm_bound(pg), runtime.query_norm_bound(pg)
        segs = [(a, n) for a, n in ((0, off), (off + lq, lk - off - lq)) if n > 0]
        if q.dtype == torch.bfloat16:
            # every pass key-split as one slice of a stacked partials buffer (the per-rank query
            # slice alone leaves CUs idle at G >= 4), one N-way LSE merge at the end
            split = lambda n: ops.key_split_parts(dtype=q.dtype, batch=1, lq=lq, heads=H, l0=n, l1=0,  # noqa: E731
                                                  mask_mode=0)
            plan = [[kv_loc, split(lq)]] + [[kv_all[a:a + n], split(n)] for a, n in segs]
            # one sr_attn_merge_n takes at most SR_ATTN_MERGE_MAX_PARTS partials: a middle rank's two
            # remote segments can each want 8 (C3 at G = 8, ranks 3 and 4: 2 + 8 + 8), so the pass
            # with the most parts gives up half of them (its chunks double) until the total fits
            while sum(p for _, p in plan) > _lib.SR_ATTN_MERGE_MAX_PARTS:
                big = max(plan, key=lambda e: e[1])
                big[1] = max(1, big[1] // 2)
            plan = [(kv, [(0, kv.shape[0], p)]) for kv, p in plan]  # one launch of p equal chunks per pass
            total = sum(pp for _, pieces in plan for _, _, pp in pieces)
            o_parts, lse_parts = ops.key_split_workspace(q.device, total, lq, C, H, name="attn_shard")
            p0 = 0
            for i, (kv, pieces) in enumerate(plan):
                if i == 1:
                    _wait(work_kv)  # the remote anchors' K/V
                for a, m, pp in pieces:
                    ops.attention_partials(q, kv[a:a + m, 0:C], kv[a:a + m, C:2 * C],
                                           o_parts[p0 * lq:(p0 + pp) * lq], lse_parts[p0:p0 + pp], heads=H,
                                           head_dim=D, lq=lq, l0=m, parts=pp, tag="attn_global", key_norm_max=kb,
                                           query_norm_max=qb, tail_readable=_SHARD_TAIL, q_scaled=_qs(pg))
                    p0 += pp
            ops.attn_merge_n(o_parts, lse_parts, o, parts=total, rows=lq, heads=H, head_dim=D)
            return
        ws = self._ws
        lse_loc = ws.get("lse_loc", H, lq, torch.float32, q.device)
        lse_rem = ws.get("lse_rem", H, lq, torch.float32, q.device)
        o_rem = ws.get("o_rem", lq, C, o.dtype, q.device)
        ops.attention(q, kv_loc[:, 0:C], kv_loc[:, C:2 * C], o, heads=H, head_dim=D, batch=1, lq=lq, q_bstride=0,
                      l0=lq, k0_bstride=0, tag="attn_global", lse=lse_loc, key_norm_max=kb, query_norm_max=qb,
                      q_scaled=_qs(pg))
        _wait(work_kv)
        (s0, n0), (s1, n1) = segs[0], (segs[1] if len(segs) > 1 else (0, 0))
        ops.attention(q, kv_all[s0:s0 + n0, 0:C], kv_all[s0:s0 + n0, C:2 * C], o_rem, heads=H, head_dim=D, batch=1,
                      lq=lq, q_bstride=0, l0=n0, k0_bstride=0, k1=kv_all[s1:s1 + n1, 0:C] if n1 else None,
                      v1=kv_all[s1:s1 + n1, C:2 * C] if n1 else None, l1=n1, k1_bstride=0, tag="attn_global",
                      lse=lse_rem, key_norm_max=kb, query_norm_max=qb, q_scaled=_qs(pg))
        ops.attn_merge(o, lse_loc, o_rem, lse_rem, o, heads=H, head_dim=D, tag="attn_merge")

    def _global_attention(self, q, k, v, o, pg, lq, lk):
        if self.fp8_global and pg.head_dim == 64 and q.dtype == torch.bfloat16:
            if self._fp8_ws is None:
                self._fp8_ws = ops.Fp8Workspace()
            ops.attention_qk8(q, k, v, o, heads=pg.heads, batch=1, lq=lq, q_bstride=0, l0=lk, k0_bstride=0,
                              tag="attn_global", ws=self._fp8_ws, fp8_v=self.fp8_v,
                              key_norm_max=runtime.key_norm_bound(pg), q_scaled=_qs(pg))
        else:
            ops.attention(q, k, v, o, heads=pg.heads, head_dim=pg.head_dim, batch=1, lq=lq, q_bstride=0, l0=lk,
                          k0_bstride=0, tag="attn_global", key_norm_max=runtime.key_norm_bound(pg),
                          query_norm_max=runtime.query_norm_bound(pg), q_scaled=_qs(pg))

    def _paired_attention(self, pr, pg, dtype, rows: int, La: int, n_sub: int) -> bool:
        """Single GPU, bf16, split reloc, a global query set that fills the chip without key
        splitting: the global attention and the reloc subsample pass in one launch
        (ops.attention_pair; SR_ATTN_PAIR=0 launches them apart)."""
        if not self._split_reloc(dtype, rows, n_sub) or self.fp8_global or La <= 0 or pg.heads != pr.heads:
            return False
        if _concurrent_stacks():
            return False
        if ops.key_split_parts(dtype=dtype, batch=1, lq=La, heads=pg.heads, l0=La, l1=0, mask_mode=0) != 1:
            return False
        return (ops.pair_eligible(dtype, La, pg.head_dim, runtime.key_norm_bound(pg)) and
                ops.pair_eligible(dtype, n_sub // 64 * 64, pr.head_dim, runtime.key_norm_bound(pr)))

    @staticmethod
    def _split_reloc(dtype, rows: int, n_sub: int) -> bool:
        """The reloc attention as two passes (bf16, a query set that fills the chip without key
        splitting; SR_RELOC_SPLIT=0 turns it off): the shared subsample's whole tiles over all query
        rows on the hand-scheduled sweep, then the own-frame pass whose epilogue folds the first in
        (sr_attn_desc.merge_o).  Measured (one box, kbench): 1.505 + 0.332 = 1.837 ms against 1.883 ms
        in one launch; whole C3 step 417.8 / 418.2 vs 419.5 / 418.9 ms (interleaved).  With a separate
        merge launch instead (round 3, first form) it was break-even."""
        return (os.environ.get("SR_RELOC_SPLIT", "1") == "1" and dtype == torch.bfloat16 and
                (rows + 255) // 256 * 16 >= _RELOC_SPLIT_MIN_WG and n_sub >= 64)

    def _aux_stream(self, attr: str, dev):
        """The second HIP stream kept in ``attr``: ``_shard_side`` for the frame-sharded reloc attention
        (SR_SHARD_CONCURRENT=1), ``_side`` for the concurrent reloc block (opt-in: SR_CONCURRENT_STACKS=1)."""
        s = getattr(self, attr, None)
        if s is None or s.device != torch.device(dev):
            s = torch.cuda.Stream(device=dev)
            setattr(self, attr, s)
        return s


# SR_SHARD_TAIL=1 (opt-in): the frame-sharded global block's key-split passes declare their chunk
# tails readable (kv_loc / kv_all are Workspace buffers with 64 padding rows), which sends them to the
# hand-scheduled sweep's ragged variant (round 3 measured it level with the compiled sweep per rank:
# DESIGN.md section 5)
_SHARD_TAIL = os.environ.get("SR_SHARD_TAIL", "0") == "1"
# SR_SHARD_CONCURRENT (default 1; 0 for the A/B): under frame sharding with grouped tails, the reloc
# attention on a second stream beside the global attention.  Rank-0 rehearsal, one box, 2 runs each
# (profiles/r05_j10_rs_*.log): G = 8 69.03 / 69.15 -> 66.87 / 66.98 ms, G = 4 121.8 / 121.0 -> 120.9 /
# 120.7 ms; the sharded GPU tests pass with it
_SHARD_CONCURRENT = os.environ.get("SR_SHARD_CONCURRENT", "1") != "0"
# SR_CAMERA_ONLY=0 (A/B switch): forward(outputs="camera") behaves as outputs="all"
_CAMERA_ONLY = os.environ.get("SR_CAMERA_ONLY", "1") != "0"
# SR_DEDUP_FRAMES=0: the DINO stack runs on every frame, duplicates included (_embed, frame_dedup.py)
_DEDUP_FRAMES = os.environ.get("SR_DEDUP_FRAMES", "1") != "0"
# smallest query set (in 256-row x head workgroups) whose reloc attention runs split (A/B switch)
_RELOC_SPLIT_MIN_WG = int(os.environ.get("SR_RELOC_SPLIT_MIN_WG", "2048"))


def _sl(t, a, b):
    return None if t is None else t[a:b]


def _qs(pb) -> bool:
    """Whether pb's QKV GEMMs here write c*q (runtime.q_prescale): the attention takes q_scaled."""
    return runtime.q_prescale(pb) > 0


def _concurrent_stacks() -> bool:
    """SR_CONCURRENT_STACKS=1 (read at every call): Aggregator._layer_plain's side stream; no pairing then."""
    return os.environ.get("SR_CONCURRENT_STACKS", "0") == "1"


def _wait(works):
    for w in works:
        w.wait()
    works.clear()


def shard_range(n: int, G: int, r: int) -> Tuple[int, int]:
    """(start, count) of rank r's contiguous share of n frames over G ranks: the first n % G
    ranks own one frame more than the rest (counts differ by at most one)."""
    base, extra = divmod(n, G)
    return r * base + min(r, extra), base + (1 if r < extra else 0)


def check_frame_lists(no_reloc_list, reloc_list, S: int) -> None:
    """The anchor and query lists of a forward over S frames (inference and training alike)."""
    if sorted(list(no_reloc_list) + list(reloc_list)) != list(range(S)):
        raise ValueError("no_reloc_list and reloc_list must be disjoint and cover every frame "
                         f"(S={S}, got {list(no_reloc_list)} / {list(reloc_list)}); the reference's "
                         "block mask (aggregator.py:302-311) assumes the same")
    if len(no_reloc_list) == 0:
        raise ValueError("at least one anchor (no_reloc) frame is required")


def subsample_rowmap(idx: np.ndarray, frames: int, P: int, psi: int) -> np.ndarray:
    """Rows of x that each layer's anchor subsample reads (aggregator.py:277-285, 580-626): per anchor
    frame its ``psi`` special rows, then the selected patch rows.  ``idx`` [depth, B, na, rank] patch
    draws (plan_subsample); x holds ``frames`` frames of P rows per batch item, anchors first
    -> int32 [depth, B, na * (psi + rank)]."""
    depth, B, na, rank = idx.shape
    base = (np.arange(B) * frames * P)[None, :, None, None] + (np.arange(na) * P)[None, None, :, None]
    sel = base + psi + idx
    spec = np.broadcast_to(base + np.arange(psi)[None, None, None, :], (depth, B, na, psi))
    return np.concatenate([spec, sel], axis=-1).astype(np.int32).reshape(depth, B, na * (psi + rank))


def camera_row_tables(B: int, Na: int, Nq: int, P: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows of the residual stream x that hold the camera token (row 0) of every anchor frame and of
    every query frame, batch-major (int32): x orders each batch item's frames as [Na anchors ; Nq
    queries] of P rows each, whatever the frames' original indices were."""
    base = np.arange(B, dtype=np.int64)[:, None] * ((Na + Nq) * P)
    anchors = (base + np.arange(Na, dtype=np.int64)[None, :] * P).reshape(-1)
    queries = (base + (Na + np.arange(Nq, dtype=np.int64))[None, :] * P).reshape(-1)
    return anchors.astype(np.int32), queries.astype(np.int32)


def gather_rows(dst: torch.Tensor, src: torch.Tensor, counts: List[int], group, rank: int) -> list:
    """Async gather of every rank's ``src`` rows into ``dst`` = [rank 0's rows ; rank 1's ; ...]
    (``counts[j]`` rows from rank j; row-contiguous tensors).  Equal counts: one
    all_gather_into_tensor (RCCL ring over xGMI).  Uneven counts: one broadcast per non-empty
    rank straight into that rank's slot of ``dst`` — the rows land compact, so no padding row
    can reach a softmax.  Returns the works to wait on."""
    dist = torch.distributed
    if isinstance(group, RankSim):  # no peers: this rank's rows land in its slot, the others stay as they are
        off = sum(counts[:rank])
        dst[off:off + counts[rank]].copy_(src)
        return []
    if len(set(counts)) == 1:
        return [dist.all_gather_into_tensor(dst, src, group=group, async_op=True)]
    offs = np.concatenate([[0], np.cumsum(counts)]).tolist()
    if counts[rank]:
        dst[offs[rank]:offs[rank + 1]].copy_(src)
    return [dist.broadcast(dst[offs[j]:offs[j + 1]], src=dist.get_global_rank(group, j), group=group, async_op=True)
            for j in range(len(counts)) if counts[j]]


class RankSim:
    """Stand-in process group for ONE rank of a ``world``-rank frame-sharded forward, run alone on
    one GPU (``Aggregator.set_frame_sharding(RankSim(8, 0))``): the rank computes exactly its
    share -- its frames' DINO / frame / MLP work, the global block's local and remote attention
    passes over every anchor's keys, the reloc block against the whole anchor subsample, the
    replicated camera head -- but the gathers move nothing (the peers' slots of the gathered K/V
    buffers keep whatever they hold).  Its outputs are therefore NOT the model's; it exists to time
    a rank's step and host submit cost before a multi-GPU run (tools/rank_sim.py)."""

    def __init__(self, world: int, rank: int):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.world, self.rank = int(world), int(rank)

