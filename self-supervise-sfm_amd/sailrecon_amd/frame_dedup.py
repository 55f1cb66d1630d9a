"""Host side of the DINO frame dedup (Aggregator._embed): pure functions of ``rep``, the
bit-identical-frame table ops.frame_groups returns, so they are testable without a GPU.

The DINO stack (patch embed, DINO's special tokens, its blocks and final norm) treats every frame
independently with row-local or per-(frame, head) kernels and a fixed k / key order, so two frames
holding the same bits leave it with the same bits.  A scene whose queries are its anchor images
again (the reference's demo and training convention) therefore needs the stack once per DISTINCT
frame; the final DINO LayerNorm writes every frame's rows from its representative's.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _lib, ops


def group_frames(rep, tokens: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``rep`` [F] (rep[f] = the first frame holding frame f's bits, or f) ->
    (``uniq`` int32 [U]: the distinct frames in ascending order, ``slot`` int32 [F]: frame f's
    position in ``uniq``, ``rowmap`` int32 [F * tokens]: row f * tokens + t of the full stream reads
    row slot[f] * tokens + t of the compact one).  An entry that does not name an earlier
    representative (rep[f] > f, negative, or rep[rep[f]] != rep[f]) keeps its frame distinct."""
    rep = np.asarray(rep, dtype=np.int64).reshape(-1)
    n = rep.shape[0]
    f = np.arange(n, dtype=np.int64)
    ok = (rep >= 0) & (rep <= f)
    root = np.where(ok, rep, f)
    root = np.where(root[root] == root, root, f)  # only a frame that stands for itself is a representative
    uniq = np.flatnonzero(root == f)
    pos = np.full(n, -1, dtype=np.int64)
    pos[uniq] = np.arange(uniq.shape[0])
    slot = pos[root]
    assert (slot >= 0).all()
    rowmap = (slot[:, None] * tokens + np.arange(tokens, dtype=np.int64)[None, :]).reshape(-1)
    if uniq.shape[0] * tokens >= 2 ** 31:
        raise ValueError("group_frames: the compact stream's rows do not fit int32")
    return uniq.astype(np.int32), slot.astype(np.int32), rowmap.astype(np.int32)


def dino_plan(frames: int, tokens: int, dim: int, hidden: int, heads: int, dtype: torch.dtype) -> tuple:
    """The row- or frame-count-dependent kernel choices of one DINO block over ``frames`` frames: the
    split-K slices of its four GEMMs (ops._splitk_plan, M <= 256 only), sr_gemm's 64 x 256 few-row
    tile (M <= 64), the attention's workgroup shape (sr_attention: 256-row tiles from 512 workgroups
    on) and its key split.  Two frame counts with equal plans run the same kernels in the same
    k / key order per row, so the dedup (U frames instead of F) is then bit-exact; where the plans
    differ it is held to the parity tolerance."""
    rows = frames * tokens
    E = _lib
    gemms = ((3 * dim, dim, E.SR_EPI_BIAS), (dim, dim, E.SR_EPI_BIAS_RESID), (hidden, dim, E.SR_EPI_BIAS_GELU),
             (dim, hidden, E.SR_EPI_BIAS))
    splits = tuple(ops._splitk_plan(rows, n, k, epi, dtype) for n, k, epi in gemms)
    wgs256 = (tokens + 255) // 256 * heads * frames
    ksplit = ops.key_split_parts(dtype=dtype, batch=frames, lq=tokens, heads=heads, l0=tokens, l1=0,
                                 mask_mode=E.SR_MASK_NONE)
    return splits, rows <= 64, wgs256 >= 512, ksplit
