"""Host side of the camera-only last layer (no GPU): sr_attention_rows' chunk plan and argument
validation, the camera-row tables, and SailRecon.forward's choice of Aggregator outputs."""

import ctypes

import numpy as np
import pytest
import torch

from sailrecon_amd import _lib, ops
from sailrecon_amd.models import aggregator as A
from sailrecon_amd.models.sail_recon import SailRecon


def desc(*, heads=16, batch=1, lq=32, l0=43968, l1=0, head_dim=64):
    d = _lib.AttnDesc()
    for i, name in enumerate(("q", "k0", "v0", "o") + (("k1", "v1") if l1 else ())):
        setattr(d, name, ctypes.c_void_p((i + 1) << 12))
    d.ldq = d.ldk0 = d.ldv0 = d.ldo = d.ldk1 = d.ldv1 = 3 * heads * 64
    d.batch, d.heads, d.head_dim, d.lq, d.l0, d.l1 = batch, heads, head_dim, lq, l0, l1
    d.q_bstride, d.k1_bstride, d.scale = lq, l1, 0.125
    return d


def plan(**kw):
    """(chunks, keys per chunk) as the library plans them: the workspace holds 66 floats per
    (item, head, chunk, query row), and equal chunks of a multiple of 32 keys cover the keys."""
    lib = _lib.load()
    d = desc(**kw)
    n = lib.sr_attention_rows_chunks(ctypes.byref(d))
    assert lib.sr_attention_rows_workspace(ctypes.byref(d)) == d.batch * d.heads * n * d.lq * 66 * 4
    assert n == ops.rows_chunks(heads=d.heads, batch=d.batch, lq=d.lq, l0=d.l0, l1=d.l1)
    total = d.l0 + d.l1
    per = -(-total // n)
    return n, -(-per // 32) * 32


def test_chunk_plan_headline_shapes():
    # C3 global: 4 head groups -> 128 chunks reach 512 workgroups (two per CU), 352 keys each
    assert plan(lq=32, l0=43968) == (128, 352)
    # the subsample pass: chunks of >= 256 keys cap the count; the last 4 of 38 chunks are empty
    n, keys = plan(lq=32, l0=9760)
    assert (n, keys) == (38, 288) and -(-9760 // keys) == 34
    # own-frame pass: 32 items x 4 head groups already give 128 workgroups per chunk
    assert plan(batch=32, lq=1, l0=1374) == (4, 352)


@pytest.mark.parametrize("l0,l1,batch,heads,want", [
    (1, 0, 1, 1, 1), (63, 0, 1, 1, 1), (65, 64, 3, 6, 1), (127, 21, 1, 16, 1),
    (1000, 0, 1, 16, 3), (1000, 64, 3, 6, 4), (4100, 0, 1, 16, 16), (4100, 64, 3, 1, 16),
    (1 << 20, 0, 1, 16, 128), (1 << 20, 0, 64, 16, 2)])
def test_chunk_plan_sweep(l0, l1, batch, heads, want):
    n, keys = plan(lq=33, l0=l0, l1=l1, batch=batch, heads=heads)
    assert n == want
    assert keys % 32 == 0 and n * keys >= l0 + l1       # the chunks cover every key
    assert n == 1 or (l0 + l1) // n >= 256                # no planned chunk under 256 keys
    groups = -(-heads // 4) * batch
    assert n == 1 or (n - 1) * groups < 512               # no more chunks than two workgroups per CU need


def test_chunk_plan_has_empty_chunks_at_4100():
    n, keys = plan(lq=32, l0=4100)
    assert (n, keys) == (16, 288) and -(-4100 // keys) == 15  # the 16th chunk starts past the last key


def test_rows_rejections_without_gpu():
    lib = _lib.load()
    ws = ctypes.c_void_p(1 << 20)

    def call(d, nbytes=None):
        need = lib.sr_attention_rows_workspace(ctypes.byref(d))
        return lib.sr_attention_rows(None, _lib.SR_BF16, ctypes.byref(d), ws, need if nbytes is None else nbytes)

    for d in (desc(lq=65), desc(head_dim=128)):
        assert lib.sr_attention_rows_chunks(ctypes.byref(d)) == 0
        assert call(d) == -3 and lib.sr_last_error()
    d = desc()
    d.mask_mode = _lib.SR_MASK_CAMERA
    assert call(d) == -3
    d = desc()
    d.merge_o = ctypes.c_void_p(1 << 13)
    assert call(d) == -3
    d = desc()
    assert call(d, lib.sr_attention_rows_workspace(ctypes.byref(d)) - 1) == -1
    assert b"workspace" in lib.sr_last_error()
    assert lib.sr_attention_rows(None, _lib.SR_F32, ctypes.byref(d), ws, 1 << 40) == -3
    d.ldq = 3 * 16 * 64 + 4
    assert call(d) == -1
    assert lib.sr_version() >= (1 << 16) | 7


def test_camera_row_tables():
    P = 21
    a, q = A.camera_row_tables(1, 3, 3, P)
    assert a.dtype == q.dtype == np.int32
    assert a.tolist() == [0, 21, 42] and q.tolist() == [63, 84, 105]
    # B = 2: batch-major, each item's frames [anchors ; queries]
    a, q = A.camera_row_tables(2, 2, 3, P)
    assert a.tolist() == [0, 21, 105, 126] and q.tolist() == [42, 63, 84, 147, 168, 189]
    # interleaved no_reloc / reloc lists do not change the tables: x is ordered [anchors ; queries]
    # internally (images[:, no_reloc + reloc]), so frame f of that order starts at row f * P
    no_reloc, reloc = [3, 1, 4], [0, 5, 2]
    order = no_reloc + reloc
    a, q = A.camera_row_tables(1, len(no_reloc), len(reloc), P)
    assert [order[r // P] for r in a.tolist()] == no_reloc and [order[r // P] for r in q.tolist()] == reloc
    assert all(r % P == 0 for r in a.tolist() + q.tolist())
    a, q = A.camera_row_tables(2, 4, 0, P)
    assert q.size == 0 and a.tolist() == [0, 21, 42, 63, 84, 105, 126, 147]


class StubAggregator(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.C, self.calls = C, []

    def _world(self):
        return None, 1, 0

    def forward(self, images, no_reloc_list, reloc_list, fix_rank=None, *, outputs="all"):
        self.calls.append(outputs)
        B, Nq = images.shape[0], len(reloc_list)
        P = 1 if outputs == "camera" else 7
        t = torch.zeros(B, Nq, P, 2 * self.C)
        return {-1: t}, 5, torch.zeros(B, len(no_reloc_list), 2 * self.C)


@pytest.mark.parametrize("point,depth,want", [(False, False, "camera"), (True, False, "all"), (False, True, "all"),
                                               (True, True, "all")])
def test_sailrecon_passes_camera_only_without_dense_heads(point, depth, want):
    C = 16
    m = SailRecon.__new__(SailRecon)  # no real aggregator (its DINO backbone) behind the stub
    torch.nn.Module.__init__(m)
    m.aggregator, m.camera_head, m.return_pose_enc = StubAggregator(C), None, False
    # stand-ins for the dense heads: forward() only asks whether they exist
    m.point_head = (lambda *a, **k: (torch.zeros(1, 2, 1), torch.zeros(1, 2, 1))) if point else None
    m.depth_head = (lambda *a, **k: (torch.zeros(1, 2, 1), torch.zeros(1, 2, 1))) if depth else None
    out = m(torch.zeros(1, 4, 3, 28, 28), no_reloc_list=[0, 1], reloc_list=[2, 3])
    assert m.aggregator.calls == [want]
    assert len(out) == 2 and tuple(out[0]["cam_tokens"].shape) == (1, 2 * C)
