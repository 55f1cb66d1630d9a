"""sr_frame_groups (ops.frame_groups) against a numpy bytes-compare, and sr_im2col_normalize_map
against im2col of the gathered frames.

rep[f] must be the first earlier frame with the same bits, or f.  The layouts put frame bases on
every 4-byte phase of a 16-byte line (base offsets 0..3 words, odd strides), so the 16-B body, the
head and tail words, and the word-by-word compare of two differently aligned frames all run."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_FRAMES = (1, 2, 5, 64)
FRAME_WORDS = (1, 3, 4, 5, 1023, 9408, 14700)   # 9408 = 3*56*56, 14700 = 3*70*70
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sailrecon_amd import ops
    return ops


def ref_rep(frames):
    """numpy bytes-compare: the first earlier frame with the same bytes, else the frame itself."""
    first = {}
    return np.array([first.setdefault(frames[f].tobytes(), f) for f in range(frames.shape[0])], dtype=np.int32)


def patterns(n, words, rng):
    """name -> uint32 [n, words].  Base frames are random fp32 bit patterns."""
    base = rng.integers(0, 2 ** 32, size=(n, words), dtype=np.uint32)
    out = {"distinct": base.copy()}
    if n < 2:
        return out
    h = n // 2
    a = base.copy(); a[h:2 * h] = a[:h]; out["second_half_equals_first"] = a
    tail = max(words - 2, 0)  # a word of the last, partial 16-B vector (or of the head when the frame is short)
    for name, w in (("flip_first", 0), ("flip_last", words - 1), ("flip_tail", tail)):
        a = base.copy(); a[h:2 * h] = a[:h]; a[2 * h - 1, w] ^= np.uint32(1 << 7); out[name] = a
        a = base.copy(); a[1] = a[0]; a[1, w] ^= np.uint32(1 << 31); out[name + "_sign"] = a
    a = base.copy(); a[0] = 0; a[1] = 0; a[1, words // 2] = np.uint32(0x80000000); out["plus_minus_zero"] = a
    a = base.copy(); a[0, words // 2] = np.uint32(0x7FC00123); a[1] = a[0]; out["equal_nan_payload"] = a
    a = base.copy(); a[0, 0] = np.uint32(0x7FC00001); a[1] = a[0]; a[1, 0] = np.uint32(0x7FC00002); out["other_nan"] = a
    if words >= 2:
        a = base.copy(); a[0, 0], a[0, words - 1] = np.uint32(1), np.uint32(2); a[1] = a[0]
        a[1, 0], a[1, words - 1] = a[0, words - 1], a[0, 0]; out["swapped_words"] = a
    if n >= 3:
        a = base.copy(); a[n - 1] = a[0]; a[n // 2] = a[0]; out["three_copies"] = a
    if n >= 5:
        a = base.copy(); a[2] = a[0]; a[4] = a[1]; a[3] = a[1]; out["interleaved"] = a
    return out


def device_frames(arr, base_off, stride):
    """arr [n, words] in a flat int32 device buffer: frame f at word base_off + f * stride."""
    n, words = arr.shape
    flat = np.full(base_off + n * stride + 8, GUARD, dtype=np.uint32)
    for f in range(n):
        flat[base_off + f * stride: base_off + f * stride + words] = arr[f]
    buf = torch.from_numpy(flat.view(np.int32)).to(DEV)
    return buf, buf[base_off:].as_strided((n, words), (stride, 1))


def run(ops, view, n, words, fp_override=None):
    """One call with guard words around out and the workspace; returns rep (host), checks the guards."""
    need = ops.frame_groups_workspace_bytes(words, n)
    assert need > 0
    out = torch.full((n + 16,), -7, device=DEV, dtype=torch.int32)
    ws = torch.full((need + 128,), 0xA5, device=DEV, dtype=torch.uint8)
    ops.frame_groups(view, out[8:8 + n], fp_override=fp_override, workspace=ws[64:64 + need])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:8] == -7).all() and (o[8 + n:] == -7).all(), "guard words around out"
    w = ws.cpu().numpy()
    assert (w[:64] == 0xA5).all() and (w[64 + need:] == 0xA5).all(), "guard bytes around the workspace"
    return o[8:8 + n].copy()


@pytest.mark.parametrize("words", FRAME_WORDS)
@pytest.mark.parametrize("n", N_FRAMES)
def test_frame_groups(ops, n, words):
    rng = np.random.default_rng(1000 * n + words)
    # (base offset in words, stride): packed and 16-B aligned; every frame on another phase; a
    # stride larger than the frame from an odd base
    layouts = [(0, words), (1, words + 1), (3, words + 6)]
    for name, arr in patterns(n, words, rng).items():
        want = ref_rep(arr)
        for base_off, stride in layouts:
            buf, view = device_frames(arr, base_off, stride)
            got = run(ops, view, n, words)
            assert np.array_equal(got, want), (name, base_off, stride, got.tolist(), want.tolist())
            again = run(ops, view, n, words)
            assert np.array_equal(again, got), (name, "two runs differ")
            assert np.array_equal(buf.cpu().numpy().view(np.uint32)[base_off + n * stride:], np.full(8, GUARD, np.uint32))
        # forced collisions: every frame carries the same fingerprint, so every frame is compared with
        # frame 0 and only the exact compare can keep unequal frames apart
        zeros = torch.zeros(n, 2, device=DEV, dtype=torch.int64)
        _, view = device_frames(arr, 1, words + 1)
        got = run(ops, view, n, words, fp_override=zeros)
        if name == "distinct":
            assert np.array_equal(got, np.arange(n)), (name, got.tolist())
        for f in range(n):  # safety: a named representative holds the same bits (a group may be lost)
            assert got[f] == f or (got[f] < f and arr[got[f]].tobytes() == arr[f].tobytes()), (name, f, got.tolist())
            assert got[f] == f or got[f] == 0


def test_frame_groups_fp32_images(ops):
    """The aggregator's call: contiguous fp32 images [F, 3, H, W] viewed as [F, words]."""
    g = torch.Generator().manual_seed(0)
    imgs = torch.rand(6, 3, 70, 70, generator=g)
    imgs[3:] = imgs[:3]
    imgs[5, 2, 69, 69] = -imgs[5, 2, 69, 69]
    rep = ops.frame_groups(imgs.to(DEV).view(6, -1))
    assert rep.cpu().tolist() == [0, 1, 2, 0, 1, 5]


def test_frame_groups_rejects_bad_arguments(ops):
    from sailrecon_amd._lib import SfmAmdError
    x = torch.zeros(4, 8, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.frame_groups(x.to(torch.int64))
    with pytest.raises(ValueError):
        ops.frame_groups(x, workspace=torch.zeros(8, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.frame_groups(x, fp_override=torch.zeros(4, 1, device=DEV, dtype=torch.int64))
    with pytest.raises(SfmAmdError):  # overlapping frames: a stride below the frame's words
        ops.frame_groups(x.view(-1).as_strided((4, 8), (4, 1)))
    assert ops.frame_groups_workspace_bytes(0, 4) == 0 and ops.frame_groups_workspace_bytes(8, 70000) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size", [56, 70])
def test_im2col_frame_map(ops, size, dtype):
    g = torch.Generator().manual_seed(size)
    imgs = torch.rand(5, 3, size, size, generator=g).to(DEV)
    fmap = torch.tensor([3, 0, 0, 4], device=DEV, dtype=torch.int32)
    kt = 64 if dtype == torch.bfloat16 else 32
    kpad = -(-3 * 14 * 14 // kt) * kt
    rows = (size // 14) ** 2
    got = torch.full((4 * rows + 2, kpad), 7.0, device=DEV, dtype=dtype)
    want = torch.full((4 * rows + 2, kpad), 7.0, device=DEV, dtype=dtype)
    ops.im2col_normalize(imgs, 14, got, kpad, frame_map=fmap)
    ops.im2col_normalize(imgs[fmap.long()].contiguous(), 14, want, kpad)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert (got[4 * rows:] == 7.0).all()  # nothing past the mapped frames' rows
    plain = torch.empty(5 * rows, kpad, device=DEV, dtype=dtype)
    mapped = torch.empty(5 * rows, kpad, device=DEV, dtype=dtype)
    ops.im2col_normalize(imgs, 14, plain, kpad)
    ops.im2col_normalize(imgs, 14, mapped, kpad, frame_map=torch.arange(5, device=DEV, dtype=torch.int32))
    assert torch.equal(plain, mapped)
