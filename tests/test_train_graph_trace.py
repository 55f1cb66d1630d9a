"""TrainGraph's launch sequence against its recorded fixture (no GPU, no library).

tests/train_trace.py runs every scene's training steps (forward + backward + refresh_packs) on CPU
tensors behind a recorder in place of ``ops``; tests/golden/g16_train_graph_trace.json.gz holds the
same traces as recorded at the commit its header names (tests/golden/make_golden_train_trace.py).
Every step must make the same ``ops`` calls, with the same operands and keywords, and the same
``grad_ready_hook`` calls, in the same order: a change of the graph's structure must leave the
fixture as it is, and a change of what is launched shows as the first differing call.  Per scene the
launches that name its path are asserted too, and beside the golden the conditions that a trace
recorded from any one commit cannot state: what a rebuilt pack does to the refresh table, and the
errors the entry points raise."""

import gzip
import json
import os

import pytest
import torch

import train_trace as T
from sailrecon_amd import runtime
from sailrecon_amd.train import engine
from sailrecon_amd.train import model as M

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_train_graph_trace.json.gz")

# scene -> (launches its path must make, launches it must not)
PATH = {
    "a01_bf16": (["gemm_group", "gemm_wgrad_pair", "qk_bwd", "weight_refresh_table", "weight_refresh_list"], []),
    "a02_fp32": (["wgrad_small", "qk_bwd"], ["gemm_group", "gemm_wgrad", "cast_bf16", "weight_refresh_table"]),
    "a06_plain_kv_fp32": (["wgrad_small"], ["qk_bwd"]),
    "a12_three_steps": (["weight_refresh_table"], []),
    "b01_bf16": (["gemm_wgrad"], ["gemm_wgrad_pair"]),   # width 384: only the 1536-wide fc2 dgrads group
    "b04_bf16_70px_resampled": (["copy2d"], []),
}


@pytest.fixture(scope="module")
def golden():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def count(calls, fn):
    return sum(c[0] == fn for c in calls)


def test_fixture_covers_every_scene(golden):
    assert sorted(golden["scenes"]) == sorted(T.SCENES)
    assert golden["header"]["models"] == json.loads(json.dumps(T.MODELS)) and golden["header"]["parent"]
    assert set(PATH) <= set(T.SCENES)


@pytest.mark.parametrize("scene", sorted(T.SCENES))
def test_trace_matches_fixture(scene, golden):
    watched = [(M, "ops"), (engine, "ops"), (runtime, "ops"), (runtime, "require_device"), (runtime, "to_device"),
               (engine, "pack_bwd"), (M, "_PAIR_FWD"), (M, "_PAIR_DGRAD"), (engine, "GELU_COLSUM"),
               (engine, "QK_COLSUM"), (engine, "_PAIR_WGRAD"), (runtime, "_FUSED_RESID_LN")]
    before = [getattr(o, a) for o, a in watched]
    env = dict(os.environ)
    calls = json.loads(json.dumps(T.run_scene(scene)))   # tuples -> lists, as the fixture has them
    assert all(getattr(o, a) is b for (o, a), b in zip(watched, before)) and dict(os.environ) == env
    assert calls, scene
    made = T.names_of(calls)
    must, must_not = PATH.get(scene, ([], []))
    assert all(n in made for n in must) and not any(n in made for n in must_not), (scene, sorted(set(made)))
    want = golden["scenes"][scene]
    for i, (got, exp) in enumerate(zip(calls, want)):
        if got != exp:
            pytest.fail(f"{scene}: call {i} differs\n  got      {T.dump_call(got)}\n  expected {T.dump_call(exp)}")
    assert len(calls) == len(want), f"{scene}: {len(calls)} calls, the fixture has {len(want)}"


def test_three_steps_build_packs_and_table_once(golden):
    """What the three-step scene is there to pin, read from the fixture itself: the backward packs are
    transposed into place on the first step only (later steps refresh them through the table), the
    refresh table is built once, and every step ends with one refresh launch."""
    calls = golden["scenes"]["a12_three_steps"]
    ends = [i for i, c in enumerate(calls) if c[0] == "weight_refresh_list"]
    assert len(ends) == 3 and count(calls, "weight_refresh_table") == 1
    first, later = calls[:ends[0]], calls[ends[0]:]
    bf16_pack = lambda c: c[0] == "transpose" and c[1][1][4] == "bfloat16"  # noqa: E731
    assert sum(map(bf16_pack, first)) == 4 * 6 and not any(map(bf16_pack, later))   # 2 layers x 3 blocks
    assert [c[1] for c in calls if c[0] == "weight_refresh_list"] == [["refresh_table0"]] * 3


def test_grad_ready_order(golden):
    """The hook's calls as the data-parallel trainer relies on them: the camera head first, then per
    layer from the last the reloc, global and frame blocks, DINO's blocks in reverse, None at the end."""
    order = [c[1][0] for c in golden["scenes"]["b01_bf16"] if c[0] == "grad_ready"]
    want = ["camera_head"]
    for l in (1, 0):
        want += [f"aggregator.{s}.{l}" for s in ("global_reloc_blocks", "global_blocks", "frame_blocks")]
    want += [f"aggregator.patch_embed.blocks.{i}" for i in reversed(range(12))] + [None]
    assert order == want


def test_rebuilt_packs_get_a_fresh_refresh_table():
    """invalidate() drops the packs and the table: after one more step refresh_packs() builds a new
    table, and its items are the NEW packs' tensors (a table kept across invalidate() would refresh
    buffers nobody reads)."""
    with T.Session("a01_bf16") as s:
        s.step(T.CANON, 56)
        old = [t for it in s.rec.tables[0] for t in it if t is not None]
        n_packs = len(s.rec.packs)
        s.tg.invalidate()
        s.step(T.CANON, 56)
        assert len(s.rec.tables) == 2 and len(s.rec.packs) == 2 * n_packs
        new = [t for it in s.rec.tables[1] for t in it if t is not None]
        packs = {id(blk): bp for blk, bp in s.rec.packs[n_packs:]}
        a = s.net.aggregator
        blocks = list(a.frame_blocks) + list(a.global_blocks) + list(a.global_reloc_blocks)
        assert len(s.rec.tables[1]) == 4 * len(blocks)
        for blk in blocks:
            pb, bp = blk._packed[torch.bfloat16], packs[id(blk)]
            for dst in (pb.w_qkv, pb.w_proj, pb.w_fc1, pb.w_fc2, bp.wt_qkv, bp.wt_proj, bp.wt_fc1, bp.wt_fc2):
                assert any(t is dst for t in new) and not any(t is dst for t in old)
        s.step(T.CANON, 56)   # and the new table is then kept
        assert len(s.rec.tables) == 2


def test_entry_point_errors():
    with T.Session("a01_bf16") as s:
        tg = s.tg
        with pytest.raises(RuntimeError):
            tg.backward(torch.zeros(1, 2, 9))
        img = lambda b, n: torch.zeros(b, n, 3, 56, 56)  # noqa: E731
        with pytest.raises(NotImplementedError):
            tg.forward(img(2, 4), [0, 1], [2, 3])
        with pytest.raises(ValueError):
            tg.forward(torch.zeros(1, 4, 1, 56, 56), [0, 1], [2, 3])
        for lists in (([0, 1], [1, 2, 3]), ([0, 1], [3]), ([], [0, 1, 2, 3]), ([0, 1, 2, 3], [])):
            with pytest.raises(ValueError):
                tg.forward(img(1, 4), *lists)
        assert s.rec.calls == []          # nothing was launched before the checks
        s.step(T.CANON, 56)               # and the graph still runs afterwards
        with pytest.raises(RuntimeError):
            tg.backward(torch.zeros(1, 2, 9))   # one backward per forward
