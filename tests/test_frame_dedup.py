"""The host side of the DINO frame dedup (sailrecon_amd/frame_dedup.py): ``rep`` -> (distinct
frames, slot of each frame, row map), and the headline's kernel plans at both frame counts."""

import numpy as np
import pytest
import torch

from sailrecon_amd.frame_dedup import dino_plan, group_frames


def brute(rep, P):
    """Row by row: frame f's rows read the rows of its representative's slot."""
    rep = list(rep)
    uniq = [f for f in range(len(rep)) if rep[f] == f]
    slot = [uniq.index(rep[f]) for f in range(len(rep))]
    rowmap = [slot[f] * P + t for f in range(len(rep)) for t in range(P)]
    return uniq, slot, rowmap


CASES = {
    "identity": [0, 1, 2, 3, 4],
    "demo": [0, 1, 2, 0, 1, 2],                    # anchors, then the same images as queries
    "interleaved": [0, 1, 0, 1, 4, 0],
    "triples": [0, 0, 0, 3, 3, 3],
    "b2": [0, 1, 0, 1, 4, 5, 4, 5],                # two batch items, each its own demo pattern
    "across_items": [0, 1, 0, 1, 0, 1, 0, 1],      # B = 2 with the same scene twice
    "single": [0],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("P", [1, 21])
def test_group_frames(name, P):
    rep = np.array(CASES[name], dtype=np.int32)
    uniq, slot, rowmap = group_frames(rep, P)
    bu, bs, br = brute(rep, P)
    assert uniq.dtype == slot.dtype == rowmap.dtype == np.int32
    assert uniq.tolist() == bu and slot.tolist() == bs and rowmap.tolist() == br
    # the compact stream gathers back to the full one: frame f's rows come from frame rep[f]'s
    compact = np.repeat(uniq, P) * 1000 + np.tile(np.arange(P), len(uniq))
    full = np.repeat(rep, P) * 1000 + np.tile(np.arange(P), len(rep))
    assert np.array_equal(compact[rowmap], full)
    if name == "identity":
        assert np.array_equal(rowmap, np.arange(len(rep) * P))


def test_group_frames_keeps_doubtful_entries_distinct():
    """An entry that names no earlier self-representing frame never merges two frames."""
    # rep[1] points forward, rep[2] is negative, rep[4] names frame 3 which names frame 0
    uniq, slot, _ = group_frames([0, 3, -1, 0, 3], 2)
    assert uniq.tolist() == [0, 1, 2, 4] and slot.tolist() == [0, 1, 2, 0, 3]


def test_headline_plans_agree():
    """ViT-L at 518 px, 32 distinct frames of 64: no split-K, no few-row tile, the same attention
    workgroup shape and no key split at either count, so the dedup changes no kernel choice."""
    full = dino_plan(64, 1374, 1024, 4096, 16, torch.bfloat16)
    half = dino_plan(32, 1374, 1024, 4096, 16, torch.bfloat16)
    assert full == half == ((1, 1, 1, 1), False, True, 1)
    # and a small shape where it does: fc2's K splits differently at 84 and at 252 rows
    assert dino_plan(4, 21, 384, 1536, 6, torch.float32) != dino_plan(12, 21, 384, 1536, 6, torch.float32)
