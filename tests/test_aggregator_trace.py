"""The inference Aggregator's launch sequence against its recorded fixture (no GPU, no library).

tests/agg_trace.py runs every scene's forward on CPU tensors behind a recorder in place of ``ops``;
tests/golden/g15_aggregator_trace.json.gz holds the same traces as recorded at the commit its header
names (tests/golden/make_golden_agg_trace.py).  Every forward must make the same ``ops`` calls, with
the same operands and keywords, in the same order: a change of the aggregator's structure must
leave the fixture as it is, and a change of what is launched shows as the first differing call.
Per scene the launch that names its path is asserted too, so that a scene cannot slide onto another
path and still match a fixture recorded the same wrong way."""

import gzip
import json
import os

import pytest

import agg_trace
from sailrecon_amd import ops, runtime
from sailrecon_amd.models import aggregator as A

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_aggregator_trace.json.gz")

# scene -> (launches its path must make, launches it must not)
PATH = {
    "s01_paired": (["attention_pair"], []),
    "s02_paired_whole_tiles": (["attention_pair"], []),
    "s03_split_unpaired": ([], ["attention_pair"]),
    "s04_one_launch_reloc": ([], ["attention_pair"]),
    "s07_camera_bf16": (["attention_rows"], []),
    "s07_camera_fp32": (["attention_rows"], []),
    "s09_shard2_overlap": (["attention_partials", "attn_merge_n"], []),
    "s09_shard2_gathered": ([], ["attention_partials"]),
    "s11_shard2_fp32": (["attn_merge"], []),
    "s13_fp8_global": (["attention_qk8"], []),
}


@pytest.fixture(scope="module")
def golden():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def test_fixture_covers_every_scene(golden):
    assert sorted(golden["scenes"]) == sorted(agg_trace.SCENES)
    assert golden["header"]["model"] == agg_trace.MODEL and golden["header"]["parent"]
    assert set(PATH) <= set(agg_trace.SCENES)


@pytest.mark.parametrize("scene", sorted(agg_trace.SCENES))
def test_trace_matches_fixture(scene, golden):
    watched = [(ops, "_ATTN_PAIR"), (ops, "ROWS_MAX_LQ"), (runtime, "ops"), (runtime, "_GROUP_TAILS"),
               (runtime, "require_device"), (runtime, "to_device"), (A, "ops"), (A, "_RELOC_SPLIT_MIN_WG")]
    before = [getattr(o, a) for o, a in watched]
    env = dict(os.environ)
    calls = json.loads(json.dumps(agg_trace.run_scene(scene)))   # tuples -> lists, as the fixture has them
    assert all(getattr(o, a) is b for (o, a), b in zip(watched, before)) and dict(os.environ) == env
    assert calls, scene
    made = agg_trace.names_of(calls)
    must, must_not = PATH.get(scene, ([], []))
    assert all(n in made for n in must) and not any(n in made for n in must_not), (scene, sorted(set(made)))
    want = golden["scenes"][scene]
    for i, (got, exp) in enumerate(zip(calls, want)):
        if got != exp:
            pytest.fail(f"{scene}: call {i} differs\n  got      {agg_trace.dump_call(got)}\n"
                        f"  expected {agg_trace.dump_call(exp)}")
    assert len(calls) == len(want), f"{scene}: {len(calls)} calls, the fixture has {len(want)}"


def test_sizes_are_the_issue_s():
    """The shapes the scenes are built around: P = 32 tokens, head_dim 64, and with fix_rank 9 a
    ragged subsample (400 rows, 384 in whole 64-key tiles)."""
    m = agg_trace.MODEL
    P = (m["img_size"] // m["patch_size"]) ** 2 + 1 + m["num_register_tokens"]
    assert P == 32 and m["embed_dim"] // m["num_heads"] == 64
    s = agg_trace.SCENES["s01_paired"]
    n_sub = s["Na"] * (s["fix_rank"] + 1 + m["num_register_tokens"])
    assert (n_sub, n_sub // 64 * 64) == (400, 384)
    s = agg_trace.SCENES["s02_paired_whole_tiles"]
    assert s["Na"] * (s["fix_rank"] + 1 + m["num_register_tokens"]) == 512
