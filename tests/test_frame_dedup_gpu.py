"""The DINO frame dedup of Aggregator._embed (SR_DEDUP_FRAMES, default on) against the same model
with the switch off, on the small model of test_camera_only_gpu.py (56 / 70 px, depth 2).

Scenes are built by repeating the golden cases' anchor images.  Every case is held to
goldens.PARITY_TOL[mode]; where the DINO blocks' kernel plans (frame_dedup.dino_plan: split-K
slices, sr_gemm's few-row tile, the attention's workgroup shape and key split) agree between the
U distinct and the F total frames, the outputs must be bit-equal (torch.equal):

  bit-equal:     b2_demo_n9 (36 frames -> 18: 378 against 756 rows, no split-K at either),
                 partial_n9 (18 -> 13: 273 against 378 rows), partial_70 (6 -> 4: fc2's K in 4
                 slices at both), all_distinct (U = F, the parent's path); in bf16 also demo_70
  PARITY_TOL:    every other case.  demo_n9, demo_70 (fp32), triples and b2_same_scene: at
                 U * P <= 256 rows ops._splitk_plan cuts the K of the GEMMs into more slices
                 than at F * P rows; demo_56, interleaved, triples and b2_same_scene: at
                 U * P = 42 <= 64 rows sr_gemm takes its 64 x 256 few-row tile
"""

import numpy as np
import pytest
import torch
import torch.nn as nn

from goldens import PARITY_TOL, load_npz, parity_tol, rel_l2, rule_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
AGG_KW = dict(img_size=56, patch_size=14, embed_dim=384, depth=2, num_heads=6, patch_embed="dinov2_vits14_reg",
              intermediate_layer_idx=[0, 1])


class Hot(nn.Module):
    def __init__(self, agg_kw, cam_kw):
        super().__init__()
        from sailrecon_amd.heads.camera_head import CameraHead
        from sailrecon_amd.models.aggregator import Aggregator
        self.aggregator = Aggregator(**agg_kw)
        self.camera_head = CameraHead(**cam_kw)


@pytest.fixture(scope="module")
def small_model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)
    m = Hot(AGG_KW, dict(dim_in=768, trunk_depth=2, num_heads=6)).eval()
    m.load_state_dict(rule_state_dict("small_state_dict_keys.json"))
    return m.to(DEV)


def anchors(tag):
    g = load_npz(f"{tag}.npz")
    n = int(g["n_views"])
    return torch.from_numpy(g["images"][0, :n])  # [n, 3, H, W]


def other(a):
    """New images of the same size (test_camera_only_gpu's second scene)."""
    return a.flip(0).roll(1, dims=-1) * 0.9 + 0.05


def scenes():
    """name -> (images [B, S, 3, H, W], no_reloc, reloc, distinct frames U)."""
    a2, a3, a9 = anchors("g1_small_56"), anchors("g1_small_70"), anchors("g1_small_56_n9")
    s = {}
    s["demo_56"] = (torch.cat([a2, a2])[None], [0, 1], [2, 3], 2)
    s["demo_70"] = (torch.cat([a3, a3])[None], [0, 1, 2], [3, 4, 5], 3)
    s["demo_n9"] = (torch.cat([a9, a9])[None], list(range(9)), list(range(9, 18)), 9)
    s["interleaved"] = (a2[[0, 0, 1, 1]][None], [0, 2], [1, 3], 2)
    q = a3.clone()
    q[1] = other(a3)[1]
    s["partial_70"] = (torch.cat([a3, q])[None], [0, 1, 2], [3, 4, 5], 4)      # one query is a new image
    q = a9.clone()
    q[4:] = other(a9)[4:]
    q[8] = a9[8]
    s["partial_n9"] = (torch.cat([a9, q])[None], list(range(9)), list(range(9, 18)), 13)
    s["triples"] = (a2[[0, 1, 0, 0, 1, 1]][None], [0, 1], [2, 3, 4, 5], 2)
    s["b2_demo_n9"] = (torch.stack([torch.cat([a9, a9]), torch.cat([other(a9), other(a9)])]),
                       list(range(9)), list(range(9, 18)), 18)
    s["b2_same_scene"] = (torch.stack([torch.cat([a2, a2])] * 2), [0, 1], [2, 3], 2)
    s["all_distinct"] = (torch.cat([a9, other(a9)])[None], list(range(9)), list(range(9, 18)), 18)
    return s


SCENES = sorted(scenes())
BIT_EQUAL = {"fp32": {"b2_demo_n9", "partial_n9", "partial_70", "all_distinct"},
             "bf16": {"b2_demo_n9", "partial_n9", "partial_70", "all_distinct", "demo_70"}}


def run(model, images, lists, mode, fix_rank=10):
    from sailrecon_amd.utils.pose_enc import pose_encoding_to_extri_intri
    model.aggregator.generator.manual_seed(0)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "bf16")):
        feats, psi, cam_last = model.aggregator(images, lists[0], lists[1], fix_rank=fix_rank)
        with torch.autocast("cuda", enabled=False):
            poses = model.camera_head(feats, cam_last)
            ext, intr = pose_encoding_to_extri_intri(poses[-1], (images.shape[-2], images.shape[-1]))
    torch.cuda.synchronize()
    return dict(feat_0=feats[0].clone(), feat_1=feats[1].clone(), cam_token_last_layer=cam_last.clone(),
                pose_enc=torch.stack(list(poses)), extrinsic=ext, intrinsic=intr,
                sub=model.aggregator.last_subsample_indices.clone()), model.aggregator.last_frame_groups


def plans_agree(U, F_, P, mode):
    from sailrecon_amd.frame_dedup import dino_plan
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    return dino_plan(U, P, 384, 1536, 6, dt) == dino_plan(F_, P, 384, 1536, 6, dt)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_bit_equal_cases_qualify(mode):
    """At least one duplicated scene per dtype takes the torch.equal check, and BIT_EQUAL is exactly
    the set of scenes whose plans agree (the docstring's table, pinned)."""
    qualify = set()
    for name, (images, _, _, U) in scenes().items():
        F_ = images.shape[0] * images.shape[1]
        P = (images.shape[-1] // 14) ** 2 + 5
        if plans_agree(U, F_, P, mode):
            qualify.add(name)
    assert qualify == BIT_EQUAL[mode]
    assert {"b2_demo_n9", "partial_n9"} <= qualify  # duplicated scenes, not only U == F


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", SCENES)
def test_dedup_on_vs_off(small_model, name, mode, monkeypatch):
    from sailrecon_amd.models import aggregator as A
    images, no_reloc, reloc, U = scenes()[name]
    images = images.to(DEV)
    F_ = images.shape[0] * images.shape[1]
    P = (images.shape[-1] // 14) ** 2 + 5
    monkeypatch.setattr(A, "_DEDUP_FRAMES", False)
    off, groups_off = run(small_model, images, (no_reloc, reloc), mode)
    assert groups_off == (F_, F_)
    monkeypatch.setattr(A, "_DEDUP_FRAMES", True)
    on, groups_on = run(small_model, images, (no_reloc, reloc), mode)
    assert groups_on == (F_, U)
    assert torch.equal(on["sub"], off["sub"])
    err = {k: rel_l2(on[k].cpu().numpy(), off[k].cpu().numpy()) for k in off if k != "sub"}
    exact = plans_agree(U, F_, P, mode)
    print(f"DEDUP-vs-OFF {name} {mode} U={U}/{F_} exact={exact}:", {k: float(f"{v:.3e}") for k, v in err.items()})
    bad = {k: (v, parity_tol(k, mode)) for k, v in err.items() if not v < parity_tol(k, mode)}
    assert not bad, bad
    assert exact == (name in BIT_EQUAL[mode])
    if exact:
        for k in off:
            assert torch.equal(on[k], off[k]), (name, mode, k)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["g1_small_56", "g1_small_70", "g1_small_56_n9"])
def test_goldens_with_dedup(small_model, tag, mode):
    """The reference goldens (queries = the anchor images again) with the switch on: the dedup runs
    and the outputs stay within the goldens' bounds."""
    g = load_npz(f"{tag}.npz")
    images = torch.from_numpy(g["images"]).to(DEV)
    n = int(g["n_views"])
    r, groups = run(small_model, images, (list(range(n)), list(range(n, 2 * n))), mode, int(g["fix_rank"]))
    assert groups == (2 * n, n)
    assert np.array_equal(r["sub"][:, 0].numpy(), g["sub_idx"])
    err = {k: rel_l2(r[k].cpu().numpy(), g[k]) for k in r if k != "sub"}
    print(f"PARITY {tag} {mode} dedup:", {k: float(f"{v:.3e}") for k, v in err.items()})
    bad = {k: (v, parity_tol(k, mode)) for k, v in err.items() if not v < parity_tol(k, mode)}
    assert not bad, bad


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_cached_forward_on_vs_off(mode, monkeypatch):
    """The anchors-only cache-filling forward (SailRecon.tmp_forward's aggregator call) and
    forward_with_cache go through _embed too: duplicated anchors and duplicated queries."""
    from sailrecon_amd.models import aggregator as A
    from sailrecon_amd.models.aggregator import Aggregator
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)
    agg = Aggregator(kv_cache=True, **AGG_KW).eval()
    sd = {k[len("aggregator."):]: v for k, v in rule_state_dict("small_state_dict_keys.json").items()
          if k.startswith("aggregator.")}
    agg.load_state_dict(sd)
    agg = agg.to(DEV)
    a9 = anchors("g1_small_56_n9")
    scene = a9[[0, 1, 2, 0, 1, 3]][None].to(DEV)   # anchors with repeats
    queries = a9[[4, 4, 0, 5]][None].to(DEV)       # queries with repeats
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(A, "_DEDUP_FRAMES", on)
        agg.generator.manual_seed(0)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "bf16")):
            feats, _, cam = agg(scene, list(range(6)), [], fix_rank=10)
            g_scene = agg.last_frame_groups
            maps, _ = agg.forward_with_cache(queries, fix_rank=10)
            g_query = agg.last_frame_groups
        torch.cuda.synchronize()
        # anchors only: the scene leaves the anchors' camera tokens and the cache the queries then read
        outs[on] = dict(cam=cam.clone(), query_0=maps[0].clone(), query_1=maps[1].clone())
        assert g_scene == (6, 4 if on else 6) and g_query == (4, 3 if on else 4)
    err = {k: rel_l2(outs[True][k].cpu().numpy(), outs[False][k].cpu().numpy()) for k in outs[False]}
    print(f"DEDUP-vs-OFF cached {mode}:", {k: float(f"{v:.3e}") for k, v in err.items()})
    assert all(v < PARITY_TOL[mode]["feat"] for v in err.values()), err
