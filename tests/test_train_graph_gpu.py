"""Whole training graph: TrainGraph.forward + backward on the HIP path
against torch autograd through the CPU oracle (aggregator_forward + camera_head_forward, the
reference's literal algorithm incl. dense reloc mask and the camera head's detach) with the same
weights, inputs and subsample draws.  Loss = <d, pose_enc of the last iteration>, so every
parameter that the reference's compute_loss reaches gets a gradient.

Small ViT-S/14 DINO + 2-layer aggregator (embed 384, head_dim 64) + 2-block camera head
(dim 768, head_dim 128) at 56 px, 2 views duplicated (4 frames), fix_rank 10 < 16 patches so
the anchor subsample is exercised.  The aggregator runs in bf16 (as train_imc.py's autocast)
against the fp32 oracle: per-parameter rel-L2 <= 4e-2, median <= 2e-2 (measured on MI355X:
worst 1.4e-2, the k-norm biases of the first layer)."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Hot(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from sailrecon_amd.heads.camera_head import CameraHead
        from sailrecon_amd.models.aggregator import Aggregator
        self.aggregator = Aggregator(img_size=56, patch_size=14, embed_dim=384, depth=2, num_heads=6,
                                     patch_embed="dinov2_vits14_reg", intermediate_layer_idx=[0, 1])
        self.camera_head = CameraHead(dim_in=768, trunk_depth=2, num_heads=6)


def _reference_grads(sd, images, sub, d, no_reloc, reloc):
    from oracle import sfm_oracle as O
    ref = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    cfg = O.AggCfg(patch=14, embed_dim=384, depth=2, heads=6, dino_depth=12, dino_heads=6, inter_idx=(0, 1))
    feats, _, cam_last = O.aggregator_forward(ref, cfg, images, no_reloc, reloc, 10, sub)
    poses = O.camera_head_forward(ref, feats[-1], cam_last, heads=6, trunk_depth=2)
    (poses[-1] * d).sum().backward()
    return poses[-1].detach(), {k: v.grad for k, v in ref.items() if v.is_floating_point()}


CASES = [(([0, 1], [2, 3]), 56), (([3, 1], [0, 2]), 56), (([0, 1], [2, 3]), 70)]
CASE_IDS = ["canonical", "frame0_query", "pos_resampled_70"]


def _run_graph(lists, px, compute_dtype):
    """TrainGraph forward + backward of <d, pose> and the oracle's fp32 autograd of the same."""
    no_reloc, reloc = lists
    from sailrecon_amd.train.model import TrainGraph
    from sailrecon_amd.utils.synth_weights import synth_state_dict_like
    torch.manual_seed(0)
    m = Hot()
    sd = synth_state_dict_like(m)
    m.load_state_dict(sd)
    m = m.to(DEV)
    tg = TrainGraph(m, compute_dtype=compute_dtype)
    n = 2
    x = torch.rand(n, 3, px, px, generator=torch.Generator().manual_seed(1))
    images = torch.cat([x, x])[None]
    m.aggregator.generator.manual_seed(0)
    pose = tg.forward(images.to(DEV), no_reloc, reloc, fix_rank=10)
    d = torch.randn(1, n, 9, generator=torch.Generator().manual_seed(2))
    tg.flat.zero_grad()
    tg.backward(d.to(DEV))
    torch.cuda.synchronize()
    sub = m.aggregator.last_subsample_indices
    ref_pose, ref_g = _reference_grads(sd, images, sub, d, no_reloc, reloc)
    errs = {}
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        rg = ref_g.get(name)
        if rg is None or float(rg.norm()) == 0.0:
            assert float(p.grad.norm()) == 0.0, f"{name}: reference grad is zero, ours is not"
            continue
        errs[name] = rel(p.grad, rg)
    return rel(pose, ref_pose), errs


@pytest.mark.parametrize("lists,px", CASES, ids=CASE_IDS)
def test_train_graph_fp32_matches_autograd(lists, px):
    """the whole training graph in fp32 (TrainGraph compute_dtype=fp32: exact
    fp32 GEMMs, attention forward and sr_attention_bwd_f32) against the oracle's fp32 autograd, at
    1e-4 rel-L2 per parameter -- far below the few-% shift a wiring error in the backward
    orchestration (dK/dV segment offsets, the subsample-gather adjoint, LayerNorm row maps, the
    special-token / pos-embed adjoints) would cause, which the bf16 graph's 4e-2 bound could hide.
    The bf16-only launch forms (grouped dgrads, paired wgrads, the concatenated-items dK/dV sweep)
    compute per-tile / per-item the same products as their one-problem forms (bit-identity tests in
    test_kernels_gpu.py / test_attn_bwd_gpu.py); here each block takes its one-problem form."""
    perr, errs = _run_graph(lists, px, torch.float32)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:8]
    print(f"fp32 graph: pose rel {perr:.2e}; worst grads:", worst)
    assert perr < 1e-5
    assert worst[0][1] < 1e-4, worst


@pytest.mark.parametrize("lists,px", CASES, ids=CASE_IDS)
def test_train_graph_matches_autograd(lists, px):
    """``frame0_query``: interleaved lists with original frame 0 a query, so no anchor takes
    camera_token[:, 0] (the special-token grads follow the forward's types).
    ``pos_resampled_70``: 70 px input on the 56 px model, so DINO's pos_embed is resampled
    (interpolate_pos_encoding) and its grad goes through the bicubic adjoint (VERDICT r3
    missing 3)."""
    perr, errs = _run_graph(lists, px, torch.bfloat16)
    assert perr < 2e-2
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:8]
    print("worst grads:", worst)
    med = sorted(errs.values())[len(errs) // 2]
    assert med < 2e-2, f"median grad rel-L2 {med}"
    assert worst[0][1] < 4e-2, worst


def test_train_graph_bias_colsum_modes(monkeypatch):
    """SR_TRAIN_BIAS_COLSUM: the bf16 bias grads of fc1 (GELU_BWD epilogue column sums) and of qkv
    (sr_qk_bwd's) against the separate column sums of dU / d(q|k|v) they replace -- the same
    bf16-rounded addends summed in another order (~1e-6); every other gradient bit-identical."""
    from sailrecon_amd.train import engine
    from sailrecon_amd.train.model import TrainGraph
    from sailrecon_amd.utils.synth_weights import synth_state_dict_like
    grads = []
    for mode in (3, 0):
        monkeypatch.setattr(engine, "GELU_COLSUM", bool(mode & 1))
        monkeypatch.setattr(engine, "QK_COLSUM", bool(mode & 2))
        torch.manual_seed(0)
        m = Hot()
        m.load_state_dict(synth_state_dict_like(m))
        m = m.to(DEV)
        tg = TrainGraph(m)
        x = torch.rand(2, 3, 56, 56, generator=torch.Generator().manual_seed(1))
        m.aggregator.generator.manual_seed(0)
        tg.forward(torch.cat([x, x])[None].to(DEV), [0, 1], [2, 3], fix_rank=10)
        tg.flat.zero_grad()
        tg.backward(torch.randn(1, 2, 9, generator=torch.Generator().manual_seed(2)).to(DEV))
        torch.cuda.synchronize()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad})
    fused, plain = grads
    n_bias = 0
    for name, g in fused.items():
        if name.endswith(("fc1.bias", "qkv.bias")) and "aggregator" in name:
            n_bias += 1
            assert rel(g, plain[name]) < 1e-4, name
        else:
            assert torch.equal(g, plain[name]), name
    assert n_bias > 0
