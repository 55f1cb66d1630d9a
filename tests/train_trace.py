"""TrainGraph's launch sequence, traced on the CPU (no GPU, no library).

train.model reaches the device only through ``ops``, ``train.engine`` and ``runtime``, which call
``ops`` themselves.  With one recorder in place of all three modules' ``ops`` and a no-op
``runtime.require_device`` whole training steps (``forward`` + ``backward`` + ``refresh_packs``) run
on CPU tensors and leave the list of their launches, normalised as tests/agg_trace.py does (its
Recorder is the base class here).  Buffers are named by what owns their storage:

  * the graph's workspaces by their workspace names (``sc2:`` in front for the global block's second
    scratch), ``delta`` for the attention backward's row-sum buffer;
  * ``tape.<kind>.<index>.<field>`` for block tapes; packed weights ``<block>.<field>`` and backward
    packs ``bwd.<block>.<field>`` with the block's qualified module name;
  * ``flat.data`` / ``flat.grad`` for everything that lives in the flat parameter / gradient buffer
    (fp32 packed fields alias it): the storage offset then says which parameter it is;
  * ``rope.cos`` / ``rope.sin``, ``misc.<field>``, ``tables`` for host index tables, ``new<k>`` else.

``weight_refresh_table`` is answered here (its items recorded, a token returned) and every
``grad_ready_hook`` call is recorded as a pseudo-call ``["grad_ready", [module name], {}]``.
SCENES are what tests/golden/g16_train_graph_trace.json.gz pins (make_golden_train_trace.py)."""

from __future__ import annotations

import contextlib
import zlib

import torch

import agg_trace
from agg_trace import BF16, F32, _storage, default_switches, name_fields, name_workspace, patched
from sailrecon_amd import runtime
from sailrecon_amd.heads.camera_head import CameraHead
from sailrecon_amd.models.aggregator import Aggregator
from sailrecon_amd.train import engine
from sailrecon_amd.train import model as M

MODEL_A = dict(img_size=56, patch_size=14, embed_dim=256, depth=2, num_heads=4, patch_embed="conv",
               intermediate_layer_idx=[0, 1], min_rank=4)
HEAD_A = dict(dim_in=512, trunk_depth=2, num_heads=4)
MODEL_B = dict(img_size=56, patch_size=14, embed_dim=384, depth=2, num_heads=6, patch_embed="dinov2_vits14_reg",
               intermediate_layer_idx=[0, 1])   # the ``Hot`` model of tests/test_train_graph_gpu.py
HEAD_B = dict(dim_in=768, trunk_depth=2, num_heads=6)
MODELS = {"A": (MODEL_A, HEAD_A), "B": (MODEL_B, HEAD_B)}


class Net(torch.nn.Module):
    def __init__(self, which: str, **agg_kw):
        super().__init__()
        agg, head = MODELS[which]
        self.aggregator = Aggregator(**dict(agg, **agg_kw))
        self.camera_head = CameraHead(**head)


class Recorder(agg_trace.Recorder):
    """agg_trace.Recorder for a TrainGraph: the training buffers' names, the host helpers that would
    load the library, the refresh tables and the backward packs as they are made."""

    PURE = ("ACT_GELU", "ACT_SILU", "RESIDUAL_LN_COLS")

    def __init__(self, tg):
        super().__init__(tg.agg)
        self.tg = tg
        self.tables = []          # the items of every weight_refresh_table, as passed
        self.packs = []           # (block, BwdPack) of every engine.pack_bwd that made a pack
        self._mod = {id(m): n for n, m in tg.model.named_modules()}

    # ---- answered here: the real ones load the library
    def colsum_blocks(self, M_):
        return (M_ + 63) // 64

    def gemm_group_eligible(self, problems):  # ops.gemm_group_eligible's rule
        return 1 <= len(problems) <= 4 and all(p["a"].dtype == BF16 and p["w"].shape[0] % 256 == 0 for p in problems)

    def wgrad_pair_splits(self, M0, M1, N, K):  # ops.wgrad_pair_splits' rule
        if N % 256 or K % 256:
            return None
        per = 256 // ((N // 256) * (K // 256))
        if per < 2 or per % 2:
            return None
        s = min(per // 2, 16)
        return max(1, min(s, -(-M0 // 64) // 8)), max(1, min(s, -(-M1 // 64) // 8))

    def weight_refresh_table(self, items, device):
        self.tables.append(items)
        self.calls.append(["weight_refresh_table", self.norm([list(it) for it in items]), {}])
        return f"refresh_table{len(self.tables) - 1}"

    def pack_bwd(self, blk, pb, dtype, into=None):
        """In place of engine.pack_bwd: remembers the packs it makes."""
        out = _pack_bwd(blk, pb, dtype, into=into)
        if into is None:
            self.packs.append((blk, out))
        return out

    def grad_ready(self, module) -> None:
        self.calls.append(["grad_ready", [None if module is None else self._mod[id(module)]], {}])

    # ---- names
    def _names(self) -> dict:
        names, tg = super()._names(), self.tg
        for n, m in tg.model.named_modules():
            if n.startswith(("aggregator.patch_embed.", "camera_head.")) and isinstance(getattr(m, "_packed", None), dict):
                for pb in m._packed.values():
                    if isinstance(pb, runtime.PackedBlock):
                        name_fields(names, n, pb)
        for blk, bp in self.packs:
            name_fields(names, "bwd." + self._mod[id(blk)], bp)
        for key, tape in tg._tapes.items():
            name_fields(names, "tape." + ".".join(str(k) for k in key), tape)
        name_workspace(names, tg._sc)
        name_workspace(names, tg._sc2, "sc2:")
        for t in engine._DELTA.values():
            names[_storage(t)] = "delta"
        names[_storage(tg.flat.data)], names[_storage(tg.flat.grad)] = "flat.data", "flat.grad"
        return names


_pack_bwd = engine.pack_bwd

CANON, MIXED = ([0, 1], [2, 3]), ([3, 1], [0, 2])   # MIXED: frame 0 a query, the anchors' type runs mixed


def _scene(model="A", dtype=BF16, steps=((CANON, 56),), fix_rank=10, agg_kw=None, **switches):
    return dict(model=model, dtype=dtype, steps=list(steps), fix_rank=fix_rank, agg_kw=agg_kw or {}, switches=switches)


PLAIN = dict(qk_norm=False, rope_freq=-1)   # no qk-norm, no RoPE: the plain-bias K/V projection
# name -> scene: ``steps`` training steps ((no_reloc, reloc), pixels) on ONE TrainGraph, each followed
# by refresh_packs(); the switches not named keep their defaults (everything on)
SCENES = {
    "a01_bf16": _scene(),
    "a02_fp32": _scene(dtype=F32),
    "a03_bf16_frame0_query": _scene(steps=[(MIXED, 56)]),
    "a04_bf16_70px": _scene(steps=[(CANON, 70)]),
    "a05_plain_kv_bf16": _scene(agg_kw=PLAIN),
    "a06_plain_kv_fp32": _scene(agg_kw=PLAIN, dtype=F32),
    "a07_rank_clipped": _scene(fix_rank=300),
    "a08_rank_drawn": _scene(fix_rank=None),
    "a09_pair_fwd_off": _scene(pair_fwd=False),
    "a10_pair_dgrad_off": _scene(pair_dgrad=False),
    "a11_bias_colsum_off": _scene(bias_colsum=False),
    "a12_three_steps": _scene(steps=[(CANON, 56), (CANON, 56), (CANON, 70)]),
    "b01_bf16": _scene(model="B"),
    "b02_fp32": _scene(model="B", dtype=F32),
    "b03_bf16_frame0_query": _scene(model="B", steps=[(MIXED, 56)]),
    "b04_bf16_70px_resampled": _scene(model="B", steps=[(CANON, 70)]),
    "b05_fp32_frame0_query_70px": _scene(model="B", dtype=F32, steps=[(MIXED, 70)]),
}


class Session:
    """One scene's TrainGraph on the CPU behind the recorder, for as long as the ``with`` block lasts."""

    def __init__(self, name: str):
        self.scene = s = SCENES[name]
        sw = dict(dict(pair_fwd=True, pair_dgrad=True, bias_colsum=True), **s["switches"])
        torch.manual_seed(0)
        self.net = Net(s["model"], **s["agg_kw"])
        self.tg = M.TrainGraph(self.net, compute_dtype=s["dtype"])
        self.net.aggregator.generator.manual_seed(zlib.crc32(name.encode()))   # seeded per scene
        self.rec = rec = Recorder(self.tg)
        self.tg.grad_ready_hook = rec.grad_ready
        to_device = runtime.to_device
        self._pairs = [(M, "ops", rec), (engine, "ops", rec), (runtime, "ops", rec),
                       (runtime, "require_device", lambda t, who: None),
                       (runtime, "to_device", lambda t, dev: rec.host_table(to_device(t, dev))),
                       (engine, "pack_bwd", rec.pack_bwd),
                       (M, "_PAIR_FWD", sw["pair_fwd"]), (M, "_PAIR_DGRAD", sw["pair_dgrad"]),
                       (engine, "GELU_COLSUM", sw["bias_colsum"]), (engine, "QK_COLSUM", sw["bias_colsum"]),
                       (engine, "_PAIR_WGRAD", True), (runtime, "_FUSED_RESID_LN", False)]
        self._stack = None

    def __enter__(self):
        self._stack = contextlib.ExitStack()
        self._stack.enter_context(default_switches())
        self._stack.enter_context(patched(self._pairs))
        self._stack.enter_context(torch.no_grad())
        return self

    def __exit__(self, *exc):
        self._stack.close()

    def step(self, lists, px: int, fix_rank="scene"):
        """One forward + backward + refresh_packs; the images and the pose gradient do not enter the trace."""
        n = len(lists[0]) + len(lists[1])
        pose = self.tg.forward(torch.zeros(1, n, 3, px, px), lists[0], lists[1],
                               fix_rank=self.scene["fix_rank"] if fix_rank == "scene" else fix_rank)
        self.tg.backward(torch.zeros_like(pose))
        self.tg.refresh_packs()


def run_scene(name: str) -> list:
    """The normalised launch trace of scene ``name``; everything it patches is restored."""
    with Session(name) as s:
        for lists, px in s.scene["steps"]:
            s.step(lists, px)
    return s.rec.calls


dump_call, names_of = agg_trace.dump_call, agg_trace.names_of
