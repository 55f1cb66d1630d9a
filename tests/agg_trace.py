"""The inference Aggregator's launch sequence, traced on the CPU (no GPU, no library).

The aggregator reaches the device only through ``ops`` and through ``runtime``, which itself calls
``ops``.  With a Recorder in place of ``aggregator.ops`` and ``runtime.ops`` and a no-op
``runtime.require_device`` a whole ``Aggregator.forward`` runs on CPU tensors and leaves the list of
its launches: per call ``[name, args, kwargs]`` with

  * every tensor as ``[base, storage_offset, shape, stride, dtype]`` (int32 tensors -- row maps,
    camera-row tables -- also carry a hash of their contents), ``base`` the NAME of the buffer whose
    storage the tensor lives in: the Workspace buffer's, ``frame_blocks.<l>.<packed field>`` and the
    like for packed weights, ``misc.<field>``, ``rope.cos`` / ``rope.sin``, ``tables`` for the
    per-forward host table, ``kv_cache.<l>``, the ``name=`` of a recorder-made key_split_workspace
    buffer, ``new<k>`` by order of first appearance for anything else (output maps, cam_loc);
  * dict keys sorted, floats by ``repr``, dtypes / devices / other objects by name.

Names are resolved when the call is made and every recorded tensor is kept alive, so a regrown
workspace buffer cannot hand its address to another tensor: the trace does not depend on addresses.
SCENES are the forwards tests/golden/g15_aggregator_trace.json.gz pins (make_golden_agg_trace.py)."""

from __future__ import annotations

import contextlib
import dataclasses
import hashlib
import json
import os

import torch

from sailrecon_amd import ops as real_ops
from sailrecon_amd import runtime
from sailrecon_amd.models import aggregator as A

# answered by the real ops module (pure host helpers; read at call time, so a patched switch holds)
PURE = ("gemm_group_eligible", "pair_eligible", "key_split_parts", "vt_tile_shape", "PAIR_VT", "ROWS_MAX_LQ",
        "RESIDUAL_LN_COLS", "Fp8Workspace")

MODEL = dict(img_size=56, patch_size=14, embed_dim=256, depth=3, num_heads=4, num_register_tokens=15,
             patch_embed="conv", intermediate_layer_idx=[2])
STACKS = ("frame_blocks", "global_blocks", "global_reloc_blocks")


def _storage(t: torch.Tensor) -> int:
    return t.untyped_storage().data_ptr()


def name_fields(names: dict, prefix: str, obj) -> None:
    """``prefix.<field>`` for every tensor field of a dataclass (a packed block, a backward pack, a tape)."""
    for f in dataclasses.fields(obj):
        t = getattr(obj, f.name)
        if isinstance(t, torch.Tensor):
            names[_storage(t)] = f"{prefix}.{f.name}"


def name_workspace(names: dict, ws, prefix: str = "") -> None:
    """A runtime.Workspace's buffers by their workspace names."""
    for name, t in ws._bufs.items():
        names[_storage(t)] = prefix + name


class Recorder:
    """Stands in for the ops module: records the normalised (name, args, keywords) of every call.
    A subclass names further buffers (``_names``) and answers further helpers (tests/train_trace.py)."""

    PURE = PURE

    def __init__(self, agg):
        self.calls, self.agg = [], agg
        self._keep, self._new, self._tables, self._ksplit = [], {}, {}, {}

    # ---- answered here: the real one allocates a per-stream device workspace
    def key_split_workspace(self, device, parts, rows, cols, heads, name="attn_ksplit"):
        n_o = (parts * rows * cols + 1) // 2
        need = n_o + parts * heads * rows
        ws = self._ksplit.get(name)
        if ws is None or ws.numel() < need:
            ws = self._ksplit[name] = torch.zeros(need, dtype=torch.float32)
        o_parts = ws[:n_o].view(torch.bfloat16)[:parts * rows * cols].view(parts * rows, cols)
        return o_parts, ws[n_o:n_o + parts * heads * rows].view(parts, heads, rows)

    def host_table(self, t):
        """runtime.to_device's result: the per-forward host table."""
        self._tables[_storage(t)] = t
        return t

    def __getattr__(self, fn):
        if fn in self.PURE:
            return getattr(real_ops, fn)
        if fn.startswith("__"):
            raise AttributeError(fn)

        def record(*args, **kw):
            self.calls.append([fn, self.norm(list(args)), self.norm(kw)])
            return args[3] if fn == "vt_tiles" else None
        return record

    # ---- names
    def _names(self) -> dict:
        agg, names = self.agg, {}
        for k, t in self._new.items():
            names[k] = t[0]
        for k in self._tables:
            names[k] = "tables"
        for name, t in self._ksplit.items():
            names[_storage(t)] = name
        for l, t in enumerate(agg._kv_cache_layers or []):
            if t is not None:
                names[_storage(t)] = f"kv_cache.{l}"
        if agg.rope is not None:
            for cos, sin in agg.rope._tables.values():
                names[_storage(cos)], names[_storage(sin)] = "rope.cos", "rope.sin"
        for key, d in agg._packed.items():
            if isinstance(d, dict):
                for f, t in d.items():
                    names[_storage(t)] = f"{key[0]}.{f}"
        for stack in STACKS:
            for l, blk in enumerate(getattr(agg, stack)):
                for pb in blk._packed.values():
                    name_fields(names, f"{stack}.{l}", pb)
        name_workspace(names, agg._ws)
        return names

    def _tensor(self, t: torch.Tensor, names: dict) -> list:
        self._keep.append(t)
        key = _storage(t)
        if key not in names:
            names[key] = f"new{len(self._new)}"
            self._new[key] = (names[key], t)
        out = [names[key], t.storage_offset(), list(t.shape), list(t.stride()), str(t.dtype).replace("torch.", "")]
        if t.dtype == torch.int32:
            out.append(hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()[:12])
        return out

    def norm(self, v, names=None):
        names = self._names() if names is None else names
        if isinstance(v, torch.Tensor):
            return self._tensor(v, names)
        if isinstance(v, dict):
            return {k: self.norm(v[k], names) for k in sorted(v)}
        if isinstance(v, (list, tuple)):
            return [self.norm(x, names) for x in v]
        if isinstance(v, float):
            return repr(v)
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        return type(v).__name__


@contextlib.contextmanager
def patched(pairs):
    """Set (object, attribute, value) triples, restore them on exit."""
    saved = [(o, a, getattr(o, a)) for o, a, _ in pairs]
    try:
        for o, a, v in pairs:
            setattr(o, a, v)
        yield
    finally:
        for o, a, v in reversed(saved):
            setattr(o, a, v)


@contextlib.contextmanager
def default_switches():
    """No SR_* variable in the environment while a scene runs (the switches read at call time)."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SR_")}
    try:
        yield
    finally:
        os.environ.update(saved)


BF16, F32 = torch.bfloat16, torch.float32
SPLIT, PAIR, ROWS, TAILS = "split_min_wg", "attn_pair", "rows_max_lq", "group_tails"


def _scene(dtype=BF16, B=1, Na=16, Nq=16, fix_rank=9, outputs="all", shard=None, overlap=True, fp8=False,
           cache_queries=None, interleaved=False, **switches):
    return dict(dtype=dtype, B=B, Na=Na, Nq=Nq, fix_rank=fix_rank, outputs=outputs, shard=shard, overlap=overlap,
                fp8=fp8, cache_queries=cache_queries, interleaved=interleaved, switches=switches)


# name -> scene; the switches not named keep their defaults (split_min_wg 2048, attn_pair on,
# rows_max_lq 64, group_tails 2)
SCENES = {
    "s01_paired": _scene(split_min_wg=1),
    "s02_paired_whole_tiles": _scene(split_min_wg=1, fix_rank=16),
    "s03_split_unpaired": _scene(split_min_wg=1, attn_pair=False),
    "s04_one_launch_reloc": _scene(),
    "s05_batch2": _scene(B=2),
    "s06_fp32": _scene(dtype=F32),
    "s07_camera_bf16": _scene(outputs="camera", split_min_wg=1),
    "s07_camera_fp32": _scene(outputs="camera", dtype=F32),
    "s08_camera_chunked": _scene(outputs="camera", split_min_wg=1, rows_max_lq=8),
    "s09_shard2_overlap": _scene(shard=(2, 1), overlap=True),
    "s09_shard2_gathered": _scene(shard=(2, 1), overlap=False),
    "s10_shard3_no_query": _scene(shard=(3, 2), Nq=2),
    "s11_shard2_fp32": _scene(shard=(2, 1), dtype=F32),
    "s12_paired_ungrouped_tails": _scene(split_min_wg=1, group_tails=0),
    "s12_shard2_ungrouped_tails": _scene(shard=(2, 1), group_tails=0),
    "s13_fp8_global": _scene(fp8=True),
    "s14_no_queries": _scene(Nq=0),
    "s15_kv_cache_bf16": _scene(Nq=0, cache_queries=4),
    "s15_kv_cache_fp32": _scene(Nq=0, cache_queries=4, dtype=F32),
    "s16_interleaved": _scene(split_min_wg=1, interleaved=True),
}


def run_scene(name: str) -> list:
    """The normalised launch trace of scene ``name``; everything it patches is restored."""
    s = SCENES[name]
    sw = dict({SPLIT: 2048, PAIR: True, ROWS: 64, TAILS: 2}, **s["switches"])
    torch.manual_seed(0)
    agg = A.Aggregator(kv_cache=s["cache_queries"] is not None, **MODEL).eval()
    agg.compute_dtype = s["dtype"]
    agg.generator.manual_seed(0)
    agg.shard_overlap = s["overlap"]
    if s["shard"] is not None:
        agg.set_frame_sharding(A.RankSim(*s["shard"]))
    if s["fp8"]:
        agg.set_fp8_global(True)
    B, Na, Nq = s["B"], s["Na"], s["Nq"]
    images = torch.rand(B, Na + Nq, 3, 56, 56)
    if s["interleaved"]:
        no_reloc, reloc = list(range(0, Na + Nq, 2)), list(range(1, Na + Nq, 2))
    else:
        no_reloc, reloc = list(range(Na)), list(range(Na, Na + Nq))
    rec = Recorder(agg)
    to_device = runtime.to_device
    pairs = [(A, "ops", rec), (runtime, "ops", rec), (runtime, "require_device", lambda t, who: None),
             (runtime, "to_device", lambda t, dev: rec.host_table(to_device(t, dev))),
             (A, "_RELOC_SPLIT_MIN_WG", sw[SPLIT]), (real_ops, "_ATTN_PAIR", sw[PAIR]),
             (real_ops, "ROWS_MAX_LQ", sw[ROWS]), (runtime, "_GROUP_TAILS", sw[TAILS])]
    with default_switches(), patched(pairs), torch.no_grad():
        agg(images, no_reloc, reloc, fix_rank=s["fix_rank"], outputs=s["outputs"])
        if s["cache_queries"] is not None:
            agg.forward_with_cache(torch.rand(1, s["cache_queries"], 3, 56, 56), fix_rank=s["fix_rank"])
    return rec.calls


def dump_call(call) -> str:
    return json.dumps(call, separators=(",", ":"), sort_keys=True)


def names_of(calls) -> list:
    return [c[0] for c in calls]
