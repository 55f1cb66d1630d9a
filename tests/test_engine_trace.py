"""The training engine's launch sequence, traced on the CPU (no GPU, no library).

train.engine reaches the GPU only through the ``ops`` module and the attention callbacks, so a
recorder in place of ``engine.ops`` sees every launch: its name, its operands (tensors by a name
looked up from pointer / shape / stride / dtype), its keywords and its timer tag.  Single blocks
and the layer's grouped reloc / global blocks run ONE stage sequence; these tests pin what that
sequence must keep: per item the grouped run does the single run's work in the single run's
order, it groups where it should (one sr_gemm_group launch per GEMM stage, one
sr_gemm_wgrad_pair per weight) and never where it must not (one problem alone, mixed widths /
dtypes / qkv epilogues), the timer tags, the fp32 path, and the caller's dicts left alone."""

import types

import pytest
import torch

from sailrecon_amd import _lib
from sailrecon_amd.train import engine

BF16, F32 = torch.bfloat16, torch.float32
C, HID = 256, 1024
GROUPED = ("gemm_group", "gemm_wgrad_pair")
FWD_KEYS = ("pb", "x", "r0", "r1", "tape", "attend", "qkv_epi")
BWD_KEYS = ("pb", "bp", "g", "tape", "dx", "dxb", "attend_bwd", "qkv_epi", "sc", "tag")


def _key(t):
    return t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype


class Recorder:
    """Stands in for the ops module: records (name, args, keywords) of every call."""

    def __init__(self, names, splits=(2, 2), eligible=True):
        self.calls, self.names, self.splits, self.eligible = [], names, splits, eligible

    def name(self, v):
        if isinstance(v, torch.Tensor):
            return self.names.get(_key(v), ("tensor",) + _key(v)[1:])
        if isinstance(v, dict):
            return {k: self.name(x) for k, x in sorted(v.items()) if x is not None}
        if isinstance(v, (list, tuple)):
            return [self.name(x) for x in v]
        return v

    # answered here: the real ones load the library
    def colsum_blocks(self, M):
        return (M + 63) // 64

    def gemm_group_eligible(self, problems):  # ops.gemm_group_eligible's rule
        return (self.eligible and 1 <= len(problems) <= 4 and
                all(p["a"].dtype == BF16 and p["w"].shape[0] % 256 == 0 for p in problems))

    def wgrad_pair_splits(self, M0, M1, N, K):
        return self.splits

    def __getattr__(self, fn):
        def record(*args, **kw):
            self.calls.append((fn, self.name(args), self.name(kw)))
        return record


def make_item(eng, names, i, dt=BF16, dim=C, hidden=HID, rows=128, scale_bias=True, epi=False):
    """One block application's forward + backward arguments as CPU tensors, every tensor named
    ``i<i>.<what>``."""
    pre = f"i{i}."

    def reg(n, t):
        names[_key(t)] = pre + n
        return t
    w = lambda n, r, c, d=dt: reg(n, torch.zeros(r, c, dtype=d))  # noqa: E731
    v = lambda n, c: reg(n, torch.zeros(c))  # noqa: E731
    opt = lambda n, c: v(n, c) if scale_bias else None  # noqa: E731
    pb = types.SimpleNamespace(
        dim=dim, eps=1e-5, ln1_w=v("ln1_w", dim), ln1_b=v("ln1_b", dim), ln2_w=v("ln2_w", dim), ln2_b=v("ln2_b", dim),
        w_qkv=w("w_qkv", 3 * dim, dim), b_qkv=opt("b_qkv", 3 * dim), w_proj=w("w_proj", dim, dim),
        b_proj=opt("b_proj", dim), g1=opt("g1", dim), w_fc1=w("w_fc1", hidden, dim), b_fc1=opt("b_fc1", hidden),
        w_fc2=w("w_fc2", dim, hidden), b_fc2=opt("b_fc2", dim), g2=opt("g2", dim))
    bp = eng.BwdPack(wt_qkv=w("wt_qkv", dim, 3 * dim), wt_proj=w("wt_proj", dim, dim), wt_fc1=w("wt_fc1", dim, hidden),
                     wt_fc2=w("wt_fc2", hidden, dim), w_proj=w("m_proj", dim, dim, F32),
                     w_fc2=w("m_fc2", dim, hidden, F32), b_proj=pb.b_proj, b_fc2=pb.b_fc2)
    gw = lambda n, r, c: w("d." + n, r, c, F32)  # noqa: E731
    gv = lambda n, c: reg("d." + n, torch.zeros(c))  # noqa: E731
    go = lambda n, c: gv(n, c) if scale_bias else None  # noqa: E731
    g = eng.BlockGrads(ln1_w=gv("ln1_w", dim), ln1_b=gv("ln1_b", dim), w_qkv=gw("w_qkv", 3 * dim, dim),
                       b_qkv=go("b_qkv", 3 * dim), qkn=gw("qkn", 4, 64) if epi else None, w_proj=gw("w_proj", dim, dim),
                       b_proj=go("b_proj", dim), g1=go("g1", dim), ln2_w=gv("ln2_w", dim), ln2_b=gv("ln2_b", dim),
                       w_fc1=gw("w_fc1", hidden, dim), b_fc1=go("b_fc1", hidden), w_fc2=gw("w_fc2", dim, hidden),
                       b_fc2=go("b_fc2", dim), g2=go("g2", dim))
    tape = eng.alloc_tape(rows, dim, hidden, dt, "cpu", 16, separate_raw=epi)
    for n in ("x0", "x1", "xn1", "raw", "qkv", "o", "lse", "xn2", "u", "h"):
        reg("tape." + n, getattr(tape, n))
    sc = eng.BwdScratch()  # the backward's scratch requests, made once here so that they carry names
    for n, r, c, d in (("colsum_tmp", 1, max(dim, hidden, 3 * dim), F32), ("dU", rows, hidden, dt),
                       ("dU_colsum", (rows + 63) // 64, hidden, F32), ("dxn", rows, dim, F32), ("dO", rows, dim, dt),
                       ("dqkv", rows, 3 * dim, F32), ("draw", rows, 3 * dim, dt)):
        t = reg("sc." + n, sc.get(n, r, c, d, "cpu"))
        if n == "colsum_tmp":
            reg("sc.colsum_tmp[:C]", t[0][:dim])
    x = reg("x", torch.zeros(rows + 7, dim))
    reg("xs", x[3:3 + rows])
    return dict(pb=pb, bp=bp, g=g, tape=tape, x=x, r0=3, r1=3 + rows, dx=reg("dx", torch.zeros(rows, dim)),
                dxb=reg("dxb", torch.zeros(rows, dim, dtype=BF16)) if dt == BF16 else None, sc=sc, tag=f"tag{i}",
                qkv_epi=dict(embed_dim=dim, head_dim=64, pos_row_base=100 * i) if epi else None)


def trace(eng, specs, via="multi", splits=(2, 2), eligible=True, tag="pair", first=0):
    """(forward calls, backward calls, the items) of ``eng`` over items made from ``specs``
    (make_item keywords; numbered from ``first``), through the list entry points or (``single``)
    one block at a time."""
    names = {}
    items = [make_item(eng, names, first + i, **s) for i, s in enumerate(specs)]
    rec = Recorder(names, splits, eligible)
    saved, eng.ops = eng.ops, rec
    for i, it in enumerate(items, first):
        it["attend"] = lambda q, o, l, i=i: rec.calls.append(("attend", [f"i{i}."] + rec.name([q, o, l]), {}))
        it["attend_bwd"] = lambda t, dO, dq, i=i: rec.calls.append(("attend_bwd", [f"i{i}."] + rec.name([dO, dq]), {}))
    try:
        if via == "multi":
            eng.run_block_train_multi([{k: it[k] for k in FWD_KEYS} for it in items])
        else:
            for it in items:
                eng.run_block_train(*[it[k] for k in FWD_KEYS])
        fwd, rec.calls = rec.calls, []
        if via == "multi":
            eng.block_bwd_multi([{k: it[k] for k in BWD_KEYS} for it in items], tag=tag)
        else:
            for it in items:
                eng.block_bwd(*[it[k] for k in BWD_KEYS[:-1]], tag=it["tag"])
    finally:
        eng.ops = saved
    return fwd, rec.calls, items


def expand(calls):
    """Every gemm_group as its problems' gemm calls, every gemm_wgrad_pair as gemm_wgrad calls."""
    out = []
    for fn, args, kw in calls:
        if fn == "gemm_group":
            out += [("gemm", [p["a"], p["w"], p["out"], args[1]],
                     dict({k: v for k, v in p.items() if k not in ("a", "w", "out")}, **kw)) for p in args[0]]
        elif fn == "gemm_wgrad_pair":
            out += [("gemm_wgrad", [p["dy"], p["x"], p["dw"]],
                     dict({k: v for k, v in p.items() if k not in ("dy", "x", "dw")}, **kw)) for p in args[0]]
        else:
            out.append((fn, args, kw))
    return out


def untagged(calls):
    return [(fn, args, {k: v for k, v in kw.items() if k != "tag"}) for fn, args, kw in calls]


def touched(call):
    """The items (indices) whose tensors a call names."""
    found = set()

    def walk(v):
        if isinstance(v, str) and v[:1] == "i" and "." in v and v[1:v.index(".")].isdigit():
            found.add(int(v[1:v.index(".")]))
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
    walk(call[1])
    walk({k: v for k, v in call[2].items() if k != "tag"})
    return found


def tags(calls, fn):
    return [kw.get("tag") for f, _, kw in calls if f == fn]


def count(calls, fn):
    return sum(f == fn for f, _, _ in calls)


@pytest.fixture(params=[(True, True, True), (False, False, False)], ids=["switches_on", "switches_off"])
def switches(request, monkeypatch):
    gelu, qk, pair = request.param
    monkeypatch.setattr(engine, "GELU_COLSUM", gelu)
    monkeypatch.setattr(engine, "QK_COLSUM", qk)
    monkeypatch.setattr(engine, "_PAIR_WGRAD", pair)
    return request.param


BF = dict(rows=128)
BF2 = dict(rows=200)
GROUPED_LISTS = {
    "pair": [BF, BF2],
    "pair_epi": [dict(BF, epi=True), dict(BF2, epi=True)],
    "pair_plain": [dict(BF, scale_bias=False), dict(BF2, scale_bias=False)],
    "pair_one_plain": [dict(BF, scale_bias=False), BF2],
    "triple": [BF, BF2, dict(rows=72)],
    "triple_epi": [dict(BF, epi=True), dict(BF2, epi=True), dict(rows=72, epi=True)],
}


@pytest.mark.parametrize("splits", [(2, 2), None], ids=["splits", "nosplits"])
@pytest.mark.parametrize("case", sorted(GROUPED_LISTS))
def test_same_work_per_item(case, splits, switches):
    specs = GROUPED_LISTS[case]
    fwd, bwd, _ = trace(engine, specs, splits=splits)
    assert count(fwd + bwd, "gemm_group") > 0
    for i, spec in enumerate(specs):
        one_f, one_b, _ = trace(engine, [spec], via="single", first=i)
        for grouped, alone in ((fwd, one_f), (bwd, one_b)):
            assert [c for c in untagged(expand(grouped)) if i in touched(c)] == untagged(alone), (case, i)
    assert all(len(touched(c)) == 1 for c in expand(fwd + bwd))


def test_pair_groups(switches):
    pair_on = switches[2]
    fwd, bwd, _ = trace(engine, [BF, BF2])
    assert count(fwd, "gemm_group") == 3 and count(fwd, "gemm") == 2           # qkv, proj, fc2; fc1 apart
    assert [a[3] for f, a, _ in fwd if f == "gemm"] == [_lib.SR_EPI_BIAS_GELU] * 2
    assert [a[1] for f, a, _ in fwd if f == "gemm_group"] == [_lib.SR_EPI_BIAS, _lib.SR_EPI_BIAS_RESID,
                                                               _lib.SR_EPI_BIAS_RESID]
    assert count(bwd, "gemm_group") == 4 and count(bwd, "gemm") == 0
    assert count(bwd, "gemm_wgrad_pair") == (4 if pair_on else 0)
    assert count(bwd, "gemm_wgrad") == (0 if pair_on else 8)
    assert [[p["dw"] for p in a[0]] for f, a, _ in bwd if f == "gemm_wgrad_pair"] == \
        ([[f"i0.d.{w}", f"i1.d.{w}"] for w in ("w_fc2", "w_fc1", "w_proj", "w_qkv")] if pair_on else [])
    for kw in (dict(splits=None), dict(specs=[BF, BF2, BF])):
        _, bwd, _ = trace(engine, kw.get("specs", [BF, BF2]), splits=kw.get("splits", (2, 2)))
        assert count(bwd, "gemm_wgrad_pair") == 0 and count(bwd, "gemm_group") == 4
        assert count(bwd, "gemm_wgrad") == 4 * len(kw.get("specs", [BF, BF2]))


def _one_after_another(calls, n):
    order = [touched(c) for c in calls]
    assert all(len(t) == 1 for t in order)
    order = [min(t) for t in order]
    assert order == sorted(order) and set(order) == set(range(n))


@pytest.mark.parametrize("case,specs,which", [
    ("single", [BF], "both"),                       # every N % 256 == 0: eligible, and still sr_gemm's own choice
    ("widths", [BF, dict(rows=200, dim=512, hidden=2048)], "both"),
    ("hidden", [BF, dict(rows=200, hidden=512)], "both"),
    ("dtypes", [BF, dict(rows=17, dt=F32)], "both"),
    ("dtypes_f32_first", [dict(rows=17, dt=F32), BF], "both"),
    ("qkv_epi", [dict(BF, epi=True), BF2], "fwd"),
])
def test_no_grouping(case, specs, which, switches):
    fwd, bwd, _ = trace(engine, specs)
    for calls in (fwd, bwd) if which == "both" else (fwd,):
        assert not any(count(calls, g) for g in GROUPED)
        _one_after_another(calls, len(specs))
    # ... and is what the single entry points do, tags included
    one_f, one_b, _ = trace(engine, specs, via="single")
    assert fwd == one_f
    if which == "both":
        assert bwd == one_b


def test_not_eligible_stays_interleaved(switches):
    fwd, bwd, _ = trace(engine, [BF, BF2], eligible=False, splits=None)
    assert not any(count(fwd + bwd, g) for g in GROUPED)
    gf, gb, _ = trace(engine, [BF, BF2], splits=None)
    assert fwd == expand(gf) and bwd == expand(gb)    # stage by stage, each problem with the group's tag
    assert tags(bwd, "gemm") == ["pair.dgrad"] * 8
    order = [min(touched(c)) for c in bwd]
    assert order != sorted(order)


def test_tags(switches):
    pair_on = switches[2]
    # single entry points: the item's tag on both
    fwd, bwd, _ = trace(engine, [BF], via="single")
    assert set(tags(fwd, "gemm")) == {"gemm"} and count(fwd, "gemm") == 4
    assert tags(bwd, "gemm") == ["tag0.dgrad"] * 4 and tags(bwd, "gemm_wgrad") == ["tag0.wgrad"] * 4
    # a list of one: the item's own tag, not the list's
    _, bwd, _ = trace(engine, [BF])
    assert tags(bwd, "gemm") == ["tag0.dgrad"] * 4 and tags(bwd, "gemm_wgrad") == ["tag0.wgrad"] * 4
    # grouped: the list's tag on what the items share, the item's on unpaired weight grads
    fwd, bwd, _ = trace(engine, [BF, BF2])
    assert set(tags(fwd, "gemm") + tags(fwd, "gemm_group")) == {"gemm"}
    assert tags(bwd, "gemm_group") == ["pair.dgrad"] * 4
    assert tags(bwd, "gemm_wgrad_pair") == (["pair.wgrad"] * 4 if pair_on else [])
    assert tags(bwd, "gemm_wgrad") == ([] if pair_on else ["tag0.wgrad", "tag1.wgrad"] * 4)
    _, bwd, _ = trace(engine, [BF, BF2], splits=None, tag="other")
    assert tags(bwd, "gemm_group") == ["other.dgrad"] * 4
    assert tags(bwd, "gemm_wgrad") == ["tag0.wgrad", "tag1.wgrad"] * 4
    # one after another (widths differ): each item's own tag
    _, bwd, _ = trace(engine, [BF, dict(rows=200, dim=512, hidden=2048)])
    assert tags(bwd, "gemm") == ["tag0.dgrad"] * 4 + ["tag1.dgrad"] * 4
    assert tags(bwd, "gemm_wgrad") == ["tag0.wgrad"] * 4 + ["tag1.wgrad"] * 4


@pytest.mark.parametrize("epi", [False, True])
def test_fp32_item(epi, switches):
    fwd, bwd, _ = trace(engine, [dict(rows=17, dt=F32, epi=epi)])
    assert count(fwd, "gemm") == 4 and count(fwd + bwd, "gemm_group") == 0
    assert count(bwd, "gemm_wgrad") == 0 and count(bwd, "colsum") == 0
    small = [(a, kw) for f, a, kw in bwd if f == "wgrad_small"]
    assert [a[2] for a, _ in small] == ["i0.d.w_fc2", "i0.d.w_fc1", "i0.d.w_proj", "i0.d.w_qkv"]
    assert [kw.get("db") for _, kw in small] == [None, "i0.d.b_fc1", None, "i0.d.b_qkv"]   # db folded in
    dgrads = [(a, kw) for f, a, kw in bwd if f == "gemm"]
    assert dgrads[0][0][:2] == ["i0.dx", "i0.wt_fc2"] and dgrads[2][0][:2] == ["i0.dx", "i0.wt_proj"]  # dx, not dxb
    assert dgrads[0][0][3] == _lib.SR_EPI_GELU_BWD and "colsum" not in dgrads[0][1]
    assert not any("i0.sc.dU_colsum" in str(c) or "i0.dxb" in str(c) for c in bwd)
    qk = [(a, kw) for f, a, kw in bwd if f == "qk_bwd"]
    if epi:  # in place on dqkv, which is then the qkv dgrad's operand
        assert len(qk) == 1 and qk[0][0][:3] == ["i0.tape.raw", "i0.sc.dqkv", "i0.sc.dqkv"]
        assert "bias_grad" not in qk[0][1]
    else:
        assert qk == []
    assert dgrads[3][0][:2] == ["i0.sc.dqkv", "i0.wt_qkv"]


def test_bf16_bias_grads(switches):
    gelu, qk, _ = switches
    _, bwd, _ = trace(engine, [BF], via="single")
    dU = next(kw for f, a, kw in bwd if f == "gemm" and a[3] == _lib.SR_EPI_GELU_BWD)
    assert dU.get("colsum") == ("i0.sc.dU_colsum" if gelu else None)
    sums = [a for f, a, _ in bwd if f == "colsum"]
    assert ["i0.sc.dU_colsum" if gelu else "i0.sc.dU", "i0.d.b_fc1"] in sums
    assert (["i0.sc.draw", "i0.d.b_qkv"] in sums) == (not qk)
    assert next(kw for f, _, kw in bwd if f == "qk_bwd").get("bias_grad") == ("i0.d.b_qkv" if qk else None)
    _, bwd, _ = trace(engine, [dict(BF, scale_bias=False)], via="single")   # no fc1 bias: no column sums at all
    assert count(bwd, "colsum") == 0 and not any("colsum" in kw for _, _, kw in bwd)


def test_callers_dicts_untouched(switches):
    names = {}
    for specs in ([BF], [BF, BF2], [BF, dict(rows=17, dt=F32)]):
        items = [make_item(engine, names, i, **s) for i, s in enumerate(specs)]
        for it in items:
            it["attend"] = it["attend_bwd"] = lambda *a: None
        f_items = [{k: it[k] for k in FWD_KEYS} for it in items]
        b_items = [{k: it[k] for k in BWD_KEYS} for it in items]
        before = [dict(d) for d in f_items + b_items]
        saved, engine.ops = engine.ops, Recorder(names)
        try:
            engine.run_block_train_multi(f_items)
            engine.block_bwd_multi(b_items, tag="pair")
        finally:
            engine.ops = saved
        assert all(set(d) == set(b) and all(d[k] is b[k] for k in b) for d, b in zip(f_items + b_items, before))

