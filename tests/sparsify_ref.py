"""numpy restatement of sr_sparsify's contract (include/sfm_amd.h, DESIGN.md "Scoring confidence maps"), and
the seeded cases of tests/golden/g21_sparsify.npz.  A stable argsort of the 64-bit keys, math.fsum per bin,
cut by its bits.  Our own data: numpy only, nothing else is read."""

import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_sparsify.npz")

CONFIDENCE, UNCERTAINTY = "confidence", "uncertainty"
ORDERS = (CONFIDENCE, UNCERTAINTY)
QNAN = np.uint32(0x7fc00000)


def key32(x):
    """sr_select_ranks' key of fp32 values: bits ^ (sign ? 0xffffffff : 0x80000000), -0 before +0."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000)).astype(np.uint32)


def finite_bits(x):
    """Exponent bits not all ones."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (b & np.uint32(0x7f800000)) != np.uint32(0x7f800000)


def bounds(n, K):
    """b_k = floor(k n / K), k = 0 .. K, in Python integers."""
    return [k * int(n) // int(K) for k in range(int(K) + 1)]


def _fsum(v):
    return math.fsum(np.asarray(v, np.float64).tolist())


def sparsify(err, conf, n_steps, mask=None, group=None, n_groups=None, order=CONFIDENCE, row_len=None):
    """The whole call on [n_rows, row_stride] arrays, of which the first ``row_len`` columns count.  Returns
    bin_sum [G, 2, K] fp64, cut [G, K] uint32 (bits), count [G, 2] int64 (considered, skipped), fsum_abs
    [G, 2, K] (the sum of |v| per bin, for tolerances) and sorted_err: per group the two lists of fp32 errors
    in order C and in order O."""
    err, conf = np.asarray(err, np.float32), np.asarray(conf, np.float32)
    assert err.ndim == 2 and err.shape == conf.shape and order in ORDERS
    n_rows = err.shape[0]
    L = err.shape[1] if row_len is None else int(row_len)
    K = int(n_steps)
    if group is None:
        group, n_groups = np.arange(n_rows), n_rows
    group, G = np.asarray(group, np.int64), int(n_groups)
    e, c = err[:, :L], conf[:, :L]  # what lies beyond row_len is never looked at
    in_range = (group >= 0) & (group < G)
    ok = finite_bits(e) & finite_bits(c) & in_range[:, None]
    if mask is not None:
        ok &= np.asarray(mask)[:, :L] != 0
    g_of = np.broadcast_to(group[:, None], e.shape)
    kc = key32(c)
    if order == UNCERTAINTY:
        kc = ~kc
    ko = ~key32(e)
    sentinel = np.uint64(G) << np.uint64(32)
    gk = np.where(ok, g_of, 0).astype(np.uint64) << np.uint64(32)
    keys_c = np.where(ok, gk | kc.astype(np.uint64), sentinel).ravel()  # flat index i = r row_len + c
    keys_o = np.where(ok, gk | ko.astype(np.uint64), sentinel).ravel()
    ef, cf = np.ascontiguousarray(e).ravel(), np.ascontiguousarray(c).ravel()
    perm_c, perm_o = np.argsort(keys_c, kind="stable"), np.argsort(keys_o, kind="stable")
    bin_sum, fsum_abs = np.zeros((G, 2, K)), np.zeros((G, 2, K))
    cut = np.full((G, K), QNAN, np.uint32)
    count = np.zeros((G, 2), np.int64)
    sorted_err = []
    start = 0
    for g in range(G):
        n = int((ok & (g_of == g)).sum())
        count[g] = n, int((group == g).sum()) * L - n
        b = bounds(n, K)
        pc, po = perm_c[start:start + n], perm_o[start:start + n]
        assert (keys_c[pc] >> np.uint64(32) == np.uint64(g)).all()
        sc, so = ef[pc], ef[po]
        for k in range(K):
            for o, s in enumerate((sc, so)):
                v = s[b[k]:b[k + 1]].astype(np.float64)
                bin_sum[g, o, k] = _fsum(v) + 0.0  # an empty bin, and a sum of -0, give +0
                fsum_abs[g, o, k] = _fsum(np.abs(v))
            if n:
                cut[g, k] = cf[pc[b[k]]].view(np.uint32)
        sorted_err.append((sc, so))
        start += n
    return dict(bin_sum=bin_sum, cut=cut, count=count, fsum_abs=fsum_abs, sorted_err=sorted_err)


def curves(res, g, n_steps, root=False):
    """The curves of group g straight from the definition: curve[c][k] = the mean (fsum) of what is left
    of order c after b_k removals (its square root under ``root``); random, ause, ause_norm, aurg, fractions."""
    K = int(n_steps)
    n = int(res["count"][g, 0])
    nan = float("nan")
    if n == 0:
        return dict(curve=np.full((2, K), nan), fractions=np.full(K, nan), random=nan, ause=nan, ause_norm=nan, aurg=nan)
    b = bounds(n, K)
    curve = np.array([[_fsum(s[b[k]:]) / (n - b[k]) for k in range(K)] for s in res["sorted_err"][g]])
    if root:
        curve = np.sqrt(curve)
    random = curve[0, 0]
    ause = _fsum(curve[0] - curve[1]) / K
    return dict(curve=curve, fractions=np.array(b[:K]) / n, random=random, ause=ause,
                ause_norm=ause / random if random != 0 else nan, aurg=_fsum(random - curve[0]) / K)


# ---------------------------------------------------------------- the golden cases
HETERO = (3, 37 * 41)
CASES = ("hetero", "planted", "zeros", "two", "empty", "stride", "inter", "oor")


def _hetero(rng, shape):
    """err = |N(0, 1) sigma| with sigma log-normal: (err, sigma) as fp32.  math.exp, element by element: the
    same bits wherever numpy's vector exp may differ."""
    z = rng.standard_normal(shape)
    sigma = np.array([math.exp(0.75 * v) for v in rng.standard_normal(shape).ravel()]).reshape(shape)
    return np.abs(z * sigma).astype(np.float32), sigma.astype(np.float32)


def gen_case(name):
    """Inputs of a case: err [rows, stride], one or more confidences conf/<tag>, optional mask, group,
    n_groups, row_len, and cfg: the (conf tag, K, order) of every stored answer."""
    rng = np.random.default_rng(2100 + CASES.index(name))
    c = {}
    if name == "hetero":
        err, sigma = _hetero(rng, HETERO)
        c["err"] = err
        c["conf/inv_sigma"] = (np.float32(1) / sigma).astype(np.float32)
        c["conf/random"] = rng.random(HETERO).astype(np.float32)
        c["conf/constant"] = np.full(HETERO, 0.5, np.float32)
        c["conf/anti"] = err.copy()
        c["cfg"] = [(t, K, CONFIDENCE) for t in ("inv_sigma", "random", "constant", "anti") for K in (1, 100)] + \
                   [("inv_sigma", 100, UNCERTAINTY)]
    elif name == "planted":
        shape = (4, 300)
        err, sigma = _hetero(rng, shape)
        conf = (np.float32(1) / sigma).astype(np.float32)
        mask = (rng.random(shape) > 0.2).astype(np.uint8)
        flat = rng.permutation(err.size)
        bad = [np.nan, np.inf, -np.inf]
        for j in range(30):
            err.flat[flat[j]] = bad[j % 3]
        for j in range(30, 60):
            conf.flat[flat[j]] = bad[j % 3]
        for j in range(60, 75):
            err.flat[flat[j]], conf.flat[flat[j]] = bad[j % 3], bad[(j + 1) % 3]
        for j in range(20, 40):
            mask.flat[flat[j]] = 0  # masked and non-finite at once
        c.update(err=err, mask=mask)
        c["conf/c"] = conf
        c["cfg"] = [("c", 7, CONFIDENCE), ("c", 7, UNCERTAINTY), ("c", 1024, CONFIDENCE)]
    elif name == "zeros":
        shape = (1, 257)
        err, _ = _hetero(rng, shape)
        c["err"] = err
        c["conf/c"] = rng.choice(np.float32([-0.0, 0.0, -1.0, 1.0, -0.0, 0.0]), shape).astype(np.float32)
        c["cfg"] = [("c", 4, CONFIDENCE), ("c", 4, UNCERTAINTY), ("c", 3, CONFIDENCE)]
    elif name == "two":
        shape = (2, 2049)
        err, _ = _hetero(rng, shape)
        c["err"] = err
        c["conf/c"] = np.where(rng.random(shape) < 0.3, np.float32(0.25), np.float32(0.75)).astype(np.float32)
        c["group"], c["n_groups"] = np.zeros(2, np.int32), np.int32(1)
        c["cfg"] = [("c", 3, CONFIDENCE), ("c", 100, UNCERTAINTY)]
    elif name == "empty":
        shape = (3, 200)
        err, sigma = _hetero(rng, shape)
        mask = np.ones(shape, np.uint8)
        mask[1] = 0
        c.update(err=err, mask=mask)
        c["conf/c"] = sigma
        c["cfg"] = [("c", 5, CONFIDENCE), ("c", 5, UNCERTAINTY)]
    elif name == "stride":
        rows, L, stride = 3, 157, 160
        err = np.full((rows, stride), np.nan, np.float32)
        conf = np.full((rows, stride), np.nan, np.float32)
        e, sigma = _hetero(rng, (rows, L))
        err[:, :L], conf[:, :L] = e, (np.float32(1) / sigma).astype(np.float32)
        c.update(err=err, row_len=np.int32(L), mask=(rng.random((rows, stride)) > 0.1).astype(np.uint8))
        c["conf/c"] = conf
        c["cfg"] = [("c", 7, CONFIDENCE), ("c", 100, CONFIDENCE)]
    elif name in ("inter", "oor"):
        shape = (5, 130)
        err, sigma = _hetero(rng, shape)
        c["err"] = err
        c["conf/c"] = (np.float32(1) / sigma + rng.random(shape).astype(np.float32)).astype(np.float32)
        if name == "inter":
            c["group"], c["n_groups"] = np.int32([0, 1, 0, 2, 1]), np.int32(3)
        else:
            c["group"], c["n_groups"] = np.int32([0, 3, 1, -1, 1]), np.int32(2)
        c["cfg"] = [("c", 7, CONFIDENCE), ("c", 2, UNCERTAINTY)]
    return c


def run_cfg(c, cfg):
    tag, K, order = cfg
    return sparsify(c["err"], c["conf/" + tag], K, mask=c.get("mask"), group=c.get("group"),
                    n_groups=None if "n_groups" not in c else int(c["n_groups"]), order=order,
                    row_len=None if "row_len" not in c else int(c["row_len"]))


def cfg_tag(cfg):
    return "%s/K%d/%s" % cfg


STORED = ("bin_sum", "cut", "count")


def build_golden():
    """Inputs of every case and the restatement's answers of every configuration."""
    z = {}
    for name in CASES:
        c = gen_case(name)
        for k, v in c.items():
            if k != "cfg":
                z[f"{name}/{k}"] = np.asarray(v)
        for cfg in c["cfg"]:
            r = run_cfg(c, cfg)
            for k in STORED:
                z[f"{name}/answers/{cfg_tag(cfg)}/{k}"] = r[k]
    return z


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case(name):
    """Inputs of a golden case as stored, its configurations under "cfg", its stored answers under "answers"
    (keyed by cfg_tag, then by output)."""
    pre = name + "/"
    c = {"cfg": gen_case(name)["cfg"], "answers": {}}
    for k, v in _npz().items():
        if k.startswith(pre):
            rest = k[len(pre):]
            if rest.startswith("answers/"):
                tag, out = rest[len("answers/"):].rsplit("/", 1)
                c["answers"].setdefault(tag, {})[out] = v
            else:
                c[rest] = v
    return c
