"""fp64 references of the GEMM family (csrc/sr_gemm.hip: gemm_kernel 128x128 and 64x256, split-K and
its reduction, the 256x256 tile body of gemm256_kernel / gemm256_group_kernel) with per-element
bounds, the seeded cases the CPU and GPU files share, and the mutants that show the bounds bite.
No GPU here: tests/test_gemm_ref.py checks the references against torch's own fp64 ops and shows that
a correct fp32-accumulate / round-once implementation (torch's CPU ops) meets every bound;
tests/test_gemm_oracle_gpu.py holds the kernels to them.

``evaluate(case, inputs)`` returns ``{name: (ref, delta)}`` for every tensor the call writes.
u = 2^-24, gamma(k) = k u / (1 - k u).  S = A W^T + bias is formed in fp64 from the stored inputs
(bf16 widened exactly), mag(S) = |A| |W|^T + |bias|.  ``delta`` bounds the fp32 value before the
store.  fp32 outputs: |got - ref| <= delta.  bf16 outputs (and bf16 aux): got must lie in
[bf16(ref - delta), bf16(ref + delta)], ends rounded from fp64 to nearest even -- one value, or two
where a rounding boundary falls inside ref +- delta; a result rounded twice, or rounded and then
scaled, leaves that interval.

Bounds (fp32 roundings counted from produce() / epilogue() / splitk_reduce_kernel; the K products
and their additions in any order -- MFMA blocks, k-tiles, split-K slices summed by the reduction --
are gamma(K)):
    BIAS      gamma(K + 2) |qs| mag(S)          the bias add, the q_scale multiply (qs = 1 elsewhere)
    F32       gamma(K + 1) mag(S)               the bias add (the library refuses q_scale with F32)
    GELU      aux: gamma(K + 1) mag(S) = dS;  out: 1.13 dS + eps.  max |gelu'| = 1.1290.
              fp32 (erff): eps = 6 u |S|: v / sqrt2 rounds (moves erf by <= 0.5 u), erff within 4 ulp
              (|erf| <= 1), 1 + erf rounds (<= 2 u): 1 + erf is within 8 u absolute, times |v| / 2,
              and the last multiply rounds (u |gelu| <= u |v|): 5 u |v|, taken as 6.
              bf16 (gelu_erf_fast = fma(-|x|, h, max(x, 0)), h = phi_tail_fast): eps = |x| EPS_H +
              u |gelu|, EPS_H = 0.75e-7 + 40 u: A&S 7.1.26's |erf error| <= 1.5e-7 halved, and the
              roundings of h = poly t e: t = rcp(fma(p, |x|, 1)) within 3 u relative (fma u, rcp
              1 ulp = 2 u); Horner's four fmas within gamma(8) sum |a_i| / 2 = 8 u 2.24, plus
              t's error through |poly'| t <= sum i |a_i| / 2 = 5.87: 36 u absolute; e = exp2(x x c):
              two multiplies and c's own rounding move the argument by 3 u |arg|, exp2 1 ulp:
              |arg| 2^-|arg| <= 0.53, so e is within 3.1 u absolute; poly t <= 1 / 2, two more
              multiplies (2 u h): 36 + 1.6 + 2.5 -> 40 u.
    RESID     gamma(K + 3) (|x0| + |gamma| mag(S))   bias add, gamma multiply, the add to x
    PATCH     gamma(K + 2) (mag(S) + |row_add|)      bias add, row_add; every other row unchanged
    GELU_BWD  gamma(K + 1) mag(acc) |g'(u)| + (|acc| + gamma(K) mag(acc)) EPS_G, u the stored aux:
              one multiply; g' = cdf + x phi: fast EPS_G = EPS_H + 5 u (1 - h rounds: u; x phi(x) <=
              0.242 with five roundings and e's 3 u |arg| ln2: <= 2 u; the last add: 1.13 u),
              fp32 EPS_G = 8 u (the cdf as above: 4 u).
    QKV       aux: dS.  Per 64-wide head of Q and K, s = S + e with |e_i| <= d_i = dS_i:
              y_i = w_i r (s_i - mu) + b_i, r = (var + eps)^-1/2, D_i = s_i - mu.
              dy_i / ds_j = w_i r (delta_ij - 1/64 - D_i D_j r^2 / 64), so to first order
                |dy_i| <= |w_i| r (d_i + mean(d) + |D_i| r^2 mean(|D| d)),
              times (1 + 4 r max(d)) for the second-order remainder (r max(d) is 1e-2 at worst here).
              With var = 0 (a constant head row) D = 0, r = eps^-1/2 and the expression stays finite
              and valid: the third term vanishes, the first two carry r.  fp32 roundings: the mean of
              64 values is within gamma(64) mean|s| -- a common shift of every D_i, passed on as
              |w_i| r gamma(64) mean|s|; D_i rounds (u), sum D^2 / 64 + eps (gamma(66), halved by
              the root), rsqrtf (1 ulp = 2 u), two multiplies (2 u): |w_i| r |D_i| 48 u; the add of
              b_i: 2 u (|w_i r D_i| + |b_i|) with the multiply before it.
              RoPE on pairs (d, d + 16) of each 32-wide half with the stored fp32 tables:
              o1 = x1 c - x2 s, o2 = x2 c + x1 s: |do1| <= |c| dx1 + |s| dx2 + 2 u (|x1 c| + |x2 s|).
              q_scale on columns < q_cols: times |qs|, + u |out|.  V: gamma(K + 1) mag(S).
    colsum    fp64 sums of the kernel's own stored rows 64 b .. 64 b + 63 (< M) per block b; bound
              gamma(64) sum |stored|; exactly colsum_blocks(M) rows are written.

Mutants (keyword ``mutant``), each a defect a Frobenius norm over the matrix cannot see:
    acc_bf16 (a), bias_shift / gamma_shift (b), row_m2 (c), drop_kt (d), qscale_post / qscale_wide (e),
    pos_prev (f), ln_on_aux (g), gelu_tanh (h), colsum_unrounded / colsum_shift (i), patch_special (j).
"""

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64 = torch.float64
BF16 = torch.bfloat16
F32 = torch.float32
GELU_SLOPE = 1.13
EPS_H = 0.75e-7 + 40 * U
EPS_G_FAST = EPS_H + 5 * U
EPS_G_F32 = 8 * U
FP32_OUT = ("resid", "f32", "patch")


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------- bf16 rounding of fp64 values
def bf16_rne(x):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64; bf16's normal range."""
    b = x.contiguous().view(torch.int64)
    drop = 52 - 7
    b = (b + ((1 << (drop - 1)) - 1) + ((b >> drop) & 1)) & ~((1 << drop) - 1)
    return b.view(F64)


def _bf16_neighbours(g):
    """The bf16 values next to |g| (below, above) as fp64, for bf16 ``g``."""
    bits = g.abs().view(torch.int16).to(torch.int32)
    up = (bits + 1).to(torch.int16).view(BF16).to(F64)
    dn = torch.where(bits > 0, (bits - 1).clamp_min(0).to(torch.int16).view(BF16).to(F64), -up)
    return dn, up


def check(got, ref, delta):
    """(every element inside its bound, worst ratio, share of elements whose interval holds more than
    one value).  fp32 ``got``: |got - ref| <= delta, ratio = |got - ref| / delta.  bf16 ``got``: the
    interval test of the module docstring; the ratio is the distance from ref to the set of reals that
    round to got, over delta (<= 1 inside, up to ties)."""
    if not bool(torch.isfinite(got).all()):
        return False, float("inf"), 0.0
    g = got.to(F64)
    if got.dtype == BF16:
        lo, hi = bf16_rne(ref - delta), bf16_rne(ref + delta)
        ok = bool(((g >= lo) & (g <= hi)).all())
        dn, up = _bf16_neighbours(got)
        a, r = g.abs(), torch.where(g < 0, -ref, ref)  # mirrored onto got's side
        need = torch.maximum((a + dn) / 2 - r, r - (a + up) / 2).clamp_min(0)
        share = float((lo != hi).double().mean())
    else:
        need = (g - ref).abs()
        ok = bool((need <= delta).all())
        share = 0.0
    ratio = torch.where(delta > 0, need / delta.clamp_min(1e-300), torch.where(need > 0, float("inf"), 0.0).to(F64))
    return ok, float(ratio.max()) if ratio.numel() else 0.0, share


def store(v, dtype):
    """An fp64 value rounded once to the output type."""
    return bf16_rne(v).to(F32).to(BF16) if dtype == BF16 else v.to(F32)


# ---------------------------------------------------------------- GELU
_AS_P = 0.3275911
_AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def phi_tail_as(x):
    """Phi(-|x|) by Abramowitz & Stegun 7.1.26, in the dtype of x: (1 - erf(|x| / sqrt2)) / 2."""
    z = x.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + _AS_P * z)
    poly = _AS_A[4]
    for a in _AS_A[3::-1]:
        poly = poly * t + a
    return 0.5 * poly * t * torch.exp(-z * z)


def gelu_as(x):
    """gelu_erf_fast's formula, max(x, 0) - |x| Phi_AS(-|x|), in exact arithmetic of x's dtype."""
    return x.clamp_min(0) - x.abs() * phi_tail_as(x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_grad(x):
    """d/dx gelu_erf(x) = Phi(x) + x phi(x)."""
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_grad_as(x):
    h = phi_tail_as(x)
    return torch.where(x >= 0, 1.0 - h, h) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------- QKV: LayerNorm, 2-D RoPE
def rope_pos(c, inp):
    """[M, 2] (y, x) of every GEMM row, as sr::rope_pos defines it: explicit pos_yx, else the token
    row (pos_rowmap[row] or pos_row_base + row) inside a frame of tokens_per_frame rows: (0, 0) for
    the special tokens before patch_start, then (p // grid_w + 1, p % grid_w + 1)."""
    if inp.get("pos_yx") is not None:
        return inp["pos_yx"].to(torch.int64)
    M = c["M"]
    tr = inp["pos_rowmap"].to(torch.int64) if inp.get("pos_rowmap") is not None else \
        torch.arange(M, dtype=torch.int64) + c["pos_row_base"]
    t = tr % c["tokens_per_frame"]
    p = (t - c["patch_start"]).clamp_min(0)
    patch = (t >= c["patch_start"]).to(torch.int64)
    return torch.stack([(p // c["grid_w"] + 1) * patch, (p % c["grid_w"] + 1) * patch], -1)


def rope_half(x, dx, p, cos, sin):
    """One 32-wide half: pairs (d, d + 16) rotated by the table row p; value and bound."""
    cc, ss = cos[p], sin[p]
    x1, x2, d1, d2 = x[:, :16], x[:, 16:], dx[:, :16], dx[:, 16:]
    o = torch.cat([x1 * cc - x2 * ss, x2 * cc + x1 * ss], -1)
    do = torch.cat([cc.abs() * d1 + ss.abs() * d2 + 2 * U * ((x1 * cc).abs() + (x2 * ss).abs()),
                    cc.abs() * d2 + ss.abs() * d1 + 2 * U * ((x2 * cc).abs() + (x1 * ss).abs())], -1)
    return o, do


def qkv_epilogue(S, dS, c, inp, mutant=None):
    M, N = S.shape
    E, off, eps = c["embed_dim"], c["col_offset"], c["qk_eps"]
    pos = rope_pos(c, inp).clone()
    if mutant == "pos_prev":
        pos[M - 1] = pos[M - 2]
    cos, sin = inp["rope_cos"].to(F64), inp["rope_sin"].to(F64)
    out, dout = S.clone(), dS.clone()
    for h in range(N // 64):
        region = (h * 64 + off) // E
        assert region < 3, "columns past q | k | v"
        if region == 2:
            continue
        sl = slice(h * 64, h * 64 + 64)
        s, d = S[:, sl], dS[:, sl]
        nw, nb = (inp["qn_w"], inp["qn_b"]) if region == 0 else (inp["kn_w"], inp["kn_b"])
        nw, nb = nw.to(F64), nb.to(F64)
        y = F.layer_norm(bf16_rne(s) if mutant == "ln_on_aux" else s, (64,), nw, nb, eps)
        mu = s.mean(-1, keepdim=True)
        D = s - mu
        r = ((D * D).mean(-1, keepdim=True) + eps) ** -0.5
        first = nw.abs() * r * (d + d.mean(-1, keepdim=True) + D.abs() * r * r * (D.abs() * d).mean(-1, keepdim=True))
        first = first * (1 + 4 * r * d.max(-1, keepdim=True).values)
        rnd = nw.abs() * r * (gamma(64) * s.abs().mean(-1, keepdim=True) + 48 * U * D.abs()) \
            + 2 * U * ((nw * r * D).abs() + nb.abs())
        dy = first + rnd
        oy, doy = rope_half(y[:, :32], dy[:, :32], pos[:, 0], cos, sin)
        ox, dox = rope_half(y[:, 32:], dy[:, 32:], pos[:, 1], cos, sin)
        out[:, sl], dout[:, sl] = torch.cat([oy, ox], -1), torch.cat([doy, dox], -1)
    qs, qc = c.get("q_scale", 0.0), c.get("q_cols", 0)
    if qs:
        if mutant == "qscale_wide":
            qc += 64
        out[:, :qc] *= qs
        dout[:, :qc] = dout[:, :qc] * abs(qs) + U * out[:, :qc].abs()
    return out, dout


# ---------------------------------------------------------------- the call
def out_dtype(c):
    return F32 if c["epi"] in FP32_OUT else c["dtype"]


def evaluate(c, inp, mutant=None):
    """{tensor name: (fp64 reference, delta)} of one case: "out", and "aux" where the call writes it.
    PATCH's "out" is the whole output buffer (rows the call leaves alone have delta 0).  With
    ``mutant`` the reference is that of the defective computation instead."""
    M, N, epi = c["M"], c["N"], c["epi"]
    A, W = inp["a"].to(F64), inp["w"].to(F64)
    K = A.shape[1]
    acc, macc = A @ W.T, A.abs() @ W.abs().T
    if mutant == "row_m2":
        acc[M - 1] = acc[M - 2]
    if mutant == "drop_kt":  # the rows of the last row tile miss the last k-tile
        r0, kw = (M - 1) // c["tile_m"] * c["tile_m"], K - c["kt"]
        acc[r0:] = A[r0:, :kw] @ W[:, :kw].T
    if mutant == "acc_bf16":
        acc = bf16_rne(acc)
    b = inp["bias"].to(F64) if inp.get("bias") is not None else torch.zeros(N, dtype=F64)
    if mutant == "bias_shift":
        b = b.clone()
        b[N - 4:] = b[N - 8:N - 4]
    S, magS = acc + b, macc + b.abs()
    dS = gamma(K + 1) * magS
    res = {}
    if epi == "bias":
        qs = torch.ones(N, dtype=F64)
        if c.get("q_scale"):
            qs[:c["q_cols"] + (64 if mutant == "qscale_wide" else 0)] = c["q_scale"]
        ref = bf16_rne(S) * qs if mutant == "qscale_post" else S * qs
        res["out"] = (ref, gamma(K + 2) * magS * qs.abs())
    elif epi == "f32":
        res["out"] = (S, dS)
    elif epi == "gelu":
        if c.get("aux"):
            res["aux"] = (S, dS)
        eps = 6 * U * (S.abs() + dS) if c["dtype"] == F32 else (S.abs() + dS) * EPS_H + U * gelu_erf(S).abs()
        res["out"] = (gelu_tanh(S) if mutant == "gelu_tanh" else gelu_erf(S), GELU_SLOPE * dS + eps)
    elif epi == "resid":
        g = inp["gamma"].to(F64)
        gm = g.clone()
        if mutant == "gamma_shift":
            gm[N - 4:] = gm[N - 8:N - 4]
        x0 = inp["x0"].to(F64)
        res["out"] = (x0 + gm * S, gamma(K + 3) * (x0.abs() + g.abs() * magS))
    elif epi == "patch":
        sr_, st, so = c["seg_rows"], c["seg_stride"], c["seg_offset"]
        ref = inp["x0"].to(F64).clone()
        delta = torch.zeros_like(ref)
        ra = inp["row_add"].to(F64)
        rows = torch.arange(M)
        f, p = rows // sr_, rows % sr_
        orow = f * st + so + p
        ref[orow] = S + ra[p]
        delta[orow] = gamma(K + 2) * (magS + ra[p].abs())
        if mutant == "patch_special":  # segment 0's first row also lands in its special-token rows
            ref[0:so] = ref[so]
        res["out"] = (ref, delta)
    elif epi == "gelu_bwd":
        u = inp["aux_in"].to(F64)
        gp = gelu_grad(u)
        eg = EPS_G_F32 if c["dtype"] == F32 else EPS_G_FAST
        res["out"] = (acc * gp, gamma(K + 1) * macc * gp.abs() + (acc.abs() + gamma(K) * macc) * eg)
    elif epi == "qkv":
        if c.get("aux"):
            res["aux"] = (S, dS)
        res["out"] = qkv_epilogue(S, dS, c, inp, mutant)
    else:
        raise KeyError(epi)
    return res


def colsum_blocks(M: int) -> int:
    return (M + 63) // 64


def colsum_ref(stored, mutant=None, unrounded=None):
    """Block b: the fp64 sum of the stored output rows 64 b .. 64 b + 63; bound gamma(64) sum |stored|.
    Mutants: "colsum_unrounded" sums ``unrounded`` (the values before the store) instead,
    "colsum_shift" puts block b's sums into row b + 1 (the last into row 0)."""
    M, N = stored.shape
    nb = colsum_blocks(M)
    src = (unrounded if mutant == "colsum_unrounded" else stored).to(F64)
    pad = torch.zeros(nb * 64 - M, N, dtype=F64)
    ref = torch.cat([src, pad]).view(nb, 64, N).sum(1)
    mag = torch.cat([stored.to(F64).abs(), pad]).view(nb, 64, N).sum(1)
    if mutant == "colsum_shift":
        ref = ref.roll(1, 0)
    return ref, gamma(64) * mag


# ---------------------------------------------------------------- the correct fp32 model (CPU ops)
def model(c, inp):
    """What a correct kernel computes, with torch's CPU ops: fp32 accumulation, every epilogue in
    fp32, one rounding to the output type; the fast GELU / its gradient as the A&S formula evaluated
    in fp64 on the fp32 argument.  {name: tensor in the stored dtype}, and "colsum"."""
    M, N, epi, dt = c["M"], c["N"], c["epi"], c["dtype"]
    acc = inp["a"].float() @ inp["w"].float().T
    S = acc + inp["bias"] if inp.get("bias") is not None else acc
    out = {}
    if epi == "bias":
        v = S.clone()
        if c.get("q_scale"):
            v[:, :c["q_cols"]] *= c["q_scale"]
        out["out"] = v.to(dt)
    elif epi == "f32":
        out["out"] = S
    elif epi == "gelu":
        if c.get("aux"):
            out["aux"] = S.to(dt)
        out["out"] = (F.gelu(S) if dt == F32 else gelu_as(S.double()).float()).to(dt)
    elif epi == "resid":
        out["out"] = inp["x0"] + S * inp["gamma"]
    elif epi == "patch":
        x = inp["x0"].clone()
        rows = torch.arange(M)
        f, p = rows // c["seg_rows"], rows % c["seg_rows"]
        x[f * c["seg_stride"] + c["seg_offset"] + p] = S + inp["row_add"][p]
        out["out"] = x
    elif epi == "gelu_bwd":
        u = inp["aux_in"].float()
        gp = (gelu_grad(u.double()) if dt == F32 else gelu_grad_as(u.double())).float()
        v = acc * gp
        out["out"] = v.to(dt)
        if c.get("colsum"):
            nb = colsum_blocks(M)
            st = torch.cat([out["out"].float(), torch.zeros(nb * 64 - M, N)])
            out["colsum"] = st.view(nb, 64, N).sum(1)
    elif epi == "qkv":
        if c.get("aux"):
            out["aux"] = S.to(dt)
        v = S.clone()
        pos = rope_pos(c, inp)
        cos, sin = inp["rope_cos"], inp["rope_sin"]
        zero = torch.zeros(M, 32)
        for h in range(N // 64):
            region = (h * 64 + c["col_offset"]) // c["embed_dim"]
            if region == 2:
                continue
            nw, nb = (inp["qn_w"], inp["qn_b"]) if region == 0 else (inp["kn_w"], inp["kn_b"])
            y = F.layer_norm(S[:, h * 64:h * 64 + 64], (64,), nw, nb, c["qk_eps"])
            v[:, h * 64:h * 64 + 64] = torch.cat([rope_half(y[:, :32], zero, pos[:, 0], cos, sin)[0],
                                                   rope_half(y[:, 32:], zero, pos[:, 1], cos, sin)[0]], -1)
        if c.get("q_scale"):
            v[:, :c["q_cols"]] *= c["q_scale"]
        out["out"] = v.to(dt)
    return out


# ---------------------------------------------------------------- cases
def C(kernel, epi, dtype, M, N, kt, **kw):
    """One case.  kernel: "k128" (gemm_kernel 128x128), "k64" (the 64x256 few-row instance), "splitk",
    "group" (gemm256_group_kernel, one problem), "k256" (gemm256_kernel through sr_gemm).  ``kt``: K in
    k-tiles (64 bf16 / 32 fp32 elements).  Keywords: aux, colsum, q_scale / q_cols, splits, pad (A, W,
    out, aux cut out of larger buffers), tune (library switches), the QKV fields, out_align (byte offset
    of out's first element modulo 16), name suffix ``tag``."""
    ktile = 64 if dtype == BF16 else 32
    c = dict(kernel=kernel, epi=epi, dtype=dtype, M=M, N=N, K=kt * ktile, kt=ktile,
             tile_m={"k128": 128, "k64": 64, "splitk": 128, "group": 256, "k256": 256}[kernel],
             aux=False, colsum=False, pad=True, tune={}, splits=1, out_align=0, ldo_extra=8)
    c.update(kw)
    if kernel == "splitk" and M <= 64 and N > 128:
        c["tile_m"] = 64
    if epi == "qkv":
        c.setdefault("qk_eps", 1e-5)
        c.setdefault("col_offset", 0)
        c.setdefault("pos", "yx")
        c.setdefault("rope_npos", 5)
        c.setdefault("tokens_per_frame", 21)
        c.setdefault("patch_start", 5)
        c.setdefault("grid_w", 4)
        c.setdefault("pos_row_base", 0)
    if epi == "patch":
        c.setdefault("seg_rows", 5 if M >= 5 else 1)
        c.setdefault("seg_offset", 3)
        c["seg_stride"] = c["seg_rows"] + c["seg_offset"]
    tune = ",".join(f"{k[3:]}={v}" for k, v in sorted(c["tune"].items()))
    # "data": what the inputs and the reference depend on (cases that differ only in library switches share
    # them, so their outputs can be compared bit for bit); "name" adds the switches
    c["data"] = "-".join(str(x) for x in (kernel, epi, "bf16" if dtype == BF16 else "f32", M, N, kt, c.get("tag", ""),
                                          "aux" if c["aux"] else "", "cs" if c["colsum"] else "") if x != "")
    c["name"] = c["data"] + ("-" + tune if tune else "")
    return c


_SEED = {}


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def inputs(c):
    """The seeded inputs of a case in their stored dtypes (CPU); computed once, never modified."""
    if c["data"] in _SEED:
        return _SEED[c["data"]]
    M, N, K, dt, epi = c["M"], c["N"], c["K"], c["dtype"], c["epi"]
    g = torch.Generator().manual_seed(_seed(c["data"]))
    inp = dict(a=torch.randn(M, K, generator=g).to(dt), w=(torch.randn(N, K, generator=g) / K ** 0.5).to(dt))
    if epi != "gelu_bwd" and not c.get("nobias"):
        inp["bias"] = torch.randn(N, generator=g)
    if epi == "resid":
        inp["gamma"], inp["x0"] = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    if epi == "gelu_bwd":
        inp["aux_in"] = (torch.randn(M, N, generator=g) * 2).to(dt)
    if epi == "patch":
        nseg = -(-M // c["seg_rows"])
        inp["row_add"] = torch.randn(c["seg_rows"], N, generator=g)
        inp["x0"] = torch.randn(nseg * c["seg_stride"], N, generator=g)
    if epi == "qkv":
        for k in ("qn_w", "qn_b", "kn_w", "kn_b"):
            inp[k] = torch.randn(64, generator=g)
        npos = c["rope_npos"]
        ang = torch.arange(npos, dtype=F32)[:, None] * (1.0 / 100.0 ** (torch.arange(0, 32, 2).float() / 32))[None]
        inp["rope_cos"], inp["rope_sin"] = ang.cos().contiguous(), ang.sin().contiguous()
        if c["pos"] == "yx":  # random positions; the last row reaches the table's last row
            p = torch.randint(0, npos, (M, 2), generator=g, dtype=torch.int32)
            p[M - 1] = npos - 1
            inp["pos_yx"] = p
        elif c["pos"] == "rowmap":
            inp["pos_rowmap"] = torch.randint(0, 4 * c["tokens_per_frame"], (M,), generator=g, dtype=torch.int32)
    _SEED[c["data"]] = inp
    return inp


_REF = {}


def reference(c):
    """evaluate(c, inputs(c)), computed once and shared (callers do not modify it)."""
    if c["data"] not in _REF:
        _REF[c["data"]] = evaluate(c, inputs(c))
    return _REF[c["data"]]


def _epis_for(kernel, dtype, M, N, kt, **kw):
    """Every epilogue a kernel serves at one shape (QKV where N is whole 64-wide heads inside q | k | v)."""
    cs = [C(kernel, "bias", dtype, M, N, kt, **kw), C(kernel, "gelu", dtype, M, N, kt, aux=True, **kw),
          C(kernel, "resid", dtype, M, N, kt, **kw), C(kernel, "f32", dtype, M, N, kt, **kw),
          C(kernel, "patch", dtype, M, N, kt, **kw), C(kernel, "gelu_bwd", dtype, M, N, kt, colsum=True, **kw)]
    if N % 64 == 0 and N <= 256:
        cs.append(C(kernel, "qkv", dtype, M, N, kt, embed_dim=64 if N <= 192 else 128, aux=True, **kw))
    return cs


def _both(fn):
    return [c for dt in (BF16, F32) for c in fn(dt)]


K128_SHAPES = [(1, 4, 1), (16, 64, 1), (127, 124, 2), (128, 128, 3), (129, 132, 2), (65, 128, 1), (257, 260, 5)]
CASES_K128 = _both(lambda dt: [c for s in K128_SHAPES for c in _epis_for("k128", dt, *s)]) + _both(lambda dt: [
    C("k128", "bias", dt, 128, 128, 1, q_scale=0.125, q_cols=64, tag="qcols64"),
    C("k128", "qkv", dt, 65, 128, 1, embed_dim=64, q_scale=0.125, q_cols=64, tag="qscale"),
    C("k128", "qkv", dt, 129, 128, 2, embed_dim=64, pos="grid", pos_row_base=7, tag="grid"),
    C("k128", "qkv", dt, 65, 128, 1, embed_dim=64, pos="rowmap", tag="rowmap"),
    C("k128", "qkv", dt, 16, 128, 1, embed_dim=64, col_offset=64, tag="kv"),
    C("k128", "gelu", dt, 127, 124, 2, tag="noaux"),
    C("k128", "bias", dt, 129, 132, 2, nobias=True, tag="nobias"),
])
K64_SHAPES = [(1, 132, 1), (64, 256, 2), (33, 260, 3), (64, 516, 1)]
CASES_K64 = _both(lambda dt: [c for s in K64_SHAPES for c in _epis_for("k64", dt, *s)])
CASES_K64_OFF = _both(lambda dt: [c for s in K64_SHAPES for c in _epis_for("k128", dt, *s, tune=dict(SR_GEMM_SMALLM=0))])
SPLITK_SHAPES = [(37, 256, 4, 2), (37, 256, 4, 4), (64, 260, 6, 3), (130, 132, 2, 2)]
CASES_SPLITK = _both(lambda dt: [C("splitk", e, dt, M, N, kt, splits=s, tag=f"s{s}")
                                 for M, N, kt, s in SPLITK_SHAPES for e in ("bias", "gelu", "resid", "f32")])

_QKV256 = dict(embed_dim=128)
_QKV512 = dict(embed_dim=192, q_scale=0.125, q_cols=192)
G_SHAPES = [(1, 256, 1), (255, 256, 2), (256, 256, 1), (257, 256, 3), (513, 256, 1), (256, 512, 2), (257, 512, 1),
            (513, 512, 3)]


def _group_epis(M, N, kt):
    q = _QKV256 if N == 256 else _QKV512
    return [C("group", "bias", BF16, M, N, kt), C("group", "gelu", BF16, M, N, kt, aux=True),
            C("group", "gelu", BF16, M, N, kt, tag="noaux"), C("group", "resid", BF16, M, N, kt),
            C("group", "qkv", BF16, M, N, kt, aux=True, **q), C("group", "qkv", BF16, M, N, kt, tag="noaux", **q),
            C("group", "f32", BF16, M, N, kt), C("group", "gelu_bwd", BF16, M, N, kt, colsum=True)]


CASES_GROUP = [c for s in G_SHAPES for c in _group_epis(*s)]
CASES_GROUP_SWITCH = (
    [C("group", e, BF16, M, 256, 1, tune=dict(SR_GEMM_REG_EPI=v), **kw) for v in (0, 1) for M in (256, 257)
     for e, kw in (("bias", {}), ("qkv", _QKV256))] +
    [C("group", "resid", BF16, M, 256, kt, tune=dict(SR_GEMM_RESID_LDS=v)) for v in (0, 1)
     for M, kt in ((256, 1), (257, 2), (1, 1))] +
    [C("group", "qkv", BF16, 257, 256, 1, rope_npos=n, tune=dict(SR_GEMM_ROPE_LDS=v), tag=f"npos{n}", **_QKV256)
     for v in (0, 1) for n in (1, 16, 17, 64, 65)] +
    [C("group", e, BF16, 1025, 512, 1, tune=dict(SR_GEMM_GROUP_M=v), **kw) for v in (0, 3, 4)
     for e, kw in (("bias", {}), ("resid", {}))] +
    [C("group", "bias", BF16, 257, 256, 1, ldo_extra=4, tag="rows8B"),          # lds_epi off: 8-B aligned rows
     C("group", "qkv", BF16, 257, 256, 1, ldo_extra=4, tag="rows8B", **_QKV256),
     C("group", "bias", BF16, 257, 256, 1, out_align=8, tag="out8B"),
     C("group", "resid", BF16, 257, 256, 1, out_align=8, tag="out8B"),           # resid_lds off: out % 16 != 0
     C("group", "resid", BF16, 256, 256, 1, out_align=8, tag="out8B"),
     C("group", "bias", BF16, 257, 256, 1, q_scale=0.125, q_cols=192, tag="qcols192"),
     C("group", "bias", BF16, 256, 256, 1, q_scale=0.125, q_cols=192, tag="qcols192"),
     C("group", "qkv", BF16, 257, 512, 1, pos="grid", pos_row_base=7, tag="grid", **_QKV512),
     C("group", "qkv", BF16, 257, 512, 1, pos="rowmap", tag="rowmap", **_QKV512),
     C("group", "qkv", BF16, 257, 256, 1, embed_dim=128, col_offset=128, tag="kv"),
     C("group", "resid", BF16, 257, 256, 1, nobias=True, tag="nobias")])

# four problems of one launch: different M, N, K; one with 9 tiles (7 padding workgroups), one with M = 1
_G4_SHAPES = [(513, 768, 1), (1, 256, 2), (300, 512, 3), (256, 256, 1)]
_G4_QKV = {768: dict(embed_dim=256, q_scale=0.125, q_cols=256), 512: _QKV512, 256: _QKV256}
GROUP4 = {e: [C("group", e, BF16, M, N, kt, tag=f"p{i}", **dict(kw, **(_G4_QKV[N] if e == "qkv" else {})))
              for i, (M, N, kt) in enumerate(_G4_SHAPES)]
          for e, kw in (("bias", {}), ("gelu", dict(aux=True)), ("resid", {}), ("qkv", dict(aux=True)), ("f32", {}),
                        ("gelu_bwd", dict(colsum=True)))}

K256_M = 511 * 256 + 1  # 512 tiles at N = 256; the last row tile holds one row
K256_EPIS = [("bias", {}), ("gelu", dict(aux=True)), ("resid", {}), ("qkv", dict(aux=True, **_QKV256)), ("f32", {}),
             ("gelu_bwd", dict(colsum=True)), ("patch", dict(seg_rows=1021))]


def k256_cases(M, tag="", tune=None, epis=None):
    return [C("k256", e, BF16, M, 256, 1, pad=False, tag=tag, tune=tune or {}, **kw) for e, kw in K256_EPIS
            if epis is None or e in epis]


def tail_m(cus: int) -> int:
    """An M at N = 256 for which launch256_tail splits: one tile past whole rounds of ``cus`` workgroups,
    the rest (129 rows) two 128-row tiles, the last holding one row."""
    rounds = max(2, -(-512 // cus))
    return rounds * cus * 256 + 129


ALL_SMALL = CASES_K128 + CASES_K64 + CASES_K64_OFF + CASES_SPLITK + CASES_GROUP + CASES_GROUP_SWITCH


# ---------------------------------------------------------------- the pure index functions, restated
def tile_origin(tile, M, N, group_m):
    """(row tile, column tile) of linear tile ``tile``: column-major inside groups of group_m row tiles."""
    ntn, ntm = N // 256, -(-M // 256)
    if group_m > 1:
        per = group_m * ntn
        grp = tile // per
        first = grp * group_m
        gm, r = min(group_m, ntm - first), tile - grp * per
        return first + r % gm, r // gm
    return tile // ntn, tile % ntn


def group_starts(tiles):
    """start[] of a grouped launch: each problem's workgroup range padded to a multiple of 8."""
    s = [0]
    for t in tiles:
        s.append(s[-1] + (t + 7) // 8 * 8)
    return s


def splitk_ranges(ktiles, splits):
    per = ktiles // splits
    return [(z * per, min(z * per + per, ktiles)) for z in range(splits)]


def tail_split(M, N, cus):
    """(main_rows, rest) of launch256_tail, or None where it launches one kernel."""
    ntn = N // 256
    tiles = ntn * -(-M // 256)
    whole = tiles // cus * cus
    main_rows = whole // ntn * 256
    rest = M - main_rows
    small = -(-rest // 128) * (N // 128)
    if tiles % cus != 0 and main_rows > 0 and rest > 0 and small <= 2 * cus:
        return main_rows, rest
    return None
