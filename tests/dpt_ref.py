"""fp64 references of the DPT head's kernels (csrc/sr_dpt.hip, sr_conv3x3_f32) with per-element
error bounds, the seeded cases the CPU and GPU files share, and the mutants that show the bounds
bite.  No GPU here: tests/test_dpt_ref.py checks these references against torch's own fp64 ops and
shows that a correct fp32 implementation (torch's CPU ops) meets every bound;
tests/test_dpt_oracle_gpu.py holds the kernels to them.

Every reference returns ``(ref, mag)``: ``mag`` is the same expression on absolute values, the
quantity a rounding error analysis scales with.  u = 2^-24 is the fp32 unit roundoff and
gamma(k) = k u / (1 - k u) bounds a length-k fp32 sum of products in any order.  Feature maps are
NHWC, like the kernels'.

Bounds (per element):
    conv3x3          gamma(9c + 2) mag      9c products, the bias add, the residual multiply-add
    gemm + scatter   gamma(cin + 1) mag     cin products and the bias add
    resize_bilinear  8 u mag (+ 2 u |add|)  coordinates and weights are computed in fp32 exactly as
                                            PyTorch defines them -- they are part of the operation:
                                            against fp64 coordinates torch's own fp32 op is off by
                                            up to 15 x this bound -- and only the blend is fp64
    pos_embed        8 u (|x| + ratio)      |pos| <= 1, the fp32 two-sided linspace is within 3 u of
                                            the ideal one, so sin / cos move by <= 3.5 u; then one
                                            multiply and one add
    head_out         act(s -+ delta) (1 -+ 4u), delta = gamma(cin + 2) mag + 4u: expf / expm1f are
                                            1-ulp functions, 1 / (1 + expf(-s)) and 1 + expf(s)
                                            round twice more
    unproject        16 u mag
    im2col3x3, convt_scatter, add_, relu_   bit-exact
"""

import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64 = torch.float64


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; a zero bound admits only got == ref."""
    d = (got.to(F64) - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, float("inf"), 0.0).to(F64))
    return float(r.max())


def rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------- conv3x3
def _w_oihw(w, c):
    return w.reshape(w.shape[0], 3, 3, c).permute(0, 3, 1, 2)


def conv3x3(x, w, bias, stride, relu_in, base=None, gamma_=None, mutant=None):
    """x [n,h,w,c], w [cout, 9c] (K order ky, kx, ci), pad 1: conv + bias, or with ``base``
    base + gamma_ * (conv + bias).  Mutants: "neighbour" -- the kx = 0 tap of output column 0
    reads the pixel at x = 0 (its neighbour) instead of the zero padding; "gamma" -- gamma_
    ignored."""
    c = x.shape[3]
    xd = x.to(F64)
    if relu_in:
        xd = xd.clamp_min(0)
    wd = _w_oihw(w.to(F64), c)

    def run(xx, ww, bb):
        xp = F.pad(xx.permute(0, 3, 1, 2), (1, 1, 1, 1))
        if mutant == "neighbour":
            xp[:, :, :, 0] = xp[:, :, :, 1]
        y = F.conv2d(xp, ww, None if bb is None else bb, stride=stride, padding=0)
        return y.permute(0, 2, 3, 1)

    ref = run(xd, wd, None if bias is None else bias.to(F64))
    mag = run(xd.abs(), wd.abs(), None if bias is None else bias.to(F64).abs())
    if base is not None:
        g = gamma_.to(F64) if mutant != "gamma" else torch.ones_like(gamma_, dtype=F64)
        ref = base.to(F64) + g * ref
        mag = base.to(F64).abs() + gamma_.to(F64).abs() * mag
    return ref, mag


def conv3x3_bound(c, mag):
    return gamma(9 * c + 2) * mag


# (n, h, w, c, cout, stride, relu_in, mode); mode: "plain" out = conv + bias, "resid1" out += conv + bias
# (gamma = 1, as the head calls it), "gamma" out += gamma * (conv + bias) with random gamma, "nobias",
# "gamma_nobias".  The first four are tests/test_dpt_gpu.py's.
CONV_CASES = [
    (2, 19, 23, 64, 32, 1, False, "plain"),
    (1, 37, 37, 128, 64, 2, False, "plain"),
    (2, 15, 11, 32, 36, 1, True, "resid1"),
    (1, 9, 130, 256, 4, 1, True, "plain"),
    (1, 8, 6, 32, 64, 2, False, "plain"),     # stride 2 on even sizes: the last window has no right / bottom pad
    (1, 8, 6, 32, 8, 2, False, "plain"),      # the narrow kernel (cout <= 32) at stride 2
    (1, 1, 7, 32, 4, 1, False, "plain"),      # h == 1: the ky = 0 and ky = 2 taps are all padding
    (1, 5, 1, 32, 36, 1, False, "plain"),     # w == 1
    (1, 16, 16, 32, 32, 1, False, "plain"),   # M = 256: exactly one narrow tile
    (1, 1, 257, 32, 32, 1, False, "plain"),   # M = 257: one pixel row past it
    (1, 6, 6, 32, 132, 1, False, "plain"),    # N crosses a 128 tile
    (2, 15, 11, 32, 36, 1, True, "gamma"),
    (1, 6, 6, 32, 132, 1, False, "gamma"),
    (1, 8, 6, 32, 8, 2, False, "gamma"),
    (1, 8, 6, 32, 8, 2, False, "nobias"),
    (1, 8, 6, 32, 64, 2, False, "nobias"),
    (2, 15, 11, 32, 36, 1, True, "gamma_nobias"),
]
_CONV = {}


def conv_case(case):
    """Inputs and (ref, mag) of one CONV_CASES entry, computed once (callers do not modify them)."""
    if case not in _CONV:
        n, h, w, c, cout, stride, relu, mode = case
        g = torch.Generator().manual_seed(n * 1000 + c + 7 * cout + h)
        x = torch.randn(n, h, w, c, generator=g)
        wt = torch.randn(cout, 9 * c, generator=g) / (3 * c ** 0.5)
        b = None if "nobias" in mode else torch.randn(cout, generator=g)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        base = gam = None
        if mode == "resid1":
            base, gam = torch.randn(n, ho, wo, cout, generator=g), torch.ones(cout)
        elif mode.startswith("gamma"):
            base, gam = torch.randn(n, ho, wo, cout, generator=g), torch.randn(cout, generator=g) * 2
        ref, mag = conv3x3(x, wt, b, stride, relu, base, gam)
        _CONV[case] = dict(x=x, w=wt, b=b, base=base, gamma=gam, ref=ref, mag=mag)
    return _CONV[case]


# ---------------------------------------------------------------- ConvTranspose (kernel == stride)
def convt(y, w, bias, k):
    """y [n,h,w,cin], w [(ky, kx, co), cin] -> [n, h k, w k, co] (F.conv_transpose2d, stride = kernel = k)."""
    cin = y.shape[3]
    co = w.shape[0] // (k * k)
    wd = w.to(F64).reshape(k, k, co, cin).permute(3, 2, 0, 1)

    def run(yy, ww, bb):
        return F.conv_transpose2d(yy.permute(0, 3, 1, 2), ww, bb, stride=k).permute(0, 2, 3, 1)

    bd = None if bias is None else bias.to(F64)
    return run(y.to(F64), wd, bd), run(y.to(F64).abs(), wd.abs(), None if bd is None else bd.abs())


CONVT_CASES = [(2, 3, 5, 32, 8, 4), (1, 4, 2, 64, 36, 2)]  # n, h, w, cin, co, k


def convt_inputs(case):
    """y, nn.ConvTranspose2d's weight [cin, co, k, k], bias, and the weight as the head's GEMM
    reads it [(ky, kx, co), cin] (DPTHead._convt_w)."""
    n, h, w, cin, co, k = case
    g = torch.Generator().manual_seed(cin + k)
    y = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cin, co, k, k, generator=g) / cin ** 0.5
    b = torch.randn(co, generator=g)
    return y, wt, b, wt.permute(2, 3, 1, 0).reshape(k * k * co, cin).contiguous()


def convt_scatter(g, n, h, w, k, co, bias):
    """g [(f, y, x), (ky, kx, c)] -> out [f, y k + ky, x k + kx, c] + bias[c]: a permutation and
    one fp32 add, bit-exact."""
    out = g.reshape(n, h, w, k, k, co).permute(0, 1, 3, 2, 4, 5).reshape(n, h * k, w * k, co)
    mag = out.abs().to(F64)
    if bias is not None:
        out = out + bias
        mag = mag + bias.abs().to(F64)
    return out.contiguous(), mag


SCATTER_CASES = [(2, 3, 5, 8, 4), (3, 4, 2, 36, 2), (1, 1, 1, 4, 4)]  # n, h, w, co, k


# ---------------------------------------------------------------- im2col
def im2col3x3(x, stride, relu_in):
    """[n ho wo, 9c] with K order (ky, kx, ci), zeros outside, ReLU on the input: a gather, bit-exact."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    xx = x.clamp_min(0) if relu_in else x
    xp = F.pad(xx, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            for ky in range(3) for kx in range(3)]
    out = torch.stack(taps, 3).reshape(n * ho * wo, 9 * c).contiguous()
    return out, out.abs().to(F64)


IM2COL_CASES = [(2, 5, 7, 4), (1, 1, 6, 36), (1, 6, 1, 8), (1, 8, 6, 32)]


# ---------------------------------------------------------------- bilinear resize
def _axis(n_in, n_out, mutant=None):
    """PyTorch's align_corners=True source index and weights of one axis, in fp32:
    s = float(in - 1) / float(out - 1) (0 when out == 1), f = s * float(o), i0 = int(f),
    l1 = f - i0, l0 = 1 - l1, i1 = i0 + (i0 < in - 1)."""
    f32 = torch.float32
    s = (torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(n_out - 1), dtype=f32)
         if n_out > 1 else torch.tensor(0.0, dtype=f32))
    f = s * torch.arange(n_out, dtype=f32)
    i0 = f.to(torch.int64).clamp_max(n_in - 1)
    l1 = f - i0.to(f32)
    l0 = 1.0 - l1
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    if mutant == "last_cell":  # x1 = x0 in the last source cell
        i1 = torch.where(i0 == n_in - 2, i0, i1)
    return i0, i1, l0.to(F64), l1.to(F64)


def resize_bilinear(x, ho, wo, add=None, mutant=None):
    """F.interpolate(bilinear, align_corners=True) of NHWC x, + ``add``: one [ho, wo, c] table for
    every frame.  fp32 coordinates (see the module docstring), fp64 blend in PyTorch's order.
    Mutants: "last_cell"; "add_per_frame" -- the table is indexed with the frame's offset still in
    the pixel index, so frame f reads it f pixels on (wrapped); one frame cannot tell."""
    n, h, w, c = x.shape
    y0, y1, ly0, ly1 = _axis(h, ho)
    x0, x1, lx0, lx1 = _axis(w, wo, mutant if mutant == "last_cell" else None)
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]

    def blend(v):
        top, bot = v[:, y0], v[:, y1]
        return ly0 * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1 * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])

    ref, mag = blend(x.to(F64)), blend(x.to(F64).abs())
    if add is not None:
        a = add.to(F64).reshape(1, ho, wo, c).expand(n, ho, wo, c)
        if mutant == "add_per_frame":
            a = torch.stack([add.to(F64).reshape(-1).roll(-f * c).reshape(ho, wo, c) for f in range(n)])
        ref = ref + a
        mag = mag + add.to(F64).abs().reshape(1, ho, wo, c)
    return ref, mag


def resize_bound(mag, add=None):
    b = 8 * U * mag
    if add is not None:
        b = b + 2 * U * add.to(F64).abs().reshape(1, *mag.shape[1:])
    return b


RESIZE_CASES = [(2, 2, 3, 8, 4, 5), (1, 19, 19, 4, 37, 37), (1, 1, 5, 4, 14, 70), (1, 5, 1, 4, 3, 1),
                (2, 8, 10, 12, 3, 4), (1, 4, 4, 4, 1, 1)]  # n, h, w, c, ho, wo


def resize_inputs(case):
    n, h, w, c, ho, wo = case
    return rand((n, h, w, c), 100 + h * w + ho), rand((ho, wo, c), 200 + h * w + ho)  # x, a non-constant add


# ---------------------------------------------------------------- positional embedding
def pos_embed(h, w, c, aspect, ratio):
    """ratio * (uv-grid sincos table) [h, w, c] in fp64 from ideal linspaces (utils.py create_uv_grid +
    position_grid_to_embed): what oracle.sfm_oracle._uv_pos_embed states, without its fp32 linspace.
    ``mag``: the ratio (|sin|, |cos| <= 1)."""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag

    def lin(span, n):
        a = -span * (n - 1) / n
        if n == 1:
            return torch.tensor([a], dtype=F64)
        return a + torch.arange(n, dtype=F64) * (2 * span * (n - 1) / n / (n - 1))

    q = c // 4
    omega = 1.0 / 100.0 ** (torch.arange(q, dtype=F64) / q)

    def one(pos):
        arg = pos[:, None] * omega[None]
        return torch.cat([arg.sin(), arg.cos()], 1)

    ex = one(lin(sx, w))[None, :, :].expand(h, w, c // 2)
    ey = one(lin(sy, h))[:, None, :].expand(h, w, c // 2)
    table = torch.cat([ex, ey], -1) * ratio
    return table, torch.full_like(table, abs(ratio))


def pos_embed_bound(x, ratio):
    return 8 * U * (x.to(F64).abs() + abs(ratio))


POS_SHAPES = [(2, 4, 5, 8), (1, 1, 1, 4), (1, 37, 28, 32), (1, 3, 70, 64)]  # (1,1,1,4): steps == 1 on both axes
POS_ASPECTS = [1.0, 70 / 56, 0.5]
POS_RATIOS = [0.1, 1.0]


# ---------------------------------------------------------------- output head
ACTS = {"inv_log": lambda s: torch.sign(s) * torch.expm1(s.abs()), "exp": torch.exp,
        "linear": lambda s: s, "relu": lambda s: s.clamp_min(0)}
CONF_ACTS = {"expp1": lambda s: 1 + torch.exp(s), "expp0": torch.exp, "sigmoid": torch.sigmoid}
MAY_BE_ZERO = {"inv_log", "linear", "relu"}  # the others are positive over s in [-12, 12]


def head_out(hidden, w, b, act, conf_act):
    """conv1x1(relu(hidden)) + b in fp64: returns (s [npix, cout], delta, f_act, f_conf) with
    delta = gamma(cin + 2) (sum |relu(h)| |w| + |b|) + 4u the slack of an fp32 s, and the two
    activations (head_act.py:82-114) as monotone fp64 functions."""
    hd = hidden.to(F64).clamp_min(0)
    s = hd @ w.to(F64).T
    mag = hd @ w.to(F64).abs().T
    if b is not None:
        s = s + b.to(F64)
        mag = mag + b.to(F64).abs()
    return s, gamma(w.shape[1] + 2) * mag + 4 * U, ACTS[act], CONF_ACTS[conf_act]


def _down(v, zero):
    return torch.where(v >= 0, v * (1 - 4 * U), v * (1 + 4 * U)) - (4 * U if zero else 0.0)


def _up(v):
    return torch.where(v >= 0, v * (1 + 4 * U), v * (1 - 4 * U))


def head_out_interval(s, delta, f, may_be_zero):
    """[f(s - delta) (1 - 4u) - 4u [f may be 0], f(s + delta) (1 + 4u)]: f is monotone
    non-decreasing, so an fp32 s within delta and a 4-ulp activation land inside; the factors swap
    for negative values."""
    return _down(f(s - delta), may_be_zero), _up(f(s + delta))


def head_out_check(got, s, delta, f, may_be_zero):
    """(every element inside its interval, the largest |got - f(s)| over the interval's reach on
    that side): the second is what the files print, below 1 inside."""
    got = got.to(F64)
    if not bool(torch.isfinite(got).all()):
        return False, float("inf")
    lo, hi = head_out_interval(s, delta, f, may_be_zero)
    mid = f(s)
    d = got - mid
    reach = torch.where(d >= 0, hi - mid, mid - lo)
    r = torch.where(d == 0, torch.zeros_like(d), d.abs() / reach.clamp_min(1e-300))
    return bool(((got >= lo) & (got <= hi)).all()), float(r.max())


HEAD_OUT_CASES = [(4, 2, 1), (32, 4, 255), (4, 4, 257), (32, 2, 1000)]  # cin, cout, npix


def head_out_inputs(cin, cout, npix, seed=0):
    """hidden, w, b with s spanning about +-12, both signs and near 0 (row p's scale ramps 0 .. 1)."""
    g = torch.Generator().manual_seed(cin * 100 + cout * 10 + npix + seed)
    ramp = torch.linspace(0, 1, npix)[:, None] if npix > 1 else torch.ones(1, 1)
    hidden = torch.randn(npix, cin, generator=g) * ramp
    w = torch.randn(cout, cin, generator=g) * (12.0 / (0.6 * cin ** 0.5) / 3)
    b = torch.randn(cout, generator=g) * 0.1
    return hidden, w, b


# ---------------------------------------------------------------- unprojection
def unproject(depth, extr, intr):
    """oracle.sfm_oracle.unproject_depth (geometry.py:19-130) and its magnitude."""
    from oracle import sfm_oracle as O
    ref = O.unproject_depth(depth, extr, intr)
    S, H, W = depth.shape[:3]
    v, u = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    mags = []
    for s in range(S):
        K, E, d = intr[s].to(F64).abs(), extr[s].to(F64).abs(), depth[s].to(F64).abs().reshape(H, W)
        cam = torch.stack([(u + K[0, 2]) * d / K[0, 0], (v + K[1, 2]) * d / K[1, 1], d], -1)
        R, t = E[:, :3], E[:, 3]
        mags.append(cam @ R + R.T @ t)
    return ref, torch.stack(mags)


def unproject_inputs():
    """(s, h, w) = (2, 5, 9): fx != fy, an off-centre principal point, depths including 0 and 1e3."""
    g = torch.Generator().manual_seed(11)
    S, H, W = 2, 5, 9
    q = torch.randn(S, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w_ = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_),
                     2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_),
                     2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)], -1).view(S, 3, 3)
    extr = torch.cat([R, torch.randn(S, 3, 1, generator=g)], -1).contiguous()
    intr = torch.zeros(S, 3, 3)
    intr[:, 0, 0], intr[:, 1, 1] = torch.tensor([7.5, 11.0]), torch.tensor([9.25, 6.0])
    intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = torch.tensor([3.1, 6.7]), torch.tensor([1.2, 3.9]), 1.0
    depth = torch.rand(S, H, W, generator=g) * 5 + 0.1
    depth[0, 0, 0], depth[1, 4, 8], depth[0, 2, 3] = 0.0, 1e3, 1e3
    return depth, extr, intr


# ---------------------------------------------------------------- the whole head
# name -> (constructor keywords beyond DPT_SMALL, B, S, H, W)
HEAD_CONFIGS = {
    "56x70": (dict(), 1, 3, 56, 70),
    "84x56-B2": (dict(), 2, 2, 84, 56),          # even patch grids (6 x 4): stride 2 on even sizes; B > 1
    "60x75": (dict(), 1, 2, 60, 75),             # not multiples of 14: the maps are 56 x 70
    "down2": (dict(down_ratio=2), 1, 2, 56, 70),
    "down2-feat": (dict(down_ratio=2, feature_only=True), 1, 3, 56, 70),
    "nopos": (dict(pos_embed=False), 1, 2, 56, 70),
    "linear-sigmoid": (dict(activation="linear", conf_activation="sigmoid"), 1, 2, 56, 70),
    "relu-expp0": (dict(activation="relu", conf_activation="expp0"), 1, 2, 56, 70),
}
_HEAD = {}


def head_metric(got, ref):
    """max |got - ref| / (|ref| + rms(ref))."""
    got, ref = got.to(F64), ref.to(F64)
    return float(((got - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max())


def head_case(name):
    """Model, state dict, seeded tokens / images of one HEAD_CONFIGS entry, the fp64 oracle's outputs
    and the metric of the fp32 CPU oracle against them; computed once and shared."""
    if name not in _HEAD:
        from goldens import DPT_SMALL, dpt_oracle_kwargs
        from oracle import sfm_oracle as O
        from sailrecon_amd.heads.dpt_head import DPTHead
        from sailrecon_amd.utils.synth_weights import synth_state_dict_like
        cfg, B, S, H, W = HEAD_CONFIGS[name]
        m = DPTHead(**DPT_SMALL, **cfg)
        sd = synth_state_dict_like(m)
        g = torch.Generator().manual_seed(len(name) * 31 + H)
        P = 5 + (H // 14) * (W // 14)
        toks = {l: torch.randn(B, S, P, DPT_SMALL["dim_in"], generator=g) for l in DPT_SMALL["intermediate_layer_idx"]}
        images = torch.rand(B, S, 3, H, W, generator=g)
        kw = dpt_oracle_kwargs(cfg)

        def run(dt):
            out = O.dpt_forward({k: v.to(dt) for k, v in sd.items()}, "", {l: t.to(dt) for l, t in toks.items()},
                                images, 5, **kw)
            return (out,) if cfg.get("feature_only") else tuple(out)

        ref, f32 = run(F64), run(torch.float32)
        _HEAD[name] = dict(model=m, sd=sd, toks=toks, images=images, ref=ref,
                           cpu_metric=[head_metric(a, b) for a, b in zip(f32, ref)])
    return _HEAD[name]
