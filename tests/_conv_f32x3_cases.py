"""The cases of tests/test_gpu_conv_f32x3_grade.py and their operands and references, shared with tests/test_conv_ref_host.py (which
proves on the CPU, for every case, that the tier A bar rejects the mutants and that the tier B operands are exact) so that the two
files cannot drift.  Nothing is imported from the package; the launchers' predicates are restated in _conv_ref."""
import functools
import zlib

import numpy as np

import _conv_ref as R
from _conv_ref import F32, F64

SLOPE = float(F32(0.2))


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# ================================================================= 1. conv3x3_f32x3_kernel / conv3x3_f32x3_ws_kernel, configurations 1 .. 12
def _f3_cases():
    """(cfg, n, h, w, gathered, produced, mode): h = TH + 1 and w in {TW, TW + 2}: one whole and one ragged tile in each direction;
    produced counts below, at and above the configuration's channel block; always (8, 4) and (72, 68); one case per configuration
    family (one-role, wave-specialised 32 wide, wave-specialised 16 wide) over 40 binades."""
    out = []
    for cfg in range(1, 13):
        th, tw, cb = R.f3_tile(cfg)
        out += [(cfg, 2, th + 1, tw, 8, 4, "randn"), (cfg, 2, th + 1, tw + 2, 72, 68, "randn"), (cfg, 2, th + 1, tw + 2, 16, 36, "randn"),
                (cfg, 2, th + 1, tw, 24, 32 if cb == 32 else 12, "randn")]
    for cfg in (2, 5, 10):
        th, tw, _ = R.f3_tile(cfg)
        out.append((cfg, 2, th + 1, tw + 2, 24, 36, "binades"))
    return out


F3_CASES = _f3_cases()
# the in-staging BatchNorm transform: the same shapes at one one-role and one wave-specialised configuration
F3_BNIN = [c[:6] for c in F3_CASES if c[0] in (3, 6) and c[6] == "randn"]
# the fused decoder input cat([nearest_x2(a), skip]): (cfg, n, h, w, ca, cs, produced), h and w even
F3_UP = [(cfg, 2, R.f3_tile(cfg)[0] + 2, R.f3_tile(cfg)[1] + 2, ca, cs, 36) for cfg in (2, 6, 10) for ca, cs in ((16, 0), (16, 16), (48, 32))]


def f3_id(case):
    return "cfg%d-n%d_%dx%d_g%d_p%d" % case[:6] + ("" if len(case) < 7 or case[6] == "randn" else "-" + case[6])


def up_id(case):
    return "cfg%d-n%d_%dx%d_ca%d_cs%d_p%d" % case


def shape_of(case):
    """A case without its configuration: configurations with the same tile share operands and references (computed once, never
    written to)."""
    return tuple(case[1:])


def unique_shapes(cases):
    return sorted({shape_of(c) for c in cases}, key=repr)


def f3_tier_a(case):
    return _f3_tier_a(shape_of(case))


@functools.lru_cache(maxsize=None)
def _f3_tier_a(shape):
    """Operands and Refs of one case: the forward g -> p and the data gradient that GATHERS g and PRODUCES p (the convolution
    p -> g), so that both launches reach the same channel blocks."""
    n, h, w, g, p, mode = shape
    rng = np.random.default_rng(seed_of("f3", shape))
    b = 40 if mode == "binades" else 0
    o = dict(x=R.randn_f32(rng, (n, h, w, g), binades=b), wt=R.randn_f32(rng, (p, 3, 3, g), (9 * g) ** -0.5, binades=b),
             bias=R.randn_f32(rng, (p,)), dy=R.randn_f32(rng, (n, h, w, g), binades=b),
             wd=R.randn_f32(rng, (g, 3, 3, p), (9 * g) ** -0.5, binades=b), old=R.randn_f32(rng, (n, h, w, p), binades=b))
    o.update(bn_operands(rng, (n, h, w, p)))
    steps = R.halo3_steps(g)
    o["fwd"] = R.x3_fwd(o["x"], o["wt"], 1, 1, steps)
    o["dgrad"] = R.x3_dgrad(o["dy"], o["wd"], 1, 1, h, w, steps)
    return o


def bn_operands(rng, shape):
    """The BatchNorm of the layer behind a data gradient: its output, batch statistics and affine parameters.  Outputs whose
    activation argument is within 1e-3 of zero are moved away from it: the mask must not hang on the last bit of an fp32 shift."""
    c = shape[-1]
    y = R.randn_f32(rng, shape)
    mean, var = y.reshape(-1, c).mean(0).astype(F32), y.reshape(-1, c).var(0)
    rstd, gamma, beta = ((var + 1e-5) ** -0.5).astype(F32), (rng.random(c) + 0.5).astype(F32), (rng.standard_normal(c) * 0.3).astype(F32)
    sc = gamma.astype(F64) * rstd
    near = np.abs(y * sc + (beta - mean * sc)) < 1e-3
    y = np.where(near, y + 0.01 / sc, y).astype(F32)
    return dict(prev_y=y, mean=mean, rstd=rstd, gamma=gamma, beta=beta)


def bnin_operands(rng, g):
    return (rng.random(g) + 0.5).astype(F32), (rng.standard_normal(g) * 0.5).astype(F32)


def f3_bnin_a(case):
    return _f3_bnin_a(shape_of(case))


@functools.lru_cache(maxsize=None)
def _f3_bnin_a(shape):
    n, h, w, g, p = shape
    rng = np.random.default_rng(seed_of("f3 bnin", shape))
    y_prev = (R.randn_f32(rng, (n, h, w, g)) * F32(1.5) + F32(0.3)).astype(F32)
    sc, sh = bnin_operands(rng, g)
    wt, bias = R.randn_f32(rng, (p, 3, 3, g), (9 * g) ** -0.5), R.randn_f32(rng, (p,))
    z = R.bn_apply_f32(y_prev, sc, sh, SLOPE)
    return dict(y_prev=y_prev, sc=sc, sh=sh, wt=wt, bias=bias, z=z, fwd=R.x3_fwd(z, wt, 1, 1, R.halo3_steps(g)))


def f3_up_a(case):
    return _f3_up_a(shape_of(case))


@functools.lru_cache(maxsize=None)
def _f3_up_a(shape):
    n, h, w, ca, cs, p = shape
    rng = np.random.default_rng(seed_of("f3 up", shape))
    a = R.randn_f32(rng, (n, h // 2, w // 2, ca))
    skip = R.randn_f32(rng, (n, h, w, cs)) if cs else None
    wt, bias = R.randn_f32(rng, (p, 3, 3, ca + cs), (9 * (ca + cs)) ** -0.5), R.randn_f32(rng, (p,))
    return dict(a=a, skip=skip, wt=wt, bias=bias, fwd=R.x3_fwd(R.upcat(a, skip), wt, 1, 1, R.halo3_steps(ca + cs)))


# --------------------------------------------------------------------------------------------------------------- tier B
def conv_tier_b(key, family, xshape, wshape, k, stride, pad, dgrad_to=None, extra=2.0, pre=None):
    """Exact operands of one family for conv(pre(x), w) (dgrad_to = (hi, wi): for the data gradient of dy = x through w): x, w, the
    small-integer bias and old, r64 (before bias / old) and mag (with |bias| + |old| <= extra).  pre: what the kernel does to x while
    it stages it (an exact map with |pre(x)| <= pre(|x|)); 'xin' is pre(x)."""
    seed = seed_of("tier b", key, family, xshape, wshape, k, stride, pad, dgrad_to)
    pre = pre or (lambda v: v)
    if dgrad_to is None:
        op = lambda a, b: R.torch_fwd(pre(a), b, stride, pad, R.torch.float64)  # noqa: E731
    else:
        op = lambda a, b: R.torch_dgrad(a, b, stride, pad, dgrad_to[0], dgrad_to[1], R.torch.float64)  # noqa: E731
    kt = k * k * (wshape[3] if dgrad_to is None else wshape[0])
    x, w, tries = R.exact_pair(seed, family, xshape, wshape, op, kt, extra)
    r64 = op(x, w)
    rng = np.random.default_rng([seed, 99])
    return dict(x=x, xin=pre(x), w=w, r64=r64, mag=op(np.abs(x), np.abs(w)) + extra, bias=R.small_ints(rng, (r64.shape[-1],)),
                old=R.small_ints(rng, r64.shape), tries=tries, u=R.FAMILIES[family][2])


def f3_tier_b(case, family):
    return _f3_tier_b(shape_of(case)[:5], family)


@functools.lru_cache(maxsize=None)
def _f3_tier_b(shape, family):
    """(forward operands, data-gradient operands) of one case in one family."""
    n, h, w, g, p = shape
    return (conv_tier_b(shape, family, (n, h, w, g), (p, 3, 3, g), 3, 1, 1),
            conv_tier_b(shape, family, (n, h, w, g), (g, 3, 3, p), 3, 1, 1, dgrad_to=(h, w)))


def relu(v):
    return np.maximum(v, 0.0)


def up_pre(ca, cs):
    """Full-resolution x -> cat([nearest_x2(x[:, ::2, ::2, :ca]), x[..., ca:]]): 'a' is the even pixels of the first ca channels."""
    return lambda v: R.upcat(v[:, ::2, ::2, :ca], v[..., ca:] if cs else None)


def f3_bnin_b(case, family):
    return _f3_bnin_b(shape_of(case), family)


@functools.lru_cache(maxsize=None)
def _f3_bnin_b(shape, family):
    """scale 1, shift 0, ReLU: the transform is exact."""
    n, h, w, g, p = shape
    return conv_tier_b(("bnin",) + shape, family, (n, h, w, g), (p, 3, 3, g), 3, 1, 1, pre=relu)


def f3_up_b(case, family):
    return _f3_up_b(shape_of(case), family)


@functools.lru_cache(maxsize=None)
def _f3_up_b(shape, family):
    n, h, w, ca, cs, p = shape
    t = conv_tier_b(("up",) + shape, family, (n, h, w, ca + cs), (p, 3, 3, ca + cs), 3, 1, 1, pre=up_pre(ca, cs))
    t["a"], t["skip"] = np.ascontiguousarray(t["x"][:, ::2, ::2, :ca]), (np.ascontiguousarray(t["x"][..., ca:]) if cs else None)
    return t


# ===================================================================================== 3. conv2d_fwd_n16 / conv2d_dgrad_n16
# (n, h, w, gathered): every gathered count conv_n16_ok accepts (8 .. 32), at 1 x 3 x 18 and 2 x 9 x 34
N16 = [(n, h, w, g) for n, h, w in ((1, 3, 18), (2, 9, 34)) for g in (8, 16, 24, 32)]


@functools.lru_cache(maxsize=None)
def n16_tier_a(case):
    n, h, w, g = case
    rng = np.random.default_rng(seed_of("n16", case))
    o = dict(x=R.randn_f32(rng, (n, h, w, g)), wt=R.randn_f32(rng, (16, 3, 3, g), (9 * g) ** -0.5), dy=R.randn_f32(rng, (n, h, w, g)),
             wd=R.randn_f32(rng, (g, 3, 3, 16), (9 * g) ** -0.5))
    o["sc"], o["sh"] = bnin_operands(rng, g)
    o.update(bn_operands(rng, (n, h, w, 16)))
    steps = R.n16_steps(g)
    o["z"] = R.bn_apply_f32(o["x"], o["sc"], o["sh"], 0.0)
    o["fwd"], o["fwd_z"] = R.x3_fwd(o["x"], o["wt"], 1, 1, steps), R.x3_fwd(o["z"], o["wt"], 1, 1, steps)
    o["dgrad"] = R.x3_dgrad(o["dy"], o["wd"], 1, 1, h, w, steps)
    return o


@functools.lru_cache(maxsize=None)
def n16_tier_b(case, family):
    """(forward, forward behind the exact transform relu(1 x + 0), data gradient)."""
    n, h, w, g = case
    return (conv_tier_b(("n16",) + case, family, (n, h, w, g), (16, 3, 3, g), 3, 1, 1, extra=0.0),
            conv_tier_b(("n16 z",) + case, family, (n, h, w, g), (16, 3, 3, g), 3, 1, 1, extra=0.0, pre=relu),
            conv_tier_b(("n16",) + case, family, (n, h, w, g), (g, 3, 3, 16), 3, 1, 1, dgrad_to=(h, w), extra=0.0))


# ================================================================================================== 4. conv2d_fwd_stem
STEM = [(1, 18, 22), (2, 34, 66)]          # 7x7 / stride 2 / pad 3, 3 channels padded to 4 -> 64


@functools.lru_cache(maxsize=None)
def stem_tier_a(case):
    n, h, w = case
    rng = np.random.default_rng(seed_of("stem", case))
    x, wt = R.randn_f32(rng, (n, h, w, 4)), R.randn_f32(rng, (64, 7, 7, 4), 196 ** -0.5)
    return dict(x=x, wt=wt, fwd=R.x3_fwd(x, wt, 2, 3))


@functools.lru_cache(maxsize=None)
def stem_tier_b(case, family):
    n, h, w = case
    return conv_tier_b(("stem",) + case, family, (n, h, w, 4), (64, 7, 7, 4), 7, 2, 3, extra=0.0)


# ============================================================ 5. the shared-source kernels with the split (F32_SPLIT = 1)
# (n, h, w, ci, co, k, stride, pad): 3x3 / stride 2, 1x1 / stride 2, 4x4 / stride 2 / pad 1, 3x3 / stride 1 with 40 -> 72 channels
X3 = [(1, 10, 14, 40, 72, 3, 2, 1), (1, 10, 14, 40, 72, 1, 2, 0), (1, 10, 14, 40, 72, 4, 2, 1), (1, 10, 14, 40, 72, 3, 1, 1),
      # output widths 7 and 14 above: conv_wgrad_x3_kernel<..., false> only.  Row-uniform (the width a multiple of the 32-row load pass):
      (1, 8, 32, 40, 72, 3, 1, 1),          # M = 256: ONE split, the plain store
      (3, 5, 32, 40, 72, 3, 1, 1),          # M = 480 in images of 160: two splits of 256, the first ends INSIDE image 1
      (1, 17, 64, 40, 72, 3, 2, 1),         # stride 2: 9 x 32 output
      (2, 12, 12, 40, 72, 1, 1, 0)]         # 1x1/1: row-uniform through the one-row rewrite (wo = M = 288) only


def out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def x3_tier_a(case):
    n, h, w, ci, co, k, s, p = case
    rng = np.random.default_rng(seed_of("x3", case))
    ho, wo = out_hw(h, w, k, s, p)
    o = dict(x=R.randn_f32(rng, (n, h, w, ci)), wt=R.randn_f32(rng, (co, k, k, ci), (k * k * ci) ** -0.5), bias=R.randn_f32(rng, (co,)),
             dy=R.randn_f32(rng, (n, ho, wo, co)), oldw=R.randn_f32(rng, (co, k, k, ci)))
    o["fwd"], o["dgrad"] = R.x3_fwd(o["x"], o["wt"], s, p), R.x3_dgrad(o["dy"], o["wt"], s, p, h, w)
    o["wgrad"] = R.x3_wgrad(o["x"], o["dy"], k, s, p)
    return o


def wgrad_tier_b(key, family, xshape, dyshape, k, stride, pad, extra=1.0, pre=None):
    """Exact operands of a weight gradient: K is the pixel axis, the sparsity is chosen over it; the family's 'w' side is dy."""
    seed = seed_of("tier b wgrad", key, family, xshape, dyshape, k, stride, pad)
    pre = pre or (lambda v: v)
    op = lambda a, b: R.torch_wgrad(pre(a), b, k, stride, pad, R.torch.float64)  # noqa: E731
    x, dy, tries = R.exact_pair(seed, family, xshape, dyshape, op, dyshape[0] * dyshape[1] * dyshape[2], extra)
    r64 = op(x, dy)
    rng = np.random.default_rng([seed, 99])
    return dict(x=x, xin=pre(x), w=dy, r64=r64, mag=op(np.abs(x), np.abs(dy)) + extra, old=R.small_ints(rng, r64.shape), tries=tries,
                u=R.FAMILIES[family][2], geom=(k, stride, pad))


@functools.lru_cache(maxsize=None)
def x3_tier_b(case, family):
    """(forward, data gradient, weight gradient)."""
    n, h, w, ci, co, k, s, p = case
    ho, wo = out_hw(h, w, k, s, p)
    return (conv_tier_b(("x3",) + case, family, (n, h, w, ci), (co, k, k, ci), k, s, p, extra=1.0),
            conv_tier_b(("x3",) + case, family, (n, ho, wo, co), (co, k, k, ci), k, s, p, dgrad_to=(h, w), extra=0.0),
            wgrad_tier_b(("x3",) + case, family, (n, h, w, ci), (n, ho, wo, co), k, s, p))


# ========================================================================================================= 6. weight gradients
# K is the pixel axis: n h w between 64 and about 700, at every channel-block shape the launchers accept at these sizes
WG_HALO = [(2, 9, 34, 64, 64), (2, 9, 34, 32, 32), (2, 9, 34, 64, 32), (2, 9, 34, 32, 64), (1, 4, 16, 64, 128), (1, 4, 16, 128, 64)]      # (n, h, w, ci, co)
WG_HALO_UP = [(2, 10, 34, 64, 64, 64), (2, 10, 34, 32, 32, 32), (1, 4, 16, 64, 64, 64)]                               # (n, h, w, ca, cs, co)
# the pair-packed forms (WGRAD_PAIR = 7): 16 gathered channels -> 8 .. 32, and 32 up-sampled channels without a skip half -> 16
WG_PAIR = [(2, 9, 34, 16, 16), (2, 9, 34, 16, 32), (1, 4, 16, 16, 8), (2, 9, 34, 16, 24)]
WG_PAIR_UP = [(2, 10, 34, 32, 0, 16)]
WG_BNIN = [(2, 9, 34, 32, 32), (2, 9, 34, 64, 64), (1, 4, 16, 128, 64)]
WG_UP = [(2, 10, 34, 64, 0, 64), (1, 4, 64, 64, 0, 64), (1, 4, 64, 64, 0, 32), (2, 10, 34, 64, 64, 64)]             # configurations 2, 1, 3, 2
WG_UP_BLOCKS = (0, 16, 600)
WG_SLICE = [(2, 9, 34, 32, 32, 64, 96)]                                                     # (n, h, w, slice channels, co, c_off, row length)


@functools.lru_cache(maxsize=None)
def wg_tier_a(kind, case):
    """x is the convolution's gathered tensor at full resolution (the fused input materialised); 'a', 'skip' its sources."""
    rng = np.random.default_rng(seed_of("wg", kind, case))
    n, h, w = case[:3]
    o = {}
    if kind in ("up", "halo_up"):
        ca, cs, co = case[3:6]
        o["a"] = R.randn_f32(rng, (n, h // 2, w // 2, ca))
        o["skip"] = R.randn_f32(rng, (n, h, w, cs)) if cs else None
        x = R.upcat(o["a"], o["skip"] if kind == "halo_up" or not cs else np.zeros((n, h, w, cs), F32))
    elif kind == "bnin":
        ci, co = case[3:5]
        o["y_prev"] = (R.randn_f32(rng, (n, h, w, ci)) * F32(1.5) + F32(0.3)).astype(F32)
        o["sc"], o["sh"] = bnin_operands(rng, ci)
        x = R.bn_apply_f32(o["y_prev"], o["sc"], o["sh"], SLOPE)
    else:
        ci, co = case[3:5]
        x = R.randn_f32(rng, (n, h, w, ci))
    o["x"], o["dy"] = x, R.randn_f32(rng, (n, h, w, co))
    o["oldw"] = R.randn_f32(rng, (co, 3, 3, x.shape[-1]))
    o["wgrad"] = R.x3_wgrad(x, o["dy"], 3, 1, 1)
    return o


@functools.lru_cache(maxsize=None)
def wg_tier_b(kind, case, family):
    n, h, w = case[:3]
    if kind in ("up", "halo_up"):
        ca, cs, co = case[3:6]
        pre = up_pre(ca, cs)
        if kind == "up" and cs:              # the phase-form launch owns the first ca channels only: the skip half is zero here
            pre = lambda v: R.upcat(v[:, ::2, ::2, :ca], np.zeros(v.shape[:3] + (cs,), F32))  # noqa: E731
        t = wgrad_tier_b((kind,) + case, family, (n, h, w, ca + cs), (n, h, w, co), 3, 1, 1, pre=pre)
        t["a"], t["skip"] = np.ascontiguousarray(t["x"][:, ::2, ::2, :ca]), (np.ascontiguousarray(t["x"][..., ca:]) if cs else None)
        return t
    ci, co = case[3:5]
    return wgrad_tier_b((kind,) + case, family, (n, h, w, ci), (n, h, w, co), 3, 1, 1, pre=relu if kind == "bnin" else None)


# ================================================================ 2. the phase kernels (csrc/conv_up_f32x3.hip), UP_CFG 1 .. 8
def _up_cases():
    """(cfg, n, h, w of the OUTPUT, ca, cs, co): the 2 x 2 output, and one whole plus one ragged tile of a in each direction
    (a: (TH + 1) x (TW + 1)); ca in {16, 48}, cs in {0, 16}, co in {8, 40}."""
    out = []
    for cfg in range(1, 9):
        th, tw, _, _ = R.up_tile(cfg, True)
        out += [(cfg, 1, 2, 2, 16, 0, 8), (cfg, 2, 2 * th + 2, 2 * tw + 2, 48, 16, 40), (cfg, 1, 2 * th + 2, 2 * tw + 2, 16, 16, 8),
                (cfg, 1, 2 * th + 2, 2 * tw + 2, 48, 0, 40)]
    return out


UP = _up_cases()


def up_tier_a(case):
    return _up_tier_a(shape_of(case))


@functools.lru_cache(maxsize=None)
def _up_tier_a(shape):
    n, h, w, ca, cs, co = shape
    rng = np.random.default_rng(seed_of("up", shape))
    o = dict(a=R.randn_f32(rng, (n, h // 2, w // 2, ca)), wt=R.randn_f32(rng, (co, 3, 3, ca + cs), (9 * (ca + cs)) ** -0.5),
             old=R.randn_f32(rng, (n, h, w, co)), dy=R.randn_f32(rng, (n, h, w, co)), olda=R.randn_f32(rng, (n, h // 2, w // 2, ca)))
    o.update(bn_operands(rng, (n, h // 2, w // 2, ca)))
    w_up = np.ascontiguousarray(o["wt"][..., :ca])
    o["fwd"], o["dgrad"] = R.x3_up_fwd(o["a"], w_up), R.x3_up_dgrad(o["dy"], w_up)
    return o


def up_tier_b(case, family):
    return _up_tier_b(shape_of(case), family)


@functools.lru_cache(maxsize=None)
def _up_tier_b(shape, family):
    """(forward, data gradient): full weights [co][3][3][ca + cs] whose skip half is zero."""
    n, h, w, ca, cs, co = shape
    f = conv_tier_b(("up phase",) + shape, family, (n, h, w, ca), (co, 3, 3, ca), 3, 1, 1, extra=1.0, pre=up_pre(ca, 0))
    f["a"] = np.ascontiguousarray(f["x"][:, ::2, ::2])
    seed = seed_of("up phase dgrad", shape, family)
    op = lambda a, b: R.pool2(R.torch_dgrad(a, b, 1, 1, h, w, R.torch.float64))  # noqa: E731
    dy, wt, tries = R.exact_pair(seed, family, (n, h, w, co), (co, 3, 3, ca), op, 36 * co, 1.0)
    rng = np.random.default_rng([seed, 99])
    b = dict(x=dy, xin=dy, w=wt, r64=op(dy, wt), mag=op(np.abs(dy), np.abs(wt)) + 1.0, old=R.small_ints(rng, (n, h // 2, w // 2, ca)), tries=tries,
             u=R.FAMILIES[family][2])
    return f, b


def widen_up(w_up, cs):
    """[co][3][3][ca] -> [co][3][3][ca + cs] with a zero skip half (the packer reads rows of ca + cs channels)."""
    return np.concatenate([w_up, np.zeros(w_up.shape[:3] + (cs,), F32)], axis=3) if cs else w_up
