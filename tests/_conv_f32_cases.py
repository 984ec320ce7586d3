"""The cases of tests/test_gpu_conv_f32_grade.py (the convolutions that multiply fp32 operands on the fp32 matrix pipe) with their
operands and references, shared with tests/test_conv_ref_host.py, which proves on the CPU that every case reaches the launch regime
its comment claims, that tier A's bar rejects the mutants and that tier B's operands are exact.  Nothing is imported from the
package; the launchers' arithmetic is restated in _conv_ref.  Everything is computed once per shape (lru_cache) and never written to:
the four tiles and the two gather loops of one geometry share it."""
import functools

import numpy as np

import _conv_f32x3_cases as X
import _conv_ref as R
from _conv_ref import F32, F64

SLOPE = X.SLOPE
seed_of, out_hw, relu = X.seed_of, X.out_hw, X.relu
FAMILIES = sorted(R.FAMILIES)
TILES = (1, 2, 3, 4)                       # IGEMM_TILE: 128 x 128, 128 x 64, 64 x 64, 128 x 32

# ============================================================================================== 1. conv_igemm_kernel, geometries
# (n, h, w, ci, co, k, stride, pad), each under every tile and both gather loops.  All of them have fewer than 384 tiles of 64 x 64:
# a plain forward (and a stride-1 plain data gradient) runs as two K-slices that add atomically, 1x1 excepted (one tap).
IG = [
    (1, 9, 15, 32, 136, 3, 1, 1),     # 3x3/1; ci a multiple of the K-tile (uniform loop unless GENERIC_GATHER); M = 135 and co = 136: full
                                      # and ragged row / column tiles in one launch at every tile; the data gradient gathers 136: generic
    (1, 9, 15, 40, 64, 3, 1, 1),      # ci = 40, no multiple of the K-tile: generic loop only; the data gradient gathers 64 (uniform), produces 40
    (1, 11, 17, 32, 72, 3, 2, 1),     # 3x3/2 on odd extents (6 x 9 output): the data gradient's four parity classes are ragged; 12 binades
    (1, 11, 17, 32, 64, 1, 2, 0),     # 1x1/2: one tap (never sliced); three EMPTY parity classes in the data gradient
    (1, 10, 14, 32, 40, 4, 2, 1),     # 4x4/2 (16 taps); co = 40, no multiple of 32
    (1, 18, 22, 4, 64, 7, 2, 3),      # the stem: 7x7/2, 4 channels, 49 taps: generic loop in both directions
    (1, 9, 13, 32, 24, 5, 2, 2),      # 5x5/2 on odd extents, co = 24 (the <= 32-channel heuristic tile)
]
IG_BINADES = {IG[2]: 12}
# the unsliced plain store (>= 384 tiles of 64 x 64): per tile a shape whose column tile is full, so that the FAST epilogue and its
# in-epilogue statistics run.  (n, h, w, ci, co), 3x3 / stride 1.
LARGE = {1: (1, 64, 192, 32, 128), 2: (1, 128, 192, 32, 64), 3: (1, 128, 192, 32, 64), 4: (1, 128, 192, 32, 32)}
# conv2d_dgrad_bnreduce (heuristic tile only; the convolution ci -> co, its gradient gathers co and PRODUCES ci): 64 x 64 and 128 x 32
BNR = [(1, 128, 192, 64, 32), (1, 128, 192, 32, 32)]
SPLIT = (1, 9, 15, 136, 32, 128)          # conv2d_dgrad_split: (n, h, w, ci, co, split): 128 is a multiple of every tile width
UPCAT = [(1, 10, 14, 32, 32, 40), (1, 10, 14, 32, 0, 40)]        # conv2d_fwd_upcat: (n, h, w, ca, cs, co), with and without a skip half


def ig_id(c):
    return "n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c


@functools.lru_cache(maxsize=None)
def ig_tier_a(case):
    n, h, w, ci, co, k, s, p = case
    rng = np.random.default_rng(seed_of("f32 ig", case))
    b = IG_BINADES.get(case, 0)
    ho, wo = out_hw(h, w, k, s, p)
    o = dict(x=R.randn_f32(rng, (n, h, w, ci), binades=b), wt=R.randn_f32(rng, (co, k, k, ci), (k * k * ci) ** -0.5, binades=b),
             bias=R.randn_f32(rng, (co,)), res=R.randn_f32(rng, (n, ho, wo, co)), old=R.randn_f32(rng, (n, ho, wo, co)),
             dy=R.randn_f32(rng, (n, ho, wo, co), binades=b), oldx=R.randn_f32(rng, (n, h, w, ci)))
    o["fwd"] = R.f32_fwd(o["x"], o["wt"], s, p, R.MFMA_32)
    o["dgrad"] = R.f32_dgrad(o["dy"], o["wt"], s, p, h, w, R.MFMA_32)
    return o


def with_res(t, key):
    """A tier B operand set plus a small-integer residual (|bias| + |residual| <= 2 = the 'extra' of its window)."""
    t["res"] = R.small_ints(np.random.default_rng(seed_of("res", key)), t["r64"].shape)
    return t


@functools.lru_cache(maxsize=None)
def ig_tier_b(case, family):
    """(forward, data gradient)."""
    n, h, w, ci, co, k, s, p = case
    ho, wo = out_hw(h, w, k, s, p)
    return (with_res(X.conv_tier_b(("f32 ig",) + case, family, (n, h, w, ci), (co, k, k, ci), k, s, p), case),
            X.conv_tier_b(("f32 ig",) + case, family, (n, ho, wo, co), (co, k, k, ci), k, s, p, dgrad_to=(h, w), extra=1.0))


@functools.lru_cache(maxsize=None)
def large_tier_a(shape):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(seed_of("f32 large", shape))
    o = dict(x=R.randn_f32(rng, (n, h, w, ci)), wt=R.randn_f32(rng, (co, 3, 3, ci), (9 * ci) ** -0.5))
    o["fwd"] = R.f32_fwd(o["x"], o["wt"], 1, 1, R.MFMA_32)
    return o


@functools.lru_cache(maxsize=None)
def large_tier_b(shape, family):
    n, h, w, ci, co = shape
    return X.conv_tier_b(("f32 large",) + shape, family, (n, h, w, ci), (co, 3, 3, ci), 3, 1, 1, extra=0.0)


@functools.lru_cache(maxsize=None)
def bnr_tier_a(case):
    n, h, w, ci, co = case
    rng = np.random.default_rng(seed_of("f32 bnr", case))
    o = dict(dy=R.randn_f32(rng, (n, h, w, co)), wt=R.randn_f32(rng, (co, 3, 3, ci), (9 * co) ** -0.5))
    o.update(X.bn_operands(rng, (n, h, w, ci)))
    o["dgrad"] = R.f32_dgrad(o["dy"], o["wt"], 1, 1, h, w, R.MFMA_32)
    return o


@functools.lru_cache(maxsize=None)
def split_tier_a():
    n, h, w, ci, co, _ = SPLIT
    rng = np.random.default_rng(seed_of("f32 split", SPLIT))
    o = dict(dy=R.randn_f32(rng, (n, h, w, co)), wt=R.randn_f32(rng, (co, 3, 3, ci), (9 * co) ** -0.5))
    o["dgrad"] = R.f32_dgrad(o["dy"], o["wt"], 1, 1, h, w, R.MFMA_32)
    return o


@functools.lru_cache(maxsize=None)
def split_tier_b(family):
    n, h, w, ci, co, _ = SPLIT
    return X.conv_tier_b(("f32 split",) + SPLIT, family, (n, h, w, co), (co, 3, 3, ci), 3, 1, 1, dgrad_to=(h, w), extra=0.0)


@functools.lru_cache(maxsize=None)
def upcat_tier_a(case, group=R.MFMA_32):
    n, h, w, ca, cs, co = case
    rng = np.random.default_rng(seed_of("f32 upcat", case))
    a = R.randn_f32(rng, (n, h // 2, w // 2, ca))
    skip = R.randn_f32(rng, (n, h, w, cs)) if cs else None
    wt, bias = R.randn_f32(rng, (co, 3, 3, ca + cs), (9 * (ca + cs)) ** -0.5), R.randn_f32(rng, (co,))
    return dict(a=a, skip=skip, wt=wt, bias=bias, fwd=R.f32_fwd(R.upcat(a, skip), wt, 1, 1, group))


@functools.lru_cache(maxsize=None)
def upcat_tier_b(case, family):
    n, h, w, ca, cs, co = case
    t = X.conv_tier_b(("f32 upcat",) + case, family, (n, h, w, ca + cs), (co, 3, 3, ca + cs), 3, 1, 1, pre=X.up_pre(ca, cs))
    t["a"], t["skip"] = np.ascontiguousarray(t["x"][:, ::2, ::2, :ca]), (np.ascontiguousarray(t["x"][..., ca:]) if cs else None)
    return t


# ======================================================================================================== 2. the small kernels
# (n, h, w, gathered, produced): the forward g -> p and the flipped launch (the data gradient of p -> g, which gathers g and
# produces p) reach the same instantiation <ceil(g / 16), ceil(p / 16)>; the weight gradient is the one of the convolution g -> p.
# 18 x 22: one whole and one partial 16 x 16 tile per axis, even (the up-sampled source); 20 x 1: a one-pixel-wide image;
# 1 x 1 x 24580 (1537 tiles) and 1 x 2 x 12300 (769 tiles): more tiles than the 1536 (<1, 1>, <1, 2>) / 768 (<2, 1>) / 512 (weight
# gradient) blocks a launch may have, so that blocks loop over several tiles, at the fewest pixels that reach that.
SM = [(2, 18, 22, 16, 16), (2, 18, 22, 8, 24), (2, 18, 22, 24, 16), (2, 18, 22, 32, 8), (2, 18, 22, 16, 32), (2, 18, 22, 8, 8),
      (1, 20, 1, 16, 16), (1, 20, 1, 8, 24), (1, 20, 1, 24, 16),
      (1, 1, 24580, 8, 8), (1, 2, 12300, 24, 8), (1, 1, 24580, 8, 24)]
SM_BINADES = {SM[1]: 12}


def sm_id(c):
    return "n%d_%dx%d_g%d_p%d" % c


def sm_up(case):
    """The up-sampled source needs even extents."""
    return case[1] % 2 == 0 and case[2] % 2 == 0


@functools.lru_cache(maxsize=None)
def sm_tier_a(case):
    n, h, w, g, p = case
    rng = np.random.default_rng(seed_of("f32 small", case))
    b = SM_BINADES.get(case, 0)
    o = dict(x=R.randn_f32(rng, (n, h, w, g), binades=b), wt=R.randn_f32(rng, (p, 3, 3, g), (9 * g) ** -0.5, binades=b),
             bias=R.randn_f32(rng, (p,)), res=R.randn_f32(rng, (n, h, w, p)), old=R.randn_f32(rng, (n, h, w, p)),
             dy=R.randn_f32(rng, (n, h, w, g), binades=b), wd=R.randn_f32(rng, (g, 3, 3, p), (9 * g) ** -0.5, binades=b),
             dyw=R.randn_f32(rng, (n, h, w, p)), oldw=R.randn_f32(rng, (p, 3, 3, g)))
    o["fwd"] = R.f32_fwd(o["x"], o["wt"], 1, 1, R.MFMA_16)
    o["dgrad"] = R.f32_dgrad(o["dy"], o["wd"], 1, 1, h, w, R.MFMA_16)
    o["wgrad"] = R.f32_wgrad(o["x"], o["dyw"], 3, 1, 1, R.MFMA_16)
    # the unwritten BatchNorm activation as the weight gradient's gathered operand
    o["y_prev"] = (R.randn_f32(rng, (n, h, w, g)) * F32(1.5) + F32(0.3)).astype(F32)
    o["sc"], o["sh"] = X.bnin_operands(rng, g)
    o["z"] = R.bn_apply_f32(o["y_prev"], o["sc"], o["sh"], SLOPE)
    o["wgrad_z"] = R.f32_wgrad(o["z"], o["dyw"], 3, 1, 1, R.MFMA_16)
    if sm_up(case):
        o["a"] = np.ascontiguousarray(o["x"][:, ::2, ::2])
        o["fwd_up"] = R.f32_fwd(R.upcat(o["a"], None), o["wt"], 1, 1, R.MFMA_16)
        o["ya"] = np.ascontiguousarray(o["y_prev"][:, ::2, ::2])
        o["wgrad_zup"] = R.f32_wgrad(R.upcat(R.bn_apply_f32(o["ya"], o["sc"], o["sh"], SLOPE), None), o["dyw"], 3, 1, 1, R.MFMA_16)
    return o


@functools.lru_cache(maxsize=None)
def sm_tier_b(case, family):
    """dict: fwd, dgrad, wgrad, wgrad behind relu(1 x + 0), and with even extents fwd_up / wgrad_up (behind relu and the up-sampling)."""
    n, h, w, g, p = case
    key = ("f32 small",) + case
    t = dict(fwd=with_res(X.conv_tier_b(key, family, (n, h, w, g), (p, 3, 3, g), 3, 1, 1), case),
             dgrad=X.conv_tier_b(key, family, (n, h, w, g), (g, 3, 3, p), 3, 1, 1, dgrad_to=(h, w), extra=1.0),
             wgrad=X.wgrad_tier_b(key, family, (n, h, w, g), (n, h, w, p), 3, 1, 1),
             wgrad_z=X.wgrad_tier_b(key + ("z",), family, (n, h, w, g), (n, h, w, p), 3, 1, 1, pre=relu))
    if sm_up(case):
        t["fwd_up"] = X.conv_tier_b(key + ("up",), family, (n, h, w, g), (p, 3, 3, g), 3, 1, 1, pre=X.up_pre(g, 0))
        t["fwd_up"]["a"] = np.ascontiguousarray(t["fwd_up"]["x"][:, ::2, ::2])
        t["wgrad_up"] = X.wgrad_tier_b(key + ("zup",), family, (n, h, w, g), (n, h, w, p), 3, 1, 1, pre=lambda v: X.up_pre(g, 0)(relu(v)))
        t["wgrad_up"]["a"] = np.ascontiguousarray(t["wgrad_up"]["x"][:, ::2, ::2])
    return t


# ======================================================================================================== 3. conv_wgrad_kernel
# (n, h, w, ci, co, k, stride, pad), (WGRAD_BLOCKS values); co > 32: the 64 x 64 tile, else 32 x 128.  The gather is row-uniform
# when the output width is a multiple of 16 (64 x 64) or 8 (32 x 128), unless WGRAD_GENERIC.
WG = [
    ((2, 32, 48, 40, 72, 3, 1, 1), (0, 64, 4096)),      # M = 3072 in two images of 1536: 12 splits of 256 (default, 4096), 6 of 512 (64)
    ((2, 32, 48, 40, 24, 3, 1, 1), (0, 64)),            # 32 x 128: three tiles; 12 splits either way (22 wanted, 12 allowed)
    ((1, 9, 16, 40, 72, 3, 1, 1), (0,)),                # M = 144: ONE split, the plain (non-atomic) store when not accumulating
    ((1, 9, 16, 40, 24, 3, 1, 1), (0,)),
    ((3, 10, 16, 40, 72, 3, 1, 1), (0,)),               # M = 480 in images of 160: two splits of 256, the first ends INSIDE image 1
    ((1, 36, 64, 4, 64, 7, 2, 3), (0,)),                # the stem geometry: 7x7/2, 4 channels, 18 x 32 output
    ((1, 36, 44, 4, 64, 7, 2, 3), (0,)),                # ... at an output width of 22: generic gather whatever the switch
    ((2, 12, 12, 40, 72, 1, 1, 0), (0,)),               # 1x1/1: the one-row rewrite (wo = M = 288) makes a 12-pixel-wide image row-uniform
    ((2, 12, 12, 40, 24, 1, 1, 0), (0,)),
    ((2, 17, 32, 40, 72, 3, 2, 1), (0,)),               # stride 2: 9 x 16 output
]
# conv2d_wgrad_part: (n, h, w, ca, cs, co): the up-sampled half fills channels [0, ca), the skip half [ca, ca + cs) of dW
WG_PART = [(2, 16, 32, 32, 40, 72), (2, 16, 32, 32, 40, 24)]


@functools.lru_cache(maxsize=None)
def wg_tier_a(case):
    n, h, w, ci, co, k, s, p = case
    rng = np.random.default_rng(seed_of("f32 wg", case))
    ho, wo = out_hw(h, w, k, s, p)
    o = dict(x=R.randn_f32(rng, (n, h, w, ci)), dy=R.randn_f32(rng, (n, ho, wo, co)), oldw=R.randn_f32(rng, (co, k, k, ci)))
    o["wgrad"] = R.f32_wgrad(o["x"], o["dy"], k, s, p, R.MFMA_32)
    return o


@functools.lru_cache(maxsize=None)
def wg_tier_b(case, family):
    n, h, w, ci, co, k, s, p = case
    ho, wo = out_hw(h, w, k, s, p)
    return X.wgrad_tier_b(("f32 wg",) + case, family, (n, h, w, ci), (n, ho, wo, co), k, s, p)


@functools.lru_cache(maxsize=None)
def part_tier_a(case):
    n, h, w, ca, cs, co = case
    rng = np.random.default_rng(seed_of("f32 part", case))
    o = dict(a=R.randn_f32(rng, (n, h // 2, w // 2, ca)), skip=R.randn_f32(rng, (n, h, w, cs)), dy=R.randn_f32(rng, (n, h, w, co)),
             oldw=R.randn_f32(rng, (co, 3, 3, ca + cs)))
    o["x"] = R.upcat(o["a"], o["skip"])
    o["wgrad"] = R.f32_wgrad(o["x"], o["dy"], 3, 1, 1, R.MFMA_32)
    return o


WG_PART_X3 = WG_PART[:1]                  # the same two launches on conv_wgrad_x3_kernel (F32_SPLIT = 1; co = 72 > 32, ca and cs multiples of 8)


@functools.lru_cache(maxsize=None)
def part_x3_tier_a(case):
    """part_tier_a's operands with the split grade's reference (the six-product model as tier A's second leg)."""
    o = dict(part_tier_a(case))
    o["wgrad"] = R.x3_wgrad(o["x"], o["dy"], 3, 1, 1)
    return o


@functools.lru_cache(maxsize=None)
def part_tier_b(case, family):
    n, h, w, ca, cs, co = case
    t = X.wgrad_tier_b(("f32 part",) + case, family, (n, h, w, ca + cs), (n, h, w, co), 3, 1, 1, pre=X.up_pre(ca, cs))
    t["a"], t["skip"] = np.ascontiguousarray(t["x"][:, ::2, ::2, :ca]), np.ascontiguousarray(t["x"][..., ca:])
    return t


# ======================================================================= 4. conv2d_fwd_fused on an X3 instance (F32_SPLIT = 1)
X3_FUSED = X.X3[3]                        # 3x3 / stride 1, 40 -> 72


@functools.lru_cache(maxsize=None)
def x3_fused_tier_a():
    o = dict(X.x3_tier_a(X3_FUSED))
    n, h, w, ci, co, k, s, p = X3_FUSED
    o["res"] = R.randn_f32(np.random.default_rng(seed_of("x3 fused", X3_FUSED)), (n,) + out_hw(h, w, k, s, p) + (co,))
    return o


@functools.lru_cache(maxsize=None)
def x3_fused_tier_b(family):
    n, h, w, ci, co, k, s, p = X3_FUSED
    return with_res(X.conv_tier_b(("x3 fused",) + X3_FUSED, family, (n, h, w, ci), (co, k, k, ci), k, s, p), ("x3 fused",))


# ================================================================================================================== 5. bn_fold
BN_FOLD = [(4, 2.0 ** -20), (24, 1.0), (64, 2.0 ** 14)]       # (channels, scale of running_var): tiny (eps dominates), ordinary, large
BN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def bn_fold_operands(case):
    c, vs = case
    rng = np.random.default_rng(seed_of("bn fold", case))
    return dict(w=R.randn_f32(rng, (c, 3, 3, 8)), bias=R.randn_f32(rng, (c,)), gamma=(rng.random(c) + 0.5).astype(F32),
                beta=R.randn_f32(rng, (c,)), rm=R.randn_f32(rng, (c,)), rv=((rng.random(c) + 0.5) * vs).astype(F32))
