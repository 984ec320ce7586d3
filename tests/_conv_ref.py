"""float64 restatement of the bf16-storage convolutions (csrc/conv_halo_bf16.hip and the bf16 instances of csrc/conv_igemm.hip,
csrc/conv_wgrad.hip, csrc/conv_wgrad_halo2.hip): forward, data gradient, weight gradient and the fused decoder input
cat([nearest_x2(a), skip]), with the epilogue terms (bias, residual, LeakyReLU, old contents of an accumulating call) and the
fused BatchNorm statistics.

Test infrastructure, in the manner of ``_norm_ref`` / ``_loss_ref``; nothing is imported from the package.  Tensors are NHWC numpy
arrays holding bf16-representable fp32 values, weights are OHWI ``[co][kh][kw][ci]``.  For the operands of one launch a ``Ref``
holds, per output element,

* ``r64``       the operation in float64 (torch's double-precision convolution / autograd),
* ``mag``       the sum of the absolute values of the terms that formed the element (the same operation on |x|, |w|),
* ``leg_rne``   torch's fp32 CPU convolution (autograd for the gradients) on the same operands,
* ``leg_trunc`` im2col in float64 with an fp32 accumulator that is truncated toward minus infinity after every group of 16 terms of
                the K axis (taps outer, channels inner; the pixel axis for the weight gradient):
                acc = trunc(float64(acc) + A[:, j:j+16] @ B[j:j+16]).  A deliberately pessimistic model of the bf16 MFMA adder,
                which truncates toward minus infinity (profiles/r04_mfma_bias.txt).

The bar is ``_norm_ref.bar`` with two legs: A = max(4 x max over the WHOLE output of max(|leg_rne - r64|, |leg_trunc - r64|) / mag,
2^-22).  fp32 outputs must satisfy |got - r64| <= A mag element-wise, bf16 outputs |got - r64| <= A mag + bf16_half_ulp(r64, A mag),
nothing masked.  LeakyReLU is 1-Lipschitz: act(r64) is graded with the bar of the pre-activation.

Fused BatchNorm statistics: the kernels sum the fp32 value before the bf16 rounding, so the reference is sum_p r64 and sum_p r64^2
per channel with magnitudes sum_p mag and sum_p mag^2; the leg is a sequential float32 cumsum over the pixels of leg_trunc (a worse
order than any blocked kernel order).  d is the leg's worst normalised deviation over ALL channels, as everywhere in _norm_ref.bar:
the error of one channel's sum of squares is a sum of terms 2 r e of either sign, a random walk whose end point in a single channel
can be arbitrarily close to 0 in the leg while it is not in the kernel (for two walks of equal scale |kernel| > 4 |leg| happens in
about 16 % of the channels), so a bar taken channel by channel would fail correct kernels; the maximum over 24 ... 136 channels
is a stable estimate of the walk's scale.  The verdict itself is per channel.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _norm_ref import F32, F64, FLOOR, bf16_half_ulp, bf16_round, normalised  # noqa: F401  (bf16_round: re-exported for the tests)

GROUP = 16                                # terms per MFMA step: v_mfma_f32_32x32x16_bf16
MARGIN = 4.0


class Ref:
    """(r64, mag, leg_rne, leg_trunc) of one output; iterable in that order."""
    def __init__(self, r64, mag, leg_rne, leg_trunc):
        self.r64, self.mag = np.asarray(r64, dtype=F64), np.asarray(mag, dtype=F64)
        self.leg_rne, self.leg_trunc = np.asarray(leg_rne, dtype=F32), np.asarray(leg_trunc, dtype=F32)

    def __iter__(self):
        return iter((self.r64, self.mag, self.leg_rne, self.leg_trunc))


def trunc_to_fp32_toward_minus_inf(x):
    """The largest fp32 value <= x (x float64, finite, inside the fp32 range)."""
    x = np.asarray(x, dtype=F64)
    y = np.atleast_1d(x.astype(F32)).copy()
    up = y.astype(F64) > np.atleast_1d(x)
    y[up] = np.nextafter(y[up], F32(-np.inf))
    return y.reshape(x.shape)


# ------------------------------------------------------------------------------------------------------------------- im2col
def _pads(pad):
    return ((pad, pad), (pad, pad)) if np.isscalar(pad) else pad


def im2col(x, k, stride, pad):
    """x [n][h][w][c] -> (A [n ho wo][k k c] float64, taps outer and channels inner, (n, ho, wo)); pad: int or ((top, bottom), (left, right))."""
    x = np.asarray(x, dtype=F64)
    n, h, w, c = x.shape
    (pt, pb), (pl, pr) = _pads(pad)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    ho, wo = (h + pt + pb - k) // stride + 1, (w + pl + pr - k) // stride + 1
    cols = [xp[:, r:r + stride * (ho - 1) + 1:stride, q:q + stride * (wo - 1) + 1:stride, :] for r in range(k) for q in range(k)]
    return np.stack(cols, axis=3).reshape(n * ho * wo, k * k * c), (n, ho, wo)


def wmat(w):
    """OHWI weights -> B [kh kw ci][co]."""
    w = np.asarray(w, dtype=F64)
    return w.reshape(w.shape[0], -1).T


def trunc_matmul(A, B, group=GROUP):
    """A @ B with the fp32 accumulator truncated toward minus infinity after every ``group`` terms of K."""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    for j in range(0, A.shape[1], group):
        acc = trunc_to_fp32_toward_minus_inf(acc.astype(F64) + A[:, j:j + group] @ B[j:j + group])
    return acc


def dgrad_as_forward(dy, w, stride, pad, hi, wi):
    """The data gradient as a stride-1 correlation: (dy dilated by the stride, flipped and transposed weights OHWI with O = ci,
    the ((top, bottom), (left, right)) padding that yields hi x wi)."""
    dy, w = np.asarray(dy), np.asarray(w)
    n, ho, wo, co = dy.shape
    k = w.shape[1]
    hd, wd = (ho - 1) * stride + 1, (wo - 1) * stride + 1
    d = np.zeros((n, hd, wd, co), dtype=dy.dtype)
    d[:, ::stride, ::stride] = dy
    lo = k - 1 - pad
    wf = np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))
    return d, wf, ((lo, hi + k - 1 - hd - lo), (lo, wi + k - 1 - wd - lo))


def upcat(a, skip):
    """cat([nearest_x2(a), skip], C), materialised."""
    up = np.repeat(np.repeat(np.asarray(a), 2, axis=1), 2, axis=2)
    return up if skip is None else np.concatenate([up, np.asarray(skip)], axis=3)


# ----------------------------------------------------------------------------------------------------------- the im2col products
def im2col_fwd(x, w, stride, pad, matmul=np.matmul):
    A, (n, ho, wo) = im2col(x, np.shape(w)[1], stride, pad)
    return matmul(A, wmat(w)).reshape(n, ho, wo, np.shape(w)[0])


def im2col_dgrad(dy, w, stride, pad, hi, wi, matmul=np.matmul):
    d, wf, pads = dgrad_as_forward(dy, w, stride, pad, hi, wi)
    return im2col_fwd(d, wf, 1, pads, matmul)


def im2col_wgrad(x, dy, k, stride, pad, matmul=np.matmul):
    """dw OHWI = dy^T [co][pixels] @ A [pixels][k k ci]: K is the pixel axis."""
    A, _ = im2col(x, k, stride, pad)
    co, ci = np.shape(dy)[3], np.shape(x)[3]
    return matmul(np.asarray(dy, dtype=F64).reshape(-1, co).T, A).reshape(co, k, k, ci)


# ---------------------------------------------------------------------------------------------------------------- torch's legs
def _nchw(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def torch_fwd(x, w, stride, pad, dt):
    return _nhwc(F.conv2d(_nchw(x, dt), _nchw(w, dt), None, stride=stride, padding=pad))


def torch_dgrad(dy, w, stride, pad, hi, wi, dt):
    xr = torch.zeros(np.shape(dy)[0], np.shape(w)[3], hi, wi, dtype=dt, requires_grad=True)
    F.conv2d(xr, _nchw(w, dt), None, stride=stride, padding=pad).backward(_nchw(dy, dt))
    return _nhwc(xr.grad)


def torch_wgrad(x, dy, k, stride, pad, dt):
    wr = torch.zeros(np.shape(dy)[3], np.shape(x)[3], k, k, dtype=dt, requires_grad=True)
    F.conv2d(_nchw(x, dt), wr, None, stride=stride, padding=pad).backward(_nchw(dy, dt))
    return _nhwc(wr.grad)


# -------------------------------------------------------------------------------------------------------------------- the Refs
def fwd(x, w, stride, pad):
    """y = conv(x, w) without any epilogue term."""
    return Ref(torch_fwd(x, w, stride, pad, torch.float64), torch_fwd(np.abs(x), np.abs(w), stride, pad, torch.float64),
               torch_fwd(x, w, stride, pad, torch.float32), im2col_fwd(x, w, stride, pad, trunc_matmul))


def fwd_upcat(a, skip, w):
    """The fused decoder input: the same 3x3 convolution on the materialised cat([nearest_x2(a), skip])."""
    return fwd(upcat(a, skip), w, 1, 1)


def dgrad(dy, w, stride, pad, hi, wi):
    return Ref(torch_dgrad(dy, w, stride, pad, hi, wi, torch.float64), torch_dgrad(np.abs(dy), np.abs(w), stride, pad, hi, wi, torch.float64),
               torch_dgrad(dy, w, stride, pad, hi, wi, torch.float32), im2col_dgrad(dy, w, stride, pad, hi, wi, trunc_matmul))


def wgrad(x, dy, k, stride, pad):
    return Ref(torch_wgrad(x, dy, k, stride, pad, torch.float64), torch_wgrad(np.abs(x), np.abs(dy), k, stride, pad, torch.float64),
               torch_wgrad(x, dy, k, stride, pad, torch.float32), im2col_wgrad(x, dy, k, stride, pad, trunc_matmul))


def leaky(t, slope, dt):
    return np.where(t < 0, t * dt(slope), t).astype(dt)


def epilogue(ref, bias=None, residual=None, slope=None, old=None):
    """act(conv + bias + residual) + old in the kernels' order, float64 for r64 and fp32 steps for the two legs; every term that
    enters adds its absolute value to the magnitude.  slope None: no activation (0.0: ReLU)."""
    r64, mag, legs = ref.r64, ref.mag, [ref.leg_rne, ref.leg_trunc]
    for term in (bias, residual):
        if term is not None:
            r64, mag = r64 + np.asarray(term, dtype=F64), mag + np.abs(np.asarray(term, dtype=F64))
            legs = [(l + np.asarray(term, dtype=F32)).astype(F32) for l in legs]
    if slope is not None:
        r64, legs = leaky(r64, slope, F64), [leaky(l, slope, F32) for l in legs]
    if old is not None:
        r64, mag = r64 + np.asarray(old, dtype=F64), mag + np.abs(np.asarray(old, dtype=F64))
        legs = [(l + np.asarray(old, dtype=F32)).astype(F32) for l in legs]
    return Ref(r64, mag, *legs)


def bar(ref, margin=MARGIN):
    """(A, d_rne, d_trunc): A = max(margin x the worse leg's worst normalised deviation over the whole output, 2^-22)."""
    d_rne = float(normalised(ref.leg_rne.astype(F64) - ref.r64, ref.mag).max(initial=0.0))
    d_trunc = float(normalised(ref.leg_trunc.astype(F64) - ref.r64, ref.mag).max(initial=0.0))
    return max(margin * max(d_rne, d_trunc), FLOOR), d_rne, d_trunc


def excess(got, r64, mag, A, bf16_out):
    """Element-wise |got - r64| beyond the half-ulp of a bf16 store, normalised by the magnitude: the verdict is excess <= A.
    inf where the shape is wrong or anything is not finite."""
    got = np.asarray(got, dtype=F64)
    if got.shape != r64.shape or not np.isfinite(got).all():
        return np.full(r64.shape, np.inf)
    err = np.abs(got - r64)
    if bf16_out:
        err = np.maximum(err - bf16_half_ulp(r64, A * mag), 0.0)
    return normalised(err, mag)


def verdict(got, ref, bf16_out):
    """(passes, e, A, d_rne, d_trunc, index of the worst element)."""
    A, d_rne, d_trunc = bar(ref)
    ex = excess(got, ref.r64, ref.mag, A, bf16_out)
    e = float(ex.max(initial=0.0))
    where = tuple(int(i) for i in np.unravel_index(int(np.argmax(ex)), ex.shape)) if ex.size else ()
    return bool(e <= A) and np.isfinite(d_rne) and np.isfinite(d_trunc), e, A, d_rne, d_trunc, where


def stats_ref(ref):
    """Per-channel (sum, sum of squares) of a [..., channels] output as two Refs; both legs are the sequential fp32 cumsum of leg_trunc."""
    c = ref.r64.shape[-1]
    r, m, l = ref.r64.reshape(-1, c), ref.mag.reshape(-1, c), ref.leg_trunc.reshape(-1, c)
    c1 = np.cumsum(l, axis=0, dtype=F32)[-1]
    c2 = np.cumsum((l * l).astype(F32), axis=0, dtype=F32)[-1]
    return Ref(r.sum(0), m.sum(0), c1, c1), Ref((r * r).sum(0), (m * m).sum(0), c2, c2)


class Grader:
    """Collects the verdicts of one case so that every figure is logged before the first assertion fires."""
    PREFIX, LEG = "conv-grade", "d_trunc"

    def __init__(self, tag, log=print):
        self.tag, self.bad, self.log = tag, [], log

    def grade(self, what, got, ref, bf16_out):
        ok, e, A, d_rne, d_trunc, where = verdict(got, ref, bf16_out)
        a_rne = max(MARGIN * d_rne, FLOOR)
        self.log(f"{self.PREFIX} {self.tag} | {what} | {'bf16' if bf16_out else 'fp32'} | e {e:.3e} d_rne {d_rne:.3e} {self.LEG} {d_trunc:.3e} "
                 f"bar {A:.3e} e/bar {e / A:.3f} e/bar_rne {e / a_rne:.3f} at {where}")
        if not ok:
            self.bad.append(f"{what}: e {e:.3e} > bar {A:.3e} at {where}")

    def exact(self, what, got, want):
        same = np.array_equal(np.asarray(got), np.asarray(want))
        self.log(f"{self.PREFIX} {self.tag} | {what} | {'exact' if same else 'DIFFERS'}")
        if not same:
            self.bad.append(f"{what}: not bit for bit")

    def note(self, what, ok, text):
        self.log(f"{self.PREFIX} {self.tag} | {what} | {text}")
        if not ok:
            self.bad.append(f"{what}: {text}")

    def done(self):
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)


# ------------------------------------------------------------------------------------------------------------------- operands
def randn_bf16(rng, shape, scale=1.0, binades=False):
    """randn rounded to bf16 (as fp32); binades: every element times 2^randint(-10, 10), operands that span 20 binades."""
    v = rng.standard_normal(shape) * scale
    if binades:
        v = v * np.exp2(rng.integers(-10, 10, size=shape))
    return bf16_round(v.astype(F32))


# ------------------------------------------------------------------------------------------ tile arithmetic of the launchers
def halo_tile(cfg):
    """(TH, TW, channels per block) of conv_halo_bf16_kernel<3, CK, WM, WN, RPW, TW>: TH = WM * RPW * (32 / TW), 32 WN channels."""
    wm, wn, rpw, tw = {1: (4, 1, 2, 32), 2: (2, 2, 4, 32), 3: (2, 4, 4, 32), 4: (2, 2, 4, 16), 5: (2, 4, 4, 16), 6: (2, 2, 2, 16)}[cfg]
    return wm * rpw * (32 // tw), tw, 32 * wn


def cdiv(a, b):
    return -(-a // b)


def halo_blocks(cfg, n, h, w, produced, classes=1):
    th, tw, cb = halo_tile(cfg)
    return n * cdiv(h, th) * cdiv(w, tw) * cdiv(produced, cb) * classes


def halo_instance(k, gathered, produced, cfg=0, up=None, s2_ck=64):
    """The rocprofv3 symbol launch_halo picks (csrc/conv_halo_bf16.hip) for a launch that is not a plain bf16-output 1x1 (those go
    to the streamer / GEMM kernel unless NO_STREAM is set).  k = 4: gathered is the VIRTUAL count, 4 x the real channels.
    cfg: HALO_CFG (0: the not-preferred fallback, by produced channels); up = (ca, cb) of a fused decoder input."""
    name = "conv_halo_bf16_kernel<%d, %d, %d, %d, %d, %d>"
    if k == 4:
        ck = 64 if s2_ck == 64 and gathered % 64 == 0 else 32
        return name % ((2, ck, 2, 2, 4, 32) if produced <= 64 else (2, ck, 2, 4, 4, 32))
    ck = 16 if gathered % 32 or (up and (up[0] % 32 or up[1] % 32)) else 32
    choice = cfg if cfg else (1 if produced <= 32 else 2 if produced <= 64 else 3)
    if choice > 3 and (k != 3 or ck != 32):
        choice = 2 if produced <= 64 else 3
    if k == 3:
        if ck == 16:
            return name % ((3, 16, 4, 1, 2, 32) if choice == 1 else (3, 16, 2, 2, 4, 32))
        return name % {1: (3, 32, 4, 1, 2, 32), 2: (3, 32, 2, 2, 4, 32), 3: (3, 32, 2, 4, 4, 32), 4: (3, 32, 2, 2, 4, 16),
                       5: (3, 32, 2, 4, 4, 16), 6: (3, 32, 2, 2, 2, 16)}[choice]
    if ck == 32 and gathered % 64 == 0:
        return name % ((1, 64, 2, 4, 4, 32) if choice == 3 else (1, 64, 2, 2, 4, 32))
    if ck == 16:
        return name % (1, 16, 2, 2, 4, 32)
    return name % ((1, 32, 2, 4, 4, 32) if choice == 3 else (1, 32, 2, 2, 4, 32))


def stream_instance(gathered, produced):
    """conv1x1_stream_bf16_kernel<CK, WM, WN>: 256-pixel flat tiles x 32 WN channels."""
    return "conv1x1_stream_bf16_kernel<%d, %d, %d>" % ((64 if gathered % 64 == 0 else 16,) + ((2, 4) if produced > 64 else (4, 2)))


def igemm_instance(tile, uniform):
    """conv_igemm_kernel<BM, BN, WAVES_M, WAVES_N, bf16, uniform-tap loop, fused input>; tile: IGEMM_TILE 1..4."""
    bm, bn, wm, wn = {1: (128, 128, 2, 2), 2: (128, 64, 2, 2), 3: (64, 64, 2, 2), 4: (128, 32, 4, 1)}[tile]
    return "conv_igemm_kernel<%d, %d, %d, %d, true, %s, false>" % (bm, bn, wm, wn, "true" if uniform else "false")


def igemm_uniform(gathered, taps, generic):
    """finish_args: the uniform-tap loop needs whole 64-element K tiles per tap and at most 32 taps."""
    return not generic and gathered % 64 == 0 and taps <= 32


def fold_factor(gathered, produced, width, no_fold=False):
    """Pixels folded into one 64-channel unit by the 3x3 / stride 1 bf16 launches of the shared implicit-GEMM source."""
    if no_fold or gathered not in (16, 32):
        return 1
    f = 64 // gathered
    if width % f or produced % 8 or (f == 4 and produced > 16):
        return 1
    return f


# =================================================================================== the fp32 convolutions on the three-term split
# csrc/conv_halo_f32x3.hip, conv_up_f32x3.hip, conv_n16_f32x3.hip, conv_stem_f32x3.hip and the X3 instances of conv_igemm.hip,
# conv_wgrad.hip, conv_wgrad_halo2.hip (tests/test_gpu_conv_f32x3_grade.py).  Operands are ARBITRARY fp32 values.  The second leg of
# a Ref (stored in ``leg_trunc``, logged as d_x3) is the six-product model: both operands split by oracle/f32x3_ref.py::split3, and
# for every step of at most 16 K-terms the six products x_i w_j (i + j <= 2, smallest first, the kernels' order) are added ONE MATRIX
# INSTRUCTION AT A TIME to an fp32 accumulator truncated toward minus infinity after each of them; the steps that
# negated_groups / up_negated_groups name run on the negated accumulator, which truncates toward plus infinity.
from oracle.f32x3_ref import negated_groups, split3  # noqa: E402

PAIRS = [(ij - j, j) for ij in (2, 1, 0) for j in range(ij + 1)]          # (term of A, term of B), smallest products first
SENTINEL = -12345.5                                                     # the guard value around every output buffer
GUARD = 256


class X3Grader(Grader):
    PREFIX, LEG = "f32x3-grade", "d_x3"


def _terms(v):
    return [t.astype(F64) for t in split3(np.asarray(v, dtype=F32))]


def x3_matmul(A, B, steps=None, drop=()):
    """The six-product model of A @ B.  steps: [(columns of K, negated)] in the kernel's order (None: 16 consecutive terms, no sign
    pattern); drop: pairs (i, j) left out (mutants)."""
    sa, sb = _terms(A), _terms(B)
    kk = np.shape(A)[1]
    if steps is None:
        steps = [(slice(j, j + GROUP), False) for j in range(0, kk, GROUP)]
    acc = np.zeros((np.shape(A)[0], np.shape(B)[1]), dtype=F32)
    for cols, neg in steps:
        a, b = [t[:, cols] for t in sa], [t[cols] for t in sb]
        for i, j in PAIRS:
            if (i, j) in drop:
                continue
            p = a[i] @ b[j]
            acc = -trunc_to_fp32_toward_minus_inf(-(acc.astype(F64) + p)) if neg else trunc_to_fp32_toward_minus_inf(acc.astype(F64) + p)
    return acc


def x3_exact(A, B, drop=(), flip=None):
    """sum over the kept pairs of A_i @ B_j in float64, nothing truncated; flip: columns of K accumulated with the wrong sign."""
    sa, sb = _terms(A), _terms(B)
    out = np.zeros((np.shape(A)[0], np.shape(B)[1]), dtype=F64)
    for i, j in PAIRS:
        if (i, j) not in drop:
            out += sa[i] @ sb[j]
            if flip is not None:
                out -= 2.0 * (sa[i][:, flip] @ sb[j][flip])
    return out


def halo3_steps(gathered, signs=True):
    """K loop of conv3x3_f32x3_kernel / _ws_kernel over im2col columns (tap (dy, dx) outer, channel inner): 16-channel chunk outer,
    dx, then dy; group G = 3 chunk + dx carries the sign (csrc/halo_common.h::f3_negated_groups)."""
    nk16 = cdiv(gathered, 16)
    neg = negated_groups(nk16) if signs else ()
    return [((dy * 3 + dx) * gathered + np.arange(16 * c, min(16 * c + 16, gathered)), 3 * c + dx in neg)
            for c in range(nk16) for dx in range(3) for dy in range(3)]


def x3_fwd(x, w, stride, pad, steps=None):
    mm = lambda A, B: x3_matmul(A, B, steps)  # noqa: E731
    return Ref(torch_fwd(x, w, stride, pad, torch.float64), torch_fwd(np.abs(x), np.abs(w), stride, pad, torch.float64),
               torch_fwd(x, w, stride, pad, torch.float32), im2col_fwd(x, w, stride, pad, mm))


def x3_dgrad(dy, w, stride, pad, hi, wi, steps=None):
    mm = lambda A, B: x3_matmul(A, B, steps)  # noqa: E731
    return Ref(torch_dgrad(dy, w, stride, pad, hi, wi, torch.float64), torch_dgrad(np.abs(dy), np.abs(w), stride, pad, hi, wi, torch.float64),
               torch_dgrad(dy, w, stride, pad, hi, wi, torch.float32), im2col_dgrad(dy, w, stride, pad, hi, wi, mm))


def x3_wgrad(x, dy, k, stride, pad):
    """K is the pixel axis; the per-tile, per-block sign pattern of the weight-gradient kernels is not restated: no signs."""
    return Ref(torch_wgrad(x, dy, k, stride, pad, torch.float64), torch_wgrad(np.abs(x), np.abs(dy), k, stride, pad, torch.float64),
               torch_wgrad(x, dy, k, stride, pad, torch.float32), im2col_wgrad(x, dy, k, stride, pad, x3_matmul))


def bn_apply_f32(y, scale, shift, slope):
    """act(fma(y, scale, shift)) with ONE fp32 rounding of the fused multiply-add, what the in-staging transform and bn_apply store."""
    z = (np.asarray(y, dtype=F64) * np.asarray(scale, dtype=F64) + np.asarray(shift, dtype=F64)).astype(F32)
    return z if slope is None else leaky(z, slope, F32)


def bn_sums_ref(ref, prev_y, mean, rstd, gamma, beta, slope):
    """The two BatchNorm-backward sums of the epilogue of a data gradient: per channel sum_p g m and sum_p g m y_hat with
    m = act'(fma(y, gamma rstd, beta - mean gamma rstd)) and y_hat = (y - mean) rstd, as two Refs: float64 definitions on r64, the
    magnitudes sum_p mag |m| and sum_p mag |m y_hat|, both legs the sequential fp32 cumsum over the pixels of the model's gradient."""
    c = ref.r64.shape[-1]
    y = np.asarray(prev_y, dtype=F32).reshape(-1, c)
    sc = (np.asarray(gamma, dtype=F32) * np.asarray(rstd, dtype=F32)).astype(F32)
    sh = (np.asarray(beta, dtype=F32) - (np.asarray(mean, dtype=F32) * sc).astype(F32)).astype(F32)
    arg = y.astype(F64) * sc + sh
    m = np.where(arg > 0, 1.0, float(F32(slope)))
    yh32 = ((y - np.asarray(mean, dtype=F32)).astype(F32) * np.asarray(rstd, dtype=F32)).astype(F32)
    yh = (y.astype(F64) - np.asarray(mean, dtype=F64)) * np.asarray(rstd, dtype=F64)
    r, mg, l = ref.r64.reshape(-1, c), ref.mag.reshape(-1, c), ref.leg_trunc.reshape(-1, c)
    g32 = (l * m.astype(F32)).astype(F32)
    c1 = np.cumsum(g32, axis=0, dtype=F32)[-1]
    c2 = np.cumsum((g32 * yh32).astype(F32), axis=0, dtype=F32)[-1]
    return (Ref((r * m).sum(0), (mg * np.abs(m)).sum(0), c1, c1), Ref((r * m * yh).sum(0), (mg * np.abs(m * yh)).sum(0), c2, c2),
            float(np.abs(arg).min()))


def randn_f32(rng, shape, scale=1.0, binades=0):
    """randn as fp32 (NOT bf16-representable); binades b: every element times 2^randint(-b / 2, b / 2)."""
    v = rng.standard_normal(shape) * scale
    if binades:
        v = v * np.exp2(rng.integers(-(binades // 2), binades // 2, size=shape))
    return v.astype(F32)


# ----------------------------------------------------------------------------------------- tier A: mutants the bar must reject
def fwd_mutants(x, w, stride, pad, old=None):
    """Wrong float64 evaluations of conv(x, w) (+ old): name -> output.  'border tap': the outputs of the last column never see
    the tap one column to their left (centre row); 'product (0,1)': the first-order product x_0 w_1 is left out everywhere."""
    x, w = np.asarray(x, dtype=F32), np.asarray(w, dtype=F32)
    k = w.shape[1]
    base = im2col_fwd(x, w, stride, pad)
    add = 0.0 if old is None else np.asarray(old, dtype=F64)
    out = {}
    if k >= 2:
        only = np.zeros_like(w)
        only[:, k // 2, k // 2 - 1] = w[:, k // 2, k // 2 - 1]
        m = base.copy()
        m[:, :, -1] -= im2col_fwd(x, only, stride, pad)[:, :, -1]
        out["border tap"] = m + add
    w2 = w.copy()
    w2[..., -1] = 0
    out["last gathered channel"] = im2col_fwd(x, w2, stride, pad) + add
    if w.shape[0] > 1:
        w3 = w.copy()
        w3[-1] = w[-2]
        out["last produced channel"] = im2col_fwd(x, w3, stride, pad) + add
    if old is not None:
        out["old twice"] = base + 2.0 * add
    out["product (0,1)"] = im2col_fwd(x, w, stride, pad, lambda A, B: x3_exact(A, B, drop=((0, 1),))) + add
    return out


# ------------------------------------------------------------------------- tier B: operands the kernel has no excuse to be off on
# Every term of every output is an integer multiple of one power of two u and mag / u <= 2^23: all partial sums in any order, every
# addend of every matrix instruction and the accumulator fit one 24-bit window, so the only correct fp32 output is r64 itself.
FAMILIES = {"x1w3": (1, 3, 2.0 ** -17, ((0, 0), (0, 1), (0, 2))), "x3w1": (3, 1, 2.0 ** -17, ((0, 0), (1, 0), (2, 0))),
            "x2w2": (2, 2, 2.0 ** -20, ((0, 0), (0, 1), (1, 0), (1, 1)))}      # terms of x, of w, u, the products that are not zero
WINDOW = 2.0 ** 23


def exact_values(rng, shape, terms, density):
    """terms 1: {-1, 0, 1}; 2: +-(1 + m 2^-10), m in {1, 3}; 3: +-(1 + 2^-9 + c 2^-17), c in {1, 3, 5, 7} (2^-9 is below half a bf16
    ulp of 1 and c 2^-17 below half an ulp of 2^-9: three terms each; a NEGATIVE middle term would make the remainder representable
    and leave two) -- zero with probability 1 - density."""
    s = rng.choice([-1.0, 1.0], size=shape)
    if terms == 2:
        s = s * (1.0 + rng.choice([1.0, 3.0], size=shape) * 2.0 ** -10)
    if terms == 3:
        s = s * (1.0 + 2.0 ** -9 + rng.choice([1.0, 3.0, 5.0, 7.0], size=shape) * 2.0 ** -17)
    return (s * (rng.random(shape) < density)).astype(F32)


def exact_pair(seed, family, xshape, wshape, mag_of, k_terms, extra=0.0):
    """(x, w, tries) of one family, the sparse side(s) thinned until max(mag_of(|x|, |w|) + extra) / u <= 2^23.  k_terms: the
    longest sum; the first density aims at a quarter of the window.  A draw that leaves fewer than 5 % of the outputs non-zero (a
    handful of operands, as at a 2 x 2 output) is drawn again at the same density."""
    tx, tw, u, _ = FAMILIES[family]
    k_terms = min(k_terms, float(np.max(mag_of(np.ones(xshape, F32), np.ones(wshape, F32)))))      # the longest sum at THIS shape
    room = WINDOW * u / 4.0
    dens = min(1.0, room / k_terms) if family != "x2w2" else min(1.0, (room / k_terms) ** 0.5)
    for tries in range(200):
        rng = np.random.default_rng([seed, tries])
        x = exact_values(rng, xshape, tx, dens if tx < 3 else 1.0)
        w = exact_values(rng, wshape, tw, dens if tw < 3 else 1.0)
        if float(np.max(mag_of(np.abs(x), np.abs(w)) + extra)) / u > WINDOW:
            dens *= 0.8
        elif (mag_of(x, w) != 0).mean() >= 0.05:
            return x, w, tries
    raise AssertionError("no sparsity fits the window")


def small_ints(rng, shape):
    return rng.integers(-1, 2, size=shape).astype(F32)


def count_terms(v):
    """Number of non-zero split3 terms of every element."""
    return sum((t != 0).astype(np.int64) for t in split3(np.asarray(v, dtype=F32)))


# ------------------------------------------------------------------------------- tile arithmetic of csrc/conv_halo_f32x3.hip
F3_CFG = {1: (0, 4, 1, 2, 32), 2: (0, 2, 2, 4, 32), 3: (0, 2, 2, 2, 32), 4: (0, 4, 2, 4, 32), 5: (1, 2, 2, 4, 32), 6: (1, 2, 2, 2, 32),
          7: (1, 4, 1, 2, 32), 8: (1, 4, 1, 4, 32), 9: (1, 2, 2, 1, 16), 10: (1, 2, 2, 2, 16), 11: (1, 4, 1, 2, 16), 12: (1, 4, 1, 1, 16)}


def f3_tile(cfg):
    """(TH, TW, channels per block) of launch_f3's configuration: TH = WM RPW (32 / TW), 32 WN channels."""
    _, wm, wn, rpw, tw = F3_CFG[cfg]
    return wm * rpw * (32 // tw), tw, 32 * wn


def f3_symbol(cfg, bnin=False):
    ws, wm, wn, rpw, tw = F3_CFG[cfg]
    t = "true" if bnin else "false"
    return ("conv3x3_f32x3_ws_kernel<%d, %d, %d, false, %d, %s>" % (wm, wn, rpw, tw, t)) if ws else ("conv3x3_f32x3_kernel<%d, %d, %d, %s>" % (wm, wn, rpw, t))


def f3_applicable(n, h, w, gathered, produced, up_ca=0):
    """csrc/conv_halo_f32x3.hip::f3_applicable for a 3x3 / stride 1 / pad 1 layer."""
    if gathered % 8 or produced % 4:
        return False
    if up_ca > 0 and (up_ca % 16 or (gathered - up_ca) % 16 or h % 2 or w % 2):
        return False
    return n * h * w * max(gathered, produced) * 4 < 2 ** 31


def n16_steps(gathered):
    """K loop of conv3x3_n16_f32x3_kernel (v_mfma_f32_16x16x32_bf16: two taps of a 16-channel chunk per step) over im2col columns:
    chunk outer, tap pair j inner; group G = 5 chunk + j carries the sign (up_negated_groups(5 chunks))."""
    from oracle.f32x3_ref import up_negated_groups
    nk = cdiv(gathered, 16)
    neg = up_negated_groups(5 * nk)
    return [(np.concatenate([t * gathered + np.arange(16 * c, min(16 * c + 16, gathered)) for t in (2 * j, 2 * j + 1) if t < 9]), 5 * c + j in neg)
            for c in range(nk) for j in range(5)]


def n16_applicable(n, h, w, gathered):
    """csrc/conv_n16_f32x3.hip::n16_applicable for a 3x3 / stride 1 / pad 1 layer producing 16 channels."""
    return gathered % 8 == 0 and 8 <= gathered <= 32 and w >= 16 and n * h * w * 32 * 4 < 2 ** 31


def stem_applicable(n, h, w, ci, co):
    return ci == 4 and co == 64 and h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0


def x3_shared_applicable(ci, co):
    """The shared-source launchers take the split only for > 32 produced channels (forward: co, data gradient: ci; weight
    gradient: co > 32 and channel counts that are multiples of 8)."""
    return co > 32 and ci > 32 and ci % 8 == 0 and co % 8 == 0


def wgrad_up_config(n, h, w, ci, co, up_ca):
    """csrc/conv_wgrad_halo2.hip::h2up_config: 0 refused; 1 / 3: 32-pixel-wide tiles of a (64 / 32 produced channels), 2: 16-pixel."""
    if h % 2 or w % 2 or h < 2 or w < 2 or up_ca <= 0 or up_ca > ci or up_ca % 64 or co % 32 or w // 2 < 16:
        return 0
    if co % 64:
        return 3 if w // 2 >= 32 else 0
    return 1 if w // 2 >= 32 else 2


# ------------------------------------------------------------ the phase kernels (csrc/conv_up_f32x3.hip), in their own K order
UP_CFG = {1: (2, 2, 1, 32), 2: (2, 2, 2, 32), 3: (4, 1, 1, 32), 4: (4, 1, 2, 32), 5: (2, 2, 1, 16), 6: (2, 2, 2, 16), 7: (4, 1, 1, 16),
          8: (2, 2, 4, 32)}           # WM, WN, RPW, TW; 8 is the data gradient's (the forward runs 2 there)


def up_tile(cfg, dgrad):
    """(TH, TW in pixels of a, channels per block, symbol) of launch_up's configuration."""
    wm, wn, rpw, tw = UP_CFG[2 if cfg == 8 and not dgrad else cfg]
    return wm * rpw * (32 // tw), tw, 32 * wn, "conv_up_%s_f32x3_kernel<%d, %d, %d, %d>" % ("dgrad" if dgrad else "fwd", wm, wn, rpw, tw)


def up_applicable(h, w, ci, co, up_ca, dgrad=False):
    """csrc/conv_up_f32x3.hip::up_applicable (h, w: the OUTPUT's extents); the data gradient gathers co in pieces of 8."""
    return not (h % 2 or w % 2 or h < 2 or w < 2 or up_ca <= 0 or up_ca > ci or up_ca % 16 or co % 4 or ci % 4 or (dgrad and co % 8))


def up_fwd_phases(a, w_up, mm):
    """conv3x3(nearest_x2(a), w_up) as the four 2x2 phase convolutions on the oracle's fp32 pre-summed weights: for phase (py, px)
    mm(A [pixels of a][(u, v, channel)], B [(u, v, channel)][co], px) -> [pixels][co].  a NHWC, w_up OHWI."""
    from oracle.f32x3_ref import phase_weights
    a = np.asarray(a, dtype=F32)
    n, h, w, ca = a.shape
    pw = phase_weights(np.ascontiguousarray(np.asarray(w_up, dtype=F32).transpose(0, 3, 1, 2)))      # [py][px][co][ca][u][v]
    co = pw.shape[2]
    y = None
    for py in range(2):
        for px in range(2):
            A, _ = im2col(a, 2, 1, ((1 - py, py), (1 - px, px)))
            out = np.asarray(mm(A, pw[py, px].transpose(2, 3, 1, 0).reshape(4 * ca, co).astype(F64), px))
            if y is None:
                y = np.zeros((n, 2 * h, 2 * w, co), dtype=out.dtype)
            y[:, py::2, px::2] = out.reshape(n, h, w, co)
    return y


def up_fwd_steps(ca, px, signs=True):
    """K loop of conv_up_fwd_f32x3_kernel as one output phase sees it: chunk outer, column offset v (group G = 4 chunk + 2 px + v),
    row offset u inner."""
    from oracle.f32x3_ref import up_negated_groups
    nk = cdiv(ca, 16)
    neg = up_negated_groups(4 * nk) if signs else ()
    return [((u * 2 + v) * ca + np.arange(16 * c, min(16 * c + 16, ca)), 4 * c + 2 * px + v in neg) for c in range(nk) for v in range(2) for u in range(2)]


def up_dgrad_matrices(dy, w_up):
    """The phase data gradient as one product: A [pixels of a][(py, px, u, v, dy channel)] @ B [...][ca]."""
    from oracle.f32x3_ref import phase_weights
    dy = np.asarray(dy, dtype=F64)
    n, h2, w2, co = dy.shape
    h, w = h2 // 2, w2 // 2
    pw = phase_weights(np.ascontiguousarray(np.asarray(w_up, dtype=F32).transpose(0, 3, 1, 2))).astype(F64)
    ca = pw.shape[3]
    cols, rows = [], []
    for py in range(2):
        for px in range(2):
            g = np.pad(dy[:, py::2, px::2], ((0, 0), (1, 1), (1, 1), (0, 0)))
            for u in range(2):
                for v in range(2):
                    di, dj = 1 - py - u, 1 - px - v                      # da[i, j] takes g[i + di, j + dj]
                    cols.append(g[:, 1 + di:1 + di + h, 1 + dj:1 + dj + w].reshape(n * h * w, co))
                    rows.append(pw[py, px, :, :, u, v])                  # [co][ca]
    return np.concatenate(cols, axis=1), np.concatenate(rows, axis=0), (n, h, w, ca)


def up_dgrad_steps(co, signs=True):
    """K loop of conv_up_dgrad_f32x3_kernel: chunk of dy channels outer, phase (group G = 4 chunk + 2 py + px), its four taps inner."""
    from oracle.f32x3_ref import up_negated_groups
    nk = cdiv(co, 16)
    neg = up_negated_groups(4 * nk) if signs else ()
    return [(((2 * py + px) * 4 + t) * co + np.arange(16 * c, min(16 * c + 16, co)), 4 * c + 2 * py + px in neg)
            for c in range(nk) for py in range(2) for px in range(2) for t in range(4)]


def pool2(v):
    """Sum over the 2x2 pixel blocks: the gradient of nearest_x2."""
    v = np.asarray(v)
    return v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]


def x3_up_fwd(a, w_up):
    x = upcat(a, None)
    return Ref(torch_fwd(x, w_up, 1, 1, torch.float64), torch_fwd(np.abs(x), np.abs(w_up), 1, 1, torch.float64), torch_fwd(x, w_up, 1, 1, torch.float32),
               up_fwd_phases(a, w_up, lambda A, B, px: x3_matmul(A, B, up_fwd_steps(np.shape(a)[3], px))))


def x3_up_dgrad(dy, w_up):
    """Gradient of a through conv3x3(nearest_x2(a), w_up): r64 the true operation (transpose convolution, 2x2 sum), the model on the
    phase weights."""
    n, h, w, co = np.shape(dy)
    A, B, shape = up_dgrad_matrices(dy, w_up)
    full32 = torch_dgrad(dy, w_up, 1, 1, h, w, torch.float32)
    rne = (((full32[:, 0::2, 0::2] + full32[:, 0::2, 1::2]).astype(F32) + full32[:, 1::2, 0::2]).astype(F32) + full32[:, 1::2, 1::2]).astype(F32)
    return Ref(pool2(torch_dgrad(dy, w_up, 1, 1, h, w, torch.float64)), pool2(torch_dgrad(np.abs(dy), np.abs(w_up), 1, 1, h, w, torch.float64)), rne,
               x3_matmul(A, B, up_dgrad_steps(co)).reshape(shape))


def wgrad_h2_config(h, w, ci, co, up_ca=0):
    """csrc/conv_wgrad_halo2.hip::h2_config for a 3x3 / stride 1 / pad 1 layer without its two pair-packed 16-channel forms: 0 refused;
    1: 64 x 64 channel blocks, 2: the same on 16-pixel-wide tiles (w < 32), 3: 64 gathered x 32 produced, 4: 32 x 32."""
    cfg = 0
    if ci % 64 == 0 and co % 64 == 0:
        cfg = 2 if w < 32 else 1
    elif ci % 64 == 0 and co % 32 == 0:
        cfg = 3
    elif ci % 32 == 0 and co % 32 == 0:
        cfg = 4
    if cfg == 0 or w < 16 or (cfg != 2 and w < 32):
        return 0
    if up_ca > 0:
        if up_ca >= ci or h % 2 or w % 2:
            return 0
        if up_ca % 64:
            if up_ca % 32 or w < 32:
                return 0
            cfg = 4
    return cfg


def wgrad_pair_config(h, w, ci, co, up_ca=0, pair=7):
    """The two pair-packed forms h2_config tries first (fp32 only; WGRAD_PAIR bits 1 | 2: 16 gathered channels and <= 16 | <= 32
    produced; bit 4: 32 up-sampled channels without a skip half -> 16): 5, 6 or 0."""
    if up_ca == 0 and ci == 16 and 8 <= co <= 32 and co % 8 == 0 and w % 2 == 0 and w >= 16 and pair & (1 if co <= 16 else 2):
        return 5
    if up_ca == 32 and ci == 32 and co == 16 and h % 2 == 0 and w % 2 == 0 and w >= 16 and pair & 4:
        return 6
    return 0


# =================================================================================== the fp32 convolutions on the fp32 matrix pipe
# csrc/conv_small.hip and the non-bf16, non-X3 instances of csrc/conv_igemm.hip and csrc/conv_wgrad.hip
# (tests/test_gpu_conv_f32_grade.py, cases in tests/_conv_f32_cases.py).  Operands are arbitrary fp32 values and enter the matrix
# instruction unrounded.  The second leg of a Ref (stored in ``leg_trunc``, logged as d_mfma) is rne_matmul: an fp32 accumulator to
# which the sum of ``group`` products is added with ONE round-to-nearest per matrix instruction, in im2col order (taps outer,
# channels inner; the pixel axis for the weight gradient).  The K-slices, the split-K partial sums and the order of their atomics are
# not restated: their error is of the same size as one more rounding per slice, far below the margin of 4.
MFMA_32 = 2                               # K terms per v_mfma_f32_32x32x2_f32: conv_igemm_kernel, conv_wgrad_kernel
MFMA_16 = 4                               # K terms per v_mfma_f32_16x16x4_f32: conv3x3_small_kernel, conv3x3_small_wgrad_kernel


class F32Grader(Grader):
    PREFIX, LEG = "f32-grade", "d_mfma"


def rne_matmul(A, B, group):
    """A @ B with an fp32 accumulator: acc = fp32(acc + sum of ``group`` products), the sum formed in float64 (exact to 2^-53 of
    its magnitude for fp32 operands: 'the exact sum'), one round-to-nearest-even per step, in the order of the K axis."""
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    for j in range(0, A.shape[1], group):
        acc = (acc.astype(F64) + A[:, j:j + group] @ B[j:j + group]).astype(F32)
    return acc


def f32_fwd(x, w, stride, pad, group):
    mm = lambda A, B: rne_matmul(A, B, group)  # noqa: E731
    return Ref(torch_fwd(x, w, stride, pad, torch.float64), torch_fwd(np.abs(x), np.abs(w), stride, pad, torch.float64),
               torch_fwd(x, w, stride, pad, torch.float32), im2col_fwd(x, w, stride, pad, mm))


def f32_dgrad(dy, w, stride, pad, hi, wi, group):
    mm = lambda A, B: rne_matmul(A, B, group)  # noqa: E731
    return Ref(torch_dgrad(dy, w, stride, pad, hi, wi, torch.float64), torch_dgrad(np.abs(dy), np.abs(w), stride, pad, hi, wi, torch.float64),
               torch_dgrad(dy, w, stride, pad, hi, wi, torch.float32), im2col_dgrad(dy, w, stride, pad, hi, wi, mm))


def f32_wgrad(x, dy, k, stride, pad, group):
    """K is the pixel axis."""
    mm = lambda A, B: rne_matmul(A, B, group)  # noqa: E731
    return Ref(torch_wgrad(x, dy, k, stride, pad, torch.float64), torch_wgrad(np.abs(x), np.abs(dy), k, stride, pad, torch.float64),
               torch_wgrad(x, dy, k, stride, pad, torch.float32), im2col_wgrad(x, dy, k, stride, pad, mm))


def f32_mutants(x, w, stride, pad, old=None):
    """fwd_mutants plus the two an fp32-pipe kernel could hide behind a 1e-3 bar: the weights rounded to bf16 (a tail path that
    stages one operand in bf16), and the lowest of the three split terms of x never multiplied (a split kernel without its low
    term: about 2^-17 of the magnitude)."""
    out = fwd_mutants(x, w, stride, pad, old)
    add = 0.0 if old is None else np.asarray(old, dtype=F64)
    out["bf16 operand"] = im2col_fwd(x, bf16_round(np.asarray(w, dtype=F32)), stride, pad) + add
    out["low split term"] = im2col_fwd(x, w, stride, pad, lambda A, B: x3_exact(A, B, drop=((2, 0),))) + add
    return out


# -------------------------------------------------------------------------- the launchers' arithmetic, restated (fp32 pipe)
def small_applicable(k, stride, pad, gathered, produced):
    """csrc/conv_small.hip::small_conv_applicable: 3x3 / stride 1 / pad 1 and at most two 16-channel groups in all."""
    return k == 3 and stride == 1 and pad == 1 and cdiv(gathered, 16) * cdiv(produced, 16) <= 2


def small_symbol(gathered, produced, wgrad=False):
    return "conv3x3_small_%skernel<%d, %d>" % ("wgrad_" if wgrad else "", cdiv(gathered, 16), cdiv(produced, 16))


def small_blocks(n, h, w, per_cu):
    """(tiles, blocks) of a small-kernel launch: 16 x 16 pixel tiles, at most 256 x per_cu blocks that loop over them (per_cu: 6 for
    <1, 1> and <1, 2>, 3 for <2, 1>, 2 for the weight gradient)."""
    tiles = n * cdiv(h, 16) * cdiv(w, 16)
    return tiles, min(tiles, 256 * per_cu)


def k_slices(m, produced, taps, plain):
    """csrc/conv_igemm.hip::k_slices: a plain (no bias / activation / residual) single-class fp32 launch with fewer than 384 tiles of
    64 x 64 splits its taps into two slices that add atomically."""
    if not plain or taps < 2:
        return 1
    tiles = cdiv(m, 64) * cdiv(produced, 64)
    if tiles >= 384:
        return 1
    return max(1, min((511 + tiles) // tiles, 2, taps))


IGEMM_TILES = {1: (128, 128, 2, 2), 2: (128, 64, 2, 2), 3: (64, 64, 2, 2), 4: (128, 32, 4, 1)}


def igemm_f32_tile(produced, override=0):
    """launch_igemm's choice on the fp32 pipe: IGEMM_TILE, else 64 x 64 above 32 produced channels and 128 x 32 up to 32."""
    return override if override else (3 if produced > 32 else 4)


def igemm_f32_uniform(gathered, taps, generic, up_ca=0):
    """finish_args for fp32: whole 32-element K tiles per tap, at most 32 taps in all classes together; GENERIC_GATHER does not
    apply to the fused up-sample + concat input (which exists on the uniform loop only)."""
    return not (generic and up_ca == 0) and gathered % 32 == 0 and up_ca % 32 == 0 and taps <= 32


def igemm_f32_symbol(tile, uniform, up=False):
    return "conv_igemm_kernel<%d, %d, %d, %d, false, %s, %s>" % (IGEMM_TILES[tile] + ("true" if uniform else "false", "true" if up else "false"))


def wgrad_f32_tile(produced):
    """conv2d_wgrad_impl on the fp32 pipe: (BMW, BNW, WAVES_M, WAVES_N)."""
    return (64, 64, 2, 2) if produced > 32 else (32, 128, 1, 4)


def wgrad_f32_plan(n, h, w, ci, co, k, stride, pad, blocks=0, generic=False, src_c=None, up=False):
    """(symbol, splits, pixels per split, M) of launch_wgrad<...>(fp32): the gather is row-uniform when the output width is a
    multiple of the 256 / (BNW / 4) rows one load pass covers; a 1x1 / stride 1 / pad 0 layer is rewritten as ONE row of M pixels."""
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    m = n * ho * wo
    bmw, bnw, wm, wn = wgrad_f32_tile(co)
    if k == 1 and stride == 1 and pad == 0 and not up:
        wo = m
    uniform = not generic and wo % (256 // (bnw // 4)) == 0
    tiles = cdiv(co, bmw) * cdiv(k * k * (src_c or ci), bnw)
    splits, kchunk = wgrad_splits(m, tiles, blocks if blocks >= 64 else 3072, 32)
    return "conv_wgrad_kernel<%d, %d, %d, %d, %s>" % (bmw, bnw, wm, wn, "true" if uniform else "false"), splits, kchunk, m


def wgrad_splits(m, tiles, target, ktile, round8=False):
    """The split-K planner of csrc/conv_wgrad.hip: (splits, pixels per split).  round8 (bf16): 16 or more splits over more than one
    tile are rounded to the nearest multiple of 8 that still tiles M, for the XCD-aware block order; some may come out empty."""
    splits = max(1, min(cdiv(target, tiles), cdiv(m, 256), 65535))
    kchunk = cdiv(cdiv(m, splits), ktile) * ktile
    splits = cdiv(m, kchunk)
    if round8 and splits >= 16 and tiles > 1 and splits % 8:
        s8 = (splits + 4) // 8 * 8
        kc = cdiv(cdiv(m, s8), ktile) * ktile
        if kc * (s8 - 8) < m:
            splits, kchunk = s8, kc
    return splits, kchunk


def wgrad_bf16_tile(produced):
    """conv2d_wgrad_impl on bf16 storage: (BMW, BNW, WAVES_M, WAVES_N)."""
    return (128, 64, 2, 2) if produced >= 128 else (64, 64, 2, 2) if produced > 32 else (32, 128, 1, 4)


def _wgrad_geometry(n, h, w, k, stride, pad, up):
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    m = n * ho * wo
    return m, (m if k == 1 and stride == 1 and pad == 0 and not up else wo)


def wgrad_bf16_plan(n, h, w, ci, co, k, stride, pad, blocks=0, generic=False, src_c=None, up=False, no_xcd=False):
    """(symbol, splits, pixels per split, M, XCD-aware order, empty splits) of launch_wgrad<...>(bf16): 64-pixel K-tiles; a load pass
    covers 256 / (BNW / 8) rows; 512 blocks wanted (2048 for the 32-row tile at >= 2^20 pixels) unless WGRAD_BLOCKS >= 64."""
    m, wo = _wgrad_geometry(n, h, w, k, stride, pad, up)
    bmw, bnw, wm, wn = wgrad_bf16_tile(co)
    uniform = not generic and wo % (256 // (bnw // 8)) == 0
    tiles = cdiv(co, bmw) * cdiv(k * k * (src_c or ci), bnw)
    target = blocks if blocks >= 64 else (2048 if bmw == 32 and m >= 1 << 20 else 512)
    splits, kchunk = wgrad_splits(m, tiles, target, 64, round8=True)
    xcd = splits % 8 == 0 and tiles > 1 and not no_xcd
    sym = "conv_wgrad_bf16_kernel<%d, %d, %d, %d, %s>" % (bmw, bnw, wm, wn, "true" if uniform else "false")
    return sym, splits, kchunk, m, xcd, splits - cdiv(m, kchunk)


def wgrad_x3_plan(n, h, w, ci, co, k, stride, pad, blocks=0, generic=False, src_c=None, up=False):
    """(symbol, splits, pixels per split, M) of launch_wgrad<X3, 64, 64, 2, 2>: 32-pixel K-tiles, a 32-row load pass; row-uniform needs
    gathered and produced channels that are multiples of 8 as well; 1024 blocks wanted unless WGRAD_X3_BLOCKS >= 64."""
    m, wo = _wgrad_geometry(n, h, w, k, stride, pad, up)
    g = src_c or ci
    assert co > 32 and g % 8 == 0 and co % 8 == 0, "conv2d_wgrad_impl does not take the split here"
    uniform = not generic and wo % 32 == 0
    splits, kchunk = wgrad_splits(m, cdiv(co, 64) * cdiv(k * k * g, 64), blocks if blocks >= 64 else 1024, 32)
    return "conv_wgrad_x3_kernel<64, 64, 2, 2, %s>" % ("true" if uniform else "false"), splits, kchunk, m


def bn_fold_ref(w, bias, gamma, beta, rm, rv, eps, dt):
    """(w', b', |terms of b'|) of csrc/norm_act.hip::bn_fold_kernel in dtype dt: s = gamma / sqrt(rv + eps), w' = w s,
    b' = beta + (bias - rm) s."""
    g, v = np.asarray(gamma, dtype=dt), np.asarray(rv, dtype=dt)
    s = (g / np.sqrt((v + dt(F32(eps))).astype(dt)).astype(dt)).astype(dt)      # eps reaches the kernel as an fp32 number
    wf = (np.asarray(w, dtype=dt) * s.reshape((-1,) + (1,) * (np.ndim(w) - 1))).astype(dt)
    b0 = np.zeros_like(g) if bias is None else np.asarray(bias, dtype=dt)
    bf = (np.asarray(beta, dtype=dt) + ((b0 - np.asarray(rm, dtype=dt)).astype(dt) * s).astype(dt)).astype(dt)
    mag = np.abs(np.asarray(beta, dtype=F64)) + (np.abs(b0.astype(F64)) + np.abs(np.asarray(rm, dtype=F64))) * np.abs(s.astype(F64))
    return wf, bf, mag
