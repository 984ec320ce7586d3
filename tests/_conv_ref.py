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
    def __init__(self, tag, log=print):
        self.tag, self.bad, self.log = tag, [], log

    def grade(self, what, got, ref, bf16_out):
        ok, e, A, d_rne, d_trunc, where = verdict(got, ref, bf16_out)
        a_rne = max(MARGIN * d_rne, FLOOR)
        self.log(f"conv-grade {self.tag} | {what} | {'bf16' if bf16_out else 'fp32'} | e {e:.3e} d_rne {d_rne:.3e} d_trunc {d_trunc:.3e} "
                 f"bar {A:.3e} e/bar {e / A:.3f} e/bar_rne {e / a_rne:.3f} at {where}")
        if not ok:
            self.bad.append(f"{what}: e {e:.3e} > bar {A:.3e} at {where}")

    def exact(self, what, got, want):
        same = np.array_equal(np.asarray(got), np.asarray(want))
        self.log(f"conv-grade {self.tag} | {what} | {'exact' if same else 'DIFFERS'}")
        if not same:
            self.bad.append(f"{what}: not bit for bit")

    def note(self, what, ok, text):
        self.log(f"conv-grade {self.tag} | {what} | {text}")
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
