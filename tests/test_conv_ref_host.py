"""tests/_conv_ref.py proven on the CPU before it judges a kernel (tests/test_gpu_conv_bf16_grade.py): the im2col products against
torch's double-precision convolution and autograd, the truncation on hand-made values, the one-sidedness of the truncating leg,
two negative controls (a truncating bf16 store, a dropped term) that must FAIL the verdicts, and the tile arithmetic of the
launchers that the GPU cases rely on."""
import numpy as np
import pytest
import torch

import _conv_ref as R
from _conv_ref import F32, F64

GEOMS = [(3, 1, 1), (1, 1, 0), (4, 2, 1), (3, 2, 1), (7, 2, 3)]       # k, stride, pad


def operands(k, stride, pad, seed=0, n=2, h=10, w=13, ci=8, co=12, binades=False):
    rng = np.random.default_rng(seed)
    x = R.randn_bf16(rng, (n, h, w, ci), binades=binades)
    wt = R.randn_bf16(rng, (co, k, k, ci), (ci * k * k) ** -0.5, binades=binades)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    dy = R.randn_bf16(rng, (n, ho, wo, co), binades=binades)
    return x, wt, dy


def rel(a, b, mag):
    return float(R.normalised(np.asarray(a, dtype=F64) - np.asarray(b, dtype=F64), mag).max(initial=0.0))


@pytest.mark.parametrize("k,stride,pad", GEOMS)
def test_im2col_products_equal_torch_in_double(k, stride, pad):
    x, wt, dy = operands(k, stride, pad)
    n, h, w, _ = x.shape
    f = R.fwd(x, wt, stride, pad)
    assert f.r64.shape == dy.shape
    assert rel(R.im2col_fwd(x, wt, stride, pad), f.r64, f.mag) <= 1e-12
    assert rel(R.im2col_fwd(np.abs(x), np.abs(wt), stride, pad), f.mag, f.mag) <= 1e-12
    d = R.dgrad(dy, wt, stride, pad, h, w)
    assert d.r64.shape == x.shape
    assert rel(R.im2col_dgrad(dy, wt, stride, pad, h, w), d.r64, d.mag) <= 1e-12
    g = R.wgrad(x, dy, k, stride, pad)
    assert g.r64.shape == wt.shape
    assert rel(R.im2col_wgrad(x, dy, k, stride, pad), g.r64, g.mag) <= 1e-12
    for ref in (f, d, g):                    # both legs are fp32-grade restatements of the same operation
        A, d_rne, d_trunc = R.bar(ref)
        assert d_rne < 1e-6 and d_trunc < 1e-5 and A < 4e-5


def test_fused_decoder_input_is_the_convolution_on_the_materialised_concatenation():
    rng = np.random.default_rng(3)
    a, skip = R.randn_bf16(rng, (2, 3, 4, 16)), R.randn_bf16(rng, (2, 6, 8, 8))
    wt = R.randn_bf16(rng, (8, 3, 3, 24), 24 ** -0.5 / 3)
    cat = R.upcat(a, skip)
    assert cat.shape == (2, 6, 8, 24)
    t = torch.nn.functional.interpolate(torch.from_numpy(a).permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    assert np.array_equal(cat[..., :16], t.permute(0, 2, 3, 1).numpy()) and np.array_equal(cat[..., 16:], skip)
    f = R.fwd_upcat(a, skip, wt)
    assert rel(R.im2col_fwd(cat, wt, 1, 1), f.r64, f.mag) <= 1e-12
    assert R.upcat(a, None).shape == (2, 6, 8, 16)


def test_truncation_toward_minus_infinity_on_hand_made_values():
    t = R.trunc_to_fp32_toward_minus_inf
    one, eps = F32(1.0), 2.0 ** -23
    below = float(np.nextafter(one, F32(0)))             # 1 - 2^-24
    cases = [(0.0, 0.0), (1.0, 1.0), (-1.0, -1.0), (1.5, 1.5), (2.0 ** -130, 2.0 ** -130),        # representable (one subnormal)
             (1.0 + 2.0 ** -40, 1.0), (1.0 - 2.0 ** -40, below),                                   # just above / below, positive
             (-1.0 + 2.0 ** -40, -1.0), (-1.0 - 2.0 ** -40, -(1.0 + eps)),                         # just above / below, negative
             (1.0 + eps - 2.0 ** -50, 1.0), (1.0 + eps + 2.0 ** -50, 1.0 + eps),                   # round-to-nearest would go up
             (2.0 ** -160, 0.0), (-2.0 ** -160, -2.0 ** -149)]                                     # around 0: below the smallest subnormal
    got = t(np.array([c[0] for c in cases]))
    assert got.dtype == F32
    assert np.array_equal(got.astype(F64), np.array([c[1] for c in cases])), list(zip(cases, got))
    assert t(np.float64(1.0 + 2.0 ** -40)).shape == () and float(t(np.float64(-1.0 - 2.0 ** -40))) == -(1.0 + eps)
    rng = np.random.default_rng(0)
    v = rng.standard_normal(10_000) * np.exp2(rng.integers(-20, 20, 10_000))
    y = t(v).astype(F64)
    assert (y <= v).all() and (np.nextafter(t(v), F32(np.inf)).astype(F64) > v).all()


@pytest.mark.parametrize("k,stride,pad", GEOMS)
def test_the_truncating_leg_is_never_above_float64(k, stride, pad):
    x, wt, dy = operands(k, stride, pad, seed=1)
    n, h, w, _ = x.shape
    slack = 2.0 ** -48                       # float64's own rounding of the two different summation orders
    for ref in (R.fwd(x, wt, stride, pad), R.dgrad(dy, wt, stride, pad, h, w), R.wgrad(x, dy, k, stride, pad)):
        assert (ref.leg_trunc.astype(F64) <= ref.r64 + slack * ref.mag).all()
        assert (ref.leg_trunc.astype(F64) < ref.r64).any()       # (short sums of bf16 products are often exact in fp32)


def test_sixteen_terms_or_fewer_are_one_truncation_of_the_float64_sum():
    rng = np.random.default_rng(2)
    for kk in (1, 7, 16):
        A, B = rng.standard_normal((50, kk)), rng.standard_normal((kk, 9))
        assert np.array_equal(R.trunc_matmul(A, B), R.trunc_to_fp32_toward_minus_inf(A @ B))
    A, B = rng.standard_normal((50, 17)), rng.standard_normal((17, 9))
    two = R.trunc_to_fp32_toward_minus_inf(R.trunc_to_fp32_toward_minus_inf(A[:, :16] @ B[:16]).astype(F64) + A[:, 16:] @ B[16:])
    assert np.array_equal(R.trunc_matmul(A, B), two)
    x = R.randn_bf16(rng, (1, 5, 6, 16))
    wt = R.randn_bf16(rng, (8, 1, 1, 16), 0.25)
    f = R.fwd(x, wt, 1, 0)                      # a 1x1 layer of 16 channels: one group
    assert np.array_equal(f.leg_trunc, R.trunc_to_fp32_toward_minus_inf(R.im2col_fwd(x, wt, 1, 0)))


def stock(binades=False):
    """3x3, 512 -> 128 channels: one (tap, channel) term is a fraction of a bf16 half-ulp of the element."""
    rng = np.random.default_rng(7)
    x = R.randn_bf16(rng, (1, 6, 6, 512), binades=binades)
    wt = R.randn_bf16(rng, (128, 3, 3, 512), 4608 ** -0.5, binades=binades)
    return x, wt, R.fwd(x, wt, 1, 1)


def bf16_truncate(v):
    return (np.ascontiguousarray(v, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def test_negative_controls_fail_and_correct_legs_pass():
    x, wt, ref = stock()
    good32 = ref.leg_rne
    assert R.verdict(good32, ref, False)[0] and R.verdict(ref.leg_trunc, ref, False)[0]
    assert R.verdict(R.bf16_round(good32), ref, True)[0] and R.verdict(R.bf16_round(ref.leg_trunc), ref, True)[0]
    # a bf16 store that truncates instead of rounding to nearest
    assert not R.verdict(bf16_truncate(good32), ref, True)[0]
    # a double rounding through an intermediate bf16 sum: acc -> bf16, + old -> bf16
    rng = np.random.default_rng(8)
    old = R.randn_bf16(rng, ref.r64.shape)
    acc = R.epilogue(ref, old=old)
    assert R.verdict(R.bf16_round(acc.leg_rne), acc, True)[0]
    assert not R.verdict(R.bf16_round(R.bf16_round(good32) + old), acc, True)[0]
    # one dropped (tap, channel) term: tap (0, 0), channel 5 never reaches the sum
    x2 = x.copy()
    wt2 = wt.copy()
    wt2[:, 0, 0, 5] = 0
    dropped = R.torch_fwd(x2, wt2, 1, 1, torch.float32)
    assert not R.verdict(dropped, ref, False)[0]
    assert not R.verdict(R.bf16_round(dropped), ref, True)[0]
    # the statistics: correct sums pass, sums of the ROUNDED output fail the sum of squares or the sum
    s1, s2 = R.stats_ref(ref)
    l = ref.leg_rne.reshape(-1, 128).astype(F64)
    assert R.verdict(l.sum(0), s1, False)[0] and R.verdict((l * l).sum(0), s2, False)[0]
    d = dropped.reshape(-1, 128).astype(F64)
    assert not (R.verdict(d.sum(0), s1, False)[0] and R.verdict((d * d).sum(0), s2, False)[0])


def test_the_verdicts_hold_over_twenty_binades_and_at_zero_magnitude():
    x, wt, ref = stock(binades=True)
    assert R.verdict(ref.leg_rne, ref, False)[0] and R.verdict(R.bf16_round(ref.leg_rne), ref, True)[0]
    assert not R.verdict(bf16_truncate(ref.leg_rne), ref, True)[0]
    # an all-zero input block and an all-zero weight row: magnitude 0, and any error at all there is infinite
    rng = np.random.default_rng(9)
    x = R.randn_bf16(rng, (1, 4, 4, 8))
    wt = R.randn_bf16(rng, (8, 3, 3, 8), 0.1)
    wt[2] = 0
    bias = rng.standard_normal(8).astype(F32)
    ref = R.epilogue(R.fwd(x, wt, 1, 1), bias=bias)
    assert (ref.r64[..., 2] == bias[2]).all() and (ref.mag[..., 2] == abs(bias[2])).all()
    z = R.fwd(np.zeros_like(x), wt, 1, 1)
    assert (z.mag == 0).all() and R.verdict(np.zeros(z.r64.shape, F32), z, False)[0]
    wrong = np.zeros(z.r64.shape, F32)
    wrong[0, 1, 1, 3] = 1e-30
    ok, e = R.verdict(wrong, z, False)[:2]
    assert not ok and e == np.inf
    assert not R.verdict(np.full(z.r64.shape, np.nan, F32), z, False)[0]


def test_epilogue_terms_enter_value_and_magnitude():
    x, wt, dy = operands(3, 1, 1, seed=4)
    rng = np.random.default_rng(5)
    base = R.fwd(x, wt, 1, 1)
    bias, res, old = rng.standard_normal(12).astype(F32), R.randn_bf16(rng, base.r64.shape), R.randn_bf16(rng, base.r64.shape)
    e = R.epilogue(base, bias=bias, residual=res, slope=0.0, old=old)
    pre = base.r64 + bias + res
    assert np.array_equal(e.r64, np.maximum(pre, 0.0) + old)
    assert np.array_equal(e.mag, base.mag + np.abs(bias.astype(F64)) + np.abs(res) + np.abs(old))
    assert e.leg_rne.dtype == F32 and R.verdict(e.leg_rne, e, False)[0]
    lk = R.epilogue(base, slope=0.2)
    assert np.allclose(lk.r64, np.where(base.r64 < 0, 0.2 * base.r64, base.r64), rtol=1e-15)


def test_the_shapes_reach_every_launch_regime():
    """Pure Python: the tile arithmetic of csrc/conv_halo_bf16.hip and csrc/conv_igemm.hip that the GPU cases rely on."""
    # TH = WM * RPW * (32 / TW): 8 x 32 pixel tiles for configurations 1, 2, 3, 16 x 16 for 4 and 5, 8 x 16 for 6
    assert [R.halo_tile(c) for c in range(1, 7)] == [(8, 32, 32), (8, 32, 64), (8, 32, 128), (16, 16, 64), (16, 16, 128), (8, 16, 64)]
    # every 3x3 case: one full tile plus a ragged one in each axis, a ragged channel block
    for cfg, (n, h, w, g, p) in [(1, (3, 9, 33, 32, 24)), (2, (3, 9, 33, 64, 72)), (3, (1, 9, 33, 64, 136)), (4, (3, 17, 18, 32, 72)),
                                 (5, (1, 17, 18, 64, 136)), (6, (3, 9, 18, 32, 72))]:
        th, tw, cb = R.halo_tile(cfg)
        assert h // th == 1 and h % th == 1 and w // tw == 1 and 0 < w % tw <= 2 and p % cb != 0, (cfg, n, h, w, g, p)
    assert R.halo_blocks(1, 3, 9, 33, 24) == 12 and R.halo_blocks(2, 3, 9, 33, 72) == 24 and R.halo_blocks(3, 1, 9, 33, 136) == 8
    assert R.halo_blocks(4, 3, 17, 18, 72) == 24 and R.halo_blocks(5, 1, 17, 18, 136) == 8 and R.halo_blocks(6, 3, 9, 18, 72) == 24
    assert R.halo_blocks(6, 2, 16, 16, 64) == 4 and R.halo_blocks(6, 2, 16, 16, 512) == 32        # the long K loop, and its data gradient
    # the XCD remap q = nblk >> 3, r = nblk & 7: counts below 8, multiples of 8, and one above 8 that is no multiple of 8
    assert R.halo_blocks(1, 3, 9, 33, 24) % 8 == 4 and R.halo_blocks(1, 3, 9, 33, 24) > 8
    assert R.halo_blocks(1, 1, 9, 33, 8) == 4
    # no forced configuration may fall back silently: chunks of 32 channels on the gathered side
    assert R.halo_instance(3, 32, 72, cfg=6) == "conv_halo_bf16_kernel<3, 32, 2, 2, 2, 16>"
    assert R.halo_instance(3, 72, 32, cfg=6) == "conv_halo_bf16_kernel<3, 16, 2, 2, 4, 32>"       # falls back: 72 % 32 != 0
    assert R.halo_instance(3, 16, 24) == "conv_halo_bf16_kernel<3, 16, 4, 1, 2, 32>"
    assert R.halo_instance(3, 48, 40) == "conv_halo_bf16_kernel<3, 16, 2, 2, 4, 32>"
    assert R.halo_instance(3, 64, 64, up=(48, 16)) == "conv_halo_bf16_kernel<3, 16, 2, 2, 4, 32>"
    # 4x4 / stride 2: 2x2 window over 4 x the real channels; 8 real channels give 32 virtual ones, 16 give 64
    assert R.halo_instance(4, 32, 64) == "conv_halo_bf16_kernel<2, 32, 2, 2, 4, 32>"
    assert R.halo_instance(4, 64, 72) == "conv_halo_bf16_kernel<2, 64, 2, 4, 4, 32>"
    assert R.halo_instance(4, 256, 136, s2_ck=32) == "conv_halo_bf16_kernel<2, 32, 2, 4, 4, 32>"
    assert R.halo_blocks(2, 2, 9, 33, 64) == 2 * 2 * 2 and R.halo_blocks(2, 1, 9, 33, 16, classes=4) == 16
    # the streamer's 256-pixel flat tiles and the GEMM kernel's 128 / 256-pixel tiles: 259, 63 and 129 pixels are ragged at each
    assert (1 * 7 * 37, 1 * 3 * 43) == (259, 129)
    assert [R.cdiv(259, t) for t in (128, 256)] == [3, 2] and [R.cdiv(129, t) for t in (128, 256)] == [2, 1] and R.cdiv(63, 256) == 1
    assert all(p % t for p in (259, 129, 63) for t in (128, 256))
    assert R.stream_instance(64, 72) == "conv1x1_stream_bf16_kernel<64, 2, 4>" and R.stream_instance(48, 24) == "conv1x1_stream_bf16_kernel<16, 4, 2>"
    # the shared implicit-GEMM source: whole 64-element K tiles per tap and at most 32 taps for the uniform-tap loop
    assert R.igemm_uniform(64, 9, False) and not R.igemm_uniform(64, 9, True) and not R.igemm_uniform(8, 49, False)
    assert not R.igemm_uniform(8, 16, False) and R.igemm_uniform(128, 16, False)
    assert R.igemm_instance(3, True) == "conv_igemm_kernel<64, 64, 2, 2, true, true, false>"
    # the pixel fold: 16 channels fold four pixels while the folded output fits 64 columns, 32 channels fold two, width permitting
    assert R.fold_factor(16, 16, 64) == 4 and R.fold_factor(32, 16, 14) == 2 and R.fold_factor(16, 24, 13) == 1
    assert R.fold_factor(16, 16, 64, no_fold=True) == 1 and R.fold_factor(16, 24, 12) == 1 and R.fold_factor(64, 16, 64) == 1
