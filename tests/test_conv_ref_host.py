"""tests/_conv_ref.py proven on the CPU before it judges a kernel (tests/test_gpu_conv_bf16_grade.py): the im2col products against
torch's double-precision convolution and autograd, the truncation on hand-made values, the one-sidedness of the truncating leg,
two negative controls (a truncating bf16 store, a dropped term) that must FAIL the verdicts, and the tile arithmetic of the
launchers that the GPU cases rely on.

For the fp32 split kernels (tests/test_gpu_conv_f32x3_grade.py, cases in tests/_conv_f32x3_cases.py): for every case of the GPU file,
tier A's bar rejects five mutants of the float64 model, and tier B's operands are exact (one 24-bit window, the intended split
terms, six-product model == float64, every exercised product and the sign pattern visible in >= 1 % of the outputs)."""
import numpy as np
import pytest
import torch

import _conv_f32x3_cases as C
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


# ================================================================================== the fp32 split kernels: tier A and tier B
def test_six_product_model_on_hand_made_values():
    rng = np.random.default_rng(11)
    A, B = R.randn_f32(rng, (40, 50), binades=20), R.randn_f32(rng, (50, 7), binades=20)
    exact = A.astype(F64) @ B.astype(F64)
    mag = np.abs(A).astype(F64) @ np.abs(B).astype(F64)
    assert rel(R.x3_exact(A, B), exact, mag) <= 2.0 ** -23            # what the three left-out products are worth
    assert rel(R.x3_exact(A, B, drop=((0, 2),)), exact, mag) <= 2.0 ** -15 and rel(R.x3_exact(A, B, drop=((0, 1),)), exact, mag) >= 2.0 ** -12
    plain = R.x3_matmul(A, B)
    assert plain.dtype == F32 and rel(plain, exact, mag) <= 4e-6
    # without a sign pattern the model is never above its own untruncated sum; with every step negated never below
    six = R.x3_exact(A, B)
    every = [(slice(j, j + 16), True) for j in range(0, 50, 16)]
    assert (plain.astype(F64) <= six + 2.0 ** -48 * mag).all() and (R.x3_matmul(A, B, every).astype(F64) >= six - 2.0 ** -48 * mag).all()
    # bf16 operands have one term: one product, the bf16 model
    Ab, Bb = R.bf16_round(A), R.bf16_round(B)
    assert np.array_equal(R.x3_matmul(Ab, Bb), R.trunc_matmul(Ab.astype(F64), Bb.astype(F64)))
    # the K loop of the halo kernels visits every im2col column once, and the groups [q1, q3) are the negated ones
    for g in (8, 16, 24, 72):
        steps = R.halo3_steps(g)
        cols = np.concatenate([c for c, _ in steps])
        assert np.array_equal(np.sort(cols), np.arange(9 * g)) and all(len(c) <= 16 for c, _ in steps)
        assert sum(neg for _, neg in steps) == 3 * len(R.negated_groups(R.cdiv(g, 16))) > 0


def test_f3_tile_table_and_case_lists():
    """The launcher's table (csrc/conv_halo_f32x3.hip::launch_f3) and what the grade needs of the case lists."""
    assert [R.f3_tile(c) for c in range(1, 13)] == [(8, 32, 32), (8, 32, 64), (4, 32, 64), (16, 32, 64), (8, 32, 64), (4, 32, 64), (8, 32, 32),
                                                     (16, 32, 32), (4, 16, 64), (8, 16, 64), (16, 16, 32), (8, 16, 32)]
    assert R.f3_symbol(4) == "conv3x3_f32x3_kernel<4, 2, 4, false>" and R.f3_symbol(12, True) == "conv3x3_f32x3_ws_kernel<4, 1, 1, false, 16, true>"
    for cfg in range(1, 13):
        th, tw, cb = R.f3_tile(cfg)
        mine = [c for c in C.F3_CASES if c[0] == cfg]
        assert {(c[4], c[5]) for c in mine} >= {(8, 4), (72, 68)}
        assert all(c[2] == th + 1 for c in mine) and {c[3] for c in mine} == {tw, tw + 2}
        prod = {c[5] for c in mine}
        assert min(prod) < cb and max(prod) > cb and any(q % cb for q in prod)
    cases = C.F3_CASES + C.F3_BNIN
    refused = [c for c in cases if not R.f3_applicable(*c[1:6])]          # (the data gradient gathers g and produces p like the forward)
    refused += [c for c in C.F3_UP if not R.f3_applicable(c[1], c[2], c[3], c[4] + c[5], c[6], up_ca=c[4])]
    assert 10 * len(refused) <= len(cases) + len(C.F3_UP) and not refused
    assert {c[0] for c in C.F3_BNIN} == {3, 6} and {(c[4], c[5]) for c in C.F3_UP} == {(16, 0), (16, 16), (48, 32)}
    assert sum(c[6] == "binades" for c in C.F3_CASES) == 3


def reject_all(ref, mutants, what):
    assert R.verdict(ref.leg_rne, ref, False)[0] and R.verdict(ref.leg_trunc, ref, False)[0], what
    for name, got in mutants.items():
        ok, e, A = R.verdict(got, ref, False)[:3]
        assert not ok, f"{what}: the bar {A:.3e} lets the mutant '{name}' pass (e {e:.3e})"
    return sorted(mutants)


ALL5 = ["border tap", "last gathered channel", "last produced channel", "old twice", "product (0,1)"]


def one_per_shape(cases):
    """Configurations with the same tile share a case's operands: one host test per distinct shape covers every case."""
    seen = {}
    for c in cases:
        seen.setdefault(C.shape_of(c), c)
    assert sorted(seen, key=repr) == C.unique_shapes(cases)
    return list(seen.values())


F3_A, F3_B = one_per_shape(C.F3_CASES), one_per_shape([c[:6] for c in C.F3_CASES if c[6] == "randn"])


@pytest.mark.parametrize("case", F3_A, ids=[C.f3_id(c) for c in F3_A])
def test_f3_tier_a_bar_rejects_the_mutants(case):
    cfg, n, h, w, g, p, mode = case
    o = C.f3_tier_a(case)
    A = R.bar(o["fwd"])[0]
    assert A <= (4e-5 if mode == "binades" else 8e-6)               # an fp32-grade bar
    old = o["old"]
    assert reject_all(R.epilogue(o["fwd"], old=old), R.fwd_mutants(o["x"], o["wt"], 1, 1, old), "forward") == ALL5
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wd"], 1, 1, h, w)
    assert reject_all(R.epilogue(o["dgrad"], old=old), R.fwd_mutants(d, wf, 1, pads, old), "data gradient") == ALL5
    s1, s2, margin = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], SLOPE_)
    assert margin > 1e-4                                            # no activation argument within rounding distance of zero
    assert R.verdict(s1.leg_rne, s1, False)[0] and R.verdict(s2.leg_rne, s2, False)[0]


SLOPE_ = C.SLOPE


@pytest.mark.parametrize("case", one_per_shape(C.F3_BNIN), ids=[C.f3_id(c) for c in one_per_shape(C.F3_BNIN)])
def test_f3_bnin_tier_a_bar_rejects_the_mutants(case):
    o = C.f3_bnin_a(case)
    m = R.fwd_mutants(o["z"], o["wt"], 1, 1)
    m["transform skipped"] = R.im2col_fwd(o["y_prev"], o["wt"], 1, 1)
    reject_all(o["fwd"], m, "forward behind the in-staging transform")


@pytest.mark.parametrize("case", one_per_shape(C.F3_UP), ids=[C.up_id(c) for c in one_per_shape(C.F3_UP)])
def test_f3_fused_input_tier_a_bar_rejects_the_mutants(case):
    o = C.f3_up_a(case)
    m = R.fwd_mutants(R.upcat(o["a"], o["skip"]), o["wt"], 1, 1)
    shifted = np.roll(R.upcat(o["a"], o["skip"]), 1, axis=2)        # the up-sampled pixel pairs taken one column off
    m["up-sampling off by one column"] = R.im2col_fwd(shifted, o["wt"], 1, 1)
    reject_all(o["fwd"], m, "fused decoder input")


def check_tier_b(t, family, steps, dgrad_to=None, pad=1, stride=1):
    """The four conditions of tier B on one launch's operands."""
    tx, tw, u, pairs = R.FAMILIES[family]
    assert float(t["mag"].max()) / u <= 2.0 ** 23, "window"
    nx, nw = R.count_terms(t["xin"]), R.count_terms(t["w"])
    assert set(np.unique(nx)) <= {0, tx} and set(np.unique(nw)) <= {0, tw} and (nx == tx).any() and (nw == tw).any(), "split terms"
    if dgrad_to is None:
        xx, ww, pp = t["xin"], t["w"], pad
    else:
        xx, ww, pp = R.dgrad_as_forward(t["xin"], t["w"], stride, pad, *dgrad_to)
    six = R.im2col_fwd(xx, ww, 1 if dgrad_to else stride, pp, R.x3_exact)
    assert np.array_equal(six, t["r64"]), "six products != float64"
    assert np.array_equal(t["r64"].astype(F32).astype(F64), t["r64"])
    assert np.array_equal(np.round(t["r64"] / u) * u, t["r64"])
    for pr in pairs:
        m = R.im2col_fwd(xx, ww, 1 if dgrad_to else stride, pp, lambda A, B: R.x3_exact(A, B, drop=(pr,)))
        assert (m != t["r64"]).mean() >= 0.01, f"product {pr} is invisible"
    if steps is not None:
        flip = np.concatenate([c for c, neg in steps if neg][:3])
        m = R.im2col_fwd(xx, ww, 1, pp, lambda A, B: R.x3_exact(A, B, flip=flip))
        assert (m != t["r64"]).mean() >= 0.01, "the sign pattern is invisible"


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("case", F3_B, ids=[C.f3_id(c) for c in F3_B])
def test_f3_tier_b_operands_are_exact(case, family):
    cfg, n, h, w, g, p = case[:6]
    f, d = C.f3_tier_b(case, family)
    check_tier_b(f, family, R.halo3_steps(g))
    check_tier_b(d, family, R.halo3_steps(g), dgrad_to=(h, w))
    assert f["x"].shape == (n, h, w, g) and d["r64"].shape == (n, h, w, p) and np.abs(f["bias"]).max() <= 1 and np.abs(d["old"]).max() <= 1


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_f3_bnin_and_fused_input_tier_b_operands_are_exact(family):
    for case in one_per_shape(C.F3_BNIN):
        check_tier_b(C.f3_bnin_b(case, family), family, R.halo3_steps(case[4]))
    for case in one_per_shape(C.F3_UP):
        t = C.f3_up_b(case, family)
        check_tier_b(t, family, R.halo3_steps(case[4] + case[5]))
        assert np.array_equal(t["xin"], R.upcat(t["a"], t["skip"]))


# ----------------------------------------------------------------- sixteen-wide tile, stem, shared-source split, weight gradients
def test_the_other_launchers_accept_every_listed_case():
    """The predicates' arithmetic, restated: no case of these lists is refused (the cap is one in ten)."""
    assert all(R.n16_applicable(*c) for c in C.N16) and {c[3] for c in C.N16} == {g for g in range(1, 65) if R.n16_applicable(2, 9, 34, g)}
    assert all(R.stem_applicable(n, h, w, 4, 64) for n, h, w in C.STEM)
    assert all(R.x3_shared_applicable(c[3], c[4]) for c in C.X3)
    assert {c[5:] for c in C.X3} == {(3, 2, 1), (1, 2, 0), (4, 2, 1), (3, 1, 1), (1, 1, 0)}
    # conv_wgrad_x3_kernel: the first four cases are generic (output widths 7 and 14), the last four row-uniform unless WGRAD_GENERIC
    xp = R.wgrad_x3_plan
    assert all(xp(*c)[0] == "conv_wgrad_x3_kernel<64, 64, 2, 2, false>" for c in C.X3[:4])
    assert all(xp(*c)[0] == "conv_wgrad_x3_kernel<64, 64, 2, 2, true>" and xp(*c, generic=True)[0].endswith("false>") for c in C.X3[4:])
    assert xp(*C.X3[4])[1:] == (1, 256, 256)                                                 # one split: the plain store
    assert xp(*C.X3[5])[1:] == (2, 256, 480) and 256 % (5 * 32) != 0                          # the first split ends inside image 1
    assert xp(*C.X3[6])[1:] == (2, 160, 288) and C.out_hw(17, 64, 3, 2, 1) == (9, 32) and C.X3[6][6] == 2
    assert C.X3[7][5:] == (1, 1, 0) and C.X3[7][2] % 32 != 0 and xp(*C.X3[7])[3] % 32 == 0       # row-uniform through a.wo = M only
    assert [R.wgrad_up_config(n, h, w, ca + cs, co, ca) for n, h, w, ca, cs, co in C.WG_UP] == [2, 1, 3, 2]
    assert {R.wgrad_h2_config(h, w, ci, co) for n, h, w, ci, co in C.WG_HALO} == {1, 2, 3, 4}       # every channel-block shape
    assert all(R.wgrad_h2_config(h, w, ci, co) for n, h, w, ci, co in C.WG_BNIN + [c[:5] for c in C.WG_SLICE])
    assert [R.wgrad_h2_config(h, w, ca + cs, co, ca) for n, h, w, ca, cs, co in C.WG_HALO_UP] == [1, 4, 2]
    assert all(R.wgrad_pair_config(h, w, ci, co) == 5 for n, h, w, ci, co in C.WG_PAIR) and {c[4] for c in C.WG_PAIR} == {8, 16, 24, 32}
    assert all(R.wgrad_pair_config(h, w, ca + cs, co, ca) == 6 for n, h, w, ca, cs, co in C.WG_PAIR_UP)
    for c in C.WG_PAIR + C.WG_PAIR_UP + C.WG_HALO + C.WG_BNIN + C.WG_HALO_UP + C.WG_UP + [x[:5] for x in C.WG_SLICE]:
        assert 64 <= c[0] * c[1] * c[2] <= 700
    for g in (8, 16, 24, 32):
        steps = R.n16_steps(g)
        assert np.array_equal(np.sort(np.concatenate([c for c, _ in steps])), np.arange(9 * g)) and all(len(c) <= 32 for c, _ in steps)


@pytest.mark.parametrize("case", C.N16, ids=["n%d_%dx%d_g%d" % c for c in C.N16])
def test_n16_tier_a_and_b(case):
    n, h, w, g = case
    o = C.n16_tier_a(case)
    reject_all(o["fwd"], R.fwd_mutants(o["x"], o["wt"], 1, 1), "forward")
    m = R.fwd_mutants(o["z"], o["wt"], 1, 1)
    m["transform skipped"] = R.im2col_fwd(o["x"], o["wt"], 1, 1)
    reject_all(o["fwd_z"], m, "forward behind the transform")
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wd"], 1, 1, h, w)
    reject_all(o["dgrad"], R.fwd_mutants(d, wf, 1, pads), "data gradient")
    assert R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], 0.0)[2] > 1e-4
    for family in sorted(R.FAMILIES):
        f, z, b = C.n16_tier_b(case, family)
        check_tier_b(f, family, R.n16_steps(g))
        check_tier_b(z, family, R.n16_steps(g))
        check_tier_b(b, family, R.n16_steps(g), dgrad_to=(h, w))


@pytest.mark.parametrize("case", C.STEM, ids=["n%d_%dx%d" % c for c in C.STEM])
def test_stem_tier_a_and_b(case):
    o = C.stem_tier_a(case)
    reject_all(o["fwd"], R.fwd_mutants(o["x"], o["wt"], 2, 3), "stem forward")
    for family in sorted(R.FAMILIES):
        check_tier_b(C.stem_tier_b(case, family), family, None, pad=3, stride=2)


def wgrad_mutants(x, dy, k, stride, pad, old):
    """Wrong float64 weight gradients: one pixel (the first of the last image) never summed, the border tap of the last column skipped, the last produced
    channel's gradient taken from the previous dy channel, old added twice, the first-order product dropped."""
    base = R.im2col_wgrad(x, dy, k, stride, pad)
    add = np.asarray(old, dtype=F64)
    x2 = np.array(x, dtype=F32)
    x2[-1, 0, 0] = 0
    dy2 = np.array(dy, dtype=F32)
    dy2[..., -1] = dy2[..., -2]
    dy3 = np.array(dy, dtype=F32)
    dy3[:, :, -1] = 0
    out = {}
    if k > 1:                                # (a 1x1 window has no border tap)
        m = base.copy()
        m[:, k // 2, k // 2 - 1] = R.im2col_wgrad(x, dy3, k, stride, pad)[:, k // 2, k // 2 - 1]
        out["border tap"] = m + add
    out.update({"one pixel": R.im2col_wgrad(x2, dy, k, stride, pad) + add,
            "last produced channel": R.im2col_wgrad(x, dy2, k, stride, pad) + add, "old twice": base + 2.0 * add,
            "product (0,1)": R.im2col_wgrad(x, dy, k, stride, pad, lambda A, B: R.x3_exact(A, B, drop=((1, 0),))) + add})
    return out


def check_wgrad_tier_b(t, family):
    tx, tw, u, pairs = R.FAMILIES[family]
    k, s, p = t["geom"]
    assert float(t["mag"].max()) / u <= 2.0 ** 23
    nx, nw = R.count_terms(t["xin"]), R.count_terms(t["w"])
    assert set(np.unique(nx)) <= {0, tx} and set(np.unique(nw)) <= {0, tw} and (nx == tx).any() and (nw == tw).any()
    assert np.array_equal(R.im2col_wgrad(t["xin"], t["w"], k, s, p, R.x3_exact), t["r64"])
    assert np.array_equal(t["r64"].astype(F32).astype(F64), t["r64"])
    for i, j in pairs:                       # the matrix product is dy^T @ im2col(x): (term of dy, term of x)
        m = R.im2col_wgrad(t["xin"], t["w"], k, s, p, lambda A, B: R.x3_exact(A, B, drop=((j, i),)))
        assert (m != t["r64"]).mean() >= 0.01, f"product {(i, j)} is invisible"


@pytest.mark.parametrize("case", C.X3, ids=["n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c for c in C.X3])
def test_shared_source_split_tier_a_and_b(case):
    n, h, w, ci, co, k, s, p = case
    o = C.x3_tier_a(case)
    m = R.fwd_mutants(o["x"], o["wt"], s, p)
    if k == 1:
        assert "border tap" not in m
    reject_all(o["fwd"], m, "forward")
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wt"], s, p, h, w)
    md = R.fwd_mutants(d, wf, 1, pads)
    md.pop("border tap", None)               # (the dilated dy of a strided layer has zero columns: that mutant may change nothing)
    reject_all(o["dgrad"], md, "data gradient")
    reject_all(R.epilogue(o["wgrad"], old=o["oldw"]), wgrad_mutants(o["x"], o["dy"], k, s, p, o["oldw"]), "weight gradient")
    for family in sorted(R.FAMILIES):
        f, b, g = C.x3_tier_b(case, family)
        check_tier_b(f, family, None, pad=p, stride=s)
        check_tier_b(b, family, None, dgrad_to=(h, w), pad=p, stride=s)
        check_wgrad_tier_b(g, family)


WG_ALL = [("halo", c) for c in C.WG_HALO + C.WG_PAIR] + [("halo_up", c) for c in C.WG_PAIR_UP] + [("halo_up", c) for c in C.WG_HALO_UP] + [("bnin", c) for c in C.WG_BNIN] + \
         [("up", c) for c in C.WG_UP] + [("halo", c[:5]) for c in C.WG_SLICE]


@pytest.mark.parametrize("kind,case", WG_ALL, ids=["%s-%s" % (k, "_".join(map(str, c))) for k, c in WG_ALL])
def test_weight_gradient_tier_a_and_b(kind, case):
    o = C.wg_tier_a(kind, case)
    reject_all(R.epilogue(o["wgrad"], old=o["oldw"]), wgrad_mutants(o["x"], o["dy"], 3, 1, 1, o["oldw"]), "weight gradient")
    for family in sorted(R.FAMILIES):
        check_wgrad_tier_b(C.wg_tier_b(kind, case, family), family)


# ------------------------------------------------------------------------------------------------------------ the phase kernels
UP_ONE = one_per_shape(C.UP)


def test_phase_kernel_tiles_and_cases():
    assert [R.up_tile(c, True)[:3] for c in range(1, 9)] == [(2, 32, 64), (4, 32, 64), (4, 32, 32), (8, 32, 32), (4, 16, 64), (8, 16, 64), (8, 16, 32),
                                                              (8, 32, 64)]
    assert R.up_tile(8, False) == R.up_tile(2, False) and R.up_tile(7, False)[3] == "conv_up_fwd_f32x3_kernel<4, 1, 1, 16>"
    refused = [c for c in C.UP if not R.up_applicable(c[2], c[3], c[4] + c[5], c[6], c[4], dgrad=True)]
    assert not refused
    for cfg in range(1, 9):
        mine = [c for c in C.UP if c[0] == cfg]
        th, tw = R.up_tile(cfg, True)[:2]
        assert {(c[2], c[3]) for c in mine} == {(2, 2), (2 * th + 2, 2 * tw + 2)}
        assert {c[4] for c in mine} == {16, 48} and {c[5] for c in mine} == {0, 16} and {c[6] for c in mine} == {8, 40}
    # the phase form IS the convolution on the up-sampled tensor, and its K loops visit every column once
    rng = np.random.default_rng(4)
    a, w = R.randn_f32(rng, (2, 3, 5, 16)), R.randn_f32(rng, (8, 3, 3, 16), 0.1)
    f = R.x3_up_fwd(a, w)
    assert rel(R.up_fwd_phases(a, w, lambda A, B, px: A @ B), f.r64, f.mag) <= 1e-6          # (the pre-sums are rounded to fp32)
    dy = R.randn_f32(rng, (2, 6, 10, 8))
    g = R.x3_up_dgrad(dy, w)
    A, B, shape = R.up_dgrad_matrices(dy, w)
    assert rel((A @ B).reshape(shape), g.r64, g.mag) <= 1e-6 and g.r64.shape == a.shape
    assert np.array_equal(np.sort(np.concatenate([c for c, _ in R.up_dgrad_steps(8)])), np.arange(16 * 8))
    assert np.array_equal(np.sort(np.concatenate([c for c, _ in R.up_fwd_steps(48, 1)])), np.arange(4 * 48))


@pytest.mark.parametrize("case", UP_ONE, ids=[C.up_id(c) for c in UP_ONE])
def test_phase_kernels_tier_a_and_b(case):
    cfg, n, h, w, ca, cs, co = case
    o = C.up_tier_a(case)
    w_up = np.ascontiguousarray(o["wt"][..., :ca])
    m = R.fwd_mutants(R.upcat(o["a"], None), w_up, 1, 1, o["old"])
    m["up-sampling off by one column"] = R.im2col_fwd(np.roll(R.upcat(o["a"], None), 1, axis=2), w_up, 1, 1) + o["old"]
    if w == 2:
        m.pop("up-sampling off by one column")          # (a has one column: the roll is the identity)
    reject_all(R.epilogue(o["fwd"], old=o["old"]), m, "phase forward")
    dg = R.epilogue(o["dgrad"], old=o["olda"])
    d, wf, pads = R.dgrad_as_forward(o["dy"], w_up, 1, 1, h, w)
    md = {k: R.pool2(v) + o["olda"] for k, v in R.fwd_mutants(d, wf, 1, pads).items()}
    md["old twice"] = dg.r64 + o["olda"]
    md["2x2 sum misses a pixel"] = dg.r64 - R.im2col_fwd(d, wf, 1, pads)[:, 1::2, 1::2]
    if w == 2:
        md.pop("border tap")
    reject_all(dg, md, "phase data gradient")
    from oracle.f32x3_ref import UP_TAPS, phase_weights
    for family in sorted(R.FAMILIES):
        f, b = C.up_tier_b(case, family)
        tx, tw_, u, pairs = R.FAMILIES[family]
        for t in (f, b):
            assert float(t["mag"].max()) / u <= 2.0 ** 23
            # the packer's fp32 pre-sums of up to four weights lose nothing: every phase weight equals its float64 sum
            pw = phase_weights(np.ascontiguousarray(t["w"].transpose(0, 3, 1, 2)))
            w64 = t["w"].astype(F64).transpose(0, 3, 1, 2)
            for (py, u), kys in UP_TAPS.items():
                for (px, v), kxs in UP_TAPS.items():
                    assert np.array_equal(pw[py, px, :, :, u, v].astype(F64), sum(w64[:, :, ky, kx] for ky in kys for kx in kxs))
            assert set(np.unique(R.count_terms(t["xin"]))) <= {0, tx} and set(np.unique(R.count_terms(t["w"]))) <= {0, tw_}
        assert np.array_equal(R.up_fwd_phases(f["a"], f["w"], lambda A, B, px: R.x3_exact(A, B)), f["r64"]), "phase six products != float64"
        A, B, shape = R.up_dgrad_matrices(b["x"], b["w"])
        assert np.array_equal(R.x3_exact(A, B).reshape(shape), b["r64"])
        for pr in pairs:
            mf = R.up_fwd_phases(f["a"], f["w"], lambda A_, B_, px: R.x3_exact(A_, B_, drop=(pr,)))
            assert (mf != f["r64"]).mean() >= 0.01 and (R.x3_exact(A, B, drop=(pr,)).reshape(shape) != b["r64"]).mean() >= 0.01, pr
        flip = lambda steps: np.concatenate([c for c, neg in steps if neg][:2])  # noqa: E731
        mf = R.up_fwd_phases(f["a"], f["w"], lambda A_, B_, px: R.x3_exact(A_, B_, flip=flip(R.up_fwd_steps(ca, px))))
        assert (mf != f["r64"]).mean() >= 0.01
        # one mis-signed group shows (at the 2 x 2 output most taps of a group fall outside a: some group, not each)
        negs = [c for c, neg in R.up_dgrad_steps(co) if neg]
        assert any((R.x3_exact(A, B, flip=np.concatenate(negs[i:i + 4])).reshape(shape) != b["r64"]).mean() >= 0.01 for i in range(0, len(negs), 4))


# =========================================================== the fp32-pipe kernels (tests/test_gpu_conv_f32_grade.py, _conv_f32_cases.py)
import _conv_f32_cases as C32  # noqa: E402


def test_rne_matmul_on_hand_made_values():
    h = 2.0 ** -24                                   # half an ulp of 1
    ones = np.ones((3, 1))
    # 1, h, h: one product per step both halves are ties that round to even (1); two per step the same; all in one step: exact
    assert R.rne_matmul([[1.0, h, h]], ones, 1)[0, 0] == 1.0 and R.rne_matmul([[1.0, h, h]], ones, 2)[0, 0] == 1.0
    assert R.rne_matmul([[1.0, h, h]], ones, 4)[0, 0] == F32(1.0 + 2 * h)
    # the small terms first: their exact sum 2h enters in one rounding
    assert R.rne_matmul([[h, h, 1.0]], ones, 2)[0, 0] == F32(1.0 + 2 * h) and R.rne_matmul([[h, 1.0, h]], ones, 2)[0, 0] == 1.0
    # a tie above an odd mantissa rounds UP to the even neighbour; the products themselves are never rounded
    assert R.rne_matmul([[1.0 + 2 * h, h]], np.ones((2, 1)), 1)[0, 0] == F32(1.0 + 4 * h)
    a = float(F32(1.0 + 2 * h))
    assert R.rne_matmul([[a, -1.0]], [[a], [1.0 + 4 * h]], 2)[0, 0] == F32(a * a - (1.0 + 4 * h)) == F32(4 * h * h)
    rng = np.random.default_rng(21)
    A, B = R.randn_f32(rng, (30, 37), binades=12), R.randn_f32(rng, (37, 5), binades=12)
    ex, mag = A.astype(F64) @ B.astype(F64), np.abs(A).astype(F64) @ np.abs(B).astype(F64)
    for g in (R.MFMA_32, R.MFMA_16):
        got = R.rne_matmul(A, B, g)
        assert got.dtype == F32 and rel(got, ex, mag) <= R.cdiv(37, g) * 2.0 ** -24
    assert np.array_equal(R.rne_matmul(A, B, 64), ex.astype(F32))
    assert not np.array_equal(R.rne_matmul(A, B, 2), R.rne_matmul(A, B, 4))              # the group is part of the model


def parity_classes(h, w, k, s, p):
    """(rows, columns, taps) of every parity class of a data gradient, as conv2d_dgrad_impl builds them."""
    out = []
    for ph in range(s):
        for pw in range(s):
            taps = sum((ph + p - r) % s == 0 for r in range(k)) * sum((pw + p - q) % s == 0 for q in range(k))
            out.append(((h - ph + s - 1) // s, (w - pw + s - 1) // s, taps))
    return out


def test_the_f32_shapes_reach_every_launch_regime():
    """small_conv_applicable, k_slices, the tile choice and the uniform / row_uniform conditions, restated in _conv_ref: every case of
    _conv_f32_cases reaches the regime its comment claims."""
    cd = R.cdiv
    assert {c[5:] for c in C32.IG} == {(3, 1, 1), (3, 2, 1), (1, 2, 0), (4, 2, 1), (7, 2, 3), (5, 2, 2)}
    for c in C32.IG:
        n, h, w, ci, co, k, s, p = c
        ho, wo = C32.out_hw(h, w, k, s, p)
        m = n * ho * wo
        assert not R.small_applicable(k, s, p, ci, co) and not R.small_applicable(k, s, p, co, ci)
        assert R.k_slices(m, co, k * k, True) == (1 if k == 1 else 2) and R.k_slices(m, co, k * k, False) == 1       # plain: sliced atomics
        assert m <= 128 * 192 and (s == 1 or k == 1 or sum(t for _, _, t in parity_classes(h, w, k, s, p)) == k * k)
    # IG[0]: a full and a ragged row tile, a full and a ragged column tile at EVERY tile: fast and generic epilogue in one launch
    n, h, w, ci, co = C32.IG[0][:5]
    for bm, bn, _, _ in R.IGEMM_TILES.values():
        assert (n * h * w) // bm >= 1 and (n * h * w) % bm and co // bn >= 1 and co % bn
    # the two gather loops: ci = 32 switches with GENERIC_GATHER, ci = 40 and the 49-tap stem are generic whatever the switch
    assert R.igemm_f32_uniform(32, 9, False) and not R.igemm_f32_uniform(32, 9, True) and not R.igemm_f32_uniform(40, 9, False)
    assert R.igemm_f32_uniform(64, 9, False) and not R.igemm_f32_uniform(136, 9, False)          # the data gradients of IG[1], IG[0]
    assert not R.igemm_f32_uniform(4, 49, False) and not R.igemm_f32_uniform(64, 49, False) and R.igemm_f32_uniform(32, 25, False)
    assert R.igemm_f32_uniform(64, 1, False) and R.igemm_f32_uniform(32, 16, False)
    assert any(c[4] % 32 for c in C32.IG) and any(c[4] <= 32 for c in C32.IG) and any(c[3] == 4 for c in C32.IG)
    assert R.igemm_f32_tile(24) == 4 and R.igemm_f32_tile(40) == 3 and R.igemm_f32_tile(24, 1) == 1
    assert R.igemm_f32_symbol(4, False) == "conv_igemm_kernel<128, 32, 4, 1, false, false, false>"
    assert R.igemm_f32_symbol(1, True, up=True) == "conv_igemm_kernel<128, 128, 2, 2, false, true, true>"
    # odd extents under stride 2: the parity classes differ in rows and columns; 1x1/2: one class has the tap, three are empty
    assert len({(r, q) for r, q, _ in parity_classes(11, 17, 3, 2, 1)}) == 4 and len({(r, q) for r, q, _ in parity_classes(9, 13, 5, 2, 2)}) == 4
    assert sorted(t for _, _, t in parity_classes(11, 17, 1, 2, 0)) == [0, 0, 0, 1]
    # the unsliced plain store: >= 384 tiles of 64 x 64, whole tiles of the forced shape (the fast epilogue everywhere), uniform loop
    for tile, (n, h, w, ci, co) in C32.LARGE.items():
        bm, bn = R.IGEMM_TILES[tile][:2]
        m = n * h * w
        assert cd(m, 64) * cd(co, 64) >= 384 and R.k_slices(m, co, 9, True) == 1 and m % bm == 0 and co % bn == 0
        assert R.igemm_f32_uniform(ci, 9, False) and not R.small_applicable(3, 1, 1, ci, co) and m * max(ci, co) <= 128 * 192 * 64
    # conv2d_dgrad_bnreduce_ok, restated: heuristic tile, no K-slices, whole tiles (64 x 64 above 32 produced channels, else 128 x 32)
    for n, h, w, ci, co in C32.BNR:
        m = n * h * w
        assert not R.small_applicable(3, 1, 1, co, ci) and R.k_slices(m, ci, 9, True) == 1 and R.igemm_f32_uniform(co, 9, False)
        assert (m % 64 == 0 and ci % 64 == 0) if ci > 32 else (m % 128 == 0 and ci % 32 == 0)
    assert {R.igemm_f32_tile(c[3]) for c in C32.BNR} == {3, 4}
    n, h, w, ci, co, split = C32.SPLIT
    assert all(split % bn == 0 for _, bn, _, _ in R.IGEMM_TILES.values()) and 0 < split < ci and R.k_slices(n * h * w, ci, 9, True) == 2
    assert not R.small_applicable(3, 1, 1, co, ci) and R.igemm_f32_uniform(co, 9, False) and not R.igemm_f32_uniform(co, 9, True)
    for n, h, w, ca, cs, co in C32.UPCAT:
        assert R.igemm_f32_uniform(ca + cs, 9, True, up_ca=ca) and not R.small_applicable(3, 1, 1, ca + cs, co) and h % 2 == 0 and w % 2 == 0
    assert {c[4] for c in C32.UPCAT} == {0, 32}
    # the small kernels: all three instantiations in both directions, partial tiles, a partial K group, one-pixel width, and both block regimes
    assert {R.small_symbol(g, p) for _, _, _, g, p in C32.SM} == {"conv3x3_small_kernel<%s>" % t for t in ("1, 1", "2, 1", "1, 2")}
    assert R.small_symbol(8, 24, wgrad=True) == "conv3x3_small_wgrad_kernel<1, 2>"
    for n, h, w, g, p in C32.SM:
        assert R.small_applicable(3, 1, 1, g, p) and R.small_applicable(3, 1, 1, p, g)
    assert any(g == 8 for _, _, _, g, _ in C32.SM) and any(p == 24 for *_, p in C32.SM) and any(w == 1 for _, _, w, _, _ in C32.SM)
    assert any(h % 16 and w % 16 and h > 16 and w > 16 and C32.sm_up(c) for c in C32.SM for _, h, w, _, _ in [c])
    for sym, per_cu in (("1, 1", 6), ("1, 2", 6), ("2, 1", 3)):
        mine = [R.small_blocks(n, h, w, per_cu) for n, h, w, g, p in C32.SM if R.small_symbol(g, p).endswith("<%s>" % sym)]
        assert any(t > b for t, b in mine) and any(t == b and t < 256 for t, b in mine), sym          # several tiles per block; fewer tiles than blocks
    assert all(R.small_blocks(n, h, w, 2)[0] > R.small_blocks(n, h, w, 2)[1] == 512 for n, h, w, _, _ in C32.SM[9:])      # the weight gradient's 512 blocks
    # conv_wgrad_kernel: both tiles under both gathers, one split / many splits / a split ending inside an image, the 1x1 rewrite
    plan = R.wgrad_f32_plan
    for case, blocks in C32.WG:
        assert not R.small_applicable(case[5], case[6], case[7], case[3], case[4])
        assert plan(*case, generic=True)[0].endswith("false>")
    syms = {plan(*case, blocks=b, generic=g)[0] for case, bl in C32.WG for b in bl for g in (False, True)}
    assert syms == {"conv_wgrad_kernel<64, 64, 2, 2, %s>" % u for u in ("true", "false")} | {"conv_wgrad_kernel<32, 128, 1, 4, %s>" % u for u in ("true", "false")}
    big = C32.WG[0][0]
    assert [plan(*big, blocks=b)[1:] for b in (0, 64, 4096)] == [(12, 256, 3072), (6, 512, 3072), (12, 256, 3072)]
    assert plan(*C32.WG[2][0])[1] == 1 and plan(*C32.WG[3][0])[1] == 1 and plan(*C32.WG[1][0])[1] == 12
    sp, chunk, m = plan(*C32.WG[4][0])[1:]
    assert (sp, chunk, m) == (2, 256, 480) and chunk % (10 * 16) != 0                       # the first split ends inside the second image
    assert plan(*C32.WG[5][0])[0].endswith("true>") and plan(*C32.WG[6][0])[0].endswith("false>") and C32.WG[5][0][5:] == (7, 2, 3)
    assert plan(*C32.WG[7][0])[0] == "conv_wgrad_kernel<64, 64, 2, 2, true>" and C32.WG[7][0][2] % 16 != 0      # row-uniform through a.wo = M only
    assert plan(*C32.WG[8][0])[0] == "conv_wgrad_kernel<32, 128, 1, 4, true>" and plan(*C32.WG[9][0])[0].endswith("true>") and C32.WG[9][0][6] == 2
    for n, h, w, ca, cs, co in C32.WG_PART:
        geom = (n, h, w, ca + cs, co, 3, 1, 1)
        assert plan(*geom, src_c=ca, up=True)[0].endswith("true>") and plan(*geom, src_c=cs)[0].endswith("true>") and ca % 4 == 0 and cs % 4 == 0
    assert {R.wgrad_f32_tile(c[5])[0] for c in C32.WG_PART} == {64, 32}
    # the same halves on conv_wgrad_x3_kernel: both row-uniform (a 32-pixel-wide output), generic under WGRAD_GENERIC
    for n, h, w, ca, cs, co in C32.WG_PART_X3:
        geom = (n, h, w, ca + cs, co, 3, 1, 1)
        for kw in (dict(src_c=ca, up=True), dict(src_c=cs)):
            assert R.wgrad_x3_plan(*geom, **kw)[0].endswith("true>") and R.wgrad_x3_plan(*geom, generic=True, **kw)[0].endswith("false>")
    assert C32.WG_PART_X3 == C32.WG_PART[:1]


ALL7 = sorted(ALL5 + ["bf16 operand", "low split term"])
# What tier A can and cannot see of a dropped low split term: it perturbs every product by at most 2^-17 of itself with a random sign,
# so over K products the worst element of the output is off by about 4 x 2^-18 / sqrt(K) of its magnitude -- about 1e-6 at K = 256, the
# size of the bar, and BELOW the rounding noise of any correct fp32 accumulation beyond that (measured on the float64 mutant: 1.0e-6
# at K = 288, 3e-7 at K = 3072).  Tier A must reject it wherever the longest sum has at most LOW_TERM_K products; at every K tier B
# catches it exactly: check_tier_b / check_wgrad_tier_b prove that product (2, 0) alone changes >= 1 % of the outputs bit for bit.
LOW_TERM_K = 256


def f32_expect(mutants, k_terms):
    if k_terms > LOW_TERM_K:
        mutants.pop("low split term")
    return mutants
F32_BAR = 2e-6                            # "an fp32-grade bar": both legs are a few 1e-7, x 4


@pytest.mark.parametrize("case", C32.IG, ids=[C32.ig_id(c) for c in C32.IG])
def test_f32_igemm_tier_a_and_b(case):
    n, h, w, ci, co, k, s, p = case
    o = C32.ig_tier_a(case)
    A, d_rne, d_mfma = R.bar(o["fwd"])
    wide = 2.0 if case in C32.IG_BINADES else 1.0          # (over 12 binades single terms dominate some elements: the legs' worst element is worse)
    assert R.FLOOR <= A <= wide * F32_BAR and 0 < d_rne < wide * 5e-7 and 0 < d_mfma < wide * 5e-7
    got = reject_all(R.epilogue(o["fwd"], old=o["old"]), f32_expect(R.f32_mutants(o["x"], o["wt"], s, p, o["old"]), k * k * ci), "forward")
    assert got == [m for m in ALL7 if (k > 1 or m != "border tap") and (k * k * ci <= LOW_TERM_K or m != "low split term")]
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wt"], s, p, h, w)
    md = f32_expect(R.f32_mutants(d, wf, 1, pads, o["oldx"]), max(t for _, _, t in parity_classes(h, w, k, s, p)) * co)
    if s > 1:
        md.pop("border tap", None)           # (the dilated dy of a strided layer has zero columns: that mutant may change nothing)
    reject_all(R.epilogue(o["dgrad"], old=o["oldx"]), md, "data gradient")
    s1, s2 = R.stats_ref(o["fwd"])
    l = o["fwd"].leg_rne.reshape(-1, co).astype(F64)
    assert R.verdict(l.sum(0), s1, False)[0] and R.verdict((l * l).sum(0), s2, False)[0]
    for family in C32.FAMILIES:
        f, b = C32.ig_tier_b(case, family)
        check_tier_b(f, family, None, pad=p, stride=s)
        check_tier_b(b, family, None, dgrad_to=(h, w), pad=p, stride=s)
        assert np.abs(f["bias"]).max() <= 1 and np.abs(f["res"]).max() <= 1 and f["res"].shape == f["r64"].shape
    f = C32.ig_tier_b(case, "x3w1")[0]         # a bf16-rounded x shows in tier B as well
    assert (R.im2col_fwd(R.bf16_round(f["x"]), f["w"], s, p) != f["r64"]).mean() >= 0.01


def test_f32_other_igemm_cases_tier_a_and_b():
    """The unsliced shape of tile 4 (the smallest of LARGE), the split and the fused decoder input."""
    shape = C32.LARGE[4]
    o = C32.large_tier_a(shape)
    assert R.bar(o["fwd"])[0] <= F32_BAR
    assert reject_all(o["fwd"], f32_expect(R.f32_mutants(o["x"], o["wt"], 1, 1), 9 * shape[3]), "unsliced forward") == [m for m in ALL7 if m not in ("old twice", "low split term")]
    n, h, w, ci, co, split = C32.SPLIT
    o = C32.split_tier_a()
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wt"], 1, 1, h, w)
    m = f32_expect(R.f32_mutants(d, wf, 1, pads), 9 * co)
    swapped = R.im2col_fwd(d, wf, 1, pads)
    m["halves swapped"] = np.concatenate([swapped[..., ci - split:], swapped[..., :ci - split]], axis=3)
    reject_all(o["dgrad"], m, "split data gradient")
    for case in C32.UPCAT:
        o = C32.upcat_tier_a(case)
        cat = R.upcat(o["a"], o["skip"])
        m = f32_expect(R.f32_mutants(cat, o["wt"], 1, 1), 9 * cat.shape[3])
        m["up-sampling off by one column"] = R.im2col_fwd(np.roll(cat, 1, axis=2), o["wt"], 1, 1)
        reject_all(o["fwd"], m, "fused decoder input")
    for family in C32.FAMILIES:
        t = C32.large_tier_b(shape, family)       # (the window and the representability; the per-product proofs run at the small shapes)
        assert float(t["mag"].max()) / R.FAMILIES[family][2] <= 2.0 ** 23 and np.array_equal(t["r64"].astype(F32).astype(F64), t["r64"])
        assert (t["r64"] != 0).mean() >= 0.05
        check_tier_b(C32.split_tier_b(family), family, None, dgrad_to=(h, w))
        for case in C32.UPCAT:
            t = C32.upcat_tier_b(case, family)
            check_tier_b(t, family, None)
            assert np.array_equal(t["xin"], R.upcat(t["a"], t["skip"]))
    for case in C32.BNR:
        assert case[0] * case[1] * case[2] * max(case[3:]) <= 128 * 192 * 64
    o = C32.bnr_tier_a(C32.BNR[1])
    s1, s2, margin = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], SLOPE_)
    assert margin > 1e-4 and R.verdict(s1.leg_rne, s1, False)[0] and R.verdict(s2.leg_rne, s2, False)[0]


def f32_wgrad_mutants(x, dy, k, s, p, old):
    m = wgrad_mutants(x, dy, k, s, p, old)
    add = np.asarray(old, dtype=F64)
    m["bf16 operand"] = R.im2col_wgrad(x, R.bf16_round(np.asarray(dy, dtype=F32)), k, s, p) + add
    m["low split term"] = R.im2col_wgrad(x, dy, k, s, p, lambda A, B: R.x3_exact(A, B, drop=((2, 0),))) + add
    return m


SM_HOST = [C32.SM[0], C32.SM[1], C32.SM[3], C32.SM[7]]      # <1, 1>, <1, 2> over 12 binades, <2, 1>, one pixel wide (the many-tile shapes draw
                                                            # from the same generators; what they add is the block loop, proven above)


@pytest.mark.parametrize("case", SM_HOST, ids=[C32.sm_id(c) for c in SM_HOST])
def test_f32_small_tier_a_and_b(case):
    n, h, w, g, p = case
    o = C32.sm_tier_a(case)
    wide = 2.0 if case in C32.SM_BINADES else 1.0
    assert R.bar(o["fwd"])[0] <= wide * F32_BAR and R.bar(o["wgrad"])[0] <= wide * F32_BAR
    m = f32_expect(R.f32_mutants(o["x"], o["wt"], 1, 1, o["old"]), 9 * g)
    d, wf, pads = R.dgrad_as_forward(o["dy"], o["wd"], 1, 1, h, w)
    md = f32_expect(R.f32_mutants(d, wf, 1, pads, o["old"]), 9 * g)
    mw = f32_expect(f32_wgrad_mutants(o["x"], o["dyw"], 3, 1, 1, o["oldw"]), n * h * w)
    if w == 1:                               # (the tap one column to the left of the only column reads padding)
        m.pop("border tap"), md.pop("border tap"), mw.pop("border tap")
    reject_all(R.epilogue(o["fwd"], old=o["old"]), m, "forward")
    reject_all(R.epilogue(o["dgrad"], old=o["old"]), md, "flipped launch")
    reject_all(R.epilogue(o["wgrad"], old=o["oldw"]), mw, "weight gradient")
    mz = f32_expect(f32_wgrad_mutants(o["z"], o["dyw"], 3, 1, 1, o["oldw"]), n * h * w)
    mz["transform skipped"] = R.im2col_wgrad(o["y_prev"], o["dyw"], 3, 1, 1) + o["oldw"]
    if w == 1:
        mz.pop("border tap")
    reject_all(R.epilogue(o["wgrad_z"], old=o["oldw"]), mz, "weight gradient behind the transform")
    if C32.sm_up(case):
        up = R.upcat(o["a"], None)
        mu = f32_expect(R.f32_mutants(up, o["wt"], 1, 1), 9 * g)
        mu["up-sampling off by one column"] = R.im2col_fwd(np.roll(up, 1, axis=2), o["wt"], 1, 1)
        reject_all(o["fwd_up"], mu, "up-sampled source")
        reject_all(o["wgrad_zup"], {"not up-sampled": R.im2col_wgrad(o["z"], o["dyw"], 3, 1, 1)}, "weight gradient behind the up-sampling")
    for family in C32.FAMILIES:
        t = C32.sm_tier_b(case, family)
        check_tier_b(t["fwd"], family, None)
        check_tier_b(t["dgrad"], family, None, dgrad_to=(h, w))
        check_wgrad_tier_b(t["wgrad"], family)
        check_wgrad_tier_b(t["wgrad_z"], family)
        if C32.sm_up(case):
            check_tier_b(t["fwd_up"], family, None)
            check_wgrad_tier_b(t["wgrad_up"], family)
            assert np.array_equal(t["fwd_up"]["xin"], R.upcat(t["fwd_up"]["a"], None))


WG_HOST = [C32.WG[i][0] for i in (0, 1, 2, 5, 7, 9)]      # both tiles, one split (144 pixels: the low split term shows), the stem, 1x1/1, stride 2


@pytest.mark.parametrize("case", WG_HOST, ids=[C32.ig_id(c) for c in WG_HOST])
def test_f32_wgrad_tier_a_and_b(case):
    n, h, w, ci, co, k, s, p = case
    o = C32.wg_tier_a(case)
    assert R.bar(o["wgrad"])[0] <= F32_BAR
    pixels = R.wgrad_f32_plan(*case)[3]
    got = reject_all(R.epilogue(o["wgrad"], old=o["oldw"]), f32_expect(f32_wgrad_mutants(o["x"], o["dy"], k, s, p, o["oldw"]), pixels), "weight gradient")
    assert ("low split term" in got) == (pixels <= LOW_TERM_K) and "bf16 operand" in got
    for family in C32.FAMILIES:
        check_wgrad_tier_b(C32.wg_tier_b(case, family), family)


def test_f32_wgrad_part_and_fused_x3_and_bn_fold_references():
    case = C32.WG_PART[0]
    n, h, w, ca, cs, co = case
    o = C32.part_tier_a(case)
    m = f32_expect(f32_wgrad_mutants(o["x"], o["dy"], 3, 1, 1, o["oldw"]), n * h * w)
    only_up = R.im2col_wgrad(R.upcat(o["a"], np.zeros_like(o["skip"])), o["dy"], 3, 1, 1) + o["oldw"]
    m["skip half missing"] = only_up
    reject_all(R.epilogue(o["wgrad"], old=o["oldw"]), m, "channel slices")
    for family in C32.FAMILIES:
        t = C32.part_tier_b(case, family)
        check_wgrad_tier_b(t, family)
        assert np.array_equal(t["xin"], R.upcat(t["a"], t["skip"]))
        f = C32.x3_fused_tier_b(family)
        check_tier_b(f, family, None)
        assert np.abs(f["bias"]).max() + np.abs(f["res"]).max() <= 2
    o = C32.x3_fused_tier_a()
    n, h, w, ci, co, k, s, p = C32.X3_FUSED
    ref = R.epilogue(o["fwd"], bias=o["bias"], residual=o["res"], slope=0.0)
    assert R.verdict(ref.leg_rne, ref, False)[0] and not R.verdict(R.epilogue(o["fwd"], bias=o["bias"], slope=0.0).r64, ref, False)[0]
    # bn_fold: the float64 restatement is the definition; the fp32 restatement stays within a few ulp of it at every variance scale
    import _norm_ref as N
    for case in C32.BN_FOLD:
        b = C32.bn_fold_operands(case)
        args = (b["w"], b["bias"], b["gamma"], b["beta"], b["rm"], b["rv"], C32.BN_EPS)
        w64, b64, mag = R.bn_fold_ref(*args, F64)
        w32, b32, _ = R.bn_fold_ref(*args, F32)
        s = b["gamma"].astype(F64) / np.sqrt(b["rv"].astype(F64) + F64(F32(C32.BN_EPS)))
        assert np.allclose(w64, b["w"] * s[:, None, None, None], rtol=1e-14) and np.allclose(b64, b["beta"] + (b["bias"].astype(F64) - b["rm"]) * s, rtol=1e-12, atol=1e-14)
        assert N.bar(w32, w64, np.abs(w64))[0] <= 2.0 ** -20 and N.bar(b32, b64, mag)[0] <= 2.0 ** -20 and w32.dtype == F32
    assert {c[0] for c in C32.BN_FOLD} == {4, 24, 64}


def test_the_bf16_weight_gradient_cases_reach_their_plans():
    """launch_wgrad<..., bf16>, restated in _conv_ref.wgrad_bf16_plan: the split-K cases of tests/test_gpu_conv_bf16_grade.py reach both
    ungraded tiles under both gathers, the XCD-aware block order with and without empty splits, and the two-dimensional grid."""
    import test_gpu_conv_bf16_grade as B16
    plan = R.wgrad_bf16_plan
    got = [plan(*c, generic=bool(g), no_xcd=bool(x)) for c, g, x in B16.WG_SPLITK]
    big, small = "conv_wgrad_bf16_kernel<128, 64, 2, 2, %s>", "conv_wgrad_bf16_kernel<32, 128, 1, 4, %s>"
    assert [t[0] for t in got] == [big % "true", big % "false", small % "true", small % "false", big % "true", big % "true", big % "true"]
    # M = 480 in images of 160 (5 x 32) / (10 x 16): two splits of 256, the first ends inside image 1; too few splits for the XCD order
    assert all(t[1:] == (2, 256, 480, False, 0) for t in got[:4]) and 256 % 160 != 0
    assert got[4][1:] == (16, 256, 4096, True, 0)                     # 9 tiles, 16 splits of 256 in XCD-aware order
    assert got[5][1:] == (24, 256, 5376, True, 3)                     # 21 splits rounded up to 24: three empty ones
    assert got[6][1:] == (24, 256, 5376, False, 3)                    # WGRAD_NO_XCD: the same plan on the two-dimensional grid
    assert R.cdiv(128, 128) * R.cdiv(9 * 64, 64) == 9 and R.wgrad_splits(5376, 9, 512, 64) == (21, 256)
    # every case of the older lists is the 64 x 64 or the 128 x 64 tile with fewer than 16 splits: what the cases above add
    for c in B16.IGEMM + [s + (3, 1, 1) for s in B16.WG]:
        assert plan(*c)[1] < 16 and not plan(*c)[0].startswith(small[:28])
    n, h, w, ca, cs, co = B16.WG_PART
    geom = (n, h, w, ca + cs, co, 3, 1, 1)
    for kw in (dict(src_c=ca, up=True), dict(src_c=cs)):
        assert plan(*geom, **kw)[0] == "conv_wgrad_bf16_kernel<64, 64, 2, 2, true>" and plan(*geom, generic=True, **kw)[0].endswith("false>")
    assert ca % 8 == 0 and cs % 8 == 0 and h % 2 == 0 and w % 2 == 0
