"""The convolutions that multiply fp32 operands on the fp32 matrix pipe (csrc/conv_small.hip: v_mfma_f32_16x16x4_f32; the non-bf16,
non-X3 instances of csrc/conv_igemm.hip and csrc/conv_wgrad.hip: v_mfma_f32_32x32x2_f32) element-wise against float64, called at
kernel level, with the entry points that put epilogues on them (conv2d_fwd_fused, conv2d_fwd_bnstats, conv2d_dgrad_bnreduce,
conv2d_dgrad_split, conv2d_fwd_upcat, conv2d_wgrad_part, conv2d_wgrad_bnin), conv2d_fwd_fused on an X3 instance, and bn_fold.
Cases, operands and references live in tests/_conv_f32_cases.py and tests/_conv_ref.py; tests/test_conv_ref_host.py proves on the CPU
that every case reaches the launch regime its comment claims, that tier A's bar rejects seven mutants (a bf16-rounded operand and
a dropped low split term among them) and that tier B's operands are exact.

Tier A (arbitrary fp32 operands, some over 12 binades): e = |kernel - f64| / magnitude element-wise (magnitude: the same operation on
|x|, |w| plus |bias|, |residual|, |old| where they enter) against A = max(4 x max(d_rne, d_mfma), 2^-22): d_rne is torch's fp32 CPU
convolution / autograd, d_mfma the model _conv_ref.rne_matmul (an fp32 accumulator, the exact sum of the 2 or 4 products of one
matrix instruction added with one round-to-nearest, in im2col order; the pixel axis for the weight gradient), both against float64
over the whole output.  No tolerance comes from a kernel.  Activations are graded with the pre-activation's bar; the fused
statistics go through stats_ref (both the in-epilogue path and the sliced-then-bn_stats path), the BatchNorm-backward sums through
bn_sums_ref.  Nothing is masked; every output is a slice of a larger allocation written over NaN, with a 256-element guard on
either side whose bits must survive.

Tier B (the three exact families of the split grade: every term a multiple of one power of two, mag / u <= 2^23): every partial sum
in any order is exact (K-slices, split-K and their atomics included), so the kernel must equal float64 BIT FOR BIT, on every launch
of tier A with its epilogue (bias + ReLU, residual, accumulation onto old).

Every launch asserts from prof_kernels() that its own instantiation ran once and nothing else ran; routes are forced with the
switchboard only (F32_SPLIT = 0, IGEMM_TILE, GENERIC_GATHER, WGRAD_GENERIC, WGRAD_BLOCKS), restored to -1 afterwards.

Symbols that run here under a route assertion (the timing table of csrc/api.hip knows every kernel by the name it registers on
its first launch; there is no fixed table and no numeric id any more):
  conv_igemm_kernel<128, 128, 2, 2 | 128, 64, 2, 2 | 64, 64, 2, 2 | 128, 32, 4, 1, false, false, false>   (generic loop)
  conv_igemm_kernel<..., false, true, false>   (uniform-tap loop),  conv_igemm_kernel<..., false, true, true>   (fused input)
  conv3x3_small_kernel<1, 1 | 2, 1 | 1, 2>,  conv3x3_small_wgrad_kernel<1, 1 | 2, 1 | 1, 2>   (small_wgrad_fold_kernel carries no
  timing record of its own: it is graded through the weight gradient it finishes)
  conv_wgrad_kernel<64, 64, 2, 2, false | true>,  conv_wgrad_kernel<32, 128, 1, 4, false | true>
conv_wgrad_kernel<128, ...> does not exist: the storage is a compile-time parameter of launch_wgrad, and conv2d_wgrad_impl takes
the 128-row tile for bf16 alone.  The bf16 launches register their own symbols, graded in test_gpu_conv_bf16_grade.py; the channel
slices are graded on conv_wgrad_x3_kernel as well (F32_SPLIT = 1).

Set UDASEG_DEVIATION_LOG to a file name to collect the figures (profiles/conv_f32_grade.txt).
"""
import numpy as np
import pytest
import torch

import _conv_f32_cases as C
import _conv_ref as R
from _conv_ref import F32, F64
from test_gpu_conv_f32x3_grade import K, NAN, Out, _log, dev, exact, grade_stats, guards, new_stats, options, ran, ran_x3, totals  # noqa: F401

pytestmark = pytest.mark.gpu
SLOPE = C.SLOPE
FAMILIES = C.FAMILIES


def packed(K, d, wt):
    """OHWI weights on the device and their data-gradient packing [ci][k][k][co]."""
    wd = dev(wt)
    wtp = torch.full((d.ci, d.kh, d.kw, d.co), NAN, device="cuda")
    K.pack_dgrad_weights(d, wd, wtp)
    return wd, wtp


# ============================================================================================== 1. conv_igemm_kernel, geometries
@pytest.mark.parametrize("generic", (0, 1), ids=("uniform", "generic"))
@pytest.mark.parametrize("tile", C.TILES, ids=["tile%d" % t for t in C.TILES])
@pytest.mark.parametrize("case", C.IG, ids=[C.ig_id(c) for c in C.IG])
def test_igemm_geometries(K, case, tile, generic):
    """conv2d_fwd (plain: K-sliced atomics; bias + LeakyReLU; accumulating), conv2d_fwd_fused (bias + residual + ReLU),
    conv2d_fwd_bnstats (no bias: sliced, then the separate statistics pass) and conv2d_dgrad (plain, accumulating) on one tile
    and one gather loop."""
    n, h, w, ci, co, k, s, p = case
    G = R.F32Grader(f"igemm tile{tile} {'generic' if generic else 'uniform'} {case}", _log)
    o = C.ig_tier_a(case)
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    fsym = R.igemm_f32_symbol(tile, R.igemm_f32_uniform(ci, k * k, generic))
    dsym = R.igemm_f32_symbol(tile, R.igemm_f32_uniform(co, k * k, generic))
    ys, xs = (n, d.ho, d.wo, co), (n, h, w, ci)
    with options(K, F32_SPLIT=0, IGEMM_TILE=tile, GENERIC_GATHER=generic):
        wd, wtp = packed(K, d, o["wt"])
        xd, dyd, bd, rd = dev(o["x"]), dev(o["dy"]), dev(o["bias"]), dev(o["res"])
        y, yl, ya, yf, yb, st = Out(ys), Out(ys), Out(ys, o["old"]), Out(ys), Out(ys), new_stats(K, co)
        dx, dxa = Out(xs), Out(xs, o["oldx"])
        ran(K, G, "fwd", fsym, lambda: K.conv2d_fwd(d, xd, wd, None, y.t))
        ran(K, G, "fwd bias leaky", fsym, lambda: K.conv2d_fwd(d, xd, wd, bd, yl.t, 1, SLOPE))
        ran(K, G, "fwd accumulate", fsym, lambda: K.conv2d_fwd(d, xd, wd, None, ya.t, accumulate=True))
        ran(K, G, "fwd fused", fsym, lambda: K.conv2d_fwd_fused(d, xd, wd, bd, rd, yf.t, act=1, slope=0.0))
        ran(K, G, "fwd bnstats", fsym, lambda: K.conv2d_fwd_bnstats(d, xd, wd, None, yb.t, st.t))
        ran(K, G, "dgrad", dsym, lambda: K.conv2d_dgrad(d, dyd, wtp, dx.t))
        ran(K, G, "dgrad accumulate", dsym, lambda: K.conv2d_dgrad(d, dyd, wtp, dxa.t, accumulate=True))
        G.grade("fwd", y.host(), o["fwd"], False)
        G.grade("fwd + bias + LeakyReLU", yl.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=SLOPE), False)
        G.grade("fwd accumulated", ya.host(), R.epilogue(o["fwd"], old=o["old"]), False)
        G.grade("fwd + bias + residual + ReLU", yf.host(), R.epilogue(o["fwd"], bias=o["bias"], residual=o["res"], slope=0.0), False)
        G.grade("fwd with statistics", yb.host(), o["fwd"], False)
        grade_stats(K, G, "fwd statistics", st, o["fwd"])
        G.grade("dgrad", dx.host(), o["dgrad"], False)
        G.grade("dgrad accumulated", dxa.host(), R.epilogue(o["dgrad"], old=o["oldx"]), False)
        outs = [y, yl, ya, yf, yb, st, dx, dxa]
        for family in FAMILIES:
            f, b = C.ig_tier_b(case, family)
            wf, _ = packed(K, d, f["w"])
            _, wb = packed(K, d, b["w"])
            fx, fb = dev(f["x"]), dev(f["bias"])
            e1, e2, e3, e4, e5 = Out(ys), Out(ys, f["old"]), Out(ys), Out(xs), Out(xs, b["old"])
            ran(K, G, f"{family} fwd bias relu", fsym, lambda: K.conv2d_fwd(d, fx, wf, fb, e1.t, 1, 0.0))
            ran(K, G, f"{family} fwd accumulate", fsym, lambda: K.conv2d_fwd(d, fx, wf, None, e2.t, accumulate=True))
            ran(K, G, f"{family} fwd fused", fsym, lambda: K.conv2d_fwd_fused(d, fx, wf, fb, dev(f["res"]), e3.t, act=1, slope=0.0))
            ran(K, G, f"{family} dgrad", dsym, lambda: K.conv2d_dgrad(d, dev(b["x"]), wb, e4.t))
            ran(K, G, f"{family} dgrad accumulate", dsym, lambda: K.conv2d_dgrad(d, dev(b["x"]), wb, e5.t, accumulate=True))
            exact(G, f"{family} fwd + bias + ReLU", e1.host(), C.relu(f["r64"] + f["bias"]))
            exact(G, f"{family} fwd accumulated", e2.host(), f["r64"] + f["old"])
            exact(G, f"{family} fwd + bias + residual + ReLU", e3.host(), C.relu(f["r64"] + f["bias"] + f["res"]))
            exact(G, f"{family} dgrad", e4.host(), b["r64"])
            exact(G, f"{family} dgrad accumulated", e5.host(), b["r64"] + b["old"])
            outs += [e1, e2, e3, e4, e5]
    guards(G, "igemm", *outs)
    G.done()


@pytest.mark.parametrize("tile", C.TILES, ids=["tile%d" % t for t in C.TILES])
def test_igemm_unsliced_plain_store_and_in_epilogue_statistics(K, tile):
    """>= 384 tiles of 64 x 64: a plain forward is ONE class with the fast epilogue, conv2d_fwd_bnstats forms its sums there."""
    shape = C.LARGE[tile]
    n, h, w, ci, co = shape
    G = R.F32Grader(f"igemm unsliced tile{tile} {shape}", _log)
    o = C.large_tier_a(shape)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    sym = R.igemm_f32_symbol(tile, True)
    with options(K, F32_SPLIT=0, IGEMM_TILE=tile):
        xd, wd = dev(o["x"]), dev(o["wt"])
        y, yb, st = Out((n, h, w, co)), Out((n, h, w, co)), new_stats(K, co)
        ran(K, G, "fwd", sym, lambda: K.conv2d_fwd(d, xd, wd, None, y.t))
        ran(K, G, "fwd bnstats", sym, lambda: K.conv2d_fwd_bnstats(d, xd, wd, None, yb.t, st.t))
        G.grade("fwd", y.host(), o["fwd"], False)
        G.grade("fwd with statistics", yb.host(), o["fwd"], False)
        grade_stats(K, G, "fwd in-epilogue statistics", st, o["fwd"])
        outs = [y, yb, st]
        for family in FAMILIES:
            t = C.large_tier_b(shape, family)
            e1, e2, s2 = Out((n, h, w, co)), Out((n, h, w, co)), new_stats(K, co)
            ran(K, G, f"{family} fwd", sym, lambda: K.conv2d_fwd(d, dev(t["x"]), dev(t["w"]), None, e1.t))
            ran(K, G, f"{family} fwd bnstats", sym, lambda: K.conv2d_fwd_bnstats(d, dev(t["x"]), dev(t["w"]), None, e2.t, s2.t))
            exact(G, f"{family} fwd", e1.host(), t["r64"])
            exact(G, f"{family} fwd with statistics", e2.host(), t["r64"])
            outs += [e1, e2, s2]
    guards(G, "unsliced", *outs)
    G.done()


@pytest.mark.parametrize("case", C.BNR, ids=["n%d_%dx%d_ci%d_co%d" % c for c in C.BNR])
def test_igemm_dgrad_with_batchnorm_backward_sums(K, case):
    """conv2d_dgrad_bnreduce: the unsliced data gradient whose fast epilogue also forms the two BatchNorm-backward sums."""
    n, h, w, ci, co = case
    G = R.F32Grader(f"igemm bnreduce {case}", _log)
    o = C.bnr_tier_a(case)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    sym = R.igemm_f32_symbol(R.igemm_f32_tile(ci), True)
    with options(K, F32_SPLIT=0):
        if not K.conv2d_dgrad_bnreduce_ok(d):
            pytest.fail(f"conv2d_dgrad_bnreduce_ok refuses {case}")
        _, wtp = packed(K, d, o["wt"])
        dx, dxb, bs = Out((n, h, w, ci)), Out((n, h, w, ci)), new_stats(K, ci)
        bn = tuple(dev(o[k]) for k in ("prev_y", "mean", "rstd", "gamma", "beta"))
        ran(K, G, "dgrad", sym, lambda: K.conv2d_dgrad(d, dev(o["dy"]), wtp, dx.t))
        ran(K, G, "dgrad bn sums", sym, lambda: K.conv2d_dgrad_bnreduce(d, dev(o["dy"]), wtp, dxb.t, *bn, 1, SLOPE, bs.t))
        G.grade("dgrad", dx.host(), o["dgrad"], False)
        G.grade("dgrad with bn sums", dxb.host(), o["dgrad"], False)
        s1, s2, _ = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], SLOPE)
        tot = totals(K, bs)
        G.grade("bn-backward sum", tot[0], s1, False)
        G.grade("bn-backward sum with y_hat", tot[1], s2, False)
    guards(G, "bnreduce", dx, dxb, bs)
    G.done()


@pytest.mark.parametrize("generic", (0, 1), ids=("uniform", "generic"))
@pytest.mark.parametrize("tile", C.TILES, ids=["tile%d" % t for t in C.TILES])
def test_igemm_dgrad_split(K, tile, generic):
    """conv2d_dgrad_split: channels [0, 128) of the gradient in one tensor, [128, 136) in another (K-sliced atomics onto both)."""
    n, h, w, ci, co, split = C.SPLIT
    G = R.F32Grader(f"igemm split tile{tile} {'generic' if generic else 'uniform'} {C.SPLIT}", _log)
    o = C.split_tier_a()
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    sym = R.igemm_f32_symbol(tile, R.igemm_f32_uniform(co, 9, generic))
    with options(K, F32_SPLIT=0, IGEMM_TILE=tile, GENERIC_GATHER=generic):
        _, wtp = packed(K, d, o["wt"])
        da, db = Out((n, h, w, split)), Out((n, h, w, ci - split))
        ran(K, G, "dgrad split", sym, lambda: K.conv2d_dgrad_split(d, dev(o["dy"]), wtp, da.t, db.t))
        G.grade("dgrad split at 128", np.concatenate([da.host(), db.host()], axis=3), o["dgrad"], False)
        outs = [da, db]
        for family in FAMILIES:
            t = C.split_tier_b(family)
            _, wb = packed(K, d, t["w"])
            ea, eb = Out((n, h, w, split)), Out((n, h, w, ci - split))
            ran(K, G, f"{family} dgrad split", sym, lambda: K.conv2d_dgrad_split(d, dev(t["x"]), wb, ea.t, eb.t))
            exact(G, f"{family} dgrad split at 128", np.concatenate([ea.host(), eb.host()], axis=3), t["r64"])
            outs += [ea, eb]
    guards(G, "split", *outs)
    G.done()


@pytest.mark.parametrize("tile", C.TILES, ids=["tile%d" % t for t in C.TILES])
@pytest.mark.parametrize("case", C.UPCAT, ids=["n%d_%dx%d_ca%d_cs%d_co%d" % c for c in C.UPCAT])
def test_igemm_fused_decoder_input(K, case, tile):
    """conv2d_fwd_upcat on the implicit-GEMM kernel: cat([nearest_x2(a), skip]) gathered in the K loop, against R.fwd_upcat's
    operation (the convolution on the materialised concatenation)."""
    n, h, w, ca, cs, co = case
    G = R.F32Grader(f"igemm fused input tile{tile} {case}", _log)
    o = C.upcat_tier_a(case)
    d = K.conv_desc(n, h, w, ca + cs, co, 3, 1, 1)
    sym = R.igemm_f32_symbol(tile, True, up=True)
    with options(K, F32_SPLIT=0, IGEMM_TILE=tile):
        ad, sd, wd = dev(o["a"]), (dev(o["skip"]) if cs else None), dev(o["wt"])
        yl, y, st = Out((n, h, w, co)), Out((n, h, w, co)), new_stats(K, co)
        ran(K, G, "fused input bias leaky", sym, lambda: K.conv2d_fwd_upcat(d, ad, sd, wd, dev(o["bias"]), yl.t, act=1, slope=SLOPE))
        ran(K, G, "fused input stats", sym, lambda: K.conv2d_fwd_upcat(d, ad, sd, wd, None, y.t, stats=st.t))
        G.grade("fused input fwd + bias + LeakyReLU", yl.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=SLOPE), False)
        G.grade("fused input fwd", y.host(), o["fwd"], False)
        grade_stats(K, G, "fused input statistics", st, o["fwd"])
        outs = [yl, y, st]
        for family in FAMILIES:
            t = C.upcat_tier_b(case, family)
            e = Out((n, h, w, co))
            sb = dev(t["skip"]) if cs else None
            ran(K, G, f"{family} fused input", sym, lambda: K.conv2d_fwd_upcat(d, dev(t["a"]), sb, dev(t["w"]), dev(t["bias"]), e.t, act=1, slope=0.0))
            exact(G, f"{family} fused input fwd + bias + ReLU", e.host(), C.relu(t["r64"] + t["bias"]))
            outs.append(e)
    guards(G, "fused input", *outs)
    G.done()


# ======================================================================================================== 2. the small kernels
@pytest.mark.parametrize("case", C.SM, ids=[C.sm_id(c) for c in C.SM])
def test_small_forward_and_flipped(K, case):
    """conv3x3_small_kernel<G, T>: forward with every epilogue term and the statistics, the flipped launch (data gradient), and
    the up-sampled source (conv2d_fwd_upcat without a skip half) where the extents are even."""
    n, h, w, g, p = case
    G = R.F32Grader(f"small {case}", _log)
    o = C.sm_tier_a(case)
    sym = R.small_symbol(g, p)
    d, dd = K.conv_desc(n, h, w, g, p, 3, 1, 1), K.conv_desc(n, h, w, p, g, 3, 1, 1)
    ys = (n, h, w, p)
    with options(K, F32_SPLIT=0):
        wd = dev(o["wt"])
        _, wtp = packed(K, dd, o["wd"])
        xd, bd = dev(o["x"]), dev(o["bias"])
        y, yl, yf, ya, yb, st = Out(ys), Out(ys), Out(ys), Out(ys, o["old"]), Out(ys), new_stats(K, p)
        dx, dxa = Out(ys), Out(ys, o["old"])
        ran(K, G, "fwd", sym, lambda: K.conv2d_fwd(d, xd, wd, None, y.t))
        ran(K, G, "fwd bias leaky", sym, lambda: K.conv2d_fwd(d, xd, wd, bd, yl.t, 1, SLOPE))
        ran(K, G, "fwd fused", sym, lambda: K.conv2d_fwd_fused(d, xd, wd, bd, dev(o["res"]), yf.t, act=1, slope=0.0))
        ran(K, G, "fwd accumulate", sym, lambda: K.conv2d_fwd(d, xd, wd, None, ya.t, accumulate=True))
        ran(K, G, "fwd bnstats", sym, lambda: K.conv2d_fwd_bnstats(d, xd, wd, bd, yb.t, st.t))
        ran(K, G, "dgrad", sym, lambda: K.conv2d_dgrad(dd, dev(o["dy"]), wtp, dx.t))
        ran(K, G, "dgrad accumulate", sym, lambda: K.conv2d_dgrad(dd, dev(o["dy"]), wtp, dxa.t, accumulate=True))
        G.grade("fwd", y.host(), o["fwd"], False)
        G.grade("fwd + bias + LeakyReLU", yl.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=SLOPE), False)
        G.grade("fwd + bias + residual + ReLU", yf.host(), R.epilogue(o["fwd"], bias=o["bias"], residual=o["res"], slope=0.0), False)
        G.grade("fwd accumulated", ya.host(), R.epilogue(o["fwd"], old=o["old"]), False)
        ref = R.epilogue(o["fwd"], bias=o["bias"])
        G.grade("fwd + bias with statistics", yb.host(), ref, False)
        grade_stats(K, G, "fwd statistics", st, ref)
        G.grade("dgrad", dx.host(), o["dgrad"], False)
        G.grade("dgrad accumulated", dxa.host(), R.epilogue(o["dgrad"], old=o["old"]), False)
        outs = [y, yl, yf, ya, yb, st, dx, dxa]
        if C.sm_up(case):
            yu, su = Out(ys), new_stats(K, p)
            ran(K, G, "up fwd", sym, lambda: K.conv2d_fwd_upcat(d, dev(o["a"]), None, wd, bd, yu.t, act=1, slope=SLOPE, stats=su.t))
            G.grade("up fwd + bias + LeakyReLU", yu.host(), R.epilogue(o["fwd_up"], bias=o["bias"], slope=SLOPE), False)
            grade_stats(K, G, "up fwd statistics", su, R.epilogue(o["fwd_up"], bias=o["bias"]))
            outs += [yu, su]
        for family in FAMILIES:
            t = C.sm_tier_b(case, family)
            f, b = t["fwd"], t["dgrad"]
            _, wb = packed(K, dd, b["w"])
            fx, fw, fb = dev(f["x"]), dev(f["w"]), dev(f["bias"])
            e1, e2, e3, e4, e5 = Out(ys), Out(ys), Out(ys, f["old"]), Out(ys), Out(ys, b["old"])
            ran(K, G, f"{family} fwd bias relu", sym, lambda: K.conv2d_fwd(d, fx, fw, fb, e1.t, 1, 0.0))
            ran(K, G, f"{family} fwd fused", sym, lambda: K.conv2d_fwd_fused(d, fx, fw, fb, dev(f["res"]), e2.t, act=1, slope=0.0))
            ran(K, G, f"{family} fwd accumulate", sym, lambda: K.conv2d_fwd(d, fx, fw, None, e3.t, accumulate=True))
            ran(K, G, f"{family} dgrad", sym, lambda: K.conv2d_dgrad(dd, dev(b["x"]), wb, e4.t))
            ran(K, G, f"{family} dgrad accumulate", sym, lambda: K.conv2d_dgrad(dd, dev(b["x"]), wb, e5.t, accumulate=True))
            exact(G, f"{family} fwd + bias + ReLU", e1.host(), C.relu(f["r64"] + f["bias"]))
            exact(G, f"{family} fwd + bias + residual + ReLU", e2.host(), C.relu(f["r64"] + f["bias"] + f["res"]))
            exact(G, f"{family} fwd accumulated", e3.host(), f["r64"] + f["old"])
            exact(G, f"{family} dgrad", e4.host(), b["r64"])
            exact(G, f"{family} dgrad accumulated", e5.host(), b["r64"] + b["old"])
            outs += [e1, e2, e3, e4, e5]
            if C.sm_up(case):
                u = t["fwd_up"]
                e6 = Out(ys)
                ran(K, G, f"{family} up fwd", sym, lambda: K.conv2d_fwd_upcat(d, dev(u["a"]), None, dev(u["w"]), dev(u["bias"]), e6.t, act=1, slope=0.0))
                exact(G, f"{family} up fwd + bias + ReLU", e6.host(), C.relu(u["r64"] + u["bias"]))
                outs.append(e6)
    guards(G, "small", *outs)
    G.done()


@pytest.mark.parametrize("case", C.SM, ids=[C.sm_id(c) for c in C.SM])
def test_small_weight_gradient(K, case):
    """conv3x3_small_wgrad_kernel<G, T> + small_wgrad_fold_kernel: conv2d_wgrad (over NaN, accumulating) and conv2d_wgrad_bnin
    (LeakyReLU(fma(y, scale, shift)) applied while staging; plain and behind the up-sampling)."""
    n, h, w, g, p = case
    G = R.F32Grader(f"small wgrad {case}", _log)
    o = C.sm_tier_a(case)
    sym = R.small_symbol(g, p, wgrad=True)
    d = K.conv_desc(n, h, w, g, p, 3, 1, 1)
    ws = (p, 3, 3, g)
    with options(K, F32_SPLIT=0):
        xd, dyd = dev(o["x"]), dev(o["dyw"])
        dw, dwa, dz, dza = Out(ws), Out(ws, o["oldw"]), Out(ws), Out(ws, o["oldw"])
        bn = (dev(o["sc"]), dev(o["sh"]), 1, SLOPE)
        ran(K, G, "wgrad", sym, lambda: K.conv2d_wgrad(d, xd, dyd, dw.t))
        ran(K, G, "wgrad accumulate", sym, lambda: K.conv2d_wgrad(d, xd, dyd, dwa.t, True))
        ran(K, G, "wgrad bnin", sym, lambda: K.conv2d_wgrad_bnin(d, dev(o["y_prev"]), *bn, dyd, dz.t, False))
        ran(K, G, "wgrad bnin accumulate", sym, lambda: K.conv2d_wgrad_bnin(d, dev(o["y_prev"]), *bn, dyd, dza.t, True))
        G.grade("wgrad over NaN", dw.host(), o["wgrad"], False)
        G.grade("wgrad accumulated", dwa.host(), R.epilogue(o["wgrad"], old=o["oldw"]), False)
        G.grade("wgrad bnin over NaN", dz.host(), o["wgrad_z"], False)
        G.grade("wgrad bnin accumulated", dza.host(), R.epilogue(o["wgrad_z"], old=o["oldw"]), False)
        outs = [dw, dwa, dz, dza]
        if C.sm_up(case):
            du = Out(ws, o["oldw"])
            ran(K, G, "wgrad bnin up accumulate", sym, lambda: K.conv2d_wgrad_bnin(d, dev(o["ya"]), *bn, dyd, du.t, True, up=True))
            G.grade("wgrad bnin up accumulated", du.host(), R.epilogue(o["wgrad_zup"], old=o["oldw"]), False)
            outs.append(du)
        one, zero = torch.ones(g, device="cuda"), torch.zeros(g, device="cuda")
        for family in FAMILIES:
            t = C.sm_tier_b(case, family)
            a, z = t["wgrad"], t["wgrad_z"]
            e1, e2, e3 = Out(ws), Out(ws, a["old"]), Out(ws, z["old"])
            ran(K, G, f"{family} wgrad", sym, lambda: K.conv2d_wgrad(d, dev(a["x"]), dev(a["w"]), e1.t))
            ran(K, G, f"{family} wgrad accumulate", sym, lambda: K.conv2d_wgrad(d, dev(a["x"]), dev(a["w"]), e2.t, True))
            ran(K, G, f"{family} wgrad bnin accumulate", sym, lambda: K.conv2d_wgrad_bnin(d, dev(z["x"]), one, zero, 1, 0.0, dev(z["w"]), e3.t, True))
            exact(G, f"{family} wgrad over NaN", e1.host(), a["r64"])
            exact(G, f"{family} wgrad accumulated", e2.host(), a["r64"] + a["old"])
            exact(G, f"{family} wgrad bnin accumulated", e3.host(), z["r64"] + z["old"])
            outs += [e1, e2, e3]
            if C.sm_up(case):
                u = t["wgrad_up"]
                e4 = Out(ws, u["old"])
                ran(K, G, f"{family} wgrad bnin up accumulate", sym,
                    lambda: K.conv2d_wgrad_bnin(d, dev(u["a"]), one, zero, 1, 0.0, dev(u["w"]), e4.t, True, up=True))
                exact(G, f"{family} wgrad bnin up accumulated", e4.host(), u["r64"] + u["old"])
                outs.append(e4)
    guards(G, "small wgrad", *outs)
    G.done()


# ======================================================================================================== 3. conv_wgrad_kernel
WG_RUNS = [(case, blocks, generic) for case, bl in C.WG for blocks in bl for generic in (0, 1)]


@pytest.mark.parametrize("case,blocks,generic", WG_RUNS, ids=["%s-blocks%d-%s" % (C.ig_id(c), b, "generic" if g else "uniform") for c, b, g in WG_RUNS])
def test_wgrad_split_k(K, case, blocks, generic):
    """conv2d_wgrad on conv_wgrad_kernel<64, 64, 2, 2, *> / <32, 128, 1, 4, *>: over NaN (one split: a plain store; several: a
    memset and atomics) and accumulating."""
    n, h, w, ci, co, k, s, p = case
    G = R.F32Grader(f"wgrad {case} blocks{blocks} {'generic' if generic else 'uniform'}", _log)
    o = C.wg_tier_a(case)
    sym = R.wgrad_f32_plan(*case, blocks=blocks, generic=bool(generic))[0]
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    ws = (co, k, k, ci)
    with options(K, F32_SPLIT=0, WGRAD_GENERIC=generic, WGRAD_BLOCKS=blocks):
        xd, dyd = dev(o["x"]), dev(o["dy"])
        dw, dwa = Out(ws), Out(ws, o["oldw"])
        ran(K, G, "wgrad", sym, lambda: K.conv2d_wgrad(d, xd, dyd, dw.t))
        ran(K, G, "wgrad accumulate", sym, lambda: K.conv2d_wgrad(d, xd, dyd, dwa.t, True))
        G.grade("wgrad over NaN", dw.host(), o["wgrad"], False)
        G.grade("wgrad accumulated", dwa.host(), R.epilogue(o["wgrad"], old=o["oldw"]), False)
        outs = [dw, dwa]
        for family in FAMILIES:
            t = C.wg_tier_b(case, family)
            e1, e2 = Out(ws), Out(ws, t["old"])
            ran(K, G, f"{family} wgrad", sym, lambda: K.conv2d_wgrad(d, dev(t["x"]), dev(t["w"]), e1.t))
            ran(K, G, f"{family} wgrad accumulate", sym, lambda: K.conv2d_wgrad(d, dev(t["x"]), dev(t["w"]), e2.t, True))
            exact(G, f"{family} wgrad over NaN", e1.host(), t["r64"])
            exact(G, f"{family} wgrad accumulated", e2.host(), t["r64"] + t["old"])
            outs += [e1, e2]
    guards(G, "wgrad", *outs)
    G.done()


def channel_slices(K, case, generic, split):
    """conv2d_wgrad_part: the up-sampled half (c_off = 0, read through nearest_x2) and the skip half (c_off = ca) of the weight
    gradient over cat([nearest_x2(a), skip]), two launches accumulating into one dW.  split: on conv_wgrad_x3_kernel, with the
    split grade's bar; else on conv_wgrad_kernel."""
    n, h, w, ca, cs, co = case
    G = (R.X3Grader if split else R.F32Grader)(f"wgrad part {'x3 ' if split else ''}{case} {'generic' if generic else 'uniform'}", _log)
    o = C.part_x3_tier_a(case) if split else C.part_tier_a(case)
    geom = (n, h, w, ca + cs, co, 3, 1, 1)
    plan = R.wgrad_x3_plan if split else R.wgrad_f32_plan
    sym_a = plan(*geom, generic=bool(generic), src_c=ca, up=True)[0]
    sym_s = plan(*geom, generic=bool(generic), src_c=cs)[0]
    d = K.conv_desc(*geom)
    with options(K, F32_SPLIT=split, WGRAD_GENERIC=generic):
        dw = Out(o["oldw"].shape, o["oldw"])
        ran(K, G, "part up", sym_a, lambda: K.conv2d_wgrad_part(d, dev(o["a"]), 0, True, dev(o["dy"]), dw.t, True))
        half = dw.host().copy()
        G.exact("skip channels after the up-sampled half's launch", half[..., ca:], o["oldw"][..., ca:])
        ran(K, G, "part skip", sym_s, lambda: K.conv2d_wgrad_part(d, dev(o["skip"]), ca, False, dev(o["dy"]), dw.t, True))
        G.exact("up-sampled channels after the skip half's launch", dw.host()[..., :ca], half[..., :ca])
        G.grade("wgrad of both halves accumulated", dw.host(), R.epilogue(o["wgrad"], old=o["oldw"]), False)
        outs = [dw]
        for family in FAMILIES:
            t = C.part_tier_b(case, family)
            e = Out(t["old"].shape, t["old"])
            ran(K, G, f"{family} part up", sym_a, lambda: K.conv2d_wgrad_part(d, dev(t["a"]), 0, True, dev(t["w"]), e.t, True))
            ran(K, G, f"{family} part skip", sym_s, lambda: K.conv2d_wgrad_part(d, dev(t["skip"]), ca, False, dev(t["w"]), e.t, True))
            exact(G, f"{family} wgrad of both halves accumulated", e.host(), t["r64"] + t["old"])
            outs.append(e)
    guards(G, "wgrad part", *outs)
    G.done()


@pytest.mark.parametrize("generic", (0, 1), ids=("uniform", "generic"))
@pytest.mark.parametrize("case", C.WG_PART, ids=["n%d_%dx%d_ca%d_cs%d_co%d" % c for c in C.WG_PART])
def test_wgrad_channel_slices(K, case, generic):
    """The two halves on conv_wgrad_kernel<64, 64, 2, 2, *> / <32, 128, 1, 4, *> (F32_SPLIT = 0)."""
    channel_slices(K, case, generic, 0)


@pytest.mark.parametrize("generic", (0, 1), ids=("uniform", "generic"))
@pytest.mark.parametrize("case", C.WG_PART_X3, ids=["n%d_%dx%d_ca%d_cs%d_co%d" % c for c in C.WG_PART_X3])
def test_wgrad_channel_slices_on_the_split(K, case, generic):
    """The two halves on conv_wgrad_x3_kernel<64, 64, 2, 2, *> (F32_SPLIT = 1): the up and c_off paths of its two gathers."""
    channel_slices(K, case, generic, 1)


# ======================================================================= 4. conv2d_fwd_fused on an X3 instance (F32_SPLIT = 1)
def test_fused_epilogue_on_the_split_instance(K):
    """The eval path's epilogue (bias + residual + ReLU) on conv_igemm_kernel<..., true>, with the split grade's bar and families."""
    case = C.X3_FUSED
    n, h, w, ci, co, k, s, p = case
    G = R.X3Grader(f"x3 fused {case}", _log)
    o = C.x3_fused_tier_a()
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    ig = ("conv_igemm_kernel<", ", true>")
    with options(K, F32_SPLIT=1):
        y = Out((n, d.ho, d.wo, co))
        ran_x3(K, G, "fwd fused", *ig, lambda: K.conv2d_fwd_fused(d, dev(o["x"]), dev(o["wt"]), dev(o["bias"]), dev(o["res"]), y.t, act=1, slope=0.0))
        G.grade("fwd + bias + residual + ReLU", y.host(), R.epilogue(o["fwd"], bias=o["bias"], residual=o["res"], slope=0.0), False)
        outs = [y]
        for family in FAMILIES:
            t = C.x3_fused_tier_b(family)
            e = Out((n, d.ho, d.wo, co))
            ran_x3(K, G, f"{family} fwd fused", *ig,
                   lambda: K.conv2d_fwd_fused(d, dev(t["x"]), dev(t["w"]), dev(t["bias"]), dev(t["res"]), e.t, act=1, slope=0.0))
            exact(G, f"{family} fwd + bias + residual + ReLU", e.host(), C.relu(t["r64"] + t["bias"] + t["res"]))
            outs.append(e)
    guards(G, "x3 fused", *outs)
    G.done()


# ================================================================================================================== 5. bn_fold
@pytest.mark.parametrize("case", C.BN_FOLD, ids=["c%d_var%g" % c for c in C.BN_FOLD])
def test_bn_fold(K, case):
    """w' = w gamma / sqrt(rv + eps), b' = beta + (bias - rm) gamma / sqrt(rv + eps) against float64, with the norm bar: 4 x the
    deviation of the fp32 restatement of the same formula, at least 2^-22, relative to the sum of the terms' absolute values."""
    import _norm_ref as N
    c, _ = case
    G = R.F32Grader(f"bn_fold {case}", _log)
    o = C.bn_fold_operands(case)
    args = (o["w"], o["bias"], o["gamma"], o["beta"], o["rm"], o["rv"], C.BN_EPS)
    w64, b64, bmag = R.bn_fold_ref(*args, F64)
    w32, b32, _ = R.bn_fold_ref(*args, F32)
    wf, bf = Out(o["w"].shape), Out((c,))
    K.bn_fold(*(dev(o[k]) for k in ("w", "bias", "gamma", "beta", "rm", "rv")), C.BN_EPS, wf.t, bf.t)
    torch.cuda.synchronize()
    for what, got, r64, leg, mag in (("folded weights", wf.host(), w64, w32, np.abs(w64)), ("folded bias", bf.host(), b64, b32, bmag)):
        A, dleg = N.bar(leg, r64, mag)
        e = float(N.normalised(got.astype(F64) - r64, mag).max(initial=0.0)) if np.isfinite(got).all() else np.inf
        G.note(what, e <= A, f"fp32 | e {e:.3e} d_rne {dleg:.3e} bar {A:.3e} e/bar {e / A:.3f}")
    guards(G, "bn_fold", wf, bf)
    G.done()
