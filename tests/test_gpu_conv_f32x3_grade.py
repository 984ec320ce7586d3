"""The fp32 convolutions on the three-term bf16 split (csrc/conv_halo_f32x3.hip, conv_up_f32x3.hip, conv_n16_f32x3.hip, conv_stem_f32x3.hip and the X3
instances of csrc/conv_igemm.hip, conv_wgrad.hip, conv_wgrad_halo2.hip) element-wise against float64, called at kernel level.  Cases,
operands and references live in tests/_conv_f32x3_cases.py and tests/_conv_ref.py; tests/test_conv_ref_host.py proves on the CPU,
for every case here, that tier A's bar rejects five mutants and that tier B's operands are exact.

Tier A (arbitrary fp32 operands): e = |kernel - f64| / magnitude element-wise (magnitude: the same operation on |x|, |w| plus |bias|,
|old| where they enter) against A = max(4 x max(d_rne, d_x3), 2^-22): d_rne is torch's fp32 CPU convolution / autograd, d_x3 the
six-product model of _conv_ref.x3_matmul (split3 terms, one truncation toward minus infinity per matrix instruction of 16 K-terms,
the negated groups truncating toward plus infinity), both against float64 over the whole output.  No tolerance comes from a kernel.
LeakyReLU is graded with the pre-activation's bar; the fused statistics go through stats_ref, the BatchNorm-backward sums through
bn_sums_ref.  Nothing is masked; every output is a slice of a larger allocation written over NaN, with a 256-element guard on
either side whose bits must survive.

Tier B (exact operands, three families that between them exercise all six products): every term is a multiple of one power of two
and mag / u <= 2^23, so a truncating adder has nothing to truncate and the kernel must equal float64 BIT FOR BIT; a missing or
mis-signed product shows in >= 1 % of the outputs (host test).

Measured (profiles/conv_f32x3_grade.txt): no kernel above 0.25 of tier A's bar (the model, one truncation per matrix instruction, is
about twice as pessimistic as the hardware), so the model needed no further term; tier B holds at the full window on both matrix
instructions (v_mfma_f32_32x32x16_bf16, v_mfma_f32_16x16x32_bf16), every check exact.

Every launch asserts from prof_kernels() that its own instantiation ran once and nothing else ran.  A launch its `_ok` query
refuses fails its test by name rather than falling back: tests/test_conv_ref_host.py restates the queries' arithmetic and proves
that none of the listed cases is refused.  Configurations 10, 11 and 12 of
launch_f3 run here for the first time under a test.  Set UDASEG_DEVIATION_LOG to a file name to collect the figures
(profiles/conv_f32x3_grade.txt).
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import _conv_f32x3_cases as C
import _conv_ref as R
from _conv_ref import F32, F64

pytestmark = pytest.mark.gpu
NAN = float("nan")
bf = torch.bfloat16
SLOPE = C.SLOPE
FAMILIES = sorted(R.FAMILIES)


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    kernels.prof_enable(1)
    try:
        yield kernels
    finally:
        kernels.prof_enable(0)


@contextlib.contextmanager
def options(K, **kv):
    try:
        for name, value in kv.items():
            K.set_option(name, value)
        yield
    finally:
        for name in kv:
            K.set_option(name, -1)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to("cuda", dtype)


class Out:
    """An output buffer: a slice (starting at a multiple of 64 elements) of a larger allocation, NaN or ``init`` inside, a
    256-element sentinel guard on either side."""
    def __init__(self, shape, init=None, dtype=torch.float32, fill=NAN):
        n = int(np.prod(shape))
        self.n, self.whole = n, torch.full((n + 2 * R.GUARD,), R.SENTINEL, device="cuda", dtype=dtype)
        self.t = self.whole[R.GUARD:R.GUARD + n].view(shape)
        assert self.t.data_ptr() % (64 * self.t.element_size()) == 0
        if init is None:
            self.t.fill_(fill)
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))

    def host(self):
        return self.t.detach().cpu().numpy()

    def intact(self):
        g = torch.cat([self.whole[:R.GUARD], self.whole[R.GUARD + self.n:]])
        return bool((g == R.SENTINEL).all())


def guards(G, what, *outs):
    G.note(what + " guards", all(o.intact() for o in outs), "256-element guards on either side " + ("intact" if all(o.intact() for o in outs) else "OVERWRITTEN"))


def ran(K, G, what, expect, launch):
    """Run one launch and assert from prof_kernels() that ``expect`` (a symbol, or a prefix ending in '<') ran exactly once and
    no other convolution symbol ran at all."""
    torch.cuda.synchronize()
    K.prof_reset()
    launch()
    torch.cuda.synchronize()
    counts = {name: n for name, _, _, n in K.prof_kernels() if n}
    hit = [name for name in counts if (name.startswith(expect) if expect.endswith("<") else name == expect)]
    G.note(what + " route", len(counts) == 1 and len(hit) == 1 and counts[hit[0]] == 1, f"expected {expect} x 1, ran {counts}")


def pack3(K, wt):
    """OHWI fp32 weights -> (forward planes, data-gradient planes) of the three-term fragment packing."""
    co, k, _, ci = wt.shape
    w32, wt32 = dev(wt), dev(wt.transpose(3, 1, 2, 0))
    nf, nd = 3 * K.frag_elems(co, ci, k), 3 * K.frag_elems(ci, co, k)
    packed = torch.full((nf + nd,), NAN, device="cuda", dtype=bf)
    K.pack_frag_batched(w32, wt32, packed, torch.tensor([[0, 0, 0, co, ci, k], [1, 0, nf, ci, co, k]], dtype=torch.int32, device="cuda"))
    assert torch.isfinite(packed.float()).all()
    return packed[:nf], packed[nf:]


def new_stats(K, c):
    return Out((K.bn_replicas() * 2 * c,), dtype=torch.float64, fill=0.0)


def totals(K, st):
    return st.t.view(K.bn_replicas(), 2, -1).sum(0).cpu().numpy()


def grade_stats(K, G, what, st, ref):
    tot = totals(K, st)
    s1, s2 = R.stats_ref(ref)
    G.grade(what + " sum", tot[0], s1, False)
    G.grade(what + " sum of squares", tot[1], s2, False)


def exact(G, what, got, r64):
    """Tier B's verdict: bit for bit the float64 result (which is an fp32 number)."""
    G.exact(what, np.asarray(got), np.asarray(r64).astype(F32))


# ======================================================================= 1. conv3x3_f32x3_kernel / conv3x3_f32x3_ws_kernel
def f3_tier_a(K, G, case):
    cfg, n, h, w, g, p, mode = case
    o = C.f3_tier_a(case)
    name = R.f3_symbol(cfg)
    # ---- forward g -> p: bias + statistics, bias + ReLU, bias + LeakyReLU
    d = K.conv_desc(n, h, w, g, p, 3, 1, 1)
    wf, _ = pack3(K, o["wt"])
    xd, bd = dev(o["x"]), dev(o["bias"])
    y, st, yr, yl = Out((n, h, w, p)), new_stats(K, p), Out((n, h, w, p)), Out((n, h, w, p))
    ran(K, G, "fwd bias stats", name, lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, y.t, stats=st.t))
    ran(K, G, "fwd relu", name, lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, yr.t, act=1, slope=0.0))
    ran(K, G, "fwd leaky", name, lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, yl.t, act=1, slope=SLOPE))
    ref = R.epilogue(o["fwd"], bias=o["bias"])
    G.grade("fwd + bias", y.host(), ref, False)
    grade_stats(K, G, "fwd fused", st, ref)
    G.grade("fwd + bias + ReLU", yr.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=0.0), False)
    G.grade("fwd + bias + LeakyReLU", yl.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=SLOPE), False)
    guards(G, "fwd", y, st, yr, yl)
    # ---- data gradient gathering g, producing p (the convolution p -> g): plain, accumulated, split, BatchNorm-backward sums
    d = K.conv_desc(n, h, w, p, g, 3, 1, 1)
    _, wfd = pack3(K, o["wd"])
    dyd = dev(o["dy"])
    dx, dxa, dxb, bs = Out((n, h, w, p)), Out((n, h, w, p), o["old"]), Out((n, h, w, p)), new_stats(K, p)
    bn = tuple(dev(o[k]) for k in ("prev_y", "mean", "rstd", "gamma", "beta")) + (1, SLOPE, bs.t)
    ran(K, G, "dgrad", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dx.t))
    ran(K, G, "dgrad accumulate", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dxa.t, accumulate=True))
    ran(K, G, "dgrad bn sums", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dxb.t, bn=bn))
    G.grade("dgrad", dx.host(), o["dgrad"], False)
    G.grade("dgrad accumulated", dxa.host(), R.epilogue(o["dgrad"], old=o["old"]), False)
    G.grade("dgrad with bn sums", dxb.host(), o["dgrad"], False)
    s1, s2, _ = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], SLOPE)
    tot = totals(K, bs)
    G.grade("bn-backward sum", tot[0], s1, False)
    G.grade("bn-backward sum with y_hat", tot[1], s2, False)
    outs = [dx, dxa, dxb, bs]
    if p > 32:
        da, db = Out((n, h, w, 32)), Out((n, h, w, p - 32))
        ran(K, G, "dgrad split", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, da.t, dx2=db.t))
        G.grade("dgrad split at 32", np.concatenate([da.host(), db.host()], axis=3), o["dgrad"], False)
        outs += [da, db]
    guards(G, "dgrad", *outs)


def f3_tier_b(K, G, case, family):
    cfg, n, h, w, g, p = case[:6]
    f, b = C.f3_tier_b(case, family)
    name = R.f3_symbol(cfg)
    d = K.conv_desc(n, h, w, g, p, 3, 1, 1)
    wf, _ = pack3(K, f["w"])
    y = Out((n, h, w, p))
    ran(K, G, f"{family} fwd", name, lambda: K.conv2d_fwd_frag(d, dev(f["x"]), None, wf, dev(f["bias"]), y.t, act=1, slope=0.0))
    exact(G, f"{family} fwd + bias + ReLU", y.host(), C.relu(f["r64"] + f["bias"]))
    d = K.conv_desc(n, h, w, p, g, 3, 1, 1)
    _, wfd = pack3(K, b["w"])
    dyd = dev(b["x"])
    dx, dxa = Out((n, h, w, p)), Out((n, h, w, p), b["old"])
    ran(K, G, f"{family} dgrad", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dx.t))
    ran(K, G, f"{family} dgrad accumulate", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dxa.t, accumulate=True))
    exact(G, f"{family} dgrad", dx.host(), b["r64"])
    exact(G, f"{family} dgrad accumulated", dxa.host(), b["r64"] + b["old"])
    outs = [y, dx, dxa]
    if p > 32:
        da, db = Out((n, h, w, 32)), Out((n, h, w, p - 32))
        ran(K, G, f"{family} dgrad split", name, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, da.t, dx2=db.t))
        exact(G, f"{family} dgrad split at 32", np.concatenate([da.host(), db.host()], axis=3), b["r64"])
        outs += [da, db]
    guards(G, family, *outs)


@pytest.mark.parametrize("case", C.F3_CASES, ids=[C.f3_id(c) for c in C.F3_CASES])
def test_f3_every_configuration(K, case):
    """Configurations 1 .. 12 of launch_f3, forward and data gradient with every epilogue term, both tiers (the 40-binade cases: tier
    A only)."""
    cfg, n, h, w, g, p, mode = case
    G = R.X3Grader(f"f3 cfg{cfg} {case[1:6]} {mode}", _log)
    d = K.conv_desc(n, h, w, g, p, 3, 1, 1)
    assert K.conv_frag_ok(d, f32=True) and K.conv_frag_ok(K.conv_desc(n, h, w, p, g, 3, 1, 1), dgrad=True, f32=True)
    with options(K, F3_CFG=cfg):
        f3_tier_a(K, G, case)
        if mode == "randn":
            for family in FAMILIES:
                f3_tier_b(K, G, case, family)
    if cfg >= 10:
        G.note(f"configuration {cfg}", not G.bad, "first run under a test: " + ("never wrong" if not G.bad else "WRONG: " + "; ".join(G.bad)))
    G.done()


@pytest.mark.parametrize("case", C.F3_BNIN, ids=[C.f3_id(c) for c in C.F3_BNIN])
def test_f3_in_staging_batchnorm_transform(K, case):
    """The `frag_bnin` route: act(fma(y, scale, shift)) applied while the halo is staged (the `..., true>` symbols)."""
    cfg, n, h, w, g, p = case
    G = R.X3Grader(f"f3 bnin cfg{cfg} {case[1:]}", _log)
    o = C.f3_bnin_a(case)
    name = R.f3_symbol(cfg, bnin=True)
    d = K.conv_desc(n, h, w, g, p, 3, 1, 1)
    assert K.conv_frag_ok(d, f32=True)
    wf, _ = pack3(K, o["wt"])
    with options(K, F3_CFG=cfg):
        y, st = Out((n, h, w, p)), new_stats(K, p)
        ran(K, G, "bnin fwd", name, lambda: K.conv2d_fwd_frag(d, dev(o["y_prev"]), None, wf, dev(o["bias"]), y.t, stats=st.t, in_scale=dev(o["sc"]),
                                                             in_shift=dev(o["sh"]), in_act=1, in_slope=SLOPE))
        ref = R.epilogue(o["fwd"], bias=o["bias"])
        G.grade("bnin fwd + bias", y.host(), ref, False)
        grade_stats(K, G, "bnin fwd fused", st, ref)
        outs = [y, st]
        one, zero = torch.ones(g, device="cuda"), torch.zeros(g, device="cuda")
        for family in FAMILIES:
            t = C.f3_bnin_b(case, family)
            wfb, _ = pack3(K, t["w"])
            yb = Out((n, h, w, p))
            ran(K, G, f"{family} bnin fwd", name, lambda: K.conv2d_fwd_frag(d, dev(t["x"]), None, wfb, dev(t["bias"]), yb.t, in_scale=one, in_shift=zero,
                                                                           in_act=1, in_slope=0.0))
            exact(G, f"{family} bnin fwd + bias", yb.host(), t["r64"] + t["bias"])
            outs.append(yb)
    guards(G, "bnin", *outs)
    G.done()


@pytest.mark.parametrize("case", C.F3_UP, ids=[C.up_id(c) for c in C.F3_UP])
def test_f3_fused_decoder_input(K, case):
    """up_ca: cat([nearest_x2(a), skip]) gathered while the halo is staged."""
    cfg, n, h, w, ca, cs, p = case
    G = R.X3Grader(f"f3 fused input cfg{cfg} {case[1:]}", _log)
    o = C.f3_up_a(case)
    name = R.f3_symbol(cfg)
    d = K.conv_desc(n, h, w, ca + cs, p, 3, 1, 1)
    assert K.conv_frag_ok(d, up_ca=ca, f32=True)
    wf, _ = pack3(K, o["wt"])
    with options(K, F3_CFG=cfg):
        y, st = Out((n, h, w, p)), new_stats(K, p)
        sd = dev(o["skip"]) if cs else None
        ran(K, G, "fused input fwd", name, lambda: K.conv2d_fwd_frag(d, dev(o["a"]), sd, wf, dev(o["bias"]), y.t, stats=st.t, up=True))
        ref = R.epilogue(o["fwd"], bias=o["bias"])
        G.grade("fused input fwd + bias", y.host(), ref, False)
        grade_stats(K, G, "fused input fwd", st, ref)
        outs = [y, st]
        for family in FAMILIES:
            t = C.f3_up_b(case, family)
            wfb, _ = pack3(K, t["w"])
            yb = Out((n, h, w, p))
            sb = dev(t["skip"]) if cs else None
            ran(K, G, f"{family} fused input fwd", name, lambda: K.conv2d_fwd_frag(d, dev(t["a"]), sb, wfb, dev(t["bias"]), yb.t, up=True))
            exact(G, f"{family} fused input fwd + bias", yb.host(), t["r64"] + t["bias"])
            outs.append(yb)
    guards(G, "fused input", *outs)
    G.done()


# ============================================================================== 3. the sixteen-wide tile (csrc/conv_n16_f32x3.hip)
def pack_n16(K, w_fwd=None, w_bwd=None):
    """OHWI weights -> the sixteen-wide packings: forward (16 produced channels), data gradient (16 input channels)."""
    rows, srcs, off, out = [], [None, None], 0, {}
    if w_fwd is not None:
        ci = w_fwd.shape[3]
        rows.append([4, 0, off, 16, ci, ci, 0, 0])
        srcs[0], out["fwd"] = dev(w_fwd), (off, K.n16_frag_elems(ci))
        off += out["fwd"][1]
    if w_bwd is not None:
        co = w_bwd.shape[0]
        rows.append([5, 0, off, 16, co, co, 0, 0])
        srcs[1], out["bwd"] = dev(w_bwd.transpose(3, 1, 2, 0)), (off, K.n16_frag_elems(co))
        off += out["bwd"][1]
    packed = torch.full((off,), NAN, device="cuda", dtype=bf)
    K.pack_up_batched(srcs[0], srcs[1], packed, torch.tensor(rows, dtype=torch.int32, device="cuda"))
    assert torch.isfinite(packed.float()).all()
    return {k: packed[o:o + n] for k, (o, n) in out.items()}


N16_PLAIN, N16_XF = "conv3x3_n16_f32x3_kernel<false>", "conv3x3_n16_f32x3_kernel<true>"


@pytest.mark.parametrize("case", C.N16, ids=["n%d_%dx%d_g%d" % c for c in C.N16])
def test_n16_forward_and_data_gradient(K, case):
    """conv2d_fwd_n16 (plain input, unwritten BatchNorm activation as input, statistics) and conv2d_dgrad_n16 (with and without the
    BatchNorm-backward sums) at every gathered count the launcher accepts."""
    n, h, w, g = case
    G = R.X3Grader(f"n16 {case}", _log)
    o = C.n16_tier_a(case)
    d, dd = K.conv_desc(n, h, w, g, 16, 3, 1, 1), K.conv_desc(n, h, w, 16, g, 3, 1, 1)
    if not (K.conv_n16_ok(d) and K.conv_n16_ok(dd, dgrad=True)):
        pytest.fail(f"conv_n16_ok refuses {case}")
    P = pack_n16(K, o["wt"], o["wd"])
    xd, dyd = dev(o["x"]), dev(o["dy"])
    y, st, yz, sz = Out((n, h, w, 16)), new_stats(K, 16), Out((n, h, w, 16)), new_stats(K, 16)
    ran(K, G, "fwd stats", N16_PLAIN, lambda: K.conv2d_fwd_n16(d, xd, P["fwd"], y.t, stats=st.t))
    ran(K, G, "fwd unwritten bn input", N16_XF, lambda: K.conv2d_fwd_n16(d, xd, P["fwd"], yz.t, stats=sz.t, in_scale=dev(o["sc"]), in_shift=dev(o["sh"]),
                                                                        in_act=1, in_slope=0.0))
    G.grade("fwd", y.host(), o["fwd"], False)
    grade_stats(K, G, "fwd fused", st, o["fwd"])
    G.grade("fwd behind the transform", yz.host(), o["fwd_z"], False)
    grade_stats(K, G, "fwd behind the transform fused", sz, o["fwd_z"])
    dx, dxb, bs = Out((n, h, w, 16)), Out((n, h, w, 16)), new_stats(K, 16)
    bn = tuple(dev(o[k]) for k in ("prev_y", "mean", "rstd", "gamma", "beta")) + (1, 0.0, bs.t)
    ran(K, G, "dgrad", N16_PLAIN, lambda: K.conv2d_dgrad_n16(dd, dyd, P["bwd"], dx.t))
    ran(K, G, "dgrad bn sums", N16_PLAIN, lambda: K.conv2d_dgrad_n16(dd, dyd, P["bwd"], dxb.t, bn=bn))
    G.grade("dgrad", dx.host(), o["dgrad"], False)
    G.grade("dgrad with bn sums", dxb.host(), o["dgrad"], False)
    s1, s2, _ = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], 0.0)
    tot = totals(K, bs)
    G.grade("bn-backward sum", tot[0], s1, False)
    G.grade("bn-backward sum with y_hat", tot[1], s2, False)
    outs = [y, st, yz, sz, dx, dxb, bs]
    one, zero = torch.ones(g, device="cuda"), torch.zeros(g, device="cuda")
    for family in FAMILIES:
        f, z, b = C.n16_tier_b(case, family)
        Pb = pack_n16(K, f["w"], b["w"])
        Pz = pack_n16(K, z["w"])
        yf, yzb, dxe = Out((n, h, w, 16)), Out((n, h, w, 16)), Out((n, h, w, 16))
        ran(K, G, f"{family} fwd", N16_PLAIN, lambda: K.conv2d_fwd_n16(d, dev(f["x"]), Pb["fwd"], yf.t))
        ran(K, G, f"{family} fwd transform", N16_XF, lambda: K.conv2d_fwd_n16(d, dev(z["x"]), Pz["fwd"], yzb.t, in_scale=one, in_shift=zero, in_act=1, in_slope=0.0))
        ran(K, G, f"{family} dgrad", N16_PLAIN, lambda: K.conv2d_dgrad_n16(dd, dev(b["x"]), Pb["bwd"], dxe.t))
        exact(G, f"{family} fwd", yf.host(), f["r64"])
        exact(G, f"{family} fwd behind relu(1 x + 0)", yzb.host(), z["r64"])
        exact(G, f"{family} dgrad", dxe.host(), b["r64"])
        outs += [yf, yzb, dxe]
    guards(G, "n16", *outs)
    G.done()


# ================================================================================================ 4. the stem (csrc/conv_stem_f32x3.hip)
@pytest.mark.parametrize("case", C.STEM, ids=["n%d_%dx%d" % c for c in C.STEM])
def test_stem_forward(K, case):
    """7x7 / stride 2 / pad 3, 3 channels padded to 4 (the 4th channel and its weights are NOT zero here) -> 64, with the statistics."""
    n, h, w = case
    G = R.X3Grader(f"stem {case}", _log)
    o = C.stem_tier_a(case)
    d = K.conv_desc(n, h, w, 4, 64, 7, 2, 3)
    if not K.conv_stem_ok(d):
        pytest.fail(f"conv_stem_ok refuses {case}")

    def pack(wt):
        packed = torch.full((K.STEM_FRAG_ELEMS,), NAN, device="cuda", dtype=bf)
        K.pack_up_batched(dev(wt), None, packed, torch.tensor([[8, 0, 0, 64, 4, 4, 0, 0]], dtype=torch.int32, device="cuda"))
        assert torch.isfinite(packed.float()).all()
        return packed

    y, st = Out((n, h // 2, w // 2, 64)), new_stats(K, 64)
    wf = pack(o["wt"])
    ran(K, G, "stem fwd stats", "conv_stem_f32x3_kernel", lambda: K.conv2d_fwd_stem(d, dev(o["x"]), wf, y.t, stats=st.t))
    G.grade("stem fwd", y.host(), o["fwd"], False)
    grade_stats(K, G, "stem fwd fused", st, o["fwd"])
    outs = [y, st]
    for family in FAMILIES:
        t = C.stem_tier_b(case, family)
        yb, wb = Out((n, h // 2, w // 2, 64)), pack(t["w"])
        ran(K, G, f"{family} stem fwd", "conv_stem_f32x3_kernel", lambda: K.conv2d_fwd_stem(d, dev(t["x"]), wb, yb.t))
        exact(G, f"{family} stem fwd", yb.host(), t["r64"])
        outs.append(yb)
    guards(G, "stem", *outs)
    G.done()


# ============================================================================ 5. the shared-source kernels with the split (F32_SPLIT = 1)
def ran_x3(K, G, what, prefix, suffix, launch):
    """As ran(), for a symbol known by its family and its X3 flag: one symbol with that prefix and suffix ran once, nothing else."""
    torch.cuda.synchronize()
    K.prof_reset()
    launch()
    torch.cuda.synchronize()
    counts = {name: n for name, _, _, n in K.prof_kernels() if n}
    hit = [name for name in counts if name.startswith(prefix) and name.endswith(suffix)]
    G.note(what + " route", len(counts) == 1 and len(hit) == 1 and counts[hit[0]] == 1, f"expected {prefix}...{suffix} x 1, ran {counts}")


@pytest.mark.parametrize("case", C.X3, ids=["n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c for c in C.X3])
def test_shared_source_split(K, case):
    """conv2d_fwd / conv2d_dgrad / conv2d_wgrad on fp32 tensors with F32_SPLIT = 1: conv_igemm_kernel<..., true> and
    conv_wgrad_x3_kernel<...> must be the symbols that ran."""
    n, h, w, ci, co, k, s, p = case
    G = R.X3Grader(f"x3 {case}", _log)
    o = C.x3_tier_a(case)
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    ig, wg = ("conv_igemm_kernel<", ", true>"), (R.wgrad_x3_plan(*case)[0], "")        # the generic or the row-uniform gather, by name

    def wpair(wt):
        wd = dev(wt)
        wtp = torch.full((ci, k, k, co), NAN, device="cuda")
        K.pack_dgrad_weights(d, wd, wtp)
        return wd, wtp

    with options(K, F32_SPLIT=1):
        wd, wtp = wpair(o["wt"])
        xd, dyd = dev(o["x"]), dev(o["dy"])
        y, yl, dx = Out((n, d.ho, d.wo, co)), Out((n, d.ho, d.wo, co)), Out((n, h, w, ci))
        dw, dwa = Out((co, k, k, ci)), Out((co, k, k, ci), o["oldw"])
        ran_x3(K, G, "fwd", *ig, lambda: K.conv2d_fwd(d, xd, wd, None, y.t))
        ran_x3(K, G, "fwd bias leaky", *ig, lambda: K.conv2d_fwd(d, xd, wd, dev(o["bias"]), yl.t, 1, SLOPE))
        ran_x3(K, G, "dgrad", *ig, lambda: K.conv2d_dgrad(d, dyd, wtp, dx.t))
        ran_x3(K, G, "wgrad", *wg, lambda: K.conv2d_wgrad(d, xd, dyd, dw.t))
        ran_x3(K, G, "wgrad accumulate", *wg, lambda: K.conv2d_wgrad(d, xd, dyd, dwa.t, True))
        G.grade("fwd", y.host(), o["fwd"], False)
        G.grade("fwd + bias + LeakyReLU", yl.host(), R.epilogue(o["fwd"], bias=o["bias"], slope=SLOPE), False)
        G.grade("dgrad", dx.host(), o["dgrad"], False)
        G.grade("wgrad over NaN", dw.host(), o["wgrad"], False)
        G.grade("wgrad accumulated", dwa.host(), R.epilogue(o["wgrad"], old=o["oldw"]), False)
        outs = [y, yl, dx, dw, dwa]
        for family in FAMILIES:
            f, b, g = C.x3_tier_b(case, family)
            yb, dxb, dwb = Out((n, d.ho, d.wo, co)), Out((n, h, w, ci)), Out((co, k, k, ci), g["old"])
            wf, _ = wpair(f["w"])
            _, wb = wpair(b["w"])
            ran_x3(K, G, f"{family} fwd", *ig, lambda: K.conv2d_fwd(d, dev(f["x"]), wf, dev(f["bias"]), yb.t, 1, 0.0))
            ran_x3(K, G, f"{family} dgrad", *ig, lambda: K.conv2d_dgrad(d, dev(b["x"]), wb, dxb.t))
            ran_x3(K, G, f"{family} wgrad accumulate", *wg, lambda: K.conv2d_wgrad(d, dev(g["x"]), dev(g["w"]), dwb.t, True))
            exact(G, f"{family} fwd + bias + ReLU", yb.host(), C.relu(f["r64"] + f["bias"]))
            exact(G, f"{family} dgrad", dxb.host(), b["r64"])
            exact(G, f"{family} wgrad accumulated", dwb.host(), g["r64"] + g["old"])
            outs += [yb, dxb, dwb]
    guards(G, "x3", *outs)
    G.done()


# ============================================================================================================ 6. weight gradients
H2, H2UP = "conv_wgrad_h2_kernel<", "conv_wgrad_up_kernel<"


def wg_launches(K, G, kind, case, launch, expect, rows=None, tag=""):
    """One weight-gradient entry point in both tiers.  launch(operands, dw tensor): dW += ...; rows: the channel slice of dW the
    launch owns (everything else must come back bit for bit)."""
    o = C.wg_tier_a(kind, case)
    old = o["oldw"]
    dw0, dwa = Out(old.shape, np.zeros_like(old)), Out(old.shape, old)
    ran(K, G, tag + "wgrad onto zeros", expect, lambda: launch(o, dw0.t))
    ran(K, G, tag + "wgrad accumulate", expect, lambda: launch(o, dwa.t))
    G.grade(tag + "wgrad onto zeros", dw0.host(), o["wgrad"], False)
    G.grade(tag + "wgrad accumulated", dwa.host(), R.epilogue(o["wgrad"], old=old), False)
    outs = [dw0, dwa]
    for family in FAMILIES:
        t = C.wg_tier_b(kind, case, family)
        dwb = Out(t["old"].shape, t["old"])
        ran(K, G, f"{tag}{family} wgrad accumulate", expect, lambda: launch(t, dwb.t))
        exact(G, f"{tag}{family} wgrad accumulated", dwb.host(), t["r64"] + t["old"])
        outs.append(dwb)
    guards(G, tag + "wgrad", *outs)


@pytest.mark.parametrize("case", C.WG_HALO, ids=["n%d_%dx%d_ci%d_co%d" % c for c in C.WG_HALO])
def test_wgrad_halo(K, case):
    n, h, w, ci, co = case
    G = R.X3Grader(f"wgrad halo {case}", _log)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    if not K.conv2d_wgrad_halo_ok(d, f32=True):
        pytest.fail(f"conv2d_wgrad_halo_ok refuses {case}")
    wg_launches(K, G, "halo", case, lambda o, dw: K.conv2d_wgrad_halo(d, dev(o["x"]), None, dev(o["w"] if "w" in o else o["dy"]), dw), H2)
    G.done()


@pytest.mark.parametrize("case", C.WG_HALO_UP, ids=["n%d_%dx%d_ca%d_cs%d_co%d" % c for c in C.WG_HALO_UP])
def test_wgrad_halo_fused_decoder_input(K, case):
    n, h, w, ca, cs, co = case
    G = R.X3Grader(f"wgrad halo fused input {case}", _log)
    d = K.conv_desc(n, h, w, ca + cs, co, 3, 1, 1)
    if not K.conv2d_wgrad_halo_ok(d, ca, f32=True):
        pytest.fail(f"conv2d_wgrad_halo_ok refuses {case}")
    wg_launches(K, G, "halo_up", case,
                lambda o, dw: K.conv2d_wgrad_halo(d, dev(o["a"]), dev(o["skip"]), dev(o["w"] if "w" in o else o["dy"]), dw, up=True), H2)
    G.done()


@pytest.mark.parametrize("case", C.WG_PAIR + C.WG_PAIR_UP, ids=["_".join(map(str, c)) for c in C.WG_PAIR + C.WG_PAIR_UP])
def test_wgrad_halo_pair_packed(K, case):
    """The two pair-packed forms of the halo-resident weight gradient under WGRAD_PAIR = 7: 16 gathered channels -> 8 .. 32, and 32
    up-sampled channels without a skip half -> 16 (conv_wgrad_h2_kernel<3, H2P<...>> / H2PU<...>)."""
    up = len(case) == 6
    n, h, w = case[:3]
    ci, co = (case[3] + case[4], case[5]) if up else case[3:5]
    G = R.X3Grader(f"wgrad halo pair-packed {case}", _log)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    with options(K, WGRAD_PAIR=7):
        if not K.conv2d_wgrad_halo_ok(d, ci if up else 0, f32=True):
            pytest.fail(f"conv2d_wgrad_halo_ok refuses {case}")
        name = "conv_wgrad_h2_kernel<3, udaseg::H2P" + ("U<" if up else "<")
        if up:
            wg_launches(K, G, "halo_up", case, lambda o, dw: K.conv2d_wgrad_halo(d, dev(o["a"]), None, dev(o["w"] if "w" in o else o["dy"]), dw, up=True), name)
        else:
            wg_launches(K, G, "halo", case, lambda o, dw: K.conv2d_wgrad_halo(d, dev(o["x"]), None, dev(o["w"] if "w" in o else o["dy"]), dw), name)
    G.done()


@pytest.mark.parametrize("case", C.WG_BNIN, ids=["n%d_%dx%d_ci%d_co%d" % c for c in C.WG_BNIN])
def test_wgrad_behind_an_unwritten_batchnorm_activation(K, case):
    """conv2d_wgrad_bnin: the gathered operand is act(fma(y, scale, shift)), applied while staging; both forms of the call (over
    NaN, accumulating)."""
    n, h, w, ci, co = case
    G = R.X3Grader(f"wgrad bnin {case}", _log)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    if not K.conv_bnin_ok(d):
        pytest.fail(f"conv_bnin_ok refuses {case}")
    o = C.wg_tier_a("bnin", case)
    one, zero = torch.ones(ci, device="cuda"), torch.zeros(ci, device="cuda")
    dw, dwa = Out(o["oldw"].shape), Out(o["oldw"].shape, o["oldw"])
    args = (dev(o["y_prev"]), dev(o["sc"]), dev(o["sh"]), 1, SLOPE, dev(o["dy"]))
    ran(K, G, "wgrad bnin", H2, lambda: K.conv2d_wgrad_bnin(d, *args, dw.t, False))
    ran(K, G, "wgrad bnin accumulate", H2, lambda: K.conv2d_wgrad_bnin(d, *args, dwa.t, True))
    G.grade("wgrad bnin over NaN", dw.host(), o["wgrad"], False)
    G.grade("wgrad bnin accumulated", dwa.host(), R.epilogue(o["wgrad"], old=o["oldw"]), False)
    outs = [dw, dwa]
    for family in FAMILIES:
        t = C.wg_tier_b("bnin", case, family)
        dwb = Out(t["old"].shape, t["old"])
        ran(K, G, f"{family} wgrad bnin accumulate", H2, lambda: K.conv2d_wgrad_bnin(d, dev(t["x"]), one, zero, 1, 0.0, dev(t["w"]), dwb.t, True))
        exact(G, f"{family} wgrad bnin accumulated", dwb.host(), t["r64"] + t["old"])
        outs.append(dwb)
    guards(G, "wgrad bnin", *outs)
    G.done()


@pytest.mark.parametrize("blocks", C.WG_UP_BLOCKS, ids=["default_blocks", "16_blocks", "600_blocks"])
@pytest.mark.parametrize("case", C.WG_UP, ids=["n%d_%dx%d_ca%d_cs%d_co%d" % c for c in C.WG_UP])
def test_wgrad_up_phase_form(K, case, blocks):
    """conv2d_wgrad_up: dW[..., :ca] += the weight gradient of conv3x3(nearest_x2(a)) from 16 phase taps at a's resolution; the
    channels of a skip half (cs > 0) belong to another launch and must come back untouched (their magnitude here is 0)."""
    n, h, w, ca, cs, co = case
    G = R.X3Grader(f"wgrad up {case} blocks{blocks}", _log)
    d = K.conv_desc(n, h, w, ca + cs, co, 3, 1, 1)
    if not K.conv2d_wgrad_up_ok(d, ca):
        pytest.fail(f"conv2d_wgrad_up_ok refuses {case}")
    with options(K, WGRAD_UP_BLOCKS=blocks):
        wg_launches(K, G, "up", case, lambda o, dw: K.conv2d_wgrad_up(d, dev(o["a"]), dev(o["w"] if "w" in o else o["dy"]), dw), H2UP)
    G.done()


@pytest.mark.parametrize("case", C.WG_SLICE, ids=["n%d_%dx%d_c%d_co%d_off%d_of%d" % c for c in C.WG_SLICE])
def test_wgrad_halo_slice(K, case):
    """conv2d_wgrad_halo_slice: the same kernel filling channels [c_off, c_off + c) of a wider layer's gradient; the other channels
    come back bit for bit."""
    n, h, w, c, co, c_off, ld = case
    G = R.X3Grader(f"wgrad halo slice {case}", _log)
    d = K.conv_desc(n, h, w, c, co, 3, 1, 1)
    if not K.conv2d_wgrad_halo_ok(d, f32=True):
        pytest.fail(f"conv2d_wgrad_halo_ok refuses the slice of {case}")
    o = C.wg_tier_a("halo", case[:5])
    rng = np.random.default_rng(C.seed_of("slice", case))

    def widen(ref_or_val, old):
        full = np.array(old, dtype=F64)
        full[..., c_off:c_off + c] += ref_or_val
        return full

    old = R.randn_f32(rng, (co, 3, 3, ld))
    zeros = np.zeros_like(old, dtype=F64)
    wide = R.Ref(widen(o["wgrad"].r64, old), widen(o["wgrad"].mag, np.abs(old)), (widen(o["wgrad"].leg_rne, zeros) + old).astype(F32),
                 (widen(o["wgrad"].leg_trunc, zeros) + old).astype(F32))
    dwa = Out(old.shape, old)
    ran(K, G, "slice wgrad accumulate", H2, lambda: K.conv2d_wgrad_halo_slice(d, dev(o["x"]), dev(o["dy"]), dwa.t, c_off))
    G.grade("slice wgrad accumulated", dwa.host(), wide, False)
    keep = np.ones(ld, dtype=bool)
    keep[c_off:c_off + c] = False
    G.exact("channels outside the slice", dwa.host()[..., keep], old[..., keep])
    outs = [dwa]
    for family in FAMILIES:
        t = C.wg_tier_b("halo", case[:5], family)
        oldb = R.small_ints(rng, old.shape)
        dwb = Out(old.shape, oldb)
        ran(K, G, f"{family} slice wgrad accumulate", H2, lambda: K.conv2d_wgrad_halo_slice(d, dev(t["x"]), dev(t["w"]), dwb.t, c_off))
        exact(G, f"{family} slice wgrad accumulated", dwb.host(), widen(t["r64"], oldb))
        outs.append(dwb)
    guards(G, "slice wgrad", *outs)
    G.done()


# ============================================================================= 2. the phase kernels (csrc/conv_up_f32x3.hip)
def pack_up(K, wt, ca):
    """OHWI weights [co][3][3][ca + cs] -> (forward, data-gradient) phase packings of the up-sampled half."""
    co, ci = wt.shape[0], wt.shape[3]
    n_uf, n_ub = 3 * K.frag_elems(co, ca, 4), 3 * K.frag_elems(ca, co, 4)
    packed = torch.full((n_uf + n_ub,), NAN, device="cuda", dtype=bf)
    rows = [[2, 0, 0, co, ca, ci, 0, 0], [3, 0, n_uf, ca, co, co, 0, 0]]
    K.pack_up_batched(dev(wt), dev(wt.transpose(3, 1, 2, 0)), packed, torch.tensor(rows, dtype=torch.int32, device="cuda"))
    assert torch.isfinite(packed.float()).all()
    return packed[:n_uf], packed[n_uf:]


@pytest.mark.parametrize("case", C.UP, ids=[C.up_id(c) for c in C.UP])
def test_phase_kernels(K, case):
    """conv_up_fwd_f32x3_kernel (overwriting, and accumulating with the statistics of the sum) and conv_up_dgrad_f32x3_kernel (plain,
    accumulating, with the BatchNorm-backward sums) under UP_CFG 1 .. 8.  r64 is the true operation on the original weights,
    conv3x3(nearest_x2(a)); the model runs on the oracle's pre-summed phase weights."""
    cfg, n, h, w, ca, cs, co = case
    G = R.X3Grader(f"up cfg{cfg} {case[1:]}", _log)
    d = K.conv_desc(n, h, w, ca + cs, co, 3, 1, 1)
    if not K.conv_up_ok(d, ca):
        pytest.fail(f"conv_up_ok refuses {case}")
    o = C.up_tier_a(case)
    name_f, name_d = R.up_tile(cfg, False)[3], R.up_tile(cfg, True)[3]
    ha, wa = h // 2, w // 2
    with options(K, UP_CFG=cfg):
        pf, pb = pack_up(K, o["wt"], ca)
        ad, dyd = dev(o["a"]), dev(o["dy"])
        y, ya, st = Out((n, h, w, co)), Out((n, h, w, co), o["old"]), new_stats(K, co)
        ran(K, G, "fwd", name_f, lambda: K.conv2d_fwd_up(d, ad, pf, y.t))
        ran(K, G, "fwd accumulate stats", name_f, lambda: K.conv2d_fwd_up(d, ad, pf, ya.t, accumulate=True, stats=st.t))
        G.grade("fwd", y.host(), o["fwd"], False)
        acc = R.epilogue(o["fwd"], old=o["old"])
        G.grade("fwd accumulated", ya.host(), acc, False)
        grade_stats(K, G, "fwd accumulated fused", st, acc)
        da, daa, dab, bs = Out((n, ha, wa, ca)), Out((n, ha, wa, ca), o["olda"]), Out((n, ha, wa, ca)), new_stats(K, ca)
        bn = tuple(dev(o[k]) for k in ("prev_y", "mean", "rstd", "gamma", "beta")) + (1, SLOPE, bs.t)
        ran(K, G, "dgrad", name_d, lambda: K.conv2d_dgrad_up(d, dyd, ca, pb, da.t))
        ran(K, G, "dgrad accumulate", name_d, lambda: K.conv2d_dgrad_up(d, dyd, ca, pb, daa.t, accumulate=True))
        ran(K, G, "dgrad bn sums", name_d, lambda: K.conv2d_dgrad_up(d, dyd, ca, pb, dab.t, bn=bn))
        G.grade("dgrad", da.host(), o["dgrad"], False)
        G.grade("dgrad accumulated", daa.host(), R.epilogue(o["dgrad"], old=o["olda"]), False)
        G.grade("dgrad with bn sums", dab.host(), o["dgrad"], False)
        s1, s2, _ = R.bn_sums_ref(o["dgrad"], o["prev_y"], o["mean"], o["rstd"], o["gamma"], o["beta"], SLOPE)
        tot = totals(K, bs)
        G.grade("bn-backward sum", tot[0], s1, False)
        G.grade("bn-backward sum with y_hat", tot[1], s2, False)
        outs = [y, ya, st, da, daa, dab, bs]
        for family in FAMILIES:
            f, b = C.up_tier_b(case, family)
            pff, _ = pack_up(K, C.widen_up(f["w"], cs), ca)
            _, pbb = pack_up(K, C.widen_up(b["w"], cs), ca)
            yb, dae = Out((n, h, w, co), f["old"]), Out((n, ha, wa, ca), b["old"])
            ran(K, G, f"{family} fwd accumulate", name_f, lambda: K.conv2d_fwd_up(d, dev(f["a"]), pff, yb.t, accumulate=True))
            ran(K, G, f"{family} dgrad accumulate", name_d, lambda: K.conv2d_dgrad_up(d, dev(b["x"]), ca, pbb, dae.t, accumulate=True))
            exact(G, f"{family} fwd accumulated", yb.host(), f["r64"] + f["old"])
            exact(G, f"{family} dgrad accumulated", dae.host(), b["r64"] + b["old"])
            outs += [yb, dae]
    guards(G, "up", *outs)
    G.done()
