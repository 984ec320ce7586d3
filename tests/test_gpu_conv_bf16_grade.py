"""The bf16-storage convolutions (csrc/conv_halo_bf16.hip: the halo kernel's 3x3, 1x1 and 4x4 / stride 2 instances, the 1x1 streamer
and GEMM kernel; the bf16 instances of csrc/conv_igemm.hip, csrc/conv_wgrad.hip and csrc/conv_wgrad_halo2.hip) element-wise against
the float64 restatement of tests/_conv_ref.py (proven on the CPU by tests/test_conv_ref_host.py), called at kernel level.

The bar is the one of tests/test_gpu_norm_grade.py with two legs: with e = |kernel - f64| / magnitude element-wise (magnitude: the
same convolution on |x|, |w| plus |bias|, |residual|, |old| where they enter), A = max(4 x max(d_rne, d_trunc), 2^-22) where d_rne is
torch's fp32 CPU convolution and d_trunc an fp32 accumulator truncated toward minus infinity after every 16 terms, both measured
against float64 over the whole output.  fp32 outputs: |got - r64| <= A mag; bf16 outputs: |got - r64| <= A mag + half a bf16 ulp of
r64 -- ONE rounding, also for the accumulating calls: conv_halo_bf16_kernel adds ``old`` to the fp32 value ahead of pack_bf16x2, and
the generic epilogue of conv_igemm_kernel (the only one an accumulating launch takes: fast_epi and lds_epi both need !accumulate)
does ``val += (float)*dst; *dst = (__bf16)val``, so conv2d_dgrad_bf16 rounds once as well.  Nothing is masked; outputs are written
over NaN.  The fused BatchNorm statistics are graded as fp32 outputs against sum r64 / sum r64^2 (see _conv_ref.stats_ref).

Every forced route asserts, from prof_kernels(), that its own instantiation ran once and no other convolution symbol ran: a forced
configuration that silently falls back fails.  Switches are set through set_option inside try / finally and restored to -1.
Where a data gradient is graded on a halo instance, the case's (gathered, produced) channels are those of the LAUNCH: the forward
runs ci = gathered, co = produced and the data gradient ci = produced, co = gathered, so that both reach the same instantiation.

Set UDASEG_DEVIATION_LOG to a file name to collect the figures (profiles/conv_bf16_grade.txt).
"""
import contextlib
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import _conv_ref as R
from _conv_ref import F32, F64

pytestmark = pytest.mark.gpu
NAN = float("nan")
bf = torch.bfloat16
SLOPE = float(F32(0.2))


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


def dev(a, dtype=bf):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to("cuda", dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def nan_out(shape, dtype=bf):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


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


def operands(rng, n, h, w, ci, co, k, mode, ho=None, wo=None):
    """x, OHWI weights scaled by 1 / sqrt(K), bias, dy.  mode 'binades': operands over 20 binades; 'zero': an all-zero block of
    gathered channels and an all-zero weight row of the last produced channel."""
    b = mode == "binades"
    x = R.randn_bf16(rng, (n, h, w, ci), binades=b)
    wt = R.randn_bf16(rng, (co, k, k, ci), (ci * k * k) ** -0.5, binades=b)
    bias = rng.standard_normal(co).astype(F32)
    dy = R.randn_bf16(rng, (n, ho or h, wo or w, co), binades=b)
    if mode == "zero":
        x[..., :max(ci // 2, 1)] = 0
        wt[co - 1] = 0
    return x, wt, bias, dy


def pack(K, wt):
    """OHWI weights -> (forward fragments, data-gradient fragments) through the batched packer."""
    co, k, _, ci = wt.shape
    w16, wt16 = dev(wt), dev(wt.transpose(3, 1, 2, 0))
    nf, nd = K.frag_elems(co, ci, k), K.frag_elems(ci, co, k)
    packed = nan_out((nf + nd,))
    K.pack_frag_batched(w16, wt16, packed, torch.tensor([[0, 0, 0, co, ci, k], [1, 0, nf, ci, co, k]], dtype=torch.int32, device="cuda"))
    return packed[:nf], packed[nf:]


def pack_s2(K, wt):
    """[co][4][4][ci] -> (forward fragments over the 4 ci phase-major channels, the four parity classes' data-gradient fragments)."""
    co, k, _, ci = wt.shape
    w16, wt16 = dev(wt), dev(wt.transpose(3, 1, 2, 0))
    nf, fe = K.frag_elems(co, 4 * ci, 2), K.frag_elems(ci, co, 2)
    packed = nan_out((nf + 4 * fe,))
    rows = [[2, 0, 0, co, ci, 4]] + [[3 + e, 0, nf + e * fe, ci, co, 4] for e in range(4)]
    K.pack_frag_batched(w16, wt16, packed, torch.tensor(rows, dtype=torch.int32, device="cuda"))
    assert torch.isfinite(packed.float()).all()
    return packed[:nf], packed[nf:]


def new_stats(K, co):
    return torch.zeros(K.bn_replicas() * 2 * co, dtype=torch.float64, device="cuda")


def grade_stats(K, G, what, st, ref):
    tot = st.view(K.bn_replicas(), 2, -1).sum(0).cpu().numpy()
    s1, s2 = R.stats_ref(ref)
    G.grade(what + " sum", tot[0], s1, False)
    G.grade(what + " sum of squares", tot[1], s2, False)


# ================================================================================================ the halo entry points, stride 1
def frag_suite(K, G, k, n, h, w, g, p, mode, names):
    """Every launch form of conv2d_fwd_frag / conv2d_dgrad_frag at one geometry.  names: the expected symbol per launch form
    ('fwd', 'f32', 'dgrad', 'split'); a missing form is not launched."""
    rng = np.random.default_rng(seed_of("frag", k, n, h, w, g, p, mode))
    pad = k // 2
    if "fwd" in names or "f32" in names:
        x, wt, bias, _ = operands(rng, n, h, w, g, p, k, mode)
        d = K.conv_desc(n, h, w, g, p, k, 1, pad)
        assert K.conv_frag_ok(d)
        wf, _ = pack(K, wt)
        xd, bd = dev(x), dev(bias, torch.float32)
        base = R.fwd(x, wt, 1, pad)
        if "fwd" in names:
            y, st = nan_out((n, h, w, p)), new_stats(K, p)
            ran(K, G, "fwd bias stats", names["fwd"], lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, y, stats=st))
            ref = R.epilogue(base, bias=bias)
            G.grade("fwd + bias -> bf16", host(y), ref, True)
            grade_stats(K, G, "fwd fused", st, ref)
        if "f32" in names:
            y32 = nan_out((n, h, w, p), torch.float32)
            ran(K, G, "fwd leaky fp32", names["f32"], lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, y32, act=1, slope=SLOPE))
            G.grade("fwd + bias + LeakyReLU -> fp32", host(y32), R.epilogue(base, bias=bias, slope=SLOPE), False)
            if mode == "zero":
                G.exact("zero weight row: fp32 output == act(bias)", host(y32)[..., p - 1], np.broadcast_to(R.leaky(bias[p - 1:], SLOPE, F32), (n, h, w)))
    if "dgrad" in names:
        # the launch gathers dy (g channels) and produces dx (p channels): the convolution p -> g
        _, wt, _, dy = operands(rng, n, h, w, p, g, k, "randn" if mode == "zero" else mode)
        if mode == "zero":
            dy[..., :max(g // 2, 1)] = 0
            wt[..., p - 1] = 0                       # input channel p - 1 reaches no output: its gradient is exactly 0
        d = K.conv_desc(n, h, w, p, g, k, 1, pad)
        assert K.conv_frag_ok(d, dgrad=True)
        _, wfd = pack(K, wt)
        dyd = dev(dy)
        base = R.dgrad(dy, wt, 1, pad, h, w)
        dx = nan_out((n, h, w, p))
        ran(K, G, "dgrad", names["dgrad"], lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dx))
        G.grade("dgrad -> bf16", host(dx), base, True)
        old = R.randn_bf16(rng, (n, h, w, p), binades=mode == "binades")
        dxa = dev(old)
        ran(K, G, "dgrad accumulate", names["dgrad"], lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dxa, accumulate=True))
        G.grade("dgrad accumulated onto bf16 (one rounding)", host(dxa), R.epilogue(base, old=old), True)
        if "split" in names:
            s = 32 if p < 128 else (p // 2) // 32 * 32
            da, db = nan_out((n, h, w, s)), nan_out((n, h, w, p - s))
            ran(K, G, "dgrad split", names["split"], lambda: K.conv2d_dgrad_frag(d, dyd, wfd, da, dx2=db))
            G.grade(f"dgrad split at {s} -> bf16", np.concatenate([host(da), host(db)], axis=3), base, True)


def names3(g, p, cfg=0):
    name = R.halo_instance(3, g, p, cfg)
    out = {"fwd": name, "f32": name, "dgrad": name}
    if p > 32:
        out["split"] = name
    return out


# (HALO_CFG, (n, h, w, gathered, produced), operands)
HALO3 = [(0, (3, 9, 33, 16, 24), "randn"), (0, (1, 9, 33, 48, 8), "randn"), (0, (1, 9, 33, 48, 40), "randn"),
         (1, (3, 9, 33, 32, 24), "randn"), (2, (3, 9, 33, 64, 72), "randn"), (3, (1, 9, 33, 64, 136), "randn"),
         (4, (3, 17, 18, 32, 72), "randn"), (5, (1, 17, 18, 64, 136), "randn"), (6, (3, 9, 18, 32, 72), "randn"),
         (6, (2, 16, 16, 512, 64), "randn"),
         (2, (3, 9, 33, 64, 72), "binades"), (6, (3, 9, 18, 32, 72), "binades"), (3, (1, 9, 33, 64, 136), "zero"), (6, (3, 9, 18, 32, 72), "zero")]


@pytest.mark.parametrize("cfg,shape,mode", HALO3, ids=["cfg%d-n%d_%dx%d_g%d_p%d-%s" % ((c,) + s + (m,)) for c, s, m in HALO3])
def test_halo_3x3_every_instance(K, cfg, shape, mode):
    """All eight 3x3 instances of launch_halo: the two 16-channel-chunk ones by their channel counts, the six 32-channel-chunk ones
    through HALO_CFG (4, 5, 6: the 16-pixel-wide tiles); one full tile plus a ragged one in each axis, a ragged channel block; a
    K loop of 4608 terms; operands over 20 binades; zero magnitudes."""
    n, h, w, g, p = shape
    G = R.Grader(f"halo3x3 cfg{cfg} {shape} {mode}", _log)
    names = names3(g, p, cfg)
    if p % 32 and cfg:
        # the data gradient of the forward's own layer gathers p channels: chunks of 16, so a forced 16-wide tile must fall back -- by name
        assert R.halo_instance(3, p, g, cfg) != R.halo_instance(3, g, p, cfg)
    with options(K, HALO_CFG=cfg) if cfg else contextlib.nullcontext():
        frag_suite(K, G, 3, n, h, w, g, p, mode, names)
    G.done()


UPCAT = [(2, (1, 10, 34, 32, 32, 72)), (2, (1, 10, 34, 16, 48, 72)), (6, (1, 10, 18, 32, 32, 72)), (6, (1, 10, 18, 48, 16, 72)),
         (4, (1, 18, 18, 32, 64, 40))]


@pytest.mark.parametrize("cfg,shape", UPCAT, ids=["cfg%d-n%d_%dx%d_ca%d_cb%d_co%d" % ((c,) + s) for c, s in UPCAT])
def test_halo_3x3_fused_decoder_input(K, cfg, shape):
    """up=True: cat([nearest_x2(a), skip]) gathered while staging, per tile width, with sources that are multiples of 32 channels
    (chunks of 32) and of 16 only (chunks of 16: the 16-wide tiles have no such instance and the launcher falls back -- by name)."""
    n, h, w, ca, cb, co = shape
    rng = np.random.default_rng(seed_of("upcat", cfg, shape))
    G = R.Grader(f"halo3x3 fused input cfg{cfg} {shape}", _log)
    a, skip = R.randn_bf16(rng, (n, h // 2, w // 2, ca)), R.randn_bf16(rng, (n, h, w, cb))
    wt = R.randn_bf16(rng, (co, 3, 3, ca + cb), (9 * (ca + cb)) ** -0.5)
    bias = rng.standard_normal(co).astype(F32)
    d = K.conv_desc(n, h, w, ca + cb, co, 3, 1, 1)
    assert K.conv_frag_ok(d, up_ca=ca)
    wf, _ = pack(K, wt)
    name = R.halo_instance(3, ca + cb, co, cfg, up=(ca, cb))
    assert ("16>" in name) == (cfg > 3 and ca % 32 == 0 and cb % 32 == 0)
    ad, sd, bd = dev(a), dev(skip), dev(bias, torch.float32)
    ref = R.epilogue(R.fwd_upcat(a, skip, wt), bias=bias)
    y, st = nan_out((n, h, w, co)), new_stats(K, co)
    y32 = nan_out((n, h, w, co), torch.float32)
    with options(K, HALO_CFG=cfg):
        ran(K, G, "fused input fwd", name, lambda: K.conv2d_fwd_frag(d, ad, sd, wf, bd, y, stats=st, up=True))
        ran(K, G, "fused input fwd fp32", name, lambda: K.conv2d_fwd_frag(d, ad, sd, wf, bd, y32, up=True))
    G.grade("fused input fwd + bias -> bf16", host(y), ref, True)
    grade_stats(K, G, "fused input fwd", st, ref)
    G.grade("fused input fwd + bias -> fp32", host(y32), ref, False)
    G.done()


# ====================================================================================================== halo kernel, 4x4 / stride 2
S2 = [((2, 18, 66, 8, 64), 64, "rgb"), ((1, 18, 66, 16, 72), 64, "randn"), ((1, 18, 66, 64, 136), 64, "randn"), ((1, 10, 34, 128, 64), 64, "randn"),
      ((1, 18, 66, 64, 136), 32, "randn"), ((1, 10, 34, 128, 64), 32, "randn"), ((1, 10, 34, 128, 64), 64, "binades")]


@pytest.mark.parametrize("shape,ck,mode", S2, ids=["n%d_%dx%d_ci%d_co%d-ck%d-%s" % (s + (c, m)) for s, c, m in S2])
def test_halo_4x4_stride2(K, shape, ck, mode):
    """The four 2x2-window instances (chunks of 64 virtual channels; of 32 with 8 real channels or HALO_S2_CK = 32; 64 or 128 output
    channels per block): forward with bias + LeakyReLU and with the statistics, the data gradient's four parity classes in one
    launch and its accumulating form.  'rgb': channels 3..7 of the image and of the weights are zero, so those channels of the data
    gradient have magnitude 0 and must be exactly 0.  The data gradient stages whole chunks of 32 of ITS gathered
    channels (co): where 32 does not divide co the query must say no (it said yes and the launch failed until this test existed)."""
    n, h, w, ci, co = shape
    rng = np.random.default_rng(seed_of("s2", shape, ck, mode))
    G = R.Grader(f"halo4x4s2 {shape} ck{ck} {mode}", _log)
    x, wt, bias, dy = operands(rng, n, h, w, ci, co, 4, mode, h // 2, w // 2)
    if mode == "rgb":
        x[..., 3:], wt[..., 3:] = 0, 0           # an RGB image in 8 physical channels: the data gradient of channels 3..7 has magnitude 0
    d = K.conv_desc(n, h, w, ci, co, 4, 2, 1)
    assert (d.ho, d.wo) == (h // 2, w // 2) and K.conv_frag_ok(d)
    wf, wfd = pack_s2(K, wt)
    xd, bd, dyd = dev(x), dev(bias, torch.float32), dev(dy)
    base = R.fwd(x, wt, 2, 1)
    y, st = nan_out((n, d.ho, d.wo, co)), new_stats(K, co)
    ya = nan_out((n, d.ho, d.wo, co))
    dx = nan_out((n, h, w, ci))
    old = R.randn_bf16(rng, (n, h, w, ci), binades=mode == "binades")
    dxa = dev(old)
    name_f, name_d = R.halo_instance(4, 4 * ci, co, s2_ck=ck), R.halo_instance(4, co, ci, s2_ck=ck)
    dgrad_ok = co % 32 == 0
    G.note("data-gradient query", K.conv_frag_ok(d, dgrad=True) == dgrad_ok, f"conv_frag_ok(dgrad) for co = {co}: expected {dgrad_ok}")
    with options(K, HALO_S2_CK=ck):
        ran(K, G, "fwd stats", name_f, lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, y, stats=st))
        ran(K, G, "fwd leaky", name_f, lambda: K.conv2d_fwd_frag(d, xd, None, wf, bd, ya, act=1, slope=SLOPE))
        if dgrad_ok:
            ran(K, G, "dgrad", name_d, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dx))
            ran(K, G, "dgrad accumulate", name_d, lambda: K.conv2d_dgrad_frag(d, dyd, wfd, dxa, accumulate=True))
    ref = R.epilogue(base, bias=bias)
    G.grade("fwd + bias -> bf16", host(y), ref, True)
    grade_stats(K, G, "fwd fused", st, ref)
    G.grade("fwd + bias + LeakyReLU -> bf16", host(ya), R.epilogue(base, bias=bias, slope=SLOPE), True)
    if dgrad_ok:
        dref = R.dgrad(dy, wt, 2, 1, h, w)
        G.grade("dgrad (four parity classes) -> bf16", host(dx), dref, True)
        G.grade("dgrad accumulated onto bf16 (one rounding)", host(dxa), R.epilogue(dref, old=old), True)
    G.done()


# ================================================================================================================== 1x1 / stride 1
STREAM = [(px, gp) for px in ((1, 7, 37), (1, 7, 9)) for gp in ((64, 72), (64, 40), (16, 136), (48, 24))]


@pytest.mark.parametrize("px,gp", STREAM, ids=["%dx%dx%d-g%d_p%d" % (a + b) for a, b in STREAM])
def test_1x1_streamer(K, px, gp):
    """conv1x1_stream_bf16_kernel<64 | 16, 2 | 4, 4 | 2> at 259 pixels (two 256-pixel flat tiles, the second ragged) and at 63."""
    (n, h, w), (g, p) = px, gp
    G = R.Grader(f"1x1 streamer {px} {gp}", _log)
    name = R.stream_instance(g, p)
    frag_suite(K, G, 1, n, h, w, g, p, "randn", {"fwd": name, "dgrad": name})
    G.done()


def test_1x1_streamer_over_twenty_binades_and_zero_magnitudes(K):
    G = R.Grader("1x1 streamer operands", _log)
    frag_suite(K, G, 1, 1, 7, 37, 64, 72, "binades", {"fwd": R.stream_instance(64, 72), "dgrad": R.stream_instance(64, 72)})
    frag_suite(K, G, 1, 1, 7, 37, 64, 72, "zero", {"fwd": R.stream_instance(64, 72), "dgrad": R.stream_instance(64, 72)})
    G.done()


GEMM = [(t, s) for t in (128, 256) for s in ((1, 7, 37, 128, 128), (1, 3, 43, 512, 192))]


@pytest.mark.parametrize("tile,shape", GEMM, ids=["tile%d-n%d_%dx%d_g%d_p%d" % ((t,) + s) for t, s in GEMM])
def test_1x1_gemm_kernel(K, tile, shape):
    """conv1x1_gemm_bf16_kernel<1 | 2> (128- / 256-pixel tiles x 128 channels) through GEMM_1X1_TILE at 259 and 129 pixels: the last
    pixel tile is ragged at both sizes; 192 produced channels: a ragged channel tile."""
    n, h, w, g, p = shape
    G = R.Grader(f"1x1 gemm tile{tile} {shape}", _log)
    name = "conv1x1_gemm_bf16_kernel<%d>" % (1 if tile == 128 else 2)
    with options(K, GEMM_1X1_TILE=tile):
        frag_suite(K, G, 1, n, h, w, g, p, "randn", {"fwd": name, "dgrad": name})
    G.done()


TILE1 = [(64, 136), (64, 40), (48, 24), (32, 136), (96, 40)]


@pytest.mark.parametrize("g,p", TILE1, ids=["g%d_p%d" % c for c in TILE1])
def test_1x1_tile_instances(K, g, p):
    """The five 1x1 instances of the halo kernel (chunks of 64, 32 and 16 channels; 64 or 128 produced channels per block): bf16 output
    under NO_STREAM = 1, and fp32 output, which the streamer does not take."""
    G = R.Grader(f"1x1 tile g{g} p{p}", _log)
    name = R.halo_instance(1, g, p)
    with options(K, NO_STREAM=1):
        frag_suite(K, G, 1, 1, 9, 33, g, p, "randn", {"fwd": name, "dgrad": name})
    frag_suite(K, G, 1, 1, 9, 33, g, p, "randn", {"f32": name})
    G.done()


# ======================================================================================== the shared implicit-GEMM source, bf16
IGEMM = [(2, 9, 7, 64, 72, 3, 1, 1), (2, 16, 16, 64, 128, 3, 2, 1), (2, 16, 16, 64, 128, 1, 2, 0), (2, 32, 32, 8, 64, 7, 2, 3),
         (2, 32, 32, 8, 64, 4, 2, 1)]


@functools.lru_cache(maxsize=None)
def igemm_case(case, mode="randn"):
    n, h, w, ci, co, k, s, p = case
    rng = np.random.default_rng(seed_of("igemm", case, mode))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x, wt, bias, dy = operands(rng, n, h, w, ci, co, k, mode, ho, wo)
    if mode == "zero":
        dy[..., co - 1] = 0
    res = R.randn_bf16(rng, (n, ho, wo, co), binades=mode == "binades")
    old = R.randn_bf16(rng, (n, h, w, ci), binades=mode == "binades")
    oldw = rng.standard_normal((co, k, k, ci)).astype(F32)
    return dict(x=x, wt=wt, bias=bias, dy=dy, res=res, old=old, oldw=oldw, fwd=R.fwd(x, wt, s, p), dgrad=R.dgrad(dy, wt, s, p, h, w),
                wgrad=R.wgrad(x, dy, k, s, p))


def igemm_names(case, tile, generic, no_fold=False):
    """(forward symbol, data-gradient symbol) of conv2d_fwd_bf16 / conv2d_dgrad_bf16."""
    n, h, w, ci, co, k, s, p = case
    out = []
    for g, pr in ((ci, co), (co, ci)):
        f = R.fold_factor(g, pr, w, no_fold) if (k, s, p) == (3, 1, 1) else 1
        g, pr = g * f, pr * f
        t = tile or (3 if pr > 32 else 4)
        out.append(R.igemm_instance(t, R.igemm_uniform(g, k * k, generic)))
    return out


def igemm_launches(K, G, case, tile, generic, no_fold=False, mode="randn", epilogues=False, tag=""):
    n, h, w, ci, co, k, s, p = case
    c = igemm_case(case, mode)
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    name_f, name_d = igemm_names(case, tile, generic, no_fold)
    xd, wd, bd, dyd = dev(c["x"]), dev(c["wt"]), dev(c["bias"], torch.float32), dev(c["dy"])
    wtd = dev(c["wt"].transpose(3, 1, 2, 0))
    y, st = nan_out((n, d.ho, d.wo, co)), new_stats(K, co)
    ran(K, G, tag + "fwd bias stats", name_f, lambda: K.conv2d_fwd_bf16(d, xd, wd, bd, None, y, stats=st))
    ref = R.epilogue(c["fwd"], bias=c["bias"])
    G.grade(tag + "fwd + bias -> bf16", host(y), ref, True)
    grade_stats(K, G, tag + "fwd fused", st, ref)
    dx = nan_out((n, h, w, ci))
    ran(K, G, tag + "dgrad", name_d, lambda: K.conv2d_dgrad_bf16(d, dyd, wtd, dx))
    G.grade(tag + "dgrad -> bf16", host(dx), c["dgrad"], True)
    if epilogues:
        y3 = nan_out((n, d.ho, d.wo, co))
        ran(K, G, tag + "fwd residual relu", name_f, lambda: K.conv2d_fwd_bf16(d, xd, wd, None, dev(c["res"]), y3, act=1, slope=0.0))
        G.grade(tag + "fwd + residual + ReLU -> bf16", host(y3), R.epilogue(c["fwd"], residual=c["res"], slope=0.0), True)
        y32 = nan_out((n, d.ho, d.wo, co), torch.float32)
        ran(K, G, tag + "fwd leaky fp32", name_f, lambda: K.conv2d_fwd_bf16(d, xd, wd, bd, None, y32, act=1, slope=SLOPE))
        G.grade(tag + "fwd + bias + LeakyReLU -> fp32", host(y32), R.epilogue(c["fwd"], bias=c["bias"], slope=SLOPE), False)
        dxa = dev(c["old"])
        ran(K, G, tag + "dgrad accumulate", name_d, lambda: K.conv2d_dgrad_bf16(d, dyd, wtd, dxa, accumulate=True))
        G.grade(tag + "dgrad accumulated onto bf16 (one rounding)", host(dxa), R.epilogue(c["dgrad"], old=c["old"]), True)
        if mode == "zero":
            G.exact(tag + "zero weight row: fp32 output == act(bias)", host(y32)[..., co - 1],
                    np.broadcast_to(R.leaky(c["bias"][co - 1:], SLOPE, F32), (n, d.ho, d.wo)))


def wgrad_launches(K, G, case, mode="randn", tag="", expect="conv_wgrad_bf16_kernel<", c=None):
    n, h, w, ci, co, k, s, p = case
    c = c or igemm_case(case, mode)
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    xd, dyd = dev(c["x"]), dev(c["dy"])
    dw = nan_out((co, k, k, ci), torch.float32)
    ran(K, G, tag + "wgrad", expect, lambda: K.conv2d_wgrad_bf16(d, xd, dyd, dw))
    G.grade(tag + "wgrad over NaN -> fp32", host(dw), c["wgrad"], False)
    dwa = dev(c["oldw"], torch.float32)
    ran(K, G, tag + "wgrad accumulate", expect, lambda: K.conv2d_wgrad_bf16(d, xd, dyd, dwa, accumulate=True))
    G.grade(tag + "wgrad accumulated onto fp32", host(dwa), R.epilogue(c["wgrad"], old=c["oldw"]), False)


@pytest.mark.parametrize("generic", [0, 1], ids=["uniform", "generic"])
@pytest.mark.parametrize("case", IGEMM, ids=[("n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c) for c in IGEMM])
def test_shared_source_every_tile(K, case, generic):
    """conv2d_fwd_bf16 / conv2d_dgrad_bf16 / conv2d_wgrad_bf16 under IGEMM_TILE = 1 .. 4 (128 x 128, 128 x 64, 64 x 64, 128 x 32) with
    the uniform-tap / row-uniform loops allowed and with GENERIC_GATHER = 1; the strided layers' data gradients run their parity
    classes in one launch."""
    G = R.Grader(f"igemm {case} generic{generic}", _log)
    with options(K, GENERIC_GATHER=generic):
        for tile in (1, 2, 3, 4):
            with options(K, IGEMM_TILE=tile):
                igemm_launches(K, G, case, tile, generic, tag=f"tile{tile} ")
        wgrad_launches(K, G, case)
    G.done()


EPI = [((2, 9, 7, 64, 72, 3, 1, 1), "randn"), ((2, 16, 16, 64, 128, 3, 2, 1), "randn"), ((2, 32, 32, 8, 64, 4, 2, 1), "randn"),
       ((2, 9, 7, 64, 72, 3, 1, 1), "binades"), ((2, 9, 7, 64, 72, 3, 1, 1), "zero")]


@pytest.mark.parametrize("case,mode", EPI, ids=[("n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c) + "-" + m for c, m in EPI])
def test_shared_source_epilogues(K, case, mode):
    """Bias, residual + ReLU to bf16, fp32 output + LeakyReLU, the statistics and both accumulating forms on the launcher's own tile."""
    G = R.Grader(f"igemm epilogues {case} {mode}", _log)
    igemm_launches(K, G, case, 0, 0, mode=mode, epilogues=True)
    wgrad_launches(K, G, case, mode=mode)
    G.done()


FOLD = [((2, 16, 64, 16, 16), 0), ((1, 10, 14, 32, 16), 0), ((2, 16, 64, 16, 16), 1), ((1, 10, 14, 32, 16), 1), ((1, 10, 13, 16, 24), 0)]


@pytest.mark.parametrize("shape,no_fold", FOLD, ids=["n%d_%dx%d_ci%d_co%d" % s + ("-nofold" if f else "") for s, f in FOLD])
def test_shared_source_pixel_fold(K, shape, no_fold):
    """16 / 32 gathered channels: four / two pixels folded into one 64-channel unit on the uniform-tap loop (forward and data gradient
    each by its own gathered count), the same layers with NO_FOLD = 1, and a width the fold does not divide."""
    case = shape + (3, 1, 1)
    G = R.Grader(f"igemm fold {shape} no_fold{no_fold}", _log)
    with options(K, NO_FOLD=1) if no_fold else contextlib.nullcontext():
        igemm_launches(K, G, case, 0, 0, no_fold=bool(no_fold), epilogues=True)
    G.done()


# ============================================================================================= halo-resident weight gradients
WG = [(2, 16, 32, 64, 64), (1, 9, 33, 64, 128), (3, 8, 32, 192, 64)]


@pytest.mark.parametrize("blocks", [-1, 3], ids=["default-blocks", "three-blocks"])
@pytest.mark.parametrize("shape", WG, ids=["n%d_%dx%d_ci%d_co%d" % s for s in WG])
def test_wgrad_halo(K, shape, blocks):
    """conv2d_wgrad_halo (dW += ...: the entry point always accumulates) onto zeros and onto a random dW; WGRAD_HALO_BLOCKS at its
    default and at 3, where three blocks each walk several pixel tiles."""
    n, h, w, ci, co = shape
    case = shape + (3, 1, 1)
    c = igemm_case(case)
    G = R.Grader(f"wgrad halo {shape} blocks{blocks}", _log)
    d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
    assert K.conv2d_wgrad_halo_ok(d)
    xd, dyd = dev(c["x"]), dev(c["dy"])
    dw0, dwa = torch.zeros((co, 3, 3, ci), device="cuda"), dev(c["oldw"], torch.float32)
    with options(K, WGRAD_HALO_BLOCKS=blocks):
        ran(K, G, "wgrad halo", "conv_wgrad_h2_kernel<", lambda: K.conv2d_wgrad_halo(d, xd, None, dyd, dw0))
        ran(K, G, "wgrad halo accumulate", "conv_wgrad_h2_kernel<", lambda: K.conv2d_wgrad_halo(d, xd, None, dyd, dwa))
    G.grade("wgrad halo onto zeros -> fp32", host(dw0), c["wgrad"], False)
    G.grade("wgrad halo accumulated onto fp32", host(dwa), R.epilogue(c["wgrad"], old=c["oldw"]), False)
    if blocks == -1:
        wgrad_launches(K, G, case, tag="split-K ")
    G.done()


@pytest.mark.parametrize("blocks", [-1, 3], ids=["default-blocks", "three-blocks"])
@pytest.mark.parametrize("mode", ["randn", "binades"])
def test_wgrad_halo_fused_decoder_input(K, blocks, mode):
    """up=True at (2, 8, 16, 64 + 64 -> 64): the weight gradient over cat([nearest_x2(a), skip]) gathered while staging."""
    n, h, w, ca, cb, co = 2, 8, 16, 64, 64, 64
    rng = np.random.default_rng(seed_of("wgrad up", mode))
    b = mode == "binades"
    G = R.Grader(f"wgrad halo fused input blocks{blocks} {mode}", _log)
    a, skip = R.randn_bf16(rng, (n, h, w, ca), binades=b), R.randn_bf16(rng, (n, 2 * h, 2 * w, cb), binades=b)
    dy = R.randn_bf16(rng, (n, 2 * h, 2 * w, co), binades=b)
    oldw = rng.standard_normal((co, 3, 3, ca + cb)).astype(F32)
    d = K.conv_desc(n, 2 * h, 2 * w, ca + cb, co, 3, 1, 1)
    assert K.conv2d_wgrad_halo_ok(d, ca)
    ref = R.wgrad(R.upcat(a, skip), dy, 3, 1, 1)
    dw0, dwa = torch.zeros((co, 3, 3, ca + cb), device="cuda"), dev(oldw, torch.float32)
    ad, sd, dyd = dev(a), dev(skip), dev(dy)
    with options(K, WGRAD_HALO_BLOCKS=blocks):
        ran(K, G, "fused wgrad halo", "conv_wgrad_h2_kernel<", lambda: K.conv2d_wgrad_halo(d, ad, sd, dyd, dw0, up=True))
        ran(K, G, "fused wgrad halo accumulate", "conv_wgrad_h2_kernel<", lambda: K.conv2d_wgrad_halo(d, ad, sd, dyd, dwa, up=True))
    G.grade("fused wgrad halo onto zeros -> fp32", host(dw0), ref, False)
    G.grade("fused wgrad halo accumulated onto fp32", host(dwa), R.epilogue(ref, old=oldw), False)
    G.done()


def test_wgrad_1x1_row_form_and_operand_edges(K):
    """conv2d_wgrad_bf16 on a 1x1 / stride 1 layer (the batch as one row of 63 pixels), and the 3x3 weight gradients over 20 binades
    and with an all-zero gathered block and an all-zero dy channel (zero magnitude: exactly the old contents)."""
    G = R.Grader("wgrad edges", _log)
    wgrad_launches(K, G, (1, 7, 9, 64, 128, 1, 1, 0), tag="1x1 row form ")
    wgrad_launches(K, G, (2, 16, 32, 64, 64, 3, 1, 1), mode="binades", tag="binades ")
    wgrad_launches(K, G, (2, 16, 32, 64, 64, 3, 1, 1), mode="zero", tag="zero ")
    for mode in ("binades", "zero"):
        n, h, w, ci, co = 2, 16, 32, 64, 64
        c = igemm_case((n, h, w, ci, co, 3, 1, 1), mode)
        d = K.conv_desc(n, h, w, ci, co, 3, 1, 1)
        dwa = dev(c["oldw"], torch.float32)
        ran(K, G, f"{mode} wgrad halo", "conv_wgrad_h2_kernel<", lambda: K.conv2d_wgrad_halo(d, dev(c["x"]), None, dev(c["dy"]), dwa))
        G.grade(f"{mode} wgrad halo accumulated onto fp32", host(dwa), R.epilogue(c["wgrad"], old=c["oldw"]), False)
    G.done()


# ================================================================================= conv_wgrad_bf16_kernel: tiles, gathers, block order
# (n, h, w, ci, co, k, stride, pad), WGRAD_GENERIC, WGRAD_NO_XCD.  The 128 x 64 tile (co >= 128: a 32-row load pass) at an output width
# of 32 and the 32 x 128 tile (co <= 32: a 16-row pass) at 16, M = 480 in three images: two splits, the first ends inside image 1.
# The XCD-aware block order needs a multiple of 8 >= 16 splits of >= 256 pixels: M = 4096 (16 splits) and M = 5376 (21 splits
# rounded to 24, three of them empty), the latter also on the two-dimensional grid.
WG_SPLITK = [((3, 5, 32, 64, 128, 3, 1, 1), 0, 0), ((3, 5, 32, 64, 128, 3, 1, 1), 1, 0),
             ((3, 10, 16, 64, 24, 3, 1, 1), 0, 0), ((3, 10, 16, 64, 24, 3, 1, 1), 1, 0),
             ((1, 64, 64, 64, 128, 3, 1, 1), 0, 0), ((1, 84, 64, 64, 128, 3, 1, 1), 0, 0), ((1, 84, 64, 64, 128, 3, 1, 1), 0, 1)]
WG_PART = (2, 16, 32, 32, 40, 72)          # conv2d_wgrad_part: (n, h, w, ca, cs, co)


@functools.lru_cache(maxsize=None)
def wgrad_case(case):
    """Operands and the reference of a weight gradient alone (igemm_case forms the forward and the data gradient as well)."""
    n, h, w, ci, co, k, s, p = case
    rng = np.random.default_rng(seed_of("wgrad", case))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x, dy = R.randn_bf16(rng, (n, h, w, ci)), R.randn_bf16(rng, (n, ho, wo, co))
    return dict(x=x, dy=dy, oldw=rng.standard_normal((co, k, k, ci)).astype(F32), wgrad=R.wgrad(x, dy, k, s, p))


@pytest.mark.parametrize("case,generic,no_xcd", WG_SPLITK,
                         ids=[("n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c) + ("-generic" if g else "-uniform") + ("-noxcd" if x else "") for c, g, x in WG_SPLITK])
def test_wgrad_split_k_tiles_and_block_order(K, case, generic, no_xcd):
    """conv2d_wgrad_bf16 on conv_wgrad_bf16_kernel<128, 64, 2, 2, *> and <32, 128, 1, 4, *> under both gathers, and the XCD-aware
    one-dimensional block order with and without empty splits; the symbol by name from the launcher's arithmetic restated in
    _conv_ref.wgrad_bf16_plan (asserted on the CPU in tests/test_conv_ref_host.py)."""
    G = R.Grader(f"wgrad split-K {case} generic{generic} no_xcd{no_xcd}", _log)
    sym = R.wgrad_bf16_plan(*case, generic=bool(generic), no_xcd=bool(no_xcd))[0]
    with options(K, WGRAD_GENERIC=generic, WGRAD_NO_XCD=no_xcd):
        wgrad_launches(K, G, case, expect=sym, c=wgrad_case(case))
    G.done()


@pytest.mark.parametrize("generic", [0, 1], ids=["uniform", "generic"])
def test_wgrad_channel_slices(K, generic):
    """conv2d_wgrad_part on bf16 tensors: the up-sampled half (c_off = 0, read through nearest_x2) and the skip half (c_off = ca) of
    the weight gradient over cat([nearest_x2(a), skip]), two launches accumulating into one fp32 dW."""
    n, h, w, ca, cs, co = WG_PART
    rng = np.random.default_rng(seed_of("wgrad part", WG_PART))
    G = R.Grader(f"wgrad part {WG_PART} generic{generic}", _log)
    a, skip, dy = R.randn_bf16(rng, (n, h // 2, w // 2, ca)), R.randn_bf16(rng, (n, h, w, cs)), R.randn_bf16(rng, (n, h, w, co))
    oldw = rng.standard_normal((co, 3, 3, ca + cs)).astype(F32)
    geom = (n, h, w, ca + cs, co, 3, 1, 1)
    sym_a = R.wgrad_bf16_plan(*geom, generic=bool(generic), src_c=ca, up=True)[0]
    sym_s = R.wgrad_bf16_plan(*geom, generic=bool(generic), src_c=cs)[0]
    d = K.conv_desc(*geom)
    dw = dev(oldw, torch.float32)
    with options(K, WGRAD_GENERIC=generic):
        ran(K, G, "part up", sym_a, lambda: K.conv2d_wgrad_part(d, dev(a), 0, True, dev(dy), dw, True))
        half = host(dw).copy()
        G.exact("skip channels after the up-sampled half's launch", half[..., ca:], oldw[..., ca:])
        ran(K, G, "part skip", sym_s, lambda: K.conv2d_wgrad_part(d, dev(skip), ca, False, dev(dy), dw, True))
    G.exact("up-sampled channels after the skip half's launch", host(dw)[..., :ca], half[..., :ca])
    G.grade("wgrad of both halves accumulated onto fp32", host(dw), R.epilogue(R.wgrad(R.upcat(a, skip), dy, 3, 1, 1), old=oldw), False)
    G.done()
