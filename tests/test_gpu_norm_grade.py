"""The streaming kernels of every training step -- BatchNorm forward / backward with its fused activation and residual add
(csrc/norm_act.hip, both storages from one body per kernel), act_bwd, channel_sum, the accumulate flags of the pooling / up-sampling
backward (csrc/pool_resize.hip) and Adam (csrc/optim.hip) -- against the float64 restatement of tests/_norm_ref.py
(proven against torch's double-precision autograd by tests/test_norm_ref_host.py).

One bar for everything, the bar of tests/test_gpu_train_aug.py, test_gpu_clahe.py and test_gpu_ingest.py taken over the whole
tensor and normalised: with e = |kernel - f64| / magnitude and d = |fp32 leg - f64| / magnitude element-wise (magnitude: the sum
of the absolute values of the terms that formed the element, from _norm_ref), max(e) <= max(4 x max(d), 2^-22).  Normalising per
element lets one wrong small channel show; the maximum of d over the whole output keeps the bar from being a noisy per-channel
estimate.  save_mean / save_rstd / running_mean / running_var are float64 values rounded one to three times: 2 ulp of fp32 at the
larger operand's magnitude, directly against float64.  bf16 storage: the reference inputs are the bf16-rounded values and a bf16
output gets half a bf16 ulp at the float64 value (the larger neighbouring spacing at a binade edge) on top of the fp32 bar.

No element is masked out.  A pre-activation within rounding distance of zero could take the other side of the activation in
fp32 and float64, so every case asserts on the CPU, before any launch, that the float64 pre-activation of every element lies
outside +-8 x 2^-24 x magnitude; the seeds are chosen so that it holds.

Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import warnings

import numpy as np
import pytest
import torch

import _norm_ref as N
from _grade import Grader, log as _log    # shared with tests/test_gpu_pool_grade.py

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))             # the values the kernels receive (their arguments are C floats)
MOM = float(np.float32(0.1))
BAND = 8 * 2.0 ** -24
F32, BF16 = "f32", "bf16"
MODES = [(N.NONE, 0.0, False), (N.LEAKY, 0.0, True), (N.LEAKY, 0.2, False)]
MODE_IDS = ["none", "relu+res", "leaky0.2"]


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    return kernels


# ------------------------------------------------------------------------------------------------------------- launch shapes
def stream_blocks(nvec, cvec, max_blocks=2048, per_thread=4):
    """(block size, blocks) of csrc/common.h stream_shape for nvec 16-byte vectors of a tensor with cvec vectors per pixel."""
    if cvec <= 256:
        bs, unit = (256 // cvec) * cvec, 1
    else:
        bs, unit = 256, (cvec + 255) // 256
        while (unit * 256) % cvec:
            unit += 1
    want = min(max(-(-nvec // (bs * per_thread)), 1), max_blocks)
    grid = -(-want // unit) * unit
    while grid * bs < cvec:
        grid += unit
    return bs, grid


def test_the_shapes_reach_every_launch_regime():
    """The cases below name the smallest size at which each path of stream_shape exists; this pins that they do."""
    assert stream_blocks(260 * 16, 16) == (256, 5)                       # vector count divides 256
    assert stream_blocks(7 * 6, 6)[0] == 252 and stream_blocks(63 * 10, 10)[0] == 250
    assert stream_blocks(7 * 3, 3)[0] == 255 and stream_blocks(63 * 5, 5)[0] == 255          # bf16: c / 8 = 3, 5
    assert stream_blocks(30 * 512, 512) == (256, 16)                     # > 256, power of two: unit 2
    assert stream_blocks(6 * 257, 257) == (256, 257)                     # unit 257 (fp32 c = 1028, bf16 c = 2056)
    assert stream_blocks(6 * 384, 384) == (256, 3)                       # unit 3 (fp32 c = 1536); bf16 c = 3072:
    assert stream_blocks(30 * 384, 384) == (256, 12)
    # REDUCE_BLOCKS = 3: 768 threads over 33280 (fp32) / 16640 (bf16) vectors: 43 / 21 steps each, the 4 x unrolled loop and its tail
    assert stream_blocks(8320 * 4, 4, 3) == (256, 3) and stream_blocks(8320 * 2, 2, 3) == (256, 3)
    # BN_APPLY_PT = 16: 9 / 5 blocks, 14.4 / 13 steps per thread
    assert stream_blocks(8320 * 4, 4, 2048, 16) == (256, 9) and stream_blocks(8320 * 2, 2, 2048, 16) == (256, 5)
    # default cap at (8320, 16): more blocks than the 16 replicas
    assert stream_blocks(8320 * 4, 4, 512)[1] == 33 and stream_blocks(8320 * 2, 2, 512)[1] == 17


# ---------------------------------------------------------------------------------------------------------------------- data
def make_case(p, c, with_res, seed, kind="plain", store=F32):
    """Operands of one layer as fp32 numpy arrays holding the STORED values (bf16-rounded for bf16 storage)."""
    g = np.random.default_rng(1_000_003 * seed + 1009 * p + c)
    y = g.standard_normal((p, c)) * 2 + 0.5
    if kind == "constant":
        y[:, 3] = 0.75
    elif kind == "small":
        y[:, 5] = 0.5 + 0.01 * g.standard_normal(p)
    elif kind == "mean64":
        y = 64 + g.standard_normal((p, c))
    elif kind == "mean1000":
        y = 1000 + g.standard_normal((p, c))
    d = {"y": y, "res": g.standard_normal((p, c)) if with_res else None, "dz": g.standard_normal((p, c)),
         "gamma": g.random(c) + 0.5, "beta": g.standard_normal(c), "rm0": g.standard_normal(c), "rv0": g.random(c) + 0.5}
    d = {k: None if v is None else v.astype(np.float32) for k, v in d.items()}
    if store == BF16:
        for k in ("y", "res", "dz"):
            d[k] = None if d[k] is None else N.bf16_round(d[k])
    return d


def assert_clear_of_zero(t64, mag, what):
    inside = int((np.abs(t64) <= BAND * mag).sum())
    assert inside == 0, f"{what}: {inside} pre-activations within 8 x 2^-24 of zero; choose another seed"


def dev(a, store=F32):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if a.ndim == 2:
        t = t.view(1, 1, *a.shape)
        if store == BF16:
            t = t.bfloat16()                                  # exact: the values are already bf16
    return t.cuda()


def host(t):
    return t.detach().float().cpu().numpy().reshape(-1, t.shape[-1]) if t.dim() == 4 else t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------- one BatchNorm layer, graded
def run_layer(K, p, c, act, slope, with_res, store, seed=0, kind="plain", recompute=False, tag=None):
    d = make_case(p, c, with_res, seed, kind, store)
    tag = tag or f"bn {store} ({p},{c}) act={act} slope={slope} res={int(with_res)} {kind}"
    bf = store == BF16
    y, res, dz, gamma, beta = d["y"], d["res"], d["dz"], d["gamma"], d["beta"]
    z64, t64, mag_z = N.bn_forward(y, gamma, beta, res, EPS, act, slope, np.float64)
    z32, _, _ = N.bn_forward(y, gamma, beta, res, EPS, act, slope, np.float32)
    if act != N.NONE:
        assert_clear_of_zero(t64, mag_z, tag)
    mean, var, rstd = N.stats(y, EPS)
    rm64, rv64, op_rm, op_rv = N.running(mean, var, p, MOM, d["rm0"], d["rv0"])
    b64 = N.bn_backward(dz, z64, y, gamma, EPS, act, slope, np.float64)
    b32 = N.bn_backward(dz, z32, y, gamma, EPS, act, slope, np.float32)

    G = Grader(tag)
    R = K.bn_replicas()
    yd, dzd, resd = dev(y, store), dev(dz, store), (dev(res, store) if with_res else None)
    gam, bet, rm, rv = dev(gamma), dev(beta), dev(d["rm0"]), dev(d["rv0"])
    sm, sr = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    sums = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    K.bn_stats(yd, sums)
    z = torch.full_like(yd, float("nan"))
    K.bn_apply(yd, sums, gam, bet, resd, z, EPS, MOM, rm, rv, sm, sr, act, slope)
    G.grade("z", host(z), z64, z32, mag_z, bf)
    G.ulp2("save_mean", host(sm), mean, np.abs(mean))
    G.ulp2("save_rstd", host(sr), rstd, np.abs(rstd))
    G.ulp2("running_mean", host(rm), rm64, op_rm)
    G.ulp2("running_var", host(rv), rv64, op_rv)

    bs = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    dy = torch.full_like(yd, float("nan"))
    dres = torch.full_like(yd, float("nan")) if with_res else None
    dg, db = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    if recompute and not bf:             # fp32: z = None, the activation's argument is re-evaluated from y, gamma, beta
        K.bn_bwd_reduce(dzd, None, yd, sm, sr, bs, act, slope, gamma=gam, beta=bet)
        K.bn_bwd_apply(dzd, None, yd, sm, sr, gam, bs, dy, None, dg, db, act, slope, beta=bet)
    elif recompute:                      # bf16: scale / shift from bn_finalize take z's place in the apply pass
        sc, sh = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
        rm2, rv2, sm2, sr2 = dev(d["rm0"]), dev(d["rv0"]), torch.empty_like(sm), torch.empty_like(sr)
        K.bn_finalize(sums, gam, bet, p, EPS, MOM, rm2, rv2, sm2, sr2, sc, sh)
        f64, f32 = (N.bn_finalize(y, gamma, beta, EPS, e) for e in (np.float64, np.float32))
        G.grade("finalize scale", host(sc), f64[0], f32[0], f64[2])
        G.grade("finalize shift", host(sh), f64[1], f32[1], f64[3])
        for a, b_ in ((rm2, rm), (rv2, rv), (sm2, sm), (sr2, sr)):
            assert torch.equal(a, b_), f"{tag}: bn_finalize and bn_apply disagree on the statistics"
        K.bn_bwd_reduce(dzd, z, yd, sm, sr, bs, act, slope)
        K.bn_bwd_apply_recompute(dzd, yd, sc, sh, sm, sr, gam, bs, dy, dg, db, act, slope)
    else:
        K.bn_bwd_reduce(dzd, z, yd, sm, sr, bs, act, slope)
        K.bn_bwd_apply(dzd, z, yd, sm, sr, gam, bs, dy, dres, dg, db, act, slope)
    G.grade("dy", host(dy), b64["dy"][0], b32["dy"][0], b64["dy"][1], bf)
    G.grade("dgamma", host(dg), b64["dgamma"][0], b32["dgamma"][0], b64["dgamma"][1])
    G.grade("dbeta", host(db), b64["dbeta"][0], b32["dbeta"][0], b64["dbeta"][1])
    if dres is not None:
        G.grade("dres", host(dres), b64["dres"][0], b32["dres"][0], b64["dres"][1], bf)
    torch.cuda.synchronize()
    G.done()


SHAPES = {F32: [(1, 16), (2, 16), (260, 64), (7, 24), (63, 40), (30, 2048), (6, 1028), (6, 1536)],
          BF16: [(1, 16), (2, 16), (260, 64), (7, 24), (63, 40), (30, 3072), (6, 2056)]}
LAYERS = [(s, p, c) for s in (F32, BF16) for p, c in SHAPES[s]]


@pytest.mark.parametrize("store,p,c", LAYERS, ids=[f"{s}-{p}x{c}" for s, p, c in LAYERS])
@pytest.mark.parametrize("act,slope,with_res", MODES, ids=MODE_IDS)
def test_layer_against_float64(K, store, p, c, act, slope, with_res):
    run_layer(K, p, c, act, slope, with_res, store)


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("act,slope,with_res", MODES, ids=MODE_IDS)
def test_layer_unrolled_loop_tail_and_few_blocks(K, store, act, slope, with_res):
    """(8320, 16) with three reduce blocks and 16 vectors per thread in the apply kernels: every thread runs the 4 x unrolled
    grid-stride loop several times and then its tail (test_the_shapes_reach_every_launch_regime has the arithmetic)."""
    try:
        K.set_option("REDUCE_BLOCKS", 3)
        K.set_option("BN_APPLY_PT", 16)
        run_layer(K, 8320, 16, act, slope, with_res, store, tag=f"bn {store} (8320,16) 3 blocks act={act} slope={slope} res={int(with_res)}")
    finally:
        K.set_option("REDUCE_BLOCKS", -1)
        K.set_option("BN_APPLY_PT", -1)


@pytest.mark.parametrize("store", [F32, BF16])
def test_layer_leaky_with_residual_and_recompute(K, store):
    run_layer(K, 260, 64, N.LEAKY, 0.2, True, store)
    run_layer(K, 260, 64, N.LEAKY, 0.2, False, store, recompute=True, tag=f"bn {store} (260,64) leaky0.2 recompute")
    run_layer(K, 260, 64, N.LEAKY, 0.0, False, store, recompute=True, tag=f"bn {store} (260,64) relu recompute")


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("kind,p,c,act,seed", [("constant", 260, 64, N.NONE, 0), ("small", 260, 64, N.NONE, 0),
                                               ("mean64", 260, 64, N.LEAKY, 0), ("mean1000", 8320, 16, N.NONE, 0)])
def test_layer_statistics_edges(K, store, kind, p, c, act, seed):
    """A constant channel (var clamps to 0, rstd = 1 / sqrt(eps)), a channel of std 0.01 (eps matters), |mean| / std = 64 under
    ReLU, and |mean| / std = 1000 over 8320 pixels, where an fp32 accumulator would miss save_rstd by orders of magnitude."""
    run_layer(K, p, c, act, 0.0, False, store, seed=seed, kind=kind)


# ------------------------------------------------------------------------------------------------------------- calling modes
def ulp_at(*operands):
    """One fp32 ulp at the largest magnitude among the operands, element-wise (float64 array)."""
    m = np.maximum.reduce([np.abs(np.asarray(o, dtype=np.float64)) for o in operands])
    return np.spacing(m.astype(np.float32)).astype(np.float64)


def check_accumulated(what, acc, old, plain, store, exact):
    """acc: the accumulating call's output on a buffer that held ``old``; plain: the non-accumulating output.

    fp32: old + plain in fp32, bit for bit where the kernel's sum is a plain add; where a multiply may fuse into the add the
    product is rounded in one call and not in the other: half an ulp of the product plus half an ulp of the sum, bounded by one
    ulp at the larger magnitude.  bf16: the kernels add in fp32 and round once; ``plain`` was itself rounded to bf16, so unless
    it is exact (a copy, dz x 1 or x 0) the two differ by half a bf16 ulp of plain plus half a bf16 ulp of the sum."""
    acc, old, plain = (np.asarray(x, dtype=np.float32) for x in (acc, old, plain))
    want = old + plain
    if store == BF16:
        want = N.bf16_round(want)
    if exact:
        assert np.array_equal(acc, want), f"{what}: accumulate is not old + result"
        return
    diff = np.abs(acc.astype(np.float64) - (old.astype(np.float64) + plain.astype(np.float64)))
    if store == BF16:
        tol = N.bf16_half_ulp(plain) + N.bf16_half_ulp(acc, N.bf16_half_ulp(plain)) + ulp_at(old, plain)
    else:
        tol = ulp_at(old, plain, want)
    worst = float((diff / tol).max())
    _log(f"norm-grade accumulate {store} {what}: worst |acc - (old + plain)| / tolerance {worst:.3f}")
    assert worst <= 1.0, f"{what}: {worst:.3f} of the tolerance"


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("p,c", [(260, 64), (7, 24)])
@pytest.mark.parametrize("act,slope", [(N.LEAKY, 0.0), (N.LEAKY, 0.2), (N.NONE, 0.0)], ids=["relu", "leaky0.2", "none"])
def test_bn_bwd_apply_in_place_and_accumulate(K, store, p, c, act, slope):
    """engine.py runs bn_bwd_apply with dy being dz's own buffer, and sets accumulate_dy / accumulate_dres / accumulate_param on
    every residual and decoder block."""
    d = make_case(p, c, True, 1, "plain", store)
    _, t64, mag = N.bn_forward(d["y"], d["gamma"], d["beta"], d["res"], EPS, act, slope)
    if act != N.NONE:
        assert_clear_of_zero(t64, mag, "in place / accumulate")
    R = K.bn_replicas()
    yd, dzd, resd, gam, bet = dev(d["y"], store), dev(d["dz"], store), dev(d["res"], store), dev(d["gamma"]), dev(d["beta"])
    sm, sr = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    sums = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    K.bn_stats(yd, sums)
    z = torch.empty_like(yd)
    K.bn_apply(yd, sums, gam, bet, resd, z, EPS, MOM, None, None, sm, sr, act, slope)
    bs = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    K.bn_bwd_reduce(dzd, z, yd, sm, sr, bs, act, slope)

    def apply(dz_, dy_, dres_, dg_, db_, **kw):
        K.bn_bwd_apply(dz_, z, yd, sm, sr, gam, bs, dy_, dres_, dg_, db_, act, slope, **kw)

    dy0, dres0 = torch.full_like(yd, float("nan")), torch.full_like(yd, float("nan"))
    dg0, db0 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    apply(dzd, dy0, dres0, dg0, db0)
    # in place: dy is dz
    buf, dres1, dg1, db1 = dzd.clone(), torch.empty_like(yd), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    apply(buf, buf, dres1, dg1, db1)
    assert torch.equal(buf, dy0), "dy written over dz differs from the out-of-place result"
    assert torch.equal(dres1, dres0) and torch.equal(dg1, dg0) and torch.equal(db1, db0)
    # accumulate: every flag, on buffers that hold something
    g = torch.Generator().manual_seed(7)
    old = {k: torch.randn(s, generator=g) for k, s in (("dy", (p, c)), ("dres", (p, c)), ("dg", (c,)), ("db", (c,)))}
    if store == BF16:
        old["dy"], old["dres"] = old["dy"].bfloat16().float(), old["dres"].bfloat16().float()
    dy2, dres2 = dev(old["dy"].numpy(), store), dev(old["dres"].numpy(), store)
    dg2, db2 = old["dg"].cuda(), old["db"].cuda()
    apply(dzd, dy2, dres2, dg2, db2, accumulate_dy=True, accumulate_dres=True, accumulate_param=True)
    tag = f"({p},{c}) act={act} slope={slope}"
    check_accumulated(f"dgamma {tag}", host(dg2), old["dg"].numpy(), host(dg0), F32, True)
    check_accumulated(f"dbeta {tag}", host(db2), old["db"].numpy(), host(db0), F32, True)
    check_accumulated(f"dres {tag}", host(dres2), old["dres"].numpy(), host(dres0), store, slope == 0.0)
    check_accumulated(f"dy {tag}", host(dy2), old["dy"].numpy(), host(dy0), store, False)
    # one flag at a time leaves the other outputs as they were
    dy3, dres3, dg3, db3 = torch.empty_like(yd), dev(old["dres"].numpy(), store), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    apply(dzd, dy3, dres3, dg3, db3, accumulate_dres=True)
    assert torch.equal(dy3, dy0) and torch.equal(dg3, dg0) and torch.equal(db3, db0) and torch.equal(dres3, dres2)


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("p,c", [(260, 64), (7, 24)])
def test_act_bwd_in_place_and_signed_zeros(K, store, p, c):
    """discriminator.py runs act_bwd(dz, z, dz); an output of exactly 0.0 or -0.0 takes the slope."""
    g = np.random.default_rng(3 + p)
    z, dz = g.standard_normal((p, c)).astype(np.float32), g.standard_normal((p, c)).astype(np.float32)
    z[0, :4], z[-1, -4:] = (0.0, -0.0, 0.0, -0.0), (-0.0, 0.0, -0.0, 0.0)
    dz[0, :4] = (1.0, 1.0, -3.0, -3.0)
    if store == BF16:
        z, dz = N.bf16_round(z), N.bf16_round(dz)
    G = Grader(f"act_bwd {store} ({p},{c})")
    for slope in (0.2, 0.0):
        r64, mag = N.act_bwd(dz, z, N.LEAKY, slope, np.float64)
        r32, _ = N.act_bwd(dz, z, N.LEAKY, slope, np.float32)
        zd, dzd = dev(z, store), dev(dz, store)
        dy = torch.full_like(zd, float("nan"))
        K.act_bwd(dzd, zd, dy, N.LEAKY, slope)
        G.grade(f"dy slope {slope}", host(dy), r64, r32, mag, store == BF16)
        want = np.float32(slope) * np.array([1.0, 1.0, -3.0, -3.0], dtype=np.float32)
        assert np.array_equal(host(dy)[0, :4], N.bf16_round(want) if store == BF16 else want), "signed zeros must take the slope"
        K.act_bwd(dzd, zd, dzd, N.LEAKY, slope)
        assert torch.equal(dzd, dy), "act_bwd written over dz differs from the out-of-place result"
    G.done()


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("shape", [(2, 16, 2, 2), (1, 8, 7, 9), (1, 8, 1, 5), (1, 8, 5, 1)])
def test_maxpool_bwd_accumulate(K, store, shape):
    n, c, h, w = shape
    dt = torch.bfloat16 if store == BF16 else torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.relu(torch.randn(n, h, w, c, generator=g)).to(dt).cuda()            # many exact ties at 0, like post-ReLU
    y, idx = K.maxpool_fwd(x)
    dy = torch.randn(y.shape, generator=g).to(dt).cuda()
    old = torch.randn(x.shape, generator=g).to(dt)
    plain = torch.full_like(x, float("nan"))
    K.maxpool_bwd(dy, idx, plain)
    acc = old.cuda()
    K.maxpool_bwd(dy, idx, acc, accumulate=True)
    # fp32: (sum of the windows' gradients) + old, the same adds in the same order: bit for bit
    check_accumulated(f"maxpool {shape}", acc.float().cpu().numpy(), old.float().numpy(), plain.float().cpu().numpy(), store, store == F32)


@pytest.mark.parametrize("store", [F32, BF16])
@pytest.mark.parametrize("ca,cb", [(32, 0), (64, 64)])
def test_upsample_concat_bwd_accumulate(K, store, ca, cb):
    n, h, w = 2, 5, 6
    dt = torch.bfloat16 if store == BF16 else torch.float32
    g = torch.Generator().manual_seed(2)
    dout = torch.randn(n, 2 * h, 2 * w, ca + cb, generator=g).to(dt).cuda()
    old_a, old_s = torch.randn(n, h, w, ca, generator=g).to(dt), (torch.randn(n, 2 * h, 2 * w, cb, generator=g).to(dt) if cb else None)
    da0 = torch.full((n, h, w, ca), float("nan"), dtype=dt, device="cuda")
    ds0 = torch.full((n, 2 * h, 2 * w, cb), float("nan"), dtype=dt, device="cuda") if cb else None
    K.upsample2x_concat_bwd(dout, da0, ds0, ca, cb)
    if cb:
        assert torch.equal(ds0, dout[..., ca:])
    da1, ds1 = old_a.cuda(), (old_s.cuda() if cb else None)
    K.upsample2x_concat_bwd(dout, da1, ds1, ca, cb, accumulate_da=True, accumulate_dskip=True)
    np_ = lambda t: t.float().cpu().numpy()
    check_accumulated(f"upcat da {ca}/{cb}", np_(da1), np_(old_a), np_(da0), store, store == F32)
    if cb:
        check_accumulated(f"upcat dskip {ca}/{cb}", np_(ds1), np_(old_s), np_(ds0), store, True)
        # one flag only: the other output is overwritten
        da2, ds2 = old_a.cuda(), old_s.cuda()
        K.upsample2x_concat_bwd(dout, da2, ds2, ca, cb, accumulate_da=False, accumulate_dskip=True)
        assert torch.equal(da2, da0) and torch.equal(ds2, ds1)


CHSUM_DIRECT_BLOCKS = 32                   # csrc/common.h: up to this many blocks add straight into the output


@pytest.mark.parametrize("store,p,c,direct", [(F32, 7, 24, True), (BF16, 7, 24, True), (F32, 8320, 16, False), (BF16, 16640, 16, False)])
def test_channel_sum_both_paths(K, store, p, c, direct):
    """channel_sum launches stream_shape(vectors, vectors per pixel, 512 blocks at most, 4 vectors per thread):
    (7, 24): 42 fp32 vectors / 21 bf16 vectors -> 1 block: the direct path (atomics into the output itself);
    (8320, 16) fp32: 33280 vectors / (256 x 4) -> 33 blocks > 32: 16 replicas and the fold kernel;
    bf16 holds 8 channels per vector, (8320, 16) would be 17 blocks and direct, so it takes (16640, 16): 33280 vectors, 33 blocks."""
    vec = 8 if store == BF16 else 4
    blocks = stream_blocks(p * (c // vec), c // vec, 512)[1]
    assert (blocks <= CHSUM_DIRECT_BLOCKS) == direct, blocks
    g = np.random.default_rng(11)
    x = (g.standard_normal((p, c)) + 0.25).astype(np.float32)          # non-zero mean: a lost replica would show
    x = N.bf16_round(x) if store == BF16 else x
    old = g.standard_normal(c).astype(np.float32)
    r64, mag = N.channel_sum(x, np.float64)
    r32, _ = N.channel_sum(x, np.float32)
    G = Grader(f"channel_sum {store} ({p},{c}) {'direct' if direct else 'replicas'}")
    xd, out = dev(x, store), dev(old)
    K.channel_sum(xd, out, accumulate=False)
    G.grade("overwrite", host(out), r64, r32, mag)
    out = dev(old)
    K.channel_sum(xd, out, accumulate=True)
    G.grade("accumulate", host(out), r64 + old, (r32 + old).astype(np.float32), mag + np.abs(old))
    G.done()


@pytest.mark.parametrize("p,c", [(260, 64), (7, 24)])
@pytest.mark.parametrize("act,slope,with_res", MODES, ids=MODE_IDS)
def test_bn_apply_eval(K, p, c, act, slope, with_res):
    d = make_case(p, c, with_res, 2)
    rv = d["rv0"].copy()
    rv[0], rv[1], rv[2] = 0.0, 1e-6, 0.0
    args = (d["y"], d["gamma"], d["beta"], d["rm0"], rv, d["res"], EPS, act, slope)
    z64, t64, mag = N.bn_eval(*args, np.float64)
    z32, _, _ = N.bn_eval(*args, np.float32)
    if act != N.NONE:
        assert_clear_of_zero(t64, mag, "eval")
    yd = dev(d["y"])
    z = torch.full_like(yd, float("nan"))
    K.bn_apply_eval(yd, dev(d["gamma"]), dev(d["beta"]), dev(d["rm0"]), dev(rv), dev(d["res"]) if with_res else None, z, EPS, act, slope)
    G = Grader(f"bn_apply_eval ({p},{c}) act={act} slope={slope} res={int(with_res)}")
    G.grade("z", host(z), z64, z32, mag)
    G.done()


# ------------------------------------------------------------------------------------------------------------- channel limit
def test_channel_limit(K):
    """fp32 bn_bwd_apply keeps 24 bytes of LDS per channel: 96 KB at the 4096 channels the argument check admits.  The device
    has 160 KB per workgroup, the launch goes through, and the result meets the bar.  The bf16 twin keeps its coefficients
    within 64 KB and refuses 4096 channels in its argument check."""
    run_layer(K, 2, 4096, N.LEAKY, 0.0, True, F32, tag="bn f32 (2,4096) channel limit")
    c = 4096
    t = torch.zeros(1, 1, 2, c, dtype=torch.bfloat16, device="cuda")
    v = torch.ones(c, device="cuda")
    bs = torch.zeros(2 * c * K.bn_replicas(), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="too many channels"):
        K.bn_bwd_apply(t, t, t, v, v, v, bs, torch.empty_like(t), None, torch.empty_like(v), torch.empty_like(v), N.LEAKY, 0.0)
    with pytest.raises(RuntimeError, match="too many channels"):
        K.bn_bwd_apply_recompute(t, t, v, v, v, v, v, bs, torch.empty_like(t), torch.empty_like(v), torch.empty_like(v), N.LEAKY, 0.0)


# ---------------------------------------------------------------------------------------------------------------------- Adam
ADAM_SETTINGS = [(1e-3, (0.9, 0.999), 1e-8), (3e-2, (0.5, 0.9), 1e-3)]


def adam_grad(rng, count, t):
    """randn x 10^(t - 3); a fixed tenth of the entries exactly 0 on every step, another tenth scaled by 1e-10 (below eps)."""
    g = rng.standard_normal(count) * 10.0 ** (t - 3)
    i = np.arange(count)
    g[i % 10 == 0] = 0.0
    g[i % 10 == 1] *= 1e-10
    return g.astype(np.float32)


def torch_adam_legs(p0, lr, betas, eps, state=None):
    legs = []
    for dt in (torch.float32, torch.float64):
        p = torch.from_numpy(p0.copy()).to(dt).requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
        if state is not None:
            opt.state[p] = {"step": torch.tensor(float(state[0])), "exp_avg": torch.from_numpy(state[1].copy()).to(dt),
                            "exp_avg_sq": torch.from_numpy(state[2].copy()).to(dt)}
        legs.append((p, opt))
    return legs


def grade_adam(G, what, dev_pmv, legs, mags):
    (p32, o32), (p64, o64) = legs
    for name, got, leg, ref, mag in zip("pmv", dev_pmv, (p32, o32.state[p32]["exp_avg"], o32.state[p32]["exp_avg_sq"]),
                                        (p64, o64.state[p64]["exp_avg"], o64.state[p64]["exp_avg_sq"]), mags):
        G.grade(f"{what} {name}", got.cpu().numpy(), ref.detach().numpy(), leg.detach().numpy(), mag)


@pytest.mark.parametrize("count", [1, 3, 4, 5, 1027, 2_098_355])
@pytest.mark.parametrize("lr,betas,eps", ADAM_SETTINGS, ids=["default", "lr3e-2-b0.5-0.9-eps1e-3"])
def test_adam_flat_against_float64(K, count, lr, betas, eps):
    """Counts below one vector (the tail-only launch), 1027, and 2 098 355 = 4 x 524 588 + 3: more vectors than one grid-stride
    pass of 2048 x 256 threads, plus a tail.  Six steps from zero moments, then one call seeded with moments and step = 1000."""
    rng = np.random.default_rng(count)
    p0 = rng.standard_normal(count).astype(np.float32)
    legs = torch_adam_legs(p0, lr, betas, eps)
    pd, m, v = torch.from_numpy(p0.copy()).cuda(), torch.zeros(count, device="cuda"), torch.zeros(count, device="cuda")
    G = Grader(f"adam count={count} lr={lr} betas={betas} eps={eps}")
    for t in range(1, 7):
        g = adam_grad(rng, count, t)
        before = [legs[1][0].detach().numpy().copy()] + [legs[1][1].state[legs[1][0]][k].numpy().copy() if t > 1 else np.zeros(count)
                                                         for k in ("exp_avg", "exp_avg_sq")]
        for p, opt in legs:
            p.grad = torch.from_numpy(g.copy()).to(p.dtype)
            opt.step()
        K.adam_flat(pd, torch.from_numpy(g).cuda(), m, v, count, lr, betas[0], betas[1], eps, 1 - betas[0] ** t, 1 - betas[1] ** t)
    _, mags = N.adam_step(*before[:1], g, *before[1:], lr, betas[0], betas[1], eps, 6)
    grade_adam(G, "6 steps", (pd, m, v), legs, mags)
    zero = np.arange(count) % 10 == 0
    assert np.array_equal(pd.cpu().numpy()[zero], p0[zero]) and not m.cpu().numpy()[zero].any() and not v.cpu().numpy()[zero].any(), \
        "entries whose gradient is 0 on every step moved"
    # late in training: bias corrections close to 1, where a correction taken at the wrong step hides in the first few steps
    m0 = (rng.standard_normal(count) * 0.1).astype(np.float32)
    v0 = (rng.random(count) * 0.01 + 1e-4).astype(np.float32)
    g = adam_grad(rng, count, 3)
    legs = torch_adam_legs(p0, lr, betas, eps, state=(1000, m0, v0))
    for p, opt in legs:
        p.grad = torch.from_numpy(g.copy()).to(p.dtype)
        opt.step()
    pd, m, v = torch.from_numpy(p0.copy()).cuda(), torch.from_numpy(m0.copy()).cuda(), torch.from_numpy(v0.copy()).cuda()
    K.adam_flat(pd, torch.from_numpy(g).cuda(), m, v, count, lr, betas[0], betas[1], eps, 1 - betas[0] ** 1001, 1 - betas[1] ** 1001)
    _, mags = N.adam_step(p0, g, m0, v0, lr, betas[0], betas[1], eps, 1001)
    grade_adam(G, "step 1001", (pd, m, v), legs, mags)
    G.done()


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_fused_adam_per_tensor_paths(K, strided):
    """FusedAdam.step() on a parameter that is no network's arena: a dense 16-byte-aligned tensor goes through the kernel per
    tensor, a strided view through the torch expressions; neither counts as a flat launch."""
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    lr, betas, eps = ADAM_SETTINGS[1]
    rng = np.random.default_rng(17)
    p0 = rng.standard_normal((36, 28)).astype(np.float32)
    base = torch.from_numpy(p0.copy()).cuda()
    if strided:
        base = torch.from_numpy(np.ascontiguousarray(p0.T)).cuda().t()
        assert not base.is_contiguous()
    else:
        assert base.data_ptr() % 16 == 0 and base.is_contiguous()
    param = torch.nn.Parameter(base)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt = FusedAdam([param], lr=lr, betas=betas, eps=eps)
        legs = torch_adam_legs(p0, lr, betas, eps)
        for t in range(1, 4):
            g = adam_grad(rng, p0.size, t).reshape(p0.shape)
            if t == 3:
                st = legs[1][1].state[legs[1][0]]
                before = (legs[1][0].detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
            for p, o in legs:
                p.grad = torch.from_numpy(g.copy()).to(p.dtype)
                o.step()
            param.grad = torch.from_numpy(g).cuda()
            opt.step()
            assert opt.flat_launches == 0
    _, mags = N.adam_step(before[0], g, before[1], before[2], lr, betas[0], betas[1], eps, 3)
    G = Grader(f"FusedAdam per tensor {'strided' if strided else 'dense'}")
    st = opt.state[param]
    assert int(st["step"]) == 3
    grade_adam(G, "3 steps", (param.detach(), st["exp_avg"], st["exp_avg_sq"]), legs, mags)
    G.done()
