"""The loss and discriminator-tail kernels (csrc/losses_seg.hip: Dice per image and pooled, focal-weighted cross entropy,
consistency; csrc/losses.hip: plain cross entropy with its column sums, global average pool -> linear -> sigmoid, BCE with logits)
against the float64 restatement of tests/_loss_ref.py (proven against torch's double-precision autograd by
tests/test_loss_ref_host.py), called at kernel level through kernels.py.

The bar is the one of tests/test_gpu_norm_grade.py: with e = |kernel - f64| / magnitude and d = |fp32 leg - f64| / magnitude
element-wise (magnitude: the sum of the absolute values of the terms that formed the element, from _loss_ref),
max(e) <= max(4 x max(d), 2^-22), scalar values included.  Logits sit in padded NHWC buffers whose pad lanes hold finite junk
(7.0, and one lane 1e30); every output buffer is pre-filled with NaN; the pad lanes and the void rows of every gradient must come
back exactly 0.  No element is masked out: the one discontinuity, focal's om > 0 branch, is absorbed by the 1 + pt magnitude, and
every focal case asserts on the CPU, before any launch, that the float32 leg meets the bar across it.

The cases, their data and the grading live in tests/_loss_cases.py, where tests/test_loss_ref_host.py runs the same code with the
float32 leg (and nine mutations of it) in the kernels' place.  Set UDASEG_DEVIATION_LOG to a file name to collect the figures
(profiles/loss_grade.txt).
"""
import os

import numpy as np
import pytest
import torch

import _loss_cases as C
import _loss_ref as R
from _loss_ref import F32, F64, f32

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def scalar(v):
    return None if v is None else torch.tensor(f32(v), dtype=torch.float32, device="cuda")


def out_like(shape, old, dtype=torch.float32):
    """An output buffer: NaN everywhere, or the seeded values an accumulating call adds to."""
    if old is None:
        return torch.full(shape, NAN, dtype=dtype, device="cuda")
    return dev(np.asarray(old, dtype=F32), dtype).reshape(shape)


class GpuBackend:
    """tests/_loss_cases.py's operations on the HIP kernels, numpy in and out."""
    def __init__(self, K, lib):
        self.K, self.seg_partials, self.ce_partials = K, K.seg_partials(), lib.udaseg_ce_partials()

    def dice(self, zbuf, t, batch, classes, smooth, eps, pooled, ignore_index, go, weight, old=None):
        K, (pixels, ldc) = self.K, zbuf.shape
        z, tt = dev(zbuf), dev(t)
        sums = torch.zeros(batch * 3 * classes, dtype=torch.float64, device="cuda")
        coef, loss = out_like((batch * 2 * classes,), None), out_like((), None)
        K.dice_fwd(z, tt, batch, pixels // batch, classes, ldc, smooth, sums, coef, loss, eps, pooled, ignore_index=ignore_index)
        d = out_like((pixels, ldc), old)
        K.dice_bwd(z, tt, coef, scalar(go), f32(weight), batch, pixels // batch, classes, ldc, d, old is not None, ignore_index=ignore_index)
        return host(loss), host(coef).reshape(batch, 2, classes), host(d)

    def focal_fwd(self, zbuf, t, class_w, alpha, gamma, mean, classes, ignore_index, old=None):
        pixels, ldc = zbuf.shape
        parts = torch.full((self.seg_partials,), NAN, dtype=torch.float64, device="cuda")
        loss = out_like((), old)
        self.K.focal_fwd(dev(zbuf), dev(t), None if class_w is None else dev(class_w), alpha, gamma, pixels, classes, ldc, mean, parts,
                         loss, old is not None, ignore_index=ignore_index)
        return host(loss)

    def focal_bwd(self, zbuf, t, class_w, alpha, gamma, classes, ignore_index, go, weight, old=None):
        pixels, ldc = zbuf.shape
        d = out_like((pixels, ldc), old)
        self.K.focal_bwd(dev(zbuf), dev(t), None if class_w is None else dev(class_w), alpha, gamma, scalar(go), f32(weight), pixels,
                         classes, ldc, d, old is not None, ignore_index=ignore_index)
        return host(d)

    def consistency(self, z1buf, z2buf, temperature, batch, classes, go, weight, which="both", old=None):
        pixels, ldc = z1buf.shape
        z1, z2 = dev(z1buf), dev(z2buf)
        parts = torch.full((self.seg_partials,), NAN, dtype=torch.float64, device="cuda")
        loss = out_like((), None)
        self.K.consistency_fwd(z1, z2, temperature, batch, pixels, classes, ldc, parts, loss)
        d1 = out_like((pixels, ldc), None if old is None else old[0]) if which in ("both", "d1") else None
        d2 = out_like((pixels, ldc), None if old is None else old[1]) if which in ("both", "d2") else None
        self.K.consistency_bwd(z1, z2, temperature, scalar(go), f32(weight), batch, pixels, classes, ldc, d1, d2, old is not None)
        return host(loss), None if d1 is None else host(d1), None if d2 is None else host(d2)

    def ce(self, zbuf, t, classes, go, fused=False):
        K, (pixels, ldc) = self.K, zbuf.shape
        z, tt = dev(zbuf), dev(t)
        parts = torch.full((self.ce_partials,), NAN, dtype=torch.float64, device="cuda")
        loss, lse, d = out_like((), None), out_like((pixels,), None), out_like((pixels, ldc), None)
        cparts = out_like((self.ce_partials * ldc,), None) if ldc <= 32 else None
        colsum = out_like((ldc,), None) if ldc <= 32 else None
        if fused:
            assert go is None
            K.ce_fwd_bwd(z, tt, pixels, classes, ldc, parts, loss, d, cparts, colsum)
            return host(loss), None, host(d), host(colsum)
        K.ce_fwd(z, tt, pixels, classes, ldc, lse, parts, loss)
        K.ce_bwd(z, tt, lse, scalar(go), pixels, classes, ldc, d, cparts, colsum)
        return host(loss), host(lse), host(d), None if colsum is None else host(colsum)

    def tail_fwd(self, z, w, b, sigmoid, bf16=False):
        n, hw, c = z.shape
        zd = dev(z.reshape(n, hw, 1, c), torch.bfloat16 if bf16 else None)      # exact: bf16 cases hold bf16-rounded values
        out, pooled = (self.K.gap_linear_sigmoid_fwd if sigmoid else self.K.gap_linear_fwd)(zd, dev(w), dev(b))
        return host(out).reshape(-1), host(pooled)

    def tail_bwd(self, dp, p, pooled, w, hw, sigmoid, old=None, bf16=False):
        n, c = pooled.shape
        dz = out_like((n, hw, 1, c), None, torch.bfloat16 if bf16 else torch.float32)
        dw = out_like((c,), None if old is None else old[0])
        db = out_like((1,), None if old is None else [old[1]])
        if sigmoid:
            self.K.gap_linear_sigmoid_bwd(dev(dp), dev(np.asarray(p, dtype=F32).reshape(n, 1)), dev(pooled), dev(w), dz, dw, db, old is not None)
        else:
            self.K.gap_linear_bwd(dev(dp), dev(pooled), dev(w), dz, dw, db, old is not None)
        return host(dz).reshape(n, hw, c), host(dw), host(db)[0]

    def bce_fwd(self, x, y, weight, old=None):
        loss = out_like((), old)
        if np.ndim(y):
            self.K.bce_logits_target_fwd(dev(x), dev(y), f32(weight), loss, old is not None)
        else:
            self.K.bce_logits_fwd(dev(x), float(y), f32(weight), loss, old is not None)
        return host(loss)

    def bce_bwd(self, x, y, weight, go, old=None):
        dx = out_like((x.size,), old)
        if np.ndim(y):
            self.K.bce_logits_target_bwd(dev(x), dev(y), f32(weight), scalar(go), dx, old is not None)
        else:
            self.K.bce_logits_bwd(dev(x), float(y), f32(weight), scalar(go), dx, old is not None)
        return host(dx)


@pytest.fixture(scope="module")
def B():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    lib = _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    return GpuBackend(kernels, lib)


def run(B, family, case):
    C.FAMILIES[family][2](B, case, _log)
    torch.cuda.synchronize()


def cases(family):
    cs, ident, _ = C.FAMILIES[family]
    return pytest.mark.parametrize("case", cs, ids=[ident(c) for c in cs])


def test_the_shapes_reach_every_launch_regime():
    """Pure Python: the grid arithmetic the cases below rely on (tests/test_loss_ref_host.py pins the rest of it)."""
    assert [C.grid_pix(p) for p in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert C.grid_pix(262_656) == 1024 and C.passes(262_656) == 2                           # SL_BLOCKS / CE_BLOCKS = 1024
    assert C.grid_pix(65_792, 256) == 256 and C.passes(65_792, 256) == 2                    # dice_stats: gridDim.x <= 256
    assert C.straddling_blocks(3, 35) == [0] and C.straddling_blocks(2, 272) == [1]         # b = p / pix_per_image within a block
    assert C.ce_row_groups(24) == (10, 240) and C.ce_row_groups(12) == (21, 252)
    assert R.gap_slices(33) == (32, 2, 17) and R.gap_slices(4096) == (32, 128, 32)


@cases("launch")
def test_segmentation_losses_at_every_launch_shape(B, case):
    """All eight template instances (ldc 4 ... 32, classes = ldc - 1; classes = ldc at 4 and 32; one class) at three images of 35
    pixels, one block that straddles all of them; 1, 255, 256, 257 pixels; the second grid-stride pass of every kernel."""
    run(B, "launch", case)


@cases("focal_edge")
def test_focal_data_edges(B, case):
    run(B, "focal_edge", case)


@cases("focal_void")
def test_focal_void_labels(B, case):
    run(B, "focal_void", case)


@cases("dice_edge")
def test_dice_data_edges(B, case):
    """A class absent from one image and one absent from the batch in every case; per image, pooled, and pooled with the clamp taken."""
    run(B, "dice_edge", case)


@cases("dice_void")
def test_dice_void_labels(B, case):
    run(B, "dice_void", case)


@cases("consistency_edge")
def test_consistency_data_edges(B, case):
    run(B, "consistency_edge", case)


@cases("seg_accumulate")
def test_segmentation_accumulate_flags(B, case):
    run(B, "seg_accumulate", case)


@cases("ce")
def test_cross_entropy(B, case):
    run(B, "ce", case)


@cases("ce_width")
def test_cross_entropy_at_every_launch_width(B, case):
    """All sixteen widths of ce_fwd and ce_bwd (the tiled kernels to ldc 32, the simple ones beyond) and the eight of ce_fwd_bwd."""
    run(B, "ce_width", case)


@cases("tail")
def test_discriminator_tail(B, case):
    run(B, "tail", case)


@cases("bce")
def test_bce_with_logits(B, case):
    run(B, "bce", case)


# ------------------------------------------------------------------------------------------------------ through the modules
MOD_SHAPE = (2, 23, 9, 11)


def module_inputs(seed, zero_copy):
    """[N, C, H, W] logits that are either the zero-copy view of a padded NHWC buffer with junk in its pad lanes (what Unet.forward
    returns; padded_nhwc takes it as it is) or a non-contiguous NCHW tensor (padded_nhwc runs its layout kernel)."""
    n, c, h, w = MOD_SHAPE
    rng = np.random.default_rng(seed)
    t = C.make_target(rng, n, h * w, c)
    z = C.make_logits(rng, n * h * w, c, "randn3", t)
    if zero_copy:
        x = dev(C.pad_buf(z, 24)).view(n, h, w, 24).permute(0, 3, 1, 2)[:, :c]
    else:
        x = dev(z.reshape(n, h, w, c).transpose(0, 3, 2, 1)).transpose(2, 3)           # [N, C, W, H] storage
        assert not x.is_contiguous() and x.stride(1) != 1
    return z, t, x.detach().requires_grad_(True), dev(t).view(n, h, w)


def pixel_major(g):
    return host(g.permute(0, 2, 3, 1)).reshape(-1, g.shape[1])


@pytest.fixture(scope="module")
def L():
    from uda_aerial_semantic_segmentation_research_amd import _lib, losses
    _lib.require_gpu()
    return losses


GO = 0.37


def back(loss):
    loss.backward(torch.tensor(f32(GO), device="cuda"))


@pytest.mark.parametrize("zero_copy", [True, False], ids=["padded-view", "non-contiguous"])
def test_dice_modules(L, zero_copy):
    n, c, h, w = MOD_SHAPE
    G = R.Grader(f"modules dice zero_copy={zero_copy}", _log)
    for name, mod, pooled, smooth in (("DiceLoss", L.DiceLoss(smooth=1.0), False, 1.0), ("MulticlassDiceLoss", L.MulticlassDiceLoss(), True, 0.0)):
        z, t, x, tt = module_inputs(11, zero_copy)
        loss = mod(x, tt)
        back(loss)
        r64, r32 = (R.dice(z, t, n, smooth, 1e-7, pooled, None, C.scales(GO, 1.0)[k], e) for k, e in ((0, F64), (1, F32)))
        G.grade(f"{name} value", host(loss), *C._trip(r64, r32, "loss"))
        G.grade(f"{name} gradient", pixel_major(x.grad), *C._trip(r64, r32, "grad"))
    G.done()


@pytest.mark.parametrize("zero_copy", [True, False], ids=["padded-view", "non-contiguous"])
def test_weighted_segmentation_module(L, zero_copy):
    n, c, h, w = MOD_SHAPE
    G = R.Grader(f"modules WeightedSegmentationLoss zero_copy={zero_copy}", _log)
    z, t, x, tt = module_inputs(12, zero_copy)
    cw = (np.random.default_rng(5).random(c) + 0.5).astype(F32)
    dw = f32(0.7)
    loss = L.WeightedSegmentationLoss(c, torch.from_numpy(cw), alpha=0.25, gamma=2.0)(x, tt, dw)
    back(loss)
    g = float(F32(f32(GO)) * F32(dw))                       # the upstream gradient the kernels receive
    legs = []
    for k, e in ((0, F64), (1, F32)):
        f = R.focal(z, t, cw, 0.25, 2.0, True, None, C.scales(g, f32(1.0 / t.size))[k], e)
        d = R.dice(z, t, n, 1.0, 1e-7, False, None, C.scales(g, 1.0)[k], e)
        legs.append({"loss": (e(dw) * (f["loss"][0] + d["loss"][0]), dw * (f["loss"][1] + d["loss"][1])),
                     "grad": (f["grad"][0] + d["grad"][0], f["grad"][1] + d["grad"][1])})
    G.grade("value", host(loss), *C._trip(legs[0], legs[1], "loss"))
    G.grade("gradient", pixel_major(x.grad), *C._trip(legs[0], legs[1], "grad"))
    G.done()


def test_consistency_module(L):
    """pred1 the padded view, pred2 non-contiguous; and identical inputs give exactly 0 everywhere."""
    n, c, h, w = MOD_SHAPE
    G = R.Grader("modules ConsistencyLoss", _log)
    z1, _, x1, _ = module_inputs(13, True)
    z2, _, x2, _ = module_inputs(14, False)
    loss = L.ConsistencyLoss(0.7)(x1, x2)
    back(loss)
    inv_t = float(F32(1) / F32(0.7))
    r64, r32 = (R.consistency(z1, z2, inv_t, n, C.scales(GO, 1.0)[k], e) for k, e in ((0, F64), (1, F32)))
    G.grade("value", host(loss), *C._trip(r64, r32, "loss"))
    G.grade("d1", pixel_major(x1.grad), *C._trip(r64, r32, "d1"))
    G.grade("d2", pixel_major(x2.grad), *C._trip(r64, r32, "d2"))
    _, _, a, _ = module_inputs(13, True)
    b = a.detach().clone().requires_grad_(True)
    same = L.ConsistencyLoss(0.5)(a, b)
    back(same)
    G.zero("identical inputs: value", host(same))
    G.zero("identical inputs: d1", host(a.grad))
    G.zero("identical inputs: d2", host(b.grad))
    G.done()


def test_bce_modules(L):
    G = R.Grader("modules BCE", _log)
    rng = np.random.default_rng(15)
    xs, xt = (rng.standard_normal((5, 1)) * 3).astype(F32), (rng.standard_normal((5, 1)) * 3).astype(F32)
    y = rng.random((5, 1)).astype(F32)
    y[0], y[1] = 0.0, 1.0
    g = f32(GO)
    # BCEWithLogitsLoss(x, y)
    a = dev(xs).requires_grad_(True)
    loss = L.BCEWithLogitsLoss()(a, dev(y))
    back(loss)
    r64, r32 = (R.bce(xs, y.reshape(-1), 1.0, g, e) for e in (F64, F32))
    G.grade("BCEWithLogitsLoss value", host(loss), *C._trip(r64, r32, "loss"))
    G.grade("BCEWithLogitsLoss gradient", host(a.grad).reshape(-1), *C._trip(r64, r32, "dx"))
    # AdversarialLoss.discriminator_loss = (bce(source, 1) + bce(target, 0)) / 2: the second term accumulates into the first
    adv = L.AdversarialLoss(lambda_adv=0.01)
    a, b = dev(xs).requires_grad_(True), dev(xt).requires_grad_(True)
    loss = adv.discriminator_loss(a, b)
    back(loss)
    s = [(R.bce(xs, 1.0, 0.5, g, e), R.bce(xt, 0.0, 0.5, g, e)) for e in (F64, F32)]
    G.grade("discriminator_loss value", host(loss), s[0][0]["loss"][0] + s[0][1]["loss"][0],
            F32(s[1][0]["loss"][0] + s[1][1]["loss"][0]), s[0][0]["loss"][1] + s[0][1]["loss"][1])
    G.grade("discriminator_loss d source", host(a.grad).reshape(-1), s[0][0]["dx"][0], s[1][0]["dx"][0], s[0][0]["dx"][1])
    G.grade("discriminator_loss d target", host(b.grad).reshape(-1), s[0][1]["dx"][0], s[1][1]["dx"][0], s[0][1]["dx"][1])
    b = dev(xt).requires_grad_(True)
    loss = adv.generator_loss(b)
    back(loss)
    r64, r32 = (R.bce(xt, 1.0, f32(0.01), g, e) for e in (F64, F32))
    G.grade("generator_loss value", host(loss), *C._trip(r64, r32, "loss"))
    G.grade("generator_loss gradient", host(b.grad).reshape(-1), *C._trip(r64, r32, "dx"))
    G.done()
