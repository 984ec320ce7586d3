"""The Lovasz-softmax loss on the device (csrc/lovasz.hip, losses.LovaszSoftmaxLoss) against the numpy mirror tests/_lovasz_ref.py.

What is integer work is compared for EQUALITY: the error histograms, the present-class map and the pixel counters (the inputs
keep every float64 error 2^-16 away from a bin edge, tests/test_lovasz_host.py asserts it, so the device's fp32 bins are the
mirror's).  The coefficient tables are held to 2 fp32 ulp of the mirror's float64.  What is floating point is graded element-wise
against float64 under tests/_grade.Grader's bar max(4 x max(d), 2^-22), d the deviation of the same arithmetic in fp32: the loss,
the gradient and the column sums of the mirror GIVEN THE KERNEL'S TABLES.  Void and non-finite pixels hold exact zeros in all ldc
lanes of the gradient.  The returned loss lies within ``sum(slack)`` below the sort-based loss of the paper.

Inputs (``_lovasz_ref.make_inputs``): logits 3 * randn; the target is the argmax at 70 % of the pixels and random elsewhere; 10 %
void (255), a few targets out of range, one row with an inf.  Pad lanes of the logits hold junk (7.0, one lane 1e30), the
gradient buffer is pre-filled with junk.
"""
import numpy as np
import pytest
import torch

import _lovasz_ref as R
import _norm_ref as N
from _grade import Grader

pytestmark = pytest.mark.gpu

SHAPES = list(R.CASES)
IGN = R.IGN
SHAPE_MODES = [(s, i, m) for s in SHAPES for i, m in R.modes(s)]


class LovaszGrader(Grader):
    PREFIX = "lovasz-grade"


@pytest.fixture(scope="module")
def env():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels, losses
    _lib.require_gpu()
    return kernels, losses, _lib.load().udaseg_ce_partials()


def ceil4(c):
    return (c + 3) // 4 * 4


def pipeline(env, shape, images, mode, ce_weight=0.0, grad=True, zero_coef=False):
    """The launches of LovaszSoftmaxLoss on a buffer with junk in the pad lanes; every result as numpy."""
    K, _, np_ = env
    z, t = R.make_inputs(shape)
    n, c, h, w = shape
    B = R.CASES[shape]
    ldc, pixels = ceil4(c), n * h * w
    buf = torch.full((pixels, ldc), 7.0)
    buf[:, :c] = z.permute(0, 2, 3, 1).reshape(pixels, c)
    if ldc > c:
        buf[:, ldc - 1] = 1e30
    buf, tgt = buf.cuda(), t.reshape(-1).cuda()
    tables = torch.zeros((images, c, 2, B), device="cuda", dtype=torch.int32)
    counters = torch.zeros(4, device="cuda", dtype=torch.int64)
    K.lovasz_hist(buf, tgt, pixels, c, ldc, IGN, images, B, tables, counters)
    coef = torch.full((images, c, 2, B), 55.0, device="cuda")
    present = torch.full((images, c), 9, device="cuda", dtype=torch.int32)
    slack = torch.full((c,), -1.0, device="cuda", dtype=torch.float64)
    K.lovasz_table(tables, images, c, B, mode == "all", coef, present, torch.empty(images * c, device="cuda", dtype=torch.float64), slack)
    used = torch.zeros_like(coef) if zero_coef else coef
    loss = torch.empty((), device="cuda")
    partials = torch.empty(np_, device="cuda", dtype=torch.float64)
    dl = colsum = None
    if grad:
        dl = torch.full((pixels, ldc), 123.0, device="cuda")
        colsum = torch.empty(ldc, device="cuda")
        K.lovasz_fwd_bwd(buf, tgt, used, counters, pixels, c, ldc, IGN, images, B, ce_weight, partials, loss, dl,
                         torch.empty(np_ * ldc, device="cuda"), colsum)
    else:
        K.lovasz_fwd_bwd(buf, tgt, used, counters, pixels, c, ldc, IGN, images, B, ce_weight, partials, loss)
    out = dict(tables=tables, counters=counters, coef=coef, present=present, slack=slack, loss=loss, dl=dl, colsum=colsum)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


_RUNS = {}


def run(env, shape, images, mode):
    key = (shape, images, mode)
    if key not in _RUNS:
        _RUNS[key] = pipeline(env, shape, images, mode)
    return _RUNS[key]


_MIRROR = {}


def mirror(shape):
    """(rows, targets, e, fg, live) of a shape in float64, made once."""
    if shape not in _MIRROR:
        z, t = R.make_inputs(shape)
        rows, tf = R.nhwc_rows(z), t.view(-1).numpy()
        _MIRROR[shape] = (rows, tf) + R.errors(rows, tf, IGN)[:3]
    return _MIRROR[shape]


def fbits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def test_the_last_shape_passes_one_full_grid_of_both_passes(env):
    n, _, h, w = SHAPES[-1]
    assert 256 * env[2] < n * h * w and 512 * 512 < n * h * w


@pytest.mark.parametrize("shape,images,mode", SHAPE_MODES, ids=str)
def test_tables_present_and_counters_equal_the_mirror(env, shape, images, mode):
    rows, tf, e, fg, live = mirror(shape)
    got = run(env, shape, images, mode)
    want = R.tables(e, fg, R.CASES[shape], live, images)
    assert (got["tables"] == want).all(), int((got["tables"] != want).sum())
    _, void, invalid, nonfinite = R.pixel_classes(tf, shape[1], IGN, rows)
    assert got["counters"].tolist() == [int(live.sum()), int(void.sum()), int(invalid.sum()), int(nonfinite.sum())]
    assert (got["present"] == (want[:, :, 0].sum(-1) > 0)).all()


@pytest.mark.parametrize("shape,images,mode", SHAPE_MODES, ids=str)
def test_coefficients_and_slack_against_float64(env, shape, images, mode):
    got = run(env, shape, images, mode)
    co = R.coefficients(got["tables"], mode)
    g = LovaszGrader(f"table {shape} images={images} {mode}")
    g.ulp2("coef", got["coef"], co["coef"], np.zeros_like(co["coef"]))
    g.grade("slack", got["slack"], co["slack"], co["slack"], co["slack"])
    g.done()
    assert (got["coef"] >= 0).all()
    if mode == "present":
        assert (got["coef"][~co["present"]] == 0).all()
    assert 0.0 <= got["slack"].sum() <= 1.0 / R.CASES[shape] * (1 + 1e-12)


@pytest.mark.parametrize("shape,images,mode", SHAPE_MODES, ids=str)
def test_loss_gradient_and_column_sums_given_the_kernels_tables(env, shape, images, mode):
    rows, tf, e, fg, live = mirror(shape)
    c = shape[1]
    got = run(env, shape, images, mode)
    co = R.coefficients(got["tables"], mode)
    r64 = R.loss_and_grad(rows, tf, IGN, co["coef"], 0.0, R.F64)
    r32 = R.loss_and_grad(rows, tf, IGN, co["coef"], 0.0, R.F32)
    assert (got["dl"][~live] == 0).all() and (got["dl"][:, c:] == 0).all()   # exact zeros: all ldc lanes of the void, pad lanes
    assert (got["colsum"][c:] == 0).all()
    g = LovaszGrader(f"{shape} images={images} {mode}")
    g.grade("loss", got["loss"], np.float64(r64["loss"][0]), np.float64(r32["loss"][0]), r64["loss"][1])
    g.grade("grad", got["dl"][:, :c][live], r64["grad"][0][live], r32["grad"][0][live], r64["grad"][1][live])
    g.grade("colsum", got["colsum"][:c], r64["colsum"][0], r32["colsum"][0], r64["colsum"][1])
    g.done()
    # the grid against the sort: 0 <= L - loss <= sum(slack), each up to the loss's own bar
    tol = N.bar(np.float64(r32["loss"][0]), np.float64(r64["loss"][0]), r64["loss"][1])[0] * r64["loss"][1]
    exact = R.exact_lovasz(rows, tf, IGN, images, mode)
    gap, slack = exact - float(got["loss"]), float(got["slack"].sum())
    print(f"lovasz-bound {shape} images={images} {mode}: exact {exact:.9f} loss {float(got['loss']):.9f} gap {gap:.3e} "
          f"slack {slack:.3e} 1/B {1.0 / R.CASES[shape]:.3e} tol {tol:.1e}")
    assert -tol <= gap <= slack + tol
    if shape == R.DISTINCT:
        assert slack == 0.0 and abs(gap) <= tol


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=str)
def test_ce_weight_adds_the_cross_entropy_term(env, shape):
    """ce_weight = 1: the cross-entropy term alone (a zero coefficient table) and the sum of both terms, each graded."""
    rows, tf, e, fg, live = mirror(shape)
    c, images, mode = shape[1], shape[0], "present"
    lov = run(env, shape, images, mode)
    co = R.coefficients(lov["tables"], mode)
    g = LovaszGrader(f"ce_weight {shape}")
    for what, zero in (("ce alone", True), ("lovasz + ce", False)):
        got = pipeline(env, shape, images, mode, ce_weight=1.0, zero_coef=zero)
        r64 = R.loss_and_grad(rows, tf, IGN, co["coef"], 1.0, R.F64, lovasz=not zero)
        r32 = R.loss_and_grad(rows, tf, IGN, co["coef"], 1.0, R.F32, lovasz=not zero)
        assert (got["dl"][~live] == 0).all() and (got["dl"][:, c:] == 0).all()
        g.grade(f"{what} loss", got["loss"], np.float64(r64["loss"][0]), np.float64(r32["loss"][0]), r64["loss"][1])
        g.grade(f"{what} grad", got["dl"][:, :c][live], r64["grad"][0][live], r32["grad"][0][live], r64["grad"][1][live])
        g.grade(f"{what} colsum", got["colsum"][:c], r64["colsum"][0], r32["colsum"][0], r64["colsum"][1])
        if not zero:                                         # the sum of the two separately graded terms
            parts = [R.loss_and_grad(rows, tf, IGN, co["coef"], w, R.F64, lovasz=lv) for w, lv in ((0.0, True), (1.0, False))]
            assert abs(r64["loss"][0] - (parts[0]["loss"][0] + parts[1]["loss"][0])) < 1e-12
            assert np.abs(r64["grad"][0] - (parts[0]["grad"][0] + parts[1]["grad"][0])).max() < 1e-12
    g.done()


def test_two_calls_give_the_same_bits(env):
    shape = SHAPES[-1]
    a, b = (pipeline(env, shape, 1, "present", ce_weight=1.0) for _ in range(2))
    assert (a["tables"] == b["tables"]).all() and (a["counters"] == b["counters"]).all()
    for k in ("coef", "loss", "dl", "colsum"):
        assert (fbits(a[k]) == fbits(b[k])).all(), k
    assert (a["slack"].view(np.uint64) == b["slack"].view(np.uint64)).all()


def test_loss_alone_equals_the_loss_of_the_gradient_pass(env):
    shape = SHAPES[2]
    a = pipeline(env, shape, 2, "present", ce_weight=1.0, grad=False)
    b = pipeline(env, shape, 2, "present", ce_weight=1.0)
    assert fbits(a["loss"])[0] == fbits(b["loss"])[0]


@pytest.mark.parametrize("per_image,mode,ce_weight", [(False, "present", 0.0), (True, "all", 1.0)])
def test_module_is_the_direct_launches(env, per_image, mode, ce_weight):
    _, L, _ = env
    shape = SHAPES[2]
    c = shape[1]
    z, t = R.make_inputs(shape)
    images = shape[0] if per_image else 1
    got = pipeline(env, shape, images, mode, ce_weight=ce_weight)
    crit = L.LovaszSoftmaxLoss(classes=mode, per_image=per_image, ignore_index=IGN, bins=R.CASES[shape], ce_weight=ce_weight)
    zc = z.cuda().requires_grad_(True)
    loss = crit(zc, t.cuda())
    g1, = torch.autograd.grad(loss, zc, retain_graph=True)
    assert len(L.COLSUM_SIDE_TABLE) == 1
    colsum = next(iter(L.COLSUM_SIDE_TABLE.values())).cpu().numpy()
    assert (fbits(colsum) == fbits(got["colsum"])).all()
    g2, = torch.autograd.grad(loss, zc, retain_graph=True)   # a second backward: the launch again on the saved tables
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    g3, = torch.autograd.grad(loss * 2.5, zc)
    assert torch.equal(g3, g1 * 2.5)
    assert fbits(loss.item())[0] == fbits(got["loss"])[0]
    gz = g1.permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy()
    assert (fbits(gz) == fbits(got["dl"][:, :c])).all()
    assert crit.last_target_stats.tolist() == got["counters"].tolist()
    assert (crit.last_present.cpu().numpy() == got["present"]).all() and tuple(crit.last_present.shape) == (images, c)
    assert (crit.last_slack.cpu().numpy().view(np.uint64) == got["slack"].view(np.uint64)).all()
    with torch.no_grad():
        loss_ng = crit(z.cuda(), t.cuda())
    assert not loss_ng.requires_grad and fbits(loss_ng.item())[0] == fbits(loss.item())[0]
    zc2 = z.cuda().requires_grad_(True)
    crit(zc2, t.cuda()).backward()
    assert torch.equal(zc2.grad.view(torch.int32), g1.view(torch.int32))


def test_all_void_batch(env):
    _, L, _ = env
    z = torch.randn(2, 5, 20, 20, generator=torch.Generator().manual_seed(1))
    t = torch.full((2, 20, 20), IGN)
    for ce_weight, check in ((0.0, lambda v: v == 0.0), (1.0, np.isnan)):
        crit = L.LovaszSoftmaxLoss(per_image=True, ignore_index=IGN, bins=64, ce_weight=ce_weight)
        zc = z.cuda().requires_grad_(True)
        loss = crit(zc, t.cuda())
        loss.backward()
        assert check(loss.item()), (ce_weight, loss.item())
        assert (zc.grad == 0).all()
        assert crit.last_target_stats.tolist() == [0, 800, 0, 0] and int(crit.last_present.sum()) == 0
        assert float(crit.last_slack.sum()) == 0.0


def test_argument_checks(env):
    _, L, _ = env
    crit = L.LovaszSoftmaxLoss()
    with pytest.raises(ValueError, match="at most 32 classes"):
        crit(torch.zeros(1, 33, 4, 4, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.long, device="cuda"))
    with pytest.raises(ValueError, match="expected logits"):
        crit(torch.zeros(1, 5, 4, 4, device="cuda"), torch.zeros(1, 4, 5, dtype=torch.long, device="cuda"))


def test_trainer_runs_with_the_lovasz_criterion(env):
    """SegmentationTrainer(criterion=LovaszSoftmaxLoss(ignore_index=255, ce_weight=1.0)): one r18 step at 2 x 3 x 64 x 64."""
    _, L, _ = env
    from uda_aerial_semantic_segmentation_research_amd import data as D
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    msk = torch.randint(0, 23, (2, 64, 64), generator=g, dtype=torch.uint8)
    msk[:, :16] = IGN
    loader = D.DeviceAugmentedLoader([(img, msk)], generator=torch.Generator().manual_seed(9))
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23)
    crit = L.LovaszSoftmaxLoss(ignore_index=IGN, ce_weight=1.0)
    tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=crit)
    assert tr.criterion is crit
    train_loss = tr.train_epoch(loader, FusedAdam(net.parameters(), lr=1e-4), 1)
    n, void, invalid, nonfinite = crit.last_target_stats.tolist()
    assert np.isfinite(train_loss) and train_loss > 0
    assert void > 0 and invalid == 0 and nonfinite == 0 and n + void == 2 * 64 * 64
    assert 0.0 <= float(crit.last_slack.sum()) <= 1.0 / 1024 * (1 + 1e-12) and int(crit.last_present.sum()) > 0


def test_hist_counters_accumulate_and_a_zero_kind_issues_nothing(env):
    """lovasz_hist's four pixel counters at 2 x 5 x 25 x 30 (1500 pixels, 750 an image: 512-thread blocks with a ragged last wave,
    one block an image adding into the same four words), into a buffer that holds 9 already; no target is out of range and no row is
    non-finite, so two of the four stay at 9.  Counted by the mirror's pixel_classes."""
    K = env[0]
    n, c, h, w, bins = 2, 5, 25, 30, 64
    ldc, pixels = 8, n * h * w
    g = torch.Generator().manual_seed(12)
    buf = torch.randn(pixels, ldc, generator=g)
    t = torch.randint(0, c, (pixels,), generator=g)
    t[::9] = IGN
    live, void, invalid, nonfinite = R.pixel_classes(t.numpy(), c, IGN, buf[:, :c].numpy())
    assert void.sum() > 0 and invalid.sum() == 0 and nonfinite.sum() == 0
    tables = torch.zeros((n, c, 2, bins), device="cuda", dtype=torch.int32)
    counters = torch.full((4,), 9, device="cuda", dtype=torch.int64)
    K.lovasz_hist(buf.cuda(), t.cuda(), pixels, c, ldc, IGN, n, bins, tables, counters)
    assert counters.tolist() == [9 + int(live.sum()), 9 + int(void.sum()), 9, 9]
    assert int(tables.sum()) == c * int(live.sum())                             # every live pixel puts one error a class
