"""CPU checks of the distillation feature: the float64 leg of tests/_distill_ref.py against torch's double-precision autograd
(``F.cross_entropy`` with probability targets, ``F.kl_div``, the symmetric term written out; weights, void pixels and divisors by
hand), the float32 leg against the bar of tests/test_gpu_distill.py on every case that test runs, each deliberate mutation of the
float32 leg caught by that grading, the mirrors of ``confidence_share`` and ``pixel_weight_sum`` against plain numpy, and the
host-side surface: refusals before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _distill_ref as D
from _distill_ref import F32, F64


def _quiet(_line):
    pass


# ------------------------------------------------------------------------------------------ float64 leg vs torch autograd
def _torch_reference(z, t, w, why, probs, kind, hp, reduction, div):
    """The textbook composition in torch float64 with autograd.  Void rows are given a harmless teacher row and weight 0."""
    dead = why != 0
    t = np.where(dead[:, None], 1.0 / z.shape[1], t.astype(F64))
    x = torch.tensor(z.astype(F64), requires_grad=True)
    tt = torch.tensor(t)
    q = tt if probs else torch.softmax(tt * float(hp["inv_temp"]), 1)
    lp = torch.log_softmax(x, 1)
    ce = F.cross_entropy(x, q, reduction="none")
    if kind == "ce":
        l = ce
    elif kind == "kl":
        l = F.kl_div(lp, q, reduction="none").sum(1)
    else:
        g = -torch.clamp(torch.log(q), min=float(hp["log_floor"]))
        l = float(hp["alpha"]) * ce + float(hp["beta"]) * (torch.softmax(x, 1) * g).sum(1)
    wt = torch.tensor(np.where(dead, 0.0, w.astype(F64)))
    loss = (wt * l).sum() / div
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize("classes", [2, 5, 23])
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("probs", [0, 1])
@pytest.mark.parametrize("reduction", D.REDUCTIONS)
def test_float64_leg_is_the_textbook(classes, kind, probs, reduction):
    batch, ppi = 3, 30
    z, tl, tp, wpx, wimg = D.make_case(batch, ppi, classes, 17 + classes)
    t = tp if probs else tl
    out = D.soft_ce(z, t, wpx, wimg, batch, ppi, probs, kind, D.HP, reduction, F64)
    w, why = D.classify(t, wpx, wimg, batch, ppi, probs, D.HP)
    assert set(np.unique(why)) == {0, 1, 2}
    div = {"mean": batch * ppi, "sum": 1.0, "weighted_mean": float(D.pixel_weight_sum(wpx, wimg, batch, ppi)[0])}[reduction]
    loss, grad = _torch_reference(z, t, w, why, probs, kind, D.HP, reduction, div)
    assert abs(float(out["loss"][0]) - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(out["grad"][0] - grad).max() <= 1e-12 * max(1.0, np.abs(grad).max())
    assert np.abs(out["colsum"][0] - grad.sum(0)).max() <= 1e-11 * max(1.0, np.abs(grad).max())
    assert not out["grad"][0][why != 0].any() and not out["grad"][1][why != 0].any()      # value 0, magnitude 0: only 0 passes
    assert (out["stats"] == [(why == 0).sum(), (why == 1).sum(), (why == 2).sum()]).all()


def test_zero_lanes_contribute_exactly_zero():
    """One-hot probabilities: the zero lanes add nothing (never 0 * inf) although the student's log probability there is -200."""
    z = np.array([[200.0, 0.0, 0.0], [0.0, 200.0, 0.0]], dtype=F32)
    tp = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=F32)
    for elem in (F64, F32):
        ce = D.soft_ce(z, tp, None, None, 1, 2, 1, "ce", D.HP, "sum", elem)
        kl = D.soft_ce(z, tp, None, None, 1, 2, 1, "kl", D.HP, "sum", elem)
        assert abs(float(ce["loss"][0]) - 200.0) < 1e-4 and abs(float(kl["loss"][0]) - 200.0) < 1e-4
        sym = D.soft_ce(z, tp, None, None, 1, 2, 1, "symmetric", dict(D.HP, alpha=0.0, beta=1.0), "sum", elem)
        # row 0: p = (1, 0, 0), g = (0, 4, 4): 0;  row 1: p = (0, 1, 0): 4
        assert abs(float(sym["loss"][0]) - 4.0) < 1e-4
        assert np.isfinite(sym["grad"][0]).all() and np.isfinite(ce["grad"][0]).all()


def test_weighted_mean_of_nothing_is_nan_and_its_gradient_zero():
    z, tl, tp, wpx, wimg = D.make_case(1, 4, 5, 3, "w_zero")
    for elem in (F64, F32):
        out = D.soft_ce(z, tl, wpx, wimg, 1, 4, 0, "ce", D.HP, "weighted_mean", elem)
        assert np.isnan(out["loss"][0]) and not out["grad"][0].any() and list(out["stats"]) == [0, 4, 0]


# --------------------------------------------------------------------------------------------- float32 leg meets the bar
@pytest.mark.parametrize("classes", D.CLASSES)
@pytest.mark.parametrize("shape", D.SHAPES)
def test_float32_leg_meets_the_bar(shape, classes):
    D.grade_case(D.LegBackend(), shape[0], shape[1], classes, 100 * classes + shape[1], _quiet).done()


@pytest.mark.parametrize("row_kind", D.ROW_KINDS)
def test_float32_leg_meets_the_bar_on_single_rows(row_kind):
    for classes in D.CLASSES:
        D.grade_case(D.LegBackend(), 1, 1, classes, 7 * classes, _quiet, row_kind=row_kind).done()


@pytest.mark.parametrize("classes,ldc,ldt", [(5, 8, 32), (5, 16, 8), (23, 24, 32)])
def test_float32_leg_meets_the_bar_with_unequal_strides(classes, ldc, ldt):
    D.grade_case(D.LegBackend(), 3, 85, classes, 41, _quiet, ldc=ldc, ldt=ldt, combos=D.COVER).done()


def test_float32_leg_meets_the_bar_past_the_grid():
    D.grade_case(D.LegBackend(), D.BIG[0], D.BIG[1], 23, 5, _quiet, combos=D.COVER[:3], weight_variants=False).done()


# ------------------------------------------------------------------------------------------------- mutations are caught
@pytest.mark.parametrize("mut,combos", [
    ("no_Q", (("ce", 1, "mean"),)),                           # the sub-normalised probability rows: Q = 0.7
    ("floor_after_negation", (("symmetric", 1, "mean"),)),
    ("floor_after_negation", (("symmetric", 0, "sum"),)),
    ("void_grad", (("kl", 0, "mean"),)),
    ("wimg_by_pixel", (("ce", 0, "mean"),)),
    ("wimg_by_pixel", (("ce", 0, "weighted_mean"),)),
    ("double_divisor", (("ce", 0, "mean"),)),
    ("double_divisor", (("symmetric", 1, "weighted_mean"),)),
    ("no_rowsum", (("symmetric", 0, "mean"),)),
])
def test_each_mutation_is_caught(mut, combos):
    assert mut in D.MUTATIONS
    g = D.grade_case(D.LegBackend(mut), 3, 85, 5, 31, _quiet, combos=combos, weight_variants=False)
    assert g.bad, f"the grading let the mutation {mut!r} through"
    with pytest.raises(AssertionError):
        g.done()
    D.grade_case(D.LegBackend(), 3, 85, 5, 31, _quiet, combos=combos, weight_variants=False).done()


def test_every_mutation_has_a_case():
    marks = [m for m in test_each_mutation_is_caught.pytestmark if m.name == "parametrize"]
    assert {row[0] for row in marks[0].args[1]} == set(D.MUTATIONS)


# ------------------------------------------------------------------------------------------------------------- mirrors
def test_confidence_share_mirror_against_plain_numpy():
    for classes, probs, tau in ((5, 0, 0.6), (23, 1, 0.3), (2, 0, 0.5)):
        batch, ppi = 3, 85
        s = D.make_scores(batch, ppi, classes, 9, probs, tau)
        above, nonfinite, share = D.conf_share(s, batch, ppi, probs, tau)
        c64 = D.conf64(s, probs)
        with np.errstate(invalid="ignore"):
            bad = ~np.isfinite(c64) | (np.isnan(s).any(1)) | ((c64 > 1) if probs else False)
            hit = ~bad & (c64 >= float(F32(tau)) - (0 if probs else 2.0 ** -20))
        img = np.arange(batch * ppi) // ppi
        assert (nonfinite == np.bincount(img[bad], minlength=batch)).all() and nonfinite.sum() > 0
        assert (above == np.bincount(img[hit], minlength=batch)).all() and 0 < above.sum() < batch * ppi
        assert (share == (above / ppi).astype(F32)).all() and share.dtype == F32
    # the >= is exact: a probability of exactly tau counts, the next float below does not
    s = np.array([[0.25, 0.75], [0.25, np.nextafter(F32(0.75), F32(0))]], dtype=F32)
    assert list(D.conf_share(s, 2, 1, 1, 0.75)[0]) == [1, 0]
    assert list(D.conf_share(np.zeros((2, 2), dtype=F32), 1, 2, 0, 0.5)[0]) == [2]       # uniform over two classes: exactly 0.5


def test_pixel_weight_sum_mirror_against_plain_numpy():
    wpx = np.array([1.0, 0.0, -1.0, np.nan, 0.5, np.inf, 2.0, 0.25], dtype=F32)
    wimg = np.array([2.0, 0.5], dtype=F32)
    d, counts = D.pixel_weight_sum(wpx, wimg, 2, 4)
    assert d == 2.0 + 0.25 + 1.0 + 0.125 and list(counts) == [1, 3]
    d, counts = D.pixel_weight_sum(None, wimg, 2, 4)
    assert d == 10.0 and list(counts) == [0, 0]
    d, counts = D.pixel_weight_sum(None, np.array([0.0, 1.0], dtype=F32), 2, 4)
    assert d == 4.0 and list(counts) == [4, 0]
    d, counts = D.pixel_weight_sum(None, None, 2, 4)
    assert d == 8.0 and list(counts) == [0, 0]
    w, why = D.pixel_weights(wpx, np.array([0.0, 1.0], dtype=F32), 2, 4)
    assert list(why) == [1, 1, 1, 2, 0, 2, 0, 0]                                          # NaN * 0 is NaN: invalid, not zero


# ------------------------------------------------------------------------------------------------------- host surface
def test_module_checks_its_arguments():
    from uda_aerial_semantic_segmentation_research_amd.losses import SoftCrossEntropyLoss
    for bad in (dict(kind="mse"), dict(reduction="none"), dict(teacher_temperature=0.0), dict(teacher_temperature=float("inf")),
                dict(log_floor=0.0), dict(log_floor=4.0), dict(alpha=float("nan")), dict(beta=float("inf"))):
        with pytest.raises(ValueError):
            SoftCrossEntropyLoss(**bad)
    loss = SoftCrossEntropyLoss("symmetric", teacher_temperature=2.0, alpha=0.1, beta=1.0, reduction="weighted_mean")
    assert "symmetric" in repr(loss) and loss.last_stats is None
    z, t = torch.zeros(2, 5, 8, 8), torch.zeros(2, 5, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(z, t)
    for c in (1, 33):
        with pytest.raises(ValueError, match="2 to 32 classes"):
            loss(torch.zeros(1, c, 8, 8), torch.zeros(1, c, 8, 8))
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        loss(torch.zeros(5, 8, 8), torch.zeros(5, 8, 8))


def test_confidence_share_checks_its_arguments():
    from uda_aerial_semantic_segmentation_research_amd.pseudo import confidence_share
    with pytest.raises(ValueError, match="tau"):
        confidence_share(torch.zeros(1, 5, 8, 8), 1.5)
    with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
        confidence_share(torch.zeros(5, 8, 8), 0.9)
    with pytest.raises(ValueError, match="num_classes"):
        confidence_share(torch.zeros(1, 33, 8, 8), 0.9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        confidence_share(torch.zeros(1, 5, 8, 8), 0.9)


def test_entry_points_validate_before_any_launch():
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    P = 4096                                     # a non-NULL, 16-byte aligned "pointer": validation fails before anything is dereferenced
    ok = dict(batch=2, ppi=32, classes=5, ldc=8, ldt=8, probs=0, kind=0, it=1.0, alpha=1.0, beta=1.0, floor=-4.0, mean=1, denom=None)

    def soft(**over):
        a = {**ok, **over}
        return lib.udaseg_soft_ce_fwd_bwd(a.get("logits", P), a.get("teacher", P), None, None, a["batch"], a["ppi"], a["classes"],
                                          a["ldc"], a["ldt"], a["probs"], a["kind"], a["it"], a["alpha"], a["beta"], a["floor"],
                                          a["mean"], a["denom"], a.get("partials", P), P, None, a.get("cparts"), a.get("colsum"),
                                          None, None)

    for over in (dict(classes=1), dict(classes=33, ldc=36, ldt=36), dict(ldc=6), dict(ldc=4), dict(ldt=4), dict(ldt=36), dict(batch=0),
                 dict(ppi=0), dict(probs=2), dict(kind=3), dict(kind=-1), dict(it=0.0), dict(it=float("inf")), dict(kind=2, floor=0.0),
                 dict(kind=2, alpha=float("nan")), dict(mean=1, denom=P), dict(logits=None), dict(teacher=None), dict(partials=None),
                 dict(logits=P + 4), dict(colsum=P), dict(cparts=P)):
        assert soft(**over) == -1, over
        assert lib.udaseg_last_error()
    assert soft(kind=3) == -1 and b"kind" in lib.udaseg_last_error()
    assert lib.udaseg_pixel_weight_sum(None, None, 0, 4, P, P, P, None) == -1
    assert lib.udaseg_pixel_weight_sum(None, None, 2, 4, None, P, P, None) == -1
    for args in ((P, 0, 64, 5, 8, 0), (P, 2, 0, 5, 8, 0), (P, 2, 64, 33, 36, 0), (P, 2, 64, 5, 6, 0), (P, 2, 64, 5, 8, 2),
                 (None, 2, 64, 5, 8, 0), (P + 4, 2, 64, 5, 8, 0), (P, 65536, 64, 5, 8, 0)):
        assert lib.udaseg_conf_share(*args, 0.9, P, P, P, None) == -1, args
    assert lib.udaseg_conf_share(P, 2, 64, 5, 8, 0, float("nan"), P, P, P, None) == -1 and b"tau" in lib.udaseg_last_error()
    assert lib.udaseg_seg_partials() == D.BLOCKS


def test_trainer_refuses_bad_arguments_and_a_gradient_reducer_before_touching_anything():
    from uda_aerial_semantic_segmentation_research_amd.distill import DistillTrainer
    tr = DistillTrainer.__new__(DistillTrainer)
    tr.grad_reducer = object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.distill_step(None, None, None, None)
    net = torch.nn.Conv2d(3, 5, 1)
    net.classes = 5
    cpu = torch.device("cpu")
    for bad in (dict(teacher=None), dict(teacher=net), dict(teacher=torch.nn.Conv2d(3, 5, 1), loss=torch.nn.MSELoss()),
                dict(teacher=torch.nn.Conv2d(3, 5, 1), tau=1.5), dict(teacher=torch.nn.Conv2d(3, 5, 1), bank=object())):
        with pytest.raises(ValueError):
            DistillTrainer(net, cpu, **bad)
    tr = DistillTrainer(net, cpu, torch.nn.Conv2d(3, 5, 1), lambda_soft=0.5)
    assert tr.teacher is None and tr.lambda_soft == 0.5 and tr.soft_loss.kind == "ce" and tr.tau == 0.968
