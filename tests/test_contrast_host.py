"""CPU checks of the prototype contrast feature: the float64 leg of tests/_contrast_ref.py against torch's double-precision
autograd of ``cross_entropy(-(dist - dist.min) * inv_tau, t)`` over the seen classes (both target forms; weights, void pixels and
divisors by hand), ``proto.contrast_mirror`` / ``proto.assign_mirror`` against that leg and against ``rectify_mirror``, the float32
leg against the bar of tests/test_gpu_contrast.py on the cases that test runs, each deliberate mutation of the float32 leg caught
by that grading, and the host-side surface: refusals before any launch."""
import numpy as np
import pytest
import torch

import _contrast_ref as R
from _contrast_ref import F32, F64


def _quiet(_line):
    pass


# ------------------------------------------------------------------------------------------ float64 leg vs torch autograd
@pytest.mark.parametrize("classes,dim", [(2, 4), (5, 16), (23, 16), (32, 64)])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("reduction", R.REDUCTIONS)
def test_float64_leg_is_the_textbook(classes, dim, form, reduction):
    batch, ppi = 3, 42
    f, labels, target, wpx, wimg, proto, seen = R.make_case(batch, ppi, classes, dim, 17 + classes)
    lab, tg = (labels, None) if form == "hard" else (None, target)
    out = R.contrast(f, lab, tg, proto, seen, R.INV_TAU, wpx, wimg, batch, ppi, reduction, F64)
    why = out["why"]
    assert set(np.unique(why)) == {0, 1, 2, 3}
    shape = lambda a: torch.tensor(a).view(batch, 1, ppi, *a.shape[1:]).movedim(-1, 1) if a.ndim == 2 else torch.tensor(a).view(batch, 1, ppi)  # noqa: E731
    x = shape(f.astype(F64)).requires_grad_()
    t = shape(labels.astype(np.int64)) if form == "hard" else shape(target.astype(F64))
    w, _ = R.pixel_weights(wpx, wimg, batch, ppi)             # the fp32 product, the number the kernel is handed
    loss, dead = R.torch_contrast_loss(x, t, torch.tensor(proto.astype(F32)), seen, float(R.INV_TAU), reduction,
                                       torch.tensor(w).view(batch, 1, ppi), None)
    loss.backward()
    grad = x.grad.movedim(1, -1).reshape(batch * ppi, dim).numpy()
    assert (dead.view(-1).numpy() == (why != 0)).all()
    assert abs(float(out["loss"][0]) - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert np.abs(out["grad"][0] - grad).max() <= 1e-10 * max(1.0, np.abs(grad).max())
    assert not out["grad"][0][why != 0].any() and not out["grad"][1][why != 0].any()      # value 0, magnitude 0: only 0 passes
    assert (out["stats"] == [(why == k).sum() for k in range(4)]).all()
    # the magnitudes are the scale of what they belong to: sum_c |T s_c - t_c| <= 2 T, so a gradient is at most twice its own
    assert abs(float(out["loss"][0])) <= out["loss"][1] * (1 + 1e-12)
    assert (np.abs(out["grad"][0]) <= 2 * out["grad"][1] * (1 + 1e-12)).all()


def test_the_first_cause_decides():
    f, labels, target, wpx, wimg, proto, seen = R.make_case(1, 56, 5, 16, 3)
    r = np.arange(56)
    _, why, _ = R.classify(f, labels, None, wpx, wimg, 1, 56, seen)
    assert why[(r % 14 == 9) & (r // 14 % 2 == 1)].tolist() == [1, 1] and np.isnan(f[23, 0])     # weight 0 and a NaN feature
    assert why[(r % 14 == 3) & (r // 14 % 2 == 1)].tolist() == [2, 2] and np.isnan(f[17, 0])     # label 255 and a NaN feature
    _, why, _ = R.classify(f, None, target, wpx, wimg, 1, 56, seen)
    assert why[(r % 14 == 6) & (r // 14 % 2 == 1)].tolist() == [2, 2] and np.isnan(f[20, 0])     # a target of 1.5 and a NaN feature
    assert why[r % 14 == 8].tolist() == [3] * 4


def test_dead_calls_and_a_weighted_mean_of_nothing():
    f, labels, target, wpx, wimg, proto, seen = R.make_case(3, 30, 5, 16, 3)
    for elem in (F64, F32):
        for kw in (dict(seen=np.zeros(5, dtype=np.int32)), dict(inv_tau=0.0)):
            a = dict(seen=seen, inv_tau=R.INV_TAU)
            a.update(kw)
            for lab, tg in ((labels, None), (None, target)):
                out = R.contrast(f, lab, tg, proto, a["seen"], a["inv_tau"], wpx, wimg, 3, 30, "weighted_mean", elem)
                assert out["loss"][0] == 0 and not out["grad"][0].any() and out["stats"].sum() == 90
        out = R.contrast(f, labels, None, proto, np.zeros(5, dtype=np.int32), R.INV_TAU, wpx, wimg, 3, 30, "mean", elem)
        assert out["stats"][0] == 0 and out["stats"][3] == 0
        z = R.make_case(1, 4, 5, 16, 3, "w_zero")
        out = R.contrast(z[0], z[1], None, z[5], z[6], R.INV_TAU, z[3], z[4], 1, 4, "weighted_mean", elem)
        assert np.isnan(out["loss"][0]) and not out["grad"][0].any() and list(out["stats"]) == [0, 4, 0, 0]


# --------------------------------------------------------------------------------------------------------------- mirrors
@pytest.mark.parametrize("classes,dim", [(2, 4), (5, 16), (23, 16)])
def test_product_mirrors_are_the_float64_leg(classes, dim):
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    batch, ppi = 3, 42
    f, labels, target, wpx, wimg, proto, seen = R.make_case(batch, ppi, classes, dim, 5 + classes)
    s, _ = R.assign(f, proto, seen, R.INV_TAU, F64)
    m = PR.assign_mirror(f, proto, seen, R.INV_TAU)
    assert np.array_equal(np.isnan(m), np.isnan(s)) and np.nanmax(np.abs(m - s)) <= 1e-13
    for reduction in R.REDUCTIONS:
        for lab, tg in ((labels, None), (None, target)):
            out = R.contrast(f, lab, tg, proto, seen, R.INV_TAU, wpx, wimg, batch, ppi, reduction, F64)
            loss, grad, stats, why = PR.contrast_mirror(f, labels if tg is None else tg, proto, seen, R.INV_TAU, wpx, wimg, batch, reduction)
            assert abs(loss - float(out["loss"][0])) <= 1e-12 * max(1.0, abs(loss))
            assert np.abs(grad - out["grad"][0]).max() <= 1e-12 * max(1.0, np.abs(grad).max())
            assert (stats == out["stats"]).all() and (why == out["why"]).all()
    loss, grad, stats, _ = PR.contrast_mirror(f, labels, proto, seen, 0.0, wpx, wimg, batch)
    assert loss == 0.0 and not grad.any() and stats[0] > 0
    loss, grad, stats, _ = PR.contrast_mirror(f, labels, proto, np.zeros(classes), R.INV_TAU, wpx, wimg, batch)
    assert loss == 0.0 and not grad.any() and stats[0] == 0
    for bad in (dict(reduction="none"), dict(batch=4), dict(pixel_weight=wpx[:-1]), dict(image_weight=wimg[:-1])):
        with pytest.raises(ValueError):
            PR.contrast_mirror(f, labels, proto, seen, R.INV_TAU, **{**dict(pixel_weight=wpx, image_weight=wimg, batch=batch), **bad})
    with pytest.raises(ValueError):
        PR.contrast_mirror(f, target[:, :-1], proto, seen, R.INV_TAU)
    with pytest.raises(ValueError):
        PR.assign_mirror(f, proto[:, :-1], seen, R.INV_TAU)


@pytest.mark.parametrize("classes", [2, 5, 23])
def test_assign_mirror_is_rectify_mirror_under_uniform_probabilities(classes):
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    f, _, _, _, _, proto, seen = R.make_case(3, 42, classes, 16, 11)
    uniform = np.full((f.shape[0], classes), 1.0 / classes)
    for sn in (seen, np.zeros(classes, dtype=np.int32)):
        a = PR.assign_mirror(f, proto, sn, R.INV_TAU)
        r = PR.rectify_mirror(f, uniform, proto, sn, R.INV_TAU, probs=True)
        assert np.array_equal(np.isnan(a), np.isnan(r)) and np.isnan(a).any()
        assert np.nanmax(np.abs(a - r)) <= 1e-14
        assert np.allclose(np.nansum(a, 1)[~np.isnan(a).any(1)], 1.0, rtol=0, atol=1e-13)


# --------------------------------------------------------------------------------------------- float32 leg meets the bar
@pytest.mark.parametrize("classes", R.CLASSES)
@pytest.mark.parametrize("dim", R.DIMS)
def test_float32_leg_meets_the_bar(dim, classes):
    for batch, ppi in R.SHAPES:
        seed = 100 * classes + dim + ppi
        R.grade_case(R.LegBackend(), batch, ppi, classes, dim, seed, _quiet).done()
        R.grade_case(R.LegBackend(), batch, ppi, classes, dim, seed + 1, _quiet, ldf=dim + 4, combos=R.COVER, weight_variants=False).done()


@pytest.mark.parametrize("row_kind", R.ROW_KINDS)
def test_float32_leg_meets_the_bar_on_single_rows(row_kind):
    for classes in R.CLASSES:
        R.grade_case(R.LegBackend(), 1, 1, classes, 16, 7 * classes, _quiet, row_kind=row_kind).done()


def test_float32_leg_meets_the_bar_on_dead_calls():
    R.grade_case(R.LegBackend(), 3, 85, 5, 16, 9, _quiet, seen=np.zeros(5, dtype=np.int32)).done()
    R.grade_case(R.LegBackend(), 3, 85, 5, 16, 9, _quiet, inv_tau=0.0).done()


# ------------------------------------------------------------------------------------------------- mutations are caught
@pytest.mark.parametrize("mut,combos", [
    ("f_terms_kept", (("hard", "mean"),)),                    # the rows 1e3 away: the cancellation against f
    ("f_terms_kept", (("soft", "sum"),)),
    ("T_is_1", (("soft", "mean"),)),                          # the mass on the unseen class is dropped: T < 1
    ("unseen_in_sum", (("hard", "mean"),)),
    ("unseen_in_sum", (("soft", "weighted_mean"),)),
    ("grad_not_divided", (("hard", "mean"),)),
    ("grad_not_divided", (("soft", "weighted_mean"),)),
    ("pad_lanes", (("hard", "sum"),)),
    ("void_grad", (("soft", "mean"),)),
    ("void_grad", (("hard", "mean"),)),
])
def test_each_mutation_is_caught(mut, combos):
    assert mut in R.MUTATIONS
    g = R.grade_case(R.LegBackend(mut), 3, 85, 5, 16, 31, _quiet, ldf=20, combos=combos, weight_variants=False)
    assert g.bad, f"the grading let the mutation {mut!r} through"
    with pytest.raises(AssertionError):
        g.done()
    R.grade_case(R.LegBackend(), 3, 85, 5, 16, 31, _quiet, ldf=20, combos=combos, weight_variants=False).done()


def test_every_mutation_has_a_case():
    marks = [m for m in test_each_mutation_is_caught.pytestmark if m.name == "parametrize"]
    assert {row[0] for row in marks[0].args[1]} == set(R.MUTATIONS)


# ------------------------------------------------------------------------------------------------------- host surface
def test_module_and_assign_check_their_arguments():
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    bank = PR.PrototypeBank(5, 16)
    for bad in (dict(bank=object()), dict(bank=bank, reduction="none")):
        with pytest.raises(ValueError):
            PR.PrototypeContrastLoss(**bad)
    loss = PR.PrototypeContrastLoss(bank, reduction="weighted_mean")
    assert loss.REDUCTIONS == ("mean", "sum", "weighted_mean") and "weighted_mean" in repr(loss) and loss.last_stats is None
    f = torch.zeros(2, 16, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(f, torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PR.assign(f, bank)
    with pytest.raises(ValueError, match=r"\[N,16,H,W\]"):
        loss(torch.zeros(2, 8, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        loss(f.double(), torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="bank must be a PrototypeBank"):
        PR.assign(f, None)


def test_entry_points_validate_before_any_launch():
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    P = 4096                                     # a non-NULL, 16-byte aligned "pointer": validation fails before anything is dereferenced
    ok = dict(ldf=16, dim=16, labels=P, target=None, ldt=0, batch=2, ppi=32, classes=5, mean=1, denom=None)

    def contrast(**over):
        a = {**ok, **over}
        return lib.udaseg_proto_contrast_fwd_bwd(a.get("feat", P), a["ldf"], a["dim"], a["labels"], a["target"], a["ldt"], None, None,
                                                 a["batch"], a["ppi"], a["classes"], a.get("proto", P), a.get("seen", P),
                                                 a.get("inv_tau", P), a["mean"], a["denom"], a.get("partials", P), a.get("loss", P),
                                                 a.get("dfeat"), None, None)

    for over in (dict(classes=0), dict(classes=33), dict(dim=0), dict(dim=6, ldf=8), dict(dim=68, ldf=68), dict(ldf=12), dict(ldf=18),
                 dict(batch=0), dict(ppi=0), dict(batch=2, ppi=1 << 30), dict(labels=None), dict(target=P, ldt=8),
                 dict(labels=None, target=P, ldt=4), dict(labels=None, target=P, ldt=6), dict(labels=None, target=P + 4, ldt=8),
                 dict(mean=1, denom=P), dict(feat=None), dict(proto=None), dict(seen=None), dict(inv_tau=None), dict(partials=None),
                 dict(loss=None), dict(feat=P + 4), dict(dfeat=P + 8)):
        assert contrast(**over) == -1, over
        assert lib.udaseg_last_error()
    assert contrast(labels=None) == -1 and b"exactly one" in lib.udaseg_last_error()

    def assign(**over):
        a = {**dict(ldf=16, dim=16, classes=5, ldc=8, pixels=64), **over}
        return lib.udaseg_proto_assign(a.get("feat", P), a["ldf"], a["dim"], a["classes"], a["ldc"], a.get("proto", P), a.get("seen", P),
                                       a.get("inv_tau", P), a["pixels"], a.get("out", P), None)

    for over in (dict(classes=0), dict(classes=33, ldc=36), dict(dim=2), dict(ldf=12), dict(ldc=4), dict(ldc=6), dict(pixels=0),
                 dict(pixels=1 << 31), dict(feat=None), dict(proto=None), dict(seen=None), dict(inv_tau=None), dict(out=None),
                 dict(feat=P + 4), dict(out=P + 8)):
        assert assign(**over) == -1, over
        assert lib.udaseg_last_error()
    assert lib.udaseg_seg_partials() == R.BLOCKS


def test_structure_trainer_refuses_bad_arguments_and_a_gradient_reducer_before_touching_anything():
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    from uda_aerial_semantic_segmentation_research_amd.distill import DistillTrainer
    from uda_aerial_semantic_segmentation_research_amd.structure import StructureTrainer
    assert issubclass(StructureTrainer, DistillTrainer)
    tr = StructureTrainer.__new__(StructureTrainer)
    tr.grad_reducer = object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        tr.distill_step(None, None, None, None)

    class Net(torch.nn.Conv2d):
        classes = 5

        def forward_parts(self, x, want):
            raise AssertionError("not reached")

    net, teacher, cpu = Net(3, 5, 1), Net(3, 5, 1), torch.device("cpu")
    bank = PR.PrototypeBank(5, 16)
    for bad in (dict(bank=None), dict(bank=object()), dict(bank=PR.PrototypeBank(6, 16)), dict(bank=bank, lambda_src=float("nan")),
                dict(bank=bank, lambda_tgt=float("inf")), dict(bank=bank, contrast=torch.nn.MSELoss())):
        with pytest.raises(ValueError):
            StructureTrainer(net, cpu, teacher, **bad)
    plain = torch.nn.Conv2d(3, 5, 1)
    plain.classes = 5
    with pytest.raises(ValueError, match="the model must offer forward_parts"):
        StructureTrainer(plain, cpu, teacher, bank=bank)
    with pytest.raises(TypeError):
        StructureTrainer(net, cpu, teacher)                    # the bank is required
    tr = StructureTrainer(net, cpu, teacher, bank=bank, lambda_tgt=0.1)
    assert tr.lambda_src == 0.0 and tr.lambda_tgt == 0.1 and tr.bank is bank and tr.contrast.bank is bank
