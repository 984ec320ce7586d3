"""CPU checks of the curves module: the finishing arithmetic (``curves_from_hist``) on the float64 restatement's tables
against sklearn's answers recorded in tests/golden/curves_ref.npz (tools/gen_curves_golden.py), the rigorous AUC bound, the
NaN / out-of-range / accumulation rules, and the error convention of the two new entry points.  No GPU, no sklearn."""
import os

import numpy as np
import pytest

import _curves_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("fixture", "sharp")


def _inputs(name):
    g = np.load(os.path.join(GOLD, "curves_ref.npz"))
    if name == "fixture":
        m = np.load(os.path.join(GOLD, "seg_metrics_ref.npz"))
        return g, m["logits"], m["target"]
    return g, g["sharp_logits_q"].astype(np.float32) / 256.0, g["sharp_target"].astype(np.int64)


def test_sharp_case_recipe_matches_the_stored_input():
    g = np.load(os.path.join(GOLD, "curves_ref.npz"))
    q, t = R.sharp_case()
    assert np.array_equal(q, g["sharp_logits_q"]) and np.array_equal(t, g["sharp_target"].astype(np.int64))
    assert int(g["bins"]) == R.SCORE_BINS and float(g["score_range"]) == R.SCORE_RANGE
    s = R.scores(q.astype(np.float32) / 256.0)
    assert s.min() < -R.SCORE_RANGE and s.max() > R.SCORE_RANGE          # both end bins are exercised


@pytest.mark.parametrize("name", CASES)
def test_auc_ap_and_curve_points_equal_sklearn_on_the_quantised_score(name):
    from uda_aerial_semantic_segmentation_research_amd.curves import SCORE_BINS, SCORE_RANGE, curves_from_hist
    assert (SCORE_BINS, SCORE_RANGE) == (R.SCORE_BINS, R.SCORE_RANGE)
    g, logits, target = _inputs(name)
    pos, neg = R.tables(logits, target)
    cur = curves_from_hist(pos, neg)
    present = np.isfinite(g[f"{name}/auc_bin"])
    assert present.sum() >= 15
    np.testing.assert_allclose(cur["auc"][present], g[f"{name}/auc_bin"][present], rtol=0, atol=1e-12)
    ap_present = np.isfinite(g[f"{name}/ap_bin"])
    np.testing.assert_allclose(cur["ap"][ap_present], g[f"{name}/ap_bin"][ap_present], rtol=0, atol=1e-12)
    roc, ro, pr, po = g[f"{name}/roc"], g[f"{name}/roc_offsets"], g[f"{name}/pr"], g[f"{name}/pr_offsets"]
    npts = 0
    for c in np.nonzero(present)[0]:
        at = {int(b): i + 1 for i, b in enumerate(cur["bins"][c])}       # bin -> index into the K + 1 point arrays
        fpr, tpr, thr = roc[:, ro[c]:ro[c + 1]]
        assert fpr[0] == 0 and tpr[0] == 0 and np.isinf(thr[0])          # sklearn opens with the point above every score too
        for f, t, b in zip(fpr[1:], tpr[1:], thr[1:]):                   # sklearn drops collinear points: compare where it keeps one
            i = at[int(b)]
            assert abs(cur["fpr"][c][i] - f) <= 1e-12 and abs(cur["tpr"][c][i] - t) <= 1e-12, (c, b)
        p, r, th = pr[:, po[c]:po[c + 1]]
        assert len(th) == len(cur["bins"][c])                             # one PR point per distinct (non-empty) bin
        idx = np.array([at[int(b)] for b in th])
        np.testing.assert_allclose(cur["precision"][c][idx], p, rtol=0, atol=1e-12)
        np.testing.assert_allclose(cur["recall"][c][idx], r, rtol=0, atol=1e-12)
        npts += len(th) + len(thr) - 1
        P, N = cur["support"][c]
        assert np.array_equal(cur["tp"][c], np.round(cur["tpr"][c][1:] * P).astype(np.int64)) and cur["tp"][c][-1] == P
        assert cur["fp"][c][-1] == N and cur["recall"][c][0] == 0 and cur["precision"][c][0] == 1
        thr_p = cur["thresholds"][c]
        assert np.all(np.diff(thr_p) < 0) and np.all((thr_p > 0) & (thr_p < 1))
    assert npts > 1000


@pytest.mark.parametrize("name", CASES)
def test_auc_of_the_exact_score_lies_within_the_slack(name):
    from uda_aerial_semantic_segmentation_research_amd.curves import curves_from_hist
    g, logits, target = _inputs(name)
    cur = curves_from_hist(*R.tables(logits, target))
    exact = g[f"{name}/auc_exact"]
    both = (cur["support"][:, 0] > 0) & (cur["support"][:, 1] > 0)
    assert np.array_equal(both, np.isfinite(exact)) and both.sum() >= 15
    diff = np.abs(cur["auc"][both] - exact[both])
    print(f"{name}: max |auc - auc_exact| {diff.max():.3e}, max slack {cur['auc_slack'][both].max():.3e}")
    assert np.all(diff <= cur["auc_slack"][both] + 1e-12)
    assert np.all(cur["auc_slack"][both] <= 5e-3)                       # the bound is not vacuous


def test_empty_classes_out_of_range_targets_and_accumulation():
    from uda_aerial_semantic_segmentation_research_amd.curves import curves_from_hist
    g, logits, target = _inputs("fixture")
    pos, neg = R.tables(logits, target)
    cur = curves_from_hist(pos, neg)
    valid = (target >= 0) & (target < 23)
    assert (~valid).sum() > 0                                            # the fixture has targets of -1 and 255
    occurs = np.array([(target == c).any() for c in range(23)])
    assert 0 < occurs.sum() < 23
    assert np.array_equal(cur["support"][:, 0], np.array([(target == c).sum() for c in range(23)]))
    assert np.all(cur["support"].sum(axis=1) == valid.sum())             # every valid pixel once per class, the others nowhere
    assert np.all(np.isnan(cur["auc"][~occurs])) and np.all(np.isnan(cur["ap"][~occurs]))
    assert np.all(np.isnan(cur["auc_slack"][~occurs])) and np.all(np.isfinite(cur["auc"][occurs]))
    for c in np.nonzero(~occurs)[0]:
        assert np.all(np.isnan(cur["tpr"][c])) and np.all(np.isfinite(cur["fpr"][c]))
    # a class that every valid pixel belongs to: no negatives -> auc NaN, ap = 1
    one = curves_from_hist(pos[3:4] + neg[3:4], np.zeros_like(pos[3:4]))
    assert np.isnan(one["auc"][0]) and one["ap"][0] == 1.0
    # two halves accumulate to the whole
    pa, na = R.tables(logits[:1], target[:1])
    pb, nb = R.tables(logits[1:], target[1:])
    assert np.array_equal(pa + pb, pos) and np.array_equal(na + nb, neg)
    two = curves_from_hist(pa + pb, na + nb)
    assert np.array_equal(two["auc"], cur["auc"], equal_nan=True) and np.array_equal(two["ap"], cur["ap"], equal_nan=True)
    with pytest.raises(ValueError):
        curves_from_hist(pos, neg[:, :100])


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    P = 4096                                                              # a non-NULL address; nothing is launched
    good = dict(logits=P, target=P, pixels=100, classes=23, ldc=24, bins=2048, score_range=16.0, pos=P, neg=P)

    def hist(**kw):
        a = {**good, **kw}
        return lib.udaseg_score_hist(a["logits"], a["target"], a["pixels"], a["classes"], a["ldc"], a["bins"], a["score_range"],
                                     a["pos"], a["neg"], None)

    for bad in (dict(logits=None), dict(target=None), dict(pos=None), dict(neg=None), dict(classes=33, ldc=36), dict(classes=0),
                dict(ldc=23), dict(classes=23, ldc=20), dict(bins=2000), dict(bins=0), dict(bins=8192), dict(score_range=0.0),
                dict(score_range=-1.0), dict(score_range=float("nan")), dict(pixels=0)):
        assert hist(**bad) == -1, bad
        assert lib.udaseg_last_error()
    assert b"bins" in (hist(bins=100), lib.udaseg_last_error())[1]
    fin = lambda pos=P, neg=P, classes=23, bins=2048, auc=P, ap=P, slack=P, support=P: lib.udaseg_curve_finish(
        pos, neg, classes, bins, auc, ap, slack, support, None)
    for bad in (dict(pos=None), dict(neg=None), dict(auc=None), dict(ap=None), dict(slack=None), dict(support=None),
                dict(classes=33), dict(classes=0), dict(bins=1000)):
        assert fin(**bad) == -1, bad


def test_operand_table_guards_the_new_entry_points():
    import torch
    from uda_aerial_semantic_segmentation_research_amd import _operands as O
    req = {nm: (dt, cnt) for nm, dt, cnt, _ in O.requirements("udaseg_score_hist", None, None, 100, 23, 24, 2048, 16.0, None, None, 0)}
    assert req == {"logits": (torch.float32, 2400), "target": (torch.int64, 100), "pos": (torch.int64, 23 * 2048),
                   "neg": (torch.int64, 23 * 2048)}
    req = {nm: (dt, cnt) for nm, dt, cnt, _ in O.requirements("udaseg_curve_finish", None, None, 23, 2048, None, None, None, None, 0)}
    assert req["support"] == (torch.int64, 46) and req["auc"] == (torch.float64, 23) and req["pos"] == (torch.int64, 23 * 2048)


def test_cpu_tensors_raise():
    import torch
    from uda_aerial_semantic_segmentation_research_amd.curves import ScoreHistogram, class_curves
    z, t = torch.zeros(1, 23, 8, 8), torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ScoreHistogram(23).update(z, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        class_curves(z, t, 23)
    with pytest.raises(ValueError):
        ScoreHistogram(23, bins=1000)
    with pytest.raises(ValueError):
        ScoreHistogram(33)
