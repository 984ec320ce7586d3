"""GPU checks of the curves module: the score-histogram kernel against the float64 restatement (tests/_curves_ref.py) edge by
edge, the finishing kernel against the host arithmetic on the kernel's own tables and against sklearn's exact-score AUC
(tests/golden/curves_ref.npz), determinism / accumulation / layouts, the trainer hook and ``evaluate``."""
import os

import numpy as np
import pytest
import torch

import _curves_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DELTA = 1e-4        # 52 fp32 ulp at the top of the range: one subtraction, one exp sum and one log on magnitudes <= 32


@pytest.fixture(scope="module")
def C():
    from uda_aerial_semantic_segmentation_research_amd import _lib, curves
    _lib.require_gpu()
    return curves


def _fixture_input():
    m = np.load(os.path.join(GOLD, "seg_metrics_ref.npz"))
    return m["logits"], m["target"]


def _sharp_input():
    g = np.load(os.path.join(GOLD, "curves_ref.npz"))
    return g["sharp_logits_q"].astype(np.float32) / 256.0, g["sharp_target"].astype(np.int64)


def _seeded_input(n, c, h, w, seed, block=8, invalid=0):
    """Targets constant on block x block squares, logits 1.5 * randn plus 12 * rand on the target's channel (the recipe of the
    fixture's sharper case at another size); ``invalid`` pixels get targets outside [0, c)."""
    g = torch.Generator().manual_seed(seed)
    tb = torch.randint(0, c, (n, h // block, w // block), generator=g)
    target = tb.repeat_interleave(block, 1).repeat_interleave(block, 2).contiguous()
    z = 1.5 * torch.randn(n, c, h, w, generator=g)
    z.scatter_add_(1, target[:, None], 12.0 * torch.rand(n, 1, h, w, generator=g))
    if invalid:
        idx = torch.randperm(target.numel(), generator=g)[:invalid]
        target.view(-1)[idx[::2]] = -1
        target.view(-1)[idx[1::2]] = c + 200
    return z.numpy(), target.numpy()


def _kernel_tables(C, logits, target, **kw):
    z, t = torch.from_numpy(np.ascontiguousarray(logits)).cuda(), torch.from_numpy(np.ascontiguousarray(target)).cuda()
    h = C.ScoreHistogram(z.shape[1], device=z.device, **kw).update(z, t)
    tab = h.tables.cpu().numpy()
    return tab[0], tab[1], h


def _reference(logits, target, bins=R.SCORE_BINS, score_range=R.SCORE_RANGE):
    """Restatement tables plus, per class / kind / edge, the number of restatement scores within DELTA of the edge.  Image by
    image, so that the 8 x 23 x 512 x 512 case stays within a few hundred MB."""
    c = logits.shape[1]
    pos = np.zeros((c, bins), dtype=np.int64)
    neg = np.zeros_like(pos)
    near = np.zeros((2, c, bins), dtype=np.int64)
    for i in range(logits.shape[0]):
        s = R.scores(logits[i:i + 1])
        t = target[i].reshape(-1)
        valid = (t >= 0) & (t < c)
        b = R.bin_index(s, bins, score_range)
        for k in range(c):
            for kind, sel in enumerate((valid & (t == k), valid & (t != k))):
                (pos, neg)[kind][k] += np.bincount(b[sel, k], minlength=bins)
                near[kind, k] += R.near_edge_counts(s[sel, k], DELTA, bins, score_range)
    return pos, neg, near


def _check_tables(name, kpos, kneg, logits, target, check_share=True, **kw):
    rpos, rneg, near = _reference(logits, target, **kw)
    c = logits.shape[1]
    worst = 0
    for kind, (kt, rt) in enumerate(((kpos, rpos), (kneg, rneg))):
        assert np.array_equal(kt.sum(axis=1), rt.sum(axis=1)), (name, "totals P / N differ")
        ck = np.cumsum(kt[:, ::-1], axis=1)[:, ::-1]         # pixels with score >= the bin's lower edge
        cr = np.cumsum(rt[:, ::-1], axis=1)[:, ::-1]
        diff = np.abs(ck - cr)
        worst = max(worst, int(diff.max()))
        bad = np.argwhere(diff > near[kind])
        assert len(bad) == 0, (name, "pos" if kind == 0 else "neg", "class, edge:", bad[:5].tolist(),
                               "diff", diff[tuple(bad[0])], "allowed", near[kind][tuple(bad[0])])
    t = target.reshape(-1)
    nvalid = int(((t >= 0) & (t < c)).sum())
    share = near.sum() / float(nvalid * c)
    print(f"{name}: largest per-edge difference {worst} counts, share of scores within {DELTA} of an edge {100 * share:.2f} %, "
          f"exact-equal tables: {bool(np.array_equal(kpos, rpos) and np.array_equal(kneg, rneg))}")
    assert share < 0.02 or not check_share, (name, share)                        # the allowance cannot swallow a wrong kernel
    assert nvalid * c == int(kpos.sum() + kneg.sum())


@pytest.mark.parametrize("name", ["fixture", "sharp", "c5", "c32", "full"])
def test_tables_edge_by_edge(C, name):
    if name == "fixture":
        logits, target = _fixture_input()
    elif name == "sharp":
        logits, target = _sharp_input()
    elif name == "c5":
        logits, target = _seeded_input(2, 5, 48, 40, seed=5, invalid=60)       # ldc = 8
    elif name == "c32":
        logits, target = _seeded_input(2, 32, 32, 48, seed=32, invalid=40)     # ldc = 32, eight class groups
    else:
        logits, target = _seeded_input(8, 23, 512, 512, seed=2, invalid=1000)  # the headline batch, ldc = 24
    kpos, kneg, _ = _kernel_tables(C, logits, target)
    _check_tables(name, kpos, kneg, logits, target)


@pytest.mark.parametrize("classes,ldc", [(ldc - 1, ldc) for ldc in range(4, 33, 4)] + [(4, 4), (32, 32)])
def test_every_row_width(C, classes, ldc):
    """All eight instantiations of the histogram kernel at kernel level, by the per-edge criterion: junk in the pad lanes, an exact
    tie of the maximum, and a NaN above channel 0, whose pixel has no number for a score and lands in bin 0 of every class."""
    import _scores_ref as S
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    rows = S.sweep_rows(classes, seed=200 + ldc)
    rng = np.random.default_rng(ldc)
    tgt = rng.integers(0, classes, S.PIXELS)
    tgt[[3, 290]] = -1, classes + 5
    tables = torch.zeros(2, classes, R.SCORE_BINS, dtype=torch.int64, device="cuda")
    K.score_hist(torch.from_numpy(S.padded(rows, ldc)).cuda(), torch.from_numpy(tgt).cuda(), S.PIXELS, classes, ldc, R.SCORE_BINS,
                 R.SCORE_RANGE, tables[0], tables[1])
    kpos, kneg = tables.cpu().numpy()
    assert np.isnan(rows[S.NAN_PIXEL]).sum() == 1
    for k in range(classes):                                          # the NaN pixel: bin 0 of every class
        (kpos if k == tgt[S.NAN_PIXEL] else kneg)[k, 0] -= 1
    assert kpos.min() >= 0 and kneg.min() >= 0
    keep = np.arange(S.PIXELS) != S.NAN_PIXEL
    logits = rows[keep].T.reshape(1, classes, 1, -1)
    _check_tables(f"classes={classes} ldc={ldc}", kpos, kneg, logits, tgt[keep].reshape(1, 1, -1))


def test_other_grids(C):
    """Coarser and finer grids (8 classes / 2 classes per block) and a narrower range (both end bins filled), by the same per-edge
    criterion; the 2 % cap on the allowance belongs to the default grid (the share grows with bins / range) and is not asserted."""
    logits, target = _seeded_input(2, 23, 32, 32, seed=9, invalid=30)
    for bins, rng in ((256, 16.0), (4096, 16.0), (1024, 6.0)):
        kpos, kneg, _ = _kernel_tables(C, logits, target, bins=bins, score_range=rng)
        assert kpos.shape == (23, bins)
        _check_tables(f"bins={bins} range={rng}", kpos, kneg, logits, target, check_share=False, bins=bins, score_range=rng)
    assert kneg[:, 0].sum() > 0 and kpos[:, -1].sum() > 0


def test_nan_scores_stay_inside_the_histogram(C):
    z = torch.randn(1, 23, 16, 16)
    z[0, :, 0, 0] = float("nan")
    z[0, 3, 0, 1] = float("inf")
    z[0, :, 0, 2] = float("-inf")
    t = torch.randint(0, 23, (1, 16, 16))
    h = C.ScoreHistogram(23, device="cuda").update(z.cuda(), t.cuda())
    tab = h.tables.cpu().numpy()
    assert tab.min() >= 0 and tab[0].sum() == 256 and tab[1].sum() == 256 * 22
    clean = C.ScoreHistogram(23, device="cuda").update(z[:, :, 1:].cuda(), t[:, 1:].cuda()).tables.cpu().numpy()
    extra = tab - clean                                                   # the 16 pixels of row 0, 13 of them ordinary
    assert extra.min() >= 0 and extra.sum() == 16 * 23


def test_finish_kernel_against_host_arithmetic_and_exact_auc(C):
    g = np.load(os.path.join(GOLD, "curves_ref.npz"))
    for name, (logits, target) in {"fixture": _fixture_input(), "sharp": _sharp_input(),
                                   "c32": _seeded_input(2, 32, 32, 48, seed=32, invalid=40)}.items():
        kpos, kneg, h = _kernel_tables(C, logits, target)
        dev = h.compute()
        assert all(v.is_cuda for v in dev.values()) and dev["auc"].dtype == torch.float64 and dev["support"].dtype == torch.int64
        host = C.curves_from_hist(kpos, kneg)
        assert np.array_equal(dev["support"].cpu().numpy(), host["support"])
        for k in ("auc", "ap", "auc_slack"):
            d = dev[k].cpu().numpy()
            assert np.array_equal(np.isnan(d), np.isnan(host[k])), (name, k)
            m = np.isfinite(d)
            rel = np.abs(d[m] - host[k][m]) / np.maximum(np.abs(host[k][m]), 1e-300)
            print(f"{name} {k}: max relative difference device / host {rel.max():.2e}")
            assert rel.max() <= 1e-12, (name, k, rel.max())
        if name in ("fixture", "sharp"):
            exact = g[f"{name}/auc_exact"]
            m = np.isfinite(exact)
            d, sl = dev["auc"].cpu().numpy(), dev["auc_slack"].cpu().numpy()
            assert np.array_equal(m, np.isfinite(d))
            print(f"{name}: max |auc - exact| {np.abs(d[m] - exact[m]).max():.3e}, max slack {sl[m].max():.3e}")
            assert np.all(np.abs(d[m] - exact[m]) <= sl[m] + 1e-6)
            assert np.all(sl[m] <= 5e-3)


def test_determinism_accumulation_bf16_and_layouts(C):
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    logits, target = _seeded_input(4, 23, 64, 64, seed=3, invalid=50)
    z, t = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda()
    one = C.ScoreHistogram(23, device="cuda").update(z, t)
    again = C.ScoreHistogram(23, device="cuda").update(z, t)
    assert torch.equal(one.tables, again.tables)
    a, b = one.compute(), again.compute()
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in a)      # bit for bit, NaN included
    halves = C.ScoreHistogram(23, device="cuda").update(z[:1], t[:1]).update(z[1:], t[1:])
    assert torch.equal(halves.tables, one.tables)
    assert torch.equal(C.ScoreHistogram(23, device="cuda").update(z, t[:, None]).tables, one.tables)          # [N,1,H,W] masks
    twice = C.ScoreHistogram(23, device="cuda").update(z, t).update(z, t)
    assert torch.equal(twice.tables, 2 * one.tables)
    twice.reset()
    assert int(twice.tables.abs().sum()) == 0
    zb = z.bfloat16()
    assert torch.equal(C.ScoreHistogram(23, device="cuda").update(zb, t).tables,
                       C.ScoreHistogram(23, device="cuda").update(zb.float(), t).tables)
    assert torch.equal(C.ScoreHistogram(23, device="cuda").update(z, t.int()).tables, one.tables)
    cur = C.class_curves(z, t, 23)
    assert np.array_equal(cur["support"], one.compute()["support"].cpu().numpy())
    # logits straight from Unet.forward: the padded NHWC buffer is read in place
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda().eval()
    with torch.no_grad():
        out = net(torch.randn(2, 3, 64, 64, device="cuda"))
    buf, ldc = padded_nhwc(out)
    assert ldc == 24 and buf.data_ptr() == out.data_ptr()
    tt = t[:2]
    assert torch.equal(C.ScoreHistogram(23, device="cuda").update(out, tt).tables,
                       C.ScoreHistogram(23, device="cuda").update(out.contiguous().clone(), tt).tables)


def _loader(n_batches, bs, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(bs, 3, hw, hw, generator=g), torch.randint(0, 23, (bs, hw, hw), generator=g)) for _ in range(n_batches)]


def _trainer(log_curves):
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(11)
    tr = SegmentationTrainer(Unet("resnet18", encoder_weights=None, in_channels=3, classes=23), torch.device("cuda"))
    tr.log_curves = log_curves
    return tr


def _epoch_with_spies(flag, train_dl, val_dl, monkeypatch):
    """One epoch + one validation pass of a fresh, seeded trainer.  Spies: every logits tensor the model returned, the number
    of score-histogram launches, and after every train_step its loss and a copy of the model's whole state."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    tr = _trainer(flag)
    spy = {"logits": [], "hist_calls": 0, "steps": [],
           "initial": {k: v.detach().clone() for k, v in tr.model.state_dict().items()}}
    tr.model.register_forward_hook(lambda m, i, o: spy["logits"].append(o.detach().clone()))
    launch = K.score_hist

    def counted(*a, **k):
        spy["hist_calls"] += 1
        return launch(*a, **k)

    monkeypatch.setattr(K, "score_hist", counted)
    step = tr.train_step

    def spied_step(images, masks, optimizer):
        loss, out = step(images, masks, optimizer)
        spy["steps"].append((loss.item(), {k: v.detach().clone() for k, v in tr.model.state_dict().items()}))
        return loss, out

    tr.train_step = spied_step
    opt = FusedAdam(tr.model.parameters(), lr=1e-3)
    tr.current_epoch = 1
    spy["loss"] = tr.train_epoch(train_dl, opt, 1)
    spy["after_epoch"] = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    spy["val"] = tr.validate(val_dl)
    monkeypatch.setattr(K, "score_hist", launch)
    return tr, spy


def test_trainer_hook(C, monkeypatch):
    """log_curves on: the scalar tags of the reference's schedule with the values of class_curves on the very logits the trainer
    saw.  log_curves off: the trainer does what it did before the flag existed -- the same tag set, no histogram launch, the
    epoch's loss is the mean of its train_step losses and the weights after the epoch are bit for bit the weights its last
    train_step left (nothing but train_step touches them; also with the flag on).

    Why the weights are compared inside one run and not between a flag-off and a flag-on run: the training step itself is not
    bit-reproducible from run to run (fp32 split-K atomics order; tests/test_gpu_suites.py bounds the spread).
    Measured on an MI355X with this model and these loaders, same seeds, flag off both times: after ONE step 12 of the 182 state
    tensors differ (max |dw| 4.5e-6), after two steps 149 (1.6e-3, Adam's lr-sized moves where a tiny gradient changes sign);
    flag off against flag on: 12 (2.0e-5) and 150 (1.66e-3), flag on twice: 12 (1.4e-5) and 149 (1.63e-3).  What IS reproducible
    -- the initial weights and everything the first step logs from them -- is compared between the two runs exactly."""
    train_dl, val_dl = _loader(2, 2, 64, seed=1), _loader(2, 2, 64, seed=2)
    off, soff = _epoch_with_spies(False, train_dl, val_dl, monkeypatch)
    on, son = _epoch_with_spies(True, train_dl, val_dl, monkeypatch)
    parent_tags = ({"train/loss", "train/iou", "train/accuracy", "train/learning_rate", "val/loss", "val/iou", "val/accuracy"}
                   | {f"val/iou_class_{c}" for c in range(23)})
    for tr, spy in ((off, soff), (on, son)):
        assert len(spy["steps"]) == 2 and len(spy["logits"]) == 4
        total, rows = 0.0, []
        for i, (loss, _) in enumerate(spy["steps"]):
            total += loss
            rows.append((i, total / (i + 1)))
        assert spy["loss"] == total / 2 and tr.logger.scalars["train/loss"] == rows
        last = spy["steps"][-1][1]
        for k, v in tr.model.state_dict().items():                       # after the epoch AND after the validation pass
            assert torch.equal(spy["after_epoch"][k], last[k]) and torch.equal(v, last[k]), k
        assert any(not torch.equal(spy["initial"][k], last[k]) for k in last)
        assert parent_tags <= set(tr.logger.scalars)
    assert set(off.logger.scalars) == parent_tags and off.last_curves == {} and soff["hist_calls"] == 0
    assert son["hist_calls"] == 2                                        # batch 0 of the epoch and of the validation pass
    for k in soff["initial"]:
        assert torch.equal(soff["initial"][k], son["initial"][k]), k
    for tag in ("train/loss", "train/iou", "train/accuracy", "train/learning_rate"):
        assert off.logger.scalars[tag][0] == on.logger.scalars[tag][0], tag
    assert soff["steps"][0][0] == son["steps"][0][0]
    d = max(float((soff["after_epoch"][k].float() - son["after_epoch"][k].float()).abs().max()) for k in soff["after_epoch"])
    print(f"flag off against flag on, weights after the epoch: max |dw| {d:.3e} (run-to-run spread of the training step, see docstring); "
          f"epoch loss {soff['loss']!r} / {son['loss']!r}")
    new = set(on.logger.scalars) - parent_tags
    assert len(new) == 2 * (2 * 23 + 2)
    # flag on: values of class_curves on the same logits (Config.LOG_INTERVAL = 10: batch 0 only)
    seen = son["logits"]
    for prefix, logits, masks, step in (("train", seen[0], train_dl[0][1], 0), ("val", seen[2], val_dl[0][1], 1)):
        want = C.class_curves(logits, masks.cuda(), 23)
        got = on.last_curves[prefix]
        assert np.isfinite(want["auc"]).sum() == 23
        for c in range(23):
            assert on.logger.scalars[f"{prefix}/auc_class_{c}"] == [(step, float(want["auc"][c]))]
            assert on.logger.scalars[f"{prefix}/ap_class_{c}"] == [(step, float(want["ap"][c]))]
            assert np.array_equal(got["fpr"][c], want["fpr"][c]) and np.array_equal(got["precision"][c], want["precision"][c])
        assert on.logger.scalars[f"{prefix}/mean_auc"] == [(step, float(want["auc"].mean()))]
        assert on.logger.scalars[f"{prefix}/mean_ap"] == [(step, float(want["ap"].mean()))]


def test_trainer_hook_figures(C):
    """A logger with log_figure (not the NullLogger) gets the reference's three figure tags when matplotlib is there."""
    pytest.importorskip("matplotlib")
    from uda_aerial_semantic_segmentation_research_amd.train import NullLogger

    class FigureLogger:
        def __init__(self):
            self.inner, self.figures = NullLogger(), {}

        def log_scalar(self, tag, value, step):
            self.inner.log_scalar(tag, value, step)

        def log_figure(self, tag, figure, step):
            self.figures[tag] = (figure, step)

    tr = _trainer(True)
    tr.logger = FigureLogger()
    tr.current_epoch = 3
    tr.validate(_loader(1, 2, 64, seed=2))
    assert set(tr.logger.figures) == {"val/roc_curves", "val/pr_curves", "val/confusion_matrix"}
    assert all(step == 3 for _, step in tr.logger.figures.values())
    assert "val/mean_auc" in tr.logger.inner.scalars


def test_evaluate(C):
    from uda_aerial_semantic_segmentation_research_amd.metrics import confusion_matrix
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(4)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda()
    loader = _loader(3, 2, 64, seed=6)
    loader[1][1][0, :4, :4] = 255                                         # targets outside [0, 23)
    net.train()
    res = C.evaluate(net, loader, 23, torch.device("cuda"))
    assert net.training
    net.eval()
    cm = torch.zeros(23, 23, dtype=torch.int64, device="cuda")
    hist = C.ScoreHistogram(23, device="cuda")
    npred = torch.zeros(23, dtype=torch.int64)
    with torch.no_grad():
        for x, y in loader:
            out = net(x.cuda())
            cm += confusion_matrix(out, y.cuda(), 23)
            hist.update(out, y.cuda())
            npred += torch.bincount(out.argmax(1).reshape(-1).cpu(), minlength=23)
    assert np.array_equal(res["confusion"], cm.cpu().numpy()) and res["confusion"].sum() == 3 * 2 * 64 * 64 - 16
    assert np.array_equal(res["pos"], hist.pos.cpu().numpy()) and np.array_equal(res["neg"], hist.neg.cpu().numpy())
    want = hist.curves()
    for k in ("auc", "ap", "auc_slack"):
        assert np.array_equal(res[k], want[k], equal_nan=True)
    dev = hist.compute()
    np.testing.assert_allclose(res["auc"], dev["auc"].cpu().numpy(), rtol=1e-12)
    assert res["mean_auc"] == float(np.nanmean(want["auc"])) and res["mean_ap"] == float(np.nanmean(want["ap"]))
    np.testing.assert_allclose(res["pred_distribution"], npred.numpy() / float(3 * 2 * 64 * 64), rtol=0, atol=1e-15)
    assert abs(res["pred_distribution"].sum() - 1.0) < 1e-12
    c = res["confusion"].astype(np.float64)
    tp = np.diag(c)
    np.testing.assert_allclose(res["iou"], tp / (c.sum(0) + c.sum(1) - tp + 1e-7), rtol=1e-12)
    np.testing.assert_allclose(res["f1"], 2 * tp / (c.sum(0) + c.sum(1) + 1e-7), rtol=1e-12)
    assert res["accuracy"] == tp.sum() / c.sum()
