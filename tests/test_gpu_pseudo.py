"""GPU checks of the pseudo-label module: exact invariants of the three kernels at edge shapes, the confidence map, bins and
labels against float64, special values, layouts, the labeler end to end and on a large frame.

The float64 grading (``test_against_float64``).  Yardstick: the error of ``torch.softmax(z, 1).amax(1)`` in fp32 on the same
device against the same float64 values.  Bar: ``max(2 * that error, 4 * 2**-23)``.  Why 2: both sides evaluate one formula in
fp32 -- a 1-ulp ``exp`` per class, a sum of C terms, one division -- and torch's error on the device turned out to be that of a
single chain of C additions (it equals a sequential fp32 replay on the CPU to three digits: 5.1e-7 at C = 23, 5.4e-7 at C = 32),
while the kernel folds the sum as four chains of C / 4 terms and so has no reason to be worse than torch; the factor 2 allows for
another ``exp`` and for rounding luck, and 4 ulps of 1 is the floor for the cases where torch is nearly exact (p ~ 1 / C, C = 2).
Figures of one MI355X run, 20000 pixels per case (torch's error / the kernel's / pixels within the bar of a bin edge at B = 4096
with this bar): scaled C=23 5.1e-7 / 2.7e-7 / 0.9 %; scaled C=32 5.4e-7 / 3.1e-7 / 0.9 %; scaled C=2 8.9e-8 / 8.9e-8 / 0.4 %;
low temperature 2.6e-7 / 1.8e-7 / 0.15 % (66 % of the pixels in the top bin, 42 % at p == 1); high temperature 1.4e-8 / 7.4e-9 /
0.3 %; planted ties 1.4e-7 / 1.0e-7 / 0.07 %.  At B = 256 the excluded share is below 0.1 % everywhere.  The same shares were
computed on the CPU (torch fp32 against float64) before the first GPU run: all inside the 2 % cap.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -23
MULTIPLE, FLOOR_ULPS, EXCLUDED_CAP = 2.0, 4.0, 0.02


@pytest.fixture(scope="module")
def P():
    from uda_aerial_semantic_segmentation_research_amd import _lib, pseudo
    _lib.require_gpu()
    return pseudo


def _logits(kind, classes, pixels, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "scaled":
        z = 3.0 * torch.randn(pixels, classes, generator=g)
    elif kind == "low_t":                                            # near one-hot: p == 1 and the top bin
        z = 40.0 * torch.randn(pixels, classes, generator=g)
    elif kind == "high_t":                                           # p ~ 1 / C
        z = 0.02 * torch.randn(pixels, classes, generator=g)
    elif kind == "ties":                                             # half-integers in [-2, 2]: exact ties of the maximum abound
        z = torch.randint(-4, 5, (pixels, classes), generator=g).float() * 0.5
    else:
        raise KeyError(kind)
    return z


def _nchw(rows, h=1):
    """[pixels, C] rows -> [1, C, h, pixels / h] tensor on the device (an ordinary NCHW tensor: the layout-kernel route)."""
    pixels, c = rows.shape
    return rows.t().reshape(1, c, h, pixels // h).contiguous().cuda()


def _bins_of(p, bins):
    return np.minimum(np.floor(np.asarray(p, dtype=np.float64) * bins), bins - 1).astype(np.int64)


# --------------------------------------------------------------------------------------------------------- 1. exact invariants
INVARIANT_CASES = [
    # classes, pixels, bins, probs
    (1, 1, 256, False),
    (2, 63, 1024, True),
    (5, 513, 4096, False),            # 4096 bins, one class group
    (23, 64 * 1024 + 1, 1024, False),  # the workload's table (92 KiB of LDS), more than one block, a scalar tail
    (23, 64 * 1024 + 1, 2048, True),   # two class groups
    (32, 64 * 1024 + 1, 4096, False),  # four class groups
    (32, 513, 256, True),
    (23, 63, 4096, False),            # three class groups, fewer pixels than one wave chunk
    (5, 1, 1024, True),
]


@pytest.mark.parametrize("classes, pixels, bins, probs", INVARIANT_CASES)
def test_exact_invariants(P, classes, pixels, bins, probs):
    z = _logits("scaled", classes, pixels, seed=100 + classes + pixels % 97 + bins)
    x = _nchw(z)
    if probs:
        x = torch.softmax(x, dim=1)
    am = x.argmax(dim=1).reshape(-1)
    h = P.ConfidenceHistogram(classes, bins).update(x, probs=probs)
    table = h.table.clone()
    assert int(h.nonfinite) == 0
    assert torch.equal(table.sum(1), torch.bincount(am, minlength=classes))
    portion = np.linspace(0.1, 1.0, classes) if classes > 1 else 0.3
    thr = h.thresholds(portion, floor=0.05, cap=0.9)
    host_thr, host_sup = P.thresholds_from_hist(table, portion, floor=0.05, cap=0.9)
    assert thr.dtype == torch.int32 and np.array_equal(thr.cpu().numpy(), host_thr)
    assert np.array_equal(h.support.cpu().numpy(), host_sup)
    thr_open = h.thresholds(0.3, floor=0.0, cap=1.0)                 # neither floor nor cap: the plain quantile bins
    assert np.array_equal(thr_open.cpu().numpy(), P.thresholds_from_hist(table, 0.3)[0])
    for t in (thr, thr_open):
        counts = torch.zeros(classes + 2, dtype=torch.int64, device="cuda")
        labels, conf = P.pseudo_labels(x, t, void=255, probs=probs, return_confidence=True, counts=counts, bins=bins)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (1, 1, pixels)
        tail = torch.stack([table[c, int(t[c]):].sum() for c in range(classes)])
        assert torch.equal(counts[:classes], tail)
        assert int(counts[:classes + 1].sum()) == pixels and int(counts[classes + 1]) == 0
        lab = labels.reshape(-1).long()
        kept = lab != 255
        assert torch.equal(lab[kept], am[kept])
        assert torch.equal(torch.bincount(lab[kept], minlength=classes), counts[:classes])
        # the labelling is the histogram's definition applied to the confidence map
        b = torch.clamp(torch.floor(conf.reshape(-1).double() * bins), max=bins - 1).long()
        assert torch.equal(kept, b >= t.long()[am])
        flat = torch.bincount(am * bins + b, minlength=classes * bins).view(classes, bins)
        assert torch.equal(flat, table)
        again = P.pseudo_labels(x, t, void=255, probs=probs, bins=bins)
        assert torch.equal(again, labels)                            # bit-identical across calls
    h2 = P.ConfidenceHistogram(classes, bins).update(x, probs=probs)
    assert torch.equal(h2.table, table)
    h2.update(x, probs=probs)
    assert torch.equal(h2.table, 2 * table)                          # accumulates
    h2.reset()
    assert int(h2.table.sum()) == 0 and int(h2.nonfinite) == 0


def test_void_label_and_unaligned_label_buffer(P):
    """Another void value, and the kernel's byte-store route: a labels buffer that starts one byte into an allocation."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    classes, pixels, bins = 5, 1030, 256
    x = _nchw(_logits("scaled", classes, pixels, seed=5))
    thr = P.ConfidenceHistogram(classes, bins).update(x).thresholds(0.5, cap=1.0)
    ref = P.pseudo_labels(x, thr, void=5, bins=bins).reshape(-1)
    assert int(ref.max()) <= 5 and int((ref == 5).sum()) > 0
    buf, ldc = padded_nhwc(x)
    raw = torch.full((pixels + 9,), 77, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(classes + 2, dtype=torch.int64, device="cuda")
    K.pseudo_labels(buf, pixels, classes, ldc, 0, bins, thr, 5, raw[1:pixels + 1], None, counts)
    assert torch.equal(raw[1:pixels + 1], ref)
    assert int(raw[0]) == 77 and bool((raw[pixels + 1:] == 77).all())


def _sweep_classes():
    import _scores_ref as S
    return S.SWEEP_CLASSES


@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("classes", _sweep_classes())
def test_every_row_width(P, classes, probs):
    """All eight instantiations of conf_hist and pseudo_labels (ceil(classes / 4) = 1 ... 8, both ends of each) at kernel level on
    300 pixels with junk in the pad lanes, an exact tie of the maximum and a NaN above channel 0 (that pixel is non-finite: void,
    in no cell, counted on its own).  Winner, labels, counts and table exactly; the confidence by test_against_float64's bar."""
    import _scores_ref as S
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    bins, pixels, ldc = 1024, S.PIXELS, (classes + 3) // 4 * 4
    rows = S.sweep_rows(classes, seed=300 + classes, nan=False)
    if probs:
        rows = torch.softmax(torch.from_numpy(rows), dim=1).numpy()          # equal logits give equal probabilities: the tie stays
    if classes >= 2:
        lo, hi = S.tie_channels(classes)
        assert rows[S.TIE_PIXEL, lo] == rows[S.TIE_PIXEL, hi] == rows[S.TIE_PIXEL].max()
        rows[S.NAN_PIXEL, classes - 1] = np.nan
    am = S.first_max(rows)
    finite = ~np.isnan(rows).any(axis=1)
    nbad = int((~finite).sum())
    assert nbad == (1 if classes >= 2 else 0)
    r64 = rows[finite].astype(np.float64)
    if probs:
        p64, bar = r64.max(axis=1), 0.0                                      # the stored value itself
    else:
        p64 = 1.0 / np.exp(r64 - r64.max(axis=1, keepdims=True)).sum(axis=1)
        x = torch.from_numpy(rows[finite]).cuda()
        torch_err = float(np.abs(torch.softmax(x, 1).amax(1).double().cpu().numpy() - p64).max())
        bar = max(MULTIPLE * torch_err, FLOOR_ULPS * ULP1)
    buf = torch.from_numpy(S.padded(rows, ldc)).cuda()
    table = torch.zeros(classes, bins, dtype=torch.int64, device="cuda")
    nonfinite = torch.zeros(1, dtype=torch.int64, device="cuda")
    K.conf_hist(buf, pixels, classes, ldc, probs, bins, table, nonfinite)
    thr0 = torch.zeros(classes, dtype=torch.int32, device="cuda")
    labels = torch.full((pixels,), 77, dtype=torch.uint8, device="cuda")
    conf = torch.full((pixels,), float("nan"), device="cuda")
    counts = torch.zeros(classes + 2, dtype=torch.int64, device="cuda")
    K.pseudo_labels(buf, pixels, classes, ldc, probs, bins, thr0, 255, labels, conf, counts)
    lab, cf = labels.cpu().numpy().astype(np.int64), conf.cpu().numpy().astype(np.float64)
    assert np.array_equal(lab, np.where(finite, am, 255))                    # the winner, tie included; the NaN pixel void
    assert (cf[~finite] == 0.0).all() and float(np.abs(cf[finite] - p64).max()) <= bar
    b = _bins_of(cf[finite], bins)
    assert np.array_equal(table.cpu().numpy(), np.bincount(am[finite] * bins + b, minlength=classes * bins).reshape(classes, bins))
    assert int(nonfinite) == nbad
    want_counts = np.concatenate([np.bincount(am[finite], minlength=classes), [nbad, nbad]])
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    # thresholds that cut: every class keeps the pixels whose bin reaches its threshold
    thr = torch.full((classes,), bins // 2, dtype=torch.int32, device="cuda")
    counts.zero_()
    K.pseudo_labels(buf, pixels, classes, ldc, probs, bins, thr, 255, labels, None, counts)
    kept = finite.copy()
    kept[finite] = b >= bins // 2
    assert np.array_equal(labels.cpu().numpy().astype(np.int64), np.where(kept, am, 255))
    assert int(counts[classes]) == pixels - int(kept.sum()) and int(counts[classes + 1]) == nbad


# --------------------------------------------------------------------------------------------------------- 2. against float64
F64_CASES = [("scaled", 23, 1), ("low_t", 23, 2), ("high_t", 23, 3), ("ties", 5, 4), ("scaled", 32, 5), ("scaled", 2, 6)]


@pytest.mark.parametrize("bins", [4096, 256])
@pytest.mark.parametrize("kind, classes, seed", F64_CASES)
def test_against_float64(P, kind, classes, seed, bins):
    pixels = 20000
    z = _logits(kind, classes, pixels, seed)
    z64 = z.double().numpy()
    am64 = z64.argmax(axis=1)                                        # first maximum; the comparison is of the stored fp32 values
    p64 = 1.0 / np.exp(z64 - z64.max(axis=1, keepdims=True)).sum(axis=1)
    b64 = _bins_of(p64, bins)
    x = _nchw(z, h=100)
    torch_err = float(np.abs(torch.softmax(x, 1).amax(1).reshape(-1).double().cpu().numpy() - p64).max())
    bar = max(MULTIPLE * torch_err, FLOOR_ULPS * ULP1)
    h = P.ConfidenceHistogram(classes, bins).update(x)
    thr = h.thresholds(0.4, floor=0.0, cap=1.0)
    labels, conf = P.pseudo_labels(x, thr, return_confidence=True, bins=bins)
    all_kept = P.pseudo_labels(x, torch.zeros(classes, dtype=torch.int32, device="cuda"), bins=bins)
    conf = conf.reshape(-1).double().cpu().numpy()
    err = float(np.abs(conf - p64).max())
    scaled = p64 * bins
    edge = np.round(scaled)
    near = (np.abs(scaled - edge) <= bar * bins) & (edge >= 1) & (edge <= bins - 1)
    share = float(near.mean())
    print(f"pseudo f64 {kind} C={classes} B={bins}: torch_err {torch_err:.3g} kernel_err {err:.3g} bar {bar:.3g} "
          f"excluded {share:.4%} top-bin share {float((b64 == bins - 1).mean()):.3f}")
    assert np.array_equal(all_kept.reshape(-1).cpu().numpy(), am64)  # argmax: exact, ties included, no exclusion
    assert err <= bar, (err, bar, torch_err)
    assert share <= EXCLUDED_CAP, share                              # a condition of the test, not a measurement
    ok = ~near
    assert np.array_equal(_bins_of(conf, bins)[ok], b64[ok])
    thr_h = thr.cpu().numpy().astype(np.int64)
    lab64 = np.where(b64 >= thr_h[am64], am64, 255)
    assert np.array_equal(labels.reshape(-1).cpu().numpy().astype(np.int64)[ok], lab64[ok])
    table = h.table.cpu().numpy()
    t64 = np.bincount(am64 * bins + b64, minlength=classes * bins).reshape(classes, bins)
    assert np.abs(table - t64).sum() <= 2 * int(near.sum())          # only the excluded pixels may sit in a neighbouring cell
    if kind == "low_t":
        assert float((conf == 1.0).mean()) > 0.3 and table[:, bins - 1].sum() >= (conf == 1.0).sum()
    if kind == "ties":
        top = np.sort(z64, axis=1)
        assert float((top[:, -1] == top[:, -2]).mean()) > 0.1        # the planted ties are there


# --------------------------------------------------------------------------------------------------------- 3. special values
def test_special_values(P):
    inf, nan = float("inf"), float("nan")
    classes, bins = 5, 1024
    rows = [[1e4, -1e4, 0.0, 0.0, 0.0],          # p = 1: top bin, class 0
            [-1e4, -1e4, -1e4, -1e4, -1e4],      # all equal: p = 0.2, class 0
            [0.5, -inf, -inf, 1.0, -inf],        # -inf on non-maximal classes: finite, class 3
            [0.0, -1e4, 1e4, 0.0, -1e4],         # class 2
            [0.0, nan, 0.0, 0.0, 0.0],           # non-finite from here on
            [nan, 0.0, 0.0, 0.0, 0.0],
            [0.0, inf, 0.0, 0.0, 0.0],
            [-inf, -inf, -inf, -inf, -inf]]
    g = torch.Generator().manual_seed(0)
    z = torch.cat([torch.tensor(rows, dtype=torch.float32), 2.0 * torch.randn(70 - len(rows), classes, generator=g)])
    x = _nchw(z)
    h = P.ConfidenceHistogram(classes, bins).update(x)
    assert int(h.nonfinite) == 4 and int(h.table.sum()) == 66
    t = h.table.cpu().numpy()
    assert t[0, bins - 1] >= 1 and t[0, int(0.2 * bins)] + t[0, int(0.2 * bins) - 1] >= 1
    p3 = 1.0 / (1.0 + np.exp(-0.5))
    assert t[3, int(p3 * bins)] >= 1 and t[2, bins - 1] >= 1
    thr0 = torch.zeros(classes, dtype=torch.int32, device="cuda")
    counts = torch.zeros(classes + 2, dtype=torch.int64, device="cuda")
    labels, conf = P.pseudo_labels(x, thr0, return_confidence=True, counts=counts, bins=bins)
    lab, conf = labels.reshape(-1).cpu().numpy(), conf.reshape(-1).cpu().numpy()
    assert list(lab[:8]) == [0, 0, 3, 2, 255, 255, 255, 255]
    assert conf[0] == 1.0 and abs(conf[1] - 0.2) < 1e-6 and abs(conf[2] - p3) < 1e-6 and conf[3] == 1.0
    assert list(conf[4:8]) == [0.0] * 4 and np.isfinite(conf).all()
    assert int(counts[classes + 1]) == 4 and int(counts[classes]) == 4 and int(counts[:classes].sum()) == 66
    # probabilities: a value above 1, a NaN in front, a NaN behind the maximum, a negative maximum
    q = torch.softmax(2.0 * torch.randn(70, classes, generator=g), dim=1)
    q[0] = torch.tensor([0.2, 0.5, 0.3, 0.0, 0.0])
    q[1] = torch.tensor([0.1, 1.5, 0.0, 0.0, 0.0])
    q[2] = torch.tensor([nan, 0.5, 0.1, 0.0, 0.0])
    q[3] = torch.tensor([0.2, 0.5, nan, 0.0, 0.0])
    q[4] = torch.tensor([-0.1, -0.2, -0.3, -0.4, -0.5])
    q[5] = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0])
    xq = _nchw(q)
    hq = P.ConfidenceHistogram(classes, bins).update(xq, probs=True)
    assert int(hq.nonfinite) == 4 and int(hq.table.sum()) == 66
    tq = hq.table.cpu().numpy()
    assert tq[1, bins // 2] >= 1 and tq[4, bins - 1] >= 1
    counts.zero_()
    lq, cq = P.pseudo_labels(xq, thr0, probs=True, return_confidence=True, counts=counts, bins=bins)
    lq, cq = lq.reshape(-1).cpu().numpy(), cq.reshape(-1).cpu().numpy()
    assert list(lq[:6]) == [1, 255, 255, 255, 255, 4] and list(cq[:6]) == [0.5, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert int(counts[classes + 1]) == 4 and int(counts[classes]) == 4 and int(counts[:classes].sum()) == 66


# --------------------------------------------------------------------------------------------------------- 4. layouts
@pytest.fixture(scope="module")
def r18():
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(0)
    return Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).to("cuda").eval()


def test_layouts(P, r18):
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        out = r18(torch.randn(2, 3, 64, 64, generator=g).cuda())
    buf, ldc = padded_nhwc(out)
    assert ldc == 24 and buf.data_ptr() == out.data_ptr()            # the zero-copy route
    copy = out.contiguous()
    assert copy.data_ptr() != out.data_ptr() and copy.stride(3) == 1
    a = P.ConfidenceHistogram(23).update(out)
    b = P.ConfidenceHistogram(23).update(copy)
    assert torch.equal(a.table, b.table) and int(a.table.sum()) == 2 * 64 * 64
    thr = a.thresholds(0.3)
    assert torch.equal(P.pseudo_labels(out, thr), P.pseudo_labels(copy, thr))
    for bad in (out[0], out.reshape(2, 23, -1), out[:, :22]):
        with pytest.raises(ValueError):
            a.update(bad)
    with pytest.raises(ValueError):
        P.pseudo_labels(out[0], thr)
    with pytest.raises(ValueError):
        P.pseudo_labels(out.reshape(2, 23, -1), thr)


# --------------------------------------------------------------------------------------------------------- 5. end to end
def test_labeler_end_to_end(P):
    from uda_aerial_semantic_segmentation_research_amd import data as D
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=5).to("cuda").train()
    batches = [torch.randint(0, 256, (4, 64, 64, 3), generator=g, dtype=torch.uint8) for _ in range(2)]
    portion, cap = 0.25, 0.9
    lab = P.PseudoLabeler(net, 5, portion=portion, floor=0.0, cap=cap)
    assert lab.fit(batches) is lab and net.training                  # the training flag is restored
    assert lab.thr_bins.dtype == torch.int32 and lab.thr_bins.is_cuda
    frames = batches[0]
    masks = lab.label(frames)
    assert net.training and masks.dtype == torch.uint8 and tuple(masks.shape) == (4, 64, 64) and masks.is_cuda
    net.eval()
    with torch.no_grad():
        out = net(D.prepare_batch(frames)[0])
    assert torch.equal(masks, P.pseudo_labels(out, lab.thr_bins))
    net.train()
    rep = lab.report()
    assert {"threshold", "support", "kept", "kept_share", "void_share", "nonfinite"} <= set(rep)
    assert rep["nonfinite"] == 0 and sum(rep["support"]) == 2 * 4 * 64 * 64 and 0.0 < rep["void_share"] < 1.0
    k_cap = P.bin_of(cap, lab.bins)
    for c in range(5):
        assert len(rep["threshold"]) == 5 and rep["threshold"][c] == int(lab.thr_bins[c]) / lab.bins
        if rep["support"][c] and 0 < int(lab.thr_bins[c]) < k_cap:   # neither floor nor cap binding
            assert rep["kept_share"][c] >= portion
        assert rep["kept"][c] <= rep["support"][c]
    pl = lab.loader(batches)
    assert len(pl) == 2
    f0, m0 = next(iter(pl))
    assert f0.dtype == torch.uint8 and f0.is_cuda and torch.equal(m0, masks)
    crit = CrossEntropyLoss(ignore_index=255)
    tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=crit)
    loss = tr.train_epoch(D.DeviceAugmentedLoader(pl, generator=torch.Generator().manual_seed(9)),
                          FusedAdam(net.parameters(), lr=1e-4), 1)
    n_valid, n_void, n_invalid = crit.last_target_stats.tolist()
    assert np.isfinite(loss) and n_void > 0 and n_invalid == 0 and n_valid + n_void == 4 * 64 * 64


# --------------------------------------------------------------------------------------------------------- 6. large frame
def test_label_large(P, r18):
    from uda_aerial_semantic_segmentation_research_amd.predict import predict_large
    g = torch.Generator().manual_seed(6)
    frame = torch.randint(0, 256, (96, 80, 3), generator=g, dtype=torch.uint8)
    lab = P.PseudoLabeler(r18, 23, portion=0.3, cap=1.0)
    lab.fit_large([frame], tile=64, overlap=0.25)
    assert not r18.training
    labels, probs = lab.label_large(frame, tile=64, overlap=0.25)
    ref = predict_large(r18, frame, tile=64, overlap=0.25)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (96, 80) and tuple(probs.shape) == (1, 23, 96, 80)
    kept = labels != 255
    assert int(kept.sum()) > 0 and torch.equal(labels[kept].long(), ref[kept])
    h = P.ConfidenceHistogram(23, lab.bins).update(probs, probs=True)
    tail = torch.stack([h.table[c, int(lab.thr_bins[c]):].sum() for c in range(23)])
    assert torch.equal(torch.bincount(labels[kept].long(), minlength=23), tail) and int(lab.hist.nonfinite) == 0
    assert torch.equal(h.table, lab.hist.table)                      # fit_large saw the same probabilities
    assert lab.report()["kept"] == [int(v) for v in tail]


def test_counters_accumulate_and_no_nonfinite_pixel_adds_nothing(P):
    """The void / non-finite pair of pseudo_labels and conf_hist's non-finite count at 1030 pixels (more than one block, a ragged last
    wave), into buffers that hold 13 already.  No pixel is non-finite, so those words keep their 13 (no atomic is issued); the kept
    and void counts are the bincount of the labels ``test_void_label_and_unaligned_label_buffer`` holds against the module."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    classes, pixels, bins = 5, 1030, 256
    x = _nchw(_logits("scaled", classes, pixels, seed=5))
    thr = P.ConfidenceHistogram(classes, bins).update(x).thresholds(0.5, cap=1.0)
    ref = P.pseudo_labels(x, thr, void=5, bins=bins).reshape(-1)
    want = torch.bincount(ref.long(), minlength=classes + 1).tolist() + [0]      # kept per class, void, non-finite
    assert want[classes] > 0
    buf, ldc = padded_nhwc(x)
    labels = torch.empty(pixels, dtype=torch.uint8, device="cuda")
    counts = torch.full((classes + 2,), 13, dtype=torch.int64, device="cuda")
    for calls in (1, 2):
        K.pseudo_labels(buf, pixels, classes, ldc, 0, bins, thr, 5, labels, None, counts)
        assert torch.equal(labels, ref) and counts.tolist() == [13 + calls * v for v in want]
    table = torch.zeros(classes, bins, dtype=torch.int64, device="cuda")
    nonfinite = torch.full((1,), 13, dtype=torch.int64, device="cuda")
    K.conf_hist(buf, pixels, classes, ldc, 0, bins, table, nonfinite)
    assert int(nonfinite) == 13 and int(table.sum()) == pixels
