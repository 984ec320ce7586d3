"""GPU checks of the prototype module: exact invariants of the three kernels at edge shapes, the accumulated sums against
float64 under a derived bar, the update bit for bit against its numpy mirror, the rectified probabilities against the float64
mirror, and the labeler end to end.

The sums (``test_accumulate_invariants_and_sums``).  Device and mirror add the same numbers in float64 in some order, and any
two orders differ by at most ``2 (n - 1) 2^-53 sum|x|``; the bar per cell is ``n_c 2^-52 sum|x|`` -- derived, not measured.

The rectified probabilities (``test_rectify_against_float64``).  Yardstick: the torch fp32 composition of the same formula
(softmax, broadcast squared distances, ``exp``, normalisation) on the same device and inputs against the same float64 values.
Bar: ``max(2 * that error, 4 * 2**-23)``, ``tests/test_gpu_pseudo.py``'s rule: both sides evaluate one fp32 formula, the 2 allows
one more ``expf`` and another summation order, 4 ulps of 1 is the floor.  The winner must equal the float64 winner wherever the
float64 top-two gap exceeds twice the bar, and at most 2 % of the pixels may be excluded that way.
Figures of one MI355X run, 20000 pixels per case (profiles/proto_grade.txt), as (C, D, logit scale, tau_scale): torch's error /
the kernel's: (23, 16, 3, 1) 2.55e-7 / 2.62e-7; (32, 16, 3, 1) 2.40e-7 / 2.43e-7; (2, 4, 3, 1) 3.22e-7 / 3.22e-7;
(23, 16, 3, 0.05) 2.38e-6 / 2.32e-6; (23, 16, 0.02, 1) 1.22e-7 / 1.42e-7 (the 4-ulp floor is the bar); (23, 64, 3, 1) 2.00e-7 /
2.63e-7 (the floor again); (5, 8, 40, 1) 3.02e-7 / 2.59e-7; probabilities in, (23, 16, 3, 1): 3.23e-7 / 2.66e-7.  The excluded
share is 0.0000 everywhere (one pixel of 20000 at logit scale 0.02) and the rectified winner differs from the raw one at 2.6 % ..
96 % of the pixels.  The same shares, and torch's error of 2.1e-7 .. 1.7e-6, were computed on the CPU (torch fp32 against float64)
before the first GPU run.
"""
import numpy as np
import pytest
import torch

from _proto_ref import accumulate_mirror, rectify_mirror, sum_bars, update_mirror

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -23
MULTIPLE, FLOOR_ULPS, EXCLUDED_CAP = 2.0, 4.0, 0.02
SHAPES = [(1, 4, 4), (2, 8, 12), (23, 16, 16), (32, 64, 64)]          # classes, dim, ldf
PIXELS = [1, 63, 64 * 1024 + 1]
PATTERNS = ("uniform", "alternating", "runs37", "void", "random")


@pytest.fixture(scope="module")
def PR():
    from uda_aerial_semantic_segmentation_research_amd import _lib, proto
    _lib.require_gpu()
    return proto


def _labels(pattern, pixels, classes, g):
    i = torch.arange(pixels)
    if pattern == "uniform":                                         # every wave carries one class
        lab = torch.full((pixels,), classes - 1)
    elif pattern == "alternating":                                   # every wave is mixed
        lab = i % min(classes, 2) if classes > 1 else i % 2 * 200    # one class: the class against void
    elif pattern == "runs37":                                        # runs that straddle the 64-pixel wave boundaries
        lab = (i // 37) % (classes + 1)                              # the label `classes` is a void run
    elif pattern == "void":
        lab = torch.full((pixels,), 255)
    else:
        lab = torch.randint(0, classes + 3, (pixels,), generator=g)
    return lab.to(torch.uint8)


def _features(pixels, dim, ldf, g):
    """[pixels, ldf] fp32 rows: randn + 2 in the channels that count, a poison value in the padding (it must not be read)."""
    f = torch.full((pixels, ldf), float("nan"))
    f[:, :dim] = torch.randn(pixels, dim, generator=g) + 2.0
    return f


def _accumulators(classes, dim):
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    return z(classes * dim, torch.float64), z(classes, torch.float64), z(classes + 2, torch.int64)


# ------------------------------------------------------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("classes,dim,ldf", SHAPES)
@pytest.mark.parametrize("pixels", PIXELS)
def test_accumulate_invariants_and_sums(PR, pixels, classes, dim, ldf):
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    g = torch.Generator().manual_seed(1000 * classes + pixels % 997)
    feat = _features(pixels, dim, ldf, g)
    planted = sorted({0, pixels // 2, pixels - 1})[: 1 if pixels == 1 else 3]
    for pattern in PATTERNS:
        lab = _labels(pattern, pixels, classes, g)
        for poison in (False, True):
            f = feat.clone()
            if poison:
                for k, p in enumerate(planted):
                    f[p, (k * 3) % dim] = (float("nan"), float("inf"), float("-inf"))[k]
            ref_sums, ref_sq, ref_counts, abs_sums, abs_sq = accumulate_mirror(f[:, :dim].numpy(), lab.numpy(), classes)
            assert int(ref_counts.sum()) == pixels
            if poison:
                assert int(ref_counts[classes + 1]) == len(planted)
            sums, sq, counts = _accumulators(classes, dim)
            fd, ld = f.cuda(), lab.cuda()
            K.proto_accumulate(fd, ldf, dim, ld, pixels, classes, sums, sq, counts)
            got_counts = counts.cpu().numpy()
            what = (pattern, poison)
            assert np.array_equal(got_counts, ref_counts), what      # bincount, the labels beyond the classes, the non-finite pixels
            bar_s, bar_q = sum_bars(ref_counts, abs_sums, abs_sq)
            err_s = np.abs(sums.cpu().numpy().reshape(classes, dim) - ref_sums)
            err_q = np.abs(sq.cpu().numpy() - ref_sq)
            assert (err_s <= bar_s).all(), (what, float((err_s - bar_s).max()))
            assert (err_q <= bar_q).all(), (what, float((err_q - bar_q).max()))
            once = sums.clone()
            K.proto_accumulate(fd, ldf, dim, ld, pixels, classes, sums, sq, counts)
            assert np.array_equal(counts.cpu().numpy(), 2 * ref_counts), what
            err2 = np.abs(sums.cpu().numpy().reshape(classes, dim) - 2.0 * ref_sums)
            assert (err2 <= 4.0 * bar_s).all(), what                 # 2 n numbers of sum 2 sum|x|
            assert torch.isfinite(once).all()


def test_accumulate_through_the_bank_layouts(PR):
    """The NHWC view (zero-copy), an ordinary NCHW tensor (one layout kernel) and bf16 features give the same counts, and sums
    within the bar."""
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    g = torch.Generator().manual_seed(5)
    n, d, h, w, C = 2, 16, 24, 40, 7
    nhwc = (torch.randn(n, h, w, d, generator=g) + 2.0).cuda()
    view = nhwc.permute(0, 3, 1, 2)
    assert padded_nhwc(view)[0].data_ptr() == nhwc.data_ptr()
    lab = torch.randint(0, C + 1, (n, h, w), generator=g, dtype=torch.uint8).cuda()
    ref_sums, ref_sq, ref_counts, abs_sums, abs_sq = accumulate_mirror(nhwc.cpu().reshape(-1, d).numpy(), lab.cpu().reshape(-1).numpy(), C)
    bar_s, _ = sum_bars(ref_counts, abs_sums, abs_sq)
    for feats in (view, view.contiguous()):
        bank = PR.PrototypeBank(C, d)
        assert bank.accumulate(feats, lab) is bank
        assert np.array_equal(bank.counts.cpu().numpy(), ref_counts)
        assert (np.abs(bank.sums.cpu().numpy() - ref_sums) <= bar_s).all()
    half = PR.PrototypeBank(C, d).accumulate(view.bfloat16(), lab)
    assert np.array_equal(half.counts.cpu().numpy(), ref_counts)
    assert np.allclose(half.sums.cpu().numpy(), ref_sums, rtol=2.0 ** -7, atol=2.0 ** -7 * abs_sums.max())
    with pytest.raises(ValueError):
        bank.accumulate(view, lab.long())
    with pytest.raises(ValueError):
        bank.accumulate(view, lab[:, :-1])


# ----------------------------------------------------------------------------------------------------------------- 2. update
def _bank_np(bank):
    return {k: getattr(bank, k).cpu().numpy().copy() for k in ("sums", "sq", "counts", "prototypes", "spread", "seen", "last_counts",
                                                               "inv_tau")}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("classes,dim,ldf", SHAPES)
@pytest.mark.parametrize("tau", ["auto", 3.0])
def test_update_is_bit_for_bit_the_mirror(PR, classes, dim, ldf, tau):
    g = torch.Generator().manual_seed(7 * classes + dim)
    bank = PR.PrototypeBank(classes, dim, momentum=0.9, min_pixels=40, tau=tau, tau_scale=0.7)
    pixels = 4000
    state = None
    for step, clear in enumerate((False, True, True)):               # first sight; EMA on the doubled sums; EMA on a fresh batch
        feats = (torch.randn(1, dim, 1, pixels, generator=g) * (1.0 + step) + 0.5 * step).cuda()
        lab = torch.randint(0, classes + 1, (pixels,), generator=g)
        if classes > 2:
            lab[lab == 1] = 0                                        # class 1 is never seen
            lab[(lab == 2) & (torch.arange(pixels) > 200 * (step + 1))] = 0      # class 2 passes min_pixels late or never
        bank.accumulate(feats, lab.to(torch.uint8).reshape(1, 1, pixels).cuda())
        before = _bank_np(bank)
        bank.update(clear=clear)
        after = _bank_np(bank)
        p, s, sn, last, inv = update_mirror(before["sums"], before["sq"], before["counts"], before["prototypes"], before["spread"],
                                            before["seen"], momentum=0.9, min_pixels=40, tau_scale=0.7 if tau == "auto" else 0.0,
                                            inv_tau=before["inv_tau"][0])
        assert _same_bits(after["prototypes"], p), step
        assert _same_bits(after["spread"], s), step
        assert _same_bits(after["seen"], sn) and _same_bits(after["last_counts"], last), step
        assert _same_bits(after["inv_tau"], np.array([inv], dtype=np.float32)), (step, after["inv_tau"], inv)
        for k in ("sums", "sq", "counts"):
            assert _same_bits(after[k], np.zeros_like(before[k]) if clear else before[k]), (step, k)
        state = after
    if tau == "auto":
        assert state["inv_tau"][0] > 0 and state["seen"].sum() >= 1
    else:
        assert state["inv_tau"][0] == np.float32(1.0 / 3.0)
    if classes > 2:
        assert state["seen"][1] == 0 and not state["prototypes"][1].any()
    rep = bank.report()
    assert rep["seen"] == [bool(v) for v in state["seen"]] and rep["last_counts"] == [int(v) for v in state["last_counts"][:classes]]
    assert len(rep["moved"]) == classes and all(m >= 0 for m in rep["moved"]) and rep["spread"] == state["spread"].tolist()
    assert rep["tau"] == 1.0 / float(state["inv_tau"][0])
    assert bank.reset() is bank and not bank.seen.any() and not bank.prototypes.any()


# ---------------------------------------------------------------------------------------------------------------- 3. rectify
def _rectify_inputs(pixels, classes, dim, g, scale=3.0):
    proto = torch.randn(classes, dim, generator=g, dtype=torch.float64)
    cls = torch.randint(0, classes, (pixels,), generator=g)
    feat = (proto[cls] + torch.randn(pixels, dim, generator=g, dtype=torch.float64)).float()
    logits = scale * torch.randn(pixels, classes, generator=g)
    return proto, feat, logits


def _kernel_rectify(feat, ldf, scores, ldc, classes, probs, proto, seen, inv_tau):
    """The kernel on [pixels, dim] features / [pixels, classes] scores re-laid with row strides ldf / ldc (poison in the padding)."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    pixels, dim = feat.shape
    fb = torch.full((pixels, ldf), float("nan"))
    fb[:, :dim] = feat
    sb = torch.full((pixels, ldc), float("nan"))
    sb[:, :classes] = scores
    out = torch.full((pixels, ldc), -7.0, device="cuda")
    args = (fb.cuda(), ldf, dim, sb.cuda(), ldc, classes, probs, proto.cuda(), torch.as_tensor(seen, dtype=torch.int32).cuda(),
            torch.tensor([inv_tau], dtype=torch.float32).cuda(), pixels)
    K.proto_rectify(*args, out)
    again = torch.empty_like(out)
    K.proto_rectify(*args, again)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))   # no atomics: the same bits, NaN rows included
    return out.cpu()


@pytest.mark.parametrize("classes,dim,ldf", SHAPES)
@pytest.mark.parametrize("pixels", PIXELS)
def test_rectify_invariants(PR, pixels, classes, dim, ldf):
    g = torch.Generator().manual_seed(31 * classes + pixels % 991)
    proto, feat, logits = _rectify_inputs(pixels, classes, dim, g)
    ldc = 4 * ((classes + 3) // 4) + (4 if classes == 2 else 0)      # classes = 2: a row stride beyond the padded width
    inv_tau = float(np.float32(1.0 / dim))
    seen = np.ones(classes, dtype=np.int32)
    if classes > 2:
        seen[[1, classes - 1]] = 0
    out = _kernel_rectify(feat, ldf, logits, ldc, classes, 0, proto, seen, inv_tau)
    assert (out[:, classes:] == 0).all()                             # padding channels
    assert (out[:, :classes][:, seen == 0] == 0).all()               # unseen classes get exactly 0
    rows = out[:, :classes].double()
    assert torch.isfinite(rows).all() and (rows >= 0).all()
    assert float((rows.sum(1) - 1.0).abs().max()) <= 4.0 * ULP1 * classes
    ref = rectify_mirror(feat.numpy(), logits.numpy(), proto.numpy(), seen, inv_tau)
    assert float(np.abs(rows.numpy() - ref).max()) < 1e-4            # the formula (graded in test_rectify_against_float64)
    # the limiting cases: inv_tau == 0 is p renormalised over the seen classes; a huge inv_tau the nearest seen prototype
    flat = _kernel_rectify(feat, ldf, logits, ldc, classes, 0, proto, seen, 0.0)[:, :classes].double()
    p = torch.softmax(logits.double(), 1) * torch.as_tensor(seen)
    assert float((flat - p / p.sum(1, keepdim=True)).abs().max()) <= 8.0 * ULP1
    sharp = _kernel_rectify(feat, ldf, logits, ldc, classes, 0, proto, seen, 1e30)[:, :classes]
    d = ((feat.double()[:, None, :] - proto.float().double()[None]) ** 2).sum(2)
    d[:, seen == 0] = float("inf")
    if int(seen.sum()) > 1:                                          # leave out the pixels whose two nearest prototypes tie in fp32
        top2 = d.topk(2, dim=1, largest=False).values
        clear = top2[:, 1] - top2[:, 0] > 1e-3
    else:
        clear = torch.ones(pixels, dtype=torch.bool)
    assert (sharp.argmax(1)[clear] == d.argmin(1)[clear]).all() and (sharp.max(1).values[clear] == 1.0).all()
    # no class seen: the softmax itself
    none = _kernel_rectify(feat, ldf, logits, ldc, classes, 0, proto, np.zeros(classes), inv_tau)[:, :classes].double()
    assert float((none - torch.softmax(logits.double(), 1)).abs().max()) <= 8.0 * ULP1


def test_rectify_nonfinite_rows_are_void_and_counted(PR):
    from uda_aerial_semantic_segmentation_research_amd import pseudo
    g = torch.Generator().manual_seed(11)
    C, D, n, h, w = 23, 16, 1, 8, 40
    proto, feat, logits = _rectify_inputs(n * h * w, C, D, g)
    bad_f, bad_z = [3, 64, 319], [0, 65, 200, 201]
    feat[bad_f[0], 0], feat[bad_f[1], 15], feat[bad_f[2], 7] = float("nan"), float("inf"), float("-inf")
    logits[bad_z[0], 22], logits[bad_z[1], 0], logits[bad_z[2], 5], logits[bad_z[3], 1] = (float("nan"), float("inf"),
                                                                                           float("-inf"), float("nan"))
    bank = PR.PrototypeBank(C, D, tau=float(D))
    bank._ensure(torch.device("cuda", 0))
    bank.prototypes.copy_(proto)
    bank.seen.fill_(1)
    feats = feat.reshape(n, h, w, D).cuda().permute(0, 3, 1, 2)
    outs = logits.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous().cuda()
    r = PR.rectify(feats, outs, bank)
    assert tuple(r.shape) == (n, C, h, w) and r.stride(1) == 1 and r.stride(3) == 24
    rows = r.permute(0, 2, 3, 1).reshape(-1, C).cpu()
    bad = sorted(bad_f + bad_z)
    good = [i for i in range(n * h * w) if i not in bad]
    assert torch.isnan(rows[bad]).all() and torch.isfinite(rows[good]).all()
    counts = torch.zeros(C + 2, dtype=torch.int64, device="cuda")
    masks = pseudo.pseudo_labels(r, torch.zeros(C, dtype=torch.int32, device="cuda"), probs=True, counts=counts)
    flat = masks.reshape(-1).cpu()
    assert (flat[bad] == 255).all() and (flat[good] < C).all()
    assert int(counts[C + 1]) == len(bad) and int(counts[C]) == len(bad) and int(counts[:C].sum()) == len(good)
    hist = pseudo.ConfidenceHistogram(C).update(r, probs=True)
    assert int(hist.nonfinite) == len(bad) and int(hist.table.sum()) == len(good)
    # probabilities outside [0, 1] and an all-zero row
    probs = torch.softmax(logits.nan_to_num(0.0, 0.0, 0.0), 1)
    probs[10, 3], probs[11, 4], probs[12] = 1.5, -0.25, 0.0
    pr = PR.rectify(feats, probs.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous().cuda(), bank, probs=True)
    prow = pr.permute(0, 2, 3, 1).reshape(-1, C).cpu()
    bad_p = sorted(bad_f + [10, 11, 12])
    assert torch.isnan(prow[bad_p]).all() and torch.isfinite(prow[[i for i in range(n * h * w) if i not in bad_p]]).all()
    with pytest.raises(ValueError):
        PR.rectify(feats, outs[:, :22], bank)
    with pytest.raises(ValueError):
        PR.rectify(feats[:, :12], outs, bank)


# (C, D, logit scale, tau_scale, probs)
GRADE_CASES = [(23, 16, 3.0, 1.0, 0), (32, 16, 3.0, 1.0, 0), (2, 4, 3.0, 1.0, 0), (23, 16, 3.0, 0.05, 0), (23, 16, 0.02, 1.0, 0),
               (23, 64, 3.0, 1.0, 0), (5, 8, 40.0, 1.0, 0), (23, 16, 3.0, 1.0, 1)]
GRADE_PIXELS = 20000


def grade_case(C, D, scale, tau_scale, probs, device="cuda", rectify=None, pixels=GRADE_PIXELS):
    """One grading case -> dict of figures.  ``rectify(feat, scores, proto, inv_tau) -> [P, C]`` is the implementation under
    test (None: only torch's own error, which needs no GPU)."""
    g = torch.Generator().manual_seed(100 * C + D + int(10 * scale))
    proto, feat, logits = _rectify_inputs(pixels, C, D, g, scale)
    scores = torch.softmax(logits, 1) if probs else logits
    inv_tau = float(np.float32(1.0 / (tau_scale * D)))
    ref = rectify_mirror(feat.numpy(), scores.numpy(), proto.numpy(), np.ones(C), inv_tau, probs=bool(probs))
    f, z, p32 = feat.to(device), scores.to(device), proto.float().to(device)
    pt = z if probs else torch.softmax(z, 1)
    d = ((f[:, None, :] - p32[None, :, :]) ** 2).sum(2)
    u = torch.exp(-(d - d.min(1, keepdim=True).values) * inv_tau)
    r = pt * u
    torch_out = (r / r.sum(1, keepdim=True)).cpu().double().numpy()
    torch_err = float(np.abs(torch_out - ref).max())
    bar = max(MULTIPLE * torch_err, FLOOR_ULPS * ULP1)
    top = np.sort(ref, axis=1)
    gap = top[:, -1] - top[:, -2]
    decided = gap > 2.0 * bar
    raw_winner = scores.argmax(1).numpy()
    fig = {"case": (C, D, scale, tau_scale, probs), "torch_err": torch_err, "bar": bar, "excluded": float(1.0 - decided.mean()),
           "moved_winner": float((ref.argmax(1) != raw_winner).mean())}
    if rectify is not None:
        out = rectify(feat, scores, proto, inv_tau).double().numpy()
        fig["kernel_err"] = float(np.abs(out - ref).max())
        fig["winner_ok"] = bool((out.argmax(1)[decided] == ref.argmax(1)[decided]).all())
    return fig


@pytest.mark.parametrize("C,D,scale,tau_scale,probs", GRADE_CASES)
def test_rectify_against_float64(PR, C, D, scale, tau_scale, probs):
    ldc = 4 * ((C + 3) // 4)
    kernel = lambda feat, scores, proto, inv_tau: _kernel_rectify(feat, D, scores, ldc, C, probs, proto, np.ones(C), inv_tau)[:, :C]
    fig = grade_case(C, D, scale, tau_scale, probs, rectify=kernel)
    print("proto_grade", fig)
    assert fig["excluded"] <= EXCLUDED_CAP, fig
    assert fig["moved_winner"] > 0.01, fig                           # returning p would not pass
    assert fig["kernel_err"] <= fig["bar"], fig
    assert fig["winner_ok"], fig


# ------------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def r18():
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(0)
    return Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).to("cuda").train()


def _frames(seed, k=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8) for _ in range(k)]


def test_labeler_before_rectification_is_the_online_labeler(PR, r18):
    from uda_aerial_semantic_segmentation_research_amd import teacher
    batches = _frames(21)
    kw = dict(portion=0.3, cap=0.9, halve_every=2)
    a = teacher.OnlineLabeler(r18, 23, **kw)
    b = PR.PrototypeLabeler(r18, 23, rectify_after=len(batches), bank=PR.PrototypeBank(23, min_pixels=1), **kw)
    for frames in batches:
        ma, mb = a.label(frames.cuda()), b.label(frames.cuda())
        assert torch.equal(ma, mb) and r18.training
    assert torch.equal(a.thr_bins, b.thr_bins) and torch.equal(a.hist.table, b.hist.table)
    assert b.bank.updates == len(batches) and int(b.bank.seen.sum()) >= 1      # the bank fills meanwhile
    assert int(b.bank.last_counts.sum()) == 2 * 64 * 64


def test_labeler_end_to_end(PR, r18):
    from uda_aerial_semantic_segmentation_research_amd import data as D, mix, pseudo
    batches = _frames(22)
    lab = PR.PrototypeLabeler(r18, 23, portion=0.3, cap=0.9, rectify_after=0, bank=PR.PrototypeBank(23, momentum=0.9, min_pixels=8))
    manual_bank = PR.PrototypeBank(23, momentum=0.9, min_pixels=8)
    hist = pseudo.ConfidenceHistogram(23)
    zeros = torch.zeros(23, dtype=torch.int32, device="cuda")
    for frames in batches:
        masks = lab.label(frames.cuda())
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (2, 64, 64) and masks.is_cuda and r18.training
        r18.eval()
        with torch.no_grad():
            out, dec = r18.forward_parts(D.prepare_batch(frames.cuda())[0], ("logits", "decoder"))
        r18.train()
        assert tuple(dec.shape) == (2, 16, 64, 64)
        manual_bank.accumulate(dec, pseudo.pseudo_labels(out, zeros)).update()
        rect = PR.rectify(dec, out, manual_bank)
        hist.update(rect, probs=True)
        thr = hist.thresholds(0.3, 0.0, 0.9)
        assert torch.equal(masks, pseudo.pseudo_labels(rect, thr, probs=True))
        assert torch.equal(thr, lab.thr_bins)
    assert torch.equal(lab.bank.prototypes, manual_bank.prototypes) and torch.equal(lab.bank.seen, manual_bank.seen)
    rep = lab.report()
    assert {"threshold", "support", "kept", "kept_share", "void_share", "nonfinite"} <= set(rep)
    assert {"seen", "last_counts", "spread", "tau", "moved"} <= set(rep)
    assert rep["nonfinite"] == 0 and sum(rep["support"]) == len(batches) * 2 * 64 * 64 and sum(rep["last_counts"]) == 2 * 64 * 64
    # drops into the mean-teacher recipe in place of OnlineLabeler
    g = torch.Generator().manual_seed(5)
    src = [(f, torch.randint(0, 23, (2, 64, 64), generator=g, dtype=torch.uint8)) for f in _frames(23, 2)]
    mixed = mix.MixedLoader(src, lab.loader(batches[:2]), num_classes=23, generator=torch.Generator().manual_seed(6))
    got = [b for b in mixed]
    assert len(got) == 2 and got[0][0].dtype == torch.uint8 and tuple(got[0][1].shape) == (4, 64, 64)   # source + mixed
    # update_bank=False leaves the bank alone
    frozen = PR.PrototypeLabeler(r18, 23, bank=lab.bank, update_bank=False)
    before = lab.bank.prototypes.clone()
    frozen.label(batches[0].cuda())
    assert torch.equal(before, lab.bank.prototypes)


def test_init_from_state_dict_and_domain_gap(PR, r18):
    g = torch.Generator().manual_seed(8)
    frames = _frames(24, 2)
    masks = [torch.randint(0, 4, (2, 64, 64), generator=g, dtype=torch.uint8) for _ in frames]
    masks[0][0, :1, :5] = 7                                          # 5 pixels of class 7: below min_pixels
    masks[1][1, :2, :8] = 9                                          # 16 pixels of class 9: exactly min_pixels
    masks[1][0, 5:9] = 255                                           # void
    lab = PR.PrototypeLabeler(r18, 23, bank=PR.PrototypeBank(23, min_pixels=16))
    assert lab.init_from(list(zip(frames, masks))) is lab and r18.training
    present = torch.bincount(torch.cat(masks).reshape(-1).long(), minlength=256)[:23]
    assert lab.bank.seen.cpu().tolist() == [int(n >= 16) for n in present]
    assert lab.bank.updates == 1 and lab.bank.last_counts[:23].cpu().tolist() == present.tolist()
    assert int(lab.bank.last_counts[23]) == 4 * 64 and int(lab.bank.seen.sum()) == 5
    # unlabelled: the raw winners label the frames
    tgt = PR.PrototypeLabeler(r18, 23, bank=PR.PrototypeBank(23, min_pixels=16))
    tgt.init_from(frames, labelled=False)
    assert int(tgt.bank.last_counts[:23].sum()) == 2 * 2 * 64 * 64 and tgt.bank.updates == 1
    gap = PR.domain_gap(lab.bank, tgt.bank)
    both = (lab.bank.seen != 0) & (tgt.bank.seen != 0)
    assert len(gap) == 23 and [np.isnan(v) for v in gap] == [not bool(b) for b in both.cpu()]
    assert all(v >= 0 for v in gap if not np.isnan(v)) and PR.domain_gap(lab.bank, lab.bank)[0] == 0.0
    with pytest.raises(ValueError):
        lab.init_from([])
    with pytest.raises(ValueError):
        lab.init_from(frames)                                        # labelled=True needs masks
    # state_dict round trip, bit for bit
    state = lab.bank.state_dict()
    assert all(not v.is_cuda for v in state.values() if torch.is_tensor(v))
    fresh = PR.PrototypeBank(23, min_pixels=3, momentum=0.5)
    assert fresh.load_state_dict(state) is fresh and fresh.min_pixels == 16 and fresh.momentum == 0.999 and fresh.updates == 1
    for k in ("prototypes", "spread", "seen", "inv_tau"):
        assert _same_bits(getattr(fresh, k).cpu().numpy(), getattr(lab.bank, k).cpu().numpy()), k
    with pytest.raises(ValueError):
        PR.PrototypeBank(5).load_state_dict(state)
