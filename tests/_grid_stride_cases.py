"""The cases of tests/test_gpu_grid_stride.py -- every capped-grid pixel kernel of tests/_launch_shapes.py at the smallest size
whose second grid-stride trip exists -- with their inputs, references and comparators, and for each case a first-trip-only
MUTANT of its reference: what a kernel that never came round its loop again would have left (an element-wise output at its
pre-fill beyond trip one, a histogram, count or sum made of trip one's pixels only).  tests/test_launch_shapes_host.py runs
every comparator on its mutant and expects a refusal, so none of them can sample or mask its way past the tail.

By convention a flat size is ``trip + 259``: on the second trip block 0 is full and block 1 holds three threads.  Nothing here
needs a GPU; the comparators take host arrays."""
import numpy as np
import torch

import _launch_shapes as L
import _scores_ref as S

GUARD = 256                                   # sentinel elements on either side of every output buffer the tests allocate
TAIL = 259


class Guarded:
    """``numel`` elements of ``dtype`` pre-filled with ``fill`` between two runs of GUARD sentinel elements."""

    def __init__(self, numel, dtype, fill, device="cuda", sentinel=-77, offset=0):
        self.sentinel, self.numel, self.lo = sentinel, numel, GUARD + offset
        self.raw = torch.full((numel + 2 * GUARD + offset,), sentinel, dtype=dtype, device=device)
        self.body = self.raw[self.lo:self.lo + numel]
        self.body.fill_(fill)

    def intact(self):
        return bool((self.raw[:self.lo] == self.sentinel).all()) and bool((self.raw[self.lo + self.numel:] == self.sentinel).all())


def bf16_round(a):
    """fp32 numpy -> the same values rounded once to bf16 (round to nearest even), as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def per_image_first_trip(launch, n, hw):
    """bool [n, hw]: the pixels of every image that trip one of a per-image launch covers."""
    return np.broadcast_to(L.first_trip(launch, hw), (n, hw))


# ------------------------------------------------------------------------------------------------------------ prepare_batch
PREPARE_FILL = 7.0
PREPARE_CASES = {                              # n, h, w, the D4 codes of each call (sample i of a call takes codes[i])
    "2x513x512": (2, 513, 512, ((0, 2), (4, 6))),
    "8x513x513": (8, 513, 513, (tuple(range(8)),)),
}
_D4 = {}


def d4_combo(code):
    """(rot90_k, flip, transpose) of oracle.data_ref.geometric that data.compose_d4 maps to ``code``."""
    if not _D4:
        from uda_aerial_semantic_segmentation_research_amd.data import compose_d4
        for k in range(4):
            for flip in (None, 0, 1, -1):
                for tr in (False, True):
                    _D4.setdefault(int(compose_d4(k, flip, tr)), (k, flip, tr))
    return _D4[code]


def prepare_inputs(name):
    n, h, w, _ = PREPARE_CASES[name]
    rng = np.random.default_rng(40 + n)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 23, (n, h, w), dtype=np.uint8)


def prepare_reference(imgs, masks, codes):
    """oracle.data_ref.to_model_input per sample -> (fp32 [n, h', w', 3], int64 [n, h', w'])."""
    from oracle.data_ref import to_model_input
    xs, ms = zip(*(to_model_input(imgs[i], masks[i], *d4_combo(c)) for i, c in enumerate(codes)))
    return np.stack(xs).transpose(0, 2, 3, 1), np.stack(ms)


def check_prepare(out, out_m, want_x, want_m, bf16):
    """out: the whole padded buffer [n, h, w, cpad] as fp32.  Bit-exact; bf16 is the fp32 result rounded once; pad lanes zero."""
    assert np.array_equal(out[..., :3], bf16_round(want_x) if bf16 else want_x)
    assert (out[..., 3:] == 0).all()
    assert np.array_equal(out_m, want_m)


def prepare_mutants(want_x, want_m, cpad, bf16):
    n, h, w, _ = want_x.shape
    first = per_image_first_trip(L.prepare_batch(h, w), n, h * w).reshape(n, h, w)
    full = np.zeros((n, h, w, cpad), dtype=np.float32)
    full[..., :3] = bf16_round(want_x) if bf16 else want_x
    yield "image", np.where(first[..., None], full, np.float32(PREPARE_FILL)), want_m
    yield "mask", full, np.where(first, want_m, -7)


# -------------------------------------------------------------------------------------------- the two augmentation pipelines
AUG_N, AUG_H, AUG_W = 2, 520, 512              # both sides multiples of 8 (CLAHE), 266 240 pixels: 4096 on the second trip
AUG_FRAMES = "random"
STRONG_LABELS = ("d4", "affine", "chain", "hsv")
STRONG_TWO_VIEWS = (("chain", "hsv"), ("affine", "d4"))
TRAIN_LABELS = ("grid", "affine+elastic", "chain", "mask_only_d4")
CLAHE_CASES = (("strong", "clahe"), ("strong", "chain"), ("train", "clahe"), ("train", "chain"))
AUG_MUTANT_FILL = 0.0                          # a plausible normalised value: no finiteness check may be what refuses it
_STRONG = {}


def strong_reference(D, label):
    """test_gpu_finetune's frames and records at the case's size with both evaluations of the restatement: made once, shared."""
    import _strong_aug_ref as R
    from test_gpu_finetune import frames, records
    if label not in _STRONG:
        imgs = frames(AUG_FRAMES, AUG_N, AUG_H, AUG_W)
        (_, P), = records(D, AUG_N, AUG_H, AUG_W, (label,))
        img64, ill = R.run(imgs, P, np.float64)
        img32, _ = R.run(imgs, P, np.float32)
        ref = dict(imgs=imgs, P=P, img64=img64, img32=img32, ill=ill)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _STRONG[label] = ref
    return _STRONG[label]


def check_strong(got, ref, label):
    """test_gpu_finetune.py's bar: per sample |kernel - f64| <= max(4 |f32 - f64|, 2 ulp), the hue-ill pixels of the HSV and
    full-chain cases left out (at most ILL_CAP of the batch).  got: fp32 [n, h, w, 3].  -> (err, dev, bar) of the worst sample, share"""
    from test_gpu_finetune import ILL_CAP, MASKED
    from test_gpu_train_aug import check_images
    ill = ref["ill"]
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref["img64"].shape and np.isfinite(got).all()
    keep = ~ill if label in MASKED else np.ones_like(ill)
    worst, failures = check_images(got, ref, keep, f"strong {label}")
    assert not failures, failures
    if label == "d4":
        assert np.array_equal(got.astype(np.float32), ref["img32"])
    return worst, float(ill.mean()) if label in MASKED else 0.0


def aug_first_trip():
    return per_image_first_trip(L.aug_output(AUG_H, AUG_W), AUG_N, AUG_H * AUG_W).reshape(AUG_N, AUG_H, AUG_W)


def image_mutant(img32):
    return np.where(aug_first_trip()[..., None], img32, np.float32(AUG_MUTANT_FILL))


def train_reference(D, label):
    from test_gpu_train_aug import reference
    return reference(D, label, AUG_FRAMES, AUG_H, AUG_W, AUG_N)


def check_train(got, got_m, ref, label):
    """test_gpu_train_aug.py's check_images / check_masks with its caps.  -> worst (err, dev, bar), ill share, band share"""
    from test_gpu_train_aug import ILL_CAP, check_images, check_masks
    ill = ref["ill"]
    masked = label == "chain"
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref["img64"].shape and np.isfinite(got).all()
    keep = ~ill if masked else np.ones_like(ill)
    tag = f"train {label}"
    worst, failures = check_images(got, ref, keep, tag)
    share = check_masks(got_m, ref, tag)
    assert not failures, failures
    if label == "mask_only_d4":
        assert np.array_equal(got.astype(np.float32), ref["img32"]) and np.array_equal(got_m, ref["m64"])
    return worst, float(ill.mean()) if masked else 0.0, float(share)


def clahe_reference(D, pipe, label):
    from test_gpu_clahe import reference
    return reference(D, pipe, label, AUG_H, AUG_W, AUG_N)


def check_clahe(got, lut, ref, pipe, label):
    """test_gpu_clahe.py's bar: the device table against the float64 one (check_tables), then the output against both evaluations
    of the restatement WITH the device's table, the pixels next to a bin boundary and the hue-ill ones left out under their caps.
    -> worst (err, dev, bar), left share, ill share, (tiles with a left-out pixel, their worst table distance)"""
    from test_gpu_clahe import ILL_CAP, LEFT_CAP, _run, check_tables
    from test_gpu_train_aug import check_images
    left, ill = ref["left"], ref["ill"]
    assert left.mean() <= LEFT_CAP, f"share next to a bin boundary {left.mean():.5f} above the cap: change the input"
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    tag = f"clahe {pipe} {label}"
    tables = check_tables(lut, ref, AUG_H, AUG_W, tag)
    d64, d32 = _run(pipe, ref["imgs"], ref["P"], np.float64, lut), _run(pipe, ref["imgs"], ref["P"], np.float32, lut)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == d64["img"].shape and np.isfinite(got).all()
    worst, failures = check_images(got, dict(img64=d64["img"], img32=d32["img"]), ~left & ~ill, tag)
    assert not failures, failures
    return worst, float(left.mean()), float(ill.mean()), tables


def clahe_leg32(ref, pipe):
    """(fp32 image, table) of the restatement's own float32 evaluation: what the mutant is made from."""
    from test_gpu_clahe import _run
    lut = np.array(ref["lut64"])
    return _run(pipe, ref["imgs"], ref["P"], np.float32, lut)["img"], lut


# ------------------------------------------------------------------------------------------------------------ predict gather
GATHER_FILL = 7.0
GATHER_CASES = {                               # frame h, w, plan_grid arguments, D4 codes
    "clamped_260x260": (260, 260, dict(tile=512), tuple(range(8))),        # the tile clamps to 288 x 288: reflect padding, two trips
    "default_600x520": (600, 520, dict(), (0, 5)),                         # 2 x 2 full 512 x 512 tiles: four trips each
}


def gather_frame(h, w):
    return np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gather_reference(P, name):
    """test_gpu_predict._tile_oracle for every (tile, code) -> frame, grid, codes, fp32 [tiles * V, th, tw, 3]"""
    from test_gpu_predict import _tile_oracle
    h, w, kw, codes = GATHER_CASES[name]
    img = gather_frame(h, w)
    g = P.plan_grid(h, w, **kw)
    want = np.stack([_tile_oracle(P, img, g, k, c) for k in range(g.rows * g.cols) for c in codes])
    return img, g, codes, want


def check_gather(out, want, bf16):
    """out: the whole buffer [tiles * V, th, tw, cpad] as fp32.  Bit-exact, pad lanes zero."""
    assert np.array_equal(out[..., :3], bf16_round(want) if bf16 else want)
    assert (out[..., 3:] == 0).all()


def gather_mutant(want, cpad, bf16):
    b, th, tw, _ = want.shape
    first = per_image_first_trip(L.predict_gather(th, tw), b, th * tw).reshape(b, th, tw)
    full = np.zeros((b, th, tw, cpad), dtype=np.float32)
    full[..., :3] = bf16_round(want) if bf16 else want
    return np.where(first[..., None], full, np.float32(GATHER_FILL))


# ---------------------------------------------------------------------------------------------- the default tile, end to end
E2E_FRAME = (600, 520)
E2E_PROB_TOL, E2E_MARGIN = 2e-6, 1e-5         # test_gpu_predict.py's blend bar and label margin
E2E_MIN_KEPT = 0.68                           # the share test_end_to_end_against_cpu_oracle measured for a random-init model


def check_predict_large(probs, labels, want):
    """probs [h, w, C], labels [h, w] against the float64 blend of the oracle tiles' logits.  -> (worst error, share of pixels kept)"""
    from test_gpu_predict import _margin_ok
    err = float(np.abs(np.asarray(probs, dtype=np.float64) - want).max())
    assert err < E2E_PROB_TOL, err
    ok = _margin_ok(want, E2E_MARGIN)
    assert ok.mean() >= E2E_MIN_KEPT, ok.mean()
    assert np.array_equal(labels[ok], want.argmax(-1)[ok])
    return err, float(ok.mean())


def predict_large_mutants(P, want):
    """The frame's pixels that no tile's first gather trip reaches keep the accumulator's zeros / the labels' pre-fill."""
    h, w = E2E_FRAME
    g = P.plan_grid(h, w)
    rows = L.predict_gather(g.th, g.tw).per_trip // g.tw         # whole tile rows in trip one
    seen = np.zeros((h, w), dtype=bool)
    for k in range(g.rows * g.cols):
        oy, ox = g.oy[k // g.cols], g.ox[k % g.cols]
        seen[oy:oy + rows, ox:ox + g.tw] = True
    assert not seen.all()
    yield "probs", np.where(seen[..., None], want, 0.0), want.argmax(-1)
    yield "labels", want, np.where(seen, want.argmax(-1), -7)


# ------------------------------------------------------------------------------------------------------------ predict finish
FINISH_PIXELS, FINISH_CLASSES, FINISH_LDC = 8192 * 256 + TAIL, 3, 4
FINISH_PROB_TOL, FINISH_MARGIN, FINISH_EXCLUDED_CAP = 2e-6, 1e-5, 0.01
_FINISH = {}


def finish_case():
    """acc [P, ldc] fp32 (uniform(0.1, 1) rows, junk in the pad lane), wsum [P] fp32 uniform(0.5, 1.5), and the float64 quotient
    with its first maximum and the pixels whose top-two margin decides the label."""
    if not _FINISH:
        rng = np.random.default_rng(81)
        rows = rng.uniform(0.1, 1.0, (FINISH_PIXELS, FINISH_CLASSES)).astype(np.float32)
        ws = rng.uniform(0.5, 1.5, FINISH_PIXELS).astype(np.float32)
        q = rows.astype(np.float64) / ws.astype(np.float64)[:, None]
        top = np.sort(q, axis=1)
        ref = dict(acc=S.padded(rows, FINISH_LDC), rows=rows, ws=ws, q=q, am=S.first_max(q), decided=top[:, -1] - top[:, -2] > FINISH_MARGIN,
                   am_rows=S.first_max(rows))
        for v in ref.values():
            v.setflags(write=False)
        _FINISH.update(ref)
    return _FINISH


def check_finish(probs, labels, ref):
    """probs [P, ldc] after the call, labels [P].  -> (worst error, excluded share)"""
    assert (probs[:, FINISH_CLASSES:] == 0).all()
    err = float(np.abs(probs[:, :FINISH_CLASSES].astype(np.float64) - ref["q"]).max())
    assert err < FINISH_PROB_TOL, err
    ok = ref["decided"]
    excluded = 1.0 - float(ok.mean())
    assert excluded < FINISH_EXCLUDED_CAP, excluded
    assert np.array_equal(labels[ok], ref["am"][ok])
    return err, excluded


def check_finish_labels_only(buf, labels, ref):
    """Without a weight sum: the first maximum of the rows as they are, the buffer untouched."""
    assert np.array_equal(labels, ref["am_rows"])
    assert np.array_equal(buf, ref["acc"])


def finish_mutants(ref):
    first = L.first_trip(L.predict_finish(FINISH_PIXELS), FINISH_PIXELS)
    done = np.zeros_like(ref["acc"])
    done[:, :FINISH_CLASSES] = (ref["q"]).astype(np.float32)
    yield "probs", np.where(first[:, None], done, ref["acc"]), ref["am"]          # divided in place: beyond trip one still the sums
    yield "labels", done, np.where(first, ref["am"], -7)


def finish_labels_only_mutant(ref):
    first = L.first_trip(L.predict_finish(FINISH_PIXELS), FINISH_PIXELS)
    return np.where(first, ref["am_rows"], -7)


# --------------------------------------------------------------------------------------------------------- predict threshold
THRESHOLD_N, THRESHOLD_HW, THRESHOLD_CLASSES, THRESHOLD_LDC = 2, 262144 + TAIL, 3, 4


def threshold_case():
    """logits [n, hw, ldc] (junk pad lane, every logit at least 1e-6 from the sigmoid's 0.5) and (sigmoid(z) > 0.5) [n, C, hw]."""
    rng = np.random.default_rng(82)
    z = (3.0 * rng.standard_normal((THRESHOLD_N, THRESHOLD_HW, THRESHOLD_CLASSES))).astype(np.float32)
    z[np.abs(z) < 1e-6] = np.float32(1e-3)
    zt = torch.from_numpy(z).permute(0, 2, 1)
    assert bool((zt.abs() >= 1e-6).all())
    want = (torch.sigmoid(zt) > 0.5).float().numpy()
    return np.stack([S.padded(zi, THRESHOLD_LDC) for zi in z]), want


def check_threshold(out, want):
    assert np.array_equal(out, want)


def threshold_mutant(want):
    first = per_image_first_trip(L.predict_threshold(THRESHOLD_HW), THRESHOLD_N, THRESHOLD_HW)
    return np.where(first[:, None, :], want, np.float32("nan"))


# ---------------------------------------------------------------------------------------------------------- argmax confusion
CONFUSION_PIXELS, CONFUSION_CLASSES, CONFUSION_LDC = 262144 + TAIL, 23, 24


def confusion_case():
    """rows [P, C] with exact ties of the maximum on the second trip (its full block and its three-thread block), targets with
    -1, ``classes`` and 255 on both trips, and the reference: first_max, np.bincount over the valid targets."""
    C, P = CONFUSION_CLASSES, CONFUSION_PIXELS
    rng = np.random.default_rng(83)
    rows = (3.0 * rng.standard_normal((P, C))).astype(np.float32)
    ties = [262144 + 5, 262144 + 255, P - 1]
    for p in ties:
        lo, hi = S.tie_channels(C)
        rows[p, lo] = rows[p, hi] = rows[p].max() + np.float32(1.0)
    tgt = rng.integers(0, C, P).astype(np.int64)
    for k, p in enumerate((3, 70000, 262143, 262144, 262144 + 100, P - 2)):
        tgt[p] = (-1, C, 255)[k % 3]
    am = S.first_max(rows)
    assert all(am[p] == S.tie_channels(C)[0] for p in ties)
    valid = (tgt >= 0) & (tgt < C)
    cm = np.bincount(tgt[valid] * C + am[valid], minlength=C * C)
    return S.padded(rows, CONFUSION_LDC), tgt, am, cm


def check_confusion(cm, pred, want_cm, want_pred, calls=1):
    assert np.array_equal(pred, want_pred)
    assert np.array_equal(cm, calls * want_cm)


def confusion_mutants(tgt, am, cm):
    C = CONFUSION_CLASSES
    first = L.first_trip(L.argmax_confusion(CONFUSION_PIXELS), CONFUSION_PIXELS)
    valid = (tgt >= 0) & (tgt < C) & first
    yield "matrix", np.bincount(tgt[valid] * C + am[valid], minlength=C * C), am
    yield "pred", cm, np.where(first, am, -7)


# --------------------------------------------------------------------------------------------------- conf_hist / pseudo_labels
ULP1 = 2.0 ** -23
PSEUDO_CASES = {                               # classes, bins, pixels
    "one_group": (23, 1024, 262144 + 1025),
    "two_groups": (23, 2048, 131072 + 1025),
    "three_groups": (23, 4096, 87040 + 1025),
    "labels_second_trip": (2, 256, 2097152 + TAIL),
}
PSEUDO_VOID = 255
_PSEUDO = {}


def bins_of(p, bins):
    return np.minimum(np.floor(np.asarray(p, dtype=np.float64) * bins), bins - 1).astype(np.int64)


def pseudo_case(name, probs):
    """rows [P, C] fp32 (3 randn logits, or their float64 softmax rounded to fp32) with NaN pixels planted on the second trip of
    both kernels where it exists, and the float64 statement of pixel_conf: first maximum, confidence, finiteness."""
    key = (name, bool(probs))
    if key not in _PSEUDO:
        C, bins, P = PSEUDO_CASES[name]
        rng = np.random.default_rng(90 + C + bins)
        z = 3.0 * rng.standard_normal((P, C))
        if probs:
            e = np.exp(z - z.max(1, keepdims=True))
            rows = np.minimum((e / e.sum(1, keepdims=True)).astype(np.float32), np.float32(1))
        else:
            rows = z.astype(np.float32)
        trip = L.conf_hist(P, C, bins).per_trip
        planted = sorted({trip + 3, trip + 1024, P - 2, L.pseudo_labels(P).per_trip + 7 if L.pseudo_labels(P).trips > 1 else trip + 600})
        for k, p in enumerate(planted):
            rows[p, k % C] = np.nan
        finite = ~np.isnan(rows).any(axis=1)
        r64 = np.nan_to_num(rows.astype(np.float64))
        am = S.first_max(r64)
        if probs:
            p64 = r64.max(axis=1)                                       # the stored value itself: exact
        else:
            p64 = 1.0 / np.exp(r64 - r64.max(axis=1, keepdims=True)).sum(axis=1)
        ref = dict(rows=rows, am=am, p64=p64, finite=finite)
        for v in ref.values():
            v.setflags(write=False)
        ref.update(classes=C, bins=bins, pixels=P, probs=bool(probs), nbad=int((~finite).sum()), planted=planted)
        _PSEUDO[key] = ref
    return _PSEUDO[key]


def pseudo_bar(ref, torch_conf):
    """test_gpu_pseudo.py's bar of the confidence: max(2 x the error of torch's fp32 softmax(z).amax on the same values, 4 ulp of 1);
    in probs mode the confidence is a stored value, the bar 0."""
    if ref["probs"]:
        return 0.0
    f = ref["finite"]
    torch_err = float(np.abs(np.asarray(torch_conf, dtype=np.float64)[f] - ref["p64"][f]).max())
    return max(2.0 * torch_err, 4.0 * ULP1)


def torch_confidence(ref, device="cpu"):
    return torch.softmax(torch.from_numpy(np.array(ref["rows"])).to(device), 1).amax(1).cpu().numpy()


def check_conf_hist(table, nonfinite, ref, bar, calls=1):
    """table [C, B], nonfinite (int) against the float64 statement: the non-finite count, every row sum (np.bincount of the first
    maximum), and cell by cell -- exactly in probs mode, and in logits mode with only the pixels whose float64 confidence lies
    within ``bar`` of a bin edge allowed in a neighbouring cell.  -> share of such pixels"""
    C, B, f = ref["classes"], ref["bins"], ref["finite"]
    assert int(nonfinite) == calls * ref["nbad"], (int(nonfinite), ref["nbad"])
    am, p64 = ref["am"][f], ref["p64"][f]
    assert np.array_equal(table.sum(1), calls * np.bincount(am, minlength=C))
    t64 = np.bincount(am * B + bins_of(p64, B), minlength=C * B).reshape(C, B)
    scaled = p64 * B
    edge = np.round(scaled)
    near = (np.abs(scaled - edge) <= bar * B) & (edge >= 1) & (edge <= B - 1)
    assert np.abs(table - calls * t64).sum() <= 2 * calls * int(near.sum())
    return float(near.mean())


def check_pseudo_labels(labels, conf, counts, table, thr, ref, bar):
    """labels [P] uint8, conf [P] fp32, counts [C + 2] of ONE call with the threshold bins ``thr``, and the table conf_hist made
    of the same scores: the confidence against float64, the labels as the table's definition applied to the confidence map,
    the table itself as the histogram of that map, the counts as np.bincount of the labels and as the table's tails."""
    C, B, f, am = ref["classes"], ref["bins"], ref["finite"], ref["am"]
    conf = np.asarray(conf, dtype=np.float64)
    assert (conf[~f] == 0.0).all()
    err = float(np.abs(conf[f] - ref["p64"][f]).max())
    assert err <= bar, (err, bar)
    b = bins_of(conf, B)
    kept = f & (b >= np.asarray(thr, dtype=np.int64)[am])
    lab = np.asarray(labels).astype(np.int64)
    assert np.array_equal(lab, np.where(kept, am, PSEUDO_VOID))
    assert np.array_equal(np.bincount(am[f] * B + b[f], minlength=C * B).reshape(C, B), table)
    want = np.concatenate([np.bincount(am[kept], minlength=C), [ref["pixels"] - int(kept.sum()), ref["nbad"]]])
    assert np.array_equal(counts, want)
    assert np.array_equal(counts[:C], [table[c, int(thr[c]):].sum() for c in range(C)])
    return err


def pseudo_leg(ref, thr, first=None):
    """(table, nonfinite, labels, conf, counts) of the float64 statement, of the pixels in ``first`` only when given: labels and
    conf keep their pre-fill (77 / NaN) elsewhere.  With ``first=None`` this is a perfect kernel; the mutants pass trip one."""
    C, B, P, f, am = ref["classes"], ref["bins"], ref["pixels"], ref["finite"], ref["am"]
    take = np.ones(P, dtype=bool) if first is None else first
    conf = np.where(f, ref["p64"], 0.0).astype(np.float32)
    b = bins_of(conf, B)
    table = np.bincount(am[f & take] * B + b[f & take], minlength=C * B).reshape(C, B)
    kept = f & (b >= np.asarray(thr, dtype=np.int64)[am])
    labels = np.where(take, np.where(kept, am, PSEUDO_VOID), 77).astype(np.uint8)
    counts = np.concatenate([np.bincount(am[kept & take], minlength=C), [int((~kept & take).sum()), int((~f & take).sum())]])
    return table, int((~f & take).sum()), labels, np.where(take, conf, np.float32("nan")), counts


# ----------------------------------------------------------------------------------------------------------------- prototypes
ACCUMULATE_PIXELS = 262144 + 65                # chunk 4096 is whole, chunk 4097 holds one pixel
ACCUMULATE_SHAPES = ((2, 4, 4), (23, 32, 32), (32, 64, 64))              # classes, dim, ldf: one per block size of PaShape
ACCUMULATE_PATTERNS = ("runs37", "random")
ACCUMULATE_BAD_PIXEL = 262144 + 10             # one NaN feature on the second trip
RECTIFY_PIXELS, RECTIFY_CASE = 1048576 + TAIL, (2, 4, 3.0, 1.0, 0)       # (C, D, logit scale, tau_scale, probs)
RECTIFY_FILL = -7.0
ASSIGN_CASE = dict(batch=1, ppi=4096 * 256 + 3, classes=2, dim=4, seed=11)


def accumulate_case(classes, dim, ldf, pattern):
    from test_gpu_proto import _features, _labels
    g = torch.Generator().manual_seed(1000 * classes + dim)
    feat = _features(ACCUMULATE_PIXELS, dim, ldf, g)
    feat[ACCUMULATE_BAD_PIXEL, dim - 1] = float("nan")
    return feat, _labels(pattern, ACCUMULATE_PIXELS, classes, g)


def check_accumulate(sums, sq, counts, mirror, calls=1):
    """Counts exactly, sums under tests/_proto_ref.py's derived bar (n_c 2^-52 sum|x| per cell; a second call doubles n and sum|x|).
    -> (worst sum error / bar, worst squared-norm error / bar)"""
    from _proto_ref import sum_bars
    ref_sums, ref_sq, ref_counts, abs_sums, abs_sq = mirror
    assert np.array_equal(counts, calls * ref_counts)
    assert int(ref_counts[-1]) == 1
    bar_s, bar_q = sum_bars(ref_counts, abs_sums, abs_sq)
    bar_s, bar_q = calls * calls * bar_s, calls * calls * bar_q
    err_s, err_q = np.abs(sums - calls * ref_sums), np.abs(sq - calls * ref_sq)
    assert (err_s <= bar_s).all(), float((err_s - bar_s).max())
    assert (err_q <= bar_q).all(), float((err_q - bar_q).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bar_s > 0, err_s / bar_s, 0.0))), float(np.nanmax(np.where(bar_q > 0, err_q / bar_q, 0.0)))


def accumulate_mutant(feat, lab, classes, dim):
    from _proto_ref import accumulate_mirror
    first = torch.from_numpy(L.first_trip(L.proto_accumulate(ACCUMULATE_PIXELS, dim), ACCUMULATE_PIXELS))
    return accumulate_mirror(feat[first][:, :dim].numpy(), lab[first].numpy(), classes)[:3]


def check_rectify(fig):
    """test_gpu_proto.test_rectify_against_float64's assertions on grade_case's figures."""
    from test_gpu_proto import EXCLUDED_CAP
    assert fig["excluded"] <= EXCLUDED_CAP, fig
    assert fig["moved_winner"] > 0.01, fig
    assert fig["kernel_err"] <= fig["bar"], fig
    assert fig["winner_ok"], fig


def rectify_mutant(feat, scores, proto, inv_tau):
    """The float64 mirror, rounded to fp32, beyond trip one at the output's pre-fill."""
    from _proto_ref import rectify_mirror
    C, _, _, _, probs = RECTIFY_CASE
    out = torch.from_numpy(rectify_mirror(feat.numpy(), scores.numpy(), proto.numpy(), np.ones(C), inv_tau, probs=bool(probs))).float()
    out[torch.from_numpy(~L.first_trip(L.proto_rectify(RECTIFY_PIXELS), RECTIFY_PIXELS))] = RECTIFY_FILL
    return out


def grade_assign(backend, log=print):
    """_contrast_ref.grade_case at the case's size with no loss combination: the assignment alone (graded, its NaN rows where the
    contract puts them, pad lanes 0, the same bits on a second call); the loss kernel has its own case past its grid."""
    import _contrast_ref as R
    c = ASSIGN_CASE
    return R.grade_case(backend, c["batch"], c["ppi"], c["classes"], c["dim"], c["seed"], log, combos=(), weight_variants=False)


def assign_mutant_backend():
    import _contrast_ref as R

    class FirstTripOnly(R.LegBackend):
        def assign(self, fbuf, dim, classes, ldc, proto, seen, inv_tau):
            out = super().assign(fbuf, dim, classes, ldc, proto, seen, inv_tau)
            out[~L.first_trip(L.proto_assign(len(out)), len(out))] = np.float32("nan")      # GpuBackend's pre-fill
            return out

    return FirstTripOnly()


# -------------------------------------------------------------------------------------------------------------- nearest resize
NEAREST_FILL = 201
NEAREST_CASES = {                              # n, source H x W, destination h x w
    "37x53_to_1025x1030": (2, 37, 53, 1025, 1030),     # 264 450 groups; rows start at both alignments, the last group is short
    "48x40_to_1026x1028": (2, 48, 40, 1026, 1028),     # 263 682 groups; every store a dword
}


def nearest_case(name):
    import _resize_ref as R
    n, H, W, h, w = NEAREST_CASES[name]
    src = np.random.default_rng(H + W).integers(0, 23, (n, H, W), dtype=np.uint8)
    return src, np.ascontiguousarray(R.nearest_resize(src, h, w))


def check_nearest(out, want):
    assert np.array_equal(out, want)


def nearest_mutant(want):
    _, h, w = want.shape
    return np.where(L.first_trip_nearest(h, w)[None], want, np.uint8(NEAREST_FILL))
