"""The labelled training augmentation on the device: ``data.train_batch`` (csrc/augment.hip, csrc/elastic_field.hip) against the float64 numpy
restatement of its definition (tests/_train_aug_ref.py; INTEGRATION.md, "Training augmentation").

Image bars as in tests/test_gpu_finetune.py: per sample, |kernel - f64| <= max(4 x |f32 - f64| of the restatement, 2 ulp of fp32
at the output's magnitude); pixels whose hue is decided by rounding noise are left out of the ``chain`` comparison only (at most
0.2 % of a batch).  Mask bar: the nearest label is decided by rounding noise where ``r + 0.5`` lies within ``band`` of an integer,
``band = max(4 x max |r_f32 - r_f64| over the sample, 2 ulp of fp32 at max(H, W))``.  Outside that band the kernel's label equals
the restatement's exactly; inside it equals the label at one of the (up to four) source pixels on either side of the tie; the
band holds at most 1 % of a sample's pixels.  Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import math
import os

import numpy as np
import pytest
import torch

import _train_aug_ref as T
from test_gpu_finetune import frames

pytestmark = pytest.mark.gpu

LABELS = ("optical", "grid", "elastic", "affine+optical", "affine+elastic", "chain", "mask_only_d4")
SIZES = ((24, 24), (65, 65), (17, 33), (130, 70), (256, 256))
ILL_CAP = 0.002
BAND_CAP = 0.01


def label_masks(n, h, w):
    """Random labels in 0..22 with a sprinkle of 255 (the ignore value has to pass through unchanged)."""
    rng = np.random.default_rng(77 + 3 * h + w)
    m = rng.integers(0, 23, (n, h, w), dtype=np.uint8)
    m[rng.random((n, h, w)) < 0.02] = 255
    return m


def _key(i, salt):
    return ((0x9E3779B9 * (i + 1)) & 0xFFFFFFFF, (salt ^ (i * 2654435761)) & 0xFFFFFFFF)


def set_distortion(D, P, i, kind, n):
    t = i / max(n - 1, 1)
    if kind == D.DISTORT_OPTICAL:
        P.set_optical(i, -0.05 + 0.1 * t, -0.05 + 0.1 * ((i * 3) % n) / max(n - 1, 1), 0.05 - 0.1 * ((i * 5) % n) / max(n - 1, 1))
    elif kind == D.DISTORT_GRID:
        P.set_grid(i, [1.0 + 0.3 * math.sin(1.7 * i + 0.9 * j + 0.3) for j in range(6)],
                   [1.0 + 0.3 * math.cos(1.3 * i + 1.1 * j + 0.2) for j in range(6)])
    else:
        P.set_elastic(i, 120.0 if i % 2 == 0 else 30.0 + 90.0 * t, _key(i, 0xC0FFEE))


def set_affine(P, i, n, h, w):
    """Generic parameters: no angle, scale or shift that puts whole lines of a small frame exactly on a nearest-label tie."""
    t = i / max(n - 1, 1)
    P.set_affine(i, (2 * t - 1) * 0.06 * w + 0.1372, (1 - 2 * t) * 0.06 * h - 0.0913, 0.81 + 0.37 * t, -43.0 + 83.0 * t)


def records(D, n, h, w, label):
    """TrainAugParams with sample i on D4 code i (non-transposing codes on non-square frames) and the label's stages on."""
    codes = list(range(8)) if h == w else [0, 2, 4, 6]
    P = D.TrainAugParams(n, h, w, [codes[i % len(codes)] for i in range(n)])
    chain = label == "chain"
    for i in range(n):
        t = i / max(n - 1, 1)
        if chain:
            P.set_noise(i, math.sqrt(10 + 40 * t), _key(i, 0xDEADBEEF))
            P.set_blur(i, i % 3, 3 if (i // 3) % 2 == 0 else 5, (i + 1) % 4)
        if "affine" in label or chain:
            set_affine(P, i, n, h, w)
        for name, kind in (("optical", D.DISTORT_OPTICAL), ("grid", D.DISTORT_GRID), ("elastic", D.DISTORT_ELASTIC)):
            if name in label.split("+"):
                set_distortion(D, P, i, kind, n)
        if chain:
            set_distortion(D, P, i, 1 + i % 3, n)
            if i % 3 == 0:
                P.set_stage5(i, D.STAGE5_SHARPEN, 0.2 + 0.3 * t, 1.0 - 0.5 * t)
            elif i % 3 == 1:
                P.set_stage5(i, D.STAGE5_EMBOSS, 0.5 - 0.3 * t, 0.2 + 0.5 * t)
            else:
                P.set_stage5(i, D.STAGE5_BRIGHTNESS_CONTRAST, -0.2 + 0.4 * t, 0.2 - 0.4 * ((i * 3) % n) / max(n - 1, 1))
            P.set_hsv(i, -20 + 40 * t, 30 - 60 * ((i * 3) % n) / max(n - 1, 1), -20 + 40 * ((i * 5) % n) / max(n - 1, 1))
    return P


_REF = {}


def reference(D, label, name, h, w, n=8):
    """The case's inputs, records and both evaluations of the restatement: computed once, shared, left unchanged."""
    key = (label, name, h, w, n)
    if key not in _REF:
        imgs, masks, P = frames(name, n, h, w), label_masks(n, h, w), records(D, n, h, w, label)
        img64, m64, r64, ill = T.run(imgs, masks, P, np.float64)
        img32, _, r32, _ = T.run(imgs, masks, P, np.float32)
        band = T.band_width(r64, r32, h, w)
        ref = dict(imgs=imgs, masks=masks, P=P, img64=img64, img32=img32, m64=m64, r64=r64, ill=ill, band=band,
                   in_band=T.tie_band(r64, band))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.fixture(scope="module")
def D():
    from uda_aerial_semantic_segmentation_research_amd import _lib, data
    _lib.require_gpu()
    return data


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).float().cpu().numpy()


def check_images(got, ref, keep, tag):
    """Per sample |kernel - f64| <= max(4 x |f32 - f64|, 2 ulp); returns the worst (err, dev, bar)."""
    worst, failures = None, []
    for i in range(got.shape[0]):
        k = keep[i]
        dev = np.abs(ref["img32"][i].astype(np.float64) - ref["img64"][i])[k].max()
        bar = max(4 * dev, 2 * float(np.spacing(np.float32(np.abs(ref["img64"][i]).max()))))
        err = np.abs(got[i] - ref["img64"][i])[k].max()
        if worst is None or err / bar > worst[0] / worst[2]:
            worst = (err, dev, bar)
        if not err <= bar:
            failures.append((i, err, dev, bar))
    return worst, failures


def check_masks(got_m, ref, tag):
    """Exact outside the tie band, one of the tie's candidates inside; the band's share per sample is capped.  Returns the
    largest share."""
    shares = []
    for i in range(got_m.shape[0]):
        band = ref["in_band"][i]
        shares.append(band.mean())
        assert band.mean() <= BAND_CAP, (tag, i, band.mean())
        assert np.array_equal(got_m[i][~band], ref["m64"][i][~band]), (tag, i, int((got_m[i] != ref["m64"][i])[~band].sum()))
        if band.any():
            cand = T.mask_candidates(ref["masks"][i], int(ref["P"].d4[i]), ref["r64"][i], ref["band"][i])
            assert (cand == got_m[i][None]).any(axis=0)[band].all(), (tag, i)
    return max(shares)


# ------------------------------------------------------------------------------- every stage and the chain, value by value
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("name", ("random", "smooth"))
@pytest.mark.parametrize("label", LABELS)
def test_stage_against_float64_definition(D, label, name, h, w):
    n = 8
    ref = reference(D, label, name, h, w, n)
    P, ill = ref["P"], ref["ill"]
    masked = label == "chain"
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    keep = ~ill if masked else np.ones_like(ill)
    dev_img, dev_msk = torch.tensor(ref["imgs"]).cuda(), torch.tensor(ref["masks"]).cuda()    # copies: the reference stays read-only
    got32, gm = D.train_batch(dev_img, dev_msk, P)
    assert got32.shape == (n, 3, h, w) and got32.dtype == torch.float32
    assert gm.shape == (n, h, w) and gm.dtype == torch.int64
    got = _nhwc(got32).astype(np.float64)
    assert np.isfinite(got).all()
    tag = f"{label} {name} {h}x{w}"
    worst, failures = check_images(got, ref, keep, tag)
    got_m = gm.cpu().numpy()
    share = check_masks(got_m, ref, tag)
    _log(f"train_aug {label:14s} {name:6s} {h:3d}x{w:<3d}  kernel-vs-f64 {worst[0]:.3e}  f32-vs-f64 {worst[1]:.3e}  bar {worst[2]:.3e}  "
         f"left out {ill.mean() if masked else 0.0:.5f}  band {ref['band'].max():.3e}  band share {share:.5f}")
    assert not failures, failures
    if label == "mask_only_d4":                                 # nothing but the basic pipeline: exact, image and mask
        assert np.array_equal(_nhwc(got32), ref["img32"]) and np.array_equal(got_m, ref["m64"])
    got16, gm16 = D.train_batch(dev_img, dev_msk, P, dtype=torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, got32.to(torch.bfloat16))
    assert torch.equal(gm16, gm)


# ------------------------------------------------------------------------------------------------ the field on its own
@pytest.mark.parametrize("h,w", SIZES)
def test_elastic_field_against_float64_definition(D, h, w):
    n = 8
    P = records(D, n, h, w, "elastic")
    got = D.elastic_field(P)
    assert got.shape == (n, h, w, 2) and got.dtype == torch.float32
    assert torch.equal(got, D.elastic_field(P))                 # two calls: the same bits
    got = got.cpu().numpy().astype(np.float64)
    worst = None
    for i in range(n):
        f64 = T.elastic_field(P.ints[i], h, w, 6.0, np.float64)
        f32 = T.elastic_field(P.ints[i], h, w, 6.0, np.float32)
        dev = np.abs(f32.astype(np.float64) - f64).max()
        bar = max(4 * dev, 2 * float(np.spacing(np.float32(np.abs(f64).max()))))
        err = np.abs(got[i] - f64).max()
        if worst is None or err / bar > worst[0] / worst[2]:
            worst = (err, dev, bar)
        assert err <= bar, (i, err, dev, bar)
    _log(f"train_aug field          {h:3d}x{w:<3d}  kernel-vs-f64 {worst[0]:.3e}  f32-vs-f64 {worst[1]:.3e}  bar {worst[2]:.3e}")
    # samples on another kind are left alone
    Q = records(D, n, h, w, "optical")
    assert float(D.elastic_field(Q).abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("h,w", [(24, 24), (17, 33), (130, 70)])
def test_all_off_is_prepare_batch_and_strong_stages_are_strong_views(D, h, w):
    n = 8
    imgs = torch.from_numpy(frames("random", n, h, w)).cuda()
    masks_np = label_masks(n, h, w)
    masks = torch.from_numpy(masks_np).cuda()
    codes = torch.tensor(list(range(8)) if h == w else [0, 2, 4, 6, 0, 2, 4, 6], dtype=torch.int32)
    off = D.TrainAugParams(n, h, w, codes.numpy())
    for dtype in (torch.float32, torch.bfloat16):
        want, want_m = D.prepare_batch(imgs, masks, codes, dtype=dtype)
        got, got_m = D.train_batch(imgs, masks, off, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, want) and got.stride() == want.stride()
        assert got_m.dtype == torch.int64 and torch.equal(got_m, want_m)
        only, none = D.train_batch(imgs, None, off, dtype=dtype)
        assert none is None and torch.equal(only, want)
    # the mask of a D4-only record is numpy indexing
    _, got_m = D.train_batch(imgs, masks, off)
    for i in range(n):
        a = masks_np[i]
        c = int(codes[i])
        a = a.T if c & 1 else a
        a = a[::-1] if c & 2 else a
        a = a[:, ::-1] if c & 4 else a
        assert np.array_equal(got_m[i].cpu().numpy(), a.astype(np.int64))
    # records that use the strong stages only: strong_views of the same first 32 words, bit for bit
    from test_gpu_finetune import records as strong_records
    for label in ("noise", "median", "motion", "affine", "sharpen", "emboss", "bc", "hsv", "chain"):
        (_, S), = strong_records(D, n, h, w, (label,))
        Tp = D.TrainAugParams(n, h, w)
        Tp.ints[:, :32] = S.ints
        assert np.array_equal(Tp.ints[:, 32:], np.zeros((n, 32), dtype=np.int32))
        for dtype in (torch.float32, torch.bfloat16):
            got, none = D.train_batch(imgs, None, Tp, dtype=dtype)
            assert none is None and torch.equal(got, D.strong_views(imgs, S, dtype=dtype)), (label, dtype)


# ---------------------------------------------------------------------------------------------------- joint geometry
def test_image_and_mask_take_the_same_map(D):
    """A frame of 8 x 8 constant blocks whose three channels carry the block's label, and the same labels as the mask: where all
    four bilinear taps fall into one block the label decoded from the output image has to be the output mask's."""
    n, h, w, b = 8, 64, 64, 8
    by, bx = np.meshgrid(np.arange(h) // b, np.arange(w) // b, indexing="ij")
    lab = ((3 * by + 5 * bx) % 23).astype(np.uint8)
    masks = np.stack([(lab + i) % 23 for i in range(n)]).astype(np.uint8)
    imgs = np.repeat(masks[..., None], 3, axis=-1)
    P = D.TrainAugParams(n, h, w, list(range(8)))
    for i in range(n):
        set_affine(P, i, n, h, w)
        set_distortion(D, P, i, D.DISTORT_ELASTIC, n)
    got, gm = D.train_batch(torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda(), P)
    level = _nhwc(got).astype(np.float64) * (T.S.STD.astype(np.float64) * 255.0) + T.S.MEAN.astype(np.float64) * 255.0
    _, _, r64, _ = T.run(imgs, masks, P, np.float64)
    x0, y0 = np.floor(r64[..., 0]).astype(np.int64), np.floor(r64[..., 1]).astype(np.int64)
    bx0, bx1 = T.S.reflect101(x0, w) // b, T.S.reflect101(x0 + 1, w) // b
    by0, by1 = T.S.reflect101(y0, h) // b, T.S.reflect101(y0 + 1, h) // b
    inner = (bx0 == bx1) & (by0 == by1)
    assert inner.mean() > 0.3
    decoded = np.rint(level[..., 0]).astype(np.int64)
    assert np.abs(level - decoded[..., None])[inner].max() < 1e-3            # a constant neighbourhood: the label itself
    assert np.array_equal(decoded[inner], gm.cpu().numpy()[inner])


# ----------------------------------------------------------------------------------------------------- drawn records
def test_drawn_records_full_pipeline(D):
    n, h, w = 16, 64, 64
    imgs, masks = frames("random", n, h, w), label_masks(n, h, w)
    P = D.draw_training_params(n, h, w, torch.Generator().manual_seed(11))
    img64, m64, r64, ill = T.run(imgs, masks, P, np.float64)
    img32, _, r32, _ = T.run(imgs, masks, P, np.float32)
    band = T.band_width(r64, r32, h, w)
    ref = dict(img64=img64, img32=img32, m64=m64, r64=r64, band=band, in_band=T.tie_band(r64, band), masks=masks, P=P)
    assert ill.mean() <= ILL_CAP
    host = D.train_batch(torch.from_numpy(imgs), torch.from_numpy(masks), P)                     # host tensors
    dev = D.train_batch(torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda(), P)        # device tensors
    again = D.train_batch(torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda(), P)
    assert torch.equal(host[0], dev[0]) and torch.equal(host[1], dev[1])
    assert torch.equal(again[0], dev[0]) and torch.equal(again[1], dev[1])                        # repeated calls: equal bits
    worst, failures = check_images(_nhwc(dev[0]).astype(np.float64), ref, ~ill, "drawn")
    share = check_masks(dev[1].cpu().numpy(), ref, "drawn")
    _log(f"train_aug drawn          random  64x64   kernel-vs-f64 {worst[0]:.3e}  f32-vs-f64 {worst[1]:.3e}  bar {worst[2]:.3e}  "
         f"left out {ill.mean():.5f}  band {band.max():.3e}  band share {share:.5f}")
    assert not failures, failures
    # params=None draws from the generator: the same seed, the same batch
    a = D.train_batch(torch.from_numpy(imgs), torch.from_numpy(masks), None, torch.Generator().manual_seed(11))
    assert torch.equal(a[0], dev[0]) and torch.equal(a[1], dev[1])


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(D):
    n, h, w = 2, 16, 16
    imgs, masks = torch.zeros((n, h, w, 3), dtype=torch.uint8), torch.zeros((n, h, w), dtype=torch.uint8)
    P = D.TrainAugParams(n, h, w)
    for bad in (dict(images_u8=imgs.float()), dict(images_u8=imgs[..., :2]), dict(images_u8=imgs[0]),
                dict(masks_u8=masks.long()), dict(masks_u8=masks[:, :8]), dict(masks_u8=masks[:1]),
                dict(params=D.StrongAugParams(n, h, w)), dict(params=P.table), dict(params=D.TrainAugParams(n, h, 8)),
                dict(dtype=torch.float16), dict(elastic_sigma=7.0)):
        kw = dict(images_u8=imgs, masks_u8=masks, params=P)
        kw.update(bad)
        if "elastic_sigma" in bad:                               # radius 21 > 18: refused when a record needs the field
            Q = D.TrainAugParams(n, h, w)
            Q.set_elastic(0, 10.0, (1, 2))
            kw["params"] = Q
        with pytest.raises(ValueError):
            D.train_batch(**kw)
    G = D.TrainAugParams(1, 4, 16)
    G.set_grid(0, [1.0] * 6, [1.0] * 6)
    with pytest.raises(ValueError):
        D.train_batch(torch.zeros((1, 4, 16, 3), dtype=torch.uint8), None, G)
    two = D.TrainAugParams(n, h, w)
    two.set_optical(0, 0.01)
    two.set_elastic(0, 10.0, (1, 2))
    with pytest.raises(ValueError):
        D.train_batch(imgs, masks, two)
    with pytest.raises(ValueError):
        D.strong_views(imgs, P)                                   # and the 64-word records are no strong records


# ---------------------------------------------------------------------------------------------------------- trainers
def _u8_batches(count, n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [(torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)),
             torch.from_numpy(rng.integers(0, 23, (n, h, w), dtype=np.uint8))) for _ in range(count)]


def test_device_augmented_loader_drives_the_trainers(D):
    from uda_aerial_semantic_segmentation_research_amd.adversarial_trainer import AdversarialTrainer
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23)
    tr = SegmentationTrainer(net, dev)
    loader = D.DeviceAugmentedLoader(_u8_batches(2, 2, 64, 64, 5), generator=torch.Generator().manual_seed(3))
    assert len(loader) == 2
    for x, m in loader:                                           # what the trainer gets: read in place by the first conv
        assert x.shape == (2, 3, 64, 64) and m.dtype == torch.int64 and m.shape == (2, 64, 64)
        assert x.to(dev) is x
        pv = net._padded_input_view(x)
        assert pv is not None and pv.data_ptr() == x.data_ptr()
    loss = tr.train_epoch(loader, FusedAdam(net.parameters(), lr=1e-4), 1)
    assert math.isfinite(loss) and all(torch.isfinite(p).all() for p in net.parameters())
    # images alone: plain tensors, which the adversarial trainer's target side takes
    target = D.DeviceAugmentedLoader([b[0] for b in _u8_batches(1, 2, 64, 64, 6)], generator=torch.Generator().manual_seed(4))
    for t in target:
        assert torch.is_tensor(t) and t.shape == (2, 3, 64, 64)
    adv = AdversarialTrainer(Unet("resnet18", encoder_weights=None, in_channels=3, classes=23), dev)
    mean_loss, metrics = adv.train_epoch(loader, target, FusedAdam(adv.model.parameters(), lr=1e-4), 1)
    assert math.isfinite(mean_loss) and all(math.isfinite(v) for v in adv.last_losses.values())
