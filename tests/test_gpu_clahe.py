"""CLAHE in the two device augmentation pipelines (csrc/clahe.hip and the output passes' stage-5 kind 3) against the numpy
restatement of its definition (tests/_clahe_ref.py; INTEGRATION.md, "CLAHE").

The table is integer arithmetic on the bins ``k = floor(L8 + 0.5)``, so it is compared exactly wherever no pixel's bin is
decided by rounding noise: on grey frames drawn from the levels whose ``L8`` keeps ``MARGIN`` from every bin boundary (254 of
the 256; the margin is asserted, as is the fp32 evaluation's distance from the float64 one), and on colour frames made of a
seeded palette with the same property.  The output is held to the float64 restatement by tests/test_gpu_train_aug.py's bar,
per sample |kernel - f64| <= max(4 x |f32 - f64| of the restatement, 2 ulp of fp32 at the output's magnitude), both evaluated
with the device's own table; pixels whose ``L8`` lies within ``max(4 x |L8_f32 - L8_f64|, 1e-4)`` of a bin boundary are left out
(at most 0.2 % of a batch, which the inputs have to satisfy by the restatement alone), and the device table is held to the
float64 one separately: equal in every tile without such a pixel, within ``1 + ceil(255 m / area)`` in a tile with ``m`` of them.
Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import math
import os

import numpy as np
import pytest
import torch

import _clahe_ref as C
from test_gpu_finetune import frames
from test_gpu_train_aug import label_masks, set_affine, set_distortion

pytestmark = pytest.mark.gpu

MARGIN = 2e-3                    # distance every L8 of the exact tests keeps from a bin boundary
LEFT_CAP = 0.002
ILL_CAP = 0.002
PALETTE_SEED = 7                 # colour palette of the exact colour test: change the seed if a colour comes within MARGIN


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


def _params(D, pipe, n, h, w, codes=None):
    return (D.TrainAugParams if pipe == "train" else D.StrongAugParams)(n, h, w, codes)


def _run(pipe, imgs, P, dt, luts=None):
    return C.run_train(imgs, None, P, dt, luts) if pipe == "train" else C.run_strong(imgs, P, dt, luts)


def _device(D, pipe, imgs, P, dtype=torch.float32, masks=None):
    """(image tensor, masks or None, tables uint8 [n,8,8,256]) of one full call."""
    n = imgs.shape[0]
    lut = torch.zeros((n, 8, 8, 256), dtype=torch.uint8, device="cuda")
    if pipe == "train":
        out, m = D.train_batch(imgs, masks, P, dtype=dtype, clahe_tables=lut)
        return out, m, lut
    return D.strong_views(imgs, P, dtype=dtype, clahe_tables=lut), None, lut


# ------------------------------------------------------------------------------------------------- the table pass, exact
def grey_levels():
    """(the grey levels whose L8 keeps MARGIN from every bin boundary, their L8 in float64, |L8_f32 - L8_f64| over them)."""
    v = np.repeat(np.arange(256, dtype=np.float64)[:, None], 3, axis=1)
    l64 = C.rgb_to_lab(v, np.float64)[0]
    l32 = C.rgb_to_lab(v.astype(np.float32), np.float32)[0]
    ok = C.boundary_distance(l64) > MARGIN
    return np.nonzero(ok)[0], l64, np.abs(l32.astype(np.float64) - l64)[ok].max()


def grey_batch(h, w):
    """Four grey frames: levels drawn from all the safe ones, from a palette of twelve, a constant frame, and a frame for the
    sample that is not on CLAHE."""
    levels, _, _ = grey_levels()
    rng = np.random.default_rng(h * 1000 + w)
    g = np.empty((4, h, w), dtype=np.uint8)
    g[0] = rng.choice(levels, (h, w))
    g[1] = rng.choice(rng.choice(levels, 12, replace=False), (h, w))
    g[2] = levels[len(levels) // 3]
    g[3] = rng.choice(levels, (h, w))
    return np.repeat(g[..., None], 3, axis=-1)


def test_grey_levels_keep_the_margin():
    levels, l64, dev32 = grey_levels()
    left = sorted(set(range(256)) - set(int(v) for v in levels))
    _log(f"clahe grey levels: within {MARGIN} of a boundary {left}; fp32 L8 off by {dev32:.2e}")
    assert left == [142, 223]
    assert dev32 <= MARGIN / 8                                    # fp32 cannot carry a safe level across a boundary


@pytest.mark.parametrize("pipe", ("strong", "train"))
@pytest.mark.parametrize("h,w,clip", [(64, 64, 1.0), (128, 96, 3.0), (256, 256, 4.0)])
def test_table_pass_exact_on_grey_frames(D, pipe, h, w, clip):
    imgs = grey_batch(h, w)
    P = _params(D, pipe, 4, h, w)
    for i in range(3):
        P.set_clahe(i, clip)
    P.set_stage5(3, D.STAGE5_SHARPEN, 0.3, 0.7)
    ref = _run(pipe, imgs, P, np.float64)
    info = [t for s in ref["info"][:3] for t in s]
    area = (h // 8) * (w // 8)
    assert all(t["limit"] == max(1, int(clip * area / 256)) for t in info)
    if (h, w) == (64, 64):                                        # limit 1, the remainder path with a step above 1
        assert info[0]["limit"] == 1 and any(t["rest"] > 0 and t["step"] > 1 for t in info)
    if (h, w) == (256, 256):                                      # area 1024, limit 16: a non-zero even share per bin
        assert info[0]["limit"] == 16 and any(t["share"] > 0 for t in info) and any(t["rest"] > 0 for t in info)
    assert all(t["excess"] == area - info[0]["limit"] for t in ref["info"][2])      # the constant frame: one bin per tile
    dev = torch.from_numpy(imgs).cuda()
    got = D.clahe_tables(dev, P)
    assert got.shape == (4, 8, 8, 256) and got.dtype == torch.uint8
    assert np.array_equal(got[:3].cpu().numpy(), ref["lut"][:3])
    assert not got[3].any()                                       # not on CLAHE: its rows are not written
    assert torch.equal(got, D.clahe_tables(dev, P))
    _, _, full = _device(D, pipe, dev, P)                         # the full call's table pass: the same bytes
    assert torch.equal(full, got)


def palette_batch(n, h, w):
    rng = np.random.default_rng(PALETTE_SEED)
    palette = rng.integers(0, 256, (200, 3), dtype=np.uint8)
    return palette[rng.integers(0, 200, (n, h, w))], palette


@pytest.mark.parametrize("pipe", ("strong", "train"))
def test_table_pass_exact_on_colour_frames(D, pipe):
    n, h, w = 4, 64, 64
    imgs, palette = palette_batch(n, h, w)
    l64 = C.rgb_to_lab(palette.astype(np.float64), np.float64)[0]
    l32 = C.rgb_to_lab(palette.astype(np.float32), np.float32)[0]
    assert C.boundary_distance(l64).min() > MARGIN, "a palette colour lies within the margin: change the seed"
    assert np.abs(l32.astype(np.float64) - l64).max() <= MARGIN / 8
    P = _params(D, pipe, n, h, w, [0, 3, 5, 6])                   # no affine; the D4 code moves pixels between tiles
    for i in range(n):
        P.set_clahe(i, 1.0 + i)
    ref = _run(pipe, imgs, P, np.float64)
    got = D.clahe_tables(torch.from_numpy(imgs).cuda(), P)
    assert np.array_equal(got.cpu().numpy(), ref["lut"])


# --------------------------------------------------------------------------------------- output against float64, value by value
LABELS = {"strong": ("clahe", "affine+clahe", "chain"), "train": ("clahe", "affine+clahe", "elastic+clahe", "chain")}
CASES = [(pipe, label) for pipe in ("strong", "train") for label in LABELS[pipe]]


def _key(i, salt):
    return ((0x9E3779B9 * (i + 1)) & 0xFFFFFFFF, (salt ^ (i * 2654435761)) & 0xFFFFFFFF)


def case_records(D, pipe, label, n, h, w):
    """Every sample on CLAHE (clip limits sweeping 1..4) after the label's stages; D4 code i (non-transposing when h != w)."""
    codes = list(range(8)) if h == w else [0, 2, 4, 6]
    P = _params(D, pipe, n, h, w, [codes[i % len(codes)] for i in range(n)])
    chain = label == "chain"
    for i in range(n):
        t = i / max(n - 1, 1)
        if chain:
            P.set_noise(i, math.sqrt(10 + 40 * t), _key(i, 0xDEADBEEF))
            P.set_blur(i, i % 3, 3 if (i // 3) % 2 == 0 else 5, (i + 1) % 4)
        if "affine" in label or chain:
            set_affine(P, i, n, h, w)
        if pipe == "train" and ("elastic" in label or chain):
            set_distortion(D, P, i, D.DISTORT_ELASTIC if "elastic" in label else 1 + i % 3, n)
        P.set_clahe(i, 1.0 + 3.0 * t)
        if chain:
            P.set_hsv(i, -20 + 40 * t, 30 - 60 * ((i * 3) % n) / max(n - 1, 1), -20 + 40 * ((i * 5) % n) / max(n - 1, 1))
    return P


def case_frames(label, n, h, w):
    """CLAHE alone: independent uniform channels.  With a gather in front, a colour gradient: the float32 gather of a noisy
    frame alone would put more pixels next to a bin boundary than the cap allows."""
    return frames("random" if label == "clahe" else "smooth", n, h, w)


_REF = {}


def reference(D, pipe, label, h, w, n=4):
    """Inputs, records and both evaluations of the restatement with the frames' own tables: computed once, left unchanged."""
    key = (pipe, label, h, w, n)
    if key not in _REF:
        imgs, P = case_frames(label, n, h, w), case_records(D, pipe, label, n, h, w)
        r64, r32 = _run(pipe, imgs, P, np.float64), _run(pipe, imgs, P, np.float32)
        band = np.maximum(4 * np.abs(r32["l8"].astype(np.float64) - r64["l8"]), 1e-4)
        ref = dict(imgs=imgs, P=P, lut64=r64["lut"], l8=r64["l8"], left=C.boundary_distance(r64["l8"]) <= band, ill=r64["ill"],
                   band=band)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def check_tables(got, ref, h, w, tag):
    """Exact in every tile without a left-out pixel, within 1 + ceil(255 m / area) elsewhere; returns (tiles with one, worst)."""
    th, tw = h // 8, w // 8
    area, touched, worst = th * tw, 0, 0
    for i in range(got.shape[0]):
        for ty in range(8):
            for tx in range(8):
                m = int(ref["left"][i, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].sum())
                d = int(np.abs(got[i, ty, tx].astype(np.int64) - ref["lut64"][i, ty, tx].astype(np.int64)).max())
                if m == 0:
                    assert d == 0, (tag, i, ty, tx, d)
                else:
                    touched += 1
                    worst = max(worst, d)
                    assert d <= 1 + math.ceil(255 * m / area), (tag, i, ty, tx, d, m)
    return touched, worst


@pytest.mark.parametrize("h,w", [(64, 64), (136, 72)])
@pytest.mark.parametrize("pipe,label", CASES)
def test_output_against_float64_definition(D, pipe, label, h, w):
    n = 4
    ref = reference(D, pipe, label, h, w, n)
    left, ill, P = ref["left"], ref["ill"], ref["P"]
    assert left.mean() <= LEFT_CAP, f"share next to a bin boundary {left.mean():.5f} above the cap: change the input"
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    dev_img = torch.tensor(ref["imgs"]).cuda()                   # a copy: the reference stays read-only
    got32, _, lut = _device(D, pipe, dev_img, P)
    assert got32.shape == (n, 3, h, w) and got32.dtype == torch.float32
    lut = lut.cpu().numpy()
    tag = f"{pipe} {label} {h}x{w}"
    touched, tworst = check_tables(lut, ref, h, w, tag)
    d64, d32 = _run(pipe, ref["imgs"], P, np.float64, lut), _run(pipe, ref["imgs"], P, np.float32, lut)
    got = _nhwc(got32).astype(np.float64)
    assert np.isfinite(got).all()
    keep = ~left & ~ill
    worst, failures = None, []
    for i in range(n):
        k = keep[i]
        dev = np.abs(d32["img"][i].astype(np.float64) - d64["img"][i])[k].max()
        bar = max(4 * dev, 2 * float(np.spacing(np.float32(np.abs(d64["img"][i]).max()))))
        err = np.abs(got[i] - d64["img"][i])[k].max()
        if worst is None or err / bar > worst[0] / worst[2]:
            worst = (err, dev, bar)
        if not err <= bar:
            failures.append((i, err, dev, bar))
    _log(f"clahe {pipe:6s} {label:13s} {h:3d}x{w:<3d}  kernel-vs-f64 {worst[0]:.3e}  f32-vs-f64 {worst[1]:.3e}  bar {worst[2]:.3e}  "
         f"left out {left.mean():.5f} (band up to {ref['band'].max():.2e})  hue-ill {ill.mean():.5f}  "
         f"tiles with a left-out pixel {touched} (table off by up to {tworst})")
    assert not failures, failures
    got16, _, lut16 = _device(D, pipe, dev_img, P, dtype=torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, got32.to(torch.bfloat16))
    assert np.array_equal(lut16.cpu().numpy(), lut)


# ------------------------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("pipe", ("strong", "train"))
def test_mixed_batch_routes_per_sample(D, pipe):
    """Sample 0 on CLAHE, 1 on sharpen, 2 all off, 3 the full chain with sharpen: 1..3 equal the plain entry points' output bit
    for bit, masks do not see CLAHE, calls repeat bit for bit, host and device inputs agree."""
    n, h, w = 4, 64, 64
    imgs = frames("random", n, h, w)
    masks = label_masks(n, h, w) if pipe == "train" else None

    def records(clahe):
        P = _params(D, pipe, n, h, w, [1, 2, 4, 7])
        set_affine(P, 0, n, h, w)
        if pipe == "train":
            set_distortion(D, P, 0, D.DISTORT_GRID, n)
            set_distortion(D, P, 3, D.DISTORT_ELASTIC, n)
        if clahe:
            P.set_clahe(0, 2.5)
        P.set_stage5(1, D.STAGE5_SHARPEN, 0.3, 0.8)
        P.set_noise(3, 5.0, (11, 12))
        P.set_blur(3, D.BLUR_MEDIAN, 3)
        set_affine(P, 3, n, h, w)
        P.set_stage5(3, D.STAGE5_EMBOSS, 0.3, 0.4)
        P.set_hsv(3, 10.0, -20.0, 5.0)
        return P

    on, off = records(True), records(False)
    dev_img = torch.from_numpy(imgs).cuda()
    dev_m = None if masks is None else torch.from_numpy(masks).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        a, am, lut = _device(D, pipe, dev_img, on, dtype, dev_m)
        b, bm, _ = _device(D, pipe, dev_img, off, dtype, dev_m)           # no CLAHE record: the plain entry point
        assert torch.equal(a[1:], b[1:]) and not torch.equal(a[0], b[0])
        assert lut[0].any() and not lut[1:].any()
        if pipe == "train":
            assert torch.equal(am, bm)
        a2, am2, lut2 = _device(D, pipe, dev_img, on, dtype, dev_m)
        assert torch.equal(a, a2) and torch.equal(lut, lut2)
        host_m = None if masks is None else torch.from_numpy(masks)
        a3, am3, _ = _device(D, pipe, torch.from_numpy(imgs), on, dtype, host_m)      # host tensors
        assert torch.equal(a, a3) and (am is None or torch.equal(am, am3))
    if pipe == "strong":                                          # two views, one of them without a CLAHE record
        va, vb = D.strong_views(dev_img, on, off)
        assert torch.equal(va, D.strong_views(dev_img, on)) and torch.equal(vb, D.strong_views(dev_img, off))


def test_bf16_is_fp32_rounded_once_and_caller_buffer_is_optional(D):
    n, h, w = 2, 64, 64
    imgs = torch.from_numpy(frames("random", n, h, w)).cuda()
    P = D.TrainAugParams(n, h, w)
    P.set_clahe(0, 2.0)
    P.set_clahe(1, 4.0)
    a, _ = D.train_batch(imgs, None, P)
    b, _ = D.train_batch(imgs, None, P, dtype=torch.bfloat16)
    assert torch.equal(b, a.to(torch.bfloat16))
    with pytest.raises(ValueError):
        D.train_batch(imgs, None, P, clahe_tables=torch.zeros(n * 8 * 8 * 256, dtype=torch.uint8))        # on the host
    with pytest.raises(ValueError):
        D.train_batch(imgs, None, P, clahe_tables=torch.zeros(8 * 8 * 256, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(D):
    import ctypes
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    n = 2
    # Python: sides not divisible by 8, a clip limit below 1
    for h, w in ((60, 64), (64, 60)):
        imgs = torch.zeros((n, h, w, 3), dtype=torch.uint8)
        for cls, call in ((D.StrongAugParams, lambda P: D.strong_views(imgs, P)), (D.TrainAugParams, lambda P: D.train_batch(imgs, None, P))):
            P = cls(n, h, w)
            call(P)                                               # without a CLAHE record the frame is fine
            P.set_clahe(1, 2.0)
            with pytest.raises(ValueError):
                call(P)
            with pytest.raises(ValueError):
                D.clahe_tables(imgs, P)
    imgs = torch.zeros((n, 64, 64, 3), dtype=torch.uint8)
    P = D.TrainAugParams(n, 64, 64)
    P.set_clahe(0, 2.0)
    P.floats[0, 15] = 0.5
    with pytest.raises(ValueError):
        D.train_batch(imgs, None, P)
    Q = D.TrainAugParams(n, 64, 64)
    Q.set_clahe(0, 2.0)
    Q.set_noise(0, 3.0, (1, 2))
    with pytest.raises(ValueError):
        D.clahe_tables(imgs, Q)                                   # needs the source pass: the full call hands its tables out
    # C level: a missing table buffer and bad sides are error codes, and the output buffer stays as it was
    h = w = 64
    img = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((n, h, w, 4), 7.0, device="cuda")
    lut = torch.full((n, 8, 8, 256), 9, dtype=torch.uint8, device="cuda")
    m255, r255 = D.normalize_constants()
    on = D.StrongAugParams(n, h, w)
    on.set_clahe(0, 2.0)
    st, tt = on.table.cuda(), D.TrainAugParams(n, h, w).table.cuda()
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.udaseg_strong_aug_clahe_u8(p(img), p(st), 1, n, h, w, None, m255, r255, p(out), 4, 0, 0, None, stream) == -1
    assert b"table buffer" in lib.udaseg_last_error()
    assert lib.udaseg_train_aug_clahe_u8(p(img), None, p(tt), n, h, w, None, None, None, 0, m255, r255, p(out), 4, 0, None, 0, 0, None,
                                         stream) == -1
    assert lib.udaseg_clahe_lut_u8(p(img), p(st), 32, 1, n, h, w, None, None, None, stream) == -1
    assert lib.udaseg_clahe_lut_u8(p(img), p(st), 48, 1, n, h, w, None, None, p(lut), stream) == -1
    assert lib.udaseg_clahe_lut_u8(p(img), p(st), 32, 1, n, 60, w, None, None, p(lut), stream) == -1
    assert lib.udaseg_strong_aug_clahe_u8(p(img), p(st), 1, n, 60, w, None, m255, r255, p(out), 4, 0, 0, p(lut), stream) == -1
    assert b"multiples of 8" in lib.udaseg_last_error()
    assert lib.udaseg_train_aug_clahe_u8(p(img), None, p(tt), n, h, 60, None, None, None, 0, m255, r255, p(out), 4, 0, None, 0, 0, p(lut),
                                         stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lut == 9).all())


# ---------------------------------------------------------------------------------------------------------------- trainers
def _first_seed(draw, count):
    """The first seed whose generator puts a record on CLAHE within ``count`` consecutive draws."""
    for seed in range(1000):
        g = torch.Generator().manual_seed(seed)
        if any(bool(draw(g).clahe.any()) for _ in range(count)):
            return seed
    raise AssertionError("no seed draws CLAHE")


def test_clahe_keyword_reaches_the_draws_of_loader_and_trainer(D):
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    from uda_aerial_semantic_segmentation_research_amd.unsupervised_trainer import UnsupervisedTrainer
    n, h, w = 2, 64, 64
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    batch = (torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)),
             torch.from_numpy(rng.integers(0, 23, (n, h, w), dtype=np.uint8)))
    seed = _first_seed(lambda g: D.draw_training_params(n, h, w, g, clahe=True), 1)
    assert D.draw_training_params(n, h, w, torch.Generator().manual_seed(seed), clahe=True).clahe.any()
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23)
    tr = SegmentationTrainer(net, dev)
    loader = D.DeviceAugmentedLoader([batch], generator=torch.Generator().manual_seed(seed), clahe=True)
    want = D.train_batch(batch[0], batch[1], None, torch.Generator().manual_seed(seed), clahe=True)
    (x, m), = list(loader)
    loader.generator.manual_seed(seed)
    assert torch.equal(x, want[0]) and torch.equal(m, want[1])
    plain = D.train_batch(batch[0], batch[1], None, torch.Generator().manual_seed(seed))
    assert not torch.equal(x, plain[0]) and torch.equal(m, plain[1])       # the stage ran; the mask never sees it
    loss = tr.train_epoch(loader, FusedAdam(net.parameters(), lr=1e-4), 1)
    assert math.isfinite(loss) and all(torch.isfinite(p).all() for p in net.parameters())
    # phase 3
    useed = _first_seed(lambda g: D.draw_strong_params(n, h, w, g, clahe=True), 2)
    ut = UnsupervisedTrainer(Unet("resnet18", encoder_weights=None, in_channels=3, classes=23), dev, rampup_length=1, seed=useed)
    g = torch.Generator().manual_seed(useed)
    assert any(D.draw_strong_params(n, h, w, g, clahe=True).clahe.any() for _ in range(2))
    opt = FusedAdam(ut.model.parameters(), lr=1e-4)
    out = ut.finetune_step(batch[0], opt, 1, clahe=True)
    assert not out["skipped"] and math.isfinite(float(out["total"]))
    assert all(torch.isfinite(p).all() for p in ut.model.parameters())
    ut2 = UnsupervisedTrainer(Unet("resnet18", encoder_weights=None, in_channels=3, classes=23), dev, rampup_length=1, seed=useed,
                              clahe=True)
    v1, v2, _ = ut2._views(batch[0], None)
    g = torch.Generator().manual_seed(useed)
    pa, pb = D.draw_strong_params(n, h, w, g, clahe=True), D.draw_strong_params(n, h, w, g, clahe=True)
    wa, wb = D.strong_views(batch[0], pa, pb)
    assert torch.equal(v1, wa) and torch.equal(v2, wb)
