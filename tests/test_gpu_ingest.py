"""Frame ingest on the device (ingest.py / csrc/resize.hip) against the numpy restatement of its definitions
(tests/_resize_ref.py; INTEGRATION.md, "Frame ingest").

The area filter, the nearest mask resize and the mask histogram are integer arithmetic and are compared with ``torch.equal``.
The antialiased bilinear + normalise output is held to the float64 restatement by the bar of tests/test_gpu_train_aug.py and
tests/test_gpu_clahe.py: per sample |kernel - f64| <= max(4 x |f32 - f64|, 2 ulp of fp32 at the output's magnitude), the f32
leg being torch's own CPU fp32 ``interpolate(..., antialias=True)`` followed by the fp32 normalisation; no pixel is left out.
Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import os

import numpy as np
import pytest
import torch

import _resize_ref as R

pytestmark = pytest.mark.gpu

AREA_SHAPES = [(128, 128, 64, 64),          # 2 x 2 blocks: ties
               (96, 144, 32, 48),           # 3 x 3 blocks
               (100, 150, 32, 64),          # fractional on both axes, 450-byte rows
               (37, 53, 32, 32),
               (64, 200, 64, 32),           # one axis is the identity
               (64, 64, 64, 64),
               (50, 70, 1, 1),
               (1100, 40, 1, 8),            # more than 256 whole rows per wave: the 16-bit row sums are flushed
               (1030, 1540, 512, 768)]      # several blocks per destination row, rows past one 1024-byte piece


@pytest.fixture(scope="module")
def G():
    from uda_aerial_semantic_segmentation_research_amd import _lib, ingest
    _lib.require_gpu()
    return ingest


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def noise(n, h, w, seed=0):
    return np.random.default_rng(seed + 31 * h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def label_masks(n, h, w, seed=0):
    """Labels drawn from {0..22, 255}."""
    rng = np.random.default_rng(seed + 17 * h + w)
    return np.append(np.arange(23), 255).astype(np.uint8)[rng.integers(0, 24, (n, h, w))]


# ------------------------------------------------------------------------------------------------------------------ area
@pytest.mark.parametrize("H,W,h,w", AREA_SHAPES)
def test_area_resize_is_exact(G, H, W, h, w):
    src = noise(1, H, W)
    want = R.area_resize(src, h, w)
    got, none = G.resize_frames(torch.from_numpy(src).cuda(), (h, w))
    assert none is None and got.dtype == torch.uint8 and got.shape == (1, h, w, 3) and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    if (H, W) == (h, w):
        assert torch.equal(got.cpu(), torch.from_numpy(src))              # byte for byte
    if (H, W, h, w) == (128, 128, 64, 64):                                # sums of four with remainder 2: half goes up
        s4 = src.reshape(1, 64, 2, 64, 2, 3).astype(np.int64).sum(axis=(2, 4))
        ties = s4 % 4 == 2
        assert ties.any()
        assert np.array_equal(got.cpu().numpy()[ties], (s4[ties] + 2) // 4) and np.array_equal(want, (s4 + 2) // 4)


def test_area_resize_batch_stride_and_host_source(G):
    src = noise(3, 100, 150, seed=5)
    assert not np.array_equal(src[0], src[1])
    want = torch.from_numpy(R.area_resize(src, 32, 64))
    from_dev, _ = G.resize_frames(torch.from_numpy(src).cuda(), (32, 64))
    from_host, _ = G.resize_frames(torch.from_numpy(src), (32, 64))
    from_numpy, _ = G.resize_frames(src, (32, 64))
    assert torch.equal(from_dev.cpu(), want) and torch.equal(from_host, from_dev) and torch.equal(from_numpy, from_dev)


def test_area_resize_accumulators_past_32_bits(G):
    """255 * H * W = 4.49e9 > 2^32: a 32-bit total wraps.  A white frame with noise on every 7th row / 5th column pixel.  One
    pixel in 35 is noise, so a destination cell's mean is 255 - (255 - noise mean) / 35 within about +-0.03 (275 000 pixels per
    cell): with noise uniform in 0..255 that is 251.36 in every cell and the result is constant.  The noise is therefore drawn
    from 10..255 (mean 132.5): the cell means sit at 251.5, the restatement's result holds both 251 and 252, and every one of
    its totals is above 2^32."""
    H, W = 4200, 4196
    assert 255 * H * W > 2 ** 32
    src = np.full((1, H, W, 3), 255, dtype=np.uint8)
    src[:, ::7, ::5] = np.random.default_rng(9).integers(10, 256, src[:, ::7, ::5].shape, dtype=np.uint8)
    want = R.area_resize(src, 8, 8)
    assert want.min() != want.max()
    assert int(R.area_total(src, 8, 8).min()) > 2 ** 32
    got, _ = G.resize_frames(torch.from_numpy(src), (8, 8))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# --------------------------------------------------------------------------------------------------------------- nearest
@pytest.mark.parametrize("H,W,h,w", AREA_SHAPES + [(48, 40, 64, 96)])
def test_nearest_resize_is_exact(G, H, W, h, w):
    m = label_masks(2, H, W)
    assert (m == 255).any()
    want = torch.from_numpy(np.ascontiguousarray(R.nearest_resize(m, h, w)))
    got = G.resize_masks(torch.from_numpy(m).cuda(), (h, w))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    if H >= h and W >= w:                                                 # the pair call: the same masks beside the frames
        f, gm = G.resize_frames(noise(2, H, W), (h, w), m)
        assert torch.equal(gm, got) and f.shape == (2, h, w, 3)


# ------------------------------------------------------------------------------------------------------------- histogram
def test_mask_histogram_and_class_balance(G):
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    m = label_masks(3, 100, 150, seed=3)
    want = R.mask_hist(m)
    hist = torch.zeros((3, 256), dtype=torch.int64, device="cuda")
    K.mask_hist_u8(torch.from_numpy(m).cuda(), hist)
    assert torch.equal(hist.cpu(), torch.from_numpy(want))
    K.mask_hist_u8(torch.from_numpy(m).cuda(), hist)                      # the counters accumulate
    assert torch.equal(hist.cpu(), torch.from_numpy(2 * want))
    const = np.full((1, 512, 512), 7, dtype=np.uint8)                     # a single value takes every count
    hist1 = torch.zeros((1, 256), dtype=torch.int64, device="cuda")
    K.mask_hist_u8(torch.from_numpy(const).cuda(), hist1)
    assert torch.equal(hist1.cpu(), torch.from_numpy(R.mask_hist(const))) and int(hist1[0, 7]) == 512 * 512
    odd = label_masks(2, 37, 53, seed=4)                                  # rows of masks that start off a 16-byte boundary
    hist2 = torch.zeros((2, 256), dtype=torch.int64, device="cuda")
    K.mask_hist_u8(torch.from_numpy(odd).cuda(), hist2)
    assert torch.equal(hist2.cpu(), torch.from_numpy(R.mask_hist(odd)))

    # ClassBalance: masks of two sizes, updated in two calls and out of order
    big = label_masks(2, 64, 96, seed=6)
    big[0, :48] = 3                                                       # one class dominates a mask
    cb = G.ClassBalance(5)
    cb.update([4, 0, 2], torch.from_numpy(m).cuda())
    cb.update([3, 1], big)
    masks = [m[1], big[1], m[2], big[0], m[0]]
    assert cb.class_stats() == R.class_stats(masks)
    wts, ref = cb.sample_weights(), R.sample_weights(masks)
    assert wts.dtype == np.float64 and np.all(np.abs(wts - ref) <= 1e-12 * ref)
    s = cb.sampler([0, 3, 4])
    sub = ref[[0, 3, 4]] / ref[[0, 3, 4]].sum()
    assert s.num_samples == 3 and s.replacement and np.all(np.abs(s.weights.numpy() - sub) <= 1e-12 * sub)
    assert len(cb.sampler()) == 5
    with pytest.raises(ValueError, match="never updated"):
        fresh = G.ClassBalance(3)
        fresh.update([0, 2], big)
        fresh.sample_weights()


# ------------------------------------------------------------------------------------ antialiased bilinear + normalise
def _padded(x, cpad):
    n, _, h, w = x.shape
    return x.as_strided((n, h, w, cpad), (h * w * cpad, w * cpad, cpad, 1), x.storage_offset())


@pytest.mark.parametrize("H,W,h,w", [(100, 150, 32, 64), (37, 53, 32, 32), (300, 500, 256, 256), (48, 40, 64, 96),
                                     (64, 6000, 8, 8)])     # 1500 source pixels under one destination pixel: five pieces per block
def test_resize_normalized_against_float64(G, H, W, h, w):
    n = 2
    src = noise(n, H, W, seed=11)
    d64 = R.normalize(R.aa_resize(src, h, w), np.float64)
    t32 = torch.nn.functional.interpolate(torch.from_numpy(src).permute(0, 3, 1, 2).float(), size=(h, w), mode="bilinear",
                                          antialias=True, align_corners=False).permute(0, 2, 3, 1).numpy()
    d32 = R.normalize(t32, np.float32)
    assert d32.dtype == np.float32
    x32 = G.resize_normalized(torch.from_numpy(src).cuda(), (h, w))
    assert x32.shape == (n, 3, h, w) and x32.dtype == torch.float32
    assert not _padded(x32, 4)[..., 3:].any()
    got = x32.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    failures = []
    for i in range(n):
        dev = np.abs(d32[i].astype(np.float64) - d64[i]).max()
        bar = max(4 * dev, 2 * float(np.spacing(np.float32(np.abs(d64[i]).max()))))
        err = np.abs(got[i] - d64[i]).max()
        _log(f"ingest aa {H}x{W}->{h}x{w} sample {i}  kernel-vs-f64 {err:.3e}  f32-vs-f64 {dev:.3e}  bar {bar:.3e}")
        if not err <= bar:
            failures.append((i, err, dev, bar))
    assert not failures, failures
    x16 = G.resize_normalized(torch.from_numpy(src).cuda(), (h, w), dtype=torch.bfloat16)
    assert x16.dtype == torch.bfloat16 and torch.equal(x16, x32.to(torch.bfloat16))
    assert not _padded(x16, 8)[..., 3:].any()
    assert torch.equal(G.resize_normalized(src, (h, w)), x32)             # a host source gives the same bytes


def test_resize_normalized_at_equal_size_is_prepare_batch(G):
    from uda_aerial_semantic_segmentation_research_amd import data
    src = torch.from_numpy(noise(2, 64, 64, seed=12)).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        a = G.resize_normalized(src, (64, 64), dtype=dtype)
        b, _ = data.prepare_batch(src, dtype=dtype)
        assert torch.equal(a, b)
        cpad = 8 if dtype == torch.bfloat16 else 4
        assert torch.equal(_padded(a, cpad), _padded(b, cpad))


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_loaders_compose(G):
    from uda_aerial_semantic_segmentation_research_amd import data
    frames, masks = noise(2, 100, 150, seed=13), label_masks(2, 100, 150, seed=13)
    small, small_m = G.resize_frames(frames, (32, 64), masks)
    assert torch.equal(small.cpu(), torch.from_numpy(R.area_resize(frames, 32, 64)))
    loader = data.DeviceAugmentedLoader(G.ResizingLoader([(torch.from_numpy(frames), torch.from_numpy(masks))], (32, 64)),
                                        generator=torch.Generator().manual_seed(21))
    (x, m), = list(loader)
    want_x, want_m = data.train_batch(small, small_m, None, torch.Generator().manual_seed(21))
    assert len(loader) == 1 and torch.equal(x, want_x) and torch.equal(m, want_m)
    plain, = list(G.ResizingLoader([frames], (32, 64)))                   # frames alone, numpy in
    assert torch.equal(plain, small)


def test_predict_mask_resizes_on_request(G):
    from uda_aerial_semantic_segmentation_research_amd.config import Config
    from uda_aerial_semantic_segmentation_research_amd.predict import predict_mask
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(3)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda()
    frame = noise(1, 300, 500, seed=14)[0]
    got = predict_mask(net, frame, resize=True)
    assert got.shape == (23,) + tuple(Config.IMAGE_SIZE)
    want = predict_mask(net, G.resize_normalized(frame[None], tuple(Config.IMAGE_SIZE)))
    assert np.array_equal(got, want)
    with pytest.raises(ValueError, match="Resize is not reproduced"):
        predict_mask(net, noise(1, 128, 256, seed=15)[0])
