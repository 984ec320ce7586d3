"""Host side of the frame ingest (ingest.py, tests/_resize_ref.py), no GPU: the numpy restatement is held to brute force and to
torch's own float64 results, the tap tables ``ingest.aa_table`` hands the kernel to the restatement, ``ClassBalance``'s
arithmetic to a hand-computed case, and every refusal of ``ingest.py`` is reached before a device is asked for."""
import ctypes

import numpy as np
import pytest
import torch

import _resize_ref as R


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.fixture(scope="module")
def G():
    from uda_aerial_semantic_segmentation_research_amd import ingest
    return ingest


def test_area_restatement_equals_dense_weights():
    src = _noise((2, 100, 150, 3), 1)
    assert np.array_equal(R.area_resize(src, 32, 64), R.area_resize_dense(src, 32, 64))
    assert (R.box_weights(100, 32).sum(axis=1) == 100).all() and R.box_weights(100, 32).max() == 32


@pytest.mark.parametrize("H,W,fy,fx", [(128, 128, 2, 2), (96, 144, 3, 3), (64, 200, 1, 5), (64, 64, 1, 1)])
def test_area_restatement_at_integer_factors_is_the_rounded_block_mean(H, W, fy, fx):
    src = _noise((1, H, W, 3), 2)
    blocks = src.reshape(1, H // fy, fy, W // fx, fx, 3).astype(np.float64).mean(axis=(2, 4))
    assert np.array_equal(R.area_resize(src, H // fy, W // fx), np.floor(blocks + 0.5).astype(np.uint8))


@pytest.mark.parametrize("shape,size", R.AA_SHAPES)
def test_antialiased_restatement_matches_torch_float64(G, shape, size):
    (H, W), (h, w) = shape, size
    src = _noise((2, H, W, 3), 3)
    want = torch.nn.functional.interpolate(torch.from_numpy(src).permute(0, 3, 1, 2).double(), size=(h, w), mode="bilinear",
                                           antialias=True, align_corners=False).permute(0, 2, 3, 1).numpy()
    assert np.abs(R.aa_resize(src, h, w) - want).max() <= 1e-10
    # the tables the kernel gets: the restatement's rows rounded to fp32, zero weights past a row's end
    for L, l in ((H, h), (W, w)):
        start, wts = G.aa_table(L, l)
        assert start.dtype == np.int32 and wts.dtype == np.float32 and wts.shape[0] == l and start.min() >= 0
        dense = np.zeros((l, L + wts.shape[1]), dtype=np.float32)
        for i in range(l):
            dense[i, start[i]:start[i] + wts.shape[1]] = wts[i]
        assert np.array_equal(dense[:, :L], R.aa_matrix(L, l).astype(np.float32)) and not dense[:, L:].any()
    if (H, W) == (h, w):
        assert np.array_equal(G.aa_table(H, h)[1], np.tile(np.float32([1, 0]), (h, 1)))


@pytest.mark.parametrize("L,l", R.AXIS_PAIRS + [(40, 96), (48, 64)])
def test_nearest_index_matches_torch(L, l):
    src = torch.arange(L, dtype=torch.float64).reshape(1, 1, 1, L)
    want = torch.nn.functional.interpolate(src, size=(1, l), mode="nearest").reshape(-1).long().numpy()
    assert np.array_equal(R.nearest_index(L, l), want)


def test_class_balance_arithmetic_by_hand(G):
    """Three masks of four pixels: A = {0,0,0,1}, B = {1,1,2,2}, C = {0,255,255,255}.  stats = {0: 4, 1: 3, 2: 2, 255: 3},
    total 12; raw weights A = 3/4*3 + 1/4*4 = 13/4, B = 1/2*4 + 1/2*6 = 5, C = 1/4*3 + 3/4*4 = 15/4; sum 12."""
    masks = np.array([[0, 0, 0, 1], [1, 1, 2, 2], [0, 255, 255, 255]], dtype=np.uint8).reshape(3, 2, 2)
    want = np.array([13 / 4, 5, 15 / 4]) / 12
    hist = R.mask_hist(masks)
    assert np.allclose(G.balance_weights(hist), want * 12, rtol=1e-15)
    assert np.allclose(R.sample_weights(masks), want, rtol=1e-15)
    cb = G.ClassBalance(3)
    cb.load_counts(hist)
    assert cb.class_stats() == {0: 4, 1: 3, 2: 2, 255: 3} == R.class_stats(masks)
    assert np.allclose(cb.sample_weights(), want, rtol=1e-15) and abs(cb.sample_weights().sum() - 1) < 1e-15
    s = cb.sampler([0, 2])
    assert isinstance(s, torch.utils.data.WeightedRandomSampler) and s.num_samples == 2 and s.replacement
    assert np.allclose(s.weights.numpy(), np.array([13, 15]) / 28, rtol=1e-15)
    assert len(cb.sampler()) == 3
    assert all(0 <= i < 2 for i in s)


def test_refusals_are_reached_without_a_device(G):
    frames = torch.zeros((2, 20, 30, 3), dtype=torch.uint8)
    masks = torch.zeros((2, 20, 30), dtype=torch.uint8)
    with pytest.raises(ValueError, match="bilinear"):             # an enlargement in area mode names the other mode
        G.resize_frames(frames, (21, 30))
    with pytest.raises(ValueError, match="bilinear"):
        G.resize_frames(frames, (20, 31))
    for bad in (frames.float(), frames[0], frames[..., :2], np.zeros((2, 20, 30, 3), dtype=np.int16), "frames", None):
        with pytest.raises(ValueError):
            G.resize_frames(bad, (10, 10))
        with pytest.raises(ValueError):
            G.resize_normalized(bad, (10, 10))
    for size in ((0, 10), (10, 0), (-1, 4), (10,), 10, (2.5, 4), (4, 4, 4), None):
        with pytest.raises(ValueError):
            G.resize_frames(frames, size)
        with pytest.raises(ValueError):
            G.resize_normalized(frames, size)
        with pytest.raises(ValueError):
            G.resize_masks(masks, size)
        with pytest.raises(ValueError):
            G.ResizingLoader([frames], size)
    for bad in (masks[:1], masks[:, :10], masks.long(), masks[..., None].expand(2, 20, 30, 3)):
        with pytest.raises(ValueError):                           # masks must match the frames
            G.resize_frames(frames, (10, 10), bad)
    with pytest.raises(ValueError):
        G.resize_normalized(frames, (10, 10), dtype=torch.float16)
    with pytest.raises(ValueError):
        G.resize_masks(frames, (10, 10))
    # class balance
    for bad in (0, -3, 2.5, None):
        with pytest.raises(ValueError):
            G.ClassBalance(bad)
    cb = G.ClassBalance(3)
    for idx, m in (([0], masks), ([0, 0], masks), ([0, 3], masks), ([-1, 0], masks), ([0, 1], masks.float()), ([0, 1], frames)):
        with pytest.raises(ValueError):
            cb.update(idx, m)
    with pytest.raises(ValueError):
        cb.load_counts(np.zeros((2, 256), dtype=np.int64))
    hist = np.zeros((3, 256), dtype=np.int64)
    hist[0, 1] = hist[2, 5] = 7
    cb.load_counts(hist)                                          # sample 1 was never updated
    assert cb.class_stats() == {1: 7, 5: 7}
    with pytest.raises(ValueError, match="never updated"):
        cb.sample_weights()
    with pytest.raises(ValueError, match="never updated"):
        cb.sampler([0, 2])
    # the model of the predict_mask(resize=True) path must live on the GPU; a frame that is no [H,W,3] array is refused
    cpu_model = torch.nn.Conv2d(3, 2, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        G.frame_for_model(cpu_model, np.zeros((30, 40, 3), dtype=np.uint8))
    from uda_aerial_semantic_segmentation_research_amd.predict import predict_mask
    with pytest.raises(RuntimeError):
        predict_mask(cpu_model, np.zeros((30, 40, 3), dtype=np.uint8), device="cuda", resize=True)


def test_library_refuses_bad_resize_arguments_before_any_launch():
    """rc -1 and a message, NULL pointers included; the area mode's u32 column sums bound H."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    P = 4096                                                      # any non-null "device pointer": nothing is dereferenced
    assert lib.udaseg_resize_area_u8(P, 1, 4, 8, 8, 8, P, None) == -1 and b"udaseg_resize_aa_u8" in lib.udaseg_last_error()
    assert lib.udaseg_resize_area_u8(P, 1, 16843010, 1, 1, 1, P, None) == -1 and b"16843009" in lib.udaseg_last_error()
    assert lib.udaseg_resize_area_u8(None, 1, 8, 8, 4, 4, P, None) == -1
    assert lib.udaseg_resize_area_u8(P, 1, 8, 8, 0, 4, P, None) == -1
    assert lib.udaseg_resize_nearest_u8(P, 1, 8, 8, 4, 4, None, None) == -1
    assert lib.udaseg_mask_hist_u8(P, 1, 0, P, None) == -1 and lib.udaseg_mask_hist_u8(P, 1, 64, None, None) == -1
    m = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.udaseg_resize_aa_u8(P, 1, 8, 8, 4, 4, P, P, 0, P, P, 2, m, m, P, 4, 0, None) == -1
    assert lib.udaseg_resize_aa_u8(P, 1, 8, 8, 4, 4, P, P, 2, P, P, 2, m, m, P, 6, 0, None) == -1
    assert lib.udaseg_resize_aa_u8(P, 1, 8, 8, 4, 4, P, None, 2, P, P, 2, m, m, P, 4, 0, None) == -1
