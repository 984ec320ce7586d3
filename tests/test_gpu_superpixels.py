"""GPU checks of the superpixel module (superpixels.py, csrc/superpixels.hip) and of regions.label_ids against the numpy mirror
tests/_superpixels_ref.py.  Every product is integers (the mean table is compared through an int32 view), so every comparison is
for equality, bit for bit.  tests/test_superpixels_host.py vets the mirror and the inputs: the fragment-heavy cases really absorb
components over chains of 8 and more, and every superpixel of every case is 4-connected.

No new kernel caps its grid (one thread per pixel, one block per tile of cells), so there is no case beyond a cap; the resolve and
finish launches udaseg_regions_label_i32 shares with udaseg_regions_label are capped and tests/test_gpu_regions.py covers them."""
import numpy as np
import pytest
import torch

import _superpixels_ref as R

pytestmark = pytest.mark.gpu
CASES = sorted(R.CASES)
PRE = 7                                            # what every counter holds before a call: they accumulate


@pytest.fixture(scope="module")
def SP():
    from uda_aerial_semantic_segmentation_research_amd import _lib, superpixels
    _lib.require_gpu()
    return superpixels


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                              # a copy: the shared references are read-only


def _min_areas(name):
    S = R.CASES[name][3]
    return (0, S * S // 4)


@pytest.mark.parametrize("name", CASES)
def test_slic_matches_the_mirror(SP, name):
    frames, _, S = R.case(name)
    n, h, w = frames.shape[:3]
    for min_area in _min_areas(name):
        ids, cen, counts, _ = R.reference(name, min_area)
        got_counts = torch.full((n, 4), PRE, dtype=torch.int64, device="cuda")
        seg = SP.slic(_dev(frames), S, R.COMPACTNESS, R.ITERATIONS, min_area, counts=got_counts)
        assert seg.grid == R.grid_of(h, w, S) and seg.step == S
        assert seg.ids.dtype == torch.int32 and seg.centres.dtype == torch.int32
        assert np.array_equal(_np(seg.centres), cen), (name, min_area)
        assert np.array_equal(_np(seg.ids), ids), (name, min_area)
        assert np.array_equal(_np(got_counts) - PRE, counts), (name, min_area, _np(got_counts) - PRE, counts)
        again = SP.slic(_dev(frames), S, R.COMPACTNESS, R.ITERATIONS, min_area)          # the same bits on a second call
        assert torch.equal(again.ids, seg.ids) and torch.equal(again.centres, seg.centres)
    single = SP.slic(_dev(frames[0]), S, R.COMPACTNESS, R.ITERATIONS)                   # [H,W,3] is N = 1
    ids0 = R.reference(name)[0][0]
    assert tuple(single.ids.shape) == (h, w) and np.array_equal(_np(single.ids), ids0)


@pytest.mark.parametrize("name", ["ragged_pair", "random", "max_step"])
def test_assign_and_connect_alone_match_the_mirror(SP, name):
    """One iteration from the mirror's centres of T - 1 iterations, with its labels; the connect step on the mirror's labels, in
    place and out of place, with sentinels around the output."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    frames, _, S = R.case(name)
    n, h, w = frames.shape[:3]
    ids, cen, counts, info = R.reference(name)
    before = R.slic(frames, S, R.COMPACTNESS, R.ITERATIONS - 1)[1] if R.ITERATIONS > 1 else None
    c = _dev(before)
    labels = torch.full((n, h, w), -5, dtype=torch.int32, device="cuda")
    K.superpixel_assign(_dev(frames), S, R.COMPACTNESS, c, labels)
    assert np.array_equal(_np(c), cen) and np.array_equal(_np(labels), info["labels"])
    c2 = _dev(before)
    K.superpixel_assign(_dev(frames), S, R.COMPACTNESS, c2, None)
    assert torch.equal(c2, c)
    raw = torch.full((n * h * w + 512,), -77, dtype=torch.int32, device="cuda")
    out = raw[256:256 + n * h * w].view(n, h, w)
    got_counts = torch.full((n, 4), PRE, dtype=torch.int64, device="cuda")
    K.superpixel_connect(labels, S, 0, out, got_counts)
    assert np.array_equal(_np(out), ids) and np.array_equal(_np(got_counts) - PRE, counts)
    assert bool((raw[:256] == -77).all()) and bool((raw[256 + n * h * w:] == -77).all())
    K.superpixel_connect(labels, S, 0, labels)
    assert np.array_equal(_np(labels), ids)


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_vote_matches_the_mirror(SP, name, i64):
    frames, _, S = R.case(name)
    n, h, w = frames.shape[:3]
    ids = R.reference(name)[0]
    gh, gw = R.grid_of(h, w, S)
    seg = SP.Segments(_dev(ids), (gh, gw), S, None)
    classes = 5
    masks = R.masks_for(name, classes)
    m = _dev(masks.astype(np.int64) if i64 else masks)
    for share, cover, ign, void in ((0.0, 0.0, 255, None), (0.6, 0.0, 255, 254), (1.0, 0.0, 255, None), (0.0, 0.5, 255, None),
                                    (0.5, 1.0, 255, None), (0.0, 0.0, None, 250)):
        want, want_counts = R.vote(ids, masks, classes, ign, share, cover, void, K=gh * gw)
        counts = torch.full((n, 3), PRE, dtype=torch.int64, device="cuda")
        raw = torch.full((n * h * w + 512,), 99, dtype=torch.uint8, device="cuda")
        out = raw[256:256 + n * h * w].view(n, h, w)
        got = SP.vote(seg, m, classes, ign, share, cover, void, counts=counts, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(_np(got), want), (name, share, cover, ign)
        assert np.array_equal(_np(counts) - PRE, want_counts), (name, share, cover, ign, _np(counts) - PRE, want_counts)
        assert bool((raw[:256] == 99).all()) and bool((raw[256 + n * h * w:] == 99).all())
    want, _ = R.vote(ids, masks, classes, 255, 0.0, 0.0, None, K=gh * gw)
    assert np.array_equal(_np(SP.vote(seg.ids, m, classes)), want)                      # a bare id map: the table of the finest grid
    assert np.array_equal(_np(SP.snap(seg.ids[0], m[0], classes)), want[0])             # [H,W]


@pytest.mark.parametrize("name", sorted(R.ROUND_TRIP))
def test_vote_returns_the_regions_of_a_clean_frame(SP, name):
    n, h, w, S, seeds = R.ROUND_TRIP[name]
    frames, regions = R.voronoi(n, h, w, seeds)
    seg = SP.slic(_dev(frames), S, R.COMPACTNESS, R.ITERATIONS)
    counts = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    out = SP.vote(seg, _dev(regions), seeds, counts=counts)
    assert np.array_equal(_np(out), regions) and int(counts.sum()) == 0


@pytest.mark.parametrize("name", CASES)
def test_mean_select_and_outline_match_the_mirror(SP, name):
    frames, _, S = R.case(name)
    n, h, w = frames.shape[:3]
    ids = R.reference(name)[0]
    gh, gw = R.grid_of(h, w, S)
    K = gh * gw
    seg = SP.Segments(_dev(ids), (gh, gw), S, None)
    values = R.values_for(name).copy()
    values[ids == ids[:, -1:, -1:]] = -1.0                                             # the last pixel's superpixel counts nothing
    want = R.mean(values, ids, K)
    got = SP.mean(_dev(values), seg)
    assert tuple(got.shape) == (n, gh, gw)
    assert np.array_equal(_np(got).reshape(n, K).view(np.int32), want.view(np.int32)), name
    assert (want == -1).any() and ((want >= 0).any() or K == 1)
    for budget in (1, 3, 0.25):
        items = budget if isinstance(budget, int) else max(1, int(np.floor(budget * K)))
        want_mask, want_counts = R.select(values, ids, K, items)
        mask, counts = SP.select(_dev(values), seg, budget)
        assert np.array_equal(_np(mask), want_mask) and np.array_equal(_np(counts), want_counts), (name, budget)
    into = np.zeros((n, h, w), dtype=np.uint8)
    into[:, ::3, ::2] = 4
    want_mask, want_counts = R.select(values, ids, K, 2, into)
    dev_into = _dev(into)
    mask, counts = SP.select(_dev(values), seg, 2, into=dev_into)
    assert mask.data_ptr() == dev_into.data_ptr() and np.array_equal(_np(mask), want_mask) and np.array_equal(_np(counts), want_counts)
    assert np.array_equal(_np(SP.outline(seg)), R.outline(ids))
    assert np.array_equal(_np(SP.outline(seg.ids[0])), R.outline(ids)[0])


@pytest.mark.parametrize("name", ["fragments", "random", "ragged_pair", "one_cluster"])
def test_label_ids_matches_the_mirror(SP, name):
    """regions.label_ids on the labels BEFORE the connect step (thousands of components over 3 x 4 tiles of the labelling in the
    fragments case: two merge levels), with negative pixels void, against the mirror's union-find."""
    from uda_aerial_semantic_segmentation_research_amd import regions as G
    info = R.reference(name)[3]
    lab = info["labels"].astype(np.int32).copy()
    lab[:, ::7, ::5] = -3                                                              # void pixels cut components apart
    lab[:, -1, -1] = 1 << 20                                                           # a value no uint8 map can hold
    n, h, w = lab.shape
    want = np.stack([R.components(np.where(lab[i] < 0, -1 - np.arange(h * w).reshape(h, w), lab[i])) for i in range(n)])
    want = np.where(lab < 0, -1, want)
    area = np.stack([np.bincount(want[i][want[i] >= 0], minlength=h * w)[np.maximum(want[i], 0)] for i in range(n)])
    area = np.where(lab < 0, 0, area)
    ids, got_area = G.label_ids(_dev(lab), return_area=True)
    assert ids.dtype == torch.int32 and np.array_equal(_np(ids), want) and np.array_equal(_np(got_area), area)
    assert np.array_equal(_np(G.label_ids(_dev(lab))), want)
    assert np.array_equal(_np(G.label_ids(_dev(lab[0]))), want[0])
    # 8-connectivity joins at least as much: the same partition or a coarser one, and the ids of a constant map are all 0
    ids8 = _np(G.label_ids(_dev(lab), connectivity=8))
    assert (ids8 <= want).all() and ((ids8 < 0) == (lab < 0)).all()
    assert int(G.label_ids(torch.full((1, 70, 130), 9, dtype=torch.int32, device="cuda")).abs().sum()) == 0
