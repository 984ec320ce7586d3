"""GPU checks of the class-mixing module (mix.py, csrc/mix.hip) against its numpy mirror tests/_mix_ref.py.  Integers only: every
comparison is bit for bit.  Synthetic masks hold classes, 255 and a label in [classes, 255)."""
import numpy as np
import pytest
import torch

import _mix_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    from uda_aerial_semantic_segmentation_research_amd import _lib, mix
    _lib.require_gpu()
    return mix


def _masks(g, n, h, w, classes, stray=True):
    """uint8 [n,h,w]: mostly classes, some 255 and, with ``stray``, some of a label in [classes, 255): classes + 3."""
    m = torch.randint(0, classes, (n, h, w), generator=g, dtype=torch.int64)
    u = torch.rand(n, h, w, generator=g)
    m[u < 0.08] = 255
    if stray:
        m[(u >= 0.08) & (u < 0.14)] = classes + 3
    return m.to(torch.uint8)


def _frames(g, n, h, w):
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def _keys(g, n):
    return torch.randint(0, 1 << 32, (n, 2), generator=g, dtype=torch.int64).numpy()


# ------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("classes", [1, 5, 23, 32])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_selection(M, n, classes):
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    g = torch.Generator().manual_seed(100 * n + classes)
    h, w = 9, 13
    masks = _masks(g, n, h, w, classes)
    masks[0] = 255                                                           # an all-void mask
    if n > 1:
        masks[1] = classes - 1                                               # a one-class mask (bit 31 at 32 classes)
    if n > 2:
        masks[2] = 0
        masks[2, 0, :4] = classes - 1                                        # four pixels of a second class: min_pixels = 5 removes it
    keys = _keys(g, n)
    dev_masks = masks.cuda()
    hist = torch.zeros((n, 256), dtype=torch.int64, device="cuda")
    K.mask_hist_u8(dev_masks, hist)
    assert np.array_equal(hist.cpu().numpy(), R.mask_hist(masks.numpy()))
    for min_pixels in (1, 5):
        sel = M.select_classes(dev_masks, classes, min_pixels=min_pixels, keys=keys)
        assert sel.dtype == torch.int32 and sel.is_cuda and tuple(sel.shape) == (n,)
        got = sel.cpu().numpy()
        assert np.array_equal(got, M.selection_from_hist(hist, classes, keys, min_pixels))
        assert np.array_equal(got, R.select(hist.cpu().numpy(), classes, keys, min_pixels))
        assert got[0] == 0
        if n > 1:
            assert M.decode_selection(got, classes)[1] == [classes - 1]
        if n > 2:                                                            # one of the two classes, or class 0 alone
            third = M.decode_selection(got, classes)[2]
            assert third == [0] if min_pixels == 5 else (len(third) == 1 and third[0] in (0, classes - 1))
    # the generator route draws the keys as documented; host masks are moved
    a = M.select_classes(masks, classes, generator=torch.Generator().manual_seed(7))
    k7 = torch.randint(0, 1 << 32, (n, 2), generator=torch.Generator().manual_seed(7), dtype=torch.int64)
    assert np.array_equal(a.cpu().numpy(), M.selection_from_hist(hist, classes, k7))


# ------------------------------------------------------------------------------------------------------------- mixing
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 16, 16), (2, 17, 31), (4, 64, 48), (1, 257, 129), (2, 128, 128)]


def _case(n, h, w, classes=23, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * h + w)
    src, tgt = _frames(g, n, h, w), _frames(g, n, h, w)
    sm, tm = _masks(g, n, h, w, classes), _masks(g, n, h, w, classes)
    hist = R.mask_hist(sm.numpy())
    sel = torch.from_numpy(R.select(hist, classes, _keys(g, n)))
    boxes = torch.zeros((n, 4), dtype=torch.int32)
    for i in range(n):                                                       # sample 0: empty, sample 1: the full frame, then inner boxes
        if i == 1:
            boxes[i] = torch.tensor([0, 0, h, w])
        elif i > 1:
            y0, x0 = (i * 3) % h, (i * 5) % w
            boxes[i] = torch.tensor([y0, x0, min(h, y0 + h // 2 + 1), min(w, x0 + w // 3 + 1)])
    return src, sm, tgt, tm, sel, boxes


def _check(M, got, want, counts_before=None):
    frames, masks, counts = got
    rf, rm, rc = want
    assert frames.dtype == torch.uint8 and masks.dtype == torch.uint8 and frames.is_cuda and masks.is_cuda
    assert np.array_equal(frames.cpu().numpy(), rf)
    assert np.array_equal(masks.cpu().numpy(), rm)
    if counts is not None:
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), rc if counts_before is None else rc + counts_before)


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_mixing(M, n, h, w):
    classes = 23
    src, sm, tgt, tm, sel, boxes = _case(n, h, w, classes)
    dsrc, dsm, dtgt, dtm = src.cuda(), sm.cuda(), tgt.cuda(), tm.cuda()
    for with_tm in (True, False):
        for with_box in (True, False):
            want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), tm.numpy() if with_tm else None, sel.numpy(),
                         boxes.numpy() if with_box else None, classes, 255)
            assert (want[2].sum(axis=1) == h * w).all()
            args = (dsrc, dsm, dtgt, dtm if with_tm else None, sel, boxes if with_box else None, classes, 255)
            got = M.class_mix(*args)                                         # a fresh zeroed table
            _check(M, got, want)
            assert int(got[2].sum()) == n * h * w
            again = M.class_mix(*args, counts=got[2])                        # accumulates: doubled
            assert again[2] is got[2] and np.array_equal(got[2].cpu().numpy(), 2 * want[2])
            _check(M, (again[0], again[1], None), want)
            none = M.class_mix(*args, counts=False)                          # no table at all
            assert none[2] is None
            _check(M, none, want)
    # host tensors are moved; another void label; a label above the classes in the target counts as void
    want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), None, sel.numpy(), None, classes, 200)
    _check(M, M.class_mix(src, sm, tgt, None, sel, None, classes, 200), want)
    # out: rows of a larger batch
    big_f = torch.full((n + 2, h, w, 3), 7, dtype=torch.uint8, device="cuda")
    big_m = torch.full((n + 2, h, w), 9, dtype=torch.uint8, device="cuda")
    want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), tm.numpy(), sel.numpy(), boxes.numpy(), classes, 255)
    f, m, _ = M.class_mix(dsrc, dsm, dtgt, dtm, sel, boxes, classes, out=(big_f[1:n + 1], big_m[1:n + 1]))
    assert f.data_ptr() == big_f[1].data_ptr() and m.data_ptr() == big_m[1].data_ptr()
    assert np.array_equal(big_f[1:n + 1].cpu().numpy(), want[0]) and np.array_equal(big_m[1:n + 1].cpu().numpy(), want[1])
    assert int((big_f[0] != 7).sum()) == 0 and int((big_f[n + 1] != 7).sum()) == 0
    assert int((big_m[0] != 9).sum()) == 0 and int((big_m[n + 1] != 9).sum()) == 0


@pytest.mark.parametrize("classes", [1, 5, 32])
def test_mixing_class_counts(M, classes):
    n, h, w = 3, 16, 16
    src, sm, tgt, tm, sel, boxes = _case(n, h, w, classes, seed=5)
    want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), tm.numpy(), sel.numpy(), boxes.numpy(), classes, 255)
    _check(M, M.class_mix(src, sm, tgt, tm, sel, boxes, classes), want)
    sm2, tm2 = sm[:, :15, :13].contiguous(), tm[:, :15, :13].contiguous()    # the scalar form
    src2, tgt2 = src[:, :15, :13].contiguous(), tgt[:, :15, :13].contiguous()
    want = R.mix(src2.numpy(), sm2.numpy(), tgt2.numpy(), tm2.numpy(), sel.numpy(), None, classes, 255)
    _check(M, M.class_mix(src2, sm2, tgt2, tm2, sel, None, classes), want)


def _offset_view(t, off=3):
    """The same values as a contiguous view at a storage offset of ``off`` bytes: not 16-byte aligned."""
    flat = torch.empty(t.numel() + 16, dtype=torch.uint8, device="cuda")
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off
    return v


@pytest.mark.parametrize("n,h,w", [(3, 16, 16), (4, 64, 48)])
def test_wide_form_equals_scalar_form(M, n, h, w):
    classes = 23
    src, sm, tgt, tm, sel, boxes = _case(n, h, w, classes, seed=9)
    dev = [t.cuda() for t in (src, sm, tgt, tm)]
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    for with_tm in (True, False):
        for with_box in (True, False):
            b = boxes if with_box else None
            wide = M.class_mix(dev[0], dev[1], dev[2], dev[3] if with_tm else None, sel, b, classes)
            assert wide[0].data_ptr() % 16 == 0 and wide[1].data_ptr() % 16 == 0
            off = [_offset_view(t) for t in dev]
            out = (_offset_view(torch.zeros_like(wide[0])), _offset_view(torch.zeros_like(wide[1])))
            scalar = M.class_mix(off[0], off[1], off[2], off[3] if with_tm else None, sel, b, classes, out=out)
            assert torch.equal(wide[0], scalar[0]) and torch.equal(wide[1], scalar[1]) and torch.equal(wide[2], scalar[2])
            # one misaligned operand is enough to leave the wide form, and changes nothing
            one = M.class_mix(dev[0], off[1], dev[2], dev[3] if with_tm else None, sel, b, classes)
            assert torch.equal(wide[0], one[0]) and torch.equal(wide[1], one[1]) and torch.equal(wide[2], one[2])
            want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), tm.numpy() if with_tm else None, sel.numpy(),
                         None if b is None else b.numpy(), classes)
            _check(M, wide, want)


@pytest.mark.parametrize("n,h,w", [(1200, 64, 128), (300, 41, 43)], ids=["wide", "scalar"])
def test_grid_stride(M, n, h, w):
    """Sizes at which the launch caps its grid (2048 blocks in all), so that a block takes more than one chunk of its sample."""
    classes = 23
    g = torch.Generator().manual_seed(n)
    src, tgt = _frames(g, n, h, w), _frames(g, n, h, w)
    sm, tm = _masks(g, n, h, w, classes), _masks(g, n, h, w, classes)
    sel = torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    want = R.mix(src.numpy(), sm.numpy(), tgt.numpy(), tm.numpy(), sel.numpy(), None, classes)
    _check(M, M.class_mix(src, sm, tgt, tm, sel, None, classes), want)


def test_selection_bit_values(M):
    n, h, w, classes = 2, 17, 31, 23
    src, sm, tgt, tm, _, _ = _case(n, h, w, classes, seed=2)
    zero = torch.zeros(n, dtype=torch.int32)
    f, m, c = M.class_mix(src, sm, tgt, tm, zero, None, classes)
    assert torch.equal(f.cpu(), tgt) and torch.equal(m.cpu(), tm) and int(c[:, 0].sum()) == 0
    ones = torch.full((n,), -1, dtype=torch.int32)
    f, m, c = M.class_mix(src, sm, tgt, tm, ones, None, classes)
    pasted = sm < classes
    assert int(pasted.sum()) not in (0, n * h * w)
    assert torch.equal(f.cpu(), torch.where(pasted[..., None], src, tgt)) and torch.equal(m.cpu(), torch.where(pasted, sm, tm))
    assert torch.equal(c[:, 0].cpu(), pasted.sum(dim=(1, 2)))
    for h2, w2 in ((16, 16), (17, 31)):                                      # both forms
        s2, sm2, t2, tm2 = (t[:, :h2, :w2].contiguous() for t in (src, sm, tgt, tm))
        f, m, _ = M.class_mix(s2, sm2, t2, tm2, ones, None, 32)              # at 32 classes bit 31 is a class, 255 and 254 are not
        p2 = sm2 < 32
        assert torch.equal(f.cpu(), torch.where(p2[..., None], s2, t2)) and torch.equal(m.cpu(), torch.where(p2, sm2, tm2))


# ------------------------------------------------------------------------------------------------------------- the loader
class _Batches:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


@pytest.mark.parametrize("mode", ["class", "box", "both"])
@pytest.mark.parametrize("include_source", [True, False])
def test_mixed_loader(M, include_source, mode):
    classes, h, w = 5, 16, 24
    g = torch.Generator().manual_seed(11)
    source = _Batches([(_frames(g, ns, h, w), _masks(g, ns, h, w, classes)) for ns in (4, 3, 2)])
    with_masks = mode != "box"
    target = _Batches([(_frames(g, nt, h, w), _masks(g, nt, h, w, classes)) if with_masks else _frames(g, nt, h, w) for nt in (3, 4)])
    loader = M.MixedLoader(source, target, classes, generator=torch.Generator().manual_seed(21), mode=mode,
                           include_source=include_source, min_pixels=2, share=(0.2, 0.4))
    assert len(loader) == 2
    ref_g = torch.Generator().manual_seed(21)
    seen = 0
    for (frames, masks), (sf, sm), tb in zip(loader, source.batches, target.batches):
        tf, tm = tb if with_masks else (tb, None)
        ns, nt = sf.shape[0], tf.shape[0]
        n = min(ns, nt)
        keys = _keys(ref_g, n) if mode != "box" else None                    # the documented order: the keys, then the boxes
        boxes = M.draw_boxes(n, h, w, ref_g, (0.2, 0.4)) if mode != "class" else None
        sel = R.select(R.mask_hist(sm[:n].numpy()), classes, keys, 2) if keys is not None else np.zeros(n, dtype=np.int32)
        want = R.mix(sf[:n].numpy(), sm[:n].numpy(), tf[:n].numpy(), None if tm is None else tm[:n].numpy(), sel,
                     None if boxes is None else boxes.numpy(), classes, 255)
        assert frames.is_cuda and masks.is_cuda and frames.dtype == torch.uint8 and masks.dtype == torch.uint8
        lead = ns if include_source else 0
        assert tuple(frames.shape) == (lead + n, h, w, 3) and tuple(masks.shape) == (lead + n, h, w)
        if include_source:
            assert torch.equal(frames[:ns].cpu(), sf) and torch.equal(masks[:ns].cpu(), sm)
        assert np.array_equal(frames[lead:].cpu().numpy(), want[0]) and np.array_equal(masks[lead:].cpu().numpy(), want[1])
        assert np.array_equal(loader.last_selection.cpu().numpy(), sel)
        assert loader.last_counts is not None and np.array_equal(loader.last_counts.cpu().numpy(), want[2])
        seen += 1
    assert seen == 2


# ------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_one_step(M):
    from uda_aerial_semantic_segmentation_research_amd import data as D
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    classes, h, w = 5, 64, 64
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=classes).to("cuda").train()
    source = _Batches([(_frames(g, 2, h, w), _masks(g, 2, h, w, classes, stray=False))])      # classes and void alone: what a
    target = _Batches([(_frames(g, 2, h, w), _masks(g, 2, h, w, classes, stray=False))])      # labelled set and a labeler give
    mixed = M.MixedLoader(source, target, classes, generator=torch.Generator().manual_seed(5))
    before = [p.detach().clone() for p in net.parameters()]
    crit = CrossEntropyLoss(ignore_index=255)
    tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=crit)
    loss = tr.train_epoch(D.DeviceAugmentedLoader(mixed, generator=torch.Generator().manual_seed(9)),
                          FusedAdam(net.parameters(), lr=1e-4), 1)
    assert np.isfinite(loss)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert all(torch.isfinite(p).all() for p in net.parameters())
    counts = mixed.last_counts.cpu().numpy()
    assert (counts.sum(axis=1) == h * w).all() and counts[:, 0].min() > 0
