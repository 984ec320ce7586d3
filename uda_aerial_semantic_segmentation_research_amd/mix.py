"""Cross-domain class mixing of a source and a target batch on the device: the step a self-training loop takes between
"pseudo-label the target batch" (``pseudo.py``) and "augment and train" (``data.DeviceAugmentedLoader``).  An EXTENSION: the
reference has no counterpart.  The method is DACS's (Tranheden et al. 2021) with ClassMix's selection (Olsson et al. 2021,
PAPERS.md): take half of the classes present in a source mask, paste their pixels -- frame and label -- onto a target frame and
its pseudo-label mask, train on the mixed pair.  Plain pseudo-label training collapses onto the confident majority classes; every
mixed sample carries true source labels for the pasted classes.

With torch this is ``unique`` per image, a host round trip for the class lists, ``randperm`` on the host, ``isin`` and three
``where`` over the frames.  Here it is the existing mask histogram (``udaseg_mask_hist_u8``), one tiny selection kernel
(``udaseg_classmix_select``) and one streaming pass (``udaseg_classmix_u8``); nothing is read back from the device.

The contract (integers only, so every output is exact)

Selection, per source mask ``i``, from the ``[n][256]`` int64 table of ``kernels.mask_hist_u8``:
    ``present`` = the ascending list of ``c`` in ``[0, classes)`` with ``hist[i][c] >= min_pixels`` (``min_pixels >= 1``),
    ``P = len(present)``, ``k = (P + 1) // 2`` (ClassMix's half of the classes, rounded up); ``P == 0`` selects nothing.
    Partial Fisher-Yates, for ``j = 0 .. k-1``: ``r`` = word 0 of Philox4x32-10 with counter ``(j, 0, 0, 0)`` and key
    ``(keys[i][0], keys[i][1])``; ``t = j + ((r * (P - j)) >> 32)`` on the 64-bit product; swap ``present[j]`` and ``present[t]``.
    ``sel[i]`` = the OR of ``1 << present[j]`` for ``j < k``, stored as the bit pattern of an int32 (``classes <= 32``: bit 31 is
    a class).  The keys are drawn on the host from the caller's CPU ``torch.Generator`` exactly as ``data.draw_strong_params``
    draws its noise keys: ``torch.randint(0, 1 << 32, (n, 2), generator=g, dtype=torch.int64)``.
    ``selection_from_hist`` is the host mirror, bit for bit.

Mixing, per sample ``i`` and pixel ``(y, x)``, with ``s = src_mask[i][y][x]``:
    ``m = (s < classes and (sel[i] >> s) & 1) or (boxes given and y0 <= y < y1 and x0 <= x < x1)``;
    ``out_frame`` = the three source bytes if ``m``, else the three target bytes;
    ``out_mask`` = ``s`` if ``m``, else ``tgt_mask[i][y][x]`` -- or ``void`` when no target masks are given, so that only the pasted
    pixels carry labels;
    ``counts[i]`` (int64 ``[n][3]``, ACCUMULATES across calls like every counter table of this library): ``[0]`` pixels with ``m``,
    ``[1]`` pixels without ``m`` whose output label is ``< classes``, ``[2]`` pixels without ``m`` whose output label is
    ``>= classes``.  The three add up to ``h * w`` per call; ``counts[i][1] / (counts[i][1] + counts[i][2])`` is DACS's
    pixel-weight statistic.

Boxes (the CutMix fallback for sources with a single class): int32 ``[n][4]`` of ``(y0, x0, y1, x1)`` with ``0 <= y0 <= y1 <= h``,
    ``0 <= x0 <= x1 <= w``, empty allowed.  ``draw_boxes`` draws them on the host: ``u = torch.rand(n, 4, generator=g,
    dtype=torch.float64)``; area share ``a = lo + u0 * (hi - lo)``; aspect ``r = exp((2 * u1 - 1) * ln 2)``;
    ``bh = min(h, max(1, round(sqrt(a * h * w * r))))``, ``bw = min(w, max(1, round(sqrt(a * h * w / r))))`` (round half to even);
    ``y0 = floor(u2 * (h - bh + 1))``, ``x0 = floor(u3 * (w - bw + 1))``.

Use::

    mixed = mix.MixedLoader(source_loader_u8, labeler.loader(target_loader_u8), num_classes=23, generator=g)
    loader = data.DeviceAugmentedLoader(mixed, generator=g)          # (frames u8, masks u8, 255 = void)
    SegmentationTrainer(model, dev, criterion=CrossEntropyLoss(ignore_index=255)).train_epoch(loader, opt, epoch)
"""
import math

import numpy as np
import torch

from . import _args as A
from . import kernels as K

MODES = ("class", "box", "both")


def _check_classes(num_classes):
    return A.int_in("mix", "num_classes", num_classes, 1, 32)


def _check_void(void, num_classes):
    return A.int_in("mix", "void", void, num_classes, 255)                # above the classes, inside uint8


def _check_min_pixels(min_pixels):
    return A.int_in("mix", "min_pixels", min_pixels, 1)


def _check_share(share):
    return A.pair("mix", "share", share, 0.0, 1.0, lo_open=True)


def _keys_u32(keys, n):
    """``[n, 2]`` keys (int64 values in ``[0, 2^32)`` as drawn, or int32 bit patterns; numpy or tensor) -> uint32 ``[n, 2]``."""
    if torch.is_tensor(keys):
        keys = keys.detach().cpu().numpy()
    keys = np.asarray(keys)
    if keys.dtype.kind not in "iu" or keys.shape != (n, 2):
        raise ValueError(f"keys must be an integer [{n}, 2] table, got dtype {keys.dtype} shape {keys.shape}")
    return (keys.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def _philox_word0(j, k0, k1):
    """Word 0 of Philox4x32-10 with counter ``(j, 0, 0, 0)`` and key ``(k0, k1)`` in Python integers (aug_common.h's rounds)."""
    c0, c1, c2, c3 = j, 0, 0, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def selection_from_hist(hist, num_classes, keys, min_pixels=1):
    """The selection rule on the host (what ``udaseg_classmix_select`` does on the device, bit for bit).  ``hist``: ``[n, 256]``
    integer table (numpy or tensor); ``keys``: ``[n, 2]`` integers.  Returns int32 ``[n]`` (numpy).  Needs no GPU."""
    classes, min_pixels = _check_classes(num_classes), _check_min_pixels(min_pixels)
    if torch.is_tensor(hist):
        hist = hist.detach().cpu().numpy()
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] != 256 or hist.dtype.kind not in "iu":
        raise ValueError(f"hist must be an integer [n, 256] table, got dtype {hist.dtype} shape {hist.shape}")
    n = hist.shape[0]
    keys = _keys_u32(keys, n)
    sel = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        present = [c for c in range(classes) if int(hist[i, c]) >= min_pixels]
        P = len(present)
        bits = 0
        for j in range((P + 1) // 2):
            r = _philox_word0(j, int(keys[i, 0]), int(keys[i, 1]))
            t = j + ((r * (P - j)) >> 32)
            present[j], present[t] = present[t], present[j]
            bits |= 1 << present[j]
        sel[i] = bits
    return sel.view(np.int32)


def decode_selection(sel, num_classes):
    """``sel`` (int32 ``[n]``, numpy or tensor) -> a list of ascending class lists, for logging.  A tensor on the device is read
    back: that is the caller's synchronisation.  Needs no GPU."""
    classes = _check_classes(num_classes)
    if torch.is_tensor(sel):
        sel = sel.detach().cpu().numpy()
    sel = np.asarray(sel)
    if sel.ndim != 1 or sel.dtype.kind not in "iu":
        raise ValueError(f"sel must be an integer [n] vector, got dtype {sel.dtype} shape {sel.shape}")
    return [[c for c in range(classes) if (int(v) >> c) & 1] for v in sel.astype(np.int64) & 0xFFFFFFFF]


def draw_boxes(n, h, w, generator=None, share=(0.25, 0.5)):
    """int32 ``[n, 4]`` host tensor of ``(y0, x0, y1, x1)`` boxes inside an ``h x w`` frame, area share uniform in ``share`` and
    aspect log-uniform in ``[1/2, 2]`` (the module docstring has the rule).  Needs no GPU."""
    lo, hi = _check_share(share)
    for name, v in (("n", n), ("h", h), ("w", w)):
        A.int_in("draw_boxes", name, v, 1)
    u = torch.rand(n, 4, generator=generator, dtype=torch.float64).numpy()
    a = lo + u[:, 0] * (hi - lo)
    r = np.exp((2.0 * u[:, 1] - 1.0) * math.log(2.0))
    bh = np.minimum(h, np.maximum(1, np.rint(np.sqrt(a * h * w * r)))).astype(np.int64)
    bw = np.minimum(w, np.maximum(1, np.rint(np.sqrt(a * h * w / r)))).astype(np.int64)
    y0 = np.floor(u[:, 2] * (h - bh + 1)).astype(np.int64)
    x0 = np.floor(u[:, 3] * (w - bw + 1)).astype(np.int64)
    return torch.from_numpy(np.stack([y0, x0, y0 + bh, x0 + bw], axis=1).astype(np.int32))


def draw_keys(n, generator=None):
    """int32 ``[n, 2]`` host tensor: the bit patterns of ``torch.randint(0, 1 << 32, (n, 2), generator, dtype=int64)``."""
    keys = torch.randint(0, 1 << 32, (n, 2), generator=generator, dtype=torch.int64).numpy()
    return torch.from_numpy(keys.astype(np.uint32).view(np.int32))


def _u8(who, name, t, shape=None, dims=None):
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise ValueError(f"{who}: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {list(shape)}, got {list(t.shape)}")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{who}: {name} must have {dims} dimensions, got shape {list(t.shape)}")
    return t


def _i32(who, name, t, shape):
    if torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == tuple(shape):
        return t
    raise ValueError(f"{who}: {name} must be an int32 {list(shape)} tensor, got {getattr(t, 'dtype', type(t).__name__)} "
                     f"{list(getattr(t, 'shape', ()))}")


def select_classes(src_masks_u8, num_classes, generator=None, min_pixels=1, keys=None):
    """int32 ``[N]`` on the device: the classes to paste of every uint8 ``[N,H,W]`` source mask.  Allocates a zeroed histogram and
    enqueues ``mask_hist_u8`` and the selection kernel; no synchronisation.  ``keys`` (``[N, 2]`` integers) override the draw from
    ``generator`` (a CPU ``torch.Generator``)."""
    classes, min_pixels = _check_classes(num_classes), _check_min_pixels(min_pixels)
    _u8("select_classes", "src_masks", src_masks_u8, dims=3)
    n = int(src_masks_u8.shape[0])
    if src_masks_u8.numel() < 1:
        raise ValueError(f"select_classes: src_masks must be [N,H,W] with N, H, W >= 1, got {list(src_masks_u8.shape)}")
    if keys is None:
        keys = draw_keys(n, generator)
    else:
        keys = torch.from_numpy(_keys_u32(keys, n).view(np.int32))
    dev = A.current_gpu()
    keys = keys.to(dev, non_blocking=True)
    masks = src_masks_u8.to(dev, non_blocking=True).contiguous()
    hist = torch.zeros((n, 256), dtype=torch.int64, device=dev)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    A.on_device(dev, K.mask_hist_u8, masks, hist)
    A.on_device(dev, K.classmix_select, hist, n, classes, min_pixels, keys, sel)
    return sel


def class_mix(src_frames, src_masks, tgt_frames, tgt_masks, sel, boxes=None, num_classes=None, void=255, out=None, counts=None):
    """One streaming pass: ``(frames [N,H,W,3] uint8, masks [N,H,W] uint8, counts [N,3] int64)`` on the device, the source where
    its class is selected by ``sel`` (int32 ``[N]``) or inside the sample's box (``boxes``: int32 ``[N,4]`` or None), the target
    elsewhere.  ``tgt_masks`` may be None: every pixel that is not pasted is labelled ``void``.  Host tensors are moved with one
    asynchronous copy each.  ``out``: a ``(frames, masks)`` pair of contiguous device tensors to write into (rows of a larger
    batch); ``counts``: a device int64 ``[N,3]`` table to accumulate into, None for a fresh zeroed one, False to keep none."""
    who = "class_mix"
    if num_classes is None:
        raise ValueError("class_mix: num_classes is required")
    classes = _check_classes(num_classes)
    void = _check_void(void, classes)
    n, h, w = A.frames_u8(who, src_frames, name="src_frames")
    _u8(who, "tgt_frames", tgt_frames, (n, h, w, 3))
    _u8(who, "src_masks", src_masks, (n, h, w))
    if tgt_masks is not None:
        _u8(who, "tgt_masks", tgt_masks, (n, h, w))
    _i32(who, "sel", sel, (n,))
    if boxes is not None:
        _i32(who, "boxes", boxes, (n, 4))
        if not boxes.is_cuda:                                                # a device table is the caller's word: no read-back
            b = boxes.numpy()
            if not ((0 <= b[:, 0]) & (b[:, 0] <= b[:, 2]) & (b[:, 2] <= h) & (0 <= b[:, 1]) & (b[:, 1] <= b[:, 3]) & (b[:, 3] <= w)).all():
                raise ValueError(f"class_mix: boxes must satisfy 0 <= y0 <= y1 <= {h} and 0 <= x0 <= x1 <= {w}, got {b.tolist()}")
    if n * h * w >= 1 << 31:
        raise ValueError(f"class_mix: N*H*W must stay below 2^31, got {n * h * w}")
    dev = A.current_gpu()
    mv = lambda t: None if t is None else t.to(dev, non_blocking=True).contiguous()      # noqa: E731
    src_frames, src_masks, tgt_frames, tgt_masks, sel, boxes = (mv(t) for t in (src_frames, src_masks, tgt_frames, tgt_masks, sel, boxes))
    if out is None:
        frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        masks = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    else:
        try:
            frames, masks = out
        except (TypeError, ValueError):
            raise ValueError("class_mix: out must be a (frames, masks) pair of tensors") from None
        _u8(who, "out frames", frames, (n, h, w, 3))
        _u8(who, "out masks", masks, (n, h, w))
        if not (frames.is_cuda and masks.is_cuda and frames.is_contiguous() and masks.is_contiguous()):
            raise ValueError("class_mix: out must be contiguous tensors on the GPU")
    if counts is None:
        counts = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    elif counts is False:
        counts = None
    else:
        A.counts_tensor(who, "counts", counts, (n, 3), dev)
    A.on_device(dev, K.classmix_u8, src_frames, src_masks, tgt_frames, tgt_masks, sel, boxes, n, h, w, classes, void, frames, masks, counts)
    return frames, masks, counts


class MixedLoader:
    """Zips a source loader of uint8 ``(frames [N,H,W,3], masks [N,H,W])`` batches with a target loader of ``(frames, masks)``
    batches (``PseudoLabeler.loader``) or of frames alone, and yields ``(frames_u8, masks_u8)`` device batches, ``void`` where no
    label is known: what ``data.DeviceAugmentedLoader`` wraps.  Its length is the shorter loader's.  A pair of batches of different
    sizes is mixed over its first ``min(n_s, n_t)`` samples; different ``H, W`` raise ``ValueError``.

    ``mode``: ``"class"`` pastes the selected classes, ``"box"`` a random box (CutMix), ``"both"`` their union.  With
    ``include_source`` (DACS's batch) a batch is the ``n_s`` source samples followed by the mixed samples: one allocation, the
    kernel writes its part.  Per batch the ``generator`` (a CPU ``torch.Generator``) is consumed in a fixed order: first the keys
    (``draw_keys``; modes ``"class"`` and ``"both"``), then the boxes (``draw_boxes`` with ``share``; modes ``"box"`` and
    ``"both"``).  ``last_selection`` (int32 ``[n]``) and ``last_counts`` (int64 ``[n,3]``) are the device tensors of the latest
    batch, for logging; nothing is read back here."""

    def __init__(self, source_loader, target_loader, num_classes, generator=None, mode="class", include_source=True, void=255,
                 min_pixels=1, share=(0.25, 0.5)):
        self.num_classes = _check_classes(num_classes)
        self.void = _check_void(void, self.num_classes)
        self.min_pixels = _check_min_pixels(min_pixels)
        self.share = _check_share(share)
        self.mode = A.choice("MixedLoader", "mode", mode, MODES)
        self.source_loader, self.target_loader = source_loader, target_loader
        self.generator, self.include_source = generator, bool(include_source)
        self.last_selection = self.last_counts = None

    def __len__(self):
        return min(len(self.source_loader), len(self.target_loader))

    def __iter__(self):
        dev = A.current_gpu()
        for source, target in zip(self.source_loader, self.target_loader):
            if torch.is_tensor(source) or len(source) != 2:
                raise ValueError("MixedLoader: a source batch must be a (frames, masks) pair")
            s_frames, s_masks = source
            if torch.is_tensor(target):
                t_frames, t_masks = target, None
            else:
                t_frames, t_masks = (target[0], target[1]) if len(target) > 1 else (target[0], None)
            ns, h, w = A.frames_u8("MixedLoader", s_frames, name="source frames")
            nt, ht, wt = A.frames_u8("MixedLoader", t_frames, name="target frames")
            if (h, w) != (ht, wt):
                raise ValueError(f"MixedLoader: source frames are {h} x {w}, target frames {ht} x {wt}")
            _u8("MixedLoader", "source masks", s_masks, (ns, h, w))
            if t_masks is not None:
                _u8("MixedLoader", "target masks", t_masks, (nt, h, w))
            n = min(ns, nt)
            keys = draw_keys(n, self.generator) if self.mode != "box" else None
            boxes = draw_boxes(n, h, w, self.generator, self.share) if self.mode != "class" else None
            s_frames = s_frames.to(dev, non_blocking=True)
            s_masks = s_masks.to(dev, non_blocking=True)
            if keys is None:
                sel = torch.zeros(n, dtype=torch.int32, device=dev)
            else:
                sel = select_classes(s_masks[:n], self.num_classes, min_pixels=self.min_pixels, keys=keys)
            out = None
            if self.include_source:
                frames = torch.empty((ns + n, h, w, 3), dtype=torch.uint8, device=dev)
                masks = torch.empty((ns + n, h, w), dtype=torch.uint8, device=dev)
                frames[:ns].copy_(s_frames)
                masks[:ns].copy_(s_masks)
                out = (frames[ns:], masks[ns:])
            mixed_f, mixed_m, counts = class_mix(s_frames[:n], s_masks[:n], t_frames[:n], None if t_masks is None else t_masks[:n], sel,
                                                 boxes, self.num_classes, self.void, out=out)
            self.last_selection, self.last_counts = sel, counts
            yield (frames, masks) if self.include_source else (mixed_f, mixed_m)
