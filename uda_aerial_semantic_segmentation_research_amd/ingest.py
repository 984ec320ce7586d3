"""Device-side frame ingest: decoded uint8 frames and label masks of ANY size -> the uint8 batch at the model's size that
``data.prepare_batch`` / ``data.train_batch`` / ``data.strong_views`` take, the resized and normalised model input of
``predict.predict_mask(resize=True)``, and the class-balance statistics of the label masks.

Upstream does these per sample on the host: ``TargetDataset.__getitem__`` (reference ``src/data/target_dataset.py:46-48``)
shrinks every 4000 x 6000 frame with ``cv2.resize(..., INTER_AREA)``, ``predict_mask`` (``src/models/predict.py:91-98``) ends its
transform with ``Resize(Config.IMAGE_SIZE)``, and ``DroneDataset`` (``src/data/dataset.py:48-111``) reads every full-size mask
twice to build ``class_stats``, ``sample_weights`` and its ``WeightedRandomSampler``.  Here they are HIP kernels
(csrc/resize.hip; definitions in include/udaseg.h and INTEGRATION.md, "Frame ingest"):

* frames: the exact integer area filter (shrinking only), uint8 -> uint8;
* masks: nearest, ``dst[i][j] = src[(i*H)//h][(j*W)//w]``;
* model input: antialiased bilinear (``torch.nn.functional.interpolate(mode="bilinear", antialias=True)``) fused with
  ``A.Normalize``, written as the channel-padded NHWC buffer the stem convolution reads;
* mask histograms ``[N,256]`` on the device, the class-balance formulas on the host from one read-back.

**Sizes are ``(height, width)`` everywhere** -- cv2's ``(width, height)`` order of ``cv2.resize(img, dsize)`` is NOT kept.
Inputs may be host or device tensors or numpy arrays (copied once, asynchronously).  No CPU path.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib
from . import kernels as K
from .config import Config
from .data import IMAGENET_MEAN, IMAGENET_STD, _model_input, normalize_constants


def _size(who, size):
    try:
        h, w = size
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be (height, width), got {size!r}") from None
    return A.int_in(who, "size (height, width)", h, 1), A.int_in(who, "size (height, width)", w, 1)


def _u8(who, what, x, trailing):
    """``x`` as a uint8 torch tensor ``[N, H, W] + trailing`` (numpy arrays are wrapped, not copied)."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise ValueError(f"{who}: {what} must be uint8, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 3 + len(trailing) or tuple(x.shape[3:]) != trailing:
        raise ValueError(f"{who}: {what} must be uint8 [N,H,W{',3' if trailing else ''}], got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if min(x.shape[:3]) < 1:
        raise ValueError(f"{who}: {what} is empty: {tuple(x.shape)}")
    return x


def _device(x):
    return x.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True).contiguous()


def aa_table(length, out_length):
    """One axis of the antialiased bilinear filter for ``length`` -> ``out_length``: (start int32 ``[l]``, weights fp32
    ``[l, taps]``), destination index ``i`` reading source ``start[i] .. start[i] + taps - 1`` (rows shorter than ``taps`` are
    padded with zero weights).  ``scale = L/l``, ``support = max(scale, 1)``, ``c = scale*(i + 0.5)``,
    ``lo = max(0, int(c - support + 0.5))``, ``hi = min(L, int(c + support + 0.5))``, ``weight_j = max(0, 1 - |(j - c + 0.5) /
    support|)`` for ``j`` in ``[lo, hi)`` divided by their sum -- in float64, rounded to fp32 once."""
    L, l = int(length), int(out_length)
    scale = L / l
    support = max(scale, 1.0)
    c = scale * (np.arange(l, dtype=np.float64) + 0.5)
    lo = np.maximum(0, (c - support + 0.5).astype(np.int64))
    hi = np.minimum(L, (c + support + 0.5).astype(np.int64))
    taps = int((hi - lo).max())
    j = lo[:, None] + np.arange(taps)[None, :]
    wts = np.maximum(0.0, 1.0 - np.abs((j - c[:, None] + 0.5) / support))
    wts[j >= hi[:, None]] = 0.0
    wts /= wts.sum(axis=1, keepdims=True)
    return lo.astype(np.int32), wts.astype(np.float32)


def resize_frames(images_u8, size, masks_u8=None):
    """images_u8 ``[N,H,W,3]`` uint8, ``size = (h, w)`` with ``h <= H`` and ``w <= W``, masks_u8 ``[N,H,W]`` uint8 or None
    -> ``(uint8 [N,h,w,3], uint8 [N,h,w] or None)`` on the device: exactly what ``prepare_batch`` / ``train_batch`` /
    ``strong_views`` take.  Frames go through the exact area filter (per channel the box-weighted mean in integers, rounded
    half up: what ``cv2.resize(INTER_AREA)`` computes in fp32, expected within one grey level of it), masks through nearest
    (``src[(i*H)//h][(j*W)//w]``, labels unchanged, any ratio).  ``size`` is (height, width), not cv2's (width, height)."""
    who = "resize_frames"
    h, w = _size(who, size)
    img = _u8(who, "images", images_u8, (3,))
    n, H, W, _ = img.shape
    if h > H or w > W:
        raise ValueError(f"{who}: {H}x{W} -> {h}x{w} enlarges an axis; the area filter only shrinks -- use the bilinear mode "
                         f"(resize_normalized)")
    msk = None
    if masks_u8 is not None:
        msk = _u8(who, "masks", masks_u8, ())
        if tuple(msk.shape) != (n, H, W):
            raise ValueError(f"{who}: masks must be uint8 [{n},{H},{W}] like the frames, got {tuple(msk.shape)}")
    _lib.require_gpu()
    img = _device(img)
    msk = None if msk is None else _device(msk)
    out = torch.empty((n, h, w, 3), device=img.device, dtype=torch.uint8)
    A.on_device(img.device, K.resize_area_u8, img, out)
    out_m = None
    if msk is not None:
        out_m = torch.empty((n, h, w), device=img.device, dtype=torch.uint8)
        A.on_device(img.device, K.resize_nearest_u8, msk, out_m)
    return out, out_m


def resize_masks(masks_u8, size):
    """masks_u8 ``[N,H,W]`` uint8 -> uint8 ``[N,h,w]`` on the device by nearest, any ratio (``resize_frames``' mask half alone)."""
    who = "resize_masks"
    h, w = _size(who, size)
    msk = _u8(who, "masks", masks_u8, ())
    _lib.require_gpu()
    msk = _device(msk)
    out = torch.empty((msk.shape[0], h, w), device=msk.device, dtype=torch.uint8)
    A.on_device(msk.device, K.resize_nearest_u8, msk, out)
    return out


def _aa_tables(H, W, h, w, dev):
    """((start, weights) of the rows, (start, weights) of the columns) on the device, kept (``_args.const_table``)."""
    return tuple(A.const_table("ingest", (L, l), lambda: aa_table(L, l), dev) for L, l in ((H, h), (W, w)))


def resize_normalized(images_u8, size, dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0):
    """images_u8 ``[N,H,W,3]`` uint8, ``size = (h, w)`` (any ratio, enlargements included) -> the ``[N,3,h,w]``-shaped view of the
    channel-padded NHWC model input in ``dtype``, as ``prepare_batch`` hands it out: antialiased bilinear resampling
    (``aa_table``; fp32 on the 0..255 scale) followed by ``A.Normalize``'s ``(v - 255*mean) * (1 / (255*std))``.  The reference
    normalises first and resizes second; the two agree up to rounding because the weights of a pixel sum to 1.  At the
    source's own size the result equals ``prepare_batch``'s bit for bit."""
    who = "resize_normalized"
    h, w = _size(who, size)
    img = _u8(who, "images", images_u8, (3,))
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: dtype must be torch.float32 or torch.bfloat16")
    n, H, W, _ = img.shape
    _lib.require_gpu()
    img = _device(img)
    ty, tx = _aa_tables(H, W, h, w, img.device)
    cpad = 8 if dtype == torch.bfloat16 else 4
    out = torch.empty((n, h, w, cpad), device=img.device, dtype=dtype)
    m255, r255 = normalize_constants(mean, std, max_pixel_value)
    A.on_device(img.device, K.resize_aa_u8, img, ty, tx, m255, r255, out)
    return _model_input(out)


def frame_for_model(model, frame_u8, size=None):
    """One decoded frame ``[H,W,3]`` uint8 of any size -> ``model``'s input at ``size`` (default ``Config.IMAGE_SIZE``) in the
    model's compute dtype, through ``resize_normalized``: the ``Resize`` + ``Normalize`` tail of the reference's ``predict_mask``.
    The input is made on the model's own device."""
    dev = A.model_device(model, "frame_for_model")
    if isinstance(frame_u8, np.ndarray) and frame_u8.ndim == 3:
        frame_u8 = frame_u8[None]
    elif torch.is_tensor(frame_u8) and frame_u8.dim() == 3:
        frame_u8 = frame_u8.unsqueeze(0)
    else:
        raise ValueError(f"frame_for_model: the frame must be uint8 [H,W,3], got {tuple(getattr(frame_u8, 'shape', ()))}")
    return A.on_device(dev, resize_normalized, frame_u8, tuple(Config.IMAGE_SIZE) if size is None else size,
                       getattr(model, "compute_dtype", torch.float32))


class ResizingLoader:
    """Wraps a loader of uint8 frames ``[N,H,W,3]`` -- or of ``(frames, masks [N,H,W])`` pairs -- of any size and yields
    ``resize_frames``' output in the same structure: uint8 batches at ``size = (height, width)`` on the device.  So
    ``DeviceAugmentedLoader(ResizingLoader(loader, size))`` and ``UnsupervisedTrainer.train(ResizingLoader(loader, size), ...)``
    work as they are.  The reference's ``TargetDataset`` default corresponds to ``size=(256, 256)``."""

    def __init__(self, loader, size=(256, 256)):
        self.loader, self.size = loader, _size("ResizingLoader", size)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch) or isinstance(batch, np.ndarray):
                yield resize_frames(batch, self.size)[0]
            else:
                images, masks = batch
                yield resize_frames(images, self.size, masks)


def balance_weights(hist):
    """The reference's sample weights from a ``[N,256]`` table of per-mask value counts: per mask
    ``sum_c (count_c / size) * (total / stats_c)`` with ``size`` the mask's pixels, ``stats_c`` the count of value ``c`` over all
    masks and ``total`` their sum; float64, not yet normalised."""
    hist = np.asarray(hist, dtype=np.int64)
    stats = hist.sum(axis=0)
    total = float(stats.sum())
    size = hist.sum(axis=1).astype(np.float64)
    present = stats > 0
    inv = np.zeros(256, dtype=np.float64)
    inv[present] = total / stats[present].astype(np.float64)
    return ((hist.astype(np.float64) / size[:, None]) * inv[None, :]).sum(axis=1)


class ClassBalance:
    """Class-balanced sampling for a dataset of ``num_samples`` label masks (``DroneDataset``'s ``class_stats``,
    ``sample_weights`` and ``get_sampler``), with the mask reads replaced by a device histogram: ``update`` batches of masks of
    any size as they are decoded, then ask for the statistics -- one read-back of the ``[N,256]`` table."""

    def __init__(self, num_samples):
        self.num_samples = A.int_in("ClassBalance", "num_samples", num_samples, 1)
        self._seen = np.zeros(self.num_samples, dtype=bool)
        self._hist = None                                      # int64 [N,256] on the device, made by the first update
        self._host = None                                      # its read-back, dropped by every update

    def update(self, indices, masks_u8):
        """Counts the pixels of ``masks_u8`` ``[B,H,W]`` uint8 (host or device, any size) into the rows ``indices`` (B distinct
        dataset indices).  A sample updated twice is counted twice."""
        msk = _u8("ClassBalance.update", "masks", masks_u8, ())
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size != msk.shape[0] or len(set(idx.tolist())) != idx.size:
            raise ValueError(f"ClassBalance.update: {msk.shape[0]} masks need as many distinct indices, got {idx.tolist()}")
        if idx.min() < 0 or idx.max() >= self.num_samples:
            raise ValueError(f"ClassBalance.update: indices must lie in 0..{self.num_samples - 1}, got {idx.tolist()}")
        _lib.require_gpu()
        msk = _device(msk)
        if self._hist is None:
            self._hist = torch.zeros((self.num_samples, 256), device=msk.device, dtype=torch.int64)
        rows = torch.zeros((idx.size, 256), device=msk.device, dtype=torch.int64)
        A.on_device(msk.device, K.mask_hist_u8, msk, rows)
        self._hist.index_add_(0, torch.from_numpy(idx).to(msk.device), rows)
        self._seen[idx] = True
        self._host = None

    def load_counts(self, hist):
        """Takes a finished ``[num_samples,256]`` table of counts (as ``counts()`` returns it) in place of the updates.  A row
        counts as updated when it holds at least one pixel; an all-zero row is a sample never updated."""
        hist = np.asarray(hist)
        if hist.shape != (self.num_samples, 256) or not np.issubdtype(hist.dtype, np.integer) or (hist < 0).any():
            raise ValueError(f"ClassBalance.load_counts: need non-negative integers [{self.num_samples},256]")
        self._host = hist.astype(np.int64)
        self._hist = None
        self._seen = self._host.sum(axis=1) > 0

    def counts(self):
        """The int64 ``[num_samples,256]`` table on the host (rows of samples never updated are zero)."""
        if self._host is None:
            self._host = (np.zeros((self.num_samples, 256), dtype=np.int64) if self._hist is None
                          else self._hist.cpu().numpy())
        return self._host

    def _require(self, idx):
        missing = idx[~self._seen[idx]]
        if missing.size:
            raise ValueError(f"ClassBalance: {missing.size} sample(s) were never updated (first: {missing[:8].tolist()})")

    def class_stats(self):
        """``{value: pixel count}`` over all updated masks, for the values present."""
        stats = self.counts().sum(axis=0)
        return {int(v): int(stats[v]) for v in np.nonzero(stats)[0]}

    def sample_weights(self):
        """float64 ``[num_samples]``: ``balance_weights`` normalised to sum 1.  Every sample must have been updated."""
        self._require(np.arange(self.num_samples))
        wts = balance_weights(self.counts())
        return wts / wts.sum()

    def sampler(self, indices=None):
        """``torch.utils.data.WeightedRandomSampler`` over ``indices`` (default: all samples): their weights renormalised to sum
        1, ``num_samples = len(indices)``, ``replacement=True``."""
        wts = self.sample_weights()
        if indices is not None:
            wts = wts[np.asarray(indices, dtype=np.int64).reshape(-1)]
        wts = wts / wts.sum()
        return torch.utils.data.WeightedRandomSampler(weights=torch.from_numpy(wts), num_samples=len(wts), replacement=True)


__all__ = ["resize_frames", "resize_masks", "resize_normalized", "frame_for_model", "ResizingLoader", "ClassBalance",
           "balance_weights", "aa_table"]
