"""Class-balanced pseudo-labels of unlabelled target frames on the device: self-training, the third standard way to use
target-domain frames next to the discriminator (phase 2) and the consistency loss (phase 3).  An EXTENSION: the reference has no
counterpart (its phase 3 is consistency only).  The method is CBST's (Zou et al. 2018): predict labels on target
frames, keep only the confident pixels, with the confidence threshold set PER CLASS so that rare classes are not starved by the
confident majority, and train the segmenter on the kept pixels with the rest marked void.

With torch this is ``softmax`` -> ``max`` -> one ``quantile`` (a sort) per class -> ``where``: several passes over the logits.
Here ONE HIP pass makes a ``[C, B]`` table of 64-bit counters (``udaseg_conf_hist``), a tiny kernel turns it into one threshold bin
per class (``udaseg_pseudo_thresholds``) and one more pass writes the uint8 masks (``udaseg_pseudo_labels``); no sort, no host copy
of the logits, and the thresholds never leave the device.

The confidence and its grid (part of the public contract; ONE device function serves the histogram and the labelling)
    For a pixel with logits ``z`` (``probs=False``): ``c^`` = the first maximum of ``z``, ``m = z[c^]``,
    ``S = sum_c expf(z_c - m)`` in fp32 (four partial sums, channel ``c`` in sum ``c % 4``, folded as ``(s0 + s1) + (s2 + s3)``),
    confidence ``p = 1 / S`` (the softmax probability of the winner).
    For a pixel with probabilities ``q`` (``probs=True``, ``predict_large(..., return_probs=True)``'s view): ``c^`` = the first
    maximum of ``q``, ``p = q[c^]``.
    Grid: ``B`` in {256, 512, 1024, 2048, 4096} uniform bins over ``[0, 1]``, ``bin(p) = min(floor(p * B), B - 1)``; the edges
    ``k / B`` are exact in fp32 and ``p == 1`` lands in bin ``B - 1``.
    A pixel whose ``p`` is not finite (a NaN logit, a ``+inf`` logit, all logits ``-inf``) or, with ``probs``, lies outside
    ``[0, 1]`` or stands beside a NaN in any of the ``C`` channels is NON-FINITE: it is counted in no table cell, is always
    labelled void and is counted on its own.

    ``table[c][b]``: the finite pixels predicted as ``c`` whose confidence is in bin ``b``.  It ACCUMULATES across ``update`` calls.

The thresholds, per class ``c``, in integers and IEEE float64 only (``thresholds_from_hist`` is the host mirror, bit for bit)
    ``n_c = sum_b table[c][b]``; ``need_c = int(ceil(portion_c * float(n_c)))``; ``k_c`` = the largest ``k`` in ``[0, B - 1]`` with
    ``sum_{b >= k} table[c][b] >= need_c`` (``B - 1`` for an empty class); then ``k_c <- min(max(k_c, k_floor), k_cap)`` with
    ``k_floor = bin(floor)``, ``k_cap = bin(cap)`` under the same rule in float64.  A pixel predicted as ``c`` is kept iff
    ``bin(p) >= k_c``, i.e. iff ``p >= k_c / B``: at least the ``portion_c`` most confident pixels of the class (whole bins), never
    one below ``floor``, and -- CBST's rule -- no class has to be more confident than ``cap`` to be kept.

Use, a batch at a time (re-fitting every few epochs as the model improves is left to the caller)::

    labeler = PseudoLabeler(model, num_classes=23, portion=0.2)
    labeler.fit(target_u8_loader)                  # uint8 [N,H,W,3] batches, as ingest.ResizingLoader yields them
    SegmentationTrainer(model, dev, criterion=CrossEntropyLoss(ignore_index=255)).train_epoch(
        data.DeviceAugmentedLoader(labeler.loader(target_u8_loader), generator=g), opt, epoch)

and for one large frame: ``labels_u8, probs = labeler.label_large(frame_u8, tile=512, overlap=0.25)`` after
``labeler.fit_large(frames)``.
"""
import numpy as np
import torch

from . import _args as A
from . import _lib
from . import kernels as K

BINS = 1024
SUPPORTED_BINS = (256, 512, 1024, 2048, 4096)


def _check_bins(bins):
    return int(A.choice("pseudo", "bins", bins, SUPPORTED_BINS))


def _check_classes(num_classes):
    return A.int_in("pseudo", "num_classes", num_classes, 1, 32)


def _check_void(void, num_classes):
    return A.int_in("pseudo", "void", void, num_classes, 255)             # above the classes, inside uint8


def bin_edges(bins=BINS):
    """Lower edge of every bin, ``k / B`` in float64 (exact)."""
    return np.arange(_check_bins(bins), dtype=np.float64) / float(bins)


def bin_of(p, bins=BINS):
    """``min(floor(p * B), B - 1)`` in float64: the bin of a probability (the rule ``floor`` and ``cap`` are turned into bins by)."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"a probability in [0, 1] is needed, got {p}")
    return int(min(np.floor(np.float64(p) * np.float64(bins)), bins - 1))


def _portions(portion, classes):
    """-> float64 [classes], every value checked to lie in (0, 1]."""
    v = np.asarray(portion, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(classes, float(v))
    if v.shape != (classes,):
        raise ValueError(f"portion must be a float or {classes} floats, got shape {v.shape}")
    if not np.all((v > 0.0) & (v <= 1.0)):
        raise ValueError(f"portion must lie in (0, 1], got {portion}")
    return v


def _floor_cap_bins(floor, cap, bins):
    if not 0.0 <= float(floor) <= 1.0:
        raise ValueError(f"floor must lie in [0, 1], got {floor}")
    if not 0.0 <= float(cap) <= 1.0:
        raise ValueError(f"cap must lie in [0, 1], got {cap}")
    if float(floor) > float(cap):
        raise ValueError(f"floor must not exceed cap, got floor={floor} cap={cap}")
    return bin_of(floor, bins), bin_of(cap, bins)


def thresholds_from_hist(hist, portion, floor=0.0, cap=1.0):
    """The threshold arithmetic on the host in numpy int64 / float64 (what ``udaseg_pseudo_thresholds`` does on the device).
    ``hist``: ``[C, B]`` integer table (numpy or tensor); ``portion``: a float or ``C`` floats in ``(0, 1]``.
    Returns ``(thr_bins [C] int32, support [C] int64)``.  Needs no GPU."""
    if torch.is_tensor(hist):
        hist = hist.detach().cpu().numpy()
    hist = np.asarray(hist).astype(np.int64)
    if hist.ndim != 2:
        raise ValueError(f"hist must be a [C, B] table, got shape {hist.shape}")
    C, B = hist.shape
    _check_bins(B)
    por = _portions(portion, C)
    k_floor, k_cap = _floor_cap_bins(floor, cap, B)
    support = hist.sum(axis=1)
    thr = np.zeros(C, dtype=np.int32)
    for c in range(C):
        need = int(np.ceil(por[c] * np.float64(support[c])))
        tail = np.cumsum(hist[c, ::-1])[::-1]                    # tail[k] = sum_{b >= k}
        ok = np.nonzero(tail >= need)[0]
        k = int(ok[-1]) if len(ok) else 0
        thr[c] = min(max(k, k_floor), k_cap)
    return thr, support


class ConfidenceHistogram(A.DeviceState):
    """Accumulates the per-class confidence table of ``[N,C,H,W]`` logits (or probabilities) on the device.  ``update`` enqueues
    one kernel and does not synchronise; ``thresholds`` enqueues the finishing kernel and returns a device tensor."""

    def __init__(self, num_classes, bins=BINS, device=None):
        self.num_classes, self.bins = _check_classes(num_classes), _check_bins(bins)
        self.device = torch.device(device) if device is not None else None
        self._buf = None                # [C * B + 1] int64 on the device: the table, then the non-finite count (one allocation)
        self.support = None             # [C] int64 on the device, written by thresholds()

    def _allocate(self, device):
        self._buf = torch.zeros(self.num_classes * self.bins + 1, dtype=torch.int64, device=device)

    @property
    def table(self):
        """``[C, B]`` int64 on the device."""
        return self._ensure()._buf[:-1].view(self.num_classes, self.bins)

    @property
    def nonfinite(self):
        """``[1]`` int64 on the device: the pixels that are in no cell."""
        return self._ensure()._buf[-1:]

    def reset(self):
        if self._buf is not None:
            self._buf.zero_()

    def update(self, outputs, probs=False):
        buf, ldc, n, _, h, w = A.scores_nchw("ConfidenceHistogram.update", outputs, self.num_classes)
        self._ensure(outputs.device)
        A.on_device(outputs.device, K.conf_hist, buf, n * h * w, self.num_classes, ldc, probs, self.bins, self.table, self.nonfinite)
        return self

    def thresholds(self, portion, floor=0.0, cap=0.9):
        """Device int32 ``[C]`` threshold bins of the accumulated table (no host sync); ``self.support`` gets ``n_c``."""
        por = _portions(portion, self.num_classes)
        k_floor, k_cap = _floor_cap_bins(floor, cap, self.bins)
        t = self.table
        thr = torch.empty(self.num_classes, dtype=torch.int32, device=t.device)
        self.support = torch.empty(self.num_classes, dtype=torch.int64, device=t.device)
        A.on_device(t.device, K.pseudo_thresholds, t, self.num_classes, self.bins, torch.from_numpy(por).to(t.device), k_floor, k_cap,
                    thr, self.support)
        return thr


def pseudo_labels(outputs, thr_bins, void=255, probs=False, return_confidence=False, counts=None, bins=BINS):
    """uint8 ``[N,H,W]`` masks on the device of ``[N,C,H,W]`` logits (or probabilities): the winning class where its confidence
    bin reaches ``thr_bins[class]``, ``void`` elsewhere and at every non-finite pixel.  ``thr_bins``: device int32 ``[C]`` made
    with the same ``bins``.  ``counts``: optional device int64 ``[C + 2]`` to accumulate kept-per-class, void, non-finite into.
    With ``return_confidence`` also the fp32 ``[N,H,W]`` confidence (0 at a non-finite pixel).  No host sync."""
    bins = _check_bins(bins)
    n, classes, h, w = A.scores_shape("pseudo_labels", outputs)
    void = _check_void(void, classes)
    if not torch.is_tensor(thr_bins) or thr_bins.dtype != torch.int32 or tuple(thr_bins.shape) != (classes,):
        raise ValueError(f"pseudo_labels: thr_bins must be an int32 [{classes}] tensor")
    A.counts_tensor("pseudo_labels", "counts", counts, (classes + 2,), outputs.device)
    dev = A.same_gpu("pseudo_labels", scores=outputs, thr_bins=thr_bins)
    buf, ldc = A.padded_nhwc(outputs.detach())
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    conf = torch.empty((n, h, w), dtype=torch.float32, device=dev) if return_confidence else None
    if counts is None:
        counts = torch.zeros(classes + 2, dtype=torch.int64, device=dev)
    A.on_device(dev, K.pseudo_labels, buf, n * h * w, classes, ldc, probs, bins, thr_bins, void, labels, conf, counts)
    return (labels, conf) if return_confidence else labels


def confidence_share(outputs, tau, probs=False, return_counts=False):
    """Device fp32 ``[N]``: per image, the share of pixels whose winner confidence (the module docstring's, the one the table is
    made of) is ``>= tau`` -- the per-image weight ``q_i`` of DACS and DAFormer, made without a host read and exact: integer
    counters, ``share[i] = float32(float64(above[i]) / (H * W))``.  Non-finite pixels are in no count.  ``outputs``: ``[N,C,H,W]``
    logits, or probabilities with ``probs``.  With ``return_counts`` also the device int64 ``[N]`` counts ``above`` and ``nonfinite``."""
    tau = A.number("confidence_share", "tau", tau, 0.0, 1.0)
    buf, ldc, n, classes, h, w = A.scores_nchw("confidence_share", outputs)
    counts = torch.empty((2, n), dtype=torch.int64, device=outputs.device)
    share = torch.empty(n, dtype=torch.float32, device=outputs.device)
    A.on_device(outputs.device, K.conf_share, buf, n, h * w, classes, ldc, probs, tau, counts[0], counts[1], share)
    return (share, counts[0], counts[1]) if return_counts else share


class _LabelledLoader:
    """``(frames_u8, masks_u8)`` device batches of a loader of uint8 frames: what ``data.DeviceAugmentedLoader`` wraps."""

    def __init__(self, labeler, loader):
        self.labeler, self.loader = labeler, loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for frames in self.loader:
            frames = _frames_of(frames)
            dev = self.labeler.device
            frames = frames.to(dev, non_blocking=True)
            yield frames, self.labeler.label(frames)


def _frames_of(batch):
    """A loader may yield frames alone or ``(frames, ...)`` tuples; the frames come first."""
    return batch if torch.is_tensor(batch) else batch[0]


class PseudoLabeler:
    """Fits per-class confidence thresholds on target frames with ``model`` and labels frames with them (module docstring).

    ``portion``: the share of each class's predicted pixels to keep at least, a float or ``num_classes`` floats in ``(0, 1]``;
    ``floor`` / ``cap``: probabilities in ``[0, 1]``, ``floor <= cap``; ``bins``: the grid; ``void``: the label of the pixels that
    are not kept (``num_classes <= void <= 255``; 255 is what ``CrossEntropyLoss(ignore_index=255)`` and ``data.train_batch``
    carry); ``dtype``: the model's input dtype (None: its ``compute_dtype``).  The thresholds describe the model AS FITTED:
    re-fit every few epochs of self-training; that schedule is the caller's."""

    def __init__(self, model, num_classes, portion=0.2, floor=0.0, cap=0.9, bins=BINS, void=255, dtype=None):
        self.num_classes, self.bins = _check_classes(num_classes), _check_bins(bins)
        self.portion = _portions(portion, self.num_classes)
        _floor_cap_bins(floor, cap, self.bins)
        self.floor, self.cap = float(floor), float(cap)
        self.void = _check_void(void, self.num_classes)
        if dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be None, torch.float32 or torch.bfloat16, got {dtype}")
        self.model = model
        self.dtype = dtype
        self.hist = ConfidenceHistogram(self.num_classes, self.bins)
        self.thr_bins = None            # device int32 [C] after fit / fit_large
        self._report = None

    @property
    def device(self):
        return A.model_device(self.model, "PseudoLabeler", 32)

    def _forward(self, frames_u8):
        from .data import prepare_batch
        dtype = self.dtype or getattr(self.model, "compute_dtype", torch.float32)
        images, _ = prepare_batch(frames_u8, None, None, dtype)              # Normalize, D4 code 0
        return self.model(images)

    def _eval_forward(self, frames_u8):
        """One eval-mode, no-grad forward; the model's training flag is restored."""
        with A.eval_mode(self.model), torch.no_grad():
            return self._forward(frames_u8)

    def _finish_fit(self):
        """The thresholds from the accumulated table, and the ONE host read of a fit: thresholds, supports, kept counts and the
        non-finite count in one transfer."""
        self.thr_bins = self.hist.thresholds(self.portion, self.floor, self.cap)
        t = self.hist.table
        above = torch.arange(self.bins, device=t.device)[None, :] >= self.thr_bins[:, None]
        kept = (t * above).sum(dim=1)
        packed = torch.cat([self.thr_bins.long(), self.hist.support, kept, self.hist.nonfinite]).cpu().numpy()
        C = self.num_classes
        thr, support, kept, bad = packed[:C], packed[C:2 * C], packed[2 * C:3 * C], int(packed[3 * C])
        total = int(support.sum()) + bad
        self._report = {
            "threshold": (thr.astype(np.float64) / self.bins).tolist(),
            "support": [int(v) for v in support],
            "kept": [int(v) for v in kept],
            "kept_share": [float(k) / float(s) if s else 0.0 for k, s in zip(kept, support)],
            "void_share": 1.0 - float(kept.sum()) / total if total else 0.0,
            "nonfinite": bad,
        }
        return self

    def fit(self, loader_u8):
        """Eval-mode pass over a loader of uint8 ``[N,H,W,3]`` target batches: accumulates the table, sets ``self.thr_bins``
        (device) and the report (one host read).  The model's training flag is restored."""
        _lib.require_gpu()
        self.hist.reset()
        frames_seen = 0
        with A.eval_mode(self.model), torch.no_grad():
            for batch in loader_u8:
                frames = _frames_of(batch)
                self.hist.update(self._forward(frames))
                frames_seen += int(frames.shape[0])
        if not frames_seen:
            raise ValueError("PseudoLabeler.fit: the loader yielded no frames")
        return self._finish_fit()

    def _need_fit(self, who):
        if self.thr_bins is None:
            raise RuntimeError(f"PseudoLabeler.{who}: call fit (or fit_large) first")

    def label(self, frames_u8):
        """uint8 ``[N,H,W]`` masks (device) of uint8 ``[N,H,W,3]`` frames under the fitted thresholds; eval-mode forward, the
        model's training flag restored."""
        self._need_fit("label")
        return pseudo_labels(self._eval_forward(frames_u8), self.thr_bins, self.void, bins=self.bins)

    def loader(self, loader_u8):
        """Iterable (with ``__len__``) of ``(frames_u8, masks_u8)`` device batches: wrap it in ``data.DeviceAugmentedLoader``."""
        self._need_fit("loader")
        return _LabelledLoader(self, loader_u8)

    def fit_large(self, frames, **predict_large_kwargs):
        """The histogram pass for large frames: ``predict_large(..., return_probs=True)`` per uint8 ``[H,W,3]`` frame, the table
        updated with ``probs=True``.  (``predict_large`` leaves the model in eval mode; the flag is restored here.)"""
        from .predict import predict_large
        self.hist.reset()
        n = 0
        with A.eval_mode(self.model):
            for frame in frames:
                _, probs = predict_large(self.model, frame, return_probs=True, **predict_large_kwargs)
                self.hist.update(probs, probs=True)
                n += 1
        if not n:
            raise ValueError("PseudoLabeler.fit_large: no frames")
        return self._finish_fit()

    def label_large(self, frame_u8, **predict_large_kwargs):
        """-> ``(labels uint8 [H,W], probs)``: ``predict_large``'s blended probabilities labelled with ``probs=True``."""
        from .predict import predict_large
        self._need_fit("label_large")
        with A.eval_mode(self.model):
            _, probs = predict_large(self.model, frame_u8, return_probs=True, **predict_large_kwargs)
        return pseudo_labels(probs, self.thr_bins, self.void, probs=True, bins=self.bins)[0], probs

    def report(self):
        """Plain dict of the last fit, for a trainer to log: per class ``threshold`` (the probability ``k_c / B``), ``support``
        (pixels predicted as the class), ``kept``, ``kept_share``; overall ``void_share`` and ``nonfinite``."""
        self._need_fit("report")
        return dict(self._report)
