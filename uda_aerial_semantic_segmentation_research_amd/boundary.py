"""Label boundary distances on the device: band erosion of masks, boundary weight maps, Boundary IoU and trimap accuracy.

One primitive serves all of it (``csrc/boundary.hip``; ``include/udaseg.h`` states the rule in full and ``tests/_boundary_ref.py``
is its numpy mirror, bit for bit): the exact squared Euclidean distance ``d2`` from every pixel to the nearest *boundary pixel*
of its own image, capped at a radius ``R <= 32``.

    label ``L``        uint8 or int64 ``[N,H,W]`` (``[H,W]`` is taken as ``N = 1``); an int64 value outside ``[0, 255]`` reads as 255.
    void               with ``ignore_index`` (``0..255``) the pixels equal to it; with ``ignore_index=None`` no pixel is void.
    boundary pixel     a pixel with a left, right, upper or lower neighbour INSIDE the same image that has another label, neither of
                       the two void.  The frame's edge is no boundary (``render``'s outline draws the same pixels).
    ``d2``             the smallest ``dy^2 + dx^2`` to a boundary pixel of the image if that is ``<= R^2``, else ``R^2 + 1`` ("far").

What is made of it, each in ONE pass that never writes ``d2`` to memory (``distance2`` alone does):

    ``erode``          a mask with ``void`` within ``R`` pixels of every label boundary: the usual treatment of pseudo-labels, which
                       are least reliable there (``ErodedLoader`` applies it to the batches of ``PseudoLabeler.loader`` /
                       ``OnlineLabeler.loader`` / ``PrototypeLabeler.loader`` / ``mix.MixedLoader``).
    ``weight_map``     ``table[d2]``: any decay with the distance, by default U-Net's ``1 + w0 exp(-d^2 / (2 sigma^2))``
                       (Ronneberger et al. 2015), usable as ``pixel_weight`` of ``SoftCrossEntropyLoss`` / ``PrototypeContrastLoss``.
    ``BoundaryStats``  Boundary IoU per class (Cheng et al., CVPR 2021) and trimap accuracy, accumulated on the device.

Where this differs from Cheng et al.'s code: their band is what ``ceil(R)`` iterations of a 3 x 3 erosion remove (a chessboard
distance to the contour, taken per class mask) and the frame's edge counts as contour; here the band is the pixels of the class
within EUCLIDEAN distance ``R`` of a boundary pixel of the label map, and the frame's edge is no contour -- a region that merely
touches the frame is not "boundary" there.  ``radius_of`` keeps their ``0.02 x diagonal`` default.

CPU tensors raise: there is no CPU path in this build.  Nothing is read back unless stated.
"""
import math

import numpy as np
import torch

from . import _args as A
from . import kernels as K

MAX_RADIUS = 32
DEFAULT_RATIO = 0.02          # Boundary IoU's dilation ratio: the band is 2 % of the image diagonal wide
_SAME = object()              # erode's ignore_index default: the void value itself


# --------------------------------------------------------------------------------------------------------------- host side
def _check_radius(who, radius):
    return A.int_in(who, "radius", radius, 0, MAX_RADIUS)


def radius_of(ratio, h, w):
    """``max(1, round(ratio * sqrt(h^2 + w^2)))``: the band width of an ``h x w`` image at a dilation ratio (Boundary IoU's default
    is ``DEFAULT_RATIO = 0.02``: 14 at 512 x 512).  A width above ``MAX_RADIUS`` raises: the capped transform stops there."""
    if not (h >= 1 and w >= 1) or not ratio > 0:
        raise ValueError(f"radius_of: need ratio > 0 and h, w >= 1, got ratio={ratio} h={h} w={w}")
    r = max(1, int(round(float(ratio) * math.sqrt(float(h) * h + float(w) * w))))
    if r > MAX_RADIUS:
        raise ValueError(f"radius_of: ratio {ratio} of a {h} x {w} image is a radius of {r}, above the limit of {MAX_RADIUS}: "
                         f"use a smaller ratio or evaluate at a lower resolution")
    return r


def table_of(radius, fn, far=0.0, void=0.0):
    """The fp32 ``[R*R + 3]`` lookup table of ``weight_map`` (numpy): ``fn(d2)`` for ``d2 = 0 .. R*R`` (``fn`` takes the float64
    array of SQUARED distances), then ``far`` for the pixels further than ``R`` from every boundary, then ``void`` for the void
    pixels.  Evaluated in float64 and rounded to fp32 once."""
    r = _check_radius("table_of", radius)
    d2 = np.arange(r * r + 1, dtype=np.float64)
    v = np.asarray(fn(d2), dtype=np.float64)
    if v.shape != d2.shape:
        raise ValueError(f"table_of: fn must return one value per squared distance ({d2.shape[0]}), got shape {v.shape}")
    return np.concatenate([v, [float(far), float(void)]]).astype(np.float32)


def unet_table(radius, w0=10.0, sigma=5.0, void_weight=0.0):
    """U-Net's boundary emphasis (Ronneberger et al. 2015, eq. 2, with the distance to the nearest boundary pixel):
    ``1 + w0 * exp(-d2 / (2 sigma^2))`` within ``radius``, 1 beyond it, ``void_weight`` on void pixels."""
    if not sigma > 0:
        raise ValueError(f"unet_table: sigma must be positive, got {sigma}")
    return table_of(radius, lambda d2: 1.0 + float(w0) * np.exp(-d2 / (2.0 * float(sigma) * float(sigma))), far=1.0, void=void_weight)


def summarize(stats, trimap):
    """The measures of ``BoundaryStats.compute`` from its raw counters (numpy, host): ``stats`` int64 ``[C,3]`` (truth band, predicted
    band, both, per class), ``trimap`` int64 ``[2]`` (pixels within the radius of a truth boundary, those of them predicted right).

    ``boundary_iou`` ``[C]`` = ``both / (t + p - both)``, 0 for a class in neither band; ``mean_boundary_iou``: its mean over the
    classes present in either band (NaN without any); ``trimap_accuracy`` (NaN for an empty trimap)."""
    s = np.asarray(stats).astype(np.int64).reshape(-1, 3)
    tm = np.asarray(trimap).astype(np.int64).reshape(2)
    t, p, both = (s[:, k].astype(np.float64) for k in range(3))
    union = t + p - both
    present = union > 0
    iou = np.divide(both, union, out=np.zeros_like(union), where=present)
    return {"boundary_iou": iou, "mean_boundary_iou": float(iou[present].mean()) if present.any() else float("nan"),
            "trimap_accuracy": float(tm[1]) / float(tm[0]) if tm[0] > 0 else float("nan"), "stats": s, "trimap": tm}


# ------------------------------------------------------------------------------------------------------------- device side
def distance2(labels, radius, ignore_index=None, out=None):
    """int32 ``d2`` of every pixel, in the labels' shape: 0 on a boundary pixel, ``radius^2 + 1`` further than ``radius`` from all."""
    lab, single = A.label_maps("distance2", labels)
    r = _check_radius("distance2", radius)
    ign = A.int_in("distance2", "ignore_index", ignore_index, 0, 255, True)
    out = A.out_tensor("distance2", "out", out, lab.shape, torch.int32, lab.device)
    A.on_device(lab.device, K.boundary_d2, lab, r, ign, out)
    return out[0] if single and out.dim() == 3 else out


def _device_table(who, table, r, dev):
    if torch.is_tensor(table) and table.is_cuda:
        if table.dtype != torch.float32 or table.numel() != r * r + 3:
            raise ValueError(f"{who}: a device table must be float32 with radius^2 + 3 = {r * r + 3} entries, got {table.dtype} "
                             f"{tuple(table.shape)}")
        return table.reshape(-1).contiguous()
    arr = np.ascontiguousarray(np.asarray(table.numpy() if torch.is_tensor(table) else table, dtype=np.float32).reshape(-1))
    if arr.shape[0] != r * r + 3:
        raise ValueError(f"{who}: the table needs radius^2 + 3 = {r * r + 3} entries (table_of / unet_table), got {arr.shape[0]}")
    return A.const_table("boundary", arr.tobytes(), arr.copy, dev)      # callers weigh every batch with the same few tables


def weight_map(labels, radius, table=None, w0=10.0, sigma=5.0, ignore_index=None, out=None):
    """fp32 weights in the labels' shape: ``table[d2]``, the last entry on void pixels.  ``table``: None (``unet_table(radius, w0,
    sigma)``), ``table_of``'s array, or a float32 device tensor of ``radius^2 + 3`` entries.  The table's bits are copied.  The result
    is what ``SoftCrossEntropyLoss`` / ``PrototypeContrastLoss`` take as ``pixel_weight``."""
    lab, single = A.label_maps("weight_map", labels)
    r = _check_radius("weight_map", radius)
    ign = A.int_in("weight_map", "ignore_index", ignore_index, 0, 255, True)
    tab = _device_table("weight_map", unet_table(r, w0, sigma) if table is None else table, r, lab.device)
    out = A.out_tensor("weight_map", "out", out, lab.shape, torch.float32, lab.device)
    A.on_device(lab.device, K.boundary_lookup, lab, r, ign, tab, out)
    return out[0] if single and out.dim() == 3 else out


def erode(labels, radius, void=255, ignore_index=_SAME, counts=None, out=None):
    """The uint8 mask with ``void`` on every pixel within ``radius`` of a label boundary (``radius = 0``: on the boundary pixels
    themselves), the labels elsewhere.  ``ignore_index``: by default ``void`` itself, so that a void region is no label of its own --
    its rim makes no boundary and it does not grow; ``None`` makes every value an ordinary label (a void speck then voids the disc
    around it).  ``counts``: an int64 ``[N,2]`` device tensor that ACCUMULATES, per image, the pixels this call voided and the pixels
    that were void already."""
    lab, single = A.label_maps("erode", labels)
    r = _check_radius("erode", radius)
    v = A.int_in("erode", "void", void, 0, 255)
    ign = v if ignore_index is _SAME else A.int_in("erode", "ignore_index", ignore_index, 0, 255, True)
    A.counts_tensor("erode", "counts", counts, (lab.shape[0], 2), lab.device)
    out = A.out_tensor("erode", "out", out, lab.shape, torch.uint8, lab.device)
    A.on_device(lab.device, K.boundary_erode, lab, r, ign, v, out, counts)
    return out[0] if single and out.dim() == 3 else out


class ErodedLoader:
    """Wraps a loader of ``(frames_u8, masks_u8)`` batches -- ``PseudoLabeler.loader``, ``OnlineLabeler.loader``,
    ``PrototypeLabeler.loader``, ``mix.MixedLoader`` -- and yields ``(frames, erode(masks, radius, void))``: the teacher's labels
    without the band around their boundaries, where they are least reliable.  The frames pass through; masks still on the host are
    moved.  ``last_counts``: the int64 ``[N,2]`` device tensor of the latest batch (voided, void before), for logging; nothing is read
    back here."""

    def __init__(self, loader, radius, void=255):
        self.loader = loader
        self.radius = _check_radius("ErodedLoader", radius)
        self.void = A.int_in("ErodedLoader", "void", void, 0, 255)
        self.last_counts = None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch) or len(batch) != 2:
                raise ValueError("ErodedLoader: a batch must be a (frames, masks) pair")
            frames, masks = batch
            if torch.is_tensor(masks) and masks.device.type != "cuda":
                masks = masks.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
            n = 1 if masks.dim() == 2 else int(masks.shape[0])
            counts = torch.zeros((n, 2), dtype=torch.int64, device=masks.device)
            out = erode(masks, self.radius, self.void, counts=counts)
            self.last_counts = counts
            yield frames, out


class BoundaryStats(A.DeviceState):
    """Accumulates the band counters of predictions against truth on the device (``udaseg_boundary_stats``).  ``update`` enqueues
    and does not synchronise; ``compute`` does ONE read-back and returns ``summarize`` of the counters.

    The inner band of class ``c`` in a map is its pixels of class ``c`` within ``radius`` of a boundary pixel of that map; Boundary
    IoU of ``c`` is ``|band_truth(c) & band_pred(c)| / |band_truth(c) | band_pred(c)|`` over everything seen.  With
    ``ignore_index`` the truth's void pixels are void in the prediction too.  Trimap accuracy: the share of the pixels within
    ``radius`` of a truth boundary that are predicted right."""

    def __init__(self, num_classes, radius, ignore_index=None, device=None):
        self.num_classes = A.int_in("BoundaryStats", "num_classes", num_classes, 1, 255)
        self.radius = _check_radius("BoundaryStats", radius)
        self.ignore_index = A.int_in("BoundaryStats", "ignore_index", ignore_index, 0, 255, True)
        self.device = torch.device(device) if device is not None else None
        self.tables = None             # int64 [3 C + 2] on the device: stats [C,3], then trimap [2] (one allocation, one transfer)

    def _allocate(self, device):
        self.tables = torch.zeros(3 * self.num_classes + 2, dtype=torch.int64, device=device)

    def reset(self):
        if self.tables is not None:
            self.tables.zero_()

    def update(self, pred, truth):
        """``pred``: a label map like ``truth`` (uint8 or int64 ``[N,H,W]``), or scores ``[N,C,H,W]`` (logits or probabilities),
        labelled by their first maximum (``udaseg_predict_finish``'s arg-max, at most 32 classes)."""
        who = "BoundaryStats.update"
        if torch.is_tensor(pred) and pred.dim() == 4:
            buf, ldc, n, c, h, w = A.scores_nchw(who, pred, self.num_classes, "pred")
            lab = torch.empty((n, h, w), dtype=torch.int64, device=pred.device)
            A.on_device(pred.device, K.predict_finish, buf, None, n * h * w, c, ldc, lab)
            pred = lab
            if torch.is_tensor(truth) and truth.dim() == 4 and truth.shape[1] == 1:
                truth = truth[:, 0]
        p, _ = A.label_maps(who, pred, "pred")
        t, _ = A.label_maps(who, truth, "truth")
        if p.shape != t.shape:
            raise ValueError(f"{who}: pred {tuple(p.shape)} and truth {tuple(t.shape)} differ in shape")
        if p.dtype != t.dtype:                                      # one dtype for both: the uint8 one is widened (lossless)
            p, t = p.long(), t.long()
        tab = self._ensure(A.same_gpu(who, truth=t, pred=p)).tables
        c3 = 3 * self.num_classes
        A.on_device(t.device, K.boundary_stats, p, t, self.radius, self.num_classes, self.ignore_index, tab[:c3], tab[c3:])
        return self

    def compute(self):
        """``summarize`` of the accumulated counters: ``boundary_iou`` [C], ``mean_boundary_iou``, ``trimap_accuracy`` and the raw
        ``stats`` [C,3] / ``trimap`` [2].  ONE device->host transfer of ``3 C + 2`` counters."""
        t = self._ensure().tables.cpu().numpy()
        c3 = 3 * self.num_classes
        return summarize(t[:c3].reshape(-1, 3), t[c3:])


def evaluate(model, loader, num_classes, device, radius=None, ignore_index=None):
    """Eval-mode pass over ``loader`` (batches of ``(images, masks)``) in the shape of ``curves.evaluate``: the band counters
    accumulate on the device and are read back ONCE at the end.  ``radius``: None takes ``radius_of(DEFAULT_RATIO, H, W)`` of the
    first batch.  Returns ``BoundaryStats.compute()``'s dict and ``radius``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model runs on the GPU (no CPU path in this build)")
    stats = None
    with A.eval_mode(model), torch.no_grad():
        for images, masks in loader:
            images = images.to(device)
            masks = masks.to(device)
            if masks.dtype not in (torch.uint8, torch.int64):
                masks = masks.long()
            outputs = model(images)
            if stats is None:
                r = radius_of(DEFAULT_RATIO, outputs.shape[2], outputs.shape[3]) if radius is None else radius
                stats = BoundaryStats(num_classes, r, ignore_index, device)
            stats.update(outputs, masks)
    if stats is None:
        raise ValueError("evaluate: the loader is empty")
    res = stats.compute()
    res["radius"] = stats.radius
    return res
