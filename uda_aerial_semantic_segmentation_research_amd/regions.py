"""Connected components of label maps on the device: region ids and areas, a sieve for small regions, per-class region statistics.

One primitive serves all of it (``csrc/regions.hip``; ``include/udaseg.h`` states the rule in full and ``tests/_regions_ref.py``
is its numpy mirror, compared for equality):

    label ``L``        uint8 or int64 ``[N,H,W]`` (``[H,W]`` is taken as ``N = 1``); an int64 value outside ``[0, 255]`` reads as 255.
    void               with ``ignore_index`` (``0..255``) the pixels equal to it; with ``ignore_index=None`` no pixel is void.
    adjacent           two pixels of one image, neither void, with the same label, that are 4-neighbours (``connectivity=4``) or
                       8-neighbours (``connectivity=8``).  Images never see each other; the frame's edge connects nothing.
    component          a class of the transitive closure of "adjacent".
    ``id``             the smallest ``y * W + x`` over the component's pixels (its first pixel in raster order), -1 on a void pixel:
                       unique, so the same bits on every run.
    ``area``           the number of pixels of the component, 0 on a void pixel.

What is made of it:

    ``label``          the ids, and the areas if asked for.
    ``label_ids``      the same of an int32 map of more than 256 values (a superpixel map): a negative value is void.
    ``sieve``          a mask with ``void`` on every component smaller than ``min_area`` of its class: a teacher's isolated islands
                       of a wrong class are confident inside and survive ``boundary.erode``; this removes them (``SievedLoader``
                       applies it to the batches of ``PseudoLabeler.loader`` / ``OnlineLabeler.loader`` /
                       ``PrototypeLabeler.loader`` / ``mix.MixedLoader``, before or after ``boundary.ErodedLoader``).
    ``RegionStats``    components, pixels, mean area and a log2 area histogram per class, accumulated on the device; ``evaluate``
                       takes them of the predictions and of the truth and gives the fragmentation ratio per class.

Removed regions are voided, not filled with the surrounding label.  CPU tensors raise: there is no CPU path in this build.
Nothing is read back unless stated.
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K

HIST_BINS = 32                # hist[floor(log2(area))]: area < 2^31
STAT_COLS = 2 + HIST_BINS     # components, pixels, hist
_SAME = object()              # sieve's ignore_index default: the void value itself


# --------------------------------------------------------------------------------------------------------------- host side
def _check_connectivity(who, connectivity):
    if A.int_in(who, "connectivity", connectivity, 4, 8) % 4:
        raise ValueError(f"{who}: connectivity must be 4 or 8, got {connectivity}")
    return int(connectivity)


def min_area_table(min_area, who="min_area_table"):
    """The int32 ``[256]`` threshold table of ``sieve`` (numpy): one int for every class, or a sequence / tensor of per-class ints;
    the classes beyond its length are kept (a threshold of 0).  A negative or non-integer threshold raises."""
    if torch.is_tensor(min_area):
        min_area = min_area.detach().cpu().numpy()
    if isinstance(min_area, bool):
        raise ValueError(f"{who}: min_area must be an int or a sequence of ints, got {min_area}")
    if isinstance(min_area, (int, np.integer)):
        arr = np.full(256, int(min_area), dtype=np.int64)
    else:
        a = np.asarray(min_area)
        if a.ndim != 1 or a.shape[0] > 256 or a.dtype.kind not in "iu":
            raise ValueError(f"{who}: min_area must be an int or at most 256 per-class ints, got {a.dtype} {a.shape}")
        arr = np.zeros(256, dtype=np.int64)
        arr[: a.shape[0]] = a
    if (arr < 0).any() or (arr > np.iinfo(np.int32).max).any():
        raise ValueError(f"{who}: every min_area must lie in [0, 2^31 - 1], got {arr.min()} .. {arr.max()}")
    return arr.astype(np.int32)


def summarize(stats):
    """The measures of ``RegionStats.compute`` from its raw counters (numpy, host): ``stats`` int64 ``[C,34]`` (components, pixels,
    then ``hist[32]`` with ``hist[k]`` the components of area ``2^k .. 2^(k+1) - 1``, per class).

    ``components`` ``[C]``, ``pixels`` ``[C]``, ``mean_area`` ``[C]`` (NaN for a class without a component), ``hist`` ``[C,32]``."""
    s = np.asarray(stats).astype(np.int64).reshape(-1, STAT_COLS)
    comp, pix = s[:, 0], s[:, 1]
    mean = np.divide(pix.astype(np.float64), comp.astype(np.float64), out=np.full(comp.shape, np.nan), where=comp > 0)
    return {"components": comp.copy(), "pixels": pix.copy(), "mean_area": mean, "hist": s[:, 2:].copy(), "stats": s}


def fragmentation(pred, truth):
    """``components_pred / components_truth`` per class from two ``summarize`` dicts; NaN where the truth has no component."""
    p = np.asarray(pred["components"], dtype=np.float64)
    t = np.asarray(truth["components"], dtype=np.float64)
    return np.divide(p, t, out=np.full(t.shape, np.nan), where=t > 0)


# ------------------------------------------------------------------------------------------------------------- device side
def label(labels, connectivity=4, ignore_index=None, return_area=False):
    """int32 ids in the labels' shape (-1 on void pixels); with ``return_area`` the pair ``(ids, area)``, both int32."""
    conn = _check_connectivity("label", connectivity)
    ign = A.int_in("label", "ignore_index", ignore_index, 0, 255, True)
    lab, single = A.label_maps("label", labels)
    ids = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    area = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)     # the labelling's own scratch when no area is asked for
    A.on_device(lab.device, K.regions_label, lab, conn, ign, ids, area)
    if single:
        ids, area = ids[0], area[0]
    return (ids, area) if return_area else ids


def label_ids(ids_i32, connectivity=4, return_area=False):
    """``label`` of an int32 map ``[N,H,W]`` (or ``[H,W]``) of more than 256 values, such as ``superpixels.slic``'s ids: every value
    ``>= 0`` is a label of its own and a negative value is void (there is no ``ignore_index``).  int32 ids in the map's shape (-1
    on void pixels); with ``return_area`` the pair ``(ids, area)``."""
    conn = _check_connectivity("label_ids", connectivity)
    if not (torch.is_tensor(ids_i32) and ids_i32.dtype == torch.int32 and ids_i32.dim() in (2, 3) and ids_i32.numel() > 0):
        raise ValueError(f"label_ids: ids must be a non-empty int32 [N,H,W] (or [H,W]) tensor, got "
                         f"{getattr(ids_i32, 'dtype', type(ids_i32).__name__)} {tuple(getattr(ids_i32, 'shape', ()))}")
    A.same_gpu("label_ids", ids=ids_i32)
    single = ids_i32.dim() == 2
    lab = (ids_i32[None] if single else ids_i32).contiguous()
    ids = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    area = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)     # the labelling's own scratch when no area is asked for
    A.on_device(lab.device, K.regions_label_i32, lab, conn, ids, area)
    if single:
        ids, area = ids[0], area[0]
    return (ids, area) if return_area else ids


def _device_table(who, min_area, dev):
    arr = min_area_table(min_area, who)
    return A.const_table("regions", arr.tobytes(), arr.copy, dev)      # callers sieve every batch with the same few tables


def sieve(labels, min_area, connectivity=4, void=255, ignore_index=_SAME, counts=None, out=None):
    """The uint8 mask with ``void`` on every component of fewer than ``min_area`` pixels, the labels elsewhere.  ``min_area``: one
    int, or per-class ints (classes beyond its length are kept).  ``ignore_index``: by default ``void`` itself, so that a void
    region is no component and is never counted; ``None`` makes every value an ordinary label.  ``counts``: an int64 ``[N,3]``
    device tensor that ACCUMULATES, per image, the pixels this call voided, the components it removed and those it kept."""
    conn = _check_connectivity("sieve", connectivity)
    v = A.int_in("sieve", "void", void, 0, 255)
    ign = v if ignore_index is _SAME else A.int_in("sieve", "ignore_index", ignore_index, 0, 255, True)
    lab, single = A.label_maps("sieve", labels)
    tab = _device_table("sieve", min_area, lab.device)
    A.counts_tensor("sieve", "counts", counts, (lab.shape[0], 3), lab.device)
    out = A.out_tensor("sieve", "out", out, lab.shape, torch.uint8, lab.device)
    ids = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    area = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    A.on_device(lab.device, K.regions_label, lab, conn, ign, ids, area)
    A.on_device(lab.device, K.regions_sieve, lab, ids, area, ign, tab, v, out, counts)
    return out[0] if single and out.dim() == 3 else out


class SievedLoader:
    """Wraps a loader of ``(frames_u8, masks_u8)`` batches -- ``PseudoLabeler.loader``, ``OnlineLabeler.loader``,
    ``PrototypeLabeler.loader``, ``mix.MixedLoader``, or ``boundary.ErodedLoader`` over one of them -- and yields ``(frames,
    sieve(masks, min_area, connectivity, void))``: the teacher's labels without their small islands.  The frames pass through;
    masks still on the host are moved.  ``last_counts``: the int64 ``[N,3]`` device tensor of the latest batch (pixels voided,
    components removed, components kept), for logging; nothing is read back here."""

    def __init__(self, loader, min_area, connectivity=4, void=255):
        self.loader = loader
        self.min_area = min_area_table(min_area, "SievedLoader")
        self.connectivity = _check_connectivity("SievedLoader", connectivity)
        self.void = A.int_in("SievedLoader", "void", void, 0, 255)
        self.last_counts = None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch) or len(batch) != 2:
                raise ValueError("SievedLoader: a batch must be a (frames, masks) pair")
            frames, masks = batch
            if torch.is_tensor(masks) and masks.device.type != "cuda":
                masks = masks.to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
            n = 1 if masks.dim() == 2 else int(masks.shape[0])
            counts = torch.zeros((n, 3), dtype=torch.int64, device=masks.device)
            out = sieve(masks, self.min_area, self.connectivity, self.void, counts=counts)
            self.last_counts = counts
            yield frames, out


class RegionStats(A.DeviceState):
    """Accumulates the per-class region counters of label maps on the device (``udaseg_regions_stats``).  ``update`` enqueues and
    does not synchronise; ``compute`` does ONE read-back and returns ``summarize`` of the counters."""

    def __init__(self, num_classes, connectivity=4, ignore_index=None, device=None):
        self.num_classes = A.int_in("RegionStats", "num_classes", num_classes, 1, 255)
        self.connectivity = _check_connectivity("RegionStats", connectivity)
        self.ignore_index = A.int_in("RegionStats", "ignore_index", ignore_index, 0, 255, True)
        self.device = torch.device(device) if device is not None else None
        self.table = None              # int64 [C, 34] on the device

    def _allocate(self, device):
        self.table = torch.zeros((self.num_classes, STAT_COLS), dtype=torch.int64, device=device)

    def reset(self):
        if self.table is not None:
            self.table.zero_()

    def update(self, pred):
        """``pred``: a label map (uint8 or int64 ``[N,H,W]`` or ``[H,W]``), or scores ``[N,C,H,W]`` (logits or probabilities),
        labelled by their first maximum (``udaseg_predict_finish``'s arg-max, at most 32 classes)."""
        if torch.is_tensor(pred) and pred.dim() == 4:
            buf, ldc, n, c, h, w = A.scores_nchw("RegionStats.update", pred, self.num_classes, "pred")
            lab = torch.empty((n, h, w), dtype=torch.int64, device=pred.device)
            A.on_device(pred.device, K.predict_finish, buf, None, n * h * w, c, ldc, lab)
            pred = lab
        lab, _ = A.label_maps("RegionStats.update", pred, "pred")
        tab = self._ensure(lab.device).table
        ids = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
        area = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
        A.on_device(lab.device, K.regions_label, lab, self.connectivity, self.ignore_index, ids, area)
        A.on_device(lab.device, K.regions_stats, lab, ids, area, self.num_classes, self.ignore_index, tab)
        return self

    def compute(self):
        """``summarize`` of the accumulated counters: ``components`` / ``pixels`` / ``mean_area`` [C], ``hist`` [C,32] and the raw
        ``stats`` [C,34].  ONE device->host transfer of ``34 C`` counters."""
        return summarize(self._ensure().table.cpu().numpy())


def evaluate(model, loader, num_classes, device, connectivity=4, ignore_index=None):
    """Eval-mode pass over ``loader`` (batches of ``(images, masks)``) in the shape of ``boundary.evaluate``: the region counters of
    the predictions and of the truth accumulate on the device and are read back ONCE each at the end.  Returns ``{"pred", "truth"}``
    (``RegionStats.compute()``'s dicts) and ``"ratio"``: ``components_pred / components_truth`` per class, NaN where the truth has
    none -- the fragmentation of the prediction, which IoU does not show."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model runs on the GPU (no CPU path in this build)")
    conn = _check_connectivity("evaluate", connectivity)
    sp = RegionStats(num_classes, conn, ignore_index, device)
    st = RegionStats(num_classes, conn, ignore_index, device)
    seen = False
    with A.eval_mode(model), torch.no_grad():
        for images, masks in loader:
            images = images.to(device)
            masks = masks.to(device)
            if masks.dtype not in (torch.uint8, torch.int64):
                masks = masks.long()
            if masks.dim() == 4 and masks.shape[1] == 1:
                masks = masks[:, 0]
            sp.update(model(images))
            st.update(masks)
            seen = True
    if not seen:
        raise ValueError("evaluate: the loader is empty")
    pred, truth = sp.compute(), st.compute()
    return {"pred": pred, "truth": truth, "ratio": fragmentation(pred, truth)}
