"""Superpixels on the device: image-adapted regions for the label maps and score maps of the other feature modules.

``boundary.erode``, ``regions.sieve``, ``active.mode_filter`` and ``crf.refine`` all treat a prediction on the pixel lattice; this
module groups the pixels by what the FRAME shows.  One primitive (``csrc/superpixels.hip``; ``include/udaseg.h`` states every rule
in full and ``tests/_superpixels_ref.py`` is its numpy mirror, compared for equality): an integer SLIC -- a ``ceil(H/step) x
ceil(W/step)`` grid of clusters, every pixel assigned to the nearest of the up to 9 clusters around its cell in colour and
position, the centres re-averaged, ``iterations`` times -- followed by a connect step after which EVERY SUPERPIXEL IS ONE
4-CONNECTED PIECE.  All of it is integer arithmetic: two calls give the same bits, and nothing is read back to the host.

    ``slic``           frames -> ``Segments(ids, grid, step, centres)``.
    ``vote`` / ``snap``  the majority class of a label map per superpixel.  On pseudo-labels (``snap(seg, masks, C)``) it moves a
                       staircase label boundary onto the edge the frame shows, the cheap alternative to ``crf.refine``; on sparse
                       labels (``vote(seg.ids, pool.sparse_masks(...), C, min_share=1.0)``) it spreads the few requested pixels of
                       ``active.ActivePool`` over their superpixels wherever they agree.
    ``mean``           the mean of a score map per superpixel, as a ``[N,gh,gw]`` table.
    ``select``         whole superpixels by the mean of ``active.acquisition``'s key, under ``active``'s budget rule (ties kept).
    ``SnappedLoader``  ``snap`` applied to the batches of a pseudo-label loader.
    ``outline``        the superpixel borders as a uint8 map, for ``render`` overlays.

What this is not: no Lab conversion (the three channels are used as they are; the colour space is the caller's) and NO GRADIENT
PERTURBATION of the seeds (SLIC moves a seed off an edge; this rule does not).  With ``min_area=0`` every non-empty cluster keeps
its main component and every superpixel is 4-connected; with ``min_area > 0`` whole clusters may vanish (on a pure-noise frame
nearly all do).  NOBODY HAS TUNED ``step`` OR ``compactness`` ON THIS DATA: the defaults are SLIC's customary ones.

CPU tensors raise: there is no CPU path in this build.  Value errors come before place errors, as ``_args`` states.
"""
from collections import namedtuple

import torch

from . import _args as A
from . import active
from . import kernels as K

MIN_STEP, MAX_STEP = 2, 64
MAX_COMPACTNESS = 1024
MAX_ITERATIONS = 64
MAX_SIDE = 32768
MAX_CLASSES = 255

Segments = namedtuple("Segments", ["ids", "grid", "step", "centres"])
Segments.__doc__ = """``ids`` int32 ``[N,H,W]`` (the cluster index ``gy * gw + gx`` of every pixel), ``grid`` ``(gh, gw)``, ``step``,
``centres`` int32 ``[N,gh*gw,6]`` = ``(Y, X, C0, C1, C2, count)`` of the last update, ``Y .. C2`` in units of 1/16."""


# --------------------------------------------------------------------------------------------------------------- host side
def grid_of(h, w, step):
    """``(gh, gw)``: the ceil-divided grid of cells of ``step`` pixels."""
    return -(-int(h) // int(step)), -(-int(w) // int(step))


def _check_slic(who, step, compactness, iterations, min_area):
    return (A.int_in(who, "step", step, MIN_STEP, MAX_STEP), A.int_in(who, "compactness", compactness, 1, MAX_COMPACTNESS),
            A.int_in(who, "iterations", iterations, 1, MAX_ITERATIONS), A.int_in(who, "min_area", min_area, 0, 2 ** 31 - 1))


def _check_frames(who, frames):
    """uint8 ``[N,H,W,3]`` or ``[H,W,3]`` within the shape limits -> (``[N,H,W,3]`` view, single)."""
    single = torch.is_tensor(frames) and frames.dim() == 3
    f4 = frames[None] if single else frames
    n, h, w = A.frames_u8(who, f4)
    if n > 65535 or max(h, w) > MAX_SIDE or h * w >= 2 ** 31:
        raise ValueError(f"{who}: frames must have N <= 65535, H, W <= {MAX_SIDE} and H * W < 2^31, got {tuple(frames.shape)}")
    return f4, single


def _check_ids(who, ids, name="ids"):
    """int32 ``[N,H,W]`` (or ``[H,W]``), non-empty -> (``[N,H,W]`` view, single).  The value alone."""
    if not (torch.is_tensor(ids) and ids.dtype == torch.int32 and ids.dim() in (2, 3) and ids.numel() > 0):
        raise ValueError(f"{who}: {name} must be a non-empty int32 [N,H,W] (or [H,W]) tensor, got "
                         f"{getattr(ids, 'dtype', type(ids).__name__)} {tuple(getattr(ids, 'shape', ()))}")
    single = ids.dim() == 2
    return (ids[None] if single else ids), single


def _ids_and_clusters(who, seg, clusters=None):
    """``seg``: a ``Segments`` or an int32 id map -> (ids ``[N,H,W]``, single, clusters).  Without a ``Segments`` and without
    ``clusters`` the table is sized for the finest grid there is, the one of ``step = 2``."""
    if isinstance(seg, Segments):
        ids, single = _check_ids(who, seg.ids)
        gh, gw = seg.grid
        return ids, single, A.int_in(who, "grid", int(gh) * int(gw), 1, 2 ** 28)
    ids, single = _check_ids(who, seg)
    if clusters is None:
        gh, gw = grid_of(ids.shape[1], ids.shape[2], MIN_STEP)
        clusters = gh * gw
    return ids, single, A.int_in(who, "clusters", clusters, 1, 2 ** 28)


# ------------------------------------------------------------------------------------------------------------- device side
def slic(frames_u8, step=16, compactness=10, iterations=10, min_area=0, counts=None):
    """``Segments`` of uint8 ``[N,H,W,3]`` (or ``[H,W,3]``) frames.  ``counts``: an int64 ``[N,4]`` device tensor that ACCUMULATES,
    per image, the components found before the connect step, the components absorbed, the pixels whose label it changed and the
    clusters that own a pixel at the end.  ``2 + 2 * iterations`` launches and the connect step's; one stream-ordered scratch
    allocation; no host read."""
    s, m, t, a = _check_slic("slic", step, compactness, iterations, min_area)
    f4, single = _check_frames("slic", frames_u8)
    n, h, w = f4.shape[:3]
    dev = A.same_gpu("slic", frames=f4)
    A.counts_tensor("slic", "counts", counts, (n, 4), dev)
    gh, gw = grid_of(h, w, s)
    ids = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    centres = torch.empty((n, gh * gw, 6), dtype=torch.int32, device=dev)
    A.on_device(dev, K.superpixel_slic, f4.contiguous(), s, m, t, a, ids, centres, counts)
    return Segments(ids[0] if single else ids, (gh, gw), s, centres[0] if single else centres)


def vote(ids, masks, num_classes, ignore_index=255, min_share=0.0, min_cover=0.0, void=None, counts=None, out=None, clusters=None):
    """The uint8 masks in which every pixel carries the majority class of its superpixel.  ``ids``: a ``Segments`` or its int32
    id map; ``masks``: uint8 or int64 ``[N,H,W]`` (or ``[H,W]``), void where the value is ``ignore_index`` or ``>= num_classes``.
    A superpixel votes if it holds a labelled pixel, its winner (ties: the smallest class) has at least ``min_share`` of the
    labelled pixels, and the labelled pixels are at least ``min_cover`` of the superpixel; otherwise its pixels come out ``void``
    (default: ``ignore_index``, 255 without one).  ``counts``: an int64 ``[N,3]`` device tensor that ACCUMULATES, per image, the
    labelled pixels whose class changed, the void pixels filled and the labelled pixels voided."""
    c = A.int_in("vote", "num_classes", num_classes, 1, MAX_CLASSES)
    ign = A.int_in("vote", "ignore_index", ignore_index, 0, 255, True)
    share = A.number("vote", "min_share", min_share, 0.0, 1.0)
    cover = A.number("vote", "min_cover", min_cover, 0.0, 1.0)
    v = A.int_in("vote", "void", (255 if ign is None else ign) if void is None else void, 0, 255)
    idm, _, k = _ids_and_clusters("vote", ids, clusters)
    if not (torch.is_tensor(masks) and masks.dtype in (torch.uint8, torch.int64) and masks.dim() in (2, 3)
            and tuple((masks[None] if masks.dim() == 2 else masks).shape) == tuple(idm.shape)):
        raise ValueError(f"vote: masks must be a uint8 or int64 tensor of the ids' shape {list(idm.shape)}, got "
                         f"{getattr(masks, 'dtype', type(masks).__name__)} {tuple(getattr(masks, 'shape', ()))}")
    lab, single = A.label_maps("vote", masks, "masks")
    dev = A.same_gpu("vote", masks=lab, ids=idm)
    A.counts_tensor("vote", "counts", counts, (lab.shape[0], 3), dev)
    out = A.out_tensor("vote", "out", out, lab.shape, torch.uint8, dev)
    A.on_device(dev, K.superpixel_vote, idm.contiguous(), lab, k, c, ign, share, cover, v, out, counts)
    return out[0] if single and out.dim() == 3 else out


snap = vote


def mean(values, seg, clusters=None):
    """fp32 ``[N,gh,gw]`` (``[N,clusters]`` for a bare id map): the mean over every superpixel of the fp32 ``values [N,H,W]`` that
    are finite and lie in ``[0, 1]``, -1 for a superpixel without one -- the form ``kernels.kth_smallest`` and
    ``kernels.acquire_select`` take.  Exact: the values are summed as integers ``rint(v * 2^24)``."""
    idm, _, k = _ids_and_clusters("mean", seg, clusters)
    if not (torch.is_tensor(values) and values.dtype == torch.float32
            and tuple((values[None] if values.dim() == 2 else values).shape) == tuple(idm.shape)):
        raise ValueError(f"mean: values must be a float32 tensor of the ids' shape {list(idm.shape)}, got "
                         f"{getattr(values, 'dtype', type(values).__name__)} {tuple(getattr(values, 'shape', ()))}")
    val = (values[None] if values.dim() == 2 else values).contiguous()
    dev = A.same_gpu("mean", values=val, ids=idm)
    n = idm.shape[0]
    out = torch.empty((n, k), dtype=torch.float32, device=dev)
    A.on_device(dev, K.superpixel_mean, val, idm.contiguous(), k, out)
    return out.view(n, *seg.grid) if isinstance(seg, Segments) else out


def select(key, seg, budget, into=None):
    """``(mask uint8 [N,H,W], counts int64 [N,2])``: the ``budget`` superpixels of every image with the smallest mean key (the
    largest mean score of ``active.acquisition``), marked in full.  ``budget``: an int (superpixels per image) or a float in
    ``(0, 1)`` (that share of the grid's clusters), ``active.select``'s rule; the threshold of an image is
    ``kth_smallest(mean[i], k)`` and EVERY TIE of the last key is kept.  ``counts[i] = {superpixels newly selected, candidate
    superpixels}``.  ``into``: an existing uint8 ``[N,H,W]`` mask that is OR-ed into and returned."""
    b = active._check_budget("select", budget)
    if not isinstance(seg, Segments):
        raise ValueError("select: seg must be the Segments of slic")
    idm, _, k = _ids_and_clusters("select", seg)
    if not torch.is_tensor(key) or key.dtype != torch.float32 or key.dim() != 3 or tuple(key.shape) != tuple(idm.shape):
        raise ValueError(f"select: key must be a float32 {list(idm.shape)} tensor")
    n, h, w = (int(v) for v in idm.shape)
    dev = key.device
    if into is not None:
        A.out_tensor("select", "into", into, (n, h, w), torch.uint8, dev, contiguous=True)
    A.same_gpu("select", key=key, ids=idm)
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device=dev) if into is None else into
    counts = torch.zeros((n, 2), dtype=torch.int64, device=dev)

    def run():
        ids = idm.contiguous()
        table = torch.empty((n, k), dtype=torch.float32, device=dev)
        K.superpixel_mean(key.contiguous(), ids, k, table)
        items = active.items_of(b, k)
        thr = torch.stack([K.kth_smallest(table[i], items) for i in range(n)])
        picked = torch.zeros((n, k), dtype=torch.uint8, device=dev)
        K.acquire_select(table, thr, picked, counts)
        K.superpixel_gather(ids, picked, k, mask)
    A.on_device(dev, run)
    return mask, counts


def outline(seg):
    """uint8 in the ids' shape, 1 where a pixel's right or lower neighbour carries another id: what ``render`` overlays take."""
    ids = _check_ids("outline", seg.ids if isinstance(seg, Segments) else seg)[0]
    A.same_gpu("outline", ids=ids)
    edge = torch.zeros(ids.shape, dtype=torch.bool, device=ids.device)
    edge[:, :, :-1] |= ids[:, :, :-1] != ids[:, :, 1:]
    edge[:, :-1, :] |= ids[:, :-1, :] != ids[:, 1:, :]
    out = edge.to(torch.uint8)
    return out[0] if (seg.ids if isinstance(seg, Segments) else seg).dim() == 2 else out


class SnappedLoader:
    """Wraps a loader of ``(frames_u8, masks_u8)`` batches -- ``PseudoLabeler.loader``, ``OnlineLabeler.loader``,
    ``PrototypeLabeler.loader``, ``mix.MixedLoader``, or ``boundary.ErodedLoader`` / ``regions.SievedLoader`` over one of them --
    and yields ``(frames, snap(slic(frames), masks))``: the teacher's labels with their boundaries on the frame's edges.  Frames
    and masks still on the host are moved.  ``last_counts``: the int64 ``[N,3]`` device tensor of the latest batch (``vote``'s
    counters), for logging; nothing is read back here."""

    def __init__(self, loader, num_classes, step=16, compactness=10, iterations=10, min_share=0.0, ignore_index=255):
        self.loader = loader
        self.num_classes = A.int_in("SnappedLoader", "num_classes", num_classes, 1, MAX_CLASSES)
        self.step, self.compactness, self.iterations, _ = _check_slic("SnappedLoader", step, compactness, iterations, 0)
        self.min_share = A.number("SnappedLoader", "min_share", min_share, 0.0, 1.0)
        self.ignore_index = A.int_in("SnappedLoader", "ignore_index", ignore_index, 0, 255, True)
        self.last_counts = None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch) or len(batch) != 2:
                raise ValueError("SnappedLoader: a batch must be a (frames, masks) pair")
            frames, masks = batch
            dev = torch.device("cuda", torch.cuda.current_device())
            if torch.is_tensor(frames) and frames.device.type != "cuda":
                frames = frames.to(dev, non_blocking=True)
            if torch.is_tensor(masks) and masks.device.type != "cuda":
                masks = masks.to(dev, non_blocking=True)
            seg = slic(frames, self.step, self.compactness, self.iterations)
            n = 1 if masks.dim() == 2 else int(masks.shape[0])
            counts = torch.zeros((n, 3), dtype=torch.int64, device=masks.device)
            out = vote(seg, masks, self.num_classes, self.ignore_index, self.min_share, counts=counts)
            self.last_counts = counts
            yield frames, out


__all__ = ["Segments", "slic", "vote", "snap", "mean", "select", "outline", "SnappedLoader", "grid_of", "MIN_STEP", "MAX_STEP",
           "MAX_COMPACTNESS", "MAX_ITERATIONS", "MAX_SIDE", "MAX_CLASSES"]
