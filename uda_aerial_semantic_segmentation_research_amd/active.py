"""Active label acquisition on the device: which pixels (or rectangles) of which target frames to label with the hour available.

Every adaptation recipe here assumes a target domain without labels.  When a few can be had, RIPU (Xie et al., CVPR 2022, "Towards
Fewer Annotations: Active Learning via Region Impurity and Prediction Uncertainty") ranks the pixels: the class IMPURITY of the
predicted labels in a small window, times the mean prediction ENTROPY of that window.  The highest scores are requested under a
budget, pixels already requested are excluded, and training runs on the sparse masks with void elsewhere
(``CrossEntropyLoss(ignore_index=255)``).

One primitive serves all of it (``csrc/window.hip``; ``include/udaseg.h`` states every rule in full and ``tests/_active_ref.py`` is
its numpy mirror): the per-class count ``n_c(p)`` of the labels in the ``(2 radius + 1)^2`` window around every pixel, clipped at
the frame, void pixels and labels ``>= num_classes`` left out.

    ``mode_filter``   the label map smoothed by its neighbours' vote (ties: the centre's own label, else the smallest class);
                      with ``fill_void`` void holes take the vote of their surroundings.
    ``agreement``     the share of the window that carries the vote's label, fp32 in ``[0, 1]``: the local agreement of a teacher's
                      labels, usable as ``pixel_weight`` of ``SoftCrossEntropyLoss`` / ``PrototypeContrastLoss``.
    ``impurity``      the entropy of the window's label histogram over ``log(num_classes)``.
    ``acquisition``   scores ``[N,C,H,W]`` -> (score, key, labels): one pass over the scores (winner and entropy), one window pass.
    ``select``        the ``budget`` best pixels or grid cells per image by the exact radix select ``kernels.kth_smallest``; every
                      tie of the last key is kept (the rule OHEM documents) and ``counts`` reports what was taken.
    ``ActivePool``    the bookkeeping of several rounds: requested maps, sparse masks, coverage, checkpoints.

Where this differs from RIPU's code: both factors are normalised to ``[0, 1]``; the region mode uses a FIXED grid of cells in place
of greedy non-overlapping squares; ties are kept.  NOBODY HAS TUNED ``radius``, ``kind`` OR ``budget`` ON THIS DATA: the defaults
are the paper's pixel mode (a 3 x 3 window).

CPU tensors raise: there is no CPU path in this build (``ActivePool``'s bookkeeping apart from ``query`` is plain torch and runs
anywhere).  Nothing is read back unless stated.
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K

MAX_RADIUS = 16
MAX_CLASSES = 32
KINDS = {"ripu": 0, "impurity": 1, "uncertainty": 2}


# --------------------------------------------------------------------------------------------------------------- host side
def _check_radius(who, radius):
    return A.int_in(who, "radius", radius, 0, MAX_RADIUS)


def _check_classes(who, num_classes):
    return A.int_in(who, "num_classes", num_classes, 2, MAX_CLASSES)


def _check_ignore(who, ignore_index, classes):
    return A.int_in(who, "ignore_index", ignore_index, classes, 255, True)           # a class cannot be void


def _check_kind(who, kind):
    return KINDS[A.choice(who, "kind", kind, sorted(KINDS))]


def _check_cell(who, cell):
    if cell is None:
        return None
    c = cell if isinstance(cell, (tuple, list)) else (cell, cell)
    if len(c) != 2:
        raise ValueError(f"{who}: cell must be None, a positive int or a pair of them, got {cell!r}")
    return A.int_in(who, "cell", c[0], 1), A.int_in(who, "cell", c[1], 1)


def _check_budget(who, budget):
    """An int (items per image, >= 1) or a float in (0, 1) (a share of them)."""
    if isinstance(budget, (float, np.floating)):
        if not 0.0 < budget < 1.0:
            raise ValueError(f"{who}: a float budget must lie in (0, 1), got {budget}")
        return float(budget)
    return A.int_in(who, "budget", budget, 1)


def items_of(budget, items):
    """The number of items per image a budget asks for among ``items`` of them: an int as it is, a fraction as
    ``max(1, floor(budget * items))``."""
    return budget if isinstance(budget, int) else max(1, int(np.floor(budget * items)))


def table_of(radius):
    """The fp32 ``[(2 radius + 1)^2 + 1]`` table of ``m log m`` (numpy), ``m = 0 .. (2 radius + 1)^2``: evaluated in float64 and
    rounded to fp32 once, as ``boundary.table_of`` does; ``0 log 0 = 0``."""
    r = _check_radius("table_of", radius)
    m = np.arange((2 * r + 1) ** 2 + 1, dtype=np.float64)
    return (m * np.log(np.maximum(m, 1.0))).astype(np.float32)


def _device_table(r, dev):
    """The table of a radius on a device, kept (``_args.const_table``): at most 17 radii per GPU, 4.4 KB each at the most."""
    return A.const_table("active", r, lambda: table_of(r), dev)


# ------------------------------------------------------------------------------------------------------------- device side
def mode_filter(masks_u8, radius, num_classes, ignore_index=255, fill_void=False, counts=None, return_agreement=False, void=None,
                out=None):
    """The uint8 label map of the window's vote, in the masks' shape (``[N,H,W]`` or ``[H,W]``; uint8 or int64 in).  A void pixel
    (``ignore_index``, or a label ``>= num_classes``) comes out as ``void`` (default: ``ignore_index``, 255 without one) unless
    ``fill_void`` and its window holds a label.  ``counts``: an int64 ``[N,3]`` device tensor that ACCUMULATES, per image, the
    pixels whose label changed, the void pixels filled and the void pixels left.  ``return_agreement``: also the fp32 agreement."""
    r = _check_radius("mode_filter", radius)
    c = _check_classes("mode_filter", num_classes)
    ign = _check_ignore("mode_filter", ignore_index, c)
    v = A.int_in("mode_filter", "void", (255 if ign is None else ign) if void is None else void, 0, 255)
    lab, single = A.label_maps("mode_filter", masks_u8, "masks")
    A.counts_tensor("mode_filter", "counts", counts, (lab.shape[0], 3), lab.device)
    out = A.out_tensor("mode_filter", "out", out, lab.shape, torch.uint8, lab.device)
    agr = torch.empty(lab.shape, dtype=torch.float32, device=lab.device) if return_agreement else None
    A.on_device(lab.device, K.window_mode, lab, r, c, ign, fill_void, v, out, agr, counts)
    res = out[0] if single and out.dim() == 3 else out
    if return_agreement:
        return res, (agr[0] if single else agr)
    return res


def agreement(masks_u8, radius, num_classes, ignore_index=255):
    """fp32 in the masks' shape: the share of every pixel's window that carries the window's vote, 0 where the window is empty."""
    return mode_filter(masks_u8, radius, num_classes, ignore_index, return_agreement=True)[1]


def impurity(masks_u8, radius, num_classes, ignore_index=255, out=None):
    """fp32 in the masks' shape: the entropy of the window's label histogram over ``log(num_classes)``, in ``[0, 1]``."""
    r = _check_radius("impurity", radius)
    c = _check_classes("impurity", num_classes)
    ign = _check_ignore("impurity", ignore_index, c)
    lab, single = A.label_maps("impurity", masks_u8, "masks")
    out = A.out_tensor("impurity", "out", out, lab.shape, torch.float32, lab.device)
    A.on_device(lab.device, K.window_impurity, lab, r, c, ign, _device_table(r, lab.device), out)
    return out[0] if single and out.dim() == 3 else out


def _check_scores(who, scores):
    n, c, h, w = A.scores_shape(who, scores, max_classes=MAX_CLASSES)
    _check_classes(who, c)
    if n > 65535:
        raise ValueError(f"{who}: scores must have N <= 65535, got {(n, c, h, w)}")
    return n, c, h, w


def prepare(scores, probs=False, counters=None):
    """``(labels uint8 [N,H,W], entropy fp32 [N,H,W])`` of ``[N,C,H,W]`` scores in ONE pass: the first maximal class and the
    normalised entropy; a row with a non-finite score gets label 255 and entropy 0.  ``counters``: an int64 ``[2]`` device tensor
    that ACCUMULATES the finite and the non-finite rows."""
    n, c, h, w = _check_scores("prepare", scores)
    A.counts_tensor("prepare", "counters", counters, (2,), scores.device)
    dev = A.same_gpu("prepare", scores=scores)
    if counters is None:
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    entropy = torch.empty((n, h, w), dtype=torch.float32, device=dev)

    def run():
        buf, ldc = A.padded_nhwc(scores.detach())
        K.acquire_prepare(buf, ldc, c, probs, n * h * w, labels, entropy, counters)
    A.on_device(dev, run)
    return labels, entropy


def score_maps(labels_u8, entropy, num_classes, radius=1, kind="ripu", exclude=None):
    """``(score, key)`` fp32 ``[N,H,W]`` of uint8 labels (255 and every label ``>= num_classes``: void) and their entropy map."""
    r = _check_radius("score_maps", radius)
    c = _check_classes("score_maps", num_classes)
    k = _check_kind("score_maps", kind)
    if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3:
        raise ValueError("score_maps: labels must be a uint8 [N,H,W] tensor")
    shape, dev = tuple(labels_u8.shape), labels_u8.device
    if not torch.is_tensor(entropy) or entropy.dtype != torch.float32 or tuple(entropy.shape) != shape:
        raise ValueError(f"score_maps: entropy must be a float32 {list(shape)} tensor")
    if exclude is not None and (not torch.is_tensor(exclude) or exclude.dtype != torch.uint8 or tuple(exclude.shape) != shape):
        raise ValueError(f"score_maps: exclude must be None or a uint8 {list(shape)} tensor")
    A.same_gpu("score_maps", labels=labels_u8, entropy=entropy, exclude=exclude)
    score = torch.empty(shape, dtype=torch.float32, device=dev)
    key = torch.empty(shape, dtype=torch.float32, device=dev)
    A.on_device(dev, K.acquire_score, labels_u8.contiguous(), entropy.contiguous(), None if exclude is None else exclude.contiguous(), r, c,
        k, _device_table(r, dev), score, key)
    return score, key


def acquisition(scores, radius=1, kind="ripu", probs=False, exclude=None):
    """``(score, key, labels)`` of ``[N,C,H,W]`` scores (logits, or probabilities with ``probs``), read in place where they are a
    ``Unet``'s output.  ``score`` fp32 ``[N,H,W]`` is RIPU's ``impurity * uncertainty`` (``kind="impurity"`` / ``"uncertainty"``:
    one factor alone), 0 where the pixel is no candidate; ``key = 1 - score`` for a candidate and -1 otherwise, the form ``select``
    takes; ``labels`` uint8 are the winners (255: a non-finite row).  ``exclude``: uint8 ``[N,H,W]``, non-zero where a pixel was
    requested already.  Two launches."""
    r = _check_radius("acquisition", radius)
    _check_kind("acquisition", kind)
    n, c, h, w = _check_scores("acquisition", scores)
    if exclude is not None and (not torch.is_tensor(exclude) or exclude.dtype != torch.uint8 or tuple(exclude.shape) != (n, h, w)):
        raise ValueError(f"acquisition: exclude must be None or a uint8 [{n},{h},{w}] tensor")
    labels, entropy = prepare(scores, probs)
    score, key = score_maps(labels, entropy, c, r, kind, exclude)
    return score, key, labels


def select(key, budget, cell=None, into=None):
    """``(mask uint8 [N,H,W], counts int64 [N,2])``: the ``budget`` candidates of every image with the smallest keys (the largest
    scores).  ``budget``: an int (items per image) or a float in ``(0, 1)`` (that share of the image's pixels, or of its cells with
    ``cell``).  The threshold of an image is ``kth_smallest(key[i], k)`` and stays on the device; EVERY TIE of the last key is
    kept, so more than ``k`` items may be taken -- ``counts[i] = {items newly selected, candidates}`` says how many.  A budget above
    the number of candidates selects exactly the candidates.  ``cell``: an int or ``(ch, cw)``: select whole cells of that fixed
    grid by their mean score (edge cells are smaller) and mark their rectangles, void pixels included; ``counts`` then counts
    cells.  ``into``: an existing uint8 ``[N,H,W]`` mask that is OR-ed into and returned; items set in it already are not counted
    as new."""
    b = _check_budget("select", budget)
    cells = _check_cell("select", cell)
    if not torch.is_tensor(key) or key.dtype != torch.float32 or key.dim() != 3 or key.numel() == 0:
        raise ValueError("select: key must be a non-empty float32 [N,H,W] tensor")
    n, h, w = (int(v) for v in key.shape)
    dev = key.device
    if into is not None:
        A.out_tensor("select", "into", into, (n, h, w), torch.uint8, dev, contiguous=True)
    A.same_gpu("select", key=key)
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device=dev) if into is None else into
    counts = torch.zeros((n, 2), dtype=torch.int64, device=dev)

    def run():
        k_map = key.contiguous()
        if cells is not None:
            ch, cw = cells
            gh, gw = -(-h // ch), -(-w // cw)
            cell_key = torch.empty((n, gh, gw), dtype=torch.float32, device=dev)
            K.acquire_cells(k_map, ch, cw, cell_key)
            k_map = cell_key
        k = items_of(b, k_map[0].numel())
        thr = torch.stack([K.kth_smallest(k_map[i], k) for i in range(n)])
        if cells is None:
            K.acquire_select(k_map, thr, mask, counts)
        else:
            cell_mask = torch.zeros(k_map.shape, dtype=torch.uint8, device=dev)
            K.acquire_select(k_map, thr, cell_mask, counts)
            K.acquire_expand(cell_mask, cells[0], cells[1], mask)
    A.on_device(dev, run)
    return mask, counts


# ------------------------------------------------------------------------------------------------------------ bookkeeping
class ActivePool:
    """The requested-pixel maps of a labelling campaign, one uint8 ``[H,W]`` map per frame index, on the device of the first query.

    ``query`` asks a model which pixels of some frames to label next (never one it asked for before); an annotator labels them;
    ``sparse_masks`` / ``loader`` hand the training code masks that carry the truth where it was requested and ``void`` elsewhere.
    Everything but ``query`` is plain torch ops and runs on CPU tensors too."""

    def __init__(self, num_classes, radius=1, kind="ripu", budget=0.01, cell=None, void=255):
        self.num_classes = _check_classes("ActivePool", num_classes)
        self.radius = _check_radius("ActivePool", radius)
        _check_kind("ActivePool", kind)
        self.kind = kind
        self.budget = _check_budget("ActivePool", budget)
        self.cell = _check_cell("ActivePool", cell)
        self.void = A.int_in("ActivePool", "void", void, self.num_classes, 255)
        self.requested = {}            # frame index -> uint8 [H,W], non-zero where a label was requested
        self.rounds = 0
        self.last_counts = None        # int64 [N,2] device tensor of the latest query: newly selected, candidates

    @staticmethod
    def _indices(indices):
        idx = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        if len(set(idx)) != len(idx):
            raise ValueError(f"ActivePool: frame indices must be distinct within a batch, got {idx}")
        return idx

    def requested_maps(self, indices, shape, device):
        """uint8 ``[N,H,W]`` on ``device``: the requested maps of these frames, zeros for a frame never queried."""
        idx = self._indices(indices)
        out = torch.zeros((len(idx),) + tuple(shape), dtype=torch.uint8, device=device)
        for j, i in enumerate(idx):
            m = self.requested.get(i)
            if m is not None:
                if tuple(m.shape) != tuple(shape):
                    raise ValueError(f"ActivePool: frame {i} was requested at {tuple(m.shape)}, not {tuple(shape)}")
                out[j] = m.to(device)
        return out

    @torch.no_grad()
    def query(self, model_or_teacher, indices, frames_u8, probs=False):
        """One eval-mode, no-grad forward of the model (or of a ``MeanTeacher``'s model) on uint8 ``[N,H,W,3]`` frames,
        ``acquisition`` with the pool's requested maps of these frame indices as ``exclude``, ``select`` into them.  Returns the NEW
        request masks, uint8 ``[N,H,W]`` (disjoint from everything requested before); a frame that is requested in full selects
        nothing.  The model's training flag is restored; ``last_counts`` holds ``select``'s counts."""
        from .data import prepare_batch
        model = getattr(model_or_teacher, "model", model_or_teacher)
        idx = self._indices(indices)
        if A.frames_u8("ActivePool.query", frames_u8)[0] != len(idx):
            raise ValueError(f"ActivePool.query: {len(idx)} indices for {frames_u8.shape[0]} frames")
        A.same_gpu("ActivePool.query", frames=frames_u8)
        with A.eval_mode(model):
            images, _ = prepare_batch(frames_u8, None, None, getattr(model, "compute_dtype", torch.float32))
            out = model(images)
        n, c, h, w = out.shape
        if c != self.num_classes:
            raise ValueError(f"ActivePool.query: the model gives {c} classes, the pool was made for {self.num_classes}")
        before = self.requested_maps(idx, (h, w), out.device)
        _, key, _ = acquisition(out, self.radius, self.kind, probs, exclude=before)
        after = before.clone()
        _, self.last_counts = select(key, self.budget, self.cell, into=after)
        for j, i in enumerate(idx):
            self.requested[i] = after[j]
        self.rounds += 1
        return after & (before == 0).to(torch.uint8)

    def sparse_masks(self, indices, truth_masks):
        """``truth`` where requested, ``void`` elsewhere: uint8 ``[N,H,W]`` on the truth's device."""
        if not torch.is_tensor(truth_masks) or truth_masks.dim() != 3:
            raise ValueError("ActivePool.sparse_masks: truth must be a [N,H,W] tensor")
        req = self.requested_maps(indices, truth_masks.shape[1:], truth_masks.device)
        if req.shape[0] != truth_masks.shape[0]:
            raise ValueError(f"ActivePool.sparse_masks: {req.shape[0]} indices for {truth_masks.shape[0]} masks")
        return torch.where(req != 0, truth_masks.to(torch.uint8), torch.full_like(req, self.void))

    def loader(self, labelled_u8_loader):
        """Wraps a loader of ``(indices, frames_u8, truth_masks)`` batches and yields ``(frames_u8, sparse masks)``, the batches
        ``DeviceAugmentedLoader`` and ``mix.MixedLoader`` take; train with ``CrossEntropyLoss(ignore_index=void)``."""
        return _SparseLoader(self, labelled_u8_loader)

    def coverage(self):
        """``{"per_frame": {index: requested pixels}, "total": their sum, "pixels": the pixels of the frames seen}`` (one host read
        per frame)."""
        per = {i: int((m != 0).sum()) for i, m in sorted(self.requested.items())}
        return {"per_frame": per, "total": sum(per.values()), "pixels": sum(int(m.numel()) for m in self.requested.values())}

    def state_dict(self):
        return {"requested": {i: m.detach().to("cpu", torch.uint8).clone() for i, m in self.requested.items()}, "rounds": self.rounds,
                "num_classes": self.num_classes, "radius": self.radius, "kind": self.kind, "budget": self.budget, "cell": self.cell,
                "void": self.void}

    def load_state_dict(self, state, device=None):
        """A resumed campaign keeps what it asked for.  ``device``: where the maps go (default: where they were saved from, the CPU)."""
        if int(state["num_classes"]) != self.num_classes:
            raise ValueError(f"ActivePool: the state is of {state['num_classes']} classes, the pool of {self.num_classes}")
        req = {}
        for i, m in state["requested"].items():
            if not torch.is_tensor(m) or m.dtype != torch.uint8 or m.dim() != 2:
                raise ValueError(f"ActivePool: the requested map of frame {i} must be a uint8 [H,W] tensor")
            req[int(i)] = m.clone() if device is None else m.to(device)
        self.requested = req
        self.rounds = int(state["rounds"])


class _SparseLoader:
    def __init__(self, pool, loader):
        self.pool, self.loader = pool, loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch) or len(batch) != 3:
                raise ValueError("ActivePool.loader: a batch must be an (indices, frames, truth masks) triple")
            indices, frames, truth = batch
            yield frames, self.pool.sparse_masks(indices, truth)


__all__ = ["mode_filter", "agreement", "impurity", "prepare", "score_maps", "acquisition", "select", "ActivePool", "table_of",
           "items_of", "KINDS", "MAX_RADIUS", "MAX_CLASSES"]
