"""Per-class ROC / PR curves, AUC and AP on the device -- the build's counterpart of the reference's
``SegmentationTrainer._log_roc_curves`` / ``_log_pr_curves`` (``src/models/train.py:275-328``), which copy
``softmax(outputs)[:, c]`` to the host class by class and let sklearn sort it.

Here ONE HIP pass over the logits (``udaseg_score_hist``) makes two ``[C, B]`` tables of 64-bit counters and a second tiny
kernel (``udaseg_curve_finish``) turns them into AUC, AP and an error bound; no sort, and at most ``2 x C x B`` counters ever
leave the device.

The score and its grid (part of the public contract)
    For a pixel with logits ``z`` the score of class ``c`` is the log-odds of its softmax probability,
    ``s_c = z_c - log(sum_{j != c} exp(z_j)) = log(p_c / (1 - p_c))``.  ROC and PR curves depend on the order of the scores
    only and ``s_c`` is strictly increasing in ``p_c``, so these are the curves of the reference's ``probs[:, c]``; unlike
    ``p_c`` in fp32 the log-odds keep their resolution near 0 and 1.  The grid is uniform in the score: ``B`` bins over
    ``[-L, L)``, ``bin = clamp(floor((s + L) * B / (2 L)), 0, B - 1)``; bin ``b``'s lower edge is ``-L + b * 2 L / B``, as a
    probability ``sigmoid(edge)``.  Scores beyond the range fall into the end bins; a NaN score (NaN or +inf logits) is
    counted in bin 0.  A pixel whose target is outside ``[0, C)`` is left out of every table.

    ``pos[c][b]``: pixels of target ``c`` whose ``s_c`` is in bin ``b``; ``neg[c][b]``: pixels of every other valid target.
    The tables ACCUMULATE across ``update`` calls, so a validation loop gets the curves of the whole set.

From the tables, per class, with ``P = sum pos``, ``N = sum neg``, bins walked from the top
    ``tp_k, fp_k`` running sums; ``tpr = tp / P``, ``fpr = fp / N``, ``precision = tp / (tp + fp)``, ``recall = tp / P``;
    ``auc`` = trapezoid over ``(fpr, tpr)`` from ``(0, 0)``; ``ap = sum_k (recall_k - recall_{k-1}) * precision_k`` over the
    non-empty bins; ``auc_slack = 0.5 * sum_b pos_b * neg_b / (P * N)``.

    ``auc`` and ``ap`` are exactly ``sklearn.metrics.roc_auc_score`` / ``average_precision_score`` OF THE QUANTISED SCORE (the bin
    index).  Against the un-quantised score ``|auc - auc_exact| <= auc_slack`` holds rigorously: quantising keeps the order of
    every pair in different bins, and a positive / negative pair sharing a bin counts 1/2 instead of 0 or 1.  AP has no such
    bound and is documented as the AP of the quantised score.  ``auc`` and ``auc_slack`` are NaN when ``P == 0`` or ``N == 0``,
    ``ap`` is NaN when ``P == 0`` (sklearn warns and returns a placeholder there; that is not imitated).
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K

SCORE_BINS = 2048
SCORE_RANGE = 16.0
SUPPORTED_BINS = (256, 512, 1024, 2048, 4096)


def bin_thresholds(bins=SCORE_BINS, score_range=SCORE_RANGE):
    """Lower edge of every bin as a probability, ``sigmoid(-L + b * 2 L / B)`` (bin 0 also holds every lower score)."""
    edges = -float(score_range) + np.arange(bins, dtype=np.float64) * (2.0 * float(score_range) / bins)
    return 1.0 / (1.0 + np.exp(-edges))


def curves_from_hist(pos, neg, score_range=SCORE_RANGE):
    """The finishing arithmetic on the host, float64 numpy (what ``udaseg_curve_finish`` does on the device, plus the curve
    arrays).  ``pos``, ``neg``: ``[C, B]`` integer tables (numpy or tensors).  Returns a dict:

    ``auc``, ``ap``, ``auc_slack`` ``[C]`` float64; ``support`` ``[C, 2]`` int64 (P, N); and per class (lists of ``C`` arrays)
    ``bins`` -- the non-empty bins from the top down (K of them) -- with ``thresholds`` (their lower edges as probabilities),
    ``tp``, ``fp`` (cumulative counts at each of them, int64), ``tpr``, ``fpr``, ``recall``, ``precision`` of length K + 1:
    they open with the point above every score, ``(fpr, tpr) = (0, 0)`` and ``(recall, precision) = (0, 1)``.
    Rates of a class without positives (or negatives) are NaN.
    """
    if torch.is_tensor(pos):
        pos = pos.detach().cpu().numpy()
    if torch.is_tensor(neg):
        neg = neg.detach().cpu().numpy()
    pos = np.asarray(pos).astype(np.int64)
    neg = np.asarray(neg).astype(np.int64)
    if pos.ndim != 2 or pos.shape != neg.shape:
        raise ValueError(f"pos and neg must be [C, B] tables of one shape, got {pos.shape} and {neg.shape}")
    C, B = pos.shape
    thr_all = bin_thresholds(B, score_range)
    out = {k: np.full(C, np.nan) for k in ("auc", "ap", "auc_slack")}
    out["support"] = np.stack([pos.sum(1), neg.sum(1)], axis=1)
    for k in ("bins", "thresholds", "tp", "fp", "tpr", "fpr", "recall", "precision"):
        out[k] = []
    nan = float("nan")
    for c in range(C):
        pb, nb = pos[c, ::-1], neg[c, ::-1]                      # from the top bin down
        tp, fp = np.cumsum(pb), np.cumsum(nb)
        P, N = int(tp[-1]), int(fp[-1])
        pf, nf, tpf, fpf = pb.astype(np.float64), nb.astype(np.float64), tp.astype(np.float64), fp.astype(np.float64)
        if P and N:
            out["auc"][c] = float(np.sum(nf * ((tpf - pf) + tpf))) / (2.0 * P * N)
            out["auc_slack"][c] = 0.5 * float(np.sum(pf * nf)) / (float(P) * float(N))
        if P:
            m = pb > 0
            out["ap"][c] = float(np.sum(pf[m] * (tpf[m] / (tpf[m] + fpf[m])))) / P
        keep = np.nonzero((pb + nb) > 0)[0]
        tk, fk = tp[keep], fp[keep]
        out["bins"].append((B - 1 - keep).astype(np.int64))
        out["thresholds"].append(thr_all[B - 1 - keep])
        out["tp"].append(tk)
        out["fp"].append(fk)
        tkf, fkf = tk.astype(np.float64), fk.astype(np.float64)
        rec = tkf / P if P else np.full(len(keep), nan)
        out["tpr"].append(np.concatenate([[0.0 if P else nan], rec]))
        out["fpr"].append(np.concatenate([[0.0 if N else nan], fkf / N if N else np.full(len(keep), nan)]))
        out["recall"].append(np.concatenate([[0.0 if P else nan], rec]))
        out["precision"].append(np.concatenate([[1.0], tkf / (tkf + fkf)]))
    return out


class ScoreHistogram(A.DeviceState):
    """Accumulates the per-class score histograms of ``[N,C,H,W]`` logits against ``[N,H,W]`` (or ``[N,1,H,W]``) masks on the
    device.  ``update`` enqueues one kernel and does not synchronise; ``compute`` enqueues the finishing kernel and returns
    device tensors; ``curves`` reads the two tables back in ONE transfer and returns ``curves_from_hist`` of them."""

    def __init__(self, num_classes, bins=SCORE_BINS, score_range=SCORE_RANGE, device=None):
        self.num_classes = A.int_in("ScoreHistogram", "num_classes", num_classes, 1, 32)
        self.bins = int(A.choice("ScoreHistogram", "bins", bins, SUPPORTED_BINS))
        self.score_range = A.number("ScoreHistogram", "score_range", score_range, 0.0, lo_open=True)
        self.device = torch.device(device) if device is not None else None
        self.tables = None              # [2, C, B] int64 on the device: pos, neg (one allocation, one transfer)

    def _allocate(self, device):
        self.tables = torch.zeros(2, self.num_classes, self.bins, dtype=torch.int64, device=device)

    @property
    def pos(self):
        return self._ensure().tables[0]

    @property
    def neg(self):
        return self._ensure().tables[1]

    def reset(self):
        if self.tables is not None:
            self.tables.zero_()

    def update(self, outputs, masks):
        who = "ScoreHistogram.update"
        n, c, h, w = A.scores_shape(who, outputs, self.num_classes, "logits")
        tgt = A.flat_targets(who, masks, n * h * w)
        dev = A.same_gpu(who, logits=outputs, masks=masks)
        t = self._ensure(dev).tables
        buf, ldc = A.padded_nhwc(outputs.detach())
        A.on_device(dev, K.score_hist, buf, tgt, n * h * w, c, ldc, self.bins, self.score_range, t[0], t[1])
        return self

    def compute(self):
        """{'auc', 'ap', 'auc_slack': [C] float64, 'support': [C, 2] int64 (P, N)} as DEVICE tensors (no host sync)."""
        t = self._ensure().tables
        C = self.num_classes
        f = torch.empty(3, C, dtype=torch.float64, device=t.device)
        support = torch.empty(C, 2, dtype=torch.int64, device=t.device)
        A.on_device(t.device, K.curve_finish, t[0], t[1], C, self.bins, f[0], f[1], f[2], support)
        return {"auc": f[0], "ap": f[1], "auc_slack": f[2], "support": support}

    def curves(self):
        """``curves_from_hist`` of the accumulated tables: ONE device->host transfer of 2 x C x B counters."""
        t = self._ensure().tables.cpu().numpy()
        return curves_from_hist(t[0], t[1], self.score_range)


def class_curves(outputs, masks, num_classes, bins=SCORE_BINS, score_range=SCORE_RANGE):
    """One-shot form: the curves (``curves_from_hist`` dict) of one batch of logits against its masks."""
    return ScoreHistogram(num_classes, bins, score_range, outputs.device).update(outputs, masks).curves()


def _nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    m = np.isfinite(v)
    return float(v[m].mean()) if m.any() else float("nan")


def evaluate(model, loader, num_classes, device, bins=SCORE_BINS, score_range=SCORE_RANGE):
    """Eval-mode pass over ``loader`` (batches of ``(images, masks)``).  The confusion matrix and the score histograms
    accumulate on the device and are read back ONCE at the end.  Returns a dict of numpy values:

    ``confusion`` [C, C] int64 (rows = target); per class ``iou``, ``f1`` (as ``metrics.SegmentationMetrics`` defines them),
    ``auc``, ``ap``, ``auc_slack``, ``support``; ``mean_iou`` (nanmean, as ``batch_iou``), ``accuracy``, ``mean_auc`` / ``mean_ap``
    (over the classes with a finite value); ``pred_distribution`` [C]: share of the pixels predicted as each class, what the
    reference's ``predict.test_model`` writes into ``prediction_stats.txt`` (``src/models/predict.py:250-257``); and ``curves``:
    the ``curves_from_hist`` dict of the accumulated tables ``pos`` / ``neg`` [C, B].  ``accuracy`` is over the pixels with a
    target in ``[0, C)``, the ones the confusion matrix holds."""
    from .metrics import confusion_matrix
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model runs on the GPU (no CPU path in this build)")
    hist = ScoreHistogram(num_classes, bins, score_range, device)
    cm = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=device)
    npred = torch.zeros(num_classes, dtype=torch.int64, device=device)
    total = 0
    with A.eval_mode(model), torch.no_grad():
        for images, masks in loader:
            images = images.to(device)
            masks = masks.to(device).long()
            outputs = model(images)
            cm += confusion_matrix(outputs, masks, num_classes)
            hist.update(outputs, masks)
            # pixels with a target outside [0, C) are not in the confusion matrix but do count in the reference's distribution
            npred += torch.bincount(outputs.argmax(dim=1).reshape(-1), minlength=num_classes)
            total += masks.numel()
    packed = torch.cat([cm.reshape(-1), npred, hist.tables.reshape(-1)]).cpu().numpy()
    k = num_classes
    cmn = packed[:k * k].reshape(k, k)
    npn = packed[k * k:k * k + k]
    tab = packed[k * k + k:].reshape(2, k, bins)
    cur = curves_from_hist(tab[0], tab[1], score_range)
    tp = np.diag(cmn).astype(np.float64)
    fp, fn = cmn.sum(axis=0) - tp, cmn.sum(axis=1) - tp
    iou = tp / (cmn.sum(axis=1) + cmn.sum(axis=0) - tp + 1e-7)
    return {"confusion": cmn, "iou": iou, "mean_iou": float(np.nanmean(iou)),
            "accuracy": float(tp.sum() / max(cmn.sum(), 1)), "f1": 2 * tp / (2 * tp + fp + fn + 1e-7),
            "auc": cur["auc"], "ap": cur["ap"], "auc_slack": cur["auc_slack"], "support": cur["support"],
            "mean_auc": _nanmean(cur["auc"]), "mean_ap": _nanmean(cur["ap"]),
            "pred_distribution": npn.astype(np.float64) / max(total, 1), "pos": tab[0], "neg": tab[1], "curves": cur}
